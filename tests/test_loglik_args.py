"""evaluation.loglik_gpu / loglik_metrics and GRU4Rec.session_log_likelihood without a GPU: the metrics on hand-made results, every
refusal that needs no device before the device model (a stand-in that records) is called, and what the stand-in's (z, zeta, Q,
eligible) become on the host (the two float64 formulas of the contract)."""
import numpy as np
import pandas as pd
import pytest

from gru4rec_amd import evaluation
from gru4rec_amd.gru4rec import GRU4Rec

BASE = 1000     # item id of item index 0


class Recorder:
    """Stand-in for the device model: loglik_events returns, for slot s, z = -s / 4, zeta = 1, Q = 2^39 * (s + 1), every third target
    ineligible."""

    def __init__(self):
        self.calls = []

    def loglik_events(self, plan, batch, items, slot, n_slots, temperature=1.0, excl_mask=None, seen=None):
        self.calls.append(dict(batch=batch, items=None if items is None else np.asarray(items).copy(), slot=np.asarray(slot).copy(),
                               n_slots=n_slots, temperature=temperature, excl_mask=excl_mask, seen=seen, T=plan['T']))
        s = np.arange(n_slots)
        return ((-s / 4.0).astype(np.float32), np.ones(n_slots, dtype=np.float32), (2 ** 39 * (s + 1)).astype(np.uint64), s % 3 != 2)


def _model(n_items=50):
    g = GRU4Rec(layers=[16])
    g.itemidmap = pd.Series(data=np.arange(n_items), index=np.arange(BASE, BASE + n_items), name='ItemIdx')
    g.n_items = n_items
    g.error_during_train = False
    g._model = Recorder()
    return g


def _table(lens, seed=0, n_items=50):
    rng = np.random.RandomState(seed)
    n = int(np.sum(lens))
    return pd.DataFrame({'SessionId': np.repeat(7 + 3 * np.arange(len(lens)), lens).astype(np.int32),
                         'ItemId': BASE + rng.randint(0, n_items, size=n), 'Time': np.arange(n, dtype=np.int64)})


# ---- loglik_metrics --------------------------------------------------------------------------------------------------------------
def test_metrics_average_the_eligible_events_only():
    res = dict(logprob=np.array([-1.0, -np.inf, -3.0, -0.5, -np.inf], dtype=np.float32), eligible=np.array([True, False, True, True, False]),
               session=np.array([4, 4, 9, 2, 2]))
    m = evaluation.loglik_metrics(res)
    assert m['n'] == 5 and m['n_ineligible'] == 2
    assert m['nll'] == pytest.approx(4.5 / 3, abs=1e-15) and m['perplexity'] == pytest.approx(np.exp(1.5), rel=1e-15)
    assert m['sessions'].tolist() == [2, 4, 9]
    assert m['session_logprob'].dtype == np.float64 and m['session_logprob'].tolist() == [-0.5, -1.0, -3.0]
    assert m['session_events'].tolist() == [1, 1, 1]
    assert sorted(m) == ['n', 'n_ineligible', 'nll', 'perplexity', 'session_events', 'session_logprob', 'sessions']


def test_metrics_sum_per_session_in_float64():
    lp = np.array([-0.1, -0.2, -0.3, -0.4], dtype=np.float32)
    m = evaluation.loglik_metrics(dict(logprob=lp, eligible=np.ones(4, dtype=bool), session=np.array([1, 1, 1, 0])))
    assert m['session_logprob'].tolist() == [float(lp[3]), float(lp[:3].astype(np.float64).sum())]
    assert m['session_events'].tolist() == [1, 3]
    assert m['nll'] == float(-lp.astype(np.float64).sum() / 4)


def test_metrics_with_no_eligible_event():
    m = evaluation.loglik_metrics(dict(logprob=np.full(3, -np.inf, dtype=np.float32), eligible=np.zeros(3, dtype=bool), session=np.array([1, 1, 2])))
    assert m['n'] == 3 and m['n_ineligible'] == 3 and np.isnan(m['nll']) and np.isnan(m['perplexity'])
    assert m['sessions'].tolist() == [1, 2] and m['session_logprob'].tolist() == [0.0, 0.0] and m['session_events'].tolist() == [0, 0]


# ---- refusals that need no device ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('temperature', [0, 0.0, -1.0, float('nan'), float('inf'), True, 1e-45, 'hot'])
def test_bad_temperatures(temperature):
    g = _model()
    with pytest.raises(ValueError, match='temperature'):
        evaluation.loglik_gpu(g, _table([3, 4]), temperature=temperature)
    with pytest.raises(ValueError, match='temperature'):
        g.session_log_likelihood([[BASE, BASE + 1]], temperature=temperature)
    assert g._model.calls == []


@pytest.mark.parametrize('batch_size', [0, -3, True, 2.5])
def test_bad_batch_sizes(batch_size):
    g = _model()
    with pytest.raises(ValueError, match='batch_size'):
        evaluation.loglik_gpu(g, _table([3, 4]), batch_size=batch_size)
    assert g._model.calls == []


def test_fewer_sessions_than_an_explicit_batch_size():
    g = _model()
    with pytest.raises(IndexError):
        evaluation.loglik_gpu(g, _table([3, 4]), batch_size=3)
    assert g._model.calls == []


def test_histories():
    g = _model()
    with pytest.raises(ValueError, match='history 1 is empty'):
        g.session_log_likelihood([[BASE], []])
    with pytest.raises(ValueError, match='histories is empty'):
        g.session_log_likelihood([])
    with pytest.raises(ValueError, match='no scored event'):
        g.session_log_likelihood([[BASE], [BASE + 3], np.array([BASE + 1])])
    with pytest.raises(KeyError):
        g.session_log_likelihood([[BASE, BASE - 1]])
    with pytest.raises(KeyError):
        g.session_log_likelihood([[BASE, BASE + 1]], predict_for_item_ids=[BASE - 1])
    with pytest.raises(KeyError):
        evaluation.loglik_gpu(g, _table([3, 4]), exclude=[BASE - 1])
    assert g._model.calls == []


def test_error_during_train():
    g = _model()
    assert callable(evaluation.loglik_gpu) and callable(g.session_log_likelihood)
    g.error_during_train = True
    # the flag is answered with a bare Exception (the reference's `raise Exception`), in front of every other check
    with pytest.raises(Exception) as e:
        evaluation.loglik_gpu(g, _table([3, 4]), temperature=0)
    assert type(e.value) is Exception
    with pytest.raises(Exception) as e:
        g.session_log_likelihood([[BASE], []], temperature=0)
    assert type(e.value) is Exception
    assert g._model.calls == []
    g.error_during_train = False
    evaluation.loglik_gpu(g, _table([3, 4]))
    g.session_log_likelihood([[BASE, BASE + 1]])
    assert len(g._model.calls) == 2


# ---- the host side of a call -----------------------------------------------------------------------------------------------------
def test_the_formulas_and_the_table_columns():
    g = _model()
    lens = [3, 2, 5]
    data = _table(lens, seed=1)
    g.predict = 'stale'
    res = evaluation.loglik_gpu(g, data.iloc[::-1].reset_index(drop=True), temperature=0.5, items=BASE + np.arange(40), exclude=[BASE + 2],
                                exclude_seen=True)
    assert g.predict is None
    c = g._model.calls[-1]
    assert c['batch'] == 3 and c['n_slots'] == 7 and c['temperature'] == 0.5 and c['items'].tolist() == list(range(40))
    assert c['slot'].shape == (c['T'], 3) and sorted(c['slot'][c['slot'] >= 0].tolist()) == list(range(7))
    assert c['excl_mask'][0] == 4 and set(c['seen']) >= {'offs', 'items', 'first', 'sess', 'pos'}
    assert res['row'].tolist() == [0, 1, 3, 5, 6, 7, 8]
    assert res['session'].tolist() == [7, 7, 10, 13, 13, 13, 13]
    assert res['target'].tolist() == data.ItemId.values[[1, 2, 4, 6, 7, 8, 9]].tolist()
    s = np.arange(7)
    z = (-s / 4.0).astype(np.float32)
    logq = np.log(np.float64(s + 1))                     # log(Q * 2^-39)
    assert res['lse'].dtype == np.float32 and res['lse'].tolist() == (2.0 + logq).astype(np.float32).tolist()
    d = ((z - np.float32(1)) * np.float32(2)).astype(np.float32)
    want = np.where(s % 3 != 2, (d.astype(np.float64) - logq).astype(np.float32), -np.inf)
    assert res['logprob'].dtype == np.float32 and res['logprob'].tolist() == want.tolist()
    assert res['target_logit'].tolist() == z.tolist() and res['eligible'].tolist() == (s % 3 != 2).tolist()
    assert res['Q'].dtype == np.uint64


def test_the_list_form_skips_one_item_histories():
    g = _model()
    hists = [[BASE + 1, BASE + 2, BASE + 1], [BASE + 5], np.array([BASE + 7, BASE + 8])]
    lp, offs = g.session_log_likelihood(hists)
    assert offs.dtype == np.int64 and offs.tolist() == [0, 2, 2, 3] and lp.shape == (3,) and lp.dtype == np.float32
    c = g._model.calls[-1]
    assert c['batch'] == 2 and c['n_slots'] == 3 and c['items'] is None and c['seen'] is None and c['excl_mask'] is None
    det = g.session_log_likelihood(hists, return_details=True)[2]
    assert det['session'].tolist() == [0, 0, 2] and det['target'].tolist() == [BASE + 2, BASE + 1, BASE + 8]

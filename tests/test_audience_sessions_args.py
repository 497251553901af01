"""GRU4Rec.audience_sessions without a GPU: every refusal that needs no device happens before the device model (a stand-in that
records) is called, and what the stand-in returns becomes the documented triple."""
import numpy as np
import pandas as pd
import pytest

from gru4rec_amd import _native
from gru4rec_amd.gru4rec import GRU4Rec

BASE = 1000     # item id of item index 0


class Recorder:
    """Stand-in for the device model: audience_sessions returns, for item position j, the sessions j, j + 1, ... (mod n) with the
    values -i / 4, min(k, n - j) of them, and the padding of the C entry behind them."""

    def __init__(self):
        self.calls = []

    def audience_sessions(self, hist_offs, hist_items, items, k, by='logprob', temperature=1.0, exclude_history=False, hidden=None):
        self.calls.append(dict(offs=np.asarray(hist_offs).copy(), hist=np.asarray(hist_items).copy(), items=np.asarray(items).copy(), k=k, by=by,
                               temperature=temperature, exclude_history=exclude_history, hidden=hidden))
        n, M = len(hist_offs) - 1, len(items)
        sessions = np.full((M, k), -1, dtype=np.int32)
        values = np.full((M, k), np.nan, dtype=np.float32)
        counts = np.zeros(M, dtype=np.int32)
        for j in range(M):
            c = max(0, min(k, n - j))
            counts[j] = c
            sessions[j, :c] = (j + np.arange(c)) % n
            values[j, :c] = -np.arange(c) / 4.0
        return sessions, values, counts


def _model(n_items=50, final_act='linear', layers=(16,)):
    g = GRU4Rec(layers=list(layers), final_act=final_act, loss='cross-entropy' if final_act.startswith('softmax') else 'bpr-max')
    g.itemidmap = pd.Series(data=np.arange(n_items), index=np.arange(BASE, BASE + n_items), name='ItemIdx')
    g.n_items = n_items
    g.error_during_train = False
    g._model = Recorder()
    return g


HISTS = [[BASE, BASE + 1], [BASE + 2], [BASE + 3, BASE + 4, BASE + 5]]


def test_empty_histories_and_an_empty_history():
    g = _model()
    with pytest.raises(ValueError, match='empty'):
        g.audience_sessions([], [BASE], 3)
    with pytest.raises(ValueError, match='history 1 is empty'):
        g.audience_sessions([[BASE], []], [BASE], 3)
    assert g._model.calls == []


def test_unknown_item_ids():
    g = _model()
    with pytest.raises(KeyError):
        g.audience_sessions(HISTS, [BASE, BASE + 50], 3)
    with pytest.raises(KeyError):
        g.audience_sessions([[BASE, 7]], [BASE], 3)
    assert g._model.calls == []


def test_empty_item_ids_and_too_many():
    g = _model()
    with pytest.raises(ValueError, match='item_ids'):
        g.audience_sessions(HISTS, [], 3)
    with pytest.raises(ValueError, match='G4R_AUDIENCE_ITEMS_MAX'):
        g.audience_sessions(HISTS, [BASE] * (_native.G4R_AUDIENCE_ITEMS_MAX + 1), 3)
    assert g._model.calls == []


@pytest.mark.parametrize('k', [0, -1, _native.G4R_AUDIENCE_MAX + 1, 2.5, True, None, 'ten'])
def test_bad_k(k):
    g = _model()
    with pytest.raises(ValueError, match='k = '):
        g.audience_sessions(HISTS, [BASE], k)
    assert g._model.calls == []


def test_k_is_bounded_by_neither_topk_max_nor_n():
    g = _model()
    s, v, c = g.audience_sessions(HISTS, [BASE], _native.G4R_AUDIENCE_MAX)
    assert s.shape == v.shape == (1, _native.G4R_AUDIENCE_MAX) and c.tolist() == [3]
    assert g._model.calls[0]['k'] == _native.G4R_AUDIENCE_MAX > _native.G4R_TOPK_MAX


def test_the_bound_on_items_times_k():
    g = _model()
    M = 200
    k = _native.G4R_AUDIENCE_ENTRIES_MAX // M + 1
    assert k <= _native.G4R_AUDIENCE_MAX
    with pytest.raises(ValueError, match='G4R_AUDIENCE_ENTRIES_MAX'):
        g.audience_sessions(HISTS, [BASE] * M, k)
    assert g._model.calls == []
    g.audience_sessions(HISTS, [BASE] * M, k - 1)
    assert len(g._model.calls) == 1


@pytest.mark.parametrize('by', ['rank', None, 'SCORE', 0])
def test_bad_by(by):
    g = _model()
    with pytest.raises(ValueError, match='by = '):
        g.audience_sessions(HISTS, [BASE], 3, by=by)
    assert g._model.calls == []


@pytest.mark.parametrize('temperature', [0, 0.0, -1.0, float('nan'), float('inf'), True, 1e-45, 'hot'])
def test_bad_temperatures(temperature):
    g = _model()
    with pytest.raises(ValueError, match='temperature'):
        g.audience_sessions(HISTS, [BASE], 3, temperature=temperature)
    assert g._model.calls == []
    g.audience_sessions(HISTS, [BASE], 3, by='score', temperature=temperature)      # read in logprob mode only
    assert g._model.calls[0]['temperature'] == 1.0


@pytest.mark.parametrize('final_act', ['softmax', 'softmax_logit'])
def test_score_mode_is_refused_for_softmax_models(final_act):
    g = _model(final_act=final_act)
    with pytest.raises(NotImplementedError, match="by='logprob'"):
        g.audience_sessions(HISTS, [BASE], 3, by='score')
    assert g._model.calls == []
    g.audience_sessions(HISTS, [BASE], 3, by='logprob')
    assert g._model.calls[0]['by'] == 'logprob'


def test_bad_hidden():
    g = _model(layers=(16, 8))
    ok = [np.zeros((3, 16), dtype=np.float32), np.zeros((3, 8), dtype=np.float32)]
    for bad in (ok[:1], [ok[0], np.zeros((3, 8))], [ok[0], np.zeros((2, 8), dtype=np.float32)], np.zeros((3, 16), dtype=np.float32)):
        with pytest.raises(ValueError, match='hidden'):
            g.audience_sessions(HISTS, [BASE], 3, hidden=bad)
    assert g._model.calls == []
    g.audience_sessions(HISTS, [BASE], 3, hidden=ok)
    assert [h.shape for h in g._model.calls[0]['hidden']] == [(3, 16), (3, 8)]


def test_the_logprob_mode_takes_at_most_2_24_items():
    g = _model()
    g.n_items = 2 ** 24 + 1
    with pytest.raises(ValueError, match='2\\^24'):
        g.audience_sessions(HISTS, [BASE], 3)
    assert g._model.calls == []
    g.audience_sessions(HISTS, [BASE], 3, by='score')
    assert len(g._model.calls) == 1


def test_what_the_device_model_is_handed():
    g = _model()
    g.audience_sessions(HISTS, np.array([BASE + 7, BASE + 7, BASE + 1]), 4, temperature=0.7, exclude_history=1)
    c = g._model.calls[0]
    assert c['offs'].tolist() == [0, 2, 3, 6] and c['hist'].tolist() == [0, 1, 2, 3, 4, 5]
    assert c['items'].tolist() == [7, 7, 1] and c['items'].dtype == np.int32
    assert c['k'] == 4 and c['by'] == 'logprob' and c['exclude_history'] is True and c['hidden'] is None
    assert c['temperature'] == float(np.float32(0.7))


def test_the_result_is_the_documented_triple():
    g = _model()
    s, v, c = g.audience_sessions(HISTS, [BASE + 7, BASE + 7, BASE + 1], 5, by='score')
    assert s.dtype == np.int64 and v.dtype == np.float32 and c.dtype == np.int32
    assert s.shape == v.shape == (3, 5) and c.shape == (3,)
    assert c.tolist() == [3, 2, 1]
    assert s.tolist() == [[0, 1, 2, -1, -1], [1, 2, -1, -1, -1], [2, -1, -1, -1, -1]]      # indices into `histories`
    for j in range(3):
        assert v[j, :c[j]].tolist() == [-i / 4.0 for i in range(c[j])]
        assert np.isnan(v[j, c[j]:]).all() and (s[j, c[j]:] == -1).all()

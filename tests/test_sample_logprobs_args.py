"""GRU4Rec.sample_sessions(top_p=, return_logprobs=) and GRU4Rec.session_log_partition without a GPU: every refusal happens before the
device model (a recording stand-in) is called, the options reach it only when one is set (otherwise the call is the old entry's, with
the old keywords), logprobs is the last element of the returned tuple with and without return_hidden, session_log_partition forms lse
from (zeta, Q) in float64, and mutant 25 is registered."""
import numpy as np
import pytest

from gru4rec_amd import _native
from gru4rec_amd import build as g4r_build
from gru4rec_amd import gru4rec as g4r_module
from test_continue_sessions_args import assert_same_state, ids, rows_of, state
from test_sample_sessions_args import SampleRecorder, _model as _plain_model


class LogprobRecorder(SampleRecorder):
    """SampleRecorder whose sample_sessions also takes the two options (logprobs = -score) and which has session_log_partition."""

    def sample_sessions(self, *a, top_p=None, return_logprobs=False, **kw):
        out = SampleRecorder.sample_sessions(self, *a, **kw)
        self.calls[-1][1].update(top_p=top_p, return_logprobs=return_logprobs, new_entry=True)
        return out + ((-out[1],) if return_logprobs else ())

    def session_log_partition(self, hist_offs, hist_items, item_idx=None, temperature=1.0, excl_offs=None, excl_items=None, excl_mask=None,
                              hidden=None):
        cp = (lambda a: None if a is None else np.asarray(a).copy())
        self.calls.append(('lse', dict(offs=cp(hist_offs), items=cp(hist_items), item_idx=cp(item_idx), temperature=temperature,
                                       excl_offs=cp(excl_offs), excl_items=cp(excl_items), excl_mask=cp(excl_mask), hidden=hidden)))
        n = len(hist_offs) - 1
        return np.arange(1, n + 1, dtype=np.float32), (np.arange(1, n + 1) * 2 ** 39).astype(np.uint64)


def _model(n_items=300, layers=(64,), final_act='linear'):
    g = _plain_model(n_items, layers, final_act)
    g._model = LogprobRecorder(n_items, [(D + 3) // 4 * 4 for D in layers])
    return g


def test_the_old_entry_is_called_when_no_option_is_set():
    g = _plain_model()                                            # its stand-in does not know the new keywords
    out = g.sample_sessions([ids(5, 6), ids(7)], 3, samples=2, top_k=4)
    assert len(out) == 2
    assert len(g.sample_sessions([ids(5, 6), ids(7)], 3, top_p=None, return_logprobs=False, return_hidden=True)) == 3
    with pytest.raises(TypeError):                                # ... and an option goes to the model as a keyword
        g.sample_sessions([ids(5, 6), ids(7)], 3, return_logprobs=True)
    g = _model()
    g.sample_sessions([ids(5, 6)], 2)
    assert 'new_entry' in g._model.last('sample')[1] and g._model.last('sample')[1]['top_p'] is None        # (keywords at their defaults)


def test_the_tuple_layout_and_what_reaches_the_device():
    g = _model()
    hists = [ids(5, 6, 5), ids(9)]
    items, scores, lp = g.sample_sessions(hists, 4, samples=3, top_k=7, top_p=0.9, return_logprobs=True)
    c = g._model.last('sample')[1]
    assert c['top_p'] == float(np.float32(0.9)) and type(c['top_p']) is float and c['return_logprobs'] is True and c['top_k'] == 7
    assert rows_of(c['excl_offs'], c['excl_items']) == [[5, 6], [9]]
    assert items.shape == scores.shape == lp.shape == (2, 3, 4) and lp.dtype == np.float32
    np.testing.assert_array_equal(lp, -scores)
    out = g.sample_sessions(hists, 4, samples=3, return_logprobs=True, return_hidden=True)
    assert len(out) == 4 and isinstance(out[2], list) and out[2][0].shape == (2, 3, 64) and out[3].shape == (2, 3, 4)
    c = g._model.last('sample')[1]
    assert c['top_p'] is None and c['return_logprobs'] is True and c['return_hidden']
    out = g.sample_sessions(hists, 4, top_k=5, top_p=1, return_hidden=True)          # top_p alone: no logprobs in the tuple
    assert len(out) == 3 and isinstance(out[2], list)
    c = g._model.last('sample')[1]
    assert c['top_p'] == 1.0 and c['return_logprobs'] is False
    assert len(g.sample_sessions(hists, 4, top_k=5, top_p=np.float32(0.25))) == 2


def _refused(g, exc, match=None, **kw):
    before = state(g)
    kw.setdefault('steps', 2)
    kw.setdefault('histories', [ids(1)])
    with pytest.raises(exc, match=match):
        g.sample_sessions(**kw)
    assert_same_state(before, state(g))


def test_refusals_happen_before_the_device(monkeypatch):
    g = _model()
    g.predict_next_batch(np.array([1, 2]), ids(10, 20), batch=2)
    for p in (0, 0.0, -0.5, 1.0000001, 2, float('nan'), float('inf'), True, False, 'x', 1e-50, [0.5]):
        _refused(g, ValueError, match='top_p', top_k=5, top_p=p)
    _refused(g, ValueError, match='needs top_k', top_p=0.9)
    _refused(g, ValueError, match='needs top_k', top_p=0.9, return_logprobs=True)
    for r in (1, 0, None, 'yes'):
        _refused(g, ValueError, match='return_logprobs', return_logprobs=r)
    # the older refusals come first and still hold with the options
    _refused(g, ValueError, match='top_k', top_k=0, top_p=0.5)
    _refused(g, ValueError, match='continue_sessions', temperature=0, return_logprobs=True)
    _refused(g, KeyError, histories=[[7]], return_logprobs=True)
    g.sample_sessions([ids(1)], 2, top_k=5, top_p=1e-30)          # a tiny top_p that float32 still holds passes
    # more than 2^24 candidate positions: refused with either option, not without
    monkeypatch.setattr(type(g), '_n_candidates', lambda self, c: 2 ** 24 + 1)
    _refused(g, ValueError, match='2\\^24', return_logprobs=True)
    _refused(g, ValueError, match='2\\^24', top_k=5, top_p=0.5)
    g.sample_sessions([ids(1)], 2, top_k=5)
    before = state(g)
    with pytest.raises(ValueError, match='2\\^24'):
        g.session_log_partition([ids(1)])
    assert_same_state(before, state(g))
    monkeypatch.setattr(type(g), '_n_candidates', lambda self, c: 2 ** 24)
    g.sample_sessions([ids(1)], 2, return_logprobs=True)


def test_session_log_partition():
    g = _model()
    g.predict_next_batch(np.array([1, 2]), ids(10, 20), batch=2)
    before = state(g)
    lse = g.session_log_partition([ids(5, 6, 5), ids(9)], temperature=0.5, exclude_history=True, exclude=ids(40, 3), exclude_per_row=[ids(8), []])
    c = g._model.last('lse')[1]
    assert c['offs'].tolist() == [0, 3, 4] and c['items'].tolist() == [5, 6, 5, 9] and c['item_idx'] is None
    assert c['temperature'] == 0.5 and type(c['temperature']) is float and c['hidden'] is None
    assert rows_of(c['excl_offs'], c['excl_items']) == [[5, 6, 8], [9]]
    assert [i for i in range(300) if (c['excl_mask'][i >> 5] >> (i & 31)) & 1] == [3, 40]
    # lse = fl32(zeta * invT + log(Q 2^-39)) from the stand-in's (zeta, Q) = (i + 1, (i + 1) 2^39)
    assert lse.dtype == np.float32 and lse.shape == (2,)
    np.testing.assert_array_equal(lse, np.array([1 * 2.0 + np.log(1.0), 2 * 2.0 + np.log(2.0)]).astype(np.float32))
    after = state(g)
    assert after[4] == before[4] + 1
    assert_same_state(before[:4] + (0,), after[:4] + (0,))
    g.session_log_partition([ids(1)], predict_for_item_ids=ids(40, 7, 40))           # duplicates are positions of their own
    assert g._model.last('lse')[1]['item_idx'].tolist() == [40, 7, 40] and g._model.last('lse')[1]['excl_offs'] is None
    for t in (0, -1.0, float('nan'), None, 'x', True):
        with pytest.raises(ValueError, match='temperature'):
            g.session_log_partition([ids(1)], temperature=t)
    with pytest.raises(ValueError):
        g.session_log_partition([ids(1), []])
    with pytest.raises(KeyError):
        g.session_log_partition([[7]])
    with pytest.raises(ValueError, match='row 0'):                                    # recommend_sessions' check with k = 1
        g.session_log_partition([ids(1)], predict_for_item_ids=ids(1, 2), exclude=ids(1, 2))


def test_the_binding_knows_the_symbols_the_bound_and_the_mutant():
    for name in ('g4r_sample_sessions_lp', 'g4r_session_log_partition', 'g4r_debug_lse_terms'):
        assert name in _native.SYMBOLS
    assert g4r_module.LSE_CAND_MAX == 2 ** 24
    assert 25 in g4r_build.MUTANTS and 'LAST' in g4r_build.MUTANTS[25] and 'normaliser' in g4r_build.MUTANTS[25]

"""GRU4Rec.score_candidates / score_candidates_sessions without a GPU: every refusal happens before the device model (a recording
stand-in) is called and leaves the prediction state as it was, what reaches it is the CSR of g4r_score_candidates* (row offsets,
candidate item indices) for 2-D and ragged input, and the results come back in the documented layout."""
import numpy as np
import pandas as pd
import pytest

from gru4rec_amd import _native
from gru4rec_amd.gru4rec import GRU4Rec

BASE = 1000     # item id of item index 0


class Recorder:
    """Stand-in for the device model: records every call.  score_candidates* return, for k = 0, the CSR position as the score; for
    k > 0 the positions k - 1, ..., 0 of every row with scores -position."""

    def __init__(self, n_items, layers):
        self.n_items, self.layers, self.calls = n_items, layers, []

    def predict_begin(self, batch):
        self.calls.append(('begin', batch))

    def predict_hidden(self, zero_mask=None):
        self.calls.append(('hidden', np.asarray(zero_mask).copy()))

    def predict_step(self, in_idx, item_idx=None):
        self.calls.append(('predict', np.asarray(in_idx).copy()))
        return np.zeros((len(in_idx), self.n_items if item_idx is None else len(item_idx)), dtype=np.float32)

    @staticmethod
    def _out(offs, k):
        n = len(offs) - 1
        if k == 0:
            return np.arange(offs[-1] - offs[0], dtype=np.float32)
        pos = np.tile(np.arange(k - 1, -1, -1, dtype=np.int32), (n, 1))
        return pos, -pos.astype(np.float32)

    def score_candidates(self, in_idx, cand_offs, cand_items, k=0):
        self.calls.append(('cand', dict(in_idx=np.asarray(in_idx).copy(), offs=np.asarray(cand_offs).copy(),
                                        items=np.asarray(cand_items).copy(), k=k)))
        return self._out(cand_offs, k)

    def score_candidates_sessions(self, hist_offs, hist_items, cand_offs, cand_items, k=0, hidden=None, return_hidden=False):
        self.calls.append(('cand_sessions', dict(hist_offs=np.asarray(hist_offs).copy(), hist_items=np.asarray(hist_items).copy(),
                                                 offs=np.asarray(cand_offs).copy(), items=np.asarray(cand_items).copy(), k=k,
                                                 hidden=None if hidden is None else [np.array(h, copy=True) for h in hidden],
                                                 return_hidden=return_hidden)))
        out = self._out(cand_offs, k)
        if not return_hidden:
            return out
        n = len(hist_offs) - 1
        return out, [(100 * l + np.arange(n, dtype=np.float32))[:, None] * np.ones((1, D), dtype=np.float32) for l, D in enumerate(self.layers)]

    def last(self, kind):
        return [c for c in self.calls if c[0] == kind][-1]


def _model(n_items=300, layers=(64,)):
    g = GRU4Rec(layers=list(layers), final_act='linear')
    g.itemidmap = pd.Series(data=np.arange(n_items), index=np.arange(BASE, BASE + n_items), name='ItemIdx')
    g.n_items = n_items
    g.error_during_train = False
    g._model = Recorder(n_items, [(D + 3) // 4 * 4 for D in layers])
    return g


def ids(*idx):
    return [BASE + i for i in idx]


def state(g):
    return (None if getattr(g, 'current_session', None) is None else np.array(g.current_session, copy=True),
            None if getattr(g, '_seen', None) is None else (g._seen.copy(), g._seen_n.copy(), g._seen_over.copy()),
            getattr(g, 'predict', None), getattr(g, 'predict_batch', None), len(g._model.calls))


def assert_same_state(a, b):
    assert (a[0] is None) == (b[0] is None) and (a[0] is None or np.array_equal(a[0], b[0]))
    assert (a[1] is None) == (b[1] is None)
    if a[1] is not None:
        for x, y in zip(a[1], b[1]):
            np.testing.assert_array_equal(x, y)
    assert a[2] == b[2] and a[3] == b[3]
    assert a[4] == b[4], 'the device model was called by a refused call'


def test_a_2d_array_reaches_the_device_as_a_csr_and_comes_back_2d():
    g = _model()
    cand = np.array([ids(5, 6, 7), ids(9, 9, 1)])
    out = g.score_candidates(np.array([1, 2]), ids(10, 20), cand, batch=2)
    c = g._model.last('cand')[1]
    assert c['offs'].dtype == np.int64 and c['items'].dtype == np.int32 and c['k'] == 0
    assert c['offs'].tolist() == [0, 3, 6] and c['items'].tolist() == [5, 6, 7, 9, 9, 1] and c['in_idx'].tolist() == [10, 20]
    assert out.dtype == np.float32 and out.shape == (2, 3)
    np.testing.assert_array_equal(out, [[0, 1, 2], [3, 4, 5]])


def test_ragged_lists_come_back_as_views_of_one_buffer():
    g = _model()
    cand = [ids(5), np.array(ids(1, 2, 3, 4)), (BASE + 8, BASE + 8)]
    out = g.score_candidates(np.array([1, 2, 3]), ids(10, 20, 30), cand, batch=3)
    c = g._model.last('cand')[1]
    assert c['offs'].tolist() == [0, 1, 5, 7] and c['items'].tolist() == [5, 1, 2, 3, 4, 8, 8]
    assert [x.tolist() for x in out] == [[0], [1, 2, 3, 4], [5, 6]]
    assert all(x.base is out[0].base for x in out)


def test_k_returns_the_items_at_the_selected_positions():
    g = _model()
    cand = [ids(5, 6, 7), ids(1, 2, 3, 4)]
    items, scores = g.score_candidates(np.array([1, 2]), ids(10, 20), cand, k=2, batch=2)
    assert g._model.last('cand')[1]['k'] == 2
    assert items.tolist() == [ids(6, 5), ids(2, 1)] and scores.dtype == np.float32 and scores.shape == (2, 2)
    items, scores = g.score_candidates(np.array([1, 2]), ids(10, 20), np.array(cand[1:] * 2), k=3, batch=2)
    assert items.tolist() == [ids(3, 2, 1), ids(3, 2, 1)]


def test_the_state_advances_as_in_predict_next_batch():
    g = _model()
    g.score_candidates(np.array([1, 2]), ids(10, 20), [ids(1), ids(2)], batch=2)
    assert g.predict_batch == 2 and g.current_session.tolist() == [1, 2]
    assert [c[0] for c in g._model.calls] == ['begin', 'hidden', 'cand']
    g.score_candidates(np.array([1, 3]), ids(11, 21), [ids(1), ids(2)], batch=2)
    assert g._model.calls[-2][0] == 'hidden' and g._model.calls[-2][1].tolist() == [0, 1]
    assert g._seen_n.tolist() == [2, 1] and g._seen[0, :2].tolist() == [10, 11] and g._seen[1, 0] == 21


def _refused(g, exc, **kw):
    before = state(g)
    args = dict(session_ids=np.array([1, 2]), input_item_ids=ids(10, 20), candidates=[ids(1, 2), ids(3)], batch=2)
    args.update(kw)
    with pytest.raises(exc):
        g.score_candidates(**args)
    assert_same_state(before, state(g))


def test_refusals_happen_before_the_device():
    g = _model()
    g.predict_next_batch(np.array([1, 2]), ids(10, 20), batch=2)
    _refused(g, KeyError, candidates=[ids(1), [BASE + 300]])                     # unknown item id
    _refused(g, KeyError, candidates=np.array([ids(1), [BASE - 1]]))
    _refused(g, KeyError, input_item_ids=ids(10, 300))
    _refused(g, ValueError, candidates=[ids(1), []])                             # an empty row
    _refused(g, ValueError, candidates=np.zeros((2, 0), dtype=np.int64))
    _refused(g, ValueError, candidates=[ids(1)])                                 # wrong row count
    _refused(g, ValueError, candidates=np.array([ids(1), ids(2), ids(3)]))
    _refused(g, ValueError, candidates=5)
    for k in (0, -1, 2.5, True, _native.G4R_TOPK_MAX + 1):
        _refused(g, ValueError, k=k)
    _refused(g, ValueError, k=2)                                                 # row 1 holds 1 position
    _refused(g, ValueError, batch=1)                                             # more rows than batch
    g.error_during_train = True
    _refused(g, Exception)


def test_size_limit(monkeypatch):
    g = _model()
    monkeypatch.setattr(_native, 'G4R_CAND_MAX', 3)
    _refused(g, ValueError, candidates=[ids(1, 2), ids(3, 4)])
    g.score_candidates(np.array([1, 2]), ids(10, 20), [ids(1, 2), ids(3)], batch=2)


def test_sessions_csr_hidden_and_layout():
    g = _model(layers=(62,))
    h = [np.full((2, 62), 0.5, dtype=np.float32)]
    out, H = g.score_candidates_sessions([ids(1, 2, 3), np.array(ids(4))], [ids(7, 8), ids(9)], hidden=h, return_hidden=True)
    c = g._model.last('cand_sessions')[1]
    assert c['hist_offs'].tolist() == [0, 3, 4] and c['hist_items'].tolist() == [1, 2, 3, 4]
    assert c['offs'].tolist() == [0, 2, 3] and c['items'].tolist() == [7, 8, 9] and c['k'] == 0 and c['return_hidden']
    assert c['hidden'][0].shape == (2, 64) and (c['hidden'][0][:, 62:] == 0).all() and (c['hidden'][0][:, :62] == 0.5).all()
    assert [x.tolist() for x in out] == [[0, 1], [2]]
    assert H[0].shape == (2, 62) and H[0][1, 0] == 1
    items, scores, H = g.score_candidates_sessions([ids(1), ids(2)], np.array([ids(5, 6), ids(7, 8)]), k=2, return_hidden=True)
    assert items.tolist() == [ids(6, 5), ids(8, 7)] and len(H) == 1
    items, scores = g.score_candidates_sessions([ids(1), ids(2)], np.array([ids(5, 6), ids(7, 8)]), k=1)
    assert items.tolist() == [ids(5), ids(7)]


def _refused_sessions(g, exc, **kw):
    before = state(g)
    args = dict(histories=[ids(1), ids(2, 3)], candidates=[ids(1, 2), ids(3)])
    args.update(kw)
    with pytest.raises(exc):
        g.score_candidates_sessions(**args)
    assert_same_state(before, state(g))


def test_sessions_refusals_and_the_untouched_prediction_state():
    g = _model()
    g.predict_next_batch(np.array([1, 2]), ids(10, 20), batch=2)
    _refused_sessions(g, ValueError, histories=[ids(1), []])
    _refused_sessions(g, ValueError, histories=[])
    _refused_sessions(g, KeyError, histories=[ids(1), [BASE + 300]])
    _refused_sessions(g, KeyError, candidates=[ids(1), [BASE + 300]])
    _refused_sessions(g, ValueError, candidates=[ids(1)])
    _refused_sessions(g, ValueError, candidates=[ids(1), []])
    _refused_sessions(g, ValueError, k=2)
    _refused_sessions(g, ValueError, hidden=[np.zeros((2, 64), dtype=np.float64)])
    _refused_sessions(g, ValueError, hidden=[np.zeros((3, 64), dtype=np.float32)])
    before = state(g)
    g.score_candidates_sessions([ids(1), ids(2, 3)], [ids(1, 2), ids(3)])
    after = state(g)
    assert after[4] == before[4] + 1 and g._model.calls[-1][0] == 'cand_sessions'
    assert_same_state(before[:4] + (after[4],), after)
    g.error_during_train = True
    _refused_sessions(g, Exception)


def test_what_k_is_taken_as():
    """None is the scores of every position; 2.0 counts as 2 (the device receives an int); True, 2.5, 0 and G4R_TOPK_MAX + 1 are
    refused with the call's own message, a k above a list's length with the list's; a string fails inside int(), with int's own
    error.  The same for the two calls."""
    g = _model()
    cand = [ids(40, 7, 41, 3, 9)]
    calls = (('cand', lambda **kw: g.score_candidates(np.array([1]), ids(10), cand, batch=1, **kw)),
             ('cand_sessions', lambda **kw: g.score_candidates_sessions([ids(10)], cand, **kw)))
    for kind, f in calls:
        scores = f(k=None)
        assert g._model.last(kind)[1]['k'] == 0 and len(scores) == 1 and scores[0].shape == (5,)
        items, scores = f(k=2.0)
        got = g._model.last(kind)[1]['k']
        assert got == 2 and type(got) is int and items.shape == scores.shape == (1, 2)
        n = len(g._model.calls)
        for k in (True, 2.5, 0, _native.G4R_TOPK_MAX + 1):
            with pytest.raises(ValueError, match='k = %r: it must be None or an integer in' % (k,)):
                f(k=k)
        with pytest.raises(ValueError, match='candidate list 0 holds 5 positions, fewer than k = 6'):
            f(k=6)
        with pytest.raises(ValueError, match='invalid literal'):
            f(k='a')
        assert len(g._model.calls) == n

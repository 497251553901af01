"""GRU4Rec.recommend_sessions without a GPU: every refusal happens before the device model (a recording stand-in) is called, what
reaches it is the CSR of g4r_recommend_sessions (histories as item indices, per-row exclusion lists sorted and de-duplicated, the
global bit mask) and the hidden state in the device layout, and the prediction state is left exactly as it was."""
import pickle

import numpy as np
import pandas as pd
import pytest

from gru4rec_amd import _native
from gru4rec_amd.gru4rec import GRU4Rec

BASE = 1000     # item id of item index 0


class Recorder:
    """Stand-in for the device model: records every call; recommend_sessions returns the first k positions and, with
    return_hidden, row i of layer l filled with 100 l + i."""

    def __init__(self, n_items, layers):
        self.n_items, self.layers, self.calls = n_items, layers, []

    def predict_begin(self, batch):
        self.calls.append(('begin', batch))

    def predict_hidden(self, zero_mask=None):
        self.calls.append(('hidden', np.asarray(zero_mask).copy()))

    def predict_step(self, in_idx, item_idx=None):
        self.calls.append(('predict', np.asarray(in_idx).copy()))
        return np.zeros((len(in_idx), self.n_items if item_idx is None else len(item_idx)), dtype=np.float32)

    def recommend_step(self, in_idx, item_idx=None, k=20):
        self.calls.append(('recommend', np.asarray(in_idx).copy()))
        return np.tile(np.arange(k, dtype=np.int32), (len(in_idx), 1)), np.zeros((len(in_idx), k), dtype=np.float32)

    def recommend_sessions(self, hist_offs, hist_items, item_idx=None, k=20, excl_offs=None, excl_items=None, excl_mask=None,
                           hidden=None, return_hidden=False):
        cp = (lambda a: None if a is None else np.asarray(a).copy())
        self.calls.append(('sessions', dict(offs=cp(hist_offs), items=cp(hist_items), item_idx=cp(item_idx), k=k, excl_offs=cp(excl_offs),
                                            excl_items=cp(excl_items), excl_mask=cp(excl_mask),
                                            hidden=None if hidden is None else [np.array(h, copy=True) for h in hidden],
                                            return_hidden=return_hidden)))
        n = len(hist_offs) - 1
        cols, scores = np.tile(np.arange(k, dtype=np.int32), (n, 1)), np.zeros((n, k), dtype=np.float32)
        if not return_hidden:
            return cols, scores
        hout = [(100 * l + np.arange(n, dtype=np.float32))[:, None] * np.ones((1, D), dtype=np.float32) for l, D in enumerate(self.layers)]
        return cols, scores, hout

    def recommend_step_filtered(self, in_idx, item_idx=None, k=20, excl_offs=None, excl_items=None, excl_mask=None):
        self.calls.append(('filtered', np.asarray(in_idx).copy(), None if excl_offs is None else np.asarray(excl_offs).copy(),
                           None if excl_items is None else np.asarray(excl_items).copy()))
        return np.tile(np.arange(k, dtype=np.int32), (len(in_idx), 1)), np.zeros((len(in_idx), k), dtype=np.float32)

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


def rows_of(offs, items):
    return [sorted(items[offs[r]:offs[r + 1]].tolist()) for r in range(len(offs) - 1)]


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


def test_histories_reach_the_device_as_a_csr_of_item_indices():
    g = _model()
    items, scores = g.recommend_sessions([ids(5, 6, 7), ids(9), np.array(ids(1, 2))], k=3)
    c = g._model.last('sessions')[1]
    assert c['offs'].dtype == np.int64 and c['items'].dtype == np.int32
    assert c['offs'].tolist() == [0, 3, 4, 6]
    assert c['items'].tolist() == [5, 6, 7, 9, 1, 2]
    assert c['item_idx'] is None and c['k'] == 3 and c['hidden'] is None and not c['return_hidden']
    assert c['excl_offs'] is None and c['excl_items'] is None and c['excl_mask'] is None
    assert items.shape == scores.shape == (3, 3)
    assert items.tolist() == [ids(0, 1, 2)] * 3


def test_candidates_are_item_indices_and_results_item_ids():
    g = _model()
    cand = ids(40, 7, 40, 3)
    items, _ = g.recommend_sessions([ids(1)], k=2, predict_for_item_ids=cand)
    c = g._model.last('sessions')[1]
    assert c['item_idx'].tolist() == [40, 7, 40, 3]
    assert items.tolist() == [ids(40, 7)]


def test_exclude_history_is_a_per_row_union_with_exclude_per_row():
    g = _model()
    g.recommend_sessions([ids(5, 6, 5), ids(9), ids(1, 2)], k=3, exclude_history=True, exclude=ids(40, 3, 40, 299),
                         exclude_per_row=[ids(9, 8, 9), [], {BASE + 100, BASE + 2}])
    c = g._model.last('sessions')[1]
    assert rows_of(c['excl_offs'], c['excl_items']) == [[5, 6, 8, 9], [9], [1, 2, 100]]
    assert c['excl_offs'].dtype == np.int64 and c['excl_items'].dtype == np.int32
    # each row's list sorted and free of duplicates as it arrives
    for r in range(3):
        row = c['excl_items'][c['excl_offs'][r]:c['excl_offs'][r + 1]].tolist()
        assert row == sorted(set(row))
    mask = c['excl_mask']
    assert len(mask) == (300 + 31) // 32 and mask.dtype == np.uint32
    assert [i for i in range(300) if (mask[i >> 5] >> (i & 31)) & 1] == [3, 40, 299]


def test_exclude_history_alone_and_a_mask_alone():
    g = _model()
    g.recommend_sessions([ids(5, 6), ids(7)], k=3, exclude_history=True)
    c = g._model.last('sessions')[1]
    assert rows_of(c['excl_offs'], c['excl_items']) == [[5, 6], [7]] and c['excl_mask'] is None
    g.recommend_sessions([ids(5, 6), ids(7)], k=3, exclude=ids(1))
    c = g._model.last('sessions')[1]
    assert c['excl_offs'] is None and c['excl_items'] is None and c['excl_mask'] is not None


def test_hidden_goes_in_padded_and_comes_back_stripped():
    g = _model(layers=(62, 8))           # 62 -> 64 device columns; 8 stays
    rng = np.random.RandomState(0)
    H = [rng.randn(2, 62).astype(np.float32), rng.randn(2, 8).astype(np.float32)]
    items, scores, Hn = g.recommend_sessions([ids(1), ids(2, 3)], k=2, hidden=H, return_hidden=True)
    c = g._model.last('sessions')[1]
    assert c['return_hidden']
    h0 = c['hidden']
    assert [h.shape for h in h0] == [(2, 64), (2, 8)]
    np.testing.assert_array_equal(h0[0][:, :62], H[0])
    assert not h0[0][:, 62:].any()
    np.testing.assert_array_equal(h0[1], H[1])
    assert [h.shape for h in Hn] == [(2, 62), (2, 8)] and all(h.dtype == np.float32 for h in Hn)
    np.testing.assert_array_equal(Hn[0], np.array([[0.] * 62, [1.] * 62], dtype=np.float32))
    np.testing.assert_array_equal(Hn[1], np.array([[100.] * 8, [101.] * 8], dtype=np.float32))
    assert items.shape == (2, 2)


def _refused(g, exc, **kw):
    before = state(g)
    with pytest.raises(exc):
        g.recommend_sessions(**kw)
    assert_same_state(before, state(g))


def test_refusals_happen_before_the_device():
    g = _model()
    g.predict_next_batch(np.array([1, 2]), ids(10, 20), batch=2)
    h = [np.zeros((2, 64), dtype=np.float32)]
    _refused(g, ValueError, histories=[ids(1), []])                                       # an empty history
    _refused(g, ValueError, histories=[])                                                # no session
    _refused(g, KeyError, histories=[ids(1), [BASE + 300]])                               # unknown item id
    _refused(g, KeyError, histories=[ids(1)], k=1, predict_for_item_ids=[BASE - 1])
    _refused(g, KeyError, histories=[ids(1)], exclude=[7])
    _refused(g, KeyError, histories=[ids(1)], exclude_per_row=[[7]])
    _refused(g, ValueError, histories=[ids(1), ids(2)], hidden=h + h)                      # layer count
    _refused(g, ValueError, histories=[ids(1), ids(2)], hidden=[np.zeros((3, 64), dtype=np.float32)])     # shape
    _refused(g, ValueError, histories=[ids(1), ids(2)], hidden=[np.zeros((2, 63), dtype=np.float32)])
    _refused(g, ValueError, histories=[ids(1), ids(2)], hidden=[np.zeros((2, 64), dtype=np.float64)])     # dtype
    _refused(g, ValueError, histories=[ids(1), ids(2)], hidden=np.zeros((1, 2, 64), dtype=np.float32))
    for k in (0, 257, 2.5):
        _refused(g, ValueError, histories=[ids(1)], k=k)
    _refused(g, ValueError, histories=[ids(1)], k=4, predict_for_item_ids=ids(1, 2, 3))
    _refused(g, ValueError, histories=[ids(1), ids(2)], exclude_per_row=[ids(3)])          # one list per row
    _refused(g, ValueError, histories=[ids(1)], k=2, predict_for_item_ids=ids(1, 2, 3), exclude_history=True, exclude=ids(2))
    _refused(g, ValueError, histories=[ids(*range(150))], k=200, exclude_history=True)    # 300 - 150 eligible < 200
    big = _model(n_items=3000)
    _refused(big, ValueError, histories=[ids(*range(1000))], exclude_history=True, exclude_per_row=[ids(*range(1000, 1100))])
    g.error_during_train = True
    _refused(g, Exception, histories=[ids(1)])


def test_a_row_with_just_k_eligible_positions_passes():
    g = _model()
    g.recommend_sessions([ids(*range(150))], k=150, exclude_history=True)
    g.recommend_sessions([ids(1, 2)], k=2, predict_for_item_ids=ids(1, 2, 3, 3), exclude_history=True)     # duplicates count
    assert len([c for c in g._model.calls if c[0] == 'sessions']) == 2


def test_the_prediction_state_is_untouched():
    g = _model()
    g.recommend_sessions([ids(1, 2)], k=2)           # before any predict call: no prediction state appears
    assert getattr(g, 'predict', None) is None and getattr(g, '_seen', None) is None
    g.predict_next_batch(np.array([1, 2]), ids(10, 20), batch=2)
    g.recommend_next_batch(np.array([1, 3]), ids(11, 21), k=2, batch=2)
    before = state(g)
    blob = pickle.dumps(g)
    g.recommend_sessions([ids(1, 2, 3), ids(4)], k=2, exclude_history=True, hidden=[np.ones((2, 64), dtype=np.float32)],
                         return_hidden=True)
    after = state(g)
    assert after[4] == before[4] + 1 and g._model.calls[-1][0] == 'sessions'
    assert_same_state(before[:4] + (0,), after[:4] + (0,))
    assert pickle.dumps(g) == blob
    # the seen-history and the slots carry on as if the call had not been made
    g.recommend_next_batch(np.array([1, 3]), ids(12, 22), k=2, batch=2, exclude_seen=True)
    _, in_idx, offs, items = g._model.last('filtered')
    assert in_idx.tolist() == [12, 22]
    assert rows_of(offs, items) == [[10, 11, 12], [21, 22]]


def test_exclude_max_names_the_history():
    g = _model(n_items=3000)
    with pytest.raises(ValueError, match='the history'):
        g.recommend_sessions([ids(*range(1025))], exclude_history=True)
    assert _native.G4R_EXCLUDE_MAX == 1024


def test_what_k_is_taken_as():
    """True counts as 1 and 2.0 as 2 (the device receives an int); 2.5, 0 and number of candidates + 1 are refused with the call's own
    message; a string and None fail inside int(), with int's own error."""
    g = _model()
    cand = ids(40, 7, 41, 3, 9)
    for k, want in ((True, 1), (2.0, 2)):
        items, scores = g.recommend_sessions([ids(1)], k=k, predict_for_item_ids=cand)
        got = g._model.last('sessions')[1]['k']
        assert got == want and type(got) is int and items.shape == scores.shape == (1, want)
    before = state(g)
    for k in (2.5, 0, 6):
        with pytest.raises(ValueError, match='k = %r: it must be an integer in' % (k,)):
            g.recommend_sessions([ids(1)], k=k, predict_for_item_ids=cand)
    with pytest.raises(ValueError, match='invalid literal'):
        g.recommend_sessions([ids(1)], k='a', predict_for_item_ids=cand)
    _refused(g, TypeError, histories=[ids(1)], k=None, predict_for_item_ids=cand)
    assert_same_state(before, state(g))

"""GRU4Rec.continue_sessions without a GPU: every refusal happens before the device model (a recording stand-in) is called, what
reaches it is the CSR of g4r_continue_sessions (histories as item indices, per-row exclusion lists sorted and de-duplicated -- the
history among them with no_repeat -- the global bit mask, the hidden state in the device layout, steps and no_repeat), the output is
[N, steps, k], and the prediction state is left exactly as it was."""
import pickle

import numpy as np
import pandas as pd
import pytest

from gru4rec_amd import _native
from gru4rec_amd.gru4rec import GRU4Rec

BASE = 1000     # item id of item index 0
XMAX = _native.G4R_EXCLUDE_MAX


class Recorder:
    """Stand-in for the device model: records every call; continue_sessions returns position (s + j) % candidates at [:, s, j] and, with
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

    def continue_sessions(self, hist_offs, hist_items, item_idx=None, k=1, steps=1, no_repeat=True, excl_offs=None, excl_items=None,
                          excl_mask=None, hidden=None, return_hidden=False, oversample=None):
        cp = (lambda a: None if a is None else np.asarray(a).copy())
        self.calls.append(('continue', dict(offs=cp(hist_offs), items=cp(hist_items), item_idx=cp(item_idx), k=k, steps=steps,
                                            no_repeat=no_repeat, excl_offs=cp(excl_offs), excl_items=cp(excl_items),
                                            excl_mask=cp(excl_mask), oversample=oversample,
                                            hidden=None if hidden is None else [np.array(h, copy=True) for h in hidden],
                                            return_hidden=return_hidden)))
        n = len(hist_offs) - 1
        n_sel = self.n_items if item_idx is None else len(item_idx)
        cols = np.tile(((np.arange(steps)[:, None] + np.arange(k)[None, :]) % n_sel).astype(np.int32), (n, 1, 1))
        scores = np.zeros((n, steps, k), dtype=np.float32)
        if not return_hidden:
            return cols, scores
        hout = [(100 * l + np.arange(n, dtype=np.float32))[:, None] * np.ones((1, D), dtype=np.float32) for l, D in enumerate(self.layers)]
        return cols, scores, hout

    def last(self, kind):
        return [c for c in self.calls if c[0] == kind][-1]


def _model(n_items=300, layers=(64,), final_act='linear'):
    g = GRU4Rec(layers=list(layers), final_act=final_act)
    g.itemidmap = pd.Series(data=np.arange(n_items), index=np.arange(BASE, BASE + n_items), name='ItemIdx')
    g.n_items = n_items
    g.error_during_train = False
    g._model = Recorder(n_items, [(D + 3) // 4 * 4 for D in layers])
    return g


def ids(*idx):
    return [BASE + i for i in idx]


def rows_of(offs, items):
    return [items[offs[r]:offs[r + 1]].tolist() for r in range(len(offs) - 1)]


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


def test_what_reaches_the_device_and_the_output_shape():
    g = _model()
    items, scores = g.continue_sessions([ids(5, 6, 5), ids(9), np.array(ids(1, 2))], 4, k=3, exclude=ids(40, 3, 40, 299),
                                        exclude_per_row=[ids(9, 8, 9), [], {BASE + 100, BASE + 2}])
    c = g._model.last('continue')[1]
    assert c['offs'].dtype == np.int64 and c['items'].dtype == np.int32
    assert c['offs'].tolist() == [0, 3, 4, 6] and c['items'].tolist() == [5, 6, 5, 9, 1, 2]
    assert c['item_idx'] is None and c['k'] == 3 and c['steps'] == 4 and c['no_repeat'] is True
    assert c['hidden'] is None and not c['return_hidden'] and c['oversample'] is None
    # the history is part of every row's list (no_repeat), each list sorted and free of duplicates
    assert c['excl_offs'].dtype == np.int64 and c['excl_items'].dtype == np.int32
    assert rows_of(c['excl_offs'], c['excl_items']) == [[5, 6, 8, 9], [9], [1, 2, 100]]
    mask = c['excl_mask']
    assert len(mask) == (300 + 31) // 32 and mask.dtype == np.uint32
    assert [i for i in range(300) if (mask[i >> 5] >> (i & 31)) & 1] == [3, 40, 299]
    assert items.shape == scores.shape == (3, 4, 3) and scores.dtype == np.float32
    assert items[1].tolist() == [ids(0, 1, 2), ids(1, 2, 3), ids(2, 3, 4), ids(3, 4, 5)]


def test_without_no_repeat_the_history_is_not_listed():
    g = _model()
    g.continue_sessions([ids(5, 6), ids(7)], 3, k=2, no_repeat=False)
    c = g._model.last('continue')[1]
    assert c['no_repeat'] is False and c['steps'] == 3
    assert c['excl_offs'] is None and c['excl_items'] is None and c['excl_mask'] is None
    g.continue_sessions([ids(5, 6), ids(7)], 3, k=2, no_repeat=False, exclude_per_row=[ids(8), ids(7, 2)])
    c = g._model.last('continue')[1]
    assert rows_of(c['excl_offs'], c['excl_items']) == [[8], [2, 7]]
    g.continue_sessions([ids(5, 6), ids(7)], 3, k=2)
    c = g._model.last('continue')[1]
    assert rows_of(c['excl_offs'], c['excl_items']) == [[5, 6], [7]] and c['excl_mask'] is None


def test_candidates_are_item_indices_and_results_item_ids():
    g = _model()
    cand = ids(40, 7, 41, 3, 9)
    items, _ = g.continue_sessions([ids(1)], 2, k=2, predict_for_item_ids=cand)
    c = g._model.last('continue')[1]
    assert c['item_idx'].tolist() == [40, 7, 41, 3, 9]
    assert items.tolist() == [[ids(40, 7), ids(7, 41)]]


def test_scan_and_oversample_pass_through():
    g = _model()
    g.continue_sessions([ids(1)], 2, k=2, scan='bf16', oversample=4)
    assert g._model.last('continue')[1]['oversample'] == 4
    g.continue_sessions([ids(1)], 2, k=2, scan='fp32', oversample=4)
    assert g._model.last('continue')[1]['oversample'] is None


def test_hidden_goes_in_padded_and_comes_back_stripped():
    g = _model(layers=(62, 8))           # 62 -> 64 device columns; 8 stays
    rng = np.random.RandomState(0)
    H = [rng.randn(2, 62).astype(np.float32), rng.randn(2, 8).astype(np.float32)]
    items, scores, Hn = g.continue_sessions([ids(1), ids(2, 3)], 3, k=2, hidden=H, return_hidden=True)
    c = g._model.last('continue')[1]
    assert c['return_hidden']
    h0 = c['hidden']
    assert [h.shape for h in h0] == [(2, 64), (2, 8)]
    np.testing.assert_array_equal(h0[0][:, :62], H[0])
    assert not h0[0][:, 62:].any()
    np.testing.assert_array_equal(h0[1], H[1])
    assert [h.shape for h in Hn] == [(2, 62), (2, 8)] and all(h.dtype == np.float32 for h in Hn)
    np.testing.assert_array_equal(Hn[0], np.array([[0.] * 62, [1.] * 62], dtype=np.float32))
    np.testing.assert_array_equal(Hn[1], np.array([[100.] * 8, [101.] * 8], dtype=np.float32))
    assert items.shape == (2, 3, 2)


def _refused(g, exc, match=None, **kw):
    before = state(g)
    kw.setdefault('steps', 2)
    with pytest.raises(exc, match=match):
        g.continue_sessions(**kw)
    assert_same_state(before, state(g))


def test_refusals_happen_before_the_device():
    g = _model()
    g.predict_next_batch(np.array([1, 2]), ids(10, 20), batch=2)
    h = [np.zeros((2, 64), dtype=np.float32)]
    for steps in (0, -1, 2.5, True, None, 'x'):
        _refused(g, ValueError, match='steps', histories=[ids(1)], steps=steps)
    _refused(g, ValueError, histories=[ids(1), []])                                       # an empty history
    _refused(g, ValueError, histories=[])                                                # no session
    _refused(g, KeyError, histories=[ids(1), [BASE + 300]])                               # unknown item id
    _refused(g, KeyError, histories=[ids(1)], k=1, predict_for_item_ids=[BASE - 1])
    _refused(g, KeyError, histories=[ids(1)], exclude=[7])
    _refused(g, KeyError, histories=[ids(1)], exclude_per_row=[[7]])
    _refused(g, ValueError, histories=[ids(1), ids(2)], hidden=h + h)                      # layer count
    _refused(g, ValueError, histories=[ids(1), ids(2)], hidden=[np.zeros((3, 64), dtype=np.float32)])     # shape
    _refused(g, ValueError, histories=[ids(1), ids(2)], hidden=[np.zeros((2, 64), dtype=np.float64)])     # dtype
    for k in (0, 257, 2.5):
        _refused(g, ValueError, histories=[ids(1)], k=k)
    _refused(g, ValueError, histories=[ids(1)], k=4, predict_for_item_ids=ids(1, 2, 3))
    _refused(g, ValueError, histories=[ids(1), ids(2)], exclude_per_row=[ids(3)])          # one list per row
    _refused(g, ValueError, histories=[ids(1)], scan='fp16')
    _refused(g, ValueError, histories=[ids(1)], scan='bf16', oversample=0)
    _refused(g, ValueError, histories=[ids(1)], k=200, scan='bf16', oversample=8)
    _refused(_model(final_act='softmax'), NotImplementedError, histories=[ids(1)], scan='bf16')
    g.error_during_train = True
    _refused(g, Exception, histories=[ids(1)])


def test_no_repeat_needs_duplicate_free_candidates():
    g = _model()
    cand = ids(40, 7, 40, 3, 9, 11)
    _refused(g, ValueError, match='duplicate-free', histories=[ids(1)], k=2, predict_for_item_ids=cand)
    g.continue_sessions([ids(1)], 2, k=2, predict_for_item_ids=cand, no_repeat=False)       # without no_repeat duplicates are allowed
    assert g._model.last('continue')[1]['item_idx'].tolist() == [40, 7, 40, 3, 9, 11]


def test_the_eligible_count_boundary():
    g = _model()
    # 12 candidates, 2 of them in row 1's history: row 1 has 10 eligible positions; steps = 6 takes 5 of them: k = 5 is the most
    cand = ids(*range(100, 112))
    hists = [ids(1, 2), ids(100, 3, 101)]
    g.continue_sessions(hists, 6, k=5, predict_for_item_ids=cand)                           # eligible - (steps - 1) == k
    assert g._model.last('continue')[1]['steps'] == 6
    _refused(g, ValueError, match='row 1', histories=hists, steps=7, k=5, predict_for_item_ids=cand)
    _refused(g, ValueError, match='row 1', histories=hists, steps=6, k=6, predict_for_item_ids=cand)
    _refused(g, ValueError, match='row 0', histories=[ids(1)], steps=6, k=5, predict_for_item_ids=cand, exclude=ids(100, 101, 102))
    # all items: 300 - 2 (history) - 1 (exclude_per_row) = 297 eligible
    g.continue_sessions([ids(1, 2)], 98, k=200, exclude_per_row=[ids(3)])
    _refused(g, ValueError, match='row 0', histories=[ids(1, 2)], steps=99, k=200, exclude_per_row=[ids(3)])
    # without no_repeat the generated items take nothing: the check is recommend_sessions' own
    g.continue_sessions([ids(1, 2)], 99, k=200, exclude_per_row=[ids(3)], no_repeat=False)
    g.continue_sessions(hists, 50, k=12, predict_for_item_ids=cand, no_repeat=False)
    _refused(g, ValueError, histories=hists, steps=50, k=12, predict_for_item_ids=cand, no_repeat=False, exclude_per_row=[[], ids(100)])


def test_the_list_length_boundary():
    g = _model(n_items=3000)
    hist = ids(*range(XMAX - 10))                                                         # 1014 distinct items listed
    g.continue_sessions([ids(5), hist], 11, k=1)                                          # 1014 + 10 == G4R_EXCLUDE_MAX
    _refused(g, ValueError, match='row 1', histories=[ids(5), hist], steps=12, k=1)
    _refused(g, ValueError, match='row 1', histories=[ids(5), hist], steps=11, k=1, exclude_per_row=[[], ids(2999)])
    g.continue_sessions([ids(5), hist], 11, k=1, exclude_per_row=[[], ids(3)])             # already listed: not one more
    g.continue_sessions([ids(5), hist], 500, k=1, no_repeat=False, exclude_per_row=[[], hist])     # the lists do not grow
    with pytest.raises(ValueError, match='the history'):
        g.continue_sessions([ids(*range(XMAX + 1))], 1)
    g.continue_sessions([ids(*range(XMAX))], 1)                                           # steps = 1 generates nothing


def test_the_prediction_state_is_untouched():
    g = _model()
    g.continue_sessions([ids(1, 2)], 3, k=2)           # before any predict call: no prediction state appears
    assert getattr(g, 'predict', None) is None and getattr(g, '_seen', None) is None
    g.predict_next_batch(np.array([1, 2]), ids(10, 20), batch=2)
    g.recommend_next_batch(np.array([1, 3]), ids(11, 21), k=2, batch=2)
    before = state(g)
    blob = pickle.dumps(g)
    g.continue_sessions([ids(1, 2, 3), ids(4)], 3, k=2, hidden=[np.ones((2, 64), dtype=np.float32)], return_hidden=True)
    after = state(g)
    assert after[4] == before[4] + 1 and g._model.calls[-1][0] == 'continue'
    assert_same_state(before[:4] + (0,), after[:4] + (0,))
    assert pickle.dumps(g) == blob


def test_what_k_is_taken_as():
    """True counts as 1 and 2.0 as 2 (the device receives an int); 2.5, 0 and number of candidates + 1 are refused with the call's own
    message; a string and None fail inside int(), with int's own error."""
    g = _model()
    cand = ids(40, 7, 41, 3, 9)
    for k, want in ((True, 1), (2.0, 2)):
        items, scores = g.continue_sessions([ids(1)], 2, k=k, predict_for_item_ids=cand)
        got = g._model.last('continue')[1]['k']
        assert got == want and type(got) is int and items.shape == scores.shape == (1, 2, want)
    for k in (2.5, 0, 6):
        _refused(g, ValueError, match='k = %r: it must be an integer in' % (k,), histories=[ids(1)], k=k, predict_for_item_ids=cand)
    _refused(g, ValueError, match='invalid literal', histories=[ids(1)], k='a', predict_for_item_ids=cand)
    _refused(g, TypeError, histories=[ids(1)], k=None, predict_for_item_ids=cand)

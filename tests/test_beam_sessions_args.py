"""GRU4Rec.beam_sessions without a GPU: every refusal happens before the device model (a recording stand-in) is called, what reaches
it is the CSR of g4r_beam_sessions, the paths come out of the back-pointer records through _native.beam_backtrack, and the NumPy
statement of the combine / order / rescale rule that the GPU test's host loop is made of (test_gpu_beam_sessions.py) does what the
contract says on hand-made values."""
import numpy as np
import pandas as pd
import pytest

from gru4rec_amd import _native
from gru4rec_amd.gru4rec import GRU4Rec
from test_gpu_beam_sessions import best_extensions, combine_scores, rescale

BASE = 1000     # item id of item index 0
XMAX = _native.G4R_EXCLUDE_MAX
BMAX = _native.G4R_BEAM_MAX


class Recorder:
    """Stand-in for the device model: records every call; beam_sessions returns, at step s, beam i extending beam (i + 1) % beams by
    candidate position (s + i) % candidates with step score 10 s + i."""

    def __init__(self, n_items, layers):
        self.n_items, self.layers, self.calls = n_items, layers, []

    def beam_sessions(self, hist_offs, hist_items, item_idx=None, beams=4, steps=1, no_repeat=True, combine='sum', excl_offs=None,
                      excl_items=None, excl_mask=None, hidden=None, oversample=None):
        cp = (lambda a: None if a is None else np.asarray(a).copy())
        self.calls.append(dict(offs=cp(hist_offs), items=cp(hist_items), item_idx=cp(item_idx), beams=beams, steps=steps,
                               no_repeat=no_repeat, combine=combine, excl_offs=cp(excl_offs), excl_items=cp(excl_items),
                               excl_mask=cp(excl_mask), oversample=oversample,
                               hidden=None if hidden is None else [np.array(h, copy=True) for h in hidden]))
        n = len(hist_offs) - 1
        n_sel = self.n_items if item_idx is None else len(item_idx)
        s, i = np.arange(steps)[:, None], np.arange(beams)[None, :]
        parent = np.tile(np.where(s == 0, i, (i + 1) % beams).astype(np.int32), (n, 1, 1))
        cols = np.tile(((s + i) % n_sel).astype(np.int32), (n, 1, 1))
        scores = np.tile((10 * s + i).astype(np.float32), (n, 1, 1))
        return parent, cols, scores, np.tile(np.arange(beams, dtype=np.float32), (n, 1)), np.full(n, -3, dtype=np.int32)


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


# ---- what reaches the device, what comes back ----------------------------------------------------------------------------------------
def test_what_reaches_the_device_and_the_output():
    g = _model()
    paths, path_scores, step_scores, scale_exp = g.beam_sessions([ids(5, 6, 5), ids(9), np.array(ids(1, 2))], 3, beams=2,
                                                                 exclude=ids(40, 3, 40, 299), exclude_per_row=[ids(7, 5), [], ids(2, 8)])
    c = g._model.calls[-1]
    assert c['beams'] == 2 and c['steps'] == 3 and c['no_repeat'] is True and c['combine'] == 'sum' and c['oversample'] is None
    assert c['item_idx'] is None and c['hidden'] is None
    assert rows_of(c['offs'], c['items']) == [[5, 6, 5], [9], [1, 2]]
    assert rows_of(c['excl_offs'], c['excl_items']) == [[5, 6, 7], [9], [1, 2, 8]]      # sorted, de-duplicated, the history among them
    assert sorted(np.flatnonzero(np.unpackbits(c['excl_mask'].view(np.uint8), bitorder='little')).tolist()) == [3, 40, 299]
    assert paths.shape == step_scores.shape == (3, 2, 3) and path_scores.shape == (3, 2) and scale_exp.tolist() == [-3, -3, -3]
    # final beam 0 <- beam 1 of step 1 <- beam 0 of step 0: positions (0 + 0, 1 + 1, 2 + 0), scores (0, 11, 20)
    assert paths[0].tolist() == [ids(0, 2, 2), ids(1, 1, 3)]
    assert step_scores[1].tolist() == [[0.0, 11.0, 20.0], [1.0, 10.0, 21.0]]
    assert step_scores.dtype == np.float32


def test_defaults_of_combine_and_the_other_arguments():
    g = _model(final_act='softmax')
    g.beam_sessions([ids(1)], 2)
    assert g._model.calls[-1]['combine'] == 'product' and g._model.calls[-1]['beams'] == 4
    g.beam_sessions([ids(1)], 2, combine='sum', no_repeat=False)
    c = g._model.calls[-1]
    assert c['combine'] == 'sum' and c['no_repeat'] is False and c['excl_offs'] is None and c['excl_mask'] is None
    g = _model(final_act='softmax_logit')
    g.beam_sessions([ids(1)], 2)
    assert g._model.calls[-1]['combine'] == 'product'
    g = _model(final_act='elu-0.5')
    cand = ids(9, 4, 250, 7, 8)
    paths, _, _, _ = g.beam_sessions([ids(1)], 2, beams=2, predict_for_item_ids=cand, scan='bf16', oversample=4)
    c = g._model.calls[-1]
    assert c['combine'] == 'sum' and c['item_idx'].tolist() == [9, 4, 250, 7, 8] and c['oversample'] == 4
    assert paths[0].tolist() == [[cand[1], cand[1]], [cand[0], cand[2]]]               # positions map through the candidates
    H = [np.arange(2 * 30, dtype=np.float32).reshape(2, 30)]
    g = _model(layers=(30,))
    g.beam_sessions([ids(1), ids(2, 3)], 2, hidden=H)
    h = g._model.calls[-1]['hidden']
    assert h[0].shape == (2, 32) and np.array_equal(h[0][:, :30], H[0]) and not h[0][:, 30:].any()


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def refused(g, exc, match, *a, **kw):
    before = len(g._model.calls)
    with pytest.raises(exc, match=match):
        g.beam_sessions(*a, **kw)
    assert len(g._model.calls) == before, 'the device model was called by a refused call'
    assert getattr(g, 'predict', None) is None and getattr(g, 'current_session', None) is None


@pytest.mark.parametrize('beams', [0, -1, 2.5, True, BMAX + 1, None, 'x'])
def test_a_bad_beams_is_refused(beams):
    refused(_model(), ValueError, 'beams', [ids(1)], 2, beams=beams)


def test_beams_above_the_candidates_is_refused():
    g = _model()
    refused(g, ValueError, 'beams', [ids(1)], 2, beams=4, predict_for_item_ids=ids(1, 2, 3))
    g.beam_sessions([ids(1)], 1, beams=3, predict_for_item_ids=ids(1, 2, 3), no_repeat=False)
    g.beam_sessions([ids(1)], 1, beams=BMAX)


@pytest.mark.parametrize('steps', [0, -2, 1.5, True, None, 'x'])
def test_a_bad_steps_is_refused(steps):
    refused(_model(), ValueError, 'steps', [ids(1)], steps)


def test_a_bad_combine_is_refused():
    refused(_model(), ValueError, 'combine', [ids(1)], 2, combine='max')
    refused(_model(final_act='softmax'), ValueError, 'combine', [ids(1)], 2, combine=0)
    for act in ('linear', 'tanh', 'elu-0.5'):
        refused(_model(final_act=act), ValueError, 'softmax', [ids(1)], 2, combine='product')
    _model(final_act='softmax').beam_sessions([ids(1)], 2, combine='product')


def test_the_refusals_of_continue_sessions_with_k_beams():
    g = _model()
    refused(g, ValueError, 'duplicate-free', [ids(1)], 2, beams=2, predict_for_item_ids=ids(4, 5, 4, 6))
    g.beam_sessions([ids(1)], 2, beams=2, predict_for_item_ids=ids(4, 5, 4, 6), no_repeat=False)
    cand = ids(*range(10, 22))                                                          # 12 candidates
    hists = [ids(1, 2), ids(3, 10)]                                                     # row 1 has 11 eligible
    refused(g, ValueError, 'row 1 has 11 eligible candidate positions, fewer than k \\+ steps - 1 = 12', hists, 5, beams=8,
            predict_for_item_ids=cand)
    g.beam_sessions(hists, 4, beams=8, predict_for_item_ids=cand)                       # eligible - (steps - 1) == beams
    g.beam_sessions(hists, 50, beams=8, predict_for_item_ids=cand, no_repeat=False)     # nothing is used up
    refused(g, ValueError, 'row 0 has 2 eligible candidate positions, fewer than k = 3', [ids(1)], 1, beams=3,
            predict_for_item_ids=ids(1, 2, 3))
    big = _model(n_items=XMAX + 40)
    hist = ids(*range(XMAX - 10))
    big.beam_sessions([ids(5), hist], 11, beams=1)                                      # 1014 + 10 == G4R_EXCLUDE_MAX
    refused(big, ValueError, 'row 1 excludes 1014 distinct items .* steps - 1 = 11 more', [ids(5), hist], 12, beams=1)
    refused(big, ValueError, 'row 0 excludes %d distinct items' % (XMAX + 1), [ids(*range(XMAX + 1))], 1)
    refused(g, ValueError, 'exclude_per_row holds 1 lists', [ids(1), ids(2)], 2, exclude_per_row=[ids(3)])
    refused(g, ValueError, 'histories is empty', [], 2)
    refused(g, ValueError, 'history 1 is empty', [ids(1), []], 2)
    refused(g, KeyError, None, [ids(1), [5]], 2)
    refused(g, KeyError, None, [ids(1)], 2, exclude=[7])
    refused(g, KeyError, None, [ids(1)], 2, predict_for_item_ids=[1, 2, 3, 4, 5])
    refused(g, ValueError, 'hidden must be a list of 1 arrays', [ids(1)], 2, hidden=[np.zeros((1, 64), np.float32)] * 2)
    refused(g, ValueError, 'hidden\\[0\\] must be a float32 array of shape \\(1, 64\\)', [ids(1)], 2, hidden=[np.zeros((2, 64), np.float32)])
    refused(g, ValueError, 'hidden\\[0\\] must be a float32 array', [ids(1)], 2, hidden=[np.zeros((1, 64), np.float64)])
    refused(g, ValueError, 'scan', [ids(1)], 2, scan='fp16')
    refused(g, ValueError, 'oversample', [ids(1)], 2, scan='bf16', oversample=0)
    refused(g, ValueError, 'k \\* oversample', [ids(1)], 2, beams=8, scan='bf16', oversample=129)
    with pytest.raises(NotImplementedError):
        _model(final_act='softmax').beam_sessions([ids(1)], 2, scan='bf16')
    with pytest.raises(TypeError):
        g.beam_sessions([ids(1)], 2, return_hidden=True)                                 # not part of this call


# ---- the backtrack ---------------------------------------------------------------------------------------------------------------------
def test_backtrack_follows_the_parents():
    # one session, 3 steps, 3 beams; the parents of step 1 and 2 are no identity: a beam dies (1 at step 1), one forks (0 at step 1)
    parent = np.array([[[0, 1, 2], [2, 0, 0], [1, 1, 0]]], dtype=np.int32)
    cols = np.array([[[10, 11, 12], [20, 21, 22], [30, 31, 32]]], dtype=np.int32)
    scores = (cols / 4).astype(np.float32)
    paths, ss = _native.beam_backtrack(parent, cols, scores)
    assert paths.dtype == np.int32 and ss.dtype == np.float32
    assert paths[0].tolist() == [[10, 21, 30], [10, 21, 31], [12, 20, 32]]
    assert ss[0].tolist() == [[2.5, 5.25, 7.5], [2.5, 5.25, 7.75], [3.0, 5.0, 8.0]]
    # two sessions with different tables do not mix
    parent2 = np.concatenate([parent, parent[:, :, ::-1]])
    paths2, _ = _native.beam_backtrack(parent2, np.concatenate([cols, cols + 100]), np.concatenate([scores, scores]))
    assert paths2[0].tolist() == paths[0].tolist()
    # session 1: step 2 parents (0, 1, 1), step 1 parents (0, 0, 2); step 0's record has no parent to follow
    assert paths2[1].tolist() == [[110, 120, 130], [110, 121, 131], [110, 121, 132]]
    one, _ = _native.beam_backtrack(parent[:, :1], cols[:, :1], scores[:, :1])             # a single step: the columns themselves
    assert one[0].tolist() == [[10], [11], [12]]


# ---- the rule of the host loop -----------------------------------------------------------------------------------------------------------
def test_combine_rule():
    f = np.float32
    s = combine_scores(f(1.0), np.array([2.0 ** -24, 0.5], dtype=f), 'sum')
    assert s.dtype == f and s.tolist() == [1.0, 1.5]                                       # rounded once, to float32 (ties to even)
    p = combine_scores(f(2.0 ** -100), np.array([2.0 ** -26, 2.0 ** -27, 0.0, 0.75], dtype=f), 'product')
    assert p.dtype == f and p.tolist() == [2.0 ** -126, 0.0, 0.0, 0.75 * 2.0 ** -100]      # below 2^-126 -> 0, 2^-126 itself stays
    p = combine_scores(f(-2.0 ** -100), np.array([2.0 ** -40], dtype=f), 'product')
    assert p.view(np.uint32).tolist() == [0]                                               # +0.0, not -0.0
    p = combine_scores(np.array([np.nan, np.inf, 1.0], dtype=f), np.array([0.5, 0.5, np.nan], dtype=f), 'product')
    assert np.isnan(p[0]) and p[1] == np.inf and np.isnan(p[2])                            # NaN is not replaced


def test_order_rule():
    p = np.array([0.5, np.nan, 2.0, 0.5, -0.0, 0.0, 2.0, -np.inf], dtype=np.float32)
    assert best_extensions(p, 8) == [2, 6, 0, 3, 4, 5, 7, 1]                              # equal scores by position, -0.0 == 0.0, NaN last
    assert best_extensions(p, 3) == [2, 6, 0]


def test_rescale_rule():
    f = np.float32
    q, e = rescale(np.array([1.0, 0.25], dtype=f))
    assert e == 0 and q.tolist() == [1.0, 0.25]                                            # m = 1.0: nothing moves
    q, e = rescale(np.array([0.75 * 2.0 ** -9, 2.0 ** -20, 0.0], dtype=f))
    assert e == -10 and q.dtype == f and q.tolist() == [1.5, 2.0 ** -10, 0.0] and 1 <= q[0] < 2
    q, e = rescale(np.array([np.nextafter(f(2.0), f(0.0)) * f(2.0 ** -30), 2.0 ** -126], dtype=f))
    assert e == -30 and 1 <= q[0] < 2 and q[1] == 2.0 ** -96                               # the largest mantissa stays below 2
    for m in (0.0, np.nan, np.inf, -1.0):
        q, e = rescale(np.array([m, 0.5], dtype=f))
        assert e == 0 and q[1] == 0.5                                                      # not finite, or not > 0: untouched
    # a long product: 40 steps of 2^-8 underflow a float32, the rescaled pair (score, exponent) does not
    cum, scale = np.array([1.0], dtype=f), 0
    for _ in range(40):
        cum, e = rescale(combine_scores(cum, f(3 * 2.0 ** -10), 'product'))
        scale += e
    assert scale < -126 and 1 <= cum[0] < 2


def test_what_beams_is_taken_as():
    """2.0 counts as 2 (the device receives an int); True, 2.5, a string, None, 0 and number of candidates + 1 are all refused with
    the call's own message."""
    g = _model()
    cand = ids(40, 7, 41, 3, 9)
    paths, path_scores, _, _ = g.beam_sessions([ids(1)], 2, beams=2.0, predict_for_item_ids=cand)
    got = g._model.calls[-1]['beams']
    assert got == 2 and type(got) is int and paths.shape == (1, 2, 2) and path_scores.shape == (1, 2)
    for beams in (True, 2.5, 'a', None, 0, 6):
        refused(g, ValueError, r'beams = %r: it must be an integer in \[1, min\(number of candidates = 5, %d\)\]' % (beams, BMAX),
                [ids(1)], 2, beams=beams, predict_for_item_ids=cand)

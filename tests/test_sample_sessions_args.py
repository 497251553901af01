"""GRU4Rec.sample_sessions without a GPU: every refusal happens before the device model (a recording stand-in) is called, what reaches
it is the CSR of g4r_sample_sessions (histories as item indices, per-session exclusion lists sorted and de-duplicated -- the history
among them with no_repeat --, the global bit mask, the hidden state in the device layout) with steps, samples, top_k, temperature,
seed and first_step, the output is [N, samples, steps], and the prediction state is left exactly as it was.  Also here: the
reference sampler of tests/sampling_ref.py checked on its own (chi-square over fixed seeds), and mutant 20's registration."""
import pickle

import numpy as np
import pytest

import sampling_ref as ref
from gru4rec_amd import _native
from gru4rec_amd import build as g4r_build
from test_continue_sessions_args import BASE, XMAX, Recorder, _model as _base_model, assert_same_state, ids, rows_of, state


class SampleRecorder(Recorder):
    """The stand-in with sample_sessions: position (i * samples + j + s) % candidates at [i, j, s], score = that position, and, with
    return_hidden, row q of layer l filled with 100 l + q."""

    def sample_sessions(self, hist_offs, hist_items, item_idx=None, steps=1, samples=1, top_k=None, temperature=1.0, seed=0, first_step=0,
                        no_repeat=True, excl_offs=None, excl_items=None, excl_mask=None, hidden=None, return_hidden=False):
        cp = (lambda a: None if a is None else np.asarray(a).copy())
        self.calls.append(('sample', dict(offs=cp(hist_offs), items=cp(hist_items), item_idx=cp(item_idx), steps=steps, samples=samples,
                                          top_k=top_k, temperature=temperature, seed=seed, first_step=first_step, no_repeat=no_repeat,
                                          excl_offs=cp(excl_offs), excl_items=cp(excl_items), excl_mask=cp(excl_mask),
                                          hidden=None if hidden is None else [np.array(h, copy=True) for h in hidden],
                                          return_hidden=return_hidden)))
        n = len(hist_offs) - 1
        n_sel = self.n_items if item_idx is None else len(item_idx)
        q = np.arange(n * samples).reshape(n, samples, 1)
        cols = ((q + np.arange(steps)[None, None, :]) % n_sel).astype(np.int32)
        scores = cols.astype(np.float32)
        if not return_hidden:
            return cols, scores
        hout = [(100 * l + np.arange(n * samples, dtype=np.float32))[:, None] * np.ones((1, D), dtype=np.float32) for l, D in enumerate(self.layers)]
        return cols, scores, hout


def _model(n_items=300, layers=(64,), final_act='linear'):
    g = _base_model(n_items, layers, final_act)
    g._model = SampleRecorder(n_items, [(D + 3) // 4 * 4 for D in layers])
    return g


def test_what_reaches_the_device_and_the_output_shape():
    g = _model()
    items, scores = g.sample_sessions([ids(5, 6, 5), ids(9), np.array(ids(1, 2))], 4, samples=3, temperature=0.5, top_k=7, seed=2 ** 63 + 5,
                                      first_step=11, exclude=ids(40, 3, 40, 299), exclude_per_row=[ids(9, 8, 9), [], {BASE + 100, BASE + 2}])
    c = g._model.last('sample')[1]
    assert c['offs'].dtype == np.int64 and c['items'].dtype == np.int32
    assert c['offs'].tolist() == [0, 3, 4, 6] and c['items'].tolist() == [5, 6, 5, 9, 1, 2]
    assert c['item_idx'] is None and c['steps'] == 4 and c['samples'] == 3 and c['no_repeat'] is True
    assert c['top_k'] == 7 and type(c['top_k']) is int and c['temperature'] == 0.5 and type(c['temperature']) is float
    assert c['seed'] == 2 ** 63 + 5 and c['first_step'] == 11 and type(c['seed']) is int and type(c['first_step']) is int
    assert c['hidden'] is None and not c['return_hidden']
    # one list per SESSION (the device expands it to the session's draws), the history in it (no_repeat), sorted, no duplicates
    assert c['excl_offs'].dtype == np.int64 and c['excl_items'].dtype == np.int32
    assert rows_of(c['excl_offs'], c['excl_items']) == [[5, 6, 8, 9], [9], [1, 2, 100]]
    mask = c['excl_mask']
    assert len(mask) == (300 + 31) // 32 and mask.dtype == np.uint32
    assert [i for i in range(300) if (mask[i >> 5] >> (i & 31)) & 1] == [3, 40, 299]
    assert items.shape == scores.shape == (3, 3, 4) and scores.dtype == np.float32
    assert items[1].tolist() == [ids(3, 4, 5, 6), ids(4, 5, 6, 7), ids(5, 6, 7, 8)]
    np.testing.assert_array_equal(scores[1, 2], np.array([5, 6, 7, 8], dtype=np.float32))


def test_defaults_and_no_lists_without_no_repeat():
    g = _model()
    items, scores = g.sample_sessions([ids(5, 6), ids(7)], 3, no_repeat=False)
    c = g._model.last('sample')[1]
    assert c['samples'] == 1 and c['top_k'] is None and c['temperature'] == 1.0 and c['seed'] == 0 and c['first_step'] == 0
    assert c['no_repeat'] is False and c['excl_offs'] is None and c['excl_items'] is None and c['excl_mask'] is None
    assert items.shape == scores.shape == (2, 1, 3)
    g.sample_sessions([ids(5, 6), ids(7)], 3)
    c = g._model.last('sample')[1]
    assert rows_of(c['excl_offs'], c['excl_items']) == [[5, 6], [7]] and c['excl_mask'] is None
    # the temperature reaches the device as the float32 value it will be used as
    g.sample_sessions([ids(1)], 1, temperature=0.1)
    assert g._model.last('sample')[1]['temperature'] == float(np.float32(0.1))


def test_candidates_are_item_indices_and_results_item_ids():
    g = _model()
    cand = ids(40, 7, 41, 3, 9)
    items, scores = g.sample_sessions([ids(1)], 2, samples=2, predict_for_item_ids=cand)
    c = g._model.last('sample')[1]
    assert c['item_idx'].tolist() == [40, 7, 41, 3, 9]
    assert items.tolist() == [[ids(40, 7), ids(7, 41)]]


def test_hidden_goes_in_padded_and_comes_back_per_draw():
    g = _model(layers=(62, 8))           # 62 -> 64 device columns; 8 stays
    rng = np.random.RandomState(0)
    H = [rng.randn(2, 62).astype(np.float32), rng.randn(2, 8).astype(np.float32)]
    items, scores, Hn = g.sample_sessions([ids(1), ids(2, 3)], 3, samples=2, hidden=H, return_hidden=True)
    c = g._model.last('sample')[1]
    assert c['return_hidden']
    h0 = c['hidden']
    assert [h.shape for h in h0] == [(2, 64), (2, 8)]
    np.testing.assert_array_equal(h0[0][:, :62], H[0])
    assert not h0[0][:, 62:].any()
    np.testing.assert_array_equal(h0[1], H[1])
    assert [h.shape for h in Hn] == [(2, 2, 62), (2, 2, 8)] and all(h.dtype == np.float32 for h in Hn)
    np.testing.assert_array_equal(Hn[0][:, :, 0], np.array([[0., 1.], [2., 3.]], dtype=np.float32))
    np.testing.assert_array_equal(Hn[1][:, :, 7], np.array([[100., 101.], [102., 103.]], dtype=np.float32))
    assert items.shape == (2, 2, 3)


def _refused(g, exc, match=None, **kw):
    before = state(g)
    kw.setdefault('steps', 2)
    with pytest.raises(exc, match=match):
        g.sample_sessions(**kw)
    assert_same_state(before, state(g))


def test_refusals_happen_before_the_device():
    g = _model()
    g.predict_next_batch(np.array([1, 2]), ids(10, 20), batch=2)
    h = [np.zeros((2, 64), dtype=np.float32)]
    for steps in (0, -1, 2.5, True, None, 'x'):
        _refused(g, ValueError, match='steps', histories=[ids(1)], steps=steps)
    for t in (0, 0.0, -1.0, float('inf'), float('nan'), None, 'x', True, 1e-60, 1e-40, 1e60):
        _refused(g, ValueError, match='continue_sessions', histories=[ids(1)], temperature=t)
    for s in (0, 65, 1.5, True, None, 'x'):
        _refused(g, ValueError, match='samples', histories=[ids(1)], samples=s)
    for seed in (-1, 2 ** 64, 0.5, True, None, 'x'):
        _refused(g, ValueError, match='seed', histories=[ids(1)], seed=seed)
    for fs in (-1, 0.5, True, None, 'x', 2 ** 31 - 2):                                   # 2^31 - 2 + steps = 2 is one too many
        _refused(g, ValueError, match='first_step', histories=[ids(1)], first_step=fs)
    g.sample_sessions([ids(1)], 2, first_step=2 ** 31 - 3, seed=2 ** 64 - 1, samples=64)   # the largest ones pass
    for top_k in (0, 257, 2.5, True, 'x'):
        _refused(g, ValueError, match='top_k', histories=[ids(1)], top_k=top_k)
    _refused(g, ValueError, match='top_k', histories=[ids(1)], top_k=4, predict_for_item_ids=ids(1, 2, 3))
    _refused(g, TypeError, histories=[ids(1)], scan='bf16')                              # the two-stage selection is not offered
    _refused(g, ValueError, histories=[ids(1), []])                                       # an empty history
    _refused(g, ValueError, histories=[])                                                # no session
    _refused(g, KeyError, histories=[ids(1), [BASE + 300]])                               # unknown item id
    _refused(g, KeyError, histories=[ids(1)], predict_for_item_ids=[BASE - 1])
    _refused(g, KeyError, histories=[ids(1)], exclude=[7])
    _refused(g, KeyError, histories=[ids(1)], exclude_per_row=[[7]])
    _refused(g, ValueError, histories=[ids(1), ids(2)], hidden=h + h)                      # layer count
    _refused(g, ValueError, histories=[ids(1), ids(2)], hidden=[np.zeros((3, 64), dtype=np.float32)])     # shape
    _refused(g, ValueError, histories=[ids(1), ids(2)], hidden=[np.zeros((2, 64), dtype=np.float64)])     # dtype
    _refused(g, ValueError, histories=[ids(1), ids(2)], exclude_per_row=[ids(3)])          # one list per session
    g.error_during_train = True
    _refused(g, Exception, histories=[ids(1)])


def test_the_number_of_draws_is_bounded(monkeypatch):
    g = _model()
    # N * samples <= 2^31 - 1: checked on the packed histories' count, before the device (a stand-in for 2^25 + 1 real sessions)
    monkeypatch.setattr(type(g), '_session_inputs', lambda self, histories, hidden: (2 ** 25 + 1, None, None, None, None))
    _refused(g, ValueError, match='N \\* samples', histories=[ids(1)], samples=64)


def test_the_session_refusals_name_the_row_with_k_from_top_k():
    g = _model()
    cand = ids(*range(100, 112))
    hists = [ids(1, 2), ids(100, 3, 101)]
    _refused(g, ValueError, match='duplicate-free', histories=[ids(1)], predict_for_item_ids=ids(40, 7, 40, 3, 9, 11))
    g.sample_sessions([ids(1)], 2, predict_for_item_ids=ids(40, 7, 40, 3, 9, 11), no_repeat=False)
    # row 1 has 10 eligible positions; steps = 6 takes 5 of them: top_k = 5 is the most, and without top_k (k = 1) 10 steps are
    g.sample_sessions(hists, 6, top_k=5, predict_for_item_ids=cand)
    _refused(g, ValueError, match='row 1', histories=hists, steps=7, top_k=5, predict_for_item_ids=cand)
    _refused(g, ValueError, match='row 1', histories=hists, steps=6, top_k=6, predict_for_item_ids=cand)
    g.sample_sessions(hists, 10, predict_for_item_ids=cand)
    _refused(g, ValueError, match='row 1', histories=hists, steps=11, predict_for_item_ids=cand)
    g.sample_sessions(hists, 50, top_k=12, predict_for_item_ids=cand, no_repeat=False)     # nothing is taken without no_repeat
    # the list length: 1014 distinct items listed + steps - 1 = 10 == G4R_EXCLUDE_MAX
    g = _model(n_items=3000)
    hist = ids(*range(XMAX - 10))
    g.sample_sessions([ids(5), hist], 11, samples=2)
    _refused(g, ValueError, match='row 1', histories=[ids(5), hist], steps=12)
    _refused(g, ValueError, match='row 1', histories=[ids(5), hist], steps=11, exclude_per_row=[[], ids(2999)])


def test_the_prediction_state_is_untouched():
    g = _model()
    g.sample_sessions([ids(1, 2)], 3, samples=2)           # before any predict call: no prediction state appears
    assert getattr(g, 'predict', None) is None and getattr(g, '_seen', None) is None
    g.predict_next_batch(np.array([1, 2]), ids(10, 20), batch=2)
    g.recommend_next_batch(np.array([1, 3]), ids(11, 21), k=2, batch=2)
    before = state(g)
    blob = pickle.dumps(g)
    g.sample_sessions([ids(1, 2, 3), ids(4)], 3, samples=4, top_k=3, hidden=[np.ones((2, 64), dtype=np.float32)], return_hidden=True)
    after = state(g)
    assert after[4] == before[4] + 1 and g._model.calls[-1][0] == 'sample'
    assert_same_state(before[:4] + (0,), after[:4] + (0,))
    assert pickle.dumps(g) == blob


def test_the_binding_knows_the_constants_and_the_mutant():
    assert _native.G4R_SAMPLE_MAX == 64 and _native.G4R_STREAM_GUMBEL == ref.STREAM_GUMBEL == 0x47554D42
    assert 20 in g4r_build.MUTANTS and 'step' in g4r_build.MUTANTS[20]


# ---- the reference sampler on its own
def test_the_reference_uniform_is_exact_and_inside_the_open_interval():
    items = np.arange(4096)
    for seed, q, step in ((0, 0, 0), (2 ** 40 + 3, 2 ** 31, 2 ** 31 - 2)):
        u = ref.uniform64(seed, q, step, items)
        assert u.min() >= 2.0 ** -24 and u.max() <= 1 - 2.0 ** -24
        np.testing.assert_array_equal(u.astype(np.float32).astype(np.float64), u)          # fp32 holds every one exactly
        g = ref.g64(seed, q, step, items)
        assert np.isfinite(g).all() and g.min() > -2.83 and g.max() < 16.64
    # words and lanes: item 4 w + e is lane e of call w
    a = ref.uniform64(7, 1, 2, np.arange(8))
    b = ref.uniform64(7, 1, 2, np.array([4, 5, 6, 7, 0, 1, 2, 3]))
    np.testing.assert_array_equal(a[4:], b[:4])
    np.testing.assert_array_equal(a[:4], b[4:])
    assert len(set(a.tolist())) == 8
    # the step, the row and both key words matter
    base = ref.uniform64(7, 1, 2, np.arange(64))
    for other in (ref.uniform64(7, 1, 3, np.arange(64)), ref.uniform64(7, 2, 2, np.arange(64)), ref.uniform64(8, 1, 2, np.arange(64)),
                  ref.uniform64(7 + 2 ** 32, 1, 2, np.arange(64))):
        assert (other != base).sum() >= 60


def test_the_selection_rule():
    z = np.array([1.0, 3.0, 3.0, np.nan, -0.0, 0.0, 2.0], dtype=np.float32)
    on = np.ones(7, dtype=bool)
    assert ref.order(z, on).tolist() == [1, 2, 6, 0, 4, 5, 3]
    g0 = np.zeros(7, dtype=np.float32)
    assert ref.choose(z, g0, 1.0, on) == 1
    off = on.copy()
    off[1] = False
    assert ref.choose(z, g0, 1.0, off) == 2
    g = np.array([0, 0, 0, 0, 0, 0, 5], dtype=np.float32)
    assert ref.choose(z, g, 1.0, on) == 6 and ref.choose(z, g, 1.0, on, top_k=2) == 1 and ref.choose(z, g, 1.0, on, top_k=3) == 6
    assert ref.choose(z, g, np.float32(8.0), on) == 1                                      # 24 against 16 + 5


@pytest.mark.parametrize('seed', [1, 2 ** 33 + 9])
def test_the_reference_sampler_draws_from_the_softmax(seed):
    """4,096 draws over 8 items against softmax(z): chi-square with 7 degrees of freedom, refused above 24.32 (p = 0.001)."""
    z = np.array([0.0, 1.0, -1.0, 0.5, 2.0, -2.0, 1.5, 0.25], dtype=np.float32)
    counts = ref.sample_counts(z, 4096, seed)
    assert counts.sum() == 4096
    chi = ref.chi_square(counts, ref.softmax64(z))
    print('seed %d: counts %s chi-square %.2f' % (seed, counts.tolist(), chi))
    assert chi <= 24.32
    # temperature 2: the draws follow softmax(z / 2)
    chi2 = ref.chi_square(ref.sample_counts(z, 4096, seed, inv_t=0.5, step=1), ref.softmax64(z.astype(np.float64) / 2))
    print('T = 2: chi-square %.2f' % chi2)
    assert chi2 <= 24.32

"""The prediction forward (g4r_predict_begin / _hidden / _step, g4r_rank_targets) against the float64 oracle, at the shapes the kernels are
written around.  Needs an MI355X.

Every other inference test compares a feature with predict_step itself ("bit for bit"), so predict_step is what those tests trust.
Its kernels: k_gru_p1<32,256> / k_gru_p1<64,256> and k_gru_p2 in both geometries with train = 0 (their own argument block,
GruFwdPredict), k_score_all<32,false>, k_softmax_rows, k_zero_rows, k_gather_rows.  What the older tests leave out and this file runs:

  widths        wide layers (D >= 256: the 64-column phase-1 tile) up to the largest g4r_create accepts, 3-8 K chunks of 256 in k_gru_p1,
                a ragged last column tile (3 D = 780), D = 512 in both k_gru_p2 geometries;
  input widths  IN != D with the chunk boundary inside the hidden part (100 + 300) and inside the input part (300 + 100), a layer
                narrower than one MFMA tile (4 + 8), one-hot input at D = 36 and at 3 D = 1020, a narrow layer under and above a
                512 one, a one-hot layer under a wide one;
  rows          prediction batches of 1, 32, 33, 128, 129 and 257 rows (k_score_all's row tile is 128: blockIdx.y >= 1), and calls
                with fewer rows than the batch: the rows that are not stepped keep their state;
  batch size    the same five sessions alone and as rows 0-4 of a 257-row batch: the same score BITS;
  candidates    lists of 1 / 31 / 32 / 33 columns (ldo rounding, partial 32-column tiles), one item forty times, every final activation,
                softmax rows shorter than k_softmax_rows' 256 threads, softmax_logit (prediction treats it as softmax), scores that
                overflow a naive exp (By drawn from +-60);
  maintenance   a zero_mask shorter than the batch, keep_rows unsorted and shorter than the batch, both branches of g4r_predict_begin;
  ranks         g4r_rank_targets on rows past the first 128-row score tile, with relu's exact ties.

A case is a list of operations (begin / step / zero / keep) played on three states: the fp32 oracle, its float64 twin on the same fp32
weights, and the device.  The standard case is three steps over all 301 items (an n_sel that is no multiple of 4 or 32) from a zero state,
then one over 77 unsorted items that hold item 0, item I - 1 and one duplicate.  No debug key exposes the prediction state, so the state
after a step is checked through the next step's scores.  Where a case depends on a kernel selection (k_gru_p2's geometry per layer,
debug keys `deep_geo` / `kernels`) it is asserted against literals first; k_gru_p1's tile follows from D alone (wide_layer: D >= 256).

The bound comes from the reference alone: d = max |s32 - s64| / max |s64| over a step's score matrix (probabilities for the softmax
names) of the two oracles, measured on the CPU for every case and recorded per family below (profiles/predict_parity.md).  Each test
asserts that its own d stays within its family's constant, and that the device stays within 4 x that constant of the twin, relative to
the matrix's largest entry (the factor test_gpu_hidden_act.py gives the MFMA chain's other summation order).  The bit-for-bit case and
the n_sel = 1 softmax check are exact.

tests/test_gpu_mutation.py: build 34 (k_score_all drops By past the first row tile) and build 35 (k_gru_p1 at prediction stops after
two K chunks) must turn named cases here red and leave the older prediction tests green."""
import numpy as np
import pytest

from test_gpu_hidden_act import _env, float64_twin
from test_gpu_parity import close_rel, make_pair, report

pytestmark = pytest.mark.gpu

I_ITEMS = 301
TRAIN_B = 24          # the model's training batch: k_gru_p2's geometry is chosen from it, not from the prediction batch
ML = 8                # G4R_MAX_LAYERS (`kernels`: 4 ML per-layer values, then 12 scalars)
SWITCHES = ('G4R_NO_LEAN', 'G4R_WIDE2', 'G4R_P2_GEO', 'G4R_BA_GEO')
# largest d = max |s32 - s64| / max |s64| of the fp32 oracle against the float64 oracle over the steps of a family's cases (CPU run of
# both oracles: profiles/predict_parity.md names the case behind each).  The device's bound is FACTOR x the constant.  The By = +-60
# models have a constant of their own: scores of 60 carry fp32 rounding of 60 * 2^-24 into the exponent, eight times the
# distance of the other candidate cases, which keep the tighter bound
ORACLE_DIST = {'widths': 5.630e-7, 'inputs': 5.412e-7, 'rows': 2.588e-7, 'candidates': 2.362e-7, 'candidates_by60': 1.860e-6,
               'maintenance': 4.245e-7}
FACTOR = 4.0


# ---------------------------------------------------------------------------------------------------------------- the three states
class RefState:
    """g4r_predict_begin / _hidden / _step on an oracle: the state is [batch, D] per layer, a step of `rows` rows reads and writes
    the first `rows` rows only, the others keep theirs."""

    def __init__(self, o):
        self.o, self.H = o, None

    def begin(self, pb):
        self.H = [np.zeros((pb, D), dtype=self.o.dtype) for D in self.o.layers]

    def step(self, in_idx, sel=None):
        M = len(in_idx)
        s, new = self.o.predict_step([h[:M] for h in self.H], in_idx, sel)
        for h, n in zip(self.H, new):
            h[:M] = n
        return np.asarray(s)

    def zero(self, mask):
        for h in self.H:
            h[:len(mask)][np.asarray(mask, dtype=bool)] = 0      # rows past the mask keep their state

    def keep(self, rows):
        for i, h in enumerate(self.H):
            n = np.zeros_like(h)                                    # rows past the list start from zero
            n[:len(rows)] = h[np.asarray(rows, dtype=np.int64)]
            self.H[i] = n


class DevState:
    def __init__(self, m):
        self.m = m

    def begin(self, pb):
        self.m.predict_begin(pb)

    def step(self, in_idx, sel=None):
        return self.m.predict_step(in_idx, sel)

    def zero(self, mask):
        self.m.predict_hidden(zero_mask=np.asarray(mask, dtype=np.uint8))

    def keep(self, rows):
        self.m.predict_hidden(keep_rows=np.asarray(rows, dtype=np.int32))


def play(state, ops):
    """The operations in order; the score matrix of every step."""
    out = []
    for op in ops:
        r = getattr(state, op[0])(*op[1:])
        if op[0] == 'step':
            out.append(r)
    return out


def subset77(rng, I=I_ITEMS):
    """77 unsorted candidates that hold item 0, item I - 1 and one item twice."""
    p = rng.permutation(np.arange(1, I - 1))[:74]
    sel = np.concatenate([p[:30], [0], p[30:60], [I - 1], p[60:], [p[10]]]).astype(np.int32)
    assert len(sel) == 77 and len(np.unique(sel)) == 76 and sel.min() == 0 and sel.max() == I - 1 and (np.diff(sel) < 0).any()
    return sel


def standard_ops(pb, seed=23, I=I_ITEMS):
    rng = np.random.RandomState(seed)
    ops = [('begin', pb)]
    for _ in range(3):
        ops.append(('step', rng.randint(0, I, size=pb).astype(np.int32)))
    sel = subset77(rng, I)
    ops.append(('step', rng.randint(0, I, size=pb).astype(np.int32), sel))
    return ops


# ---------------------------------------------------------------------------------------------------------------- model and comparison
def make_trio(layers, geo=None, by_range=None, seed=3, **kw):
    """(fp32 oracle, float64 twin, device model) on the same fp32 weights; Bh and By carry random values (make_pair).  geo: G4R_P2_GEO,
    set around model creation only.  by_range: By drawn uniformly from +-by_range instead."""
    kw = dict(dict(loss='bpr-max', final_act='linear'), layers=tuple(layers), **kw)
    if 'embedding' in kw:
        kw['constrained_embedding'] = False
    env = dict.fromkeys(SWITCHES)
    env['G4R_P2_GEO'] = geo
    with _env(**env):
        o, m = make_pair(I_ITEMS, TRAIN_B, 0, store_rows=0, seed=seed, **kw)
    if by_range is not None:
        o.By = np.random.RandomState(seed + 1).uniform(-by_range, by_range, size=I_ITEMS).astype(np.float32)
        m.set_param('By', o.By)
    assert all(np.abs(b).min() > 0 for b in o.Bh) and np.abs(o.By).min() > 0      # a dropped bias shows
    return o, float64_twin(o, I_ITEMS, TRAIN_B, 0, 0, seed, kw), m


def assert_p2_geometry(m, want):
    """k_gru_p2 per layer: 1 = 8 waves x 256-deep chunks (k_gru_p2<512, 256>), 0 = 4 waves (`kernels`: p2_deep + 2 ba_deep per layer;
    `deep_geo`: the same of layer 0)."""
    k = m.get_debug('kernels', 4 * ML + 12)
    got = tuple(int(k[2 * ML + l]) & 1 for l in range(len(want)))
    assert got == tuple(want), 'k_gru_p2 geometry per layer %s, expected %s' % (got, tuple(want))
    assert int(m.get_debug('deep_geo', 1)[0]) & 1 == want[0]


def oracle_distance(s32, s64):
    err, scale = float(np.abs(np.asarray(s32, dtype=np.float64) - s64).max()), float(np.abs(s64).max())
    return err / scale if scale > 0 else err


def reference(o, o64, ops, fam, tag):
    """The two oracles over the operations: the float64 scores of every step, after asserting that the fp32 oracle stays within the
    family's recorded distance of them."""
    s32, s64 = play(RefState(o), ops), play(RefState(o64), ops)
    ds = [oracle_distance(a, b) for a, b in zip(s32, s64)]
    report('--- predict edges %s: fp32-vs-float64 oracle distance per step %s (family %s: %.2e)' % (
        tag, ' '.join('%.3e' % d for d in ds), fam, ORACLE_DIST[fam]))
    assert all(np.isfinite(s).all() for s in s64)
    assert max(ds) <= 1.001 * ORACLE_DIST[fam], 'the oracles are %.3e apart: ORACLE_DIST[%r] no longer is their largest distance' % (max(ds), fam)
    return s64


def compare(o, o64, m, ops, fam, tag, errs):
    """Reference first, then the device: every step's scores within FACTOR x the family's distance of the float64 twin's, relative to
    the matrix's largest entry.  Report lines `<tag> s<step>`.  Returns (device scores, float64 scores)."""
    s64 = reference(o, o64, ops, fam, tag)
    got = play(DevState(m), ops)
    assert len(got) == len(s64)
    for i, (g, w) in enumerate(zip(got, s64)):
        assert g.shape == w.shape, (tag, i, g.shape, w.shape)
        close_rel('%s s%d' % (tag, i), g, w, 0.0, FACTOR * ORACLE_DIST[fam], errs)
    return got, s64


# ---------------------------------------------------------------------------------------------------------------- 1. widths
# name: (layers, G4R_P2_GEO, k_gru_p2 geometry per layer).  K = 2 D in chunks of 256: 520 = 2 chunks + 8 columns, 640, 1024, 1536, 2048
WIDTHS = {'d260': ((260,), None, (0,)), 'd320': ((320,), None, (0,)), 'd512_geo0': ((512,), 0, (0,)), 'd512_geo1': ((512,), 1, (1,)),
          'd768': ((768,), None, (1,)), 'd1024': ((1024,), None, (1,))}


@pytest.mark.parametrize('name', sorted(WIDTHS))
def test_widths(name):
    """Constrained embedding, linear scores, 37 rows.  Report lines `w <name> s<step>`."""
    layers, geo, deep = WIDTHS[name]
    o, o64, m = make_trio(layers, geo=geo, constrained_embedding=True)
    try:
        assert_p2_geometry(m, deep)
        errs = []
        compare(o, o64, m, standard_ops(37), 'widths', 'w ' + name, errs)
        assert not errs, errs
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------------- 2. input widths
# name: (model arguments, k_gru_p2 geometry per layer).  No embedding argument and not constrained: one-hot input
INPUTS = {'e100_d300': (dict(layers=(300,), embedding=100), (0,)),            # K = 400: the chunk boundary falls inside H
          'e300_d100': (dict(layers=(100,), embedding=300), (0,)),            # IN > D: the boundary falls inside y
          'e4_d8': (dict(layers=(8,), embedding=4), (0,)),
          'onehot36': (dict(layers=(36,)), (0,)),
          'onehot340': (dict(layers=(340,)), (0,)),                          # 3 D = 1020, just under the one-hot limit of 1024
          's36_512': (dict(layers=(36, 512), constrained_embedding=True), (0, 1)),      # K = 512 + 36 and 36 + 512
          's512_36': (dict(layers=(512, 36), constrained_embedding=True), (1, 0)),      # K = 36 + 512 and 512 + 36
          'onehot132_260_64': (dict(layers=(132, 260, 64)), (0, 0, 0))}


@pytest.mark.parametrize('name', sorted(INPUTS))
def test_input_widths(name):
    """Linear scores, 37 rows.  Report lines `i <name> s<step>`."""
    kw, deep = INPUTS[name]
    o, o64, m = make_trio(**kw)
    try:
        assert o.onehot == name.startswith('onehot')
        assert_p2_geometry(m, deep)
        errs = []
        compare(o, o64, m, standard_ops(37), 'inputs', 'i ' + name, errs)
        assert not errs, errs
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------------- 3. rows
ROWS_KW = dict(layers=(64,), constrained_embedding=True, final_act='elu-0.5')


@pytest.mark.parametrize('pb', [1, 32, 33, 128, 129, 257])
def test_rows(pb):
    """Every row of a prediction batch of pb rows (k_gru_p1 / k_gru_p2 row tiles of 32, k_score_all's of 128).  Report lines `r <pb> s<step>`."""
    o, o64, m = make_trio(**ROWS_KW)
    try:
        assert_p2_geometry(m, (0,))
        errs = []
        got, _ = compare(o, o64, m, standard_ops(pb), 'rows', 'r %d' % pb, errs)
        assert all(g.shape[0] == pb for g in got)
        assert not errs, errs
    finally:
        m.close()


def test_fewer_rows_than_the_batch():
    """predict_begin(200), then steps of 200, 131, 5 and 200 rows: a step leaves the rows it does not take as they are.  In the last step
    rows 5 .. 130 go on from their state after the second step and rows 131 .. 199 from theirs after the first.  Report lines `r seq s<step>`
    and `r seq last rows 5+` (the rows the third step left out)."""
    o, o64, m = make_trio(**ROWS_KW)
    try:
        assert_p2_geometry(m, (0,))
        rng = np.random.RandomState(29)
        ops = [('begin', 200)] + [('step', rng.randint(0, I_ITEMS, size=n).astype(np.int32)) for n in (200, 131, 5, 200)]
        errs = []
        got, s64 = compare(o, o64, m, ops, 'rows', 'r seq', errs)
        assert [g.shape[0] for g in got] == [200, 131, 5, 200]
        close_rel('r seq last rows 5+', got[3][5:], s64[3][5:], 0.0, FACTOR * ORACLE_DIST['rows'], errs)
        assert not errs, errs
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------------- 4. batch size
@pytest.mark.parametrize('D,deep', [(64, 0), (512, 1)])
def test_scores_do_not_depend_on_the_batch_size(D, deep):
    """Five sessions stepped three times alone (predict_begin(5)) and as rows 0-4 of a 257-row batch: identical score bits (the fp32
    summation order of the hidden state and of the scores must not depend on the evaluation batch size).  D = 512 in the model's
    default k_gru_p2 geometry."""
    o, _, m = make_trio(layers=(D,), constrained_embedding=True)
    try:
        assert_p2_geometry(m, (deep,))
        rng = np.random.RandomState(31)
        big = [rng.randint(0, I_ITEMS, size=257).astype(np.int32) for _ in range(3)]
        m.predict_begin(5)
        alone = [m.predict_step(x[:5]).copy() for x in big]
        m.predict_begin(257)
        batch = [m.predict_step(x).copy() for x in big]
        assert np.isfinite(alone[2]).all() and len(np.unique(alone[2])) > 1000      # (three different steps of five different rows)
        for a, b in zip(alone, batch):
            assert a.shape == (5, I_ITEMS) and b.shape == (257, I_ITEMS)
            np.testing.assert_array_equal(a.view(np.uint32), b[:5].view(np.uint32))
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------------- 5. candidates
FINAL_ACTS = ['linear', 'relu', 'tanh', 'elu-0.5', 'softmax', 'softmax_logit']
SOFTMAX = ('softmax', 'softmax_logit')
CAND_ROWS = 130       # a second 128-row score tile


def candidate_ops(item, pb=CAND_ROWS):
    """The standard case, then lists of 1 / 31 / 32 / 33 unsorted items and `item` forty times.  Returns (ops, n_sel per step)."""
    ops = standard_ops(pb)
    rng = np.random.RandomState(37)
    lists = [rng.permutation(I_ITEMS)[:n].astype(np.int32) for n in (1, 31, 32, 33)] + [np.full(40, item, dtype=np.int32)]
    for sel in lists:
        ops.append(('step', rng.randint(0, I_ITEMS, size=pb).astype(np.int32), sel))
    return ops, [I_ITEMS] * 3 + [77, 1, 31, 32, 33, 40]


@pytest.mark.parametrize('fa', FINAL_ACTS)
def test_candidate_lists(fa):
    """D = 36, 130 rows.  Report lines `c <final_act> s<step>`: steps 0-2 all items, 3 the 77-item subset, 4-7 n_sel = 1 / 31 / 32 / 33,
    8 one item forty times (the item of the largest bias)."""
    o, o64, m = make_trio(layers=(36,), constrained_embedding=True, final_act=fa)
    try:
        assert_p2_geometry(m, (0,))
        ops, n_sel = candidate_ops(int(np.argmax(o.By)))      # (the largest bias: relu leaves its scores mostly positive)
        errs = []
        got, s64 = compare(o, o64, m, ops, 'candidates', 'c ' + fa, errs)
        assert [g.shape for g in got] == [(CAND_ROWS, n) for n in n_sel]
        assert (got[8] == got[8][:, :1]).all()      # one item forty times: forty equal scores
        if fa in SOFTMAX:
            assert (got[4] == 1.0).all()             # a list of one candidate: its probability is exactly 1
            for g in got:
                assert np.abs(g.astype(np.float64).sum(axis=1) - 1.0).max() <= 1e-5
        assert not errs, errs
    finally:
        m.close()


@pytest.mark.parametrize('fa', SOFTMAX)
def test_softmax_of_scores_that_overflow_a_naive_exp(fa):
    """By drawn from +-60: the scores of a row spread over more than 88.7 = log(FLT_MAX), exp(s) alone would be inf.  Report lines
    `c60 <final_act> s<step>`."""
    o, o64, m = make_trio(layers=(36,), constrained_embedding=True, final_act=fa, by_range=60.0)
    try:
        assert_p2_geometry(m, (0,))
        assert o.By.max() - o.By.min() > 100.0
        errs = []
        got, _ = compare(o, o64, m, standard_ops(CAND_ROWS), 'candidates_by60', 'c60 ' + fa, errs)
        for g in got:
            assert np.isfinite(g).all() and np.abs(g.astype(np.float64).sum(axis=1) - 1.0).max() <= 1e-5
        assert not errs, errs
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------------- 6. maintenance
def test_hidden_state_maintenance():
    """Layers (36, 132), 40 rows: two steps, a zero_mask of 25 bytes (rows 25 .. 39 keep their state), keep_rows as an unsorted selection of
    31 rows (rows 31 .. 39 then score as fresh sessions), predict_begin(40) again (the memset branch: the state is zero again),
    predict_begin(33) then predict_begin(40) (the reallocation branch); a step after each.  Report lines `m s<step>`."""
    o, o64, m = make_trio(layers=(36, 132), constrained_embedding=True)
    try:
        assert_p2_geometry(m, (0, 0))
        rng = np.random.RandomState(41)
        items = lambda n: rng.randint(0, I_ITEMS, size=n).astype(np.int32)
        mask = (rng.rand(25) < 0.4).astype(np.uint8)
        keep = rng.permutation(40)[:31].astype(np.int32)
        assert 0 < mask.sum() < 25 and (np.diff(keep) < 0).any() and keep.max() >= 31
        ops = [('begin', 40), ('step', items(40)), ('step', items(40)),
               ('zero', mask), ('step', items(40)),
               ('keep', keep), ('step', items(40)),
               ('begin', 40), ('step', items(40)),
               ('begin', 33), ('step', items(33)),
               ('begin', 40), ('step', items(40))]
        errs = []
        got, s64 = compare(o, o64, m, ops, 'maintenance', 'm', errs)
        # the reference side says what the construction says: rows 31 .. 39 of the step after keep_rows, and every row of the steps after
        # a predict_begin, are fresh sessions -- the scores of a one-row batch of the same item from a zero state
        fresh = RefState(o64)
        for s, n0 in ((3, 31), (4, 0), (6, 0)):
            in_idx = [op for op in ops if op[0] == 'step'][s][1]
            for r in (n0, 39):
                fresh.begin(1)
                np.testing.assert_allclose(fresh.step(in_idx[r:r + 1])[0], s64[s][r], rtol=1e-12, atol=1e-14)
        close_rel('m s3 rows 31+', got[3][31:], s64[3][31:], 0.0, FACTOR * ORACLE_DIST['maintenance'], errs)
        assert not errs, errs
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------------- 7. ranks
def test_ranks_past_the_first_score_tile():
    """g4r_rank_targets after one all-items step of the relu model at 130 rows, in the three deterministic modes, against NumPy counts on
    the returned scores.  relu makes exact ties (zeros); every second target is a zero score where the row has one."""
    o, _, m = make_trio(layers=(36,), constrained_embedding=True, final_act='relu')
    try:
        rng = np.random.RandomState(43)
        m.predict_begin(CAND_ROWS)
        got = m.predict_step(rng.randint(0, I_ITEMS, size=CAND_ROWS).astype(np.int32))
        tgt = rng.randint(0, I_ITEMS, size=CAND_ROWS).astype(np.int32)
        for r in range(0, CAND_ROWS, 2):
            z = np.flatnonzero(got[r] == 0)
            if len(z):
                tgt[r] = z[len(z) // 2]
        t = got[np.arange(CAND_ROWS), tgt][:, None]
        gt, eq = (got > t).sum(axis=1), (got == t).sum(axis=1)
        assert (eq[128:] > 1).any() and (eq[:128] > 1).any() and (eq == 1).any()      # ties on both sides of row 128, and rows without
        for mode, ref in (('standard', gt + 1), ('conservative', gt + eq), ('median', gt + 0.5 * (eq - 1) + 1)):
            np.testing.assert_array_equal(m.rank_targets(tgt, 0, mode), ref.astype(np.float32))
    finally:
        m.close()

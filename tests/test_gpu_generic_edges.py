"""Oracle parity of the generic optimizer path (g4r_update_kernels.cuh: k_grad_sqsum / k_grad_clip, dense_apply_elem, opt_rule,
k_sparse_update_generic<1|2|4>) on the shapes its geometry is written around: both sides of the lane-group edges (rows of 64 / 68
and 128 / 132 floats: LW 16 / 32 / 64 with RPI 4 / 2 / 1 occurrences per load) and of the chunk edges (256 / 260 and 512 / 516
floats: one, two, four float4 chunks per lane, the last with the LATE row loads), separate tables (an embedding wider and narrower
than the layer, one-hot input) with one id owned once per table in the same step, the duplicate-weighted terms (fn * reg,
fn * mom * w, Adam's fn * out), Adam's step counters on rows that are touched in some steps only, both branches of the clip factor
and a dense gradient longer than one grid of k_grad_sqsum, items with more than 64 and more than 128 earlier occurrences in a step
(second and third pass of the owner walk), and graph replay.

Every case first asserts the selection (get_debug('generic') == 1 and k.chunks of get_debug('kernels')), so that a dispatch change
turns it red instead of quietly testing something else.  Then a few steps with a ragged tail (M ends inside a tile, a last step
with M = 5, items repeated between inputs, targets and negatives, a skewed support: many items occur 2-20 times per step, so the
walk's NB * RPI row trips end in partial trips) against OracleGRU4Rec: per-step cost rtol 5e-4 + atol 5e-6, and EVERYTHING the
optimizer keeps by compare_params (parameters as updates, acc_*, acc2_*, cnt_* exactly, vel_*).

Hot items (test_hot_items): the float32 oracle adds an item's ~150 per-occurrence increments to the parameter one by one and is
itself off by more than one lost occurrence would be for some optimizers, so the rows of the hot items are compared against the
FLOAT64 oracle (same weights, plan and sample store); the bound of a hot row is the larger of compare_params' own bound and twice
the float32 oracle's measured distance from the float64 one on that row (both are fp32 roundings of the same sums in different
orders) -- see _hot_rows and the figures in test_hot_items' docstring."""
import copy

import numpy as np
import pytest

from test_gpu_parity import close, compare_params, kink_twin, make_pair, oracle_steps, random_plan, report

pytestmark = pytest.mark.gpu

NKEY = 4 * 8 + 12      # get_debug('kernels'): 4 x G4R_MAX_LAYERS per-layer slots, then 12 choices; [.. + 8] = update, [.. + 9] = chunks
UP_SPLIT = 2

OPT = {
    'rmsprop': dict(adapt='rmsprop', adapt_params=(0.9,), learning_rate=0.01),
    'adadelta': dict(adapt='adadelta', adapt_params=(0.95,), learning_rate=1.0),
    'adam': dict(adapt='adam', adapt_params=(0.9, 0.999), learning_rate=0.001),
    'sgd_mom': dict(adapt=None, learning_rate=0.5, momentum=0.2),
    'adagrad_cap': dict(grad_cap=0.01, learning_rate=0.05),      # (below every step's norm at these shapes: asserted in the case)
}
BPR = dict(loss='bpr-max', final_act='elu-0.5', bpreg=0.5)
XE = dict(loss='cross-entropy', final_act='softmax')


def chunks_of(width):
    return 1 if width <= 256 else (2 if width <= 512 else 4)


def selection(m):
    k = m.get_debug('kernels', (NKEY,))
    return int(m.get_debug('generic', (1,))[0]), int(k[4 * 8 + 8]), int(k[4 * 8 + 9])


def skewed_support(I, seed=1):
    """A Zipf-like head over a flat tail: with 150-300 negatives a few dozen items occur 2-20 times per step, none 64 times."""
    return 4000.0 / (1.0 + np.arange(I)) ** 1.5 + np.random.RandomState(seed).randint(1, 4, size=I)


def ragged_plan(o, I, B, T, seed=77, items=None):
    plan = random_plan(I, B, T, seed=seed, tail=True)
    if items is not None:      # inputs drawn from `items` only
        plan['in_idx'] = np.random.RandomState(seed + 1).choice(items, size=(T, B)).astype(np.int32)
    plan['M'][:] = B
    plan['M'][T // 2:] = B - 37 if B > 48 else B - 3      # ends inside a 16-row and inside a 32-row tile
    plan['M'][-1] = 5
    if items is None:
        plan['in_idx'][:, :6] = o.ST[0][:6]      # items repeated between input, targets and negatives
    plan['out_idx'][:, 6:12] = plan['in_idx'][:, :6]
    return plan


def id_lists(o, plan, t):
    """The occurrence list of step t as the update kernels see it: X (B entries, -1 past M) | Y (B, -1 past M) | samples."""
    B, M = o.batch_size, int(plan['M'][t])
    x = np.full(B, -1, dtype=np.int64)
    y = np.full(B, -1, dtype=np.int64)
    x[:M], y[:M] = plan['in_idx'][t][:M], plan['out_idx'][t][:M]
    assert t < o.generate_length      # (no refill inside the run: row t of the store is step t's negatives)
    return np.concatenate([x, y, np.asarray(o.ST[t], dtype=np.int64)])


def f64_twin(o):
    """The (not yet stepped) oracle in float64: same weights, popularity table and sample store."""
    t = copy.deepcopy(o)
    t.dtype = np.dtype(np.float64)
    t._cast()
    t._init_opt_state()
    return t


def _run(tag, I, B, ns, T, width, items=None, support=None, check_lists=None, check=None, hot=None, seed=77, **kw):
    """width: the widest gathered row (floats) -- k.chunks is asserted from it.  check_lists(lists): assertions on the T occurrence
    lists.  check(o, m, plan, rec): extra assertions after the last step (rec: per-step gradient norm / clipped).  hot: see
    _hot_rows."""
    o, m = make_pair(I, B, ns, store_rows=max(T, 8), support=skewed_support(I) if support is None else support, **kw)
    try:
        sel = selection(m)
        assert sel == (1, UP_SPLIT, chunks_of(width)), '%s: (generic, update, chunks) = %s, expected %s' % (tag, sel, (1, UP_SPLIT, chunks_of(width)))
        twin = kink_twin(o)
        o64 = f64_twin(o) if hot else None
        plan = ragged_plan(o, I, B, T, seed=seed, items=items)
        lists = [id_lists(o, plan, t) for t in range(T)]
        if check_lists is not None:
            check_lists(lists)
        m.set_plan(plan)
        rec = []
        want_cost, kink = oracle_steps(o, plan, T, twin=twin, record=rec)
        if o64 is not None:
            oracle_steps(o64, plan, T)
        m.train_steps(0, T)
        errs = []
        report('--- generic %s (generic, update, chunks = %s)' % (tag, sel))
        close('loss curve', m.get_losses(0, T), np.array(want_cost), atol=5e-6, rtol=5e-4, errs=errs)
        compare_params(o, m, errs, tag, Mrows=int(plan['M'][-1]), skip_items=kink, twin=twin if kink else None, leave_rows=hot or ())
        if hot:
            _hot_rows(o, o64, m, errs, tag, hot, lists)
        if check is not None:
            check(o, m, plan, rec)
        assert not errs, errs
    finally:
        m.close()


def moderate_repeats(lists):
    """Many items 2-20 times in a step, none more than 64 times (one pass of the owner walk)."""
    for l in lists[:-1]:
        c = np.bincount(l[l >= 0])
        assert c.max() <= 64 and int(((c >= 2) & (c <= 20)).sum()) >= 10 and c.max() >= 9, (c.max(), int((c >= 2).sum()))


# ------------------------------------------------------------------------------------------------ row-width boundaries
WIDTHS = [(64, 'rmsprop'), (64, 'adadelta'), (64, 'adam'), (64, 'sgd_mom'), (64, 'adagrad_cap'),          # LW 16, RPI 4
          (68, 'adam'), (68, 'sgd_mom'), (128, 'rmsprop'), (128, 'adadelta'), (128, 'adagrad_cap'),       # LW 32, RPI 2
          (132, 'rmsprop'), (132, 'adam'), (256, 'adadelta'), (256, 'sgd_mom'), (256, 'adagrad_cap'),     # LW 64
          (260, 'rmsprop'), (260, 'adadelta'), (260, 'adam'), (260, 'sgd_mom'), (260, 'adagrad_cap'),     # two chunks per lane
          (512, 'adam'), (512, 'sgd_mom'),
          (516, 'rmsprop'), (516, 'adadelta'), (516, 'adam'), (516, 'sgd_mom'), (516, 'adagrad_cap')]     # four chunks, LATE loads


def _all_clipped(o, m, plan, rec):
    assert all(r['clipped'] for r in rec), [r['grad_norm'] for r in rec]


@pytest.mark.parametrize('D,opt', WIDTHS)
def test_row_width(D, opt):
    """Constrained embedding, rows of D floats, B = 33, 200 negatives: both sides of the LW 16 / 32, 32 / 64, chunks 1 / 2 and 2 / 4
    edges; every optimizer at every lane-group width and chunk count."""
    _run('%s D=%d' % (opt, D), I=700, B=33, ns=200, T=5, width=D, check_lists=moderate_repeats,
         check=_all_clipped if opt == 'adagrad_cap' else None, constrained_embedding=True, layers=(D,), **BPR, **OPT[opt])


# ------------------------------------------------------------------------------------------------ separate tables
SEP_HOT = np.arange(8)      # the head of the support: the inputs come from these ids only, the negatives mostly


def _owned_in_both_tables(lists):
    B = 33
    for l in lists:
        x, ys = l[:B], l[B:]
        both = [i for i in SEP_HOT if (x == i).any() and (ys == i).any()]
        assert both, 'no id occurs in the X part and in the Y | samples part of one step'


@pytest.mark.parametrize('opt', ['adam', 'adadelta'])
@pytest.mark.parametrize('name,width,kw', [
    ('emb516_D64', 516, dict(constrained_embedding=False, embedding=516, layers=(64,))),
    ('emb8_D260', 260, dict(constrained_embedding=False, embedding=8, layers=(260,))),
    ('onehot_D100', 300, dict(layers=(100,))),
    ('onehot_D176', 528, dict(layers=(176,)))])
def test_separate_tables(name, width, kw, opt):
    """Two tables (E or the one-hot Wx[0] for the inputs, Wy for targets and negatives) of different row widths: the same id is
    owned once per table in the same step, each owner walks the occurrences of its own table only (same_table)."""
    _run('%s %s' % (opt, name), I=700, B=33, ns=200, T=5, width=width, items=SEP_HOT, check_lists=_owned_in_both_tables, **XE, **kw, **OPT[opt])


# ------------------------------------------------------------------------------------------------ duplicate-weighted terms
@pytest.mark.parametrize('D', [64, 516])
@pytest.mark.parametrize('opt', ['rmsprop', 'adam'])
def test_momentum_with_l2_on_duplicates(opt, D):
    """momentum and lmbd > 0 together: an item with n occurrences takes n * mom * v0 and n * lr * lmbd * p0 (and Adam n * out)."""
    kw = dict(OPT[opt], momentum=0.3, lmbd=0.01)
    _run('%s mom+l2 D=%d' % (opt, D), I=700, B=33, ns=200, T=5, width=D, check_lists=moderate_repeats, constrained_embedding=True,
         layers=(D,), **BPR, **kw)


# ------------------------------------------------------------------------------------------------ Adam's step counters
def test_adam_counters_of_rows_touched_in_two_steps_only():
    """Items 680-699 carry (almost) no sampling mass and occur as inputs / targets of steps 0 and 3 only: their counters are 2 after
    five steps, the rows of the head 5.  Exact: no tolerance."""
    I, B, T, D = 700, 33, 5, 68
    rare = np.arange(680, 700)
    support = skewed_support(I)
    support[rare] = 1e-12

    def lists_ok(lists):
        for t, l in enumerate(lists):
            assert bool(np.isin(l, rare).any()) == (t in (0, 3)), t

    def check(o, m, plan, rec):
        cw, cb = m.get_param('cnt_Wy', (I, D)), m.get_param('cnt_By', (I,))
        assert (o.cnt['Wy'][rare] == 2).all() and set(np.unique(o.cnt['Wy'])) >= {0.0, 2.0, 5.0}
        np.testing.assert_array_equal(cw, o.cnt['Wy'])
        np.testing.assert_array_equal(cb, o.cnt['By'])

    o, m = make_pair(I, B, 200, store_rows=8, support=support, constrained_embedding=True, layers=(D,), **BPR, **OPT['adam'])
    try:
        assert selection(m) == (1, UP_SPLIT, 1)
        plan = ragged_plan(o, I, B, T)
        rng = np.random.RandomState(5)
        for n in ('in_idx', 'out_idx'):
            plan[n][np.isin(plan[n], rare)] = 3
        plan['M'][:] = [B, B, B - 3, B - 3, 5]
        for t in (0, 3):
            plan['in_idx'][t, 12:22] = rare[:10]
            plan['out_idx'][t, 10:30] = rng.permutation(rare)      # (inside M = 30 of step 3)
        lists_ok([id_lists(o, plan, t) for t in range(T)])
        m.set_plan(plan)
        twin = kink_twin(o)
        want_cost, kink = oracle_steps(o, plan, T, twin=twin)
        m.train_steps(0, T)
        errs = []
        report('--- generic adam counters')
        close('loss curve', m.get_losses(0, T), np.array(want_cost), atol=5e-6, rtol=5e-4, errs=errs)
        compare_params(o, m, errs, 'adam cnt', Mrows=5, skip_items=kink, twin=twin if kink else None)
        check(o, m, plan, None)
        assert not errs, errs
    finally:
        m.close()


# ------------------------------------------------------------------------------------------------ clipping
CLIP_KW = dict(I=700, B=33, ns=200, T=5, width=64, constrained_embedding=True, layers=(64,), **BPR, **OPT['rmsprop'])


@pytest.fixture(scope='module')
def clip_norms():
    """The oracle's own per-step gradient norms of the clipping configuration under a cap that nothing reaches."""
    kw = {k: v for k, v in CLIP_KW.items() if k not in ('I', 'B', 'ns', 'T', 'width')}
    o, m = make_pair(CLIP_KW['I'], CLIP_KW['B'], CLIP_KW['ns'], store_rows=8, support=skewed_support(CLIP_KW['I']), grad_cap=1e30, **kw)
    m.close()
    rec = []
    oracle_steps(o, ragged_plan(o, CLIP_KW['I'], CLIP_KW['B'], CLIP_KW['T']), CLIP_KW['T'], record=rec)
    return [r['grad_norm'] for r in rec]


@pytest.mark.parametrize('which', ['below_all', 'between'])
def test_clip_factor_both_branches(clip_norms, which):
    """Two caps chosen from the oracle's own per-step gradient norms: half the smallest (every step is scaled) and the mean of the
    smallest and the largest (k_grad_clip takes the branch where the factor is 1 in some steps and the one that scales in others)."""
    lo, hi = min(clip_norms), max(clip_norms)
    assert hi > 1.5 * lo, clip_norms
    cap = 0.5 * lo if which == 'below_all' else 0.5 * (lo + hi)

    def check(o, m, plan, rec):
        cl = [r['clipped'] for r in rec]
        report('clip %s: cap %.4e, step norms %s, clipped %s' % (which, cap, ['%.4e' % r['grad_norm'] for r in rec], cl))
        assert all(cl) if which == 'below_all' else (any(cl) and not all(cl)), (cap, rec)

    _run('clip %s' % which, check=check, check_lists=moderate_repeats, grad_cap=float(cap), **CLIP_KW)


def test_clip_norm_over_more_than_one_grid():
    """D = 512, two layers: 3.1 M dense gradients, far more than k_grad_sqsum's G4R_NORM_BLOCKS * 256 = 65536 threads cover in one
    grid-stride trip; the cap scales every step."""
    def check(o, m, plan, rec):
        assert int(m.get_debug('dense_count', (1,))[0]) > 40 * 65536
        assert all(r['clipped'] for r in rec), rec

    _run('clip wide', I=700, B=33, ns=200, T=4, width=512, check=check, constrained_embedding=True, layers=(512, 512), grad_cap=0.01,
         **BPR, **OPT['rmsprop'])


# ------------------------------------------------------------------------------------------------ hot items
HOT_I, HOT_B, HOT_NS, HOT_T = 300, 64, 1000, 6
HOT = (0, 1)
PR, PA, AR, AA = 1e-3, 1e-4, 2e-4, 1e-5      # compare_params' bounds


def hot_support():
    return np.r_[1100.0, 600.0, np.random.RandomState(1).randint(1, 40, size=HOT_I - 2)]


def _hot_lists(lists):
    """Item 0: more than 128 earlier occurrences (three passes of the owner walk), item 1: more than 64 (two), in every full step;
    their positions span more than 256 list entries (the LDS scan takes several 256-entry steps from first_j & ~255)."""
    for l in lists[:-1]:
        p0, p1 = np.flatnonzero(l == 0), np.flatnonzero(l == 1)
        assert len(p0) - 1 > 128 and 128 >= len(p1) - 1 > 64, (len(p0), len(p1))
        assert p0[-1] - p0[0] > 256 and p1[-1] - p1[0] > 256


def _hot_rows(o, o64, m, errs, tag, hot, lists, measured=True):
    """The rows of the hot items of Wy / By and their state against the float64 oracle.  Bound per element: the larger of
    compare_params' own (relative part on the float64 value, absolute part on the float64 tensor's scale) and twice the float32
    oracle's largest distance from the float64 one on that row.  For the parameter rows that bound must stay below a quarter of
    1 / n_occ of the row's largest update element -- one lost occurrence cannot pass; asserted here from the two oracles alone."""
    I, D = o.n_items, o.layers[-1]
    n_occ = {r: max(int((l == r).sum()) for l in lists) for r in hot}
    tens = [('dWy', m.get_param('Wy', (I, D)) - o.init0['Wy'].astype(np.float64), o.Wy - o.init0['Wy'].astype(np.float64),
             o64.Wy - o.init0['Wy'].astype(np.float64), PR, PA, True),
            ('dBy', m.get_param('By', (I,)) - o.init0['By'].astype(np.float64), o.By - o.init0['By'].astype(np.float64),
             o64.By - o.init0['By'].astype(np.float64), PR, PA, True),
            ('acc_Wy', m.get_param('acc_Wy', (I, D)), o.acc['Wy'], o64.acc['Wy'], AR, AA, False),
            ('acc_By', m.get_param('acc_By', (I,)), o.acc['By'], o64.acc['By'], AR, AA, False)]
    if o.adapt in ('adadelta', 'adam'):
        tens += [('acc2_Wy', m.get_param('acc2_Wy', (I, D)), o.acc2['Wy'], o64.acc2['Wy'], AR, AA, False),
                 ('acc2_By', m.get_param('acc2_By', (I,)), o.acc2['By'], o64.acc2['By'], AR, AA, False)]
    if o.momentum > 0:
        tens += [('vel_By', m.get_param('vel_By', (I,)), o.vel['By'], o64.vel['By'], PR, PA, False)]
    for name, got, w32, w64, rel, ab, is_update in tens:
        got, w32, w64 = (np.asarray(x, dtype=np.float64) for x in (got, w32, w64))
        scale = float(np.abs(w64).max())
        floor = 4.0 * float(np.spacing(np.float32(max(np.abs(o64.Wy if name == 'dWy' else o64.By).max(), 1e-30)))) if is_update else 0.0
        for r in hot:
            g, a, b = np.atleast_1d(got[r]), np.atleast_1d(w32[r]), np.atleast_1d(w64[r])
            own = rel * np.abs(b) + ab * scale + floor
            d32 = float(np.abs(a - b).max())
            tol = np.maximum(own, 2.0 * d32) if measured else own
            if is_update:
                top = int(np.abs(b).argmax())
                assert tol[top] < 0.25 * abs(b[top]) / n_occ[r], '%s %s row %d: bound %.3e is not below a quarter of one of %d occurrences of %.3e' % (
                    tag, name, r, tol[top], n_occ[r], abs(b[top]))
            err = np.abs(g - b)
            worst = float((err / np.maximum(tol, 1e-300)).max())
            bad = not np.isfinite(g).all() or worst > 1.0
            report('%-28s max_abs_err %.3e  max|want| %.3e  worst/tol %.3f %s   (hot row %d vs float64; float32 oracle vs float64 %.3e = %.2e of the row, %d occurrences)' % (
                '%s %s hot%d' % (tag, name, r), float(err.max()), float(np.abs(b).max()), worst, 'FAIL' if bad else 'ok', r, d32,
                d32 / max(float(np.abs(b).max()), 1e-300), n_occ[r]))
            if bad:
                errs.append('%s %s hot%d' % (tag, name, r))


HOT_OPT = dict(OPT, sgd_mom=dict(adapt=None, learning_rate=1.0, momentum=0.2))      # (lr: see the docstring of test_hot_items)


@pytest.mark.parametrize('opt', ['rmsprop', 'adadelta', 'adam', 'sgd_mom'])
@pytest.mark.parametrize('D', [40, 300, 516])
def test_hot_items(D, opt):
    """I = 300, B = 64, 1000 negatives drawn with sample_alpha = 1 from a support of (1100, 600, 1..39 ...): items 0 and 1 occur
    ~150 and ~85 times per step.  D = 40: RPI = 4 occurrences per load; D = 300: two chunks; D = 516: four chunks.
    Hot rows against the float64 oracle, bound = max(compare_params' own, 2 x float32-oracle-to-float64 distance of the row), see
    _hot_rows; every other row and tensor by compare_params against the float32 oracle.

    Measured on the CPU (float32 oracle against float64 oracle, six steps, largest element distance of the row as a fraction of the
    row's largest update; item 0 has up to 169 occurrences in a step with the repeated inputs / targets, item 1 up to 93):
                    dWy row 0            dWy row 1            dBy row 0            dBy row 1
      rmsprop   1.5e-5 .. 2.0e-5     7.7e-6 .. 1.2e-5     6.5e-6 .. 3.5e-5     3.9e-7 .. 7.2e-6
      adadelta  4.0e-5 .. 5.5e-5     3.4e-5 .. 7.1e-5     4.1e-6 .. 6.5e-6     2.5e-6 .. 1.0e-5
      adam      3.7e-5 .. 7.7e-5     3.1e-5 .. 4.2e-5     3.8e-6 .. 1.4e-5     3.3e-6 .. 5.5e-6
      sgd_mom   2.5e-5 .. 3.0e-5     2.4e-5 .. 3.4e-5     2.1e-7 .. 1.0e-5     7.3e-8 .. 2.1e-6
    (ranges over D = 40 / 300 / 516; absolute distances 1e-6 .. 7e-6).  Twice these stays below compare_params' own bound
    (1e-3 of the element + 1e-4 of the tensor's largest update), so that bound decides, and it is below a quarter of one
    occurrence (0.25 / 169 = 1.5e-3 of the row's largest update element): _hot_rows asserts both for every row.
    Plain SGD runs at learning rate 1 here: at 0.05 the hot row's whole update is ~1e-4, the float32 oracle adds it as ~150
    increments to a parameter whose spacing is 7.5e-9, and its own error (1.6 % of the update) is more than one lost occurrence;
    at 1 the update is ~0.1 and the same rounding is 3e-5 of it."""
    _run('hot %s D=%d' % (opt, D), I=HOT_I, B=HOT_B, ns=HOT_NS, T=HOT_T, width=D, support=hot_support(), check_lists=_hot_lists, hot=HOT,
         sample_alpha=1.0, constrained_embedding=True, layers=(D,), **XE, **HOT_OPT[opt])


# ------------------------------------------------------------------------------------------------ graph replay
def test_graph_replay_of_the_generic_step_is_bit_identical_to_eager():
    """adam with momentum, rows of 260 floats (two chunks), 16 steps with a ragged tail: the captured step graph and eager launches
    leave the same bits in the parameters and in every statistic."""
    I, B, ns, T, D = 700, 33, 200, 16, 260
    kw = dict(OPT['adam'], momentum=0.2, constrained_embedding=True, layers=(D,), **BPR)
    outs = []
    for g in (0, 1):
        o, m = make_pair(I, B, ns, store_rows=20, support=skewed_support(I), use_graph=g, **dict(kw))
        try:
            assert selection(m) == (1, UP_SPLIT, 2)
            m.set_plan(ragged_plan(o, I, B, T))
            m.train_steps(0, T)
            outs.append([m.get_losses(0, T).copy()] + [m.get_param(p + 'Wy', (I, D)).copy() for p in ('', 'acc_', 'acc2_', 'cnt_', 'vel_')] +
                        [m.get_param(p + 'By', (I,)).copy() for p in ('', 'acc_', 'acc2_', 'cnt_', 'vel_')] +
                        [m.get_param(p + 'Wh', (D, D), 0).copy() for p in ('', 'acc_', 'acc2_', 'cnt_', 'vel_')])
        finally:
            m.close()
    for a, b in zip(outs[0], outs[1]):
        np.testing.assert_array_equal(a, b)

"""k_loss_rows (g4r_loss_kernel.cuh) alone, on score rows the test supplies (Model.debug_loss_rows: the loss launch of a training
step, nothing before or behind it), against the oracle's own final_act_fwd / loss_fwd_bwd / final_act_bwd in float64 on the active
part of the matrix -- rows [0, M), columns [0, M) and [B, N), the positive of row i in column i, the result divided by B: the
compression OracleGRU4Rec.train_step uses.

Every case first asserts the instantiation from get_debug('kernels') (loss_spec, loss_long, loss_quads) and the row pitch, so that a
change of the predicates turns the case red instead of moving it to another form.  The three forms: `v1` one column per thread
(ldSc < 4096), `v4` four columns per thread, `long` the rows whose second copy lives in the score row itself.  Geometries (GEOMS)
sit on the edges of the kernel's loops: the second group of a thread (N = 1024 / 1025), all four prefetched groups with padding
behind them (N = 4071), the threshold ldSc = 4096, a last quad that straddles N (4099), the first loop trip past the prefetched
groups (8192 / 8195 / 12301), the last short row and largest LDS request (ldSc = 19824), the first long row (ldSc = 19840) and a
long row on which every thread makes a loop trip past the prefetch (N > 24576).  B = 37 is no multiple of 4: one quad holds
in-batch columns and negatives; the values of M put the positive in the first and in the last lane of its quad, in the quad that
straddles M, and leave no in-batch negative at all (M = 1).  Inactive in-batch columns, padding columns and the rows >= M hold a
stand-in of 30 -- far above every active score: a column that leaks into a maximum or a sum is seen.

Assertions per (case, M): d cost / d s on the active rows and columns |got - want| <= 1e-3 |want| + a max|want| of the same row;
lossrow[:M] with the cost bound (rtol 2e-4 + atol 2e-6); inactive in-batch and padding columns of the rows < M exactly 0; nothing
non-finite.  The coefficient a is derived, not tuned: 8 x the largest distance, in that same row-relative form, between the FLOAT32
oracle and the float64 one over the ordinary cases (the margin covers __expf, rcp and a 1024-thread reduction tree in place of
NumPy's exact exp and pairwise sums), 8 x 2.253e-6 = 1.8e-5; the extreme matrices have a measured value of their own
(8 x 7.6e-10 .. 4.7e-7), with one floor: all but three rows of an extreme matrix are ordinary rows, for which the ordinary
coefficient is the derived one, and 6e-9 of a row's maximum lies under the spacing of float32 itself (6e-8), so an extreme matrix's
coefficient is not taken below the ordinary one; neither may exceed 1e-4, compare_params' absolute fraction.  Figures: profiles/loss_rows_edges.md.  tests/test_loss_rows_reference.py runs the same cases
with the float32 oracle in the device's place and re-measures the distances."""
import numpy as np
import pytest

from gru4rec_amd import _native
from oracle.model import final_act_bwd, final_act_fwd, loss_fwd_bwd, parse_act
from test_gpu_generic_edges import NKEY      # floats of get_debug('kernels'): 4 x G4R_MAX_LAYERS per-layer slots, then the 12 choices
from test_gpu_parity import make_pair, random_plan, report

pytestmark = pytest.mark.gpu

TAIL = 4 * _native.G4R_MAX_LAYERS      # where the choices begin; [TAIL + 1 / 2 / 3] = loss_spec / loss_long / loss_quads
FILL = 30.0            # stand-in of every inactive entry of a supplied matrix
A_CAP = 1e-4           # compare_params' own absolute fraction: no coefficient may exceed it
# 8 x the largest float32-oracle distance over the ordinary cases (2.253e-6: tanh + top1 at N = 4096, M = 36; next 1.9e-7)
A_ORD = 8 * 2.253e-6
# the extreme matrices, per family group: 8 x the float32 oracle's distance on them (softmax 4.7e-7, max 7.6e-10, piecewise 1.5e-9),
# but no less than A_ORD: all but three rows of an extreme matrix are ordinary rows
EXT_MEASURED = {'softmax': 4.72e-7, 'max': 7.6e-10, 'piecewise': 1.5e-9}
A_EXT = {g: max(8 * v, A_ORD) for g, v in EXT_MEASURED.items()}
# softmax + cross-entropy with smoothing: with the positive 60 above everything the other probabilities (e^-60 / Z ~ 1e-26) sink under
# the loss's epsilon of 1e-24 and the FLOAT32 oracle itself leaves the bound (0.025 of the row's maximum); 55 above keeps it inside
EXT_GAP = {'smxe2': 55.0}

# tag (report lines), SPEC, configuration, family group of the extreme matrix
FAMILIES = [
    ('elubm', 1, dict(final_act='elu-0.5', loss='bpr-max', bpreg=0.5), 'piecewise'),
    ('smxe', 2, dict(final_act='softmax', loss='cross-entropy'), 'softmax'),
    ('elut1m', 3, dict(final_act='elu-0.5', loss='top1-max'), 'piecewise'),
    ('linbm', 0, dict(final_act='linear', loss='bpr-max'), 'max'),
    ('tanht1m', 0, dict(final_act='tanh', loss='top1-max'), None),
    ('smbm', 0, dict(final_act='softmax', loss='bpr-max'), 'softmax'),
    ('sllg1', 0, dict(final_act='softmax_logit', loss='xe_logit', smoothing=0.1), 'softmax'),
    # (the choice of SPEC does not look at the smoothing: the SPEC 2 build, in which `smooth != 0` leaves the fused branch for the generic one)
    ('smxe2', 2, dict(final_act='softmax', loss='cross-entropy', smoothing=0.2), 'softmax'),
    ('elulg', 0, dict(final_act='elu-1.0', loss='xe_logit'), 'piecewise'),
    ('linbpr', 0, dict(final_act='linear', loss='bpr'), None),
    ('tanht1', 0, dict(final_act='tanh', loss='top1'), None),
    ('lkbm', 0, dict(final_act='leaky-0.2', loss='bpr-max'), 'piecewise'),
    ('selubm', 0, dict(final_act='selu-1.05-1.67', loss='bpr-max'), 'piecewise'),
    ('relubm', 0, dict(final_act='relu', loss='bpr-max'), 'piecewise'),
]
FAM = {f[0]: f for f in FAMILIES}
M_V1, M_V4, M_LONG = (37, 34, 5, 1), (37, 36, 35, 34, 5, 1), (9, 6, 1)
# tag, form, B, N, ldSc, the values of M, runs the form's extreme matrices
GEOMS = [
    ('n60', 'v1', 37, 60, 64, M_V1, False),
    ('n1024', 'v1', 37, 1024, 1024, M_V1, False),
    ('n1025', 'v1', 37, 1025, 1040, M_V1, False),
    ('n4071', 'v1', 37, 4071, 4080, M_V1, True),
    ('q4096', 'v4', 37, 4096, 4096, M_V4, False),
    ('q4099', 'v4', 37, 4099, 4112, M_V4, False),
    ('q8192', 'v4', 37, 8192, 8192, M_V4, False),
    ('q8195', 'v4', 37, 8195, 8208, M_V4, False),
    ('q12301', 'v4', 37, 12301, 12304, M_V4, False),
    ('q19813', 'v4', 37, 19813, 19824, M_V4, True),
    ('l19825', 'long', 9, 19825, 19840, M_LONG, True),
    ('l24593', 'long', 9, 24593, 24608, M_LONG, False),
]
GEO = {g[0]: g for g in GEOMS}
EVERY_FAMILY = ('q19813', 'l19825', 'l24593')      # these geometries run every family
V1_TAGS, V4_TAGS = ('n60', 'n1024', 'n1025', 'n4071'), ('q4096', 'q4099', 'q8192', 'q8195', 'q12301')


def cases():
    """(family tag, geometry tag): the three pairs BASELINE's configurations use (SPEC 1 .. 3) on every geometry; every other family on
    the three geometries that run every family, one one-column geometry and one more four-column geometry (round robin): every
    family meets every form."""
    out = []
    for k, (ftag, spec, _, _) in enumerate(FAMILIES):
        tags = [g[0] for g in GEOMS] if k < 3 else [V1_TAGS[k % 4], V4_TAGS[k % 5]] + list(EVERY_FAMILY)
        out += [(ftag, t) for t in tags]
    return out


CASES = cases()
_matrices = {}


def base_matrix(gtag):
    """Standard normal scores x 2 from a seed fixed per geometry, [B, ldSc] float32 (shared by the families; never written to)."""
    if gtag not in _matrices:
        _, _, B, N, ld, _, _ = GEO[gtag]
        a = (np.random.RandomState(1000 + [g[0] for g in GEOMS].index(gtag)).randn(B, ld) * 2.0).astype(np.float32)
        a.setflags(write=False)
        _matrices[gtag] = a
    return _matrices[gtag]


def supplied(S, B, N, M):
    """The matrix as it is handed to the kernel: inactive in-batch columns, padding and the rows >= M hold FILL."""
    X = np.array(S, dtype=np.float32)
    X[:, M:B] = FILL
    X[:, N:] = FILL
    X[M:] = FILL
    return X


def extreme_matrix(group, S, B, N, gap=60.0):
    """One matrix per family group, M = B.  softmax: row 0's positive 60 above everything, row 1's positive 60 below the maximum,
    row 2 with two equal maxima.  max (an unbounded activation under a -max loss): rows 0 / 1 with max - positive = 78 / 95, either
    side of the kernel's clamp at 80; row 2's negatives spread over 200, so that softmax numerators underflow to 0.  piecewise: two
    quads of in-batch columns, two of negatives and the last columns before N at +1e-9 / -1e-9 in turn: d cost / d s must carry the
    slope of the input's sign (the output alone no longer tells: exp(-1e-9) - 1 rounds to -0)."""
    X = np.array(S, dtype=np.float32)
    big = int(np.abs(X[:3, :N]).max()) + 1
    if group == 'softmax':
        X[0, 0] = big + gap
        X[1, 1] = X[1, :N].max() - 60.0
        X[2, B + 5] = X[2, N - 2] = big + 3.0
    elif group == 'max':
        X[0, B + 7], X[0, 0] = 40.0, 40.0 - 78.0
        X[1, N - 3], X[1, 1] = 50.0, 50.0 - 95.0
        X[2, B:N] = np.linspace(-100.0, 100.0, N - B, dtype=np.float32)[np.random.RandomState(5).permutation(N - B)]
        X[2, 2] = 0.0
    else:
        cols = np.r_[0:8, B + 3:B + 11, N - 9:N]
        X[:, cols] = np.where(cols % 2 == 0, 1e-9, -1e-9).astype(np.float32)[None, :]
    return X


def oracle_rows(cfg, X, B, N, M, dtype):
    """(d cost / d s [M, M + N - B], row losses [M]) of the active part of X, by the oracle's own three functions in `dtype`."""
    fa = parse_act(cfg['final_act'])
    cols = np.r_[0:M, B:N]
    s = np.ascontiguousarray(X[:M][:, cols], dtype=dtype)      # (row-major, as train_step's y @ Sy.T: NumPy's pairwise row sums)
    colmask = np.ones(len(cols), dtype=bool)
    yhat = final_act_fwd(*fa, s, colmask).astype(dtype)
    L, dy = loss_fwd_bwd(cfg['loss'], yhat, M, np.arange(M), colmask, cfg.get('bpreg', 1.0), cfg.get('smoothing', 0.0), per_row=True)
    ds = (final_act_bwd(*fa, s, yhat, dy, colmask) / np.dtype(dtype).type(B)).astype(dtype)
    return ds, np.asarray(L, dtype=dtype)


def oracle32_as_device(cfg, X, B, N, M):
    """What debug_loss_rows returns, computed by the float32 oracle: the rows >= M as they came, inactive columns of the others 0."""
    ds, L = oracle_rows(cfg, X, B, N, M, np.float32)
    out = np.array(X, dtype=np.float32)
    out[:M] = 0.0
    out[:M, :M] = ds[:, :M]
    out[:M, B:N] = ds[:, M:]
    lossrow = np.zeros(B, dtype=np.float32)
    lossrow[:M] = L
    return out, lossrow


def needed_a(got, want):
    """The smallest a with |got - want| <= 1e-3 |want| + a max|want| of the same row."""
    err = np.abs(np.asarray(got, dtype=np.float64) - want) - 1e-3 * np.abs(want)
    return float((np.maximum(err, 0.0) / np.abs(want).max(axis=1, keepdims=True)).max())


def check(name, got_ds, got_L, X, cfg, B, N, M, a, errs):
    """One (case, M): two report lines, `name ds` and `name loss`, in test_gpu_parity's format; the names of what failed go to errs.
    Returns the float64 reference's (ds, L)."""
    assert a <= A_CAP
    want, wantL = oracle_rows(cfg, X, B, N, M, np.float64)
    act = np.concatenate([got_ds[:M, :M], got_ds[:M, B:N]], axis=1).astype(np.float64)
    scale = np.abs(want).max(axis=1, keepdims=True)
    err = np.abs(act - want)
    tol = 1e-3 * np.abs(want) + a * scale
    finite = bool(np.isfinite(got_ds[:M]).all() and np.isfinite(got_L[:M]).all())
    worst = float((err / tol).max()) if finite else float('inf')
    at = np.unravel_index(int(np.argmax(np.where(np.isfinite(err), err / tol, np.inf))), err.shape)
    col = int(at[1]) if at[1] < M else int(at[1]) - M + B
    zeros = bool((got_ds[:M, M:B] == 0).all() and (got_ds[:M, N:] == 0).all())
    bad = not finite or worst > 1.0 or not zeros
    report('%-28s max_abs_err %.3e  max|want| %.3e  worst/tol %.3f %s' % (
        name + ' ds', float(np.nanmax(err)), float(scale.max()), worst, 'FAIL' if bad else 'ok'))
    if bad:      # the element, not just the tensor
        report('    %s ds: worst at row %d column %d, got %.9g want %.9g; inactive columns %s' % (
            name, int(at[0]), col, float(act[at]), float(want[at]), 'zero' if zeros else 'NOT zero'))
        errs.append(name + ' ds')
    lerr = np.abs(got_L[:M].astype(np.float64) - wantL)
    ltol = 2e-6 + 2e-4 * np.abs(wantL)
    lbad = not finite or bool((lerr > ltol).any())
    report('%-28s max_abs_err %.3e  max|want| %.3e  worst/tol %.3f %s' % (
        name + ' loss', float(np.nanmax(lerr)), float(np.abs(wantL).max()), float(np.nanmax(lerr / ltol)), 'FAIL' if lbad else 'ok'))
    if lbad:
        errs.append(name + ' loss')
    return want, wantL


def run_case(ftag, gtag, run, errs, measure=None):
    """Every M of the case, then the form's extreme matrix where the geometry carries one.  run(cfg, X, M) -> (ds [B, ldSc], lossrow [B])."""
    _, _, cfg, group = FAM[ftag]
    _, _, B, N, ld, Ms, ext = GEO[gtag]
    S = base_matrix(gtag)
    for M in Ms:
        X = supplied(S, B, N, M)
        ds, L = run(cfg, X, M)
        want, _ = check('%s %s M=%d' % (ftag, gtag, M), ds, L, X, cfg, B, N, M, A_ORD, errs)
        if measure is not None:
            measure('ordinary', needed_a(np.concatenate([ds[:M, :M], ds[:M, B:N]], axis=1), want))
    if ext and group:
        X = supplied(extreme_matrix(group, S, B, N, EXT_GAP.get(ftag, 60.0)), B, N, B)
        ds, L = run(cfg, X, B)
        want, _ = check('%s %s X' % (ftag, gtag), ds, L, X, cfg, B, N, B, A_EXT[group], errs)
        if measure is not None:
            measure(group, needed_a(np.concatenate([ds[:B, :B], ds[:B, B:N]], axis=1), want))


def loss_model(cfg, B, ns):
    """A tiny model whose training step launches the k_loss_rows under test (the catalogue plays no part: 64 items)."""
    fa = parse_act(cfg['final_act'])
    return _native.Model(n_items=64, layers=[4], batch_size=B, n_sample=ns, loss=_native.LOSS_IDS[cfg['loss']],
                         final_act=_native.ACT_IDS[fa[0]], final_act_p0=fa[1], final_act_p1=fa[2], hidden_act=2, embed_mode=0,
                         learning_rate=0.05, momentum=0.0, bpreg=cfg.get('bpreg', 1.0), smoothing=cfg.get('smoothing', 0.0),
                         sample_alpha=0.5, sample_store=2 * ns, seed=1, device=0, rank=0, nranks=1, use_graph=0)


@pytest.mark.parametrize('ftag,gtag', CASES, ids=['%s-%s' % c for c in CASES])
def test_loss_rows(ftag, gtag):
    _, spec, cfg, _ = FAM[ftag]
    _, form, B, N, ld, _, _ = GEO[gtag]
    m = loss_model(cfg, B, N - B)
    try:
        tail = m.get_debug('kernels', (NKEY,))[TAIL:]
        assert int(m.get_debug('ldSc', (1,))[0]) == ld
        assert (int(tail[1]), int(tail[2]), int(tail[3])) == (spec, int(form == 'long'), int(form != 'v1')), tail
        errs = []
        run_case(ftag, gtag, lambda cfg_, X, M: m.debug_loss_rows(X, M), errs)
        assert not errs, errs
    finally:
        m.close()


def test_refusals():
    m = loss_model(FAM['elubm'][2], 37, 23)
    try:
        X = np.zeros((37, 64), dtype=np.float32)
        for bad, M, text in ((X[:, :48], 5, 'size mismatch'), (X, 0, 'M outside'), (X, 38, 'M outside')):
            with pytest.raises(_native.NativeError, match=text):
                m.debug_loss_rows(bad, M)
    finally:
        m.close()


@pytest.mark.parametrize('use_graph', [0, 1])
def test_debug_call_leaves_training_untouched(use_graph):
    """A model that runs debug_loss_rows between set_plan and train_steps(0, 6), and one that runs it between two train_steps calls,
    leave the bits of a model that made the same train_steps calls and never called it: losses, Wy, acc_Wy, Wx.  The supplied
    matrix is full of the stand-in, with M = 5 of 37 rows."""
    B, ns, T = 37, 4062, 6
    kw = dict(loss='bpr-max', final_act='elu-0.5', bpreg=0.5, constrained_embedding=True, layers=(4,), use_graph=use_graph)
    X = supplied(base_matrix('q4099'), B, B + ns, 5)

    def run(split, where):
        o, m = make_pair(64, B, ns, store_rows=8, **kw)
        m.set_plan(random_plan(64, B, T, seed=11, tail=True))
        if where == 0:
            m.debug_loss_rows(X, 5)
        m.train_steps(0, split)
        if where == 1:
            m.debug_loss_rows(X, 5)
        if split < T:
            m.train_steps(split, T - split)
        out = [m.get_losses(0, T), m.get_param('Wy', o.Wy.shape), m.get_param('acc_Wy', o.Wy.shape), m.get_param('Wx', o.Wx[0].shape)]
        m.close()
        return out

    for split, where in ((T, 0), (2, 1)):
        for a, b in zip(run(split, None), run(split, where)):
            assert np.isfinite(a).all() and np.array_equal(a, b), (split, where)

"""The hidden activation (`hidden_act`) through every GRU kernel family, against the float64 oracle.  Needs an MI355X.

`hidden_act` is a run-time argument of every GRU kernel, and each family carries its own copy of the code that applies it: the lean
pair (k_gru_h / k_gru_da), the fused pair (k_gru_fwd_fused / k_gru_bwd_fused), the three-launch tiles (k_gru_p2 / k_gru_bwd_pre), the
wide tiles in both geometries and K-sliced, the one-hot layer, and the prediction GRU.  The rest of the suite runs `tanh` (and one
`relu` case on the lean pair).  Here every family runs relu, linear, leaky, elu, selu and a tanh control:

  (a) one step with M = B - 3: r, z, c, hd, dV (all three thirds), dSx and the cost against OracleGRU4Rec(dtype=float64) on the same
      fp32 weights, then every parameter / accumulator against the fp32 oracle (compare_params);
  (b) four steps with a ragged tail (M = B, B, B - 3, 5, items repeated between input and negatives): losses and parameters with
      the tolerances of test_gpu_lean_edges.py / test_gpu_wide_layers.py;
  (c) the sign-bit path: candidate pre-activations of exactly +-1e-9 (zero weights plus a bias).  exp(a) - 1 rounds to 0 in fp32, the
      backward kernels only see c, so the slope has to travel in the sign bit of the zero (g4r_device.cuh: neg_branch) through c[l];
  (d) prediction (predict_step) for every activation, both k_gru_p2 geometries at 256 units;
  (e) graph replay == eager launches, bit for bit, with elu.

Every family case first asserts the kernel selection (get_debug('kernels')), so a predicate change turns the case red instead of
quietly testing another family.

Kink margin.  A hidden pre-activation a rounding away from 0 lands on either slope depending on the summation order.  (a) and (b)
assert, on the float64 oracle alone, for every step and layer, that
    min |a| / (eps32 * (|H r| @ |Wh| + |y| @ |Wx[:, :D]| + |Bh[:D]|)) > KINK_MARGIN = 8
(twice the oracle's kink_ulps = 4 window): a property of the inputs, not of the code under test.  Minima per case:
profiles/hidden_act_parity.md.

dV bound.  The fp32 oracle and the float64 oracle run the same step; the largest |dV32 - dV64| / max|dV64 of that third| over all (a)
cases of this file is DV_ORACLE_DIST (measured on the CPU, profiles/hidden_act_parity.md); the kernels sum in another order and use
v_exp / v_rcp (~1e-6 relative each), so they get DV_BOUND = 4 x that, relative to the third's scale.

tests/test_gpu_mutation.py: builds 22 (branch decided on the value of c) and 23 (negative-branch slope x 1.01) must turn named
report lines of (c) / (a) red."""
import os

import numpy as np
import pytest

from gru4rec_amd import _native
from oracle.model import OracleGRU4Rec, act_bwd, parse_act
from test_gpu_parity import close, close_rel, compare_params, make_pair, random_plan, report, snapshot

pytestmark = pytest.mark.gpu

ACTS = ['relu', 'linear', 'leaky-0.2', 'elu-0.5', 'selu-1.0507-1.6733']
ALL_ACTS = ['tanh'] + ACTS
SIGN_ACTS = ['leaky-0.2', 'elu-0.5', 'selu-1.0507-1.6733', 'relu']
PIECEWISE = ('relu', 'leaky', 'elu', 'selu')
KINK_MARGIN = 8.0
# largest |dV(fp32 oracle) - dV(float64 oracle)| / max|dV(float64) of that third| over the one-step cases of this file (CPU run of
# both oracles, every family x activation x dropout x loss row below: profiles/hidden_act_parity.md; the largest is that of
# lean_tiles-elu-0.5-xe-dh0.00), and the kernels' bound: 4 x that = 6.70e-6 of the third's scale
DV_ORACLE_DIST = 1.675e-6
DV_BOUND = 4.0 * DV_ORACLE_DIST

SWITCHES = ('G4R_NO_LEAN', 'G4R_WIDE2', 'G4R_P2_GEO', 'G4R_BA_GEO')
WIDE = (3000, 96, 512, (256,))
# name: shape (I, B, ns, layers), switches, expected GruFwdKind / GruBwdKind per layer, p2_deep + 2 ba_deep of layer 0 (None: not pinned),
# wide_mask (None: not pinned), one-hot input, hidden dropout 0.25 as well (kernels that regenerate the mask in the backward)
FAMILIES = {
    'lean': dict(shape=(900, 33, 150, (36,)), env={}, fwd=(0,), bwd=(0,), drop=True),
    'lean2': dict(shape=(3000, 64, 300, (36, 124)), env={}, fwd=(0, 0), bwd=(0, 0), drop=True),
    'fused36': dict(shape=(900, 33, 150, (36,)), env=dict(G4R_NO_LEAN=1), fwd=(1,), bwd=(1,), drop=True),
    'fused100': dict(shape=(900, 33, 150, (100,)), env=dict(G4R_NO_LEAN=1), fwd=(1,), bwd=(1,), drop=True),
    'tiles132': dict(shape=(3000, 33, 150, (132,)), env={}, fwd=(4,), bwd=(4,), drop=True),
    # dy hand-off from k_gru_bwd_b into k_gru_da.  A separate 36-wide embedding: with the constrained one layer 0 reads rows of Wy, 132 wide,
    # past the lean kernels' limit of 128 input columns
    'lean_tiles': dict(shape=(3000, 64, 300, (36, 132)), env={}, fwd=(0, 4), bwd=(0, 4), drop=True, embedding=36),
    'onehot': dict(shape=(300, 33, 150, (36,)), env={}, fwd=(4,), bwd=(2,), onehot=True),
    'wide_w4': dict(shape=WIDE, env=dict(G4R_WIDE2=0, G4R_P2_GEO=0, G4R_BA_GEO=0), fwd=(3,), bwd=(4,), geo=0),
    'wide_w8d': dict(shape=WIDE, env=dict(G4R_WIDE2=0, G4R_P2_GEO=1, G4R_BA_GEO=1), fwd=(3,), bwd=(4,), geo=3),
    'wide_ks': dict(shape=WIDE, env=dict(G4R_WIDE2=25), fwd=(2,), bwd=(3,), wide_mask=25),
}
# plan seeds of the cases whose default plan (seed 5 for one step, 77 for four) leaves a pre-activation inside the kink margin
PLAN_SEED = {('a', 'lean2-relu-bprmax-dh0.25'): 6,              # (seed 5: margin 4.2)
             ('b', 'lean_tiles-elu-0.5-bprmax-dh0.00'): 78,      # (seed 77: 2.2)
             ('b', 'lean_tiles-elu-0.5-bprmax-dh0.25'): 78}      # (seed 77: 3.1)


def _env(**kv):
    class _E:
        def __enter__(self):
            self.old = {k: os.environ.get(k) for k in kv}
            for k, v in kv.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = str(v)

        def __exit__(self, *a):
            for k, v in self.old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
    return _E()


def one_step_cases():
    """(family, activation, loss row, hidden dropout) of (a) and (b): every activation and the tanh control per family on bpr-max /
    linear, hidden dropout 0.25 as well where the backward regenerates the mask, one cross-entropy / softmax row per family."""
    out = []
    for fam, F in FAMILIES.items():
        for act in ALL_ACTS:
            for dh in ((0.0, 0.25) if F.get('drop') else (0.0,)):
                out.append((fam, act, 'bprmax', dh))
        out.append((fam, 'elu-0.5', 'xe', 0.0))
    return out


def case_id(c):
    return '%s-%s-%s-dh%.2f' % c


def model_kwargs(fam, act, loss, dh):
    F = FAMILIES[fam]
    kw = dict(layers=F['shape'][3], hidden_act=act, learning_rate=0.1, bpreg=0.5, dropout_p_hidden=dh)
    kw.update(dict(loss='bpr-max', final_act='linear') if loss == 'bprmax' else dict(loss='cross-entropy', final_act='softmax'))
    if F.get('embedding'):
        kw.update(constrained_embedding=False, embedding=F['embedding'])
    elif not F.get('onehot'):
        kw['constrained_embedding'] = True
    return kw


def float64_twin(o, I, B, ns, store_rows, seed, kw):
    """The float64 oracle on the fp32 oracle's weights, state, popularity and sample store, cast up."""
    o64 = OracleGRU4Rec(n_items=I, batch_size=B, n_sample=ns, dtype=np.float64, seed=seed, **kw)
    o64.set_popularity(o.P0.astype(np.float64))
    o64.make_sample_store(store_rows * ns if ns else 0)
    if ns:
        np.testing.assert_array_equal(o64.ST, o.ST)
    for n in ('Wx', 'Wh', 'Wrz', 'Bh', 'H'):
        setattr(o64, n, [a.astype(np.float64) for a in getattr(o, n)])
    o64.Wy, o64.By = o.Wy.astype(np.float64), o.By.astype(np.float64)
    if o.E is not None:
        o64.E = o.E.astype(np.float64)
    o64.init0 = snapshot(o64)
    return o64


def make_trio(fam, act, loss, dh, store_rows=6, seed=3, use_graph=0):
    """(fp32 oracle, float64 oracle, device model) with identical fp32 weights, the family's switches set while the model is created."""
    I, B, ns, _ = FAMILIES[fam]['shape']
    kw = model_kwargs(fam, act, loss, dh)
    env = dict.fromkeys(SWITCHES)
    env.update(FAMILIES[fam]['env'])
    with _env(**env):
        o, m = make_pair(I, B, ns, store_rows=store_rows, seed=seed, use_graph=use_graph, **kw)
    return o, float64_twin(o, I, B, ns, store_rows, seed, kw), m


def assert_selection(m, fam):
    F = FAMILIES[fam]
    ML = _native.G4R_MAX_LAYERS
    k = m.get_debug('kernels', 4 * ML + 12)
    L = len(F['shape'][3])
    got = (tuple(int(v) for v in k[:L]), tuple(int(v) for v in k[ML:ML + L]))
    assert got == (F['fwd'], F['bwd']), '%s: GruFwdKind / GruBwdKind %s, expected %s' % (fam, got, (F['fwd'], F['bwd']))
    if F.get('geo') is not None:
        assert int(k[2 * ML]) == F['geo'], '%s: p2_deep + 2 ba_deep = %d, expected %d' % (fam, int(k[2 * ML]), F['geo'])
    if F.get('wide_mask') is not None:
        assert int(m.get_debug('wide_mask', 1)[0]) == F['wide_mask'], fam


def one_step_plan(fam, cid):
    I, B, _, _ = FAMILIES[fam]['shape']
    plan = random_plan(I, B, 1, seed=PLAN_SEED.get(('a', cid), 5))
    plan['M'][:] = B - 3
    return plan


def ragged_plan(fam, cid, o, T=4):
    I, B, _, _ = FAMILIES[fam]['shape']
    plan = random_plan(I, B, T, seed=PLAN_SEED.get(('b', cid), 77))
    plan['M'][:] = [B, B, B - 3, 5][:T] if T == 4 else B
    plan['in_idx'][:, :6] = o.ST[0][:6]      # items repeated between input and negatives
    plan['out_idx'][:, 6:12] = plan['in_idx'][:, :6]
    return plan


def pre_step(o):
    """The weights the next step's pre-activations are formed from (the step overwrites them)."""
    return dict(Wx=[w.copy() for w in o.Wx], Wh=[w.copy() for w in o.Wh], Bh=[b.copy() for b in o.Bh])


def kink_margin(o, pre, dbg, in_idx, M):
    """min over layers and elements of |a| / (eps32 * (|H r| @ |Wh| + |y| @ |Wx[:, :D]| + |Bh[:D]|)) of a float64 oracle step."""
    eps = float(np.finfo(np.float32).eps)
    worst = np.inf
    for l, cch in enumerate(dbg['caches']):
        D = o.layers[l]
        terms = np.abs(cch['H'] * cch['r']) @ np.abs(pre['Wh'][l]) + np.abs(pre['Bh'][l][:D])[None, :]
        if o.onehot and l == 0:
            terms = terms + np.abs(pre['Wx'][0][np.asarray(in_idx[:M], dtype=np.int64)][:, :D])
        else:
            terms = terms + np.abs(cch['y']) @ np.abs(pre['Wx'][l][:, :D])
        worst = min(worst, float((np.abs(cch['a']) / (eps * terms)).min()))
    return worst


def oracle_step(o, plan, t):
    return o.train_step(plan['in_idx'][t], plan['out_idx'][t], int(plan['M'][t]), plan['reset'][t], return_debug=True)


def dv_thirds(D):
    return (('da', slice(0, D)), ('drp', slice(D, 2 * D)), ('dzp', slice(2 * D, 3 * D)))


def oracle_dv_distance(dbg32, dbg64, layers):
    """Largest |dV32 - dV64| / max|dV64 of that third| over the layers and thirds of one step of the two oracles."""
    worst = 0.0
    for l, D in enumerate(layers):
        a, b = np.asarray(dbg32['caches'][l]['dV'], dtype=np.float64), dbg64['caches'][l]['dV']
        for _, sl in dv_thirds(D):
            worst = max(worst, float(np.abs(a[:, sl] - b[:, sl]).max() / np.abs(b[:, sl]).max()))
    return worst


@pytest.mark.parametrize('case', one_step_cases(), ids=case_id)
def test_one_step_against_the_float64_oracle(case):
    """(a): report lines `ha <tensor>`."""
    fam, act, loss, dh = case
    cid = case_id(case)
    I, B, ns, layers = FAMILIES[fam]['shape']
    o, o64, m = make_trio(fam, act, loss, dh)
    try:
        assert_selection(m, fam)
        plan = one_step_plan(fam, cid)
        M = int(plan['M'][0])
        m.set_plan(plan)
        pre = pre_step(o64)
        cost64, dbg64 = oracle_step(o64, plan, 0)
        _, dbg32 = oracle_step(o, plan, 0)
        margin = kink_margin(o64, pre, dbg64, plan['in_idx'][0], M)
        dist = oracle_dv_distance(dbg32, dbg64, layers)
        report('--- hidden_act one step %s: kink margin %.1f, fp32-vs-float64 oracle dV distance %.3e' % (cid, margin, dist))
        if parse_act(act)[0] in PIECEWISE:
            assert margin > KINK_MARGIN, 'a pre-activation on the kink (margin %.2f): pick another plan seed (PLAN_SEED)' % margin
        assert dist <= 1.001 * DV_ORACLE_DIST, 'the oracles are %.3e apart on dV: DV_ORACLE_DIST no longer is their largest distance' % dist
        m.train_steps(0, 1)
        errs = []
        for l, D in enumerate(layers):
            cch = dbg64['caches'][l]
            for n in ('r', 'z', 'c', 'hd'):
                close('ha %s%d' % (n, l), m.get_debug('%s%d' % (n, l), (B, D))[:M], cch[n], errs=errs)
            dV = m.get_debug('dV%d' % l, (B, 3 * D))[:M]
            for n, sl in dv_thirds(D):
                close_rel('ha dV%d %s' % (l, n), dV[:, sl], cch['dV'][:, sl], 0.0, DV_BOUND, errs=errs)
        generic = (o.adapt != 'adagrad' or o.grad_cap > 0)
        g = np.asarray(dbg64['dSx'], dtype=np.float64)      # the producers store the Adagrad step (accumulators are 0 before step 0)
        want = g if generic else o.learning_rate * g / np.sqrt(g * g + 1e-6)
        n_in = layers[-1] if o.constrained_embedding else (o.embedding or 3 * layers[0])
        close('ha dSx(step)', m.get_debug('dSx', (B, n_in))[:M], want, atol=2e-6, rtol=2e-3, errs=errs)
        close('ha cost', m.get_losses(0, 1), [cost64], atol=2e-6, rtol=2e-4, errs=errs)
        compare_params(o, m, errs, 'ha', Mrows=M)
        assert not errs, errs
    finally:
        m.close()


@pytest.mark.parametrize('case', one_step_cases(), ids=case_id)
def test_four_steps_with_a_ragged_tail(case):
    """(b): report lines `hb <tensor>`."""
    fam, act, loss, dh = case
    cid = case_id(case)
    I, B, ns, layers = FAMILIES[fam]['shape']
    T = 4
    o, o64, m = make_trio(fam, act, loss, dh)
    try:
        assert_selection(m, fam)
        plan = ragged_plan(fam, cid, o)
        m.set_plan(plan)
        want, margin = [], np.inf
        for t in range(T):
            pre = pre_step(o64)
            _, dbg64 = oracle_step(o64, plan, t)
            margin = min(margin, kink_margin(o64, pre, dbg64, plan['in_idx'][t], int(plan['M'][t])))
            want.append(o.train_step(plan['in_idx'][t], plan['out_idx'][t], int(plan['M'][t]), plan['reset'][t]))
        report('--- hidden_act four steps %s: kink margin %.1f' % (cid, margin))
        if parse_act(act)[0] in PIECEWISE:
            assert margin > KINK_MARGIN, 'a pre-activation on the kink (margin %.2f): pick another plan seed (PLAN_SEED)' % margin
        m.train_steps(0, T)
        errs = []
        close('hb loss curve', m.get_losses(0, T), np.array(want), atol=5e-6, rtol=5e-4, errs=errs)
        compare_params(o, m, errs, 'hb', Mrows=5)
        assert not errs, errs
    finally:
        m.close()


@pytest.mark.parametrize('act', SIGN_ACTS)
@pytest.mark.parametrize('fam', sorted(FAMILIES))
def test_branch_travels_in_the_sign_bit_of_the_stored_candidate(fam, act):
    """(c): Wx[l][:, :D] = 0, Wh[l] = 0, Bh[l][:D] = +1e-9 on even and -1e-9 on odd columns, every layer: the candidate pre-activation
    is +-1e-9 in any summation order (zero products plus the bias), elu / selu give exp(a) - 1 = 0 in fp32.  dV<l>[:, :D] (da) against
    the float64 oracle with the bounds of the final activation's test of the same property.  Report lines `sb dV<l> da`."""
    I, B, ns, layers = FAMILIES[fam]['shape']
    kind, p0, p1 = parse_act(act)
    o, o64, m = make_trio(fam, act, 'bprmax', 0.0)
    try:
        assert_selection(m, fam)
        for l, D in enumerate(layers):
            bias = np.where(np.arange(D) % 2 == 0, 1e-9, -1e-9).astype(np.float32)
            for x in (o, o64):
                x.Wx[l][:, :D] = 0
                x.Wh[l][:] = 0
                x.Bh[l][:D] = bias
            m.set_param('Wx', o.Wx[l], l)
            m.set_param('Wh', o.Wh[l], l)
            m.set_param('Bh', o.Bh[l], l)
        plan = one_step_plan(fam, None)
        M = int(plan['M'][0])
        m.set_plan(plan)
        cost64, dbg64 = oracle_step(o64, plan, 0)
        m.train_steps(0, 1)
        errs = []
        report('--- hidden_act sign bit %s %s' % (fam, act))
        pos, neg = {'relu': (1.0, 0.0), 'leaky': (1.0, p0), 'elu': (1.0, p0), 'selu': (p0, p0 * p1)}[kind]
        for l, D in enumerate(layers):
            cch = dbg64['caches'][l]
            even, odd = np.arange(0, D, 2), np.arange(1, D, 2)
            # the reference side: the pre-activations are what the construction says, the two slopes differ by the factor alpha
            assert (cch['a'][:, even] == np.float64(np.float32(1e-9))).all() and (cch['a'][:, odd] == np.float64(np.float32(-1e-9))).all()
            slope = act_bwd(kind, p0, p1, cch['a'], cch['c'])
            np.testing.assert_allclose(slope[:, even], pos, rtol=1e-8)
            np.testing.assert_allclose(slope[:, odd], neg, rtol=1e-8, atol=0)
            da = cch['dV'][:, :D]
            assert (np.abs(da[:, even]) > 0).all()
            assert (da[:, odd] == 0).all() if kind == 'relu' else (np.abs(da[:, odd]) > 0).all()
            close('sb dV%d da' % l, m.get_debug('dV%d' % l, (B, 3 * D))[:M, :D], da, atol=1e-9, rtol=2e-3, errs=errs)
        close('sb cost', m.get_losses(0, 1), [cost64], atol=2e-6, rtol=2e-4, errs=errs)
        assert not errs, errs
    finally:
        m.close()


PREDICT = {'d36': ((36,), None), 'd132': ((132,), None), 'd36_132': ((36, 132), None), 'd256_geo0': ((256,), 0), 'd256_geo1': ((256,), 1)}


@pytest.mark.parametrize('act', ALL_ACTS)
@pytest.mark.parametrize('name', sorted(PREDICT))
def test_predict_step(name, act):
    """(d): predict_begin(37), three predict_steps and one over a 77-item subset against the oracle (test_predict_and_ranks' bounds)."""
    layers, geo = PREDICT[name]
    I, B, pb = 300, 24, 37
    env = dict.fromkeys(SWITCHES)
    env['G4R_P2_GEO'] = geo
    with _env(**env):
        o, m = make_pair(I, B, 0, store_rows=0, loss='bpr-max', final_act='linear', hidden_act=act, constrained_embedding=True, layers=layers)
    try:
        if geo is not None:
            assert int(m.get_debug('deep_geo', 1)[0]) == geo
        rng = np.random.RandomState(23)
        m.predict_begin(pb)
        H = [np.zeros((pb, D), dtype=np.float32) for D in layers]
        errs = []
        report('--- hidden_act predict %s %s' % (name, act))
        for step in range(3):
            in_idx = rng.randint(0, I, size=pb)
            want, H = o.predict_step(H, in_idx)
            close('hp scores step %d' % step, m.predict_step(in_idx), want, atol=2e-6, rtol=3e-4, errs=errs)
        sel = rng.permutation(I)[:77]
        in_idx = rng.randint(0, I, size=pb)
        want, H = o.predict_step(H, in_idx, sel)
        close('hp scores subset', m.predict_step(in_idx, sel), want, atol=2e-6, rtol=3e-4, errs=errs)
        assert not errs, errs
    finally:
        m.close()


@pytest.mark.parametrize('fam', sorted(FAMILIES))
def test_graph_replay_is_bit_identical_to_eager(fam):
    """(e): 8 steps with elu-0.5 as a graph replay and as eager launches: the same bits in the losses, Wy, Wx and acc_Wh."""
    I, B, ns, layers = FAMILIES[fam]['shape']
    T = 8
    outs = []
    for g in (0, 1):
        o, _, m = make_trio(fam, 'elu-0.5', 'bprmax', 0.0, store_rows=10, use_graph=g)
        try:
            assert_selection(m, fam)
            plan = ragged_plan(fam, None, o, T=T)
            plan['M'][T // 2:] = B - 3
            plan['M'][-1] = 5
            m.set_plan(plan)
            m.train_steps(0, T)
            out = [m.get_losses(0, T).copy(), m.get_param('Wy', (I, layers[-1])).copy()]
            for l, D in enumerate(layers):
                out += [m.get_param('Wx', o.Wx[l].shape, l).copy(), m.get_param('acc_Wh', (D, D), l).copy()]
            outs.append(out)
        finally:
            m.close()
    assert np.isfinite(outs[0][0]).all() and len(np.unique(outs[0][0])) == T
    for a, b in zip(outs[0], outs[1]):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize('name', ['softmax', 'softmax_logit'])
def test_library_refuses_the_softmax_names_as_hidden_activations(name):
    with pytest.raises(_native.NativeError, match='not a hidden activation'):
        _native.Model(n_items=10, layers=[8], batch_size=4, n_sample=0, loss=_native.LOSS_IDS['bpr-max'], final_act=_native.ACT_IDS['linear'],
                      hidden_act=_native.ACT_IDS[name], embed_mode=0, learning_rate=0.1, sample_store=0, seed=1, device=0, rank=0, nranks=1)

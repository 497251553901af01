"""Oracle parity of the wide-layer K-sliced kernels (g4r_wide_kernels.cuh: k_gru_p1s + k_gru_gate, k_gru_bwd_bw, finish_rows /
k_finish_rows, k_dense_grad2) on the shapes they are written around: the largest layer g4r_create accepts (every fixed-size array of
the slice consumers full at once: 8 input + 8 hidden slices in k_gru_gate, 16 dy planes in finish_rows), 16 dy slices and one past
them, dy slices of two and of three ring stages of gemm_tile3<3, 32> and a short last slice, input widths of one column tile (64), a
partial second one (80) and two uneven input slices (144), widths that fall off the wide path (48, 72), a wide layer above a lean,
a three-launch and a fused layer (k_gru_da / k_gru_bwd_pre add the dy planes up, or nobody does), k_finish_rows in front of the
merged k_update (mask 8 alone), row tiles that hold one row and row tiles that a shrinking batch empties, and the L2 term of
k_dense_grad2's two in-place epilogues with and without momentum.

Every case first asserts its selection from the debug keys `kernels` (GruFwdKind / GruBwdKind per layer, update, chunks, wide_dense,
finish_rows) and `wide_geo` (per layer use, ny, nh, kys, khs, bbn, bbk) against LITERAL numbers: a predicate change in
choose_kernels that moves a shape off its edge turns the case red instead of quietly testing another path.  Where a dy slice count
follows from the CU count it is min(n_cu / tiles, 3 D / 128) = 6 with at most 12 tiles, so the literal holds on any device of more
than 72 CUs; the one case whose geometry is decided by the CU count (max_width) skips on a device that does not
have 256.  Then 6-7 steps of a ragged plan (M = B, a live batch that ends inside a 64-row tile, a last step with M = 5, items
repeated between inputs, targets and negatives) against OracleGRU4Rec with the tolerances of test_gpu_lean_edges.py: per-step cost
rtol 5e-4 + atol 5e-6, parameters / accumulators / velocities by compare_params with loosen = 1.  The switches are set around model
creation only (they are read at g4r_create).

tests/test_gpu_mutation.py: a build whose finish_rows leaves out the sixteenth plane turns test_dy_16_slices red and leaves
test_two_stage_slices green; a build whose k_gru_p1s keys the embedding-dropout mask inside the slice turns test_input_width[144]
red and leaves test_input_width[80] green."""
import numpy as np
import pytest

from test_gpu_parity import close, compare_params, kink_twin, make_pair, oracle_steps, random_plan, report
from test_gpu_wide_layers import _env

pytestmark = pytest.mark.gpu

ALL = 1 | 8 | 16      # G4R_WIDE2: k_gru_p1s + k_gru_gate, k_gru_bwd_bw, k_dense_grad2
ML = 8                # G4R_MAX_LAYERS: `kernels` holds 4 ML per-layer values and 12 scalars, `wide_geo` 7 per layer
FWD_LEAN, FWD_FUSED, FWD_P1S, FWD_P1_N64, FWD_P1_N32 = range(5)      # GruFwdKind (g4r_host_model.hpp)
BWD_LEAN, BWD_FUSED, BWD_ONEHOT, BWD_BW, BWD_B = range(5)            # GruBwdKind
UP_LEAN, UP_MERGED, UP_SPLIT = range(3)                              # UpdateKind
OFF = (0, 1, 1, 0, 0, 1, 0)      # WideGeo's defaults: a layer off the wide path
SWITCHES = ('G4R_WIDE2', 'G4R_BB_KS', 'G4R_P1_KS', 'G4R_NO_LEAN', 'G4R_P2_GEO', 'G4R_BA_GEO', 'G4R_NO_MERGE', 'G4R_LEAN_UPDATE', 'G4R_DEFER')
RECORDED_CUS = 256

BPRMAX = dict(loss='bpr-max', final_act='elu-0.5', learning_rate=0.1, bpreg=0.5)
XE = dict(loss='cross-entropy', final_act='softmax', learning_rate=0.065, logq=1.0)


def selection(m, L):
    """{'fwd', 'bwd', 'use': per layer; 'update', 'chunks', 'wide_dense', 'finish_rows'; 'geo': per layer the seven WideGeo values}."""
    k = [int(v) for v in m.get_debug('kernels', 4 * ML + 12)]
    g = [int(v) for v in m.get_debug('wide_geo', 7 * ML)]
    return dict(fwd=tuple(k[:L]), bwd=tuple(k[ML:ML + L]), use=tuple(k[3 * ML:3 * ML + L]), update=k[4 * ML + 8], chunks=k[4 * ML + 9],
                wide_dense=k[4 * ML + 10], finish_rows=k[4 * ML + 11], geo=tuple(tuple(g[7 * l:7 * l + 7]) for l in range(L)),
                past=(k[L:ML], g[7 * L:]))


def ms_of(B, T):
    """M per step: B, then a live batch that ends inside a 64-row tile (and empties the later row tiles), a last step of 5 rows."""
    M = np.full(T, B, dtype=np.int32)
    M[T // 2:] = B - 37 if B > 48 else max(1, B - 1)
    M[-1] = min(5, B)
    return M


def ragged_plan(o, I, B, T, Ms=None, seed=77):
    plan = random_plan(I, B, T, seed=seed, tail=True)
    plan['M'][:] = ms_of(B, T) if Ms is None else np.asarray(Ms, dtype=np.int32)
    k = min(6, B // 2)      # items repeated between inputs, targets and negatives
    plan['in_idx'][:, :k] = o.ST[0][:k]
    plan['out_idx'][:, k:2 * k] = plan['in_idx'][:, :k]
    plan['in_idx'][:, 0] = plan['out_idx'][:, 0]      # (inside the last step's five rows as well)
    return plan


def build(I, B, ns, T, env, use_graph=0, **kw):
    clean = dict.fromkeys(SWITCHES)
    clean.update(env)
    with _env(**clean):
        o, m = make_pair(I, B, ns, store_rows=T + 1, use_graph=use_graph, **kw)
    return o, m


def n_cu(m):
    return int(m.get_debug('n_cu', 1)[0])


def run(tag, I, B, ns, T, env, want, Ms=None, plan_fix=None, check=None, need_cus=None, **kw):
    """want: {key of selection(): expected value}, asserted before anything runs.  plan_fix(o, plan): edits of the plan; check(o, m,
    plan): extra assertions on the device state after the last step.  need_cus: the CU count the expected geometry was derived for."""
    o, m = build(I, B, ns, T, env, **kw)
    try:
        if need_cus is not None and n_cu(m) != need_cus:
            pytest.skip('the expected geometry is that of a %d-CU device; this one has %d CUs' % (need_cus, n_cu(m)))
        sel = selection(m, len(o.layers))
        assert not any(sel['past'][0]) and not any(sel['past'][1]), sel['past']
        for key, val in want.items():
            assert sel[key] == val, '%s: %s is %s, expected %s (selection %s)' % (tag, key, sel[key], val, sel)
        twin = kink_twin(o)
        plan = ragged_plan(o, I, B, T, Ms)
        if plan_fix is not None:
            plan_fix(o, plan)
        m.set_plan(plan)
        want_cost, kink = oracle_steps(o, plan, T, twin=twin)
        assert np.isfinite(want_cost).all(), want_cost
        m.train_steps(0, T)
        errs = []
        report('--- wide edge %s (geo %s, fwd %s, bwd %s, update %d, wide_dense %d, finish_rows %d)' % (
            tag, sel['geo'], sel['fwd'], sel['bwd'], sel['update'], sel['wide_dense'], sel['finish_rows']))
        close('loss curve', m.get_losses(0, T), np.array(want_cost), atol=5e-6, rtol=5e-4, errs=errs)
        compare_params(o, m, errs, tag, Mrows=int(plan['M'][-1]), loosen=1.0, skip_items=kink, twin=twin if kink else None)
        if check is not None:
            check(o, m, plan)
        assert not errs, errs
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------------------------- the largest layer
MAXW = dict(I=2000, B=64, ns=256, T=6, env={}, need_cus=RECORDED_CUS, loss='bpr-max', final_act='elu-0.5', bpreg=0.5, learning_rate=0.01,
            constrained_embedding=True, layers=(1024,))
MAXW_WANT = dict(fwd=(FWD_P1S,), bwd=(BWD_BW,), geo=((9, 8, 8, 128, 128, 16, 192),), wide_dense=1, chunks=4, update=UP_SPLIT, finish_rows=0)


@pytest.mark.parametrize('de,dh', [(0.0, 0.0), (0.3, 0.2)])
def test_max_width(de, dh):
    """layers = (1024,), the largest g4r_create accepts, B = 64, constrained, under the DEFAULT policy (no switch set): k_gru_gate adds 8
    input + 8 hidden slices (vc[8], vr[16], vz[16] full), finish_rows 16 planes of dy (v[16] full), item rows of four chunks.
    Selection: fwd FWD_P1S, bwd BWD_BW, wide_geo (use 9, ny 8, nh 8, kys 128, khs 128, bbn 16, bbk 192 -- the dy slices are 256 CUs / 16
    tiles: skipped on another CU count), wide_dense 1, chunks 4, update UP_SPLIT, finish_rows 0 (k_dense_grad2 finishes the rows).
    Learning rate 0.01: the oracle stays finite at this width (test_gpu_widths.py needed it at 640).  With and without embedding (0.3) and
    hidden (0.2) dropout."""
    run('mw e%.1f' % de, want=MAXW_WANT, dropout_p_embed=de, dropout_p_hidden=dh, **MAXW)


def test_max_width_graph_replay_is_bit_identical_to_eager():
    """test_max_width's model (same selection asserted) as a graph replay (use_graph = 1) and as eager launches: the same bits in the
    losses, Wy, Wx, Bh and acc_Wh (16 + 16 slices added in slice order by whichever workgroup gets there)."""
    kw = dict(MAXW, dropout_p_embed=0.3, dropout_p_hidden=0.2)
    I, B, ns, T, env, cus = (kw.pop(n) for n in ('I', 'B', 'ns', 'T', 'env', 'need_cus'))
    outs = []
    for g in (0, 1):
        o, m = build(I, B, ns, T, env, use_graph=g, **dict(kw))
        try:
            if n_cu(m) != cus:
                pytest.skip('the expected geometry is that of a %d-CU device; this one has %d CUs' % (cus, n_cu(m)))
            sel = selection(m, len(o.layers))
            for key, val in MAXW_WANT.items():
                assert sel[key] == val, (key, sel)
            m.set_plan(ragged_plan(o, I, B, T))
            m.train_steps(0, T)
            outs.append((m.get_losses(0, T).copy(), m.get_param('Wy', (I, 1024)).copy(), m.get_param('Wx', (1024, 3072), 0).copy(),
                         m.get_param('Bh', (3072,), 0).copy(), m.get_param('acc_Wh', (1024, 1024), 0).copy()))
        finally:
            m.close()
    assert np.isfinite(outs[0][0]).all()
    for a, b in zip(outs[0], outs[1]):
        np.testing.assert_array_equal(a, b)


# ---------------------------------------------------------------------------------------------------------------- dy slices
D512 = dict(I=3000, B=96, ns=512, T=7, constrained_embedding=True, layers=(512,), **XE)


def test_dy_16_slices():
    """layers = (512,), B = 96, G4R_WIDE2 = 25, G4R_BB_KS = 96: 3 D / 96 = 16 dy slices of three ring stages each, the most the guard
    cdiv(3 D, ks) <= 16 lets through; finish_rows' v[16] full.  Selection: fwd FWD_P1S, bwd BWD_BW, wide_geo (use 9, ny 4, nh 4, kys 128,
    khs 128, bbn 16, bbk 96), wide_dense 1, finish_rows 0.  Report tag `dy16` (tests/test_gpu_mutation.py, mutant 29)."""
    run('dy16', env=dict(G4R_WIDE2=ALL, G4R_BB_KS=96), want=dict(fwd=(FWD_P1S,), bwd=(BWD_BW,), geo=((9, 4, 4, 128, 128, 16, 96),),
                                                                 wide_dense=1, finish_rows=0, update=UP_SPLIT), **D512)


def test_dy_one_past_16_slices():
    """The same model with G4R_BB_KS = 64: 24 slices, past the guard.  The layer keeps k_gru_p1s (use & 1) and hands dy back to
    k_gru_bwd_b.  Selection: fwd FWD_P1S, bwd BWD_B, wide_geo (use 1, ny 4, nh 4, kys 128, khs 128, bbn 1, bbk 0 -- WideGeo's defaults),
    wide_dense 1, finish_rows 0."""
    run('dy24', env=dict(G4R_WIDE2=ALL, G4R_BB_KS=64), want=dict(fwd=(FWD_P1S,), bwd=(BWD_B,), use=(1,), geo=((1, 4, 4, 128, 128, 1, 0),),
                                                                 wide_dense=1, finish_rows=0), **D512)


def test_two_stage_slices():
    """layers = (256,), B = 96, G4R_BB_KS = 64: 12 dy slices of 64 = two stages of gemm_tile3<3, 32> -- the prologue fills the ring and no
    stage is issued inside the loop.  Selection: fwd FWD_P1S, bwd BWD_BW, wide_geo (use 9, ny 2, nh 2, kys 128, khs 128, bbn 12, bbk 64),
    wide_dense 1.  Report tag `st2` (the green side of mutant 29: 12 planes)."""
    run('st2', I=3000, B=96, ns=512, T=7, env=dict(G4R_WIDE2=ALL, G4R_BB_KS=64),
        want=dict(fwd=(FWD_P1S,), bwd=(BWD_BW,), geo=((9, 2, 2, 128, 128, 12, 64),), wide_dense=1, finish_rows=0),
        constrained_embedding=True, layers=(256,), **BPRMAX)


def test_short_last_slice():
    """layers = (320,), B = 96, G4R_BB_KS = 128: 3 D = 960 = 7 slices of 128 (four stages: the ring wraps) and a last one of 64; phase 1 in
    three slices of 112 (320 = 112 + 112 + 96: a short last slice there as well).  Selection: fwd FWD_P1S, bwd BWD_BW, wide_geo (use 9,
    ny 3, nh 3, kys 112, khs 112, bbn 8, bbk 128), wide_dense 1, chunks 2."""
    run('short', I=3000, B=96, ns=512, T=7, env=dict(G4R_WIDE2=ALL, G4R_BB_KS=128),
        want=dict(fwd=(FWD_P1S,), bwd=(BWD_BW,), geo=((9, 3, 3, 112, 112, 8, 128),), wide_dense=1, chunks=2),
        constrained_embedding=True, layers=(320,), dropout_p_embed=0.2, **BPRMAX)


# ---------------------------------------------------------------------------------------------------------------- input widths
@pytest.mark.parametrize('E', [64, 80, 144])
def test_input_width(E):
    """A separate embedding of E columns under layers = (256,), B = 80 (a 64-row tile and one of 16 rows), embedding dropout 0.3,
    G4R_WIDE2 = 25.  E = 64: the minimum, one column tile of k_gru_bwd_bw, one input slice.  E = 80: a partial second column tile
    (n0 + r < IN), 20 quads per row in finish_rows, one input slice of five 16-deep chunks.  E = 144: two uneven input slices (80 + 64):
    the Philox counter (ks + 16 i + sc) >> 2 of k_gru_p1s' mask must agree with the (row, c4 >> 2) of the mask finish_rows regenerates.
    Selection: fwd FWD_P1S, bwd BWD_BW, wide_geo (use 9, ny 1 / 1 / 2, nh 2, kys 64 / 80 / 80, khs 128, bbn 6, bbk 128), wide_dense 1,
    chunks 1.  Report tags `in64`, `in80`, `in144` (mutant 30: red at 144, green at 80)."""
    ny, kys = {64: (1, 64), 80: (1, 80), 144: (2, 80)}[E]
    run('in%d' % E, I=2500, B=80, ns=384, T=7, env=dict(G4R_WIDE2=ALL),
        want=dict(fwd=(FWD_P1S,), bwd=(BWD_BW,), geo=((9, ny, 2, kys, 128, 6, 128),), wide_dense=1, chunks=1, finish_rows=0),
        constrained_embedding=False, embedding=E, layers=(256,), dropout_p_embed=0.3, **BPRMAX)


@pytest.mark.parametrize('E', [48, 72])
def test_input_width_off_the_wide_path(E):
    """E = 48 (below 64) and E = 72 (no multiple of 16) under the same model and switches: the layer falls back to the round-1 kernels
    as a whole.  Selection: fwd FWD_P1_N64, bwd BWD_B, wide_geo WideGeo's defaults (use 0, ny 1, nh 1, kys 0, khs 0, bbn 1, bbk 0),
    finish_rows 0."""
    run('in%d' % E, I=2500, B=80, ns=384, T=7, env=dict(G4R_WIDE2=ALL),
        want=dict(fwd=(FWD_P1_N64,), bwd=(BWD_B,), use=(0,), geo=(OFF,), finish_rows=0),
        constrained_embedding=False, embedding=E, layers=(256,), dropout_p_embed=0.3, **BPRMAX)


# ---------------------------------------------------------------------------------------------------------------- the layer below
@pytest.mark.parametrize('dh', [0.0, 0.2])
def test_lean_layer_below_a_wide_one(dh):
    """Embedding 64, layers = (64, 256), B = 64, G4R_WIDE2 = 25: layer 0 runs the lean launches and its k_gru_da adds up the six planes of
    dy that layer 1's k_gru_bwd_bw leaves; k_dense_grad2 takes the tiles of both layers.  Selection: fwd (FWD_LEAN, FWD_P1S), bwd
    (BWD_LEAN, BWD_BW), wide_geo layer 0 the defaults, layer 1 (use 9, ny 1, nh 2, kys 64, khs 128, bbn 6, bbk 128), wide_dense 1.  Both
    hidden-dropout states (k_gru_da regenerates the mask on the sum)."""
    run('lw h%.1f' % dh, I=2500, B=64, ns=384, T=7, env=dict(G4R_WIDE2=ALL),
        want=dict(fwd=(FWD_LEAN, FWD_P1S), bwd=(BWD_LEAN, BWD_BW), geo=(OFF, (9, 1, 2, 64, 128, 6, 128)), wide_dense=1, update=UP_SPLIT),
        constrained_embedding=False, embedding=64, layers=(64, 256), dropout_p_hidden=dh, dropout_p_embed=0.1, **BPRMAX)


def test_three_launch_layer_below_a_wide_one():
    """Embedding 64, layers = (144, 256), B = 64, hidden dropout 0.2: layer 0 (D = 144: neither lean nor fused nor wide) runs k_gru_bwd_pre /
    _a / _b and k_gru_bwd_pre adds up layer 1's dy planes; layer 1 reads 144 inputs as slices of 80 + 64.  Selection: fwd (FWD_P1_N32,
    FWD_P1S), bwd (BWD_B, BWD_BW), wide_geo layer 0 the defaults, layer 1 (use 9, ny 2, nh 2, kys 80, khs 128, bbn 6, bbk 128)."""
    run('tw', I=2500, B=64, ns=384, T=7, env=dict(G4R_WIDE2=ALL),
        want=dict(fwd=(FWD_P1_N32, FWD_P1S), bwd=(BWD_B, BWD_BW), geo=(OFF, (9, 2, 2, 80, 128, 6, 128)), wide_dense=1),
        constrained_embedding=False, embedding=64, layers=(144, 256), dropout_p_hidden=0.2, **BPRMAX)


def test_fused_layer_below_a_wide_one():
    """Embedding 64, layers = (112, 256), B = 64, G4R_NO_LEAN = 1: layer 0 runs k_gru_bwd_fused, which adds no planes, so layer 1 has no
    consumer for sliced dy: it keeps k_gru_p1s (one input slice of 112) and hands dy back to k_gru_bwd_b.  Selection: fwd (FWD_FUSED,
    FWD_P1S), bwd (BWD_FUSED, BWD_B), use (0, 1), wide_geo layer 0 the defaults, layer 1 (use 1, ny 1, nh 2, kys 112, khs 128, bbn 1, bbk 0)."""
    run('fw', I=2500, B=64, ns=384, T=7, env=dict(G4R_WIDE2=ALL, G4R_NO_LEAN=1),
        want=dict(fwd=(FWD_FUSED, FWD_P1S), bwd=(BWD_FUSED, BWD_B), use=(0, 1), geo=(OFF, (1, 1, 2, 112, 128, 1, 0)), wide_dense=1),
        constrained_embedding=False, embedding=64, layers=(112, 256), dropout_p_hidden=0.2, **BPRMAX)


# ---------------------------------------------------------------------------------------------------------------- k_finish_rows alone
M8_B, M8_NS = 96, 512


def _m8_plan(o, plan):
    """The last step (M = 5): rows 0 and 1 read the same item, row 2 an item that no other input, no target and no stored negative is."""
    t = len(plan['M']) - 1
    used = set(o.ST.ravel().tolist()) | set(plan['out_idx'][t].tolist()) | set(plan['in_idx'][t].tolist())
    lone = [i for i in range(o.n_items) if i not in used]
    assert lone, 'every item is a stored negative: no input can occur once'
    plan['in_idx'][t, 1] = plan['in_idx'][t, 0]
    plan['in_idx'][t, 2] = lone[0]


def _m8_check(o, m, plan):
    occ = m.get_debug('occ_idx', 2 * M8_B + M8_NS).view(np.int32)      # X (B, -1 past M) | B targets | the step's negatives
    M = int(plan['M'][-1])
    x = occ[:M]
    assert (occ[M:M8_B] == -1).all() and (x >= 0).all(), occ[:M8_B]
    counts = [int((occ == i).sum()) for i in x]
    report('mask 8: occurrences of the last step\'s inputs %s' % counts)
    # finish_rows: an item that occurs once takes its accumulator in place (cnt1 == 1), any other goes through dAx
    assert 1 in counts and max(counts) > 1, counts


def test_mask8_alone():
    """layers = (256,), constrained, B = 96, embedding dropout 0.3, G4R_WIDE2 = 8 -- the default policy's choice at D = 256: k_gru_bwd_bw
    leaves six dy planes, k_finish_rows adds them up as a launch of its own in front of the merged k_update.  Selection: fwd FWD_P1_N64,
    bwd BWD_BW, wide_geo (use 8, ny 1, nh 1, kys 0, khs 0, bbn 6, bbk 128), wide_dense 0, finish_rows 1, update UP_MERGED.  The last step's
    occurrence list (occ_idx) holds an input item that occurs once and one that occurs several times: both branches of finish_rows'
    accumulator store (in place / dAx) are taken."""
    run('m8', I=3000, B=M8_B, ns=M8_NS, T=7, env=dict(G4R_WIDE2=8), plan_fix=_m8_plan, check=_m8_check,
        want=dict(fwd=(FWD_P1_N64,), bwd=(BWD_BW,), geo=((8, 1, 1, 0, 0, 6, 128),), wide_dense=0, finish_rows=1, update=UP_MERGED),
        constrained_embedding=True, layers=(256,), dropout_p_embed=0.3, **BPRMAX)


# ---------------------------------------------------------------------------------------------------------------- row tiles
ROW_MS = {3: (3, 3, 3, 2, 2, 1), 64: (64, 64, 63, 33, 27, 5), 65: (65, 65, 64, 63, 28, 5), 129: (129, 128, 65, 64, 63, 5)}


@pytest.mark.parametrize('B', sorted(ROW_MS))
def test_row_tiles(B):
    """layers = (256,), constrained, hidden dropout 0.2, G4R_WIDE2 = 25, B = 3 (one tile of three rows), 64 (one full tile), 65 and 129 (a
    last 64-row tile that holds ONE row), with a live batch that shrinks tile by tile (B = 129: M = 129, 128, 65, 64, 63, 5): whole row
    tiles return early (m0 >= M) in k_gru_p1s and k_gru_bwd_bw, and k_gru_gate / finish_rows / k_dense_grad2 stop at row M.  Selection:
    fwd FWD_P1S, bwd BWD_BW, wide_geo (use 9, ny 2, nh 2, kys 128, khs 128, bbn 6, bbk 128), wide_dense 1.  (B = 3 at learning rate 0.02:
    at 0.1 three rows that revisit one item every step diverge -- the ORACLE's cost goes 0.70, 0.55, 1.6, 0.49, 7.4, 65 -- and a run that
    blows up measures how rounding is amplified, not the kernels.)"""
    kw = dict(BPRMAX, learning_rate=0.02) if B == 3 else BPRMAX
    run('rt%d' % B, I=2000, B=B, ns=256, T=6, env=dict(G4R_WIDE2=ALL), Ms=ROW_MS[B],
        want=dict(fwd=(FWD_P1S,), bwd=(BWD_BW,), use=(9,), geo=((9, 2, 2, 128, 128, 6, 128),), wide_dense=1, finish_rows=0),
        constrained_embedding=True, layers=(256,), dropout_p_hidden=0.2, **kw)


# ---------------------------------------------------------------------------------------------------------------- k_dense_grad2's L2 term
@pytest.mark.parametrize('opt', ['l2', 'momentum_l2'])
def test_dense_grad2_l2(opt):
    """layers = (256,), B = 96, lmbd = 0.01, without and with momentum 0.3, G4R_WIDE2 = 25: the L2 term of k_dense_grad2's two in-place
    epilogues (64 x 64 tile and bias row): p (1 - lr lmbd) - lr g / sqrt(acc), and with momentum v = mom v - lr (g / sqrt(acc) + lmbd p).
    Selection: fwd FWD_P1S, bwd BWD_BW, wide_geo (use 9, ny 2, nh 2, kys 128, khs 128, bbn 6, bbk 128), wide_dense 1, update UP_SPLIT."""
    kw = dict(lmbd=0.01, momentum=0.3) if opt == 'momentum_l2' else dict(lmbd=0.01)
    run(opt[:6], I=3000, B=96, ns=512, T=7, env=dict(G4R_WIDE2=ALL),
        want=dict(fwd=(FWD_P1S,), bwd=(BWD_BW,), geo=((9, 2, 2, 128, 128, 6, 128),), wide_dense=1, update=UP_SPLIT),
        constrained_embedding=True, layers=(256,), **dict(BPRMAX, **kw))

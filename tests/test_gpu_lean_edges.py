"""Oracle parity of the narrow-layer lean launches (g4r_lean_kernels.cuh: k_gru_v / k_gru_h / k_gru_da / k_gru_dy, k_score_s /
k_score_b, k_update_l) on the shapes they are written around: in = D = LN_MAXD (eight 16-deep super-steps) and one step past it,
k_score_b's bias column alone in its 64-wide d block (D = 64, 128) or sharing the last one (D = 60, 124), partial 16 x 16 tiles
(D = 20, 36; B = 17, 33), an embedding width unlike D at both extremes, two lean layers, the B = 128 / 129 boundary where
k_score_b and k_update_l switch off but k_score_s keeps running, score rows that end inside a 32-column tile / 128-column slab,
an item whose owner scan in k_update_l reaches a second 1024-id slice, items whose occurrences are all sampled negatives, and
k_update_l's momentum and L2 paths.

Every case first asserts the selection (get_debug('lean'): bit l = lean_gru of layer l, lean_scores, lean_score_bwd, lean_update,
computed from the predicates launch_step dispatches on), so that a predicate change which moves a shape off the lean path turns
it red instead of quietly testing the fallback.  Then a few steps with a ragged tail (a live batch that ends inside a 16-row and a
32-row tile, a last step with M = 5, items repeated between input and negatives) against OracleGRU4Rec, with the tolerances of
test_gpu_dma_tiles.py: per-step cost rtol 5e-4 + atol 5e-6, parameters / accumulators / velocities by compare_params.  Both
hidden-dropout states: the lean kernels regenerate the Philox masks in the forward and in the backward."""
import numpy as np
import pytest

from test_gpu_parity import close, compare_params, kink_twin, make_pair, oracle_steps, random_plan, report

pytestmark = pytest.mark.gpu

DROP = [0.0, 0.25]


def _ragged_plan(o, I, B, T, seed=77, repeat=True, items=None):
    plan = random_plan(I, B, T, seed=seed, tail=True)
    if items is not None:      # inputs and targets drawn from `items` only
        rng = np.random.RandomState(seed + 1)
        plan['in_idx'] = rng.choice(items, size=(T, B)).astype(np.int32)
        plan['out_idx'] = rng.choice(items, size=(T, B)).astype(np.int32)
    plan['M'][:] = B
    plan['M'][T // 2:] = B - 37 if B > 48 else B - 3      # ends inside a 16-row and inside a 32-row tile
    plan['M'][-1] = 5
    if repeat:
        plan['in_idx'][:, :6] = o.ST[0][:6]      # items repeated between input and negatives
        plan['out_idx'][:, 6:12] = plan['in_idx'][:, :6]
    return plan


def lean_selection(m):
    return tuple(int(v) for v in m.get_debug('lean', 4))


def _run(tag, I, B, ns, T, store_rows, want, repeat=True, items=None, check=None, support=None, **kw):
    """want: the expected lean selection (layer bitmask, lean_scores, lean_score_bwd, lean_update).  check(o, m, plan): extra
    assertions on the device state after the last step."""
    o, m = make_pair(I, B, ns, store_rows=store_rows, support=support, **kw)
    try:
        sel = lean_selection(m)
        assert sel == tuple(want), '%s: lean selection %s, expected %s' % (tag, sel, tuple(want))
        twin = kink_twin(o)
        plan = _ragged_plan(o, I, B, T, repeat=repeat, items=items)
        m.set_plan(plan)
        want_cost, kink = oracle_steps(o, plan, T, twin=twin)
        m.train_steps(0, T)
        errs = []
        report('--- lean %s (selection %s)' % (tag, sel))
        close('loss curve', m.get_losses(0, T), np.array(want_cost), atol=5e-6, rtol=5e-4, errs=errs)
        compare_params(o, m, errs, tag, Mrows=int(plan['M'][-1]), skip_items=kink, twin=twin if kink else None)
        if check is not None:
            check(o, m, plan)
        assert not errs, errs
    finally:
        m.close()


def _occ(m, B, ns):
    """The occurrence list of the last step: X (B, -1 past M) | score columns (B targets, ns samples)."""
    return m.get_debug('occ_idx', 2 * B + ns).view(np.int32)


@pytest.mark.parametrize('dh', DROP)
def test_k_at_the_limit(dh):
    """in = D = LN_MAXD = 128: eight 16-deep super-steps in k_gru_v / k_gru_h / k_gru_dy, eight drp planes summed by k_gru_dy."""
    _run('K128 dh%.2f' % dh, I=5000, B=128, ns=1000, T=8, store_rows=12, want=(1, 1, 1, 1), loss='bpr-max', final_act='elu-0.5',
         constrained_embedding=True, layers=(128,), learning_rate=0.1, bpreg=0.5, dropout_p_hidden=dh)


@pytest.mark.parametrize('dh', DROP)
def test_one_step_past_the_limit_falls_back(dh):
    """D = 132 > LN_MAXD: the GRU and the scoring pair take the older kernels (k_update_l only needs rows of <= 256 floats)."""
    _run('D132 dh%.2f' % dh, I=5000, B=128, ns=1000, T=8, store_rows=12, want=(0, 0, 0, 1), loss='bpr-max', final_act='elu-0.5',
         constrained_embedding=True, layers=(132,), learning_rate=0.1, bpreg=0.5, dropout_p_hidden=dh)


@pytest.mark.parametrize('dh', DROP)
@pytest.mark.parametrize('D', [60, 64, 124, 128])
def test_bias_column_block(D, dh):
    """k_score_b role A adds a ones column at d == D in 64-wide d blocks: alone in an extra block at D = 64 / 128, inside the last
    data block (zeros behind it) at D = 60 / 124.  dBy and acc_By carry what that column computes."""
    _run('bias D=%d dh%.2f' % (D, dh), I=6000, B=96, ns=700, T=8, store_rows=12, want=(1, 1, 1, 1), loss='cross-entropy',
         final_act='softmax', constrained_embedding=True, layers=(D,), learning_rate=0.07, logq=1.0, dropout_p_hidden=dh)


@pytest.mark.parametrize('dh', DROP)
@pytest.mark.parametrize('B', [17, 33])
@pytest.mark.parametrize('D', [20, 36])
def test_partial_16_tiles(D, B, dh):
    """D % 16 != 0 and B % 16 != 0: partial 16 x 16 tiles in every lean launch."""
    _run('partial D=%d B=%d dh%.2f' % (D, B, dh), I=900, B=B, ns=150, T=8, store_rows=12, want=(1, 1, 1, 1), loss='top1-max',
         final_act='tanh', constrained_embedding=True, layers=(D,), learning_rate=0.1, dropout_p_hidden=dh)


@pytest.mark.parametrize('dh', DROP)
@pytest.mark.parametrize('E,D', [(128, 4), (4, 128)])
def test_embedding_unlike_the_layer(E, D, dh):
    """in != D in k_gru_v / k_gru_dy at both extremes (IN >= 4 is in the predicate); the embedding table E takes the X rows."""
    _run('emb E=%d D=%d dh%.2f' % (E, D, dh), I=3000, B=64, ns=400, T=8, store_rows=12, want=(1, 1, 1, 1), loss='bpr-max',
         final_act='elu-0.5', constrained_embedding=False, embedding=E, layers=(D,), learning_rate=0.1, bpreg=0.5, dropout_p_hidden=dh,
         dropout_p_embed=0.1)


@pytest.mark.parametrize('dh', DROP)
def test_two_lean_layers(dh):
    """layers (36, 124): layer 1 reads layer 0's output, its dy feeds k_gru_da of layer 0."""
    _run('two layers dh%.2f' % dh, I=4000, B=64, ns=500, T=8, store_rows=12, want=(3, 1, 1, 1), loss='bpr-max', final_act='linear',
         constrained_embedding=True, layers=(36, 124), learning_rate=0.1, bpreg=0.5, dropout_p_hidden=dh)


@pytest.mark.parametrize('dh', DROP)
@pytest.mark.parametrize('B', [128, 129])
def test_batch_boundary(B, dh):
    """B = 129: k_score_s keeps running, k_score_b and k_update_l hand over to k_score_bwd / k_update.  Both sides match the oracle."""
    _run('B=%d dh%.2f' % (B, dh), I=6000, B=B, ns=900, T=8, store_rows=12, want=(1, 1, 1, 1) if B <= 128 else (1, 1, 0, 0),
         loss='cross-entropy', final_act='softmax', constrained_embedding=True, layers=(64,), learning_rate=0.07, logq=1.0,
         dropout_p_hidden=dh)


@pytest.mark.parametrize('ns', [925, 955, 1051])
def test_score_row_not_whole_tiles(ns):
    """B = 100: N = B + ns = 1025 / 1055 / 1151 live columns, N % 128 = 1 / 31 / 127 (ldSc, N rounded up to 16, is 1040 / 1056 /
    1152): the last 32-column tile of k_score_s and the last 128-column slab of k_score_b are partial or end in padding."""
    _run('ldSc ns=%d' % ns, I=8000, B=100, ns=ns, T=8, store_rows=12, want=(1, 1, 1, 1), loss='bpr-max', final_act='elu-0.5',
         constrained_embedding=True, layers=(48,), learning_rate=0.1, bpreg=0.5)


HOT_B, HOT_NS = 128, 2048


def _check_hot(o, m, plan):
    occ = _occ(m, HOT_B, HOT_NS)
    pos = np.flatnonzero(occ == 0)
    # the owner (last occurrence) of item 0 scans more than 1024 earlier ids, so its scan runs past the first slice
    assert len(pos) - 1 > 1024 and pos[-1] - (pos[0] & ~3) > 2047, (len(pos), pos[:3], pos[-3:])
    report('hot item: %d earlier occurrences over positions [%d, %d]' % (len(pos) - 1, pos[0], pos[-1]))


@pytest.mark.parametrize('dh', DROP)
def test_hot_item_past_1024(dh):
    """An 8-item catalogue with item 0 at ~65 % of the sampling mass, B = 128, 2048 negatives: item 0 occurs ~1370 times per step, its
    owner in k_update_l reads the earlier ids in three 1024-slices.  (Not more concentrated: with ~2000 Adagrad steps of size ~lr on
    one row per step the run diverges, and fp32 rounding differences grow past every bound.  tests/test_gpu_mutation.py: a build that
    drops one id per later slice turns this red on dWy.  The loss and step size are chosen so that the item row's update does not
    cancel to a small difference of ~1400 steps of size lr: there the kernel's order -- the earlier rows summed, then subtracted --
    and the oracle's -- each row added to the parameter in turn -- differ by more than the bound in fp32 alone.)"""
    support = np.ones(8)
    support[0] = 30.0
    _run('hot', I=8, B=HOT_B, ns=HOT_NS, T=6, store_rows=8, want=(1, 1, 1, 1), support=support, check=_check_hot, loss='bpr-max',
         final_act='elu-0.5', constrained_embedding=True, layers=(32,), learning_rate=0.02, bpreg=1.0, dropout_p_hidden=dh)


NEG_B, NEG_NS = 64, 600


def _check_all_negatives(o, m, plan):
    occ = _occ(m, NEG_B, NEG_NS)
    head = set(occ[:2 * NEG_B].tolist())
    tail = occ[2 * NEG_B:]
    only_neg = [i for i in range(4) if i not in head and int((tail == i).sum()) > 1]
    assert only_neg, 'no item was sampled repeatedly as a negative only: the shortcut was not reached'


@pytest.mark.parametrize('dh', DROP)
def test_items_that_are_only_sampled_negatives(dh):
    """Items 0-3 hold most of the sampling mass but never occur as an input or a target: each is sampled dozens of times per step
    and its owner takes the (count - 1) x own row shortcut."""
    I = 500
    support = np.r_[np.full(4, 3000.0), np.random.RandomState(1).randint(1, 40, size=I - 4)]
    _run('all-neg dh%.2f' % dh, I=I, B=NEG_B, ns=NEG_NS, T=8, store_rows=12, want=(1, 1, 1, 1), repeat=False, items=np.arange(4, I),
         support=support, check=_check_all_negatives, loss='bpr-max', final_act='elu-0.5', constrained_embedding=True, layers=(40,),
         learning_rate=0.1, bpreg=0.5, dropout_p_hidden=dh)


@pytest.mark.parametrize('dh', DROP)
@pytest.mark.parametrize('opt', ['momentum', 'l2'])
def test_update_l_optimizer_variants(opt, dh):
    """k_update_l<true> (momentum: velocity rows and the n mom V0 term) and the L2 term (lmbd > 0) of its sparse and dense rules."""
    kw = dict(momentum=0.3) if opt == 'momentum' else dict(lmbd=0.01)
    _run('%s dh%.2f' % (opt, dh), I=700, B=64, ns=256, T=8, store_rows=12, want=(1, 1, 1, 1), loss='bpr-max', final_act='elu-0.5',
         constrained_embedding=True, layers=(36,), learning_rate=0.1, bpreg=0.5, dropout_p_hidden=dh, **kw)


def test_graph_replay_of_the_lean_step_is_bit_identical_to_eager():
    """in = D = 128, ragged tail: the captured step graph (use_graph = 1) and eager launches leave the same bits."""
    I, B, ns, T = 5000, 128, 1000, 12
    kw = dict(loss='bpr-max', final_act='elu-0.5', constrained_embedding=True, layers=(128,), learning_rate=0.1, bpreg=0.5,
              dropout_p_hidden=0.25)
    outs = []
    for g in (0, 1):
        o, m = make_pair(I, B, ns, store_rows=12, use_graph=g, **dict(kw))
        assert lean_selection(m) == (1, 1, 1, 1)
        m.set_plan(_ragged_plan(o, I, B, T))
        m.train_steps(0, T)
        outs.append((m.get_losses(0, T).copy(), m.get_param('Wy', (I, 128)).copy(), m.get_param('acc_Wy', (I, 128)).copy(),
                     m.get_param('By', (I,)).copy(), m.get_param('Wx', (128, 384), 0).copy(), m.get_param('acc_Wh', (128, 128), 0).copy()))
        m.close()
    for a, b in zip(outs[0], outs[1]):
        np.testing.assert_array_equal(a, b)

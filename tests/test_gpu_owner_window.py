"""The owner tables of the lean update written once per window of steps (k_owner_window, g4r_update_kernels.cuh: one launch in front
of a graph replay or of up to 16 eager steps) against the pre-scan inside every step's k_loss_rows launch (G4R_OWNER_WINDOW=0, read at
create): the same rows in the same order, so the same bits -- losses, item tables, accumulators, velocities, dense parameters, H.
T = 23 steps: a 16-step replay, a 4-step replay and three eager steps where the sample store lets a run go that far; the same steps
as two calls (9 + 14) give the same bits again.  Every slot of the owner ring (debug key own_pos_ring) is checked against the host
rule (test_owner_window_rule.py) after one 16-step window; a list too long for the kernel's LDS keeps the pre-scan."""
import os

import numpy as np
import pytest

from test_gpu_parity import make_pair, random_plan
from test_owner_window_rule import check_table, expected_rows, occurrences

T = 23
BPR = dict(loss='bpr-max', final_act='elu-0.5', constrained_embedding=True, learning_rate=0.1, bpreg=1.0)
CASES = {
    # name: (I, B, ns, store_rows, support of item 0 (None: random), M = 0 steps at the end, kwargs)
    'cfg2_shape_refill_at_12': (3000, 128, 2048, 12, None, 0, dict(BPR, layers=(100,))),
    'momentum': (3000, 128, 2048, 24, None, 0, dict(BPR, layers=(100,), momentum=0.3)),
    'no_samples': (150, 64, 0, 0, None, 0, dict(loss='cross-entropy', final_act='softmax', constrained_embedding=True, layers=(48,),
                                                learning_rate=0.1)),
    'two_tables': (400, 96, 512, 24, None, 0, dict(loss='top1-max', final_act='elu-0.5', constrained_embedding=False, embedding=40,
                                                   layers=(64,), learning_rate=0.1)),
    'two_layers_dropout': (900, 128, 1024, 24, None, 0, dict(BPR, layers=(48, 64), bpreg=0.5, dropout_p_hidden=0.2)),
    'hot_item': (8, 128, 2048, 24, 30.0, 0, dict(BPR, layers=(32,), learning_rate=0.02)),
    'ragged_tail_then_empty_steps': (500, 64, 256, 24, None, 2, dict(BPR, layers=(32,))),
}


def _plan(I, B, n_steps, ST, empty=0):
    """test_gpu_owner_lists.py's doctoring, with the sampled items of every step taken from THAT step's row of the store."""
    plan = random_plan(I, B, n_steps, seed=11, tail=True)
    plan['out_idx'][:, 1] = plan['out_idx'][:, 0]          # an item twice in Y
    plan['in_idx'][:, 2] = plan['out_idx'][:, 3]           # an item in X and in Y
    if ST is not None and ST.shape[1] > 8:
        for t in range(n_steps):
            row = ST[t % ST.shape[0]]
            plan['in_idx'][t, :4] = row[:4]                # items in X and among the samples
            plan['out_idx'][t, 4:8] = row[4:8]             # items in Y and among the samples
    if empty:
        plan['M'][-empty:] = 0                             # steps past the tail: nothing is touched
    return plan


class _env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        for k, v in self.kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _make(case, graph, window):
    I, B, ns, store_rows, hot, empty, kw = CASES[case]
    support = None
    if hot is not None:
        support = np.ones(I)
        support[0] = hot
    with _env(G4R_OWNER_WINDOW=None if window else '0', G4R_OWNER_SCAN=None):      # (read at create)
        o, m = make_pair(I, B, ns, store_rows=store_rows, support=support, use_graph=graph, **dict(kw))
    return o, m


def _state(m, I, kw, n_steps):
    D, L = kw['layers'][-1], len(kw['layers'])
    out = {'loss': m.get_losses(0, n_steps).copy()}
    names = ['Wy', 'acc_Wy', 'By', 'acc_By']
    if kw.get('momentum'):
        names += ['vel_Wy', 'vel_By']
    for nm in names:
        out[nm] = m.get_param(nm, (I, D) if nm.endswith('Wy') else (I,)).copy()
    if not kw['constrained_embedding']:
        out['E'] = m.get_param('E', (I, kw['embedding'])).copy()
        out['acc_E'] = m.get_param('acc_E', (I, kw['embedding'])).copy()
    ins = [kw['embedding'] if not kw['constrained_embedding'] else D] + list(kw['layers'][:-1])
    for l in range(L):
        Dl, INl = kw['layers'][l], ins[l]
        for nm, shape in (('Wx', (INl, 3 * Dl)), ('Wh', (Dl, Dl)), ('Wrz', (Dl, 2 * Dl)), ('Bh', (3 * Dl,))):
            out['%s%d' % (nm, l)] = m.get_param(nm, shape, l).copy()
            out['acc_%s%d' % (nm, l)] = m.get_param('acc_' + nm, shape, l).copy()
            if kw.get('momentum'):
                out['vel_%s%d' % (nm, l)] = m.get_param('vel_' + nm, shape, l).copy()
    return out


def _run(case, graph, window, calls=(T,)):
    I, B, ns, store_rows, hot, empty, kw = CASES[case]
    o, m = _make(case, graph, window)
    try:
        assert int(m.get_debug('lean', 4)[3]) == 1, 'k_update_l was not chosen for %s' % case
        assert int(m.get_debug('owner_window', 1)[0]) == (1 if window else 0)
        m.set_plan(_plan(I, B, T, o.ST if ns else None, empty))
        t = 0
        for n in calls:
            m.train_steps(t, n)
            t += n
        assert t == T
        out = _state(m, I, kw, T)
        for l, Dl in enumerate(kw['layers']):
            out['H%d' % l] = m.get_param('H', (B, Dl), l).copy()
        return out
    finally:
        m.close()


def _same_bits(got, ref):
    assert sorted(got) == sorted(ref)
    for k in ref:
        np.testing.assert_array_equal(got[k].view(np.uint32), ref[k].view(np.uint32), err_msg=k)


@pytest.mark.gpu
@pytest.mark.parametrize('graph', [0, 1])
@pytest.mark.parametrize('case', sorted(CASES))
def test_window_tables_bit_identical_to_the_pre_scan_in_the_step(case, graph):
    ref = _run(case, graph, window=False)
    got = _run(case, graph, window=True)
    assert np.isfinite(ref['loss']).all()
    _same_bits(got, ref)
    _same_bits(_run(case, graph, window=True, calls=(9, 14)), ref)


RING = dict(I=3000, B=128, ns=2048, store_rows=20, n_steps=16)      # one 16-step graph window, no refill inside it


def _ring_plan(ST):
    return _plan(RING['I'], RING['B'], RING['n_steps'], ST)


def check_every_slot():
    """One 16-step graph window at the cfg #2 shape: the table of EVERY slot of the owner ring against the host rule for that step's
    plan row and store row.  Returns the number of steps in which an owner read a list."""
    I, B, ns, rows, n_steps = RING['I'], RING['B'], RING['ns'], RING['store_rows'], RING['n_steps']
    with _env(G4R_OWNER_WINDOW=None, G4R_OWNER_SCAN=None):
        o, m = make_pair(I, B, ns, store_rows=rows, use_graph=1, **dict(BPR, layers=(100,)))
    try:
        assert int(m.get_debug('owner_window', 1)[0]) == 1
        plan = _ring_plan(o.ST)
        # on the CPU, before anything runs: the doctored plan gives every step with M >= 8 an owner that reads a list
        occs = [occurrences(plan, o.ST, t, t % rows, B, ns) for t in range(n_steps)]
        want_lists = [sum(1 for n, _ in expected_rows(occ, B, True).values() if n > 0) for occ in occs]
        assert all(w > 0 for w, M in zip(want_lists, plan['M']) if M >= 8) and sum(1 for w in want_lists if w > 0) >= 12, want_lists
        m.set_plan(plan)
        m.train_steps(0, n_steps)
        assert int(m.get_debug('graph_mode', 1)[0]) == 1
        R = 2 * B + ns
        ring = m.get_debug('own_pos_ring', (16 * 16 * R,)).view(np.int32).reshape(16, R, 16)
        last = m.get_debug('own_pos', (16 * R,)).view(np.int32).reshape(R, 16)
        np.testing.assert_array_equal(last, ring[n_steps - 1])
        occ_dev = m.get_debug('occ_idx', (R,)).view(np.int32)
        np.testing.assert_array_equal(occ_dev, occs[-1])      # the host's list of the last step is the device's
        steps_with_lists = 0
        for t in range(n_steps):
            steps_with_lists += 1 if check_table(ring[t], occs[t], B, True) > 0 else 0
        return steps_with_lists
    finally:
        m.close()


@pytest.mark.gpu
def test_every_slot_of_the_ring_holds_its_steps_owner_rows():
    assert check_every_slot() >= 12


@pytest.mark.gpu
def test_a_list_past_the_lds_cap_keeps_the_pre_scan():
    """R = 2 * 32 + 12288 > 12288 ids: no window launch (owner_window = 0), the pre-scan in k_loss_rows writes the table; bit for bit the
    in-kernel scan of G4R_OWNER_SCAN=1 over 4 steps."""
    I, B, ns, n_steps = 2000, 32, 12288, 4
    kw = dict(BPR, layers=(16,))
    outs = []
    for scan in ('1', None):
        with _env(G4R_OWNER_WINDOW=None, G4R_OWNER_SCAN=scan):
            o, m = make_pair(I, B, ns, store_rows=5, use_graph=1, **dict(kw))
        try:
            assert int(m.get_debug('lean', 4)[3]) == 1
            assert int(m.get_debug('owner_window', 1)[0]) == 0
            m.set_plan(_plan(I, B, n_steps, o.ST))
            m.train_steps(0, n_steps)
            outs.append(_state(m, I, kw, n_steps))
            if scan is None:
                R = 2 * B + ns
                occ = m.get_debug('occ_idx', (R,)).view(np.int32)
                pos = m.get_debug('own_pos', (16 * R,)).view(np.int32).reshape(R, 16)
                assert check_table(pos, occ, B, True) > 0
        finally:
            m.close()
    assert np.isfinite(outs[0]['loss']).all()
    _same_bits(outs[1], outs[0])


@pytest.mark.gpu
def test_a_short_list_keeps_the_pre_scan_unless_the_window_is_asked_for():
    """R = 2 * 32 = 64 ids: the pre-scan would add four workgroups to k_loss_rows, too few to pay for a launch per window, so the default
    is the pre-scan (owner_window = 0); G4R_OWNER_WINDOW=1 asks for the window form at any length.  Both give the same bits over 20
    steps (a 16-step and a 4-step replay)."""
    I, B, n_steps = 60, 32, 20
    kw = dict(loss='cross-entropy', final_act='softmax', constrained_embedding=True, layers=(32,), learning_rate=0.1)
    outs = []
    for asked, want in ((None, 0), ('1', 1)):
        with _env(G4R_OWNER_WINDOW=asked, G4R_OWNER_SCAN=None):
            o, m = make_pair(I, B, 0, store_rows=0, use_graph=1, **dict(kw))
        try:
            assert int(m.get_debug('lean', 4)[3]) == 1
            assert int(m.get_debug('owner_window', 1)[0]) == want
            m.set_plan(_plan(I, B, n_steps, None))
            m.train_steps(0, n_steps)
            outs.append(_state(m, I, kw, n_steps))
            R = 2 * B
            occ = m.get_debug('occ_idx', (R,)).view(np.int32)
            pos = m.get_debug('own_pos', (16 * R,)).view(np.int32).reshape(R, 16)
            assert check_table(pos, occ, B, True) > 0
        finally:
            m.close()
    assert np.isfinite(outs[0]['loss']).all()
    _same_bits(outs[1], outs[0])

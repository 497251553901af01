"""The owner pre-scan of the lean update (g4r_loss_kernel.cuh: owner_prescan, run by extra workgroups of k_loss_rows) against
k_update_l's own scan of the occurrence ids (G4R_OWNER_SCAN=1, read at create): the same rows added in the same order, so the same
bits -- losses, item tables, accumulators, velocities, dense parameters.  Cases: a hot item whose occurrences lie more than 1024
positions apart (three slices), items in X and among the samples, items twice in Y, momentum, n_sample = 0, two item tables, two
layers, graph replay and eager launches.  One step's owner table (debug key own_pos) is also checked against the ordered occurrences
computed on the host from occ_idx."""
import os

import numpy as np
import pytest

from test_gpu_parity import make_pair, random_plan

pytestmark = pytest.mark.gpu

CASES = {
    # name: (I, B, ns, T, store_rows, support item 0 (None: random), kwargs)
    'hot_item_three_slices': (8, 128, 2048, 6, 8, 30.0, dict(loss='bpr-max', final_act='elu-0.5', constrained_embedding=True, layers=(32,),
                                                             learning_rate=0.02, bpreg=1.0)),
    'cfg2_shape_momentum': (3000, 128, 2048, 8, 12, None, dict(loss='bpr-max', final_act='elu-0.5', constrained_embedding=True, layers=(100,),
                                                               learning_rate=0.1, bpreg=1.0, momentum=0.3)),
    'no_samples': (150, 64, 0, 10, 0, None, dict(loss='cross-entropy', final_act='softmax', constrained_embedding=True, layers=(48,),
                                                 learning_rate=0.1)),
    'two_tables': (400, 96, 512, 8, 12, None, dict(loss='top1-max', final_act='elu-0.5', constrained_embedding=False, embedding=40,
                                                   layers=(64,), learning_rate=0.1)),
    'two_layers_dropout': (900, 128, 1024, 8, 12, None, dict(loss='bpr-max', final_act='elu-0.5', constrained_embedding=True, layers=(48, 64),
                                                             learning_rate=0.1, bpreg=0.5, dropout_p_hidden=0.2)),
}


def _plan(I, B, T, ST):
    plan = random_plan(I, B, T, seed=11, tail=True)
    plan['out_idx'][:, 1] = plan['out_idx'][:, 0]          # an item twice in Y
    plan['in_idx'][:, 2] = plan['out_idx'][:, 3]           # an item in X and in Y
    if ST is not None and ST.shape[1] > 8:
        plan['in_idx'][:, :4] = ST[0][:4]                  # items in X and among the samples
        plan['out_idx'][:, 4:8] = ST[0][4:8]               # items in Y and among the samples
    return plan


def _run(case, graph, owner_scan, check_lists=False):
    I, B, ns, T, store_rows, hot, kw = CASES[case]
    support = None
    if hot is not None:
        support = np.ones(I)
        support[0] = hot
    old = os.environ.get('G4R_OWNER_SCAN')
    if owner_scan:
        os.environ['G4R_OWNER_SCAN'] = '1'
    else:
        os.environ.pop('G4R_OWNER_SCAN', None)
    try:
        o, m = make_pair(I, B, ns, store_rows=store_rows, support=support, use_graph=graph, **dict(kw))
    finally:
        if old is None:
            os.environ.pop('G4R_OWNER_SCAN', None)
        else:
            os.environ['G4R_OWNER_SCAN'] = old
    try:
        assert int(m.get_debug('lean', 4)[3]) == 1, 'k_update_l was not chosen for %s' % case
        m.set_plan(_plan(I, B, T, o.ST if ns else None))
        m.train_steps(0, T)
        D, L = kw['layers'][-1], len(kw['layers'])
        out = {'loss': m.get_losses(0, T).copy()}
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
            out['Wx%d' % l] = m.get_param('Wx', (INl, 3 * Dl), l).copy()
            out['acc_Wh%d' % l] = m.get_param('acc_Wh', (Dl, Dl), l).copy()
        if check_lists:
            _check_lists(m, B, ns, kw['constrained_embedding'])
        return out
    finally:
        m.close()


def _owners(occ, B, constrained):
    """Host rule of k_update_l's owners that scan: {owner position: ascending earlier positions}."""
    groups = {}
    for k, item in enumerate(occ.tolist()):
        if item < 0:
            continue
        table = 0 if (constrained or k >= B) else 1
        groups.setdefault((table, item), []).append(k)
    out = {}
    for pos in groups.values():
        if len(pos) > 1 and pos[0] < 2 * B:      # (all occurrences among the sampled negatives: the shortcut, no list)
            out[pos[-1]] = pos[:-1]
    return out


INLINE = 15      # G4R_OWN_INLINE: earlier occurrences an owner-table row holds; more: the owner scans in k_update_l


def _check_lists(m, B, ns, constrained):
    R = 2 * B + ns
    occ = m.get_debug('occ_idx', (R,)).view(np.int32)
    pos = m.get_debug('own_pos', (16 * R,)).view(np.int32).reshape(R, 16)
    owners = _owners(occ, B, constrained)
    assert owners, 'no owner took the scan path in the last step'
    for k, want in owners.items():
        if len(want) > INLINE:
            assert pos[k, 0] == -1, (k, pos[k, 0], len(want))
            continue
        assert pos[k, 0] == len(want), (k, pos[k, 0], len(want))
        np.testing.assert_array_equal(pos[k, 1:1 + len(want)], np.array(want, dtype=np.int32), err_msg='owner %d' % k)


@pytest.mark.parametrize('graph', [0, 1])
@pytest.mark.parametrize('case', sorted(CASES))
def test_owner_lists_bit_identical_to_the_in_kernel_scan(case, graph):
    ref = _run(case, graph, owner_scan=True)
    got = _run(case, graph, owner_scan=False, check_lists=(graph == 0))
    assert np.isfinite(ref['loss']).all()
    for k in ref:
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k)


def test_hot_item_owner_scans_and_the_rest_read_their_rows():
    """The hot item's owner (> 1024 earlier occurrences reaching past the second 1024-id slice) is marked -1 in the owner table and scans
    in k_update_l; every other owner of the step reads its row (_check_lists)."""
    I, B, ns, T, store_rows, hot, kw = CASES['hot_item_three_slices']
    support = np.ones(I)
    support[0] = hot
    os.environ.pop('G4R_OWNER_SCAN', None)
    o, m = make_pair(I, B, ns, store_rows=store_rows, support=support, **dict(kw))
    try:
        m.set_plan(_plan(I, B, T, o.ST))
        m.train_steps(0, 1)
        R = 2 * B + ns
        occ = m.get_debug('occ_idx', (R,)).view(np.int32)
        owners = _owners(occ, B, True)
        k = max(owners, key=lambda q: len(owners[q]))
        p = owners[k]
        assert len(p) > 1024 and p[-1] - (p[0] & ~3) > 2047, (len(p), p[0], p[-1])
        _check_lists(m, B, ns, True)
    finally:
        m.close()

"""k_score_b's role A (dSy, dSBy, the item rows' Adagrad pieces) as extra workgroups of the top layer's k_gru_dy launch (the default where
both lean kernels are chosen; g4r_lean_kernels.cuh: k_gru_dy_a) against the same tiles inside k_score_b (G4R_SCORE_B_SPLIT=0, read at
create): the same instructions per tile, so the same bits -- losses, every parameter, accumulator and velocity table, the hidden state.
Each run is a child process of its own (this file, run as a script, is the worker).  The debug key score_b_split tells which form a model
runs: the default must say 1 and the switch 0, so the comparison cannot be one path with itself.  Shapes: BASELINE configs[0] / [1] / [4]
over a small catalogue, momentum, B = 100 with ragged batches (M < B), D = 64; items shared between X, Y and the samples (a constrained
embedding: one accumulator table under both epilogues of the hosted launch)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = {
    # name: (I, B, ns, T, store_rows, ragged M, kwargs)
    'cfg1_shape': (1500, 32, 0, 10, 0, False, dict(loss='cross-entropy', final_act='softmax', constrained_embedding=True, layers=(100,),
                                                   learning_rate=0.1)),
    'cfg2_shape': (3000, 128, 2048, 8, 12, False, dict(loss='bpr-max', final_act='elu-0.5', constrained_embedding=True, layers=(100,),
                                                       learning_rate=0.1, bpreg=1.0)),
    'cfg5_shape': (3000, 128, 2048, 8, 12, False, dict(loss='top1-max', final_act='elu-0.5', constrained_embedding=True, layers=(100, 100),
                                                       learning_rate=0.1, bpreg=1.0, dropout_p_embed=0.2)),
    'momentum': (2000, 128, 1024, 8, 12, False, dict(loss='bpr-max', final_act='elu-0.5', constrained_embedding=True, layers=(100,),
                                                     learning_rate=0.1, bpreg=1.0, momentum=0.3)),
    'b100_ragged': (900, 100, 600, 10, 12, True, dict(loss='bpr-max', final_act='elu-0.5', constrained_embedding=True, layers=(100,),
                                                      learning_rate=0.1, bpreg=1.0)),
    'd64_two_tables': (700, 96, 512, 8, 12, True, dict(loss='top1-max', final_act='elu-0.5', constrained_embedding=False, embedding=40,
                                                       layers=(64,), learning_rate=0.1)),
}


def _worker(case, graph, out):
    """One run in this process (the library reads G4R_SCORE_B_SPLIT at create) -> every compared array in `out` (.npz)."""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    from test_gpu_parity import make_pair, random_plan
    I, B, ns, T, store_rows, ragged, kw = CASES[case]
    o, m = make_pair(I, B, ns, store_rows=store_rows, use_graph=graph, **dict(kw))
    try:
        plan = random_plan(I, B, T, seed=11, tail=ragged)
        plan['out_idx'][:, 1] = plan['out_idx'][:, 0]          # an item twice in Y
        plan['in_idx'][:, 2] = plan['out_idx'][:, 3]           # an item in X and in Y
        if ns:
            plan['in_idx'][:, 4:8] = o.ST[0][:4]               # items in X and among the samples
            plan['out_idx'][:, 8:12] = o.ST[0][4:8]            # items in Y and among the samples
        m.set_plan(plan)
        m.train_steps(0, T)
        D, L = kw['layers'][-1], len(kw['layers'])
        res = {'moved': m.get_debug('score_b_split', (1,)).copy(), 'lean': m.get_debug('lean', (4,)).copy(), 'loss': m.get_losses(0, T).copy()}
        mom = bool(kw.get('momentum'))
        for nm in ['Wy', 'acc_Wy', 'By', 'acc_By'] + (['vel_Wy', 'vel_By'] if mom else []):
            res[nm] = m.get_param(nm, (I, D) if nm.endswith('Wy') else (I,)).copy()
        if not kw['constrained_embedding']:
            for nm in ['E', 'acc_E'] + (['vel_E'] if mom else []):
                res[nm] = m.get_param(nm, (I, kw['embedding'])).copy()
        ins = [kw['embedding'] if not kw['constrained_embedding'] else D] + list(kw['layers'][:-1])
        for l in range(L):
            Dl, INl = kw['layers'][l], ins[l]
            for pre in ['', 'acc_'] + (['vel_'] if mom else []):
                res['%sWx%d' % (pre, l)] = m.get_param(pre + 'Wx', (INl, 3 * Dl), l).copy()
                res['%sWh%d' % (pre, l)] = m.get_param(pre + 'Wh', (Dl, Dl), l).copy()
                res['%sWrz%d' % (pre, l)] = m.get_param(pre + 'Wrz', (Dl, 2 * Dl), l).copy()
                res['%sBh%d' % (pre, l)] = m.get_param(pre + 'Bh', (3 * Dl,), l).copy()
            res['H%d' % l] = m.get_param('H', (B, Dl), l).copy()
        np.savez(out, **res)
    finally:
        m.close()


if __name__ == '__main__':
    _worker(sys.argv[1], int(sys.argv[2]), sys.argv[3])
    sys.exit(0)

pytestmark = pytest.mark.gpu


def _run(case, graph, split, tmp_path):
    out = str(tmp_path / ('%s_%d_%s.npz' % (case, graph, split)))
    env = dict(os.environ)
    env.pop('G4R_SCORE_B_SPLIT', None)
    if split is not None:
        env['G4R_SCORE_B_SPLIT'] = split
    r = subprocess.run([sys.executable, os.path.abspath(__file__), case, str(graph), out], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    with np.load(out) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize('graph', [0, 1])
@pytest.mark.parametrize('case', sorted(CASES))
def test_hosted_role_a_bit_identical_to_role_a_in_k_score_b(case, graph, tmp_path):
    ref = _run(case, graph, '0', tmp_path)
    got = _run(case, graph, None, tmp_path)
    # both runs take k_score_b and the lean GRU launches; only the default moved role A
    assert int(ref['lean'][2]) == 1 and int(got['lean'][2]) == 1 and (int(got['lean'][0]) >> (len(CASES[case][6]['layers']) - 1)) & 1, (ref['lean'], got['lean'])
    assert int(got['moved'][0]) == 1, 'the default did not move role A into k_gru_dy for %s' % case
    assert int(ref['moved'][0]) == 0, 'G4R_SCORE_B_SPLIT=0 did not keep role A in k_score_b for %s' % case
    assert np.isfinite(ref['loss']).all()
    assert sorted(ref) == sorted(got)
    for k in sorted(ref):
        if k in ('moved',):
            continue
        assert ref[k].dtype == got[k].dtype and ref[k].shape == got[k].shape, k
        np.testing.assert_array_equal(got[k].view(np.uint32), ref[k].view(np.uint32), err_msg=k)

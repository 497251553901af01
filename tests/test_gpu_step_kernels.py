"""The kernels a training step runs, as choose_kernels (g4r_host_model.hpp) decides them at g4r_create, pinned for BASELINE's five
configuration shapes and the switch / optimizer / embedding variants around them (debug key `kernels`; enum values in
g4r_host_model.hpp).

How the expected values were established: the choice used to be re-derived by predicates in four places.  When it became one
value, every case below was run with the library before and after that change: under rocprofv3 --kernel-trace, the kernel-symbol
sequences of one eager step, one replay of the 16-step graph, one profiled step and one profile-split step were equal case for case,
and so were the losses.  The table is what the new library's `kernels` key reported for those runs.  Some values depend on the
device's CU count (k_score_mt / k_score_bmt, the k_score_bwd2 slabs): they were recorded on a 256-CU MI355X, and a device with another
count skips with that reason.  The choice does not read n_items, so the catalogues here are small.  Cases with environment switches
run in a child process.  The key reports kinds, flags and slab counts; the grids built from them are covered by the parity suite."""
import json
import os
import subprocess
import sys

import pytest

from gru4rec_amd import _native

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = dict(layers=[100], batch_size=128, n_sample=2048, loss=1, final_act=4, final_act_p0=0.5, hidden_act=2, embed_mode=0,
            learning_rate=0.1, momentum=0.0, bpreg=1.0, logq=0.0, dropout_p_embed=0.0)
CFG4 = dict(layers=[256], batch_size=512, n_sample=8192)
# case: (model settings, environment, expected).  Expected: per layer (GruFwdKind, GruBwdKind, p2_deep + 2 ba_deep, WideGeo::use),
# then (score_fwd, loss_spec, loss_long, loss_quads, score_bwd, kch, ksplit, bmt_slabs, update, chunks, wide_dense, finish_rows)
CASES = {
    'cfg1': (dict(layers=[100], batch_size=32, n_sample=0, loss=0, final_act=6, bpreg=0.0), {},
             ([(0, 0, 0, 0)], (0, 2, 0, 0, 0, 128, 1, 0, 0, 1, 0, 0))),
    'cfg2': (dict(), {}, ([(0, 0, 0, 0)], (0, 1, 0, 0, 0, 128, 17, 0, 0, 1, 0, 0))),
    'cfg3': (dict(layers=[512], batch_size=240, n_sample=2048, loss=0, final_act=6, bpreg=0.0, logq=1.0, dropout_p_embed=0.45), {},
             ([(2, 3, 3, 9)], (2, 2, 0, 0, 2, 160, 15, 0, 2, 2, 1, 0))),
    'cfg4': (CFG4, {}, ([(3, 3, 0, 8)], (1, 1, 0, 1, 1, 544, 16, 16, 1, 1, 0, 1))),
    'cfg5': (dict(layers=[100, 100], loss=2, dropout_p_embed=0.2), {},
             ([(0, 0, 0, 0), (0, 0, 0, 0)], (0, 3, 0, 0, 0, 128, 17, 0, 0, 1, 0, 0))),
    'cfg2_no_lean': (dict(), {'G4R_NO_LEAN': '1'}, ([(1, 1, 0, 0)], (5, 1, 0, 0, 4, 256, 9, 0, 1, 1, 0, 0))),
    'cfg2_momentum': (dict(momentum=0.1), {}, ([(0, 0, 0, 0)], (0, 1, 0, 0, 0, 128, 17, 0, 0, 1, 0, 0))),
    'cfg2_adam': (dict(adapt=3, adapt_p0=0.9, adapt_p1=0.999), {}, ([(0, 0, 0, 0)], (0, 1, 0, 0, 0, 128, 17, 0, 2, 1, 0, 0))),
    'cfg2_defer': (dict(), {'G4R_DEFER': '1'}, ([(0, 0, 0, 0)], (0, 1, 0, 0, 0, 128, 17, 0, 1, 1, 0, 0))),
    'cfg2_lean_update_0': (dict(), {'G4R_LEAN_UPDATE': '0'}, ([(0, 0, 0, 0)], (0, 1, 0, 0, 0, 128, 17, 0, 1, 1, 0, 0))),
    'cfg2_onehot': (dict(embed_mode=2), {}, ([(4, 2, 0, 0)], (0, 1, 0, 0, 0, 128, 17, 0, 1, 2, 0, 0))),
    'separate_512_256': (dict(layers=[512, 256], embed_mode=1, embedding=128), {},
                         ([(2, 3, 3, 9), (3, 3, 0, 8)], (2, 1, 0, 0, 4, 128, 17, 0, 2, 1, 1, 0))),
    'cfg4_no_mt_no_bmt': (CFG4, {'G4R_NO_MT': '1', 'G4R_NO_BMT': '1'}, ([(3, 3, 0, 8)], (2, 1, 0, 1, 2, 584, 15, 0, 1, 1, 0, 1))),
    'cfg2_force_staged': (dict(), {'G4R_FORCE_STAGED': '1'}, ([(0, 0, 0, 0)], (0, 1, 0, 0, 0, 128, 17, 0, 1, 1, 0, 0))),
}
NKEY = 44      # 4 x G4R_MAX_LAYERS + 12
RECORDED_CUS = 256


def _model(settings):
    c = dict(BASE, **settings)
    return _native.Model(n_items=20000, sample_store=max(c['n_sample'], 1) * 64, sample_alpha=0.75, seed=9, device=0, rank=0, nranks=1,
                         use_graph=1, **c)


@pytest.fixture(scope='module', autouse=True)
def _recorded_cu_count():
    m = _model({})
    n = int(m.get_debug('n_cu', (1,))[0])
    m.close()
    if n != RECORDED_CUS:
        pytest.skip('the expected choices were recorded on a %d-CU device; this one has %d CUs' % (RECORDED_CUS, n))


def _kernels(settings):
    m = _model(settings)
    try:
        return [int(x) for x in m.get_debug('kernels', (NKEY,))]
    finally:
        m.close()


def _expected(layers, tail):
    v = [0] * NKEY
    for l, (fwd, bwd, deep, wide) in enumerate(layers):
        v[l], v[8 + l], v[16 + l], v[24 + l] = fwd, bwd, deep, wide
    v[32:] = tail
    return v


@pytest.mark.parametrize('case', sorted(CASES))
def test_step_kernels(case):
    settings, env, want = CASES[case]
    if not env:
        got = _kernels(settings)
    else:      # (the switches are read at g4r_create: a child process keeps them out of the other tests' models)
        code = ('import json, sys; sys.path.insert(0, %r); from tests.test_gpu_step_kernels import _kernels; '
                'print("KERNELS", json.dumps(_kernels(%r)))' % (ROOT, settings))
        r = subprocess.run([sys.executable, '-c', code], cwd=ROOT, env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
        got = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('KERNELS ')][-1][8:])
    assert got == _expected(*want), (case, got)

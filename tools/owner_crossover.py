"""Step time of the owner tables' pre-scan form (G4R_OWNER_WINDOW=0) against the window form (=1) at list lengths between bench cfg #1's
and cfg #2's (profiles/owner_window.md, section 2c): python tools/owner_crossover.py"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import bench
STEPS, WARM = 3200, 320
def run(cfg, form):
    os.environ['G4R_OWNER_WINDOW'] = form
    plan, support = bench.make_plan(cfg, STEPS + WARM, 0, 1)
    T = STEPS + WARM
    for k in ('in_idx', 'out_idx', 'reset', 'M'):
        plan[k] = plan[k][:T]
    plan['T'] = T; plan['n_compact'] = 0
    m = bench.create_model(cfg, support, 0, 1, 0, None, use_graph=True)
    ow = int(m.get_debug('owner_window', (1,))[0])
    assert ow == int(form), (ow, form)
    m.set_plan(plan); m.reset_hidden()
    m.train_steps(0, WARM)
    t0 = time.perf_counter()
    m.train_steps(WARM, STEPS)
    dt = time.perf_counter() - t0
    m.close()
    return dt / STEPS * 1e6
for B, ns in ((32, 0), (64, 0), (128, 0), (128, 256), (128, 768), (128, 2048)):
    cfg = dict(bench.CONFIGS['cfg2'], batch_size=B, n_sample=ns)
    if ns == 0:
        cfg = dict(bench.CONFIGS['cfg1'], batch_size=B)
    res = {'0': [], '1': []}
    for rep in range(3):
        for form in ('0', '1'):
            res[form].append(run(cfg, form))
    a, b = sorted(res['0']), sorted(res['1'])
    print('R = %5d (B = %3d, ns = %4d, pre-scan workgroups %3d): pre-scan %s  window %s  median window - pre-scan %+.3f us' % (
        2 * B + ns, B, ns, (2 * B + ns + 15) // 16, ' / '.join('%.3f' % x for x in res['0']), ' / '.join('%.3f' % x for x in res['1']), b[1] - a[1]), flush=True)

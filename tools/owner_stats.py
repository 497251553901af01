"""How often k_update_l's owners of repeated items take the owner-list path (the pre-scan in k_loss_rows) on a bench configuration:
steps with at least one such owner, owners per step, the largest occurrence count n of one.  Eager single steps; the owners are
computed on the host from the step's occurrence ids (debug key occ_idx) by k_update_l's rule, and the lists the pre-scan wrote
(own_pos) are checked against them.  CFG=cfg2 STEPS=300 python tools/owner_stats.py"""
import os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
name = os.environ.get('CFG', 'cfg2')
cfg = bench.CONFIGS[name]
T = int(os.environ.get('STEPS', '300'))
plan, support = bench.make_plan(cfg, T + 1, 0, 1)
m = bench.create_model(cfg, support, 0, 1, 0, None, use_graph=False)
for k in ('in_idx', 'out_idx', 'reset', 'M'):
    plan[k] = plan[k][:T + 1]
plan['T'] = T + 1; plan['n_compact'] = 0
m.set_plan(plan); m.reset_hidden()
B, ns = cfg['batch_size'], cfg['n_sample']
R = 2 * B + ns
constrained = cfg.get('constrained_embedding', True)
steps_with, per_step, nmax, mism, hot = 0, [], 0, 0, 0
for t in range(T):
    m.train_steps(t, 1)
    occ = m.get_debug('occ_idx', (R,)).view(np.int32)
    groups = {}
    for k, item in enumerate(occ.tolist()):
        if item >= 0:
            groups.setdefault((0 if (constrained or k >= B) else 1, item), []).append(k)
    owners = {p[-1]: p[:-1] for p in groups.values() if len(p) > 1 and p[0] < 2 * B}
    per_step.append(len(owners))
    if owners:
        steps_with += 1
        nmax = max(nmax, max(len(p) + 1 for p in owners.values()))
        pos = m.get_debug('own_pos', (16 * R,)).view(np.int32).reshape(R, 16)
        for k, p in owners.items():
            if len(p) > 15:
                hot += 1
                mism += int(pos[k, 0] != -1)
            elif pos[k, 0] != len(p) or not np.array_equal(pos[k, 1:1 + len(p)], p):
                mism += 1
ps = np.array(per_step)
print('%s: %d steps; %d with >= 1 owner outside the negatives-only shortcut; such owners per step mean %.2f max %d; largest n %d; owners past '
      'the 15-position row (scan in k_update_l): %d; rows that differ from the host rule: %d' % (name, T, steps_with, ps.mean(), ps.max(), nmax, hot, mism))

"""Times GRU4Rec.continue_sessions (steps selections per session, the winners fed back on the device) against the host loop it
replaces: recommend_sessions on the histories, then steps - 1 times recommend_sessions on the one-item histories [[previous winner]]
from the returned hidden state, the exclusion lists rebuilt on the host every round.  One JSON line per (shape, steps, k):

  python tools/bench_continue_sessions.py [--shapes rsc15,10M] [--steps 5,20] [--ks 1,20] [--reps 7] [--warmup 2] [--md FILE]

Shapes: rsc15 = 37,483 items x 100 units, 10M = 10,000,000 items x 256 units with scan='bf16' (steps 5 only); N = 512 sessions of 2 to
6 items, no_repeat on.  Every time is the median of --reps synchronous calls after --warmup, with the spread (max - min) next to it;
`faster` says whether the call's median is below the loop's by more than the loop's own spread.  --md appends the table of
profiles/continue_sessions.md to FILE; --loop-only times the host loop alone (it runs on a checkout without continue_sessions too: the
baseline on the parent commit).  Kernel times do not come from this script: the per-step table of the profile is the kernel_stats CSV of
`rocprofv3 --kernel-trace --stats -- python tools/bench_continue_sessions.py --shapes rsc15 --steps 20 --ks 20 --reps 3 --warmup 1
--call-only`, a run of its own."""
import argparse
import json
import time

import numpy as np

from bench_common import as_gru4rec, serving_model

SHAPES = {'rsc15': (37_483, 100, 'fp32'), '10M': (10_000_000, 256, 'bf16')}
ROWS = 512


def host_loop(g, hists, steps, k, scan):
    N = len(hists)
    ids, sc, H = g.recommend_sessions(hists, k=k, exclude_history=True, return_hidden=True, scan=scan)
    out = [ids]
    gen = [[] for _ in hists]
    for _ in range(1, steps):
        for i in range(N):
            gen[i].append(ids[i, 0])
        xs = [list(hists[i]) + gen[i] for i in range(N)]
        ids, sc, H = g.recommend_sessions([[gen[i][-1]] for i in range(N)], k=k, exclude_per_row=xs, hidden=H, return_hidden=True, scan=scan)
        out.append(ids)
    return np.stack(out, axis=1)


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(max(ts) - min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='rsc15,10M')
    ap.add_argument('--steps', default='5,20')
    ap.add_argument('--ks', default='1,20')
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--md', default=None)
    ap.add_argument('--call-only', action='store_true', help='time the call alone (for a kernel trace)')
    ap.add_argument('--loop-only', action='store_true', help='time the host loop alone (works on a checkout without continue_sessions)')
    a = ap.parse_args()
    rows = []
    for name in a.shapes.split(','):
        I, D, scan = SHAPES[name]
        rng = np.random.RandomState(0)
        g = as_gru4rec(serving_model(I, D, ROWS, 'linear', rng), I, D, 'linear')
        ids = g.itemidmap.index.values
        hists = [ids[rng.randint(0, I, size=n)] for n in rng.randint(2, 7, size=ROWS)]
        for steps in [int(s) for s in a.steps.split(',')]:
            if name == '10M' and steps != 5:
                continue
            for k in [int(x) for x in a.ks.split(',')]:
                out = dict(shape=name, n_items=I, D=D, rows=ROWS, steps=steps, k=k, scan=scan)
                if a.loop_only:
                    t_l, s_l = timed(lambda: host_loop(g, hists, steps, k, scan), a.reps, a.warmup)
                    out.update(ms_loop=round(t_l, 2), spread_loop=round(s_l, 2))
                    print(json.dumps(out), flush=True)
                    continue
                t_c, s_c = timed(lambda: g.continue_sessions(hists, steps, k=k, scan=scan), a.reps, a.warmup)
                out.update(ms_call=round(t_c, 2), spread_call=round(s_c, 2))
                if not a.call_only:
                    same = bool((g.continue_sessions(hists, steps, k=k, scan=scan)[0] == host_loop(g, hists, steps, k, scan)).all())
                    t_l, s_l = timed(lambda: host_loop(g, hists, steps, k, scan), a.reps, a.warmup)
                    out.update(ms_loop=round(t_l, 2), spread_loop=round(s_l, 2), speedup=round(t_l / t_c, 2), same_items=same,
                               faster=bool(t_c < t_l - s_l))
                print(json.dumps(out), flush=True)
                rows.append(out)
        g.close()
    if a.md and rows and not a.call_only and not a.loop_only:
        with open(a.md, 'a') as f:
            f.write('\n| shape | steps | k | scan | call ms (spread) | loop ms (spread) | loop / call | call below loop by more than the spread of the loop |\n')
            f.write('|---|---|---|---|---|---|---|---|\n')
            for r in rows:
                f.write('| %s | %d | %d | %s | %.2f (%.2f) | %.2f (%.2f) | %.2f | %s |\n' % (
                    r['shape'], r['steps'], r['k'], r['scan'], r['ms_call'], r['spread_call'], r['ms_loop'], r['spread_loop'], r['speedup'],
                    'yes' if r['faster'] else 'NO'))


if __name__ == '__main__':
    main()

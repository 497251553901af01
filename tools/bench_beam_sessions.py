"""Times GRU4Rec.beam_sessions (beam search over session continuations, selection and re-parenting on the device) against the host loop
of its contract: recommend_sessions on the histories with k = beams, then per step one recommend_sessions call over all N x beams
beams, the beams x beams candidates of every session combined and ordered in NumPy, states and exclusion lists re-parented on the
host.  One JSON line per (beams, steps):

  python tools/bench_beam_sessions.py [--beams 4,16] [--steps 5,20] [--reps 7] [--warmup 2] [--md FILE]

Shape: 37,483 items x 100 units, final_act linear (combine='sum'), N = 512 sessions of 2 to 6 items, no_repeat on.  Every time is the
median of --reps synchronous calls after --warmup, timed with time.perf_counter around the whole call (host work included), with the
spread (max - min) next to it.  --md appends the table of profiles/beam_sessions.md to FILE.  Two modes need nothing of this feature
and so run on the parent commit too (the baselines): --loop-only times the host loop alone; --floor times continue_sessions on
512 x beams rows with k = beams, the same GRU steps and selections per step without k_beam_select / k_beam_advance."""
import argparse
import json
import time

import numpy as np

from bench_common import as_gru4rec, serving_model

N_ITEMS, UNITS, ROWS = 37_483, 100, 512


def host_loop(g, hists, steps, W):
    """The contract's loop ('sum'), vectorised where NumPy allows: what a user has to write without beam_sessions."""
    N = len(hists)
    ids, sc, H = g.recommend_sessions(hists, k=W, exclude_history=True, return_hidden=True)
    paths = ids[:, :, None]                                   # [N, W, s]
    cum = sc.copy()
    H = [np.repeat(h, W, axis=0) for h in H]
    rows = np.arange(N)[:, None]
    for _ in range(1, steps):
        xs = [list(hists[n]) + paths[n, b].tolist() for n in range(N) for b in range(W)]
        ids, sc, Hn = g.recommend_sessions([[x] for x in paths[:, :, -1].ravel()], k=W, exclude_per_row=xs, hidden=H, return_hidden=True)
        p = (cum[:, :, None] + sc.reshape(N, W, W)).reshape(N, W * W)
        win = np.argsort(-p, axis=1, kind='stable')[:, :W]       # score descending, equal scores by the lower b W + j
        cum = p[rows, win]
        par = win // W
        paths = np.concatenate([paths[rows, par], ids.reshape(N, W * W)[rows, win][:, :, None]], axis=2)
        take = (rows * W + par).ravel()
        H = [h[take] for h in Hn]
    return paths, cum


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
    ap.add_argument('--beams', default='4,16')
    ap.add_argument('--steps', default='5,20')
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--md', default=None)
    ap.add_argument('--call-only', action='store_true', help='time the call alone (for a kernel trace)')
    ap.add_argument('--loop-only', action='store_true', help='time the host loop alone (works on a checkout without beam_sessions)')
    ap.add_argument('--floor', action='store_true', help='time continue_sessions on 512 x beams rows, k = beams (works there too)')
    a = ap.parse_args()
    rng = np.random.RandomState(0)
    g = as_gru4rec(serving_model(N_ITEMS, UNITS, ROWS, 'linear', rng), N_ITEMS, UNITS, 'linear')
    ids = g.itemidmap.index.values
    hists = [ids[rng.randint(0, N_ITEMS, size=n)] for n in rng.randint(2, 7, size=ROWS)]
    rows = []
    for W in [int(x) for x in a.beams.split(',')]:
        for steps in [int(s) for s in a.steps.split(',')]:
            out = dict(n_items=N_ITEMS, D=UNITS, sessions=ROWS, beams=W, steps=steps)
            if a.floor:
                wide = [hists[i % ROWS] for i in range(ROWS * W)]
                t, s = timed(lambda: g.continue_sessions(wide, steps, k=W), a.reps, a.warmup)
                out.update(ms_floor=round(t, 2), spread_floor=round(s, 2))
            elif a.loop_only:
                t, s = timed(lambda: host_loop(g, hists, steps, W), a.reps, a.warmup)
                out.update(ms_loop=round(t, 2), spread_loop=round(s, 2))
            else:
                t_c, s_c = timed(lambda: g.beam_sessions(hists, steps, beams=W), a.reps, a.warmup)
                out.update(ms_call=round(t_c, 2), spread_call=round(s_c, 2))
                if not a.call_only:
                    got, want = g.beam_sessions(hists, steps, beams=W), host_loop(g, hists, steps, W)
                    same = bool((got[0] == want[0]).all() and (got[1].view(np.uint32) == want[1].view(np.uint32)).all())
                    t_l, s_l = timed(lambda: host_loop(g, hists, steps, W), a.reps, a.warmup)
                    out.update(ms_loop=round(t_l, 2), spread_loop=round(s_l, 2), speedup=round(t_l / t_c, 2), same_result=same,
                               faster=bool(t_c < t_l - s_l))
                    rows.append(out)
            print(json.dumps(out), flush=True)
    g.close()
    if a.md and rows:
        with open(a.md, 'a') as f:
            f.write('\n| beams | steps | call ms (spread) | loop ms (spread) | loop / call | same result | call below loop by more than the spread of the loop |\n')
            f.write('|---|---|---|---|---|---|---|\n')
            for r in rows:
                f.write('| %d | %d | %.2f (%.2f) | %.2f (%.2f) | %.2f | %s | %s |\n' % (
                    r['beams'], r['steps'], r['ms_call'], r['spread_call'], r['ms_loop'], r['spread_loop'], r['speedup'],
                    'yes' if r['same_result'] else 'NO', 'yes' if r['faster'] else 'NO'))


if __name__ == '__main__':
    main()

"""Times the per-group caps (g4r_recommend_sessions_capped, g4r_continue_sessions_capped) against what they are built on and what they
replace.  One JSON line per shape and measurement, appended to --out when given:

  python tools/bench_group_caps.py [--what capped,recommend,continue] [--sessions 512] [--pool 100] [--k 20] [--cap 2] [--steps 5,20]
                                   [--calls 15] [--warmup 3] [--small-only] [--package-root DIR] [--out FILE]

Shapes: 37,483 items x 100 units with the exact selection, and 10,000,000 x 256 with the bf16 scan (oversample 8).  Histories of 1 to 10
items.  Groups: item index i is ungrouped when i % 7 == 0, otherwise its group is i % 5 (the groups of the tests: cap 2 leaves some lists short).  ms_* are (min, median, max) wall times of
synchronous calls:
capped      recommend_sessions_capped(k, pool, cap)
recommend   recommend_sessions(k = pool) with the same arguments: the selection the new stage follows.  In one process the two calls
            alternate, so what disturbs one disturbs the other; added_ms is the difference of the medians and recommend_spread the
            margin of that comparison.  --package-root DIR --what recommend times the same call with the package of another checkout
            (the commit before this feature), which has no capped entry.
continue    continue_sessions_capped(k = 1, pool, cap, steps, no_repeat) against the loop it replaces: one recommend_sessions(k = pool)
            call per step from the returned hidden states, the walk and the exclusion lists kept on the host in NumPy -- the same
            paths (checked here on every call).
Kernel times do not come from this script: run it under `rocprofv3 --kernel-trace --stats -- python tools/bench_group_caps.py
--what continue --small-only` in a run of its own and read k_group_cap next to k_topk_range / k_topk_merge in the kernel statistics."""
import argparse
import json
import os
import sys
import time

import numpy as np


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def stats(t):
    return [round(float(x), 3) for x in (np.min(t), np.median(t), np.max(t))]


def host_continue(m, offs, items, G, n_groups, a, steps, over):
    """The host loop for k = 1: the first position of every step's pool whose group is not full (position 0 when there is none)."""
    N = len(offs) - 1
    counts = np.zeros((N, n_groups), dtype=np.int32)
    rows = np.arange(N)
    seen = [np.unique(items[offs[i]:offs[i + 1]]) for i in range(N)]
    path = np.empty((N, steps), dtype=np.int32)
    o, it, H = offs, items, None
    for s in range(steps):
        xo = np.concatenate([[0], np.cumsum([len(x) for x in seen])]).astype(np.int64)
        cols, _, H = m.recommend_sessions(o, it, None, a.pool, xo, np.concatenate(seen).astype(np.int32), None, hidden=H, return_hidden=True,
                                          oversample=over)
        g = G[cols]
        ok = (g < 0) | (counts[rows[:, None], np.maximum(g, 0)] < a.cap)
        win = cols[rows, np.where(ok.any(axis=1), ok.argmax(axis=1), 0)]
        path[:, s] = win
        gw = G[win]
        np.add.at(counts, (rows[gw >= 0], gw[gw >= 0]), 1)
        seen = [np.union1d(x, [w]) for x, w in zip(seen, win)]
        o, it = np.arange(N + 1, dtype=np.int64), win.astype(np.int32)
    return path


def emit(a, res):
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, 'a') as f:
            f.write(line + '\n')


def bench(a, I, D, over):
    from bench_common import dense_weights, serving_model
    rng = np.random.default_rng(0)
    m = serving_model(I, D, 32, 'linear', rng, weights=dense_weights)
    lens = rng.integers(1, 11, size=a.sessions)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    items = rng.integers(0, I, size=int(offs[-1])).astype(np.int32)
    what = a.what.split(',')
    idx = np.arange(I)
    G = np.where(idx % 7 == 0, -1, idx % 5).astype(np.int32)
    capped_ok = hasattr(m, 'recommend_sessions_capped')
    if capped_ok:
        m.set_item_groups(G)
    base = dict(n_items=I, D=D, sessions=a.sessions, pool=a.pool, k=a.k, cap=a.cap, scan='bf16 x%d' % over if over else 'fp32',
                package=os.path.abspath(a.package_root) if a.package_root else 'this tree')
    # ---- (a) capped lists next to the selection they follow
    rec = lambda: m.recommend_sessions(offs, items, None, a.pool, oversample=over)      # noqa: E731
    fns = {'recommend': rec}
    if capped_ok:
        fns['capped'] = lambda: m.recommend_sessions_capped(offs, items, None, a.k, a.pool, a.cap, oversample=over)
    order = [w for w in ('capped', 'recommend') if w in what and w in fns]
    if order:
        for _ in range(a.warmup):
            for w in order:
                fns[w]()
        t = {w: [] for w in order}
        for _ in range(a.calls):      # alternating
            for w in order:
                t[w].append(timed(fns[w])[0])
        res = dict(base, what='lists')
        for w in order:
            res['ms_' + w] = stats(t[w])
        if len(order) == 2:
            c, r = np.median(t['capped']), np.median(t['recommend'])
            kept = fns['capped']()[3]
            res.update(added_ms=round(float(c - r), 3), added_over_recommend=round(float((c - r) / r), 4),
                       recommend_spread=round(float((np.max(t['recommend']) - np.min(t['recommend'])) / r), 4),
                       rows_full=int((kept == a.k).sum()), rows_short=int((kept < a.k).sum()))
        emit(a, res)
    # ---- (b) the capped continuation next to the host loop it replaces
    if 'continue' in what and capped_ok:
        seen = [np.unique(items[offs[i]:offs[i + 1]]) for i in range(a.sessions)]      # no_repeat: the histories are the rows' first exclusions
        xo, xi = np.concatenate([[0], np.cumsum([len(x) for x in seen])]).astype(np.int64), np.concatenate(seen).astype(np.int32)
        for steps in [int(x) for x in a.steps.split(',')]:
            dev = lambda: m.continue_sessions_capped(offs, items, None, 1, a.pool, a.cap, steps, True, xo, xi, oversample=over)      # noqa: E731
            for _ in range(a.warmup):
                dev()
            td, th = [], []
            for _ in range(a.calls):
                ms, out = timed(dev)
                td.append(ms)
            for _ in range(max(2, a.calls // 5)):
                ms, path = timed(lambda: host_continue(m, offs, items, G, 5, a, steps, over))
                assert np.array_equal(path, out[0][:, :, 0]), 'the host loop and the device disagree'
                th.append(ms)
            emit(a, dict(base, what='continue', steps=steps, k=1, ms_device=stats(td), ms_host=stats(th), host_paths_equal=True,
                         fallback_steps=int((out[2] == 0).sum()), host_over_device=round(float(np.median(th) / np.median(td)), 2)))
    m.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--what', default='capped,recommend,continue')
    ap.add_argument('--sessions', type=int, default=512)
    ap.add_argument('--pool', type=int, default=100)
    ap.add_argument('--k', type=int, default=20)
    ap.add_argument('--cap', type=int, default=2)
    ap.add_argument('--steps', default='5,20')
    ap.add_argument('--calls', type=int, default=15)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--small-only', action='store_true', help='the 37,483 x 100 shape only')
    ap.add_argument('--package-root', default=None, help='import gru4rec_amd from this checkout (for --what recommend at another commit)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.package_root:
        sys.path.insert(0, os.path.join(os.path.abspath(a.package_root), 'tools'))
    bench(a, 37_483, 100, None)
    if not a.small_only:
        bench(a, 10_000_000, 256, 8)


if __name__ == '__main__':
    main()

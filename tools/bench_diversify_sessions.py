"""Times g4r_diversify_sessions (GRU4Rec.diversify_sessions) against what it is built on and what it replaces.  One JSON line per shape,
appended to --out when given:

  python tools/bench_diversify_sessions.py [--what diversify,recommend,host] [--sessions 512] [--pool 100] [--k 20] [--calls 15]
                                           [--warmup 3] [--small-only] [--package-root DIR] [--out FILE]

Shapes: 37,483 items x 100 units with the exact selection, and 10,000,000 x 256 with the bf16 scan (oversample 8).  Histories of 1 to 10
items, cosine in the output space, trade-off 0.7, normalised relevance.  ms_* are (min, median, max) wall times of synchronous calls:
diversify   diversify_sessions(k, pool)
recommend   recommend_sessions(k = pool) with the same arguments: the selection the new stage follows.  In one process the two calls
            alternate, so what disturbs one disturbs the other; added_ms is the difference of the medians and recommend_spread the
            margin of that comparison.  --package-root DIR --what recommend times the same call with the package of another checkout
            (the commit before this feature), which has no diversify entry.
host        the loop the entry replaces: recommend_sessions(k = pool), one similar_items call per session for its pool x pool pair
            scores, and the greedy selection in NumPy float32 -- the same picks, bit for bit (checked here on every call).
Kernel times do not come from this script: run it under `rocprofv3 --kernel-trace --stats -- python tools/bench_diversify_sessions.py
--what diversify --small-only` in a run of its own and read k_mmr_rerank next to k_topk_range / k_topk_merge in the kernel statistics."""
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


def greedy(s, S, k, lam, normalize):
    """The selection of include/gru4rec_hip.h in np.float32 (tests/test_gpu_diversify.py)."""
    mu = np.float32(1.0) - lam
    r = s
    if normalize:
        lo, hi = s.min(), s.max()
        r = (s - lo) / (hi - lo) if hi > lo else np.zeros_like(s)
    lr = lam * r
    free = np.ones(len(s), dtype=bool)
    pos, m = [], None
    for t in range(k):
        if t == 0:
            v = lr
        else:
            sim = S[pos[-1]]
            m = sim if t == 1 else np.where(sim > m, sim, m)
            v = lr - mu * m
        j = int(np.argmax(np.where(free, v, -np.inf)))
        pos.append(j)
        free[j] = False
    return pos


def host_loop(m, rec, a, lam):
    cols, scores = rec()
    P = cols.shape[1]
    out = np.empty((len(cols), a.k), dtype=np.int32)
    for i in range(len(cols)):
        it, sc = m.similar_items(cols[i], cols[i], P - 1, 'cosine', 'output')      # positions in the pool, the query's own skipped
        S = np.zeros((P, P), dtype=np.float32)
        S[np.arange(P)[:, None], it] = sc
        out[i] = greedy(scores[i], S, a.k, lam, True)
    return out


def bench(a, I, D, over):
    from bench_common import dense_weights, serving_model
    rng = np.random.default_rng(0)
    m = serving_model(I, D, 32, 'linear', rng, weights=dense_weights)
    lens = rng.integers(1, 11, size=a.sessions)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    items = rng.integers(0, I, size=int(offs[-1])).astype(np.int32)
    lam = np.float32(0.7)
    what = a.what.split(',')
    rec = lambda: m.recommend_sessions(offs, items, None, a.pool, oversample=over)      # noqa: E731
    fns = {'recommend': rec}
    if 'diversify' in what:
        fns['diversify'] = lambda: m.diversify_sessions(offs, items, None, a.k, a.pool, float(lam), 'cosine', 'output', True, oversample=over)
    order = [w for w in ('diversify', 'recommend') if w in what and w in fns]
    for _ in range(a.warmup):
        for w in order:
            fns[w]()
    t = {w: [] for w in order}
    for _ in range(a.calls):      # alternating
        for w in order:
            t[w].append(timed(fns[w])[0])
    res = dict(what='sessions', n_items=I, D=D, sessions=a.sessions, pool=a.pool, k=a.k, scan='bf16 x%d' % over if over else 'fp32',
               package=os.path.abspath(a.package_root) if a.package_root else 'this tree')
    for w in order:
        res['ms_' + w] = stats(t[w])
    if len(order) == 2:
        d, r = np.median(t['diversify']), np.median(t['recommend'])
        res.update(added_ms=round(float(d - r), 3), added_over_recommend=round(float((d - r) / r), 4),
                   recommend_spread=round(float((np.max(t['recommend']) - np.min(t['recommend'])) / r), 4))
    if 'host' in what and 'diversify' in fns:
        th = []
        want = fns['diversify']()[2]
        for _ in range(max(2, a.calls // 5)):
            ms, pos = timed(lambda: host_loop(m, rec, a, lam))
            assert np.array_equal(pos, want), 'the host loop and the device disagree'
            th.append(ms)
        res.update(ms_host=stats(th), host_picks_equal=True)
        if 'diversify' in t:
            res['host_over_diversify'] = round(float(np.median(th) / np.median(t['diversify'])), 1)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, 'a') as f:
            f.write(line + '\n')
    m.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--what', default='diversify,recommend,host')
    ap.add_argument('--sessions', type=int, default=512)
    ap.add_argument('--pool', type=int, default=100)
    ap.add_argument('--k', type=int, default=20)
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

"""Times the audience selection (g4r_audience_sessions) against the host routes it replaces.  One JSON line per shape and measurement,
appended to --out when given:

  python tools/bench_audience_sessions.py [--sessions 100000] [--items 100] [--k 100,10000] [--max-len 30] [--calls 3] [--warmup 1]
                                          [--small-only] [--out FILE]

Shapes: 37,483 items x 100 units with by = score and by = logprob, and 10,000,000 x 256 with by = score only (2^24 items is the limit of
the exact row normaliser).  Histories of 1 to --max-len items.  ms_* are (min, median, max) wall times of synchronous calls:
device   audience_sessions(histories, items, k, by)
host     score:   score_candidates_sessions with the same M items for every session -- the N x M matrix comes down --, then per item
                  argpartition + a sort of the k kept (the same sessions as the device's: checked on every call);
         logprob: that matrix, session_log_partition for every session's (zeta, Q), the log-probabilities in float64 on the host, the
                  same selection (the last place of a value may differ from the device's, so only the share of equal sessions is shown).
kernel_ms: one more device call under g4r_profile -- the total time of k_audience_keys and k_audience_merge from the library's kernel
timers (event pairs around every launch), their launches, and their share of that call's wall time."""
import argparse
import json
import time

import numpy as np


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def stats(t):
    return [round(float(x), 3) for x in (np.min(t), np.median(t), np.max(t))]


def emit(a, res):
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, 'a') as f:
            f.write(line + '\n')


def select(V, k):
    """per column of V[N, M]: the k rows with the largest value, value descending then row ascending -> int64[M, min(k, N)]"""
    N, M = V.shape
    k = min(k, N)
    out = np.empty((M, k), dtype=np.int64)
    for j in range(M):
        v = V[:, j]
        keep = np.argpartition(-v, k - 1)[:k] if k < N else np.arange(N)
        cut = v[keep].min()
        keep = np.flatnonzero(v >= cut)      # (ties at the cut: all of them, the sort decides)
        out[j] = keep[np.lexsort((keep, -v[keep]))][:k]
    return out


def bench(a, I, D, modes):
    from bench_common import dense_weights, serving_model
    rng = np.random.default_rng(0)
    m = serving_model(I, D, 32, 'linear', rng, weights=dense_weights)
    N, M = a.sessions, a.items
    lens = rng.integers(1, a.max_len + 1, size=N)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    hist = rng.integers(0, I, size=int(offs[-1])).astype(np.int32)
    items = rng.choice(I, size=M, replace=False).astype(np.int32)
    coffs = (np.arange(N + 1, dtype=np.int64) * M)
    citems = np.tile(items, N)

    def host(by, k):
        V = m.score_candidates_sessions(offs, hist, coffs, citems, 0).reshape(N, M)
        if by == 'logprob':
            zeta, Q = m.session_log_partition(offs, hist, None, 1.0)
            V = ((V - zeta[:, None]).astype(np.float64) - np.log(Q.astype(np.float64) * 2.0 ** -39)[:, None]).astype(np.float32)
        return select(V, k)

    for by in modes:
        for k in [int(x) for x in a.k.split(',')]:
            dev = lambda: m.audience_sessions(offs, hist, items, k, by=by)      # noqa: E731
            for _ in range(a.warmup):
                dev()
            td, th, same = [], [], []
            for _ in range(a.calls):
                ms, out = timed(dev)
                td.append(ms)
                ms, want = timed(lambda: host(by, k))
                th.append(ms)
                eq = float((out[0][:, :want.shape[1]] == want).mean())
                assert by == 'logprob' or eq == 1.0, 'the host route and the device disagree'
                same.append(eq)
            m.profile(True)
            wall, _ = timed(dev)
            kt = m.kernel_times()
            m.profile(False)
            km = {n: [round(kt[n][0], 3), int(kt[n][1])] for n in ('k_audience_keys', 'k_audience_merge')}
            emit(a, dict(n_items=I, D=D, sessions=N, items=M, k=k, by=by, max_len=a.max_len, ms_device=stats(td), ms_host=stats(th),
                         host_over_device=round(float(np.median(th) / np.median(td)), 2), sessions_equal=round(min(same), 6), kernel_ms=km,
                         kernel_share=round(sum(v[0] for v in km.values()) / wall, 4), host_matrix_mb=round(N * M * 4 / 2 ** 20, 1),
                         device_result_mb=round(M * k * 8 / 2 ** 20, 3)))
    m.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sessions', type=int, default=100_000)
    ap.add_argument('--items', type=int, default=100)
    ap.add_argument('--k', default='100,10000')
    ap.add_argument('--max-len', type=int, default=30)
    ap.add_argument('--calls', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--small-only', action='store_true', help='the 37,483 x 100 shape only')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    bench(a, 37_483, 100, ('score', 'logprob'))
    if not a.small_only:
        bench(a, 10_000_000, 256, ('score',))


if __name__ == '__main__':
    main()

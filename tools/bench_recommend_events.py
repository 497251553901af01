#!/usr/bin/env python
"""Per-step wall time of g4r_recommend_events against g4r_evaluate on the same plan, and the same data through the two routes that
existed before it (a predict_step loop with a host argpartition; recommend_sessions over every prefix).  One JSON line per shape.

    python tools/bench_recommend_events.py --items 37483 --units 100 --batch 100 --sessions 2000 --routes
    python tools/bench_recommend_events.py --items 10000000 --units 256 --batch 512 --sessions 1200 --max_len 6
"""
import argparse
import functools
import json
import time

import numpy as np

from bench_common import serving_model, tiled_weights      # (first: it puts the repository root on sys.path)
from gru4rec_amd import _native, evaluation


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--items', type=int, default=37483)
    ap.add_argument('--units', type=int, default=100)
    ap.add_argument('--batch', type=int, default=100)
    ap.add_argument('--sessions', type=int, default=2000)
    ap.add_argument('--max_len', type=int, default=30)
    ap.add_argument('--k', type=int, default=20)
    ap.add_argument('--repeat', type=int, default=3)
    ap.add_argument('--routes', action='store_true', help='also time the predict_step loop and recommend_sessions over all prefixes')
    o = ap.parse_args()
    I, D, B, k = o.items, o.units, o.batch, o.k
    rng = np.random.RandomState(1)
    m = serving_model(I, D, 32, 'linear', rng, weights=functools.partial(tiled_weights, blk=min(I, 65536), by=0.01, w=0.1), seed=3)
    lens = rng.randint(2, o.max_len + 1, size=o.sessions)
    offs = np.r_[0, np.cumsum(lens)].astype(np.int64)
    titems = rng.randint(0, I, size=int(offs[-1])).astype(np.int32)
    plan = _native.build_plan(offs.astype(np.int32), np.arange(len(lens)), titems, B, 1)
    _, table = evaluation.slot_map(offs, B)
    has_next = np.ones(len(titems), dtype=bool)
    has_next[offs[1:] - 1] = False
    rows = np.flatnonzero(has_next)
    number = np.full(len(titems) + 1, -1, dtype=np.int64)
    number[rows] = np.arange(len(rows))
    slot = number[table]
    T = plan['T']

    def best(f):
        ts = []
        for _ in range(o.repeat):
            t0 = time.perf_counter()
            f()
            ts.append(time.perf_counter() - t0)
        return min(ts)

    m.evaluate(plan, B, None, [20], 'standard')      # warm-up: allocations
    m.recommend_events(plan, B, None, 'standard', slot, len(rows), k)
    t_eval = best(lambda: m.evaluate(plan, B, None, [20], 'standard'))
    t_ev = best(lambda: m.recommend_events(plan, B, None, 'standard', slot, len(rows), k))
    t_rank = best(lambda: m.recommend_events(plan, B, None, 'standard', slot, len(rows), k, want_lists=False))
    out = dict(items=I, units=D, batch=B, k=k, steps=int(T), events=int(len(rows)), evaluate_ms_per_step=1e3 * t_eval / T,
               events_ms_per_step=1e3 * t_ev / T, events_no_download_ms_per_step=1e3 * t_rank / T, evaluate_s=t_eval, events_s=t_ev)
    # the cost of selection the project already carries: g4r_recommend_step against g4r_predict_step without a download
    inp = titems[:B]
    m.predict_begin(B)
    m.predict_step(inp, None, want_scores=False)
    m.recommend_step(inp, None, k)
    n = 50 if I < 1000000 else 5

    def loop(f):
        t0 = time.perf_counter()
        for _ in range(n):
            f()
        return (time.perf_counter() - t0) / n
    out['predict_step_ms'] = 1e3 * min(loop(lambda: m.predict_step(inp, None, want_scores=False)) for _ in range(3))
    out['recommend_step_ms'] = 1e3 * min(loop(lambda: m.recommend_step(inp, None, k)) for _ in range(3))
    if o.routes:
        def stepwise():
            m.predict_begin(B)
            for t in range(T):
                Mt = int(plan['M'][t])
                sc = m.predict_step(plan['in_idx'][t, :Mt], None)
                top = np.argpartition(-sc, k - 1, axis=1)[:, :k]
                np.take_along_axis(sc, top, axis=1)
        # (hidden-state upkeep between the steps left out: it only adds to this route)
        out['predict_loop_s'] = best(stepwise)
        sess = np.searchsorted(offs, rows, side='right') - 1
        hl = rows + 1 - offs[sess]
        hoffs = np.r_[0, np.cumsum(hl)].astype(np.int64)
        hist = np.concatenate([titems[offs[s]:r + 1] for s, r in zip(sess, rows)])
        out['recommend_sessions_s'] = best(lambda: m.recommend_sessions(hoffs, hist, None, k))
    print(json.dumps(out))


if __name__ == '__main__':
    main()

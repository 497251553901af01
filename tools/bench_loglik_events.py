#!/usr/bin/env python
"""Wall time of g4r_loglik_events (evaluation.loglik_gpu's device call) per call (`*_ms_per_step` is that time divided by the plan's
steps: a quotient, not a measurement of a step), against g4r_recommend_events with
k = 1 on the same plan in the same process (one scan of the candidates per step against two) and against the route that existed
before it: session_log_partition + score_candidates_sessions over EVERY prefix, 512 rows a call.  Every timed call ends in the
library's own stream synchronisation, so a host clock around it covers all its device work; a warm-up call first, then `--repeat`
timed calls, reported as their median with the smallest and largest.  One JSON line per shape; --md appends a table row to a file.

    python tools/bench_loglik_events.py --items 37483 --units 100 --batch 100 --sessions 2000 --max_len 30
    python tools/bench_loglik_events.py --items 37483 --units 100 --batch 64 --sessions 64 --min_len 450 --max_len 550
    python tools/bench_loglik_events.py --items 10000000 --units 256 --batch 512 --sessions 4096 --max_len 6
"""
import argparse
import functools
import json
import time

import numpy as np

from bench_common import serving_model, tiled_weights      # (first: it puts the repository root on sys.path)
from gru4rec_amd import _native, evaluation


def timed(f, repeat):
    f()                                                     # warm-up: allocations, code objects
    ts = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return dict(median=float(np.median(ts)), min=float(min(ts)), max=float(max(ts)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--items', type=int, default=37483)
    ap.add_argument('--units', type=int, default=100)
    ap.add_argument('--batch', type=int, default=100)
    ap.add_argument('--sessions', type=int, default=2000)
    ap.add_argument('--min_len', type=int, default=2)
    ap.add_argument('--max_len', type=int, default=30)
    ap.add_argument('--repeat', type=int, default=5)
    ap.add_argument('--exclude_seen', action='store_true')
    ap.add_argument('--no_prefix_loop', action='store_true')
    ap.add_argument('--md', help='append one table row to this file')
    o = ap.parse_args()
    I, D, B = o.items, o.units, o.batch
    rng = np.random.RandomState(1)
    m = serving_model(I, D, 32, 'linear', rng, weights=functools.partial(tiled_weights, blk=min(I, 65536), by=0.01, w=0.1), seed=3)
    lens = rng.randint(o.min_len, o.max_len + 1, size=o.sessions)
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
    T = int(plan['T'])
    seen = None
    if o.exclude_seen:
        seen = evaluation.seen_tables(titems, offs)
        row_sess = np.repeat(np.arange(len(lens)), lens)
        safe = np.maximum(table, 0)
        seen['sess'] = row_sess[safe].astype(np.int32)
        seen['pos'] = (safe - offs[row_sess[safe]]).astype(np.int32)

    out = dict(items=I, units=D, batch=B, sessions=int(o.sessions), steps=T, events=int(len(rows)), exclude_seen=bool(o.exclude_seen),
               repeat=o.repeat)
    res = {}
    out['loglik_s'] = timed(lambda: res.update(ll=m.loglik_events(plan, B, None, slot, len(rows), 1.0, None, seen)), o.repeat)
    out['loglik_scans_per_step'] = m.events_launches()[1] / float(T)
    out['recommend_k1_s'] = timed(lambda: m.recommend_events(plan, B, None, 'standard', slot, len(rows), 1, None, seen), o.repeat)
    out['recommend_k1_scans_per_step'] = m.events_launches()[1] / float(T)
    out['recommend_k20_s'] = timed(lambda: m.recommend_events(plan, B, None, 'standard', slot, len(rows), 20, None, seen), o.repeat)
    if not o.no_prefix_loop:
        # the route without the call: every prefix replayed, 512 rows a call -- the partition, then the target's logit
        sess = np.searchsorted(offs, rows, side='right') - 1
        hl = rows + 1 - offs[sess]
        hist = [titems[offs[s]:r + 1] for s, r in zip(sess, rows)]
        tgt = titems[rows + 1]
        chunks = []
        for c0 in range(0, len(rows), 512):
            c1 = min(len(rows), c0 + 512)
            ho = np.r_[0, np.cumsum(hl[c0:c1])].astype(np.int64)
            hi = np.concatenate(hist[c0:c1]).astype(np.int32)
            xo = xi = None
            if o.exclude_seen:
                own = [np.unique(h) for h in hist[c0:c1]]
                xo, xi = np.r_[0, np.cumsum([len(x) for x in own])].astype(np.int64), np.concatenate(own).astype(np.int32)
            chunks.append((ho, hi, np.arange(c1 - c0 + 1, dtype=np.int64), tgt[c0:c1].astype(np.int32), xo, xi))

        def prefix_loop():
            zeta, Q, z = [], [], []
            for ho, hi, co, ci, xo, xi in chunks:
                a, b = m.session_log_partition(ho, hi, None, 1.0, xo, xi)
                zeta.append(a)
                Q.append(b)
                z.append(np.ravel(m.score_candidates_sessions(ho, hi, co, ci)))
            res['loop'] = (np.concatenate(z), np.concatenate(zeta), np.concatenate(Q))
        out['prefix_loop_s'] = timed(prefix_loop, max(1, min(o.repeat, 3)))
        out['prefix_loop_calls'] = 2 * len(chunks)
        out['prefix_loop_replayed_events'] = int(hl.sum())
        z, zeta, Q, _ = res['ll']
        out['same_bits_as_prefix_loop'] = bool(np.array_equal(z.view(np.uint32), res['loop'][0].astype(np.float32).view(np.uint32)) and
                                               np.array_equal(zeta.view(np.uint32), res['loop'][1].view(np.uint32)) and
                                               np.array_equal(Q, res['loop'][2]))
    for key in ('loglik_s', 'recommend_k1_s', 'recommend_k20_s'):
        out[key.replace('_s', '_ms_per_step')] = 1e3 * out[key]['median'] / T
    print(json.dumps(out))
    if o.md:
        def cell(d):
            return '%.4f (%.4f - %.4f)' % (d['median'], d['min'], d['max'])
        with open(o.md, 'a') as f:
            f.write('| %d x %d | %d | %d | %d | %d | %s | %s | %s | %.3f | %.3f | %s | %s |\n' % (
                I, D, B, o.sessions, T, len(rows), 'yes' if o.exclude_seen else 'no', cell(out['loglik_s']), cell(out['recommend_k1_s']),
                out['loglik_ms_per_step'], out['recommend_k1_ms_per_step'], cell(out['recommend_k20_s']),
                '%s [%s]' % (cell(out['prefix_loop_s']), 'same bits' if out['same_bits_as_prefix_loop'] else 'DIFFERENT') if 'prefix_loop_s' in out
                else 'not run'))


if __name__ == '__main__':
    main()

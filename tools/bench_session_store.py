"""Times the session store's serving call -- one new event per session, then the top-k: store.push(k=20, exclude_seen=True) -- against
the routes a service has without it, measured in the same process on the same model.  One JSON line per shape:

  python tools/bench_session_store.py [--shapes rsc15,10M] [--reps 9] [--warmup 3] [--md FILE] [--store-only]

Shapes: rsc15 = 37,483 items x 100 units (scan='fp32'), 10M = 10,000,000 items x 256 units with scan='bf16'; 512 sessions, k = 20, every
session has PRIOR events behind it when the timing starts (seen_cap = 64).
  store   store.push(sessions, one item each, k=20, exclude_seen=True)
  (a)     the stateless call with the state carried by the caller: recommend_sessions(one-item histories, hidden=, return_hidden=True,
          exclude_per_row=lists), INCLUDING the host work of keeping the lists (every session's list gains the item before the call)
  (b)     the stateless call replaying full histories of 5 and of 30 events: recommend_sessions(histories, exclude_history=True)
  floor   recommend_next_batch at batch=512 with exclude_seen=True: fixed slots, one event per slot -- what no store can beat
Every time is the median of --reps synchronous calls after --warmup, each on fresh random items, with the spread (max - min) next to
it.  `ok` says that push is not slower than (a) beyond (a)'s own spread.  bytes_per_million: the store's device bytes per 10^6 sessions.
--store-only times the push alone (for `rocprofv3 --kernel-trace --stats -- python tools/bench_session_store.py --store-only ...`, a
run of its own: the k_store_* kernels' share of a call comes from its kernel_stats CSV).  --md appends the table to FILE."""
import argparse
import json
import time

import numpy as np

from bench_common import as_gru4rec, serving_model

SHAPES = {'rsc15': (37_483, 100, 'fp32'), '10M': (10_000_000, 256, 'bf16')}
ROWS, K, PRIOR, SEEN_CAP = 512, 20, 5, 64


def timed(fn, reps, warmup):
    for i in range(warmup):
        fn(i)
    ts = []
    for i in range(reps):
        t0 = time.perf_counter()
        fn(warmup + i)
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(ts)), 3), round(float(max(ts) - min(ts)), 3)


def bench(name, reps, warmup, store_only):
    I, D, scan = SHAPES[name]
    rng = np.random.RandomState(0)
    g = as_gru4rec(serving_model(I, D, ROWS, 'linear', rng), I, D, 'linear')
    ids = g.itemidmap.index.values
    sess = np.arange(ROWS)
    prior = ids[rng.randint(0, I, size=(ROWS, PRIOR))]
    events = ids[rng.randint(0, I, size=(warmup + reps, ROWS))]      # call i pushes events[i]
    kw = dict(scan=scan, oversample=8)
    out = dict(shape=name, n_items=I, D=D, rows=ROWS, k=K, scan=scan, prior_events=PRIOR, seen_cap=SEEN_CAP, reps=reps, warmup=warmup)

    st = g.open_session_store(ROWS, seen_cap=SEEN_CAP)
    st.push(np.repeat(sess, PRIOR), prior.ravel())
    out['ms_store'], out['spread_store'] = timed(lambda i: st.push(sess, events[i], k=K, exclude_seen=True, **kw), reps, warmup)
    out['bytes_per_million'] = int(round(st.stats()['device_bytes'] / ROWS * 1e6))
    st.close()
    if store_only:
        g.close()
        return out

    # (a) the caller carries the state and the lists
    _, _, H = g.recommend_sessions(list(prior), k=K, return_hidden=True, **kw)
    lists = [list(p) for p in prior]
    state = dict(H=H)

    def route_a(i):
        for lst, item in zip(lists, events[i]):
            lst.append(item)
        _, _, state['H'] = g.recommend_sessions(events[i][:, None], k=K, hidden=state['H'], return_hidden=True, exclude_per_row=lists, **kw)
    out['ms_a'], out['spread_a'] = timed(route_a, reps, warmup)

    # (b) full replays
    for T in (5, 30):
        hists = ids[rng.randint(0, I, size=(ROWS, T))]
        out['ms_b%d' % T], out['spread_b%d' % T] = timed(lambda i: g.recommend_sessions(hists, k=K, exclude_history=True, **kw), reps, warmup)

    # the floor: fixed slots
    g.predict = None
    for p in range(PRIOR):
        g.predict_next_batch(sess, prior[:, p], predict_for_item_ids=ids[:1], batch=ROWS)
    out['ms_floor'], out['spread_floor'] = timed(lambda i: g.recommend_next_batch(sess, events[i], k=K, batch=ROWS, exclude_seen=True, **kw),
                                                 reps, warmup)
    out['a_over_store'] = round(out['ms_a'] / out['ms_store'], 3)
    out['ok'] = bool(out['ms_store'] <= out['ms_a'] + out['spread_a'])
    g.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='rsc15,10M')
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--md', default=None)
    ap.add_argument('--store-only', action='store_true', help='time the push alone (for a kernel trace)')
    a = ap.parse_args()
    rows = []
    for name in a.shapes.split(','):
        rows.append(bench(name, a.reps, a.warmup, a.store_only))
        print(json.dumps(rows[-1]), flush=True)
    if a.md and not a.store_only:
        with open(a.md, 'a') as f:
            f.write('\n| shape | scan | push ms (spread) | (a) carried state ms (spread) | (b) replay 5 ms | (b) replay 30 ms | floor ms (spread) | '
                    '(a) / push | push within (a) + its spread | store bytes per 10^6 sessions |\n|---|---|---|---|---|---|---|---|---|---|\n')
            for r in rows:
                f.write('| %s | %s | %.2f (%.2f) | %.2f (%.2f) | %.2f (%.2f) | %.2f (%.2f) | %.2f (%.2f) | %.2f | %s | %d |\n' % (
                    r['shape'], r['scan'], r['ms_store'], r['spread_store'], r['ms_a'], r['spread_a'], r['ms_b5'], r['spread_b5'], r['ms_b30'],
                    r['spread_b30'], r['ms_floor'], r['spread_floor'], r['a_over_store'], 'yes' if r['ok'] else 'NO', r['bytes_per_million']))


if __name__ == '__main__':
    main()

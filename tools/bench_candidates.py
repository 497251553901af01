"""Times g4r_score_candidates (per-row candidate lists: each row scored against its own list) against the two routes a caller had
before it: the union of all rows' lists as one g4r_predict_step candidate list (scores of every row against every list, copied to
the host), and the full-catalogue g4r_recommend_step.  One JSON line per (shape, final activation):

  python tools/bench_candidates.py [--shapes 10M,rsc15] [--acts linear,softmax] [--seconds 1.0] [--warmup 2]

Shapes: 10M = 10,000,000 items, D = 256, 512 rows x 1,000 random candidates; rsc15 = 37,483 items, D = 100, 128 rows x 100.
Fields: us_none (k = 0: every score back in CSR order), us_k20 (k = 20), us_union (predict_step over the union), us_full_topk
(recommend_step over the catalogue, k = 20), speedup_vs_union = us_union / us_none; gathered_MB = sum C_i x Dtop x 4 bytes, and
gather_TBps_call / frac_8TBps_call: those bytes over the whole k = 0 call (host packing, uploads, the GRU step and the copy back
included) -- a lower bound of the kernel's rate, whose own time comes from a rocprofv3 kernel trace.  Each time is the mean of
back-to-back synchronous calls over a window of at least --seconds after the warm-up."""
import argparse
import json
import time

import numpy as np

from bench_common import serving_model

SHAPES = {'10M': (10_000_000, 256, 512, 1000), 'rsc15': (37_483, 100, 128, 100)}


def timed(fn, seconds, warmup):
    for _ in range(warmup):
        fn()
    n, t0 = 0, time.perf_counter()
    while True:
        fn()
        n += 1
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return dt / n * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='10M,rsc15')
    ap.add_argument('--acts', default='linear,softmax')
    ap.add_argument('--seconds', type=float, default=1.0)
    ap.add_argument('--warmup', type=int, default=2)
    a = ap.parse_args()
    for name in a.shapes.split(','):
        I, D, rows, C = SHAPES[name]
        for act in a.acts.split(','):
            rng = np.random.RandomState(0)
            m = serving_model(I, D, rows, act, rng)
            in_idx = rng.randint(0, I, size=rows).astype(np.int32)
            cand = rng.randint(0, I, size=rows * C).astype(np.int32)
            offs = (np.arange(rows + 1) * C).astype(np.int64)
            union = np.unique(cand).astype(np.int32)
            m.predict_begin(rows)
            t_none = timed(lambda: m.score_candidates(in_idx, offs, cand, 0), a.seconds, a.warmup)
            t_k = timed(lambda: m.score_candidates(in_idx, offs, cand, 20), a.seconds, a.warmup)
            t_union = timed(lambda: m.predict_step(in_idx, union), a.seconds, 1)
            t_full = timed(lambda: m.recommend_step(in_idx, None, 20), a.seconds, 1)
            gathered = rows * C * D * 4
            print(json.dumps(dict(shape=name, n_items=I, D=D, rows=rows, C=C, final_act=act, union_cols=len(union),
                                  us_none=round(t_none, 1), us_k20=round(t_k, 1), us_union=round(t_union, 1), us_full_topk=round(t_full, 1),
                                  speedup_vs_union=round(t_union / t_none, 2), speedup_k20_vs_full_topk=round(t_full / t_k, 2),
                                  gathered_MB=round(gathered / 1e6, 1), gather_TBps_call=round(gathered / t_none / 1e6, 3),
                                  frac_8TBps_call=round(gathered / t_none / 1e6 / 8.0, 4))), flush=True)
            m.close()


if __name__ == '__main__':
    main()

"""Times the two-stage top-k (g4r_recommend_step_scan: bf16 scan, exact fp32 re-rank) against the exact call (g4r_recommend_step) in
the same process, same model, same inputs.  One JSON line per shape, appended to --out when given:

  python tools/bench_recommend_scan.py [--shapes 10M,rsc15] [--k 20] [--oversample 8] [--calls 15] [--warmup 3] [--out FILE]

Shapes: 10M = 10,000,000 items, D = 256, 512 rows; rsc15 = 37,483 items, D = 100, 128 rows.  Weights are random (N(0, 0.1), a
different row for every item: the scan's survivor traffic depends on the score distribution, so no repeated block here).
Fields: ms_fp32 / ms_bf16: median wall time of a synchronous call (uploads, the GRU step, the selection and the copy back) after
--warmup calls; the first bf16 call, which builds the shadow table, is timed apart (ms_bf16_first); speedup = ms_fp32 / ms_bf16;
overlap: mean share of the exact top k the two-stage call returned; table_MB: the shadow table.  Kernel times do not come from
this script: run it under `rocprofv3 --kernel-trace --stats -- python tools/bench_recommend_scan.py --calls 3 --warmup 1` in a
run of its own and read k_scan_bf16 / k_topk_range / k_scan_merge / k_score_cand from the kernel statistics."""
import argparse
import json
import time

import numpy as np

from bench_common import dense_weights, serving_model

SHAPES = {'10M': (10_000_000, 256, 512), 'rsc15': (37_483, 100, 128)}


def median_ms(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return float(np.median(t) * 1e3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='10M,rsc15')
    ap.add_argument('--k', type=int, default=20)
    ap.add_argument('--oversample', type=int, default=8)
    ap.add_argument('--calls', type=int, default=15)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    for name in a.shapes.split(','):
        I, D, rows = SHAPES[name]
        rng = np.random.default_rng(0)
        m = serving_model(I, D, rows, 'linear', rng, weights=dense_weights)
        in_idx = rng.integers(0, I, size=rows).astype(np.int32)
        m.predict_begin(rows)
        t0 = time.perf_counter()
        m.recommend_step_filtered(in_idx, None, a.k, oversample=a.oversample)
        first = (time.perf_counter() - t0) * 1e3
        ms_bf16 = median_ms(lambda: m.recommend_step_filtered(in_idx, None, a.k, oversample=a.oversample), a.calls, a.warmup)
        ms_fp32 = median_ms(lambda: m.recommend_step(in_idx, None, a.k), a.calls, a.warmup)
        m.predict_begin(rows)
        ec, _ = m.recommend_step(in_idx, None, a.k)
        m.predict_begin(rows)
        sc, _ = m.recommend_step_filtered(in_idx, None, a.k, oversample=a.oversample)
        overlap = float(np.mean([len(set(x) & set(y)) / a.k for x, y in zip(ec, sc)]))
        line = json.dumps(dict(shape=name, n_items=I, D=D, rows=rows, k=a.k, oversample=a.oversample, ms_fp32=round(ms_fp32, 3),
                               ms_bf16=round(ms_bf16, 3), ms_bf16_first=round(first, 3), speedup=round(ms_fp32 / ms_bf16, 2),
                               overlap=round(overlap, 4), table_MB=round(m.scan_table()[0] / 1e6, 1)))
        print(line, flush=True)
        if a.out:
            with open(a.out, 'a') as f:
                f.write(line + '\n')
        m.close()


if __name__ == '__main__':
    main()

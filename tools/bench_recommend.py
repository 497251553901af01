"""Times g4r_recommend_step (top-k on the device) against g4r_predict_step(want_scores=False) -- the same GRU forward plus the full score
matrix written to HBM, nothing copied back -- at the same shape and hidden state.  One JSON line per (shape, final activation):

  python tools/bench_recommend.py [--shapes 10M,rsc15] [--acts linear,softmax] [--seconds 1.0] [--warmup 3] [--exclude E,F]

--exclude E,F adds g4r_recommend_step_filtered at the same shape: E random items excluded per row plus a random fraction F of the
catalogue in the global mask (us_recommend_filtered, and ratio_filtered = filtered / unfiltered recommend_step).

Each time is the mean of back-to-back synchronous calls over a window of at least --seconds after the warm-up.  mfma_frac: the
scoring GEMM (2 * rows * n_items * D flop) over the call's time, as a fraction of the 157.3 TFLOP/s fp32 MFMA peak."""
import argparse
import json
import time

import numpy as np

from bench_common import serving_model

PEAK = 157.3e12
SHAPES = {'10M': (10_000_000, 256, 512, 20), 'rsc15': (37_483, 100, 128, 20)}


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
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--exclude', default=None, help='E,F: E items per row, fraction F of the catalogue masked')
    a = ap.parse_args()
    excl = None if a.exclude is None else (int(a.exclude.split(',')[0]), float(a.exclude.split(',')[1]))
    for name in a.shapes.split(','):
        I, D, rows, k = SHAPES[name]
        for act in a.acts.split(','):
            rng = np.random.RandomState(0)
            m = serving_model(I, D, rows, act, rng)
            in_idx = rng.randint(0, I, size=rows).astype(np.int32)
            m.predict_begin(rows)
            # the hidden state advances every call (as in serving); both calls see the same sequence of states
            t_rec = timed(lambda: m.recommend_step(in_idx, None, k), a.seconds, a.warmup)
            m.predict_begin(rows)
            t_pred = timed(lambda: m.predict_step(in_idx, want_scores=False), a.seconds, a.warmup)
            flop = 2.0 * rows * I * D
            out = dict(shape=name, n_items=I, D=D, rows=rows, k=k, final_act=act, us_recommend_step=round(t_rec, 1),
                       us_predict_step_no_copy=round(t_pred, 1), ratio=round(t_rec / t_pred, 3),
                       mfma_frac_recommend=round(flop / (t_rec * 1e-6) / PEAK, 4), mfma_frac_predict=round(flop / (t_pred * 1e-6) / PEAK, 4))
            if excl is not None:
                E, F = excl
                items = rng.randint(0, I, size=rows * E).astype(np.int32)      # (a repeat is allowed: the host de-duplicates)
                offs = np.arange(rows + 1, dtype=np.int64) * E
                mask = np.zeros((I + 31) // 32, dtype=np.uint32)
                gl = np.unique(rng.randint(0, I, size=int(F * I)))
                np.bitwise_or.at(mask, gl >> 5, np.left_shift(1, gl & 31).astype(np.uint32))
                m.predict_begin(rows)
                t_x = timed(lambda: m.recommend_step_filtered(in_idx, None, k, offs, items, mask), a.seconds, a.warmup)
                out.update(exclude_per_row=E, exclude_frac=F, us_recommend_filtered=round(t_x, 1), ratio_filtered=round(t_x / t_rec, 3))
            print(json.dumps(out), flush=True)
            m.close()


if __name__ == '__main__':
    main()

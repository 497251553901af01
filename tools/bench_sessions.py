"""Times g4r_recommend_sessions (stateless top-k after replaying whole histories) against g4r_recommend_step at the same shape, and
against the cheapest stepwise route through the prediction state (T - 1 g4r_predict_step calls with a one-item candidate list, then
one g4r_recommend_step).  One JSON line per (shape, final activation, history lengths):

  python tools/bench_sessions.py [--shapes 10M,rsc15] [--acts linear,softmax] [--lens 1,20,synth] [--seconds 1.0] [--warmup 2]

--lens: T = every history that long; 'synth' = the session lengths of gru4rec_amd.synth.make_sessions (2 + geometric, up to 200).
Fields: us_sessions (the call), us_recommend_step, ratio_to_step = us_sessions / us_recommend_step, us_stepwise (the stepwise route
for the longest history: the slots of shorter ones would idle through the rest) and speedup_vs_stepwise; ratio_T_to_T1 compares a
call with its T = 1 call at the same shape and activation when --lens holds 1 before it.  Each time is the mean of back-to-back
synchronous calls over a window of at least --seconds after the warm-up."""
import argparse
import json
import time

import numpy as np

from bench_common import serving_model      # (first: it puts the repository root on sys.path)
from gru4rec_amd import synth

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


def lengths(spec, rows):
    if spec == 'synth':
        d = synth.make_sessions(rows, seed=7)
        return d.groupby('SessionId').size().values.astype(np.int64)[:rows]
    return np.full(rows, int(spec), dtype=np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='10M,rsc15')
    ap.add_argument('--acts', default='linear,softmax')
    ap.add_argument('--lens', default='1,20,synth')
    ap.add_argument('--seconds', type=float, default=1.0)
    ap.add_argument('--warmup', type=int, default=2)
    a = ap.parse_args()
    for name in a.shapes.split(','):
        I, D, rows, k = SHAPES[name]
        for act in a.acts.split(','):
            rng = np.random.RandomState(0)
            m = serving_model(I, D, rows, act, rng)
            in_idx = rng.randint(0, I, size=rows).astype(np.int32)
            one = np.zeros(1, dtype=np.int32)
            m.predict_begin(rows)
            t_rec = timed(lambda: m.recommend_step(in_idx, None, k), a.seconds, a.warmup)
            t1 = None
            for spec in a.lens.split(','):
                lens = lengths(spec, rows)
                offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
                items = rng.randint(0, I, size=int(offs[-1])).astype(np.int32)
                t_s = timed(lambda: m.recommend_sessions(offs, items, None, k), a.seconds, a.warmup)
                T = int(lens.max())

                def stepwise():
                    m.predict_begin(rows)
                    for _ in range(T - 1):
                        m.predict_step(in_idx, one)
                    m.recommend_step(in_idx, None, k)
                t_w = timed(stepwise, a.seconds, 1)
                out = dict(shape=name, n_items=I, D=D, rows=rows, k=k, final_act=act, lens=spec, T_max=T, T_mean=round(float(lens.mean()), 2),
                           us_sessions=round(t_s, 1), us_recommend_step=round(t_rec, 1), ratio_to_step=round(t_s / t_rec, 3),
                           us_stepwise=round(t_w, 1), speedup_vs_stepwise=round(t_w / t_s, 3))
                if spec == '1':
                    t1 = t_s
                elif t1 is not None:
                    out['ratio_T_to_T1'] = round(t_s / t1, 3)
                print(json.dumps(out), flush=True)
            m.close()


if __name__ == '__main__':
    main()

"""Times recommend_sessions(nprobe=) over an item index against scan='fp32' and scan='bf16' in the same process, same model, same
histories, and measures its recall on a trained model.  One JSON line per measurement, appended to --out when given:

  python tools/bench_item_index.py [--parts time,recall] [--shapes 10M,rsc15] [--rows 1,16,512] [--nprobe 1,4,16,64] [--k 20]
                                   [--oversample 8] [--calls 15] [--warmup 3] [--iters N] [--out FILE]

time.    Shapes: 10M = 10,000,000 items, D = 256; rsc15 = 37,483 items, D = 100.  Weights are random (N(0, 0.1), every row drawn).
         The index has the default number of lists; --iters rounds of k-means (default: 0 at 10M -- the centroids are a sample of the
         items, which skips the host k-means and leaves the device assignment -- and 10 at rsc15).  Histories hold one item.  Fields:
         ms_fp32 / ms_bf16 / ms_ivf: median wall time of a synchronous call after --warmup calls; build: the statistics
         build_item_index returns; index_MB: the index's device tables.  Kernel times do not come from this script: run it under
         `rocprofv3 --kernel-trace --stats -- python tools/bench_item_index.py --parts time --calls 3 --warmup 1` in a run of its own.
recall.  A model of 100 units trained for --epochs epochs on synth.make_sessions data (--sessions sessions, 37,483 items); the test
         histories are the prefixes of held-out sessions.  recall_at_k: the mean share of the exact top k (scan='fp32') the call
         returned; found_mean: the mean number of entries a row received."""
import argparse
import json
import time

import numpy as np

from bench_common import as_gru4rec, dense_weights, serving_model
from gru4rec_amd import synth
from gru4rec_amd.gru4rec import GRU4Rec

SHAPES = {'10M': (10_000_000, 256), 'rsc15': (37_483, 100)}


def median_ms(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return float(np.median(t) * 1e3)


def emit(a, **fields):
    line = json.dumps(fields)
    print(line, flush=True)
    if a.out:
        with open(a.out, 'a') as f:
            f.write(line + '\n')


def probes_of(a, n_lists):
    return [p for p in a.nprobe if p <= n_lists and p * min(a.k * a.oversample, 1024) <= 65536]


def part_time(a):
    for name in a.shapes:
        I, D = SHAPES[name]
        rng = np.random.default_rng(0)
        keep = {'Wy': None, 'By': None}
        m = serving_model(I, D, max(a.rows), 'linear', rng, weights=dense_weights, keep=keep)
        g = as_gru4rec(m, I, D, 'linear')
        g.Wy, g.By = keep['Wy'], keep['By'].reshape(-1, 1)
        iters = a.iters if a.iters is not None else (0 if I > 1_000_000 else 10)
        stats = g.build_item_index(iters=iters)
        info = m.ivf_info()
        emit(a, part='build', shape=name, n_items=I, D=D, iters=iters, index_MB=round(info[2] / 1e6, 1), blocks=info[1],
             build={k: (round(v, 3) if isinstance(v, float) else v) for k, v in stats.items()})
        ids = g.itemidmap.index.values
        for rows in a.rows:
            hs = [[i] for i in ids[rng.integers(0, I, size=rows)]]
            ms_fp32 = median_ms(lambda: g.recommend_sessions(hs, k=a.k), a.calls, a.warmup)
            ms_bf16 = median_ms(lambda: g.recommend_sessions(hs, k=a.k, scan='bf16', oversample=a.oversample), a.calls, a.warmup)
            exact = g.recommend_sessions(hs, k=a.k)[0]
            for p in probes_of(a, stats['n_lists']):
                ms = median_ms(lambda: g.recommend_sessions(hs, k=a.k, oversample=a.oversample, nprobe=p), a.calls, a.warmup)
                got, _, found = g.recommend_sessions(hs, k=a.k, oversample=a.oversample, nprobe=p)
                rec = float(np.mean([len(set(x) & set(y[:n])) / a.k for x, y, n in zip(exact, got, found)]))
                emit(a, part='time', shape=name, rows=rows, k=a.k, oversample=a.oversample, nprobe=p, ms_fp32=round(ms_fp32, 3),
                     ms_bf16=round(ms_bf16, 3), ms_ivf=round(ms, 3), recall_random_weights=round(rec, 4), found_mean=round(float(found.mean()), 2))
        m.scan_table_release()
        g.drop_item_index()
        m.close()


def part_recall(a):
    data = synth.make_sessions(a.sessions)
    train, test = synth.train_test_split(data)
    g = GRU4Rec(layers=[100], loss='bpr-max', final_act='elu-0.5', n_epochs=a.epochs, batch_size=128, n_sample=2048, learning_rate=0.1,
                momentum=0.0, sample_alpha=0.5, bpreg=1.0, constrained_embedding=True)
    g.fit(train)
    hs = [grp.ItemId.values[:-1] for _, grp in test.groupby('SessionId')][:a.recall_rows]
    hs = [h for h in hs if len(h)]
    exact = g.recommend_sessions(hs, k=a.k)[0]
    bf16 = g.recommend_sessions(hs, k=a.k, scan='bf16', oversample=a.oversample)[0]
    stats = g.build_item_index()
    emit(a, part='recall_build', n_items=g.n_items, rows=len(hs), build={k: (round(v, 3) if isinstance(v, float) else v) for k, v in stats.items()},
         recall_bf16=round(float(np.mean([len(set(x) & set(y)) / a.k for x, y in zip(exact, bf16)])), 4))
    for p in probes_of(a, stats['n_lists']):
        got, _, found = g.recommend_sessions(hs, k=a.k, oversample=a.oversample, nprobe=p)
        rec = float(np.mean([len(set(x) & set(y[:n])) / a.k for x, y, n in zip(exact, got, found)]))
        emit(a, part='recall', nprobe=p, k=a.k, oversample=a.oversample, recall_at_k=round(rec, 4), found_mean=round(float(found.mean()), 2),
             share_of_items_probed=round(p / stats['n_lists'], 4))


def main():
    ints = lambda s: [int(x) for x in s.split(',')]      # noqa: E731
    ap = argparse.ArgumentParser()
    ap.add_argument('--parts', default='time,recall')
    ap.add_argument('--shapes', type=lambda s: s.split(','), default=['10M', 'rsc15'])
    ap.add_argument('--rows', type=ints, default=[1, 16, 512])
    ap.add_argument('--nprobe', type=ints, default=[1, 4, 16, 64])
    ap.add_argument('--k', type=int, default=20)
    ap.add_argument('--oversample', type=int, default=8)
    ap.add_argument('--calls', type=int, default=15)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--iters', type=int, default=None)
    ap.add_argument('--sessions', type=int, default=300000)
    ap.add_argument('--epochs', type=int, default=3)
    ap.add_argument('--recall-rows', type=int, default=2000)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if 'recall' in a.parts:
        part_recall(a)
    if 'time' in a.parts:
        part_time(a)


if __name__ == '__main__':
    main()

"""Times g4r_similar_items (GRU4Rec.similar_items / item_neighbors).  One JSON line per measurement, appended to --out when given:

  python tools/bench_similar_items.py [--what chunk,table,norms] [--k 20] [--calls 9] [--warmup 2] [--out FILE]

chunk   512 queries, cosine, at 37,483 x 100 and 10,000,000 x 256, against g4r_recommend_step at the same rows x items x width in the
        same process, the two calls alternating (the recommend kernels are instruction for instruction those of the commit before
        this feature: the build's listing shows it).  ms_* are (min, median, max) wall times of synchronous calls; the spread of the
        recommend call is the margin of the comparison.
table   the whole neighbour table (all items as queries) at 37,483 x 100 and 1,000,000 x 128: seconds, the achieved share of the fp32
        MFMA peak (2 n^2 D flop over 157.3 TFLOP/s), the bytes one chunk needs from HBM by the model of DESIGN.md (the table once, the
        chunk's query rows, its lists) -- and the host baseline: float32 BLAS product + argpartition + sort in chunks of --host-rows
        query rows on the CPUs the process may use.  The host baseline runs --host-chunks chunks and is scaled to the table
        (host_extrapolated = true when that is not all of it).
norms   k_item_norms at 10,000,000 x 256: wall time of the first cosine call after an upload minus that of the next one (the same
        call with the norms cached), and the share of the HBM peak (8 TB/s spec; 6.29 TB/s measured copy) that makes of n x D x 4 bytes.
Kernel times do not come from this script: run it under `rocprofv3 --kernel-trace --stats -- python tools/bench_similar_items.py
--calls 3 --warmup 1` in a run of its own and read k_sim_range / k_item_norms / k_topk_merge from the kernel statistics."""
import argparse
import json
import os
import time

import numpy as np

from bench_common import dense_weights, serving_model

PEAK_F32_MFMA = 157.3e12
PEAK_HBM = 8.0e12
CHUNK_ROWS = 4096      # G4R_SIM_CHUNK_ROWS


def model(I, D, rows, rng, keep_table=False):
    kept = {'Wy': None} if keep_table else None
    m = serving_model(I, D, rows, 'linear', rng, weights=dense_weights, keep=kept)
    return m, (kept['Wy'] if keep_table else None)


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def stats(t):
    return [round(float(x), 3) for x in (np.min(t), np.median(t), np.max(t))]


def emit(a, **kw):
    line = json.dumps(kw)
    print(line, flush=True)
    if a.out:
        with open(a.out, 'a') as f:
            f.write(line + '\n')


def bench_chunk(a, I, D, rows=512, norms=False):
    rng = np.random.default_rng(0)
    m, _ = model(I, D, rows, rng)
    q = rng.integers(0, I, size=rows).astype(np.int32)
    m.predict_begin(rows)
    sim = lambda: m.similar_items(q, None, a.k, 'cosine')      # noqa: E731
    rec = lambda: m.recommend_step(q, None, a.k)               # noqa: E731
    for _ in range(a.warmup):
        sim(); rec()
    ts, tr = [], []
    for _ in range(a.calls):      # alternating: what disturbs one disturbs the other
        ts.append(timed(sim)); tr.append(timed(rec))
    emit(a, what='chunk', n_items=I, D=D, rows=rows, k=a.k, ms_similar=stats(ts), ms_recommend=stats(tr),
         ratio_of_medians=round(float(np.median(ts) / np.median(tr)), 4),
         recommend_spread=round(float((np.max(tr) - np.min(tr)) / np.median(tr)), 4))
    if norms:      # (on the table that is already there: drawing and uploading 10 GB takes longer than every measurement here)
        bench_norms(a, m, I, D)
    m.close()


def host_neighbours(T, q0, q1, k):
    """cosine top k of query rows [q0, q1) on the host: float32 BLAS product, argpartition, sort of the k kept."""
    inv = 1.0 / np.sqrt((T * T).sum(1, dtype=np.float32))
    S = (T[q0:q1] * inv[q0:q1, None]) @ T.T
    S *= inv[None, :]
    S[np.arange(q1 - q0), np.arange(q0, q1)] = -np.inf
    part = np.argpartition(-S, k - 1, axis=1)[:, :k]
    sc = np.take_along_axis(S, part, 1)
    o = np.argsort(-sc, axis=1, kind='stable')
    return np.take_along_axis(part, o, 1), np.take_along_axis(sc, o, 1)


def bench_table(a, I, D):
    rng = np.random.default_rng(0)
    m, T = model(I, D, 32, rng, keep_table=True)
    q = np.arange(I, dtype=np.int32)
    m.similar_items(q[:CHUNK_ROWS], None, a.k, 'cosine')      # warm-up: code objects, buffers, the norms
    t0 = time.perf_counter()
    cols, _ = m.similar_items(q, None, a.k, 'cosine')
    sec = time.perf_counter() - t0
    flop = 2.0 * I * I * D
    # HBM bytes of one chunk: the table once, the inverse norms once, the chunk's query rows, the per-range lists
    # written by the scan and read by the merge (ranges = compute units / row blocks), the result
    rows_c = min(I, CHUNK_ROWS)
    ranges = max(1, a.cus // ((rows_c + 127) // 128))
    hbm_chunk = I * D * 4 + I * 4 + rows_c * D * 4 + 2 * rows_c * ranges * a.k * 8 + rows_c * a.k * 8
    n_host = min((I + a.host_rows - 1) // a.host_rows, a.host_chunks)
    t0 = time.perf_counter()
    same = []
    for c in range(n_host):
        q0, q1 = c * a.host_rows, min(I, (c + 1) * a.host_rows)
        hc, _ = host_neighbours(T, q0, q1, a.k)
        same.append(np.mean([len(set(x) & set(y)) / a.k for x, y in zip(hc, cols[q0:q1])]))
    host = (time.perf_counter() - t0) * I / min(I, n_host * a.host_rows)
    emit(a, what='table', n_items=I, D=D, k=a.k, seconds=round(sec, 4), tflops=round(flop / sec / 1e12, 2),
         mfma_fraction=round(flop / sec / PEAK_F32_MFMA, 4), chunks=(I + CHUNK_ROWS - 1) // CHUNK_ROWS, hbm_bytes_per_chunk_model=int(hbm_chunk),
         host_seconds=round(host, 2), host_extrapolated=bool(n_host * a.host_rows < I), host_threads=int(os.environ.get('OMP_NUM_THREADS') or len(os.sched_getaffinity(0))),
         host_over_device=round(host / sec, 1), overlap_with_host=round(float(np.mean(same)), 4))
    m.close()


def bench_norms(a, m, I, D):
    q = np.zeros(1, dtype=np.int32)
    by = np.zeros(I, dtype=np.float32)
    m.similar_items(q, None, a.k, 'cosine')
    first, cached = [], []
    for _ in range(max(3, a.calls // 2)):
        m.set_param('By', by)      # any upload invalidates the norms
        first.append(timed(lambda: m.similar_items(q, None, a.k, 'cosine')))
        cached.append(timed(lambda: m.similar_items(q, None, a.k, 'cosine')))
    ms = float(np.median(first) - np.median(cached))
    emit(a, what='norms', n_items=I, D=D, ms_first=stats(first), ms_cached=stats(cached), ms_norms=round(ms, 3),
         tb_per_s=round(I * D * 4 / (ms * 1e-3) / 1e12, 3), hbm_peak_fraction=round(I * D * 4 / (ms * 1e-3) / PEAK_HBM, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--what', default='chunk,table,norms')
    ap.add_argument('--k', type=int, default=20)
    ap.add_argument('--calls', type=int, default=9)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--small-only', action='store_true', help='the 37,483 x 100 shapes only')
    ap.add_argument('--host-rows', type=int, default=2048)
    ap.add_argument('--host-chunks', type=int, default=4)
    ap.add_argument('--cus', type=int, default=256, help='compute units of the device (the library sizes the ranges of a chunk by it)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    what = a.what.split(',')
    if 'chunk' in what or 'norms' in what:
        bench_chunk(a, 37_483, 100)
        if not a.small_only:
            bench_chunk(a, 10_000_000, 256, norms='norms' in what)
    if 'table' in what:
        bench_table(a, 37_483, 100)
        if not a.small_only:
            bench_table(a, 1_000_000, 128)


if __name__ == '__main__':
    main()

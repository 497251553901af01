"""Times GRU4Rec.sample_sessions (stochastic decoding on the device) against (a) continue_sessions(k=1) at the same rows and steps -- the
same replay, GRU steps and fused scan without the noise: the difference is what the noise costs -- and (b) the host loop the call
replaces: score_candidates_sessions over all items every step, the full score rows downloaded, a NumPy Gumbel argmax, the drawn items fed
back as one-item histories.  One process, one JSON line per case:

  timeout 900 python tools/bench_sample_sessions.py [--shapes rsc15,10M] [--steps 5,20] [--samples 1,8] [--top-ks 0,50] [--reps 5]
                                                    [--warmup 2] [--budget 600] [--label TEXT] [--md FILE]

Shapes: rsc15 = 37,483 items x 100 units, 10M = 10,000,000 items x 256 units (5 steps, samples 1, no top_k); 512 draw rows in all
(512 / samples sessions of 2 to 6 items), no_repeat on, temperature 0.7.  Every time is the median of --reps synchronous calls after
--warmup, with the spread (max - min) next to it.  At 10M the host loop is timed on --host-rows rows and scaled to 512 (its score rows
alone are 20 GB per step).  --budget: seconds after which no further case is started (the remaining ones are reported as not measured).
--label names the library in the table (a kernel experiment is a second run with G4R_LIB set to the variant library).  --md appends
the table of profiles/sample_sessions.md to FILE.  --legs (default logprobs,top_p,partition; '' for none) adds, per (shape, samples, steps) and
beside the untruncated case: sample_sessions(return_logprobs=True), sample_sessions(top_k=50, top_p=0.9) and -- once per shape and samples --
session_log_partition on the 512 histories of (a), history excluded.  Kernel times do not come from this script: run it under
`rocprofv3 --kernel-trace --stats -- python tools/bench_sample_sessions.py --shapes rsc15 --steps 20 --samples 1 --top-ks 0 --reps 3
--warmup 1 --call-only` in a run of its own."""
import argparse
import json
import time

import numpy as np

from bench_common import as_gru4rec, serving_model

SHAPES = {'rsc15': (37_483, 100), '10M': (10_000_000, 256)}
ROWS = 512
TEMPERATURE = 0.7


def host_loop(m, hoffs, hidx, n_items, steps, inv_t, rng, rows_per_call):
    """(b) on the device model's own interface (no id mapping): rows in slices of rows_per_call, so that a slice's candidate positions
    stay below G4R_CAND_MAX."""
    N = len(hoffs) - 1
    out = np.empty((N, steps), dtype=np.int64)
    for r0 in range(0, N, rows_per_call):
        r1 = min(N, r0 + rows_per_call)
        n = r1 - r0
        offs = hoffs[r0:r1 + 1] - hoffs[r0]
        items = hidx[hoffs[r0]:hoffs[r1]]
        coffs = np.arange(n + 1, dtype=np.int64) * n_items
        cidx = np.tile(np.arange(n_items, dtype=np.int32), n)
        gone = np.zeros((n, n_items), dtype=bool)
        gone[np.repeat(np.arange(n), np.diff(offs)), items] = True
        H = None
        for s in range(steps):
            z, H = m.score_candidates_sessions(offs, items, coffs, cidx, 0, hidden=H, return_hidden=True)
            key = z.reshape(n, n_items) * np.float32(inv_t) + rng.gumbel(size=(n, n_items)).astype(np.float32)
            key[gone] = -np.inf
            pick = key.argmax(axis=1)
            out[r0:r1, s] = pick
            gone[np.arange(n), pick] = True
            offs, items = np.arange(n + 1, dtype=np.int64), pick.astype(np.int32)
    return out


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(ts)), 2), round(float(max(ts) - min(ts)), 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='rsc15,10M')
    ap.add_argument('--steps', default='5,20')
    ap.add_argument('--samples', default='1,8')
    ap.add_argument('--top-ks', default='0,50')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--host-rows', type=int, default=8, help='rows the host loop is timed on at the 10M shape')
    ap.add_argument('--budget', type=float, default=600.0)
    ap.add_argument('--label', default='product')
    ap.add_argument('--md', default=None)
    ap.add_argument('--legs', default='logprobs,top_p,partition', help='the log-probability / nucleus / log-partition legs to time')
    ap.add_argument('--call-only', action='store_true', help='time sample_sessions alone (for a kernel trace)')
    a = ap.parse_args()
    t_start = time.perf_counter()
    rows = []
    legs = [x for x in a.legs.split(',') if x]
    for name in a.shapes.split(','):
        I, D = SHAPES[name]
        rng = np.random.RandomState(0)
        g = as_gru4rec(serving_model(I, D, ROWS, 'linear', rng), I, D, 'linear')
        m = g._model
        ids = g.itemidmap.index.values
        for samples in [int(x) for x in a.samples.split(',')]:
            if name == '10M' and samples != 1:
                continue
            N = ROWS // samples
            hists = [ids[rng.randint(0, I, size=n)] for n in rng.randint(2, 7, size=N)]
            wide = [ids[rng.randint(0, I, size=n)] for n in rng.randint(2, 7, size=ROWS)]      # (a): the same number of ROWS
            for steps in [int(s) for s in a.steps.split(',')]:
                if name == '10M' and steps != 5:
                    continue
                base = None
                for top_k in [int(x) for x in a.top_ks.split(',')]:
                    if name == '10M' and top_k:
                        continue
                    out = dict(shape=name, n_items=I, D=D, rows=ROWS, samples=samples, steps=steps, top_k=top_k or None, label=a.label)
                    if time.perf_counter() - t_start > a.budget:
                        out.update(not_measured='the time budget of the run was used up')
                        print(json.dumps(out), flush=True)
                        continue
                    kw = dict(samples=samples, temperature=TEMPERATURE, top_k=top_k or None, seed=7)
                    out['ms_sample'], out['spread_sample'] = timed(lambda: g.sample_sessions(hists, steps, **kw), a.reps, a.warmup)
                    if not top_k:
                        if 'logprobs' in legs:
                            out['ms_logprobs'], out['spread_logprobs'] = timed(lambda: g.sample_sessions(hists, steps, return_logprobs=True, **kw),
                                                                               a.reps, a.warmup)
                        if 'top_p' in legs:
                            kp = dict(kw, top_k=50, top_p=0.9)
                            out['ms_top_p'], out['spread_top_p'] = timed(lambda: g.sample_sessions(hists, steps, **kp), a.reps, a.warmup)
                        if 'partition' in legs and steps == int(a.steps.split(',')[0]):
                            out['ms_partition'], out['spread_partition'] = timed(
                                lambda: g.session_log_partition(wide, temperature=TEMPERATURE, exclude_history=True), a.reps, a.warmup)
                    if not a.call_only:
                        if base is None:      # (a) does not depend on top_k
                            base = timed(lambda: g.continue_sessions(wide, steps, k=1), a.reps, a.warmup)
                        out['ms_continue'], out['spread_continue'] = base
                        out['sample_over_continue'] = round(out['ms_sample'] / base[0], 2)
                        if not top_k:      # (b) draws from the untruncated distribution
                            hr = ROWS if name != '10M' else a.host_rows
                            hoffs = np.concatenate([[0], np.cumsum([len(h) for h in wide[:hr]])]).astype(np.int64)
                            hidx = g.itemidmap[np.concatenate(wide[:hr])].values.astype(np.int32)
                            per = max(1, min(hr, (2 ** 31 - 256) // I))
                            nrng = np.random.default_rng(0)
                            t_h, s_h = timed(lambda: host_loop(m, hoffs, hidx, I, steps, 1.0 / TEMPERATURE, nrng, per), max(1, a.reps // 2), 1)
                            scale = ROWS / hr
                            out.update(ms_host_loop=round(t_h * scale, 1), spread_host_loop=round(s_h * scale, 1), host_rows_timed=hr,
                                       host_over_sample=round(t_h * scale / out['ms_sample'], 1))
                    print(json.dumps(out), flush=True)
                    rows.append(out)
        g.close()
    if a.md and rows and not a.call_only:
        with open(a.md, 'a') as f:
            f.write('\n### %s\n\n| shape | samples | steps | top_k | sample_sessions ms (spread) | continue_sessions(k=1) ms (spread) | sample / continue | '
                    'host loop ms (spread; rows timed) | host loop / sample |\n|---|---|---|---|---|---|---|---|---|\n' % a.label)
            for r in rows:
                if 'ms_sample' not in r:
                    f.write('| %s | %d | %d | %s | not measured | | | | |\n' % (r['shape'], r['samples'], r['steps'], r['top_k'] or '-'))
                    continue
                host = '%.1f (%.1f; %d)' % (r['ms_host_loop'], r['spread_host_loop'], r['host_rows_timed']) if 'ms_host_loop' in r else '-'
                f.write('| %s | %d | %d | %s | %.2f (%.2f) | %.2f (%.2f) | %.2f | %s | %s |\n' % (
                    r['shape'], r['samples'], r['steps'], r['top_k'] or '-', r['ms_sample'], r['spread_sample'], r['ms_continue'],
                    r['spread_continue'], r['sample_over_continue'], host, r.get('host_over_sample', '-')))
    if a.md and legs and any('ms_logprobs' in r or 'ms_top_p' in r or 'ms_partition' in r for r in rows):
        cell = (lambda r, k: '%.2f (%.2f)' % (r['ms_' + k], r['spread_' + k]) if 'ms_' + k in r else '-')
        with open(a.md, 'a') as f:
            f.write('\n### %s: log-probabilities, nucleus, log-partition\n\n| shape | samples | steps | sample_sessions ms (spread) | return_logprobs ms '
                    '(spread) | logprobs / plain | top_k=50, top_p=0.9 ms (spread) | session_log_partition, 512 sessions ms (spread) |\n'
                    '|---|---|---|---|---|---|---|---|\n' % a.label)
            for r in rows:
                if r['top_k'] or 'ms_sample' not in r:
                    continue
                ratio = '%.2f' % (r['ms_logprobs'] / r['ms_sample']) if 'ms_logprobs' in r else '-'
                f.write('| %s | %d | %d | %s | %s | %s | %s | %s |\n' % (r['shape'], r['samples'], r['steps'], cell(r, 'sample'), cell(r, 'logprobs'), ratio,
                                                                       cell(r, 'top_p'), cell(r, 'partition')))


if __name__ == '__main__':
    main()

"""The cap rule of include/gru4rec_hip.h on the host, shared by tests/test_group_caps_args.py and tests/test_gpu_group_caps.py.

A row's list has P positions with the groups g (-1 = ungrouped), a cap c >= 1 and a prior multiset of groups.  Position j is kept iff
g_j < 0 or n0(g_j) + #{i < j : g_i == g_j} < c; the result is the first min(k, kept) kept positions in list order."""
from collections import Counter

import numpy as np


def cap_rule(groups, k, cap, prior=()):
    """The rule as NumPy states it: (pos int32[k], -1 behind the kept positions; n_kept)."""
    g = np.asarray(groups, dtype=np.int64)
    pr = np.asarray(prior, dtype=np.int64).reshape(-1)
    n0 = (g[:, None] == pr[None, :]).sum(axis=1)
    earlier = np.tril(g[:, None] == g[None, :], -1).sum(axis=1)
    kept = np.flatnonzero((g < 0) | (n0 + earlier < cap))[:k]
    pos = np.full(k, -1, dtype=np.int32)
    pos[:len(kept)] = kept
    return pos, len(kept)


def cap_walk(groups, k, cap, prior=()):
    """The same as the greedy walk down the list with one counter per group."""
    count = Counter(int(x) for x in prior)
    kept = []
    for j, g in enumerate(groups):
        if len(kept) == k:
            break
        if g < 0:
            kept.append(j)
        else:
            if count[int(g)] < cap:
                kept.append(j)
            count[int(g)] += 1
    return np.array(kept + [-1] * (k - len(kept)), dtype=np.int32), len(kept)


def apply_cap(items, scores, groups_of_items, k, cap, priors=None):
    """The rule over N pools (items[N, P] as item indices, scores[N, P]): (pos[N, k], n_kept[N], items[N, k] with -1 pads,
    scores[N, k] with NaN pads)."""
    N, P = items.shape
    pos = np.empty((N, k), dtype=np.int32)
    kept = np.empty(N, dtype=np.int32)
    for i in range(N):
        pos[i], kept[i] = cap_rule(groups_of_items[items[i]], k, cap, () if priors is None else priors[i])
    rows = np.arange(N)[:, None]
    pad = pos < 0
    out_items = np.where(pad, -1, items[rows, np.maximum(pos, 0)])
    out_scores = np.where(pad, np.float32('nan'), scores[rows, np.maximum(pos, 0)]).astype(np.float32)
    return pos, kept, out_items, out_scores

"""float64 helpers of the item-index tests (tests/test_ivf_ref.py checks them on hand-made cases; tests/test_gpu_item_index.py uses them).

Assignment rule.  Item i is the vector v = [Wy[i], By[i]] and list l has the objective J = v.c_l - |c_l|^2 / 2, in float64.  The device
forms J in fp32 -- D + 1 products summed one after the other, the half norm subtracted -- so what it compares is off by at most
    tau(v, c) = (D + 3) * 2^-24 * (|v| |c| + |c|^2 / 2)
per list (Cauchy-Schwarz bounds the sum of the |products|; the three extra roundings are the half norm's, its subtraction's and
slack).  A list is ACCEPTABLE for an item when its J is within the two lists' tau of the best J: J_best - J_l <= tau(v, c_l) +
tau(v, c_best) -- "within 2 tau".  The probe rule is the same bound on s = h.c_w + c_b with tau = (D + 3) * 2^-24 * (|h| |c_w| + |c_b|).
A check built on these is only worth something when nearly every item (pair) has ONE acceptable answer: `ambiguous_*` count the
others, and the tests assert that at most 1 % of their own inputs are."""
import numpy as np

U24 = 2.0 ** -24


def item_vectors(Wy, By):
    """[n_items, D + 1] float64: v_i = [Wy[i], By[i]]."""
    return np.concatenate([np.asarray(Wy, dtype=np.float64), np.asarray(By, dtype=np.float64).reshape(-1, 1)], axis=1)


def assign_objective(V, cen):
    """(J [n, n_lists], tau [n, n_lists]) of the assignment rule for item vectors V and centroids cen [n_lists, D + 1]."""
    V, cen = np.asarray(V, dtype=np.float64), np.asarray(cen, dtype=np.float64)
    half = 0.5 * (cen ** 2).sum(axis=1)
    J = V @ cen.T - half
    D = V.shape[1] - 1
    tau = (D + 3) * U24 * (np.linalg.norm(V, axis=1)[:, None] * np.linalg.norm(cen, axis=1)[None, :] + half[None, :])
    return J, tau


def acceptable(J, tau):
    """bool [n, n_lists]: list l is an acceptable answer for row i (J within the two taus of the row's best J)."""
    best = np.argmax(J, axis=1)
    rows = np.arange(len(J))
    return J[rows, best][:, None] - J <= tau + tau[rows, best][:, None]


def check_assignment(V, cen, lists):
    """(ok [n] -- the device's list of every item is acceptable --, the share of items with more than one acceptable list)."""
    J, tau = assign_objective(V, cen)
    acc = acceptable(J, tau)
    lists = np.asarray(lists)
    return acc[np.arange(len(J)), lists], float((acc.sum(axis=1) > 1).mean())


def probe_scores(H, cen):
    """(s [rows, n_lists], tau [rows, n_lists]) of the probe rule: s = h.c_w + c_b for final hidden states H [rows, D]."""
    H, cen = np.asarray(H, dtype=np.float64), np.asarray(cen, dtype=np.float64)
    cw, cb = cen[:, :-1], cen[:, -1]
    D = H.shape[1]
    s = H @ cw.T + cb
    tau = (D + 3) * U24 * (np.linalg.norm(H, axis=1)[:, None] * np.linalg.norm(cw, axis=1)[None, :] + np.abs(cb)[None, :])
    return s, tau


def check_probes(s, tau, probes):
    """(ok [rows], the share of (row, list) pairs that may fall on either side of the row's cut).  Row r's probes (list numbers, best
    first) are accepted when: they are distinct; consecutive ones do not rise by more than their two taus (equal scores: the lower
    list first); and no list left out beats a probed one by more than the two taus."""
    s, tau, probes = np.asarray(s), np.asarray(tau), np.asarray(probes)
    rows, nl = s.shape
    npb = probes.shape[1]
    ok = np.ones(rows, dtype=bool)
    amb = 0
    for r in range(rows):
        p = probes[r]
        if len(set(p.tolist())) != npb or p.min() < 0 or p.max() >= nl:
            ok[r] = False
            continue
        sp, tp = s[r, p], tau[r, p]
        for j in range(1, npb):
            if sp[j] - sp[j - 1] > tp[j] + tp[j - 1] or (sp[j] == sp[j - 1] and tp[j] == 0 and tp[j - 1] == 0 and p[j] < p[j - 1]):
                ok[r] = False
        out = np.setdiff1d(np.arange(nl), p)
        if len(out):
            j = int(np.argmin(sp))
            if (s[r, out] - sp[j] > tau[r, out] + tp[j]).any():
                ok[r] = False
        # the cut: the npb-th best score in float64; a list within the two taus of it (other than that list) is ambiguous
        order = np.lexsort((np.arange(nl), -s[r]))
        cut = order[npb - 1]
        near = np.abs(s[r] - s[r, cut]) <= tau[r] + tau[r, cut]
        near[cut] = False
        amb += int(near.sum())
    return ok, amb / float(rows * nl)


def topk_by_contract(scores, items, k):
    """The k best of (scores float32 [n], items int [n]) in the contract's order: score descending, equal scores (float ==) by the
    lower item, NaN last.  Returns positions into the two arrays."""
    scores = np.asarray(scores, dtype=np.float32)
    nan = np.isnan(scores)
    key = np.where(nan, 0.0, -scores.astype(np.float64))
    return np.lexsort((np.asarray(items), key, nan))[:k]

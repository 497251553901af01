"""Test-side reference of the log-probabilities and the nucleus of GRU4Rec.sample_sessions (not a test module): the host twin of the
contract's arithmetic -- d in NumPy float32, the terms q either from the device function (debug_lse_terms) or as an unrounded
float64, Q / C_j as Python integers, the nucleus rule and the final values in np.float64 -- and the host loop of sampling_ref
extended by them."""
import numpy as np

import sampling_ref as ref

SCALE = 2.0 ** 39


def d32(z, zeta, inv_t):
    """d = fl32(fl32(z - zeta) * inv_t): two float32 roundings."""
    with np.errstate(all='ignore'):
        return ((np.asarray(z, dtype=np.float32) - np.float32(zeta)).astype(np.float32) * np.float32(inv_t)).astype(np.float32)


def q64(d):
    """The unrounded term 2^39 * e^d in float64 (0 for a NaN d)."""
    d = np.asarray(d, dtype=np.float64)
    with np.errstate(all='ignore'):
        return np.where(np.isnan(d), 0.0, SCALE * np.exp(d))


def total(q):
    """The exact integer sum of the terms q."""
    return sum(int(x) for x in np.asarray(q).ravel().tolist())


def lse(zeta, inv_t, Q):
    """fl32(float64(zeta) * float64(inv_t) + log(float64(Q) * 2^-39))."""
    return np.float32(np.float64(np.float32(zeta)) * np.float64(np.float32(inv_t)) + np.log(np.float64(Q) * 2.0 ** -39))


def logprob(d_c, den):
    """fl32(float64(d_c) - log(float64(Den) * 2^-39))."""
    return np.float32(np.float64(np.float32(d_c)) - np.log(np.float64(den) * 2.0 ** -39))


def nucleus(q_best, top_p, Q):
    """(m, C_m): q_best the integer terms of the row's t best in the selection's order, Q the integer mass of the whole eligible set;
    m is the smallest j with float64(C_j) >= float64(fl32(top_p)) * float64(Q), or t when no prefix reaches that mass."""
    need = np.float64(np.float32(top_p)) * np.float64(Q)
    c = 0
    for j, q in enumerate(q_best):
        c += int(q)
        if np.float64(c) >= need:
            return j + 1, c
    return len(q_best), c


def draw(z, g, inv_t, eligible, terms, top_k=None, top_p=None):
    """One draw of the contract: (position, log-probability, zeta, Q or None).  z float32 logits of the candidate positions, g the
    float32 noise of their items, terms(z, zeta, inv_t) the integer terms (the device's, or q64 rounded)."""
    z = np.asarray(z, dtype=np.float32)
    by_z = ref.order(z, eligible)
    zeta = z[by_z[0]]
    Q = None
    if top_k is None or top_p is not None:
        Q = total(np.asarray(terms(z, zeta, inv_t))[eligible])
    if top_k is None:
        keep, den = eligible, Q
    else:
        best = by_z[:top_k]
        qb = [int(x) for x in np.asarray(terms(z[best], zeta, inv_t)).tolist()]
        m, den = (len(best), sum(qb)) if top_p is None else nucleus(qb, top_p, Q)
        keep = np.zeros(len(z), dtype=bool)
        keep[best[:m]] = True
    key = (z * np.float32(inv_t)).astype(np.float32) + np.asarray(g, dtype=np.float32)
    p = int(ref.order(key, keep)[0])
    return p, logprob(d32(z[p], zeta, inv_t), den), zeta, Q


def eligibility(g, hists, cand_ids, no_repeat, exclude, xpr):
    """[N, candidates] bool: the candidate positions row i may receive."""
    gone = set() if exclude is None else set(np.asarray(exclude).tolist())
    on = np.ones((len(hists), len(cand_ids)), dtype=bool)
    for i in range(len(hists)):
        out = set(gone)
        if no_repeat:
            out |= set(np.asarray(hists[i]).tolist())
        if xpr is not None:
            out |= set(np.asarray(list(xpr[i])).tolist())
        on[i] = ~np.isin(cand_ids, list(out))
    return on


def host_loop(g, hists, steps, samples=1, temperature=1.0, top_k=None, top_p=None, seed=0, first_step=0, no_repeat=True, cand=None,
              exclude=None, xpr=None, hidden=None, noise=None, terms=None):
    """sampling_ref.host_loop with the contract's log-probabilities and nucleus: per step every z over all candidates
    (score_candidates_sessions), the eligible set, zeta, the terms, Q / C_t / m, the argmax over the first m.  Returns (item_ids, scores,
    [hidden], logprobs), each [N, samples, steps] (hidden [N, samples, D])."""
    N, S = len(hists), samples
    cand_ids = g.itemidmap.index.values if cand is None else np.asarray(cand)
    cand_idx = g.itemidmap[cand_ids].values
    inv_t = np.float32(1.0) / np.float32(temperature)
    Z, H = g.score_candidates_sessions(hists, np.tile(cand_ids, (N, 1)), hidden=hidden, return_hidden=True)
    Z = np.repeat(np.asarray(Z, dtype=np.float32), S, axis=0)
    H = [np.repeat(h, S, axis=0) for h in H]
    eligible = np.repeat(eligibility(g, hists, cand_ids, no_repeat, exclude, xpr), S, axis=0)
    items = np.empty((N * S, steps), dtype=cand_ids.dtype)
    scores = np.empty((N * S, steps), dtype=np.float32)
    lps = np.empty((N * S, steps), dtype=np.float32)
    for s in range(steps):
        for q in range(N * S):
            p, lps[q, s], _, _ = draw(Z[q], noise(seed, q, first_step + s, cand_idx), inv_t, eligible[q], terms, top_k, top_p)
            items[q, s], scores[q, s] = cand_ids[p], Z[q, p]
            if no_repeat:
                eligible[q] &= cand_ids != cand_ids[p]
        if s < steps - 1:
            Z, H = g.score_candidates_sessions([[x] for x in items[:, s]], np.tile(cand_ids, (N * S, 1)), hidden=H, return_hidden=True)
            Z = np.asarray(Z, dtype=np.float32)
    return items.reshape(N, S, steps), scores.reshape(N, S, steps), [h.reshape(N, S, -1) for h in H], lps.reshape(N, S, steps)

"""Test-side reference of GRU4Rec.sample_sessions (not a test module): the float64 twin of the device's Gumbel noise, built on
oracle.philox, the selection rule, and the host replay loop of the contract -- candidate scores through score_candidates_sessions,
the key formed in NumPy float32, the argmax with the tie rule, the drawn item fed back as a one-item history."""
import numpy as np

from oracle.philox import philox4x32_10

STREAM_GUMBEL = 0x47554D42      # G4R_STREAM_GUMBEL


def uniform64(seed, q, step, items):
    """u of the contract, exactly (float64 holds it): lane item & 3 of the Philox call (item >> 2, q, step, STREAM_GUMBEL) keyed by
    seed's low and high word -> (x >> 9) * 2^-23 + 2^-24."""
    items = np.asarray(items, dtype=np.int64)
    r = philox4x32_10((items >> 2).astype(np.uint32), np.uint32(q & 0xFFFFFFFF), np.uint32(step & 0xFFFFFFFF), np.uint32(STREAM_GUMBEL),
                      seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    x = np.stack(r, axis=-1)[np.arange(len(items)), items & 3].astype(np.uint32)
    return (x >> np.uint32(9)).astype(np.float64) * 2.0 ** -23 + 2.0 ** -24


def g64(seed, q, step, items):
    """The Gumbel noise of (seed, row id q, step, item index) in float64: -log(-log(u))."""
    return -np.log(-np.log(uniform64(seed, q, step, items)))


def order(values, eligible):
    """The eligible positions in the selection's order: value descending, equal values (-0.0 == +0.0) by the lower position, NaN last."""
    pos = np.flatnonzero(eligible)
    v = np.asarray(values)[pos].astype(np.float64)
    nan = np.isnan(v)
    return pos[np.lexsort((pos, -np.where(nan, 0.0, v), nan))]


def choose(z, g, inv_t, eligible, top_k=None):
    """The position a draw takes: z float32 logits of the candidate positions, g float32 noise of their items, inv_t float32; the
    key is fl32(fl32(z * inv_t) + g); with top_k the eligible positions are first cut to the top_k best by z."""
    z, g = np.asarray(z, dtype=np.float32), np.asarray(g, dtype=np.float32)
    if top_k is not None:
        keep = np.zeros(len(z), dtype=bool)
        keep[order(z, eligible)[:top_k]] = True
        eligible = keep
    key = (z * np.float32(inv_t)).astype(np.float32) + g
    return int(order(key, eligible)[0])


def sample_counts(logits, draws, seed, inv_t=1.0, step=0):
    """The reference sampler alone: `draws` draws (row ids 0 .. draws - 1) over len(logits) items (item index = position) with the
    float64 noise rounded to float32: the count of every position."""
    logits = np.asarray(logits, dtype=np.float32)
    items = np.arange(len(logits))
    on = np.ones(len(logits), dtype=bool)
    counts = np.zeros(len(logits), dtype=np.int64)
    for q in range(draws):
        counts[choose(logits, g64(seed, q, step, items).astype(np.float32), np.float32(inv_t), on)] += 1
    return counts


def chi_square(counts, p):
    counts, p = np.asarray(counts, dtype=np.float64), np.asarray(p, dtype=np.float64)
    e = counts.sum() * p
    return float(((counts - e) ** 2 / e).sum())


def softmax64(z):
    z = np.asarray(z, dtype=np.float64)
    e = np.exp(z - z.max())
    return e / e.sum()


def host_loop(g, hists, steps, samples=1, temperature=1.0, top_k=None, seed=0, first_step=0, no_repeat=True, cand=None, exclude=None,
              xpr=None, hidden=None, noise=None):
    """The contract's route for final activations whose score IS the logit (not softmax / softmax_logit), out of calls that exist
    without sample_sessions: score_candidates_sessions over all candidates gives every z (predict_next_batch's bits) and the hidden
    state; noise(seed, q, step, item indices) the noise (the device's own through debug_gumbel, or g64 rounded).  Returns
    (item_ids[N, samples, steps], scores[N, samples, steps] float32, [hidden [N, samples, D] per layer])."""
    N, S = len(hists), samples
    cand_ids = g.itemidmap.index.values if cand is None else np.asarray(cand)
    cand_idx = g.itemidmap[cand_ids].values
    inv_t = np.float32(1.0) / np.float32(temperature)
    if noise is None:
        noise = lambda sd, q, st, it: g64(sd, q, st, it).astype(np.float32)
    Z, H = g.score_candidates_sessions(hists, np.tile(cand_ids, (N, 1)), hidden=hidden, return_hidden=True)
    Z = np.repeat(np.asarray(Z, dtype=np.float32), S, axis=0)
    H = [np.repeat(h, S, axis=0) for h in H]
    gone = set() if exclude is None else set(np.asarray(exclude).tolist())
    eligible = np.ones((N * S, len(cand_ids)), dtype=bool)
    for i in range(N):
        out = set(gone)
        if no_repeat:
            out |= set(np.asarray(hists[i]).tolist())
        if xpr is not None:
            out |= set(np.asarray(list(xpr[i])).tolist())
        eligible[i * S:(i + 1) * S] = ~np.isin(cand_ids, list(out))
    items = np.empty((N * S, steps), dtype=cand_ids.dtype)
    scores = np.empty((N * S, steps), dtype=np.float32)
    for s in range(steps):
        for q in range(N * S):
            p = choose(Z[q], noise(seed, q, first_step + s, cand_idx), inv_t, eligible[q], top_k)
            items[q, s], scores[q, s] = cand_ids[p], Z[q, p]
            if no_repeat:
                eligible[q] &= cand_ids != cand_ids[p]
        if s < steps - 1:
            Z, H = g.score_candidates_sessions([[x] for x in items[:, s]], np.tile(cand_ids, (N * S, 1)), hidden=H, return_hidden=True)
            Z = np.asarray(Z, dtype=np.float32)
    return items.reshape(N, S, steps), scores.reshape(N, S, steps), [h.reshape(N, S, -1) for h in H]

"""GRU4Rec.diversify_sessions / diversify_lists (k_mmr_rerank) against the host loop they replace, bit for bit, and against fp64.

The host loop: the pool is recommend_sessions(k=P), the pair matrix comes from similar_items over the pool's items, and the greedy
selection runs in np.float32 in the order include/gru4rec_hip.h defines (NumPy rounds every elementwise float32 operation once and
fuses nothing): r = s or (s - lo) / (hi - lo); pick 0 by lam * r; pick t by (lam * r) - (mu * m), m the running maximum of the
similarities to the picks; the largest value wins, the lower position first.

The fp64 check (test_picks_against_fp64) takes the device's own picks as the prefix and recomputes every value in float64 from the
downloaded table, with lam the float32 the device got and mu the float32 1 - lam (both exact parameters of the definition).  With
u = 2^-24 the device's value of position j is within
    b(j) = 4 u lam |r_j| + mu (b_sim(j) + u |m_j|) + u |v_j|
of the float64 one: three roundings in the normalisation and one in lam * r; the similarity's own bound b_sim (tests/
test_gpu_similar_items.py: (2 D + 16) u S for cosine, (D + 2) u S for dot, of the similarity that produced m_j, the largest in float64
over the picks so far) and one rounding in mu * m; one rounding in the subtraction.
The device picked p because its value was the largest, so v64(p) + b(p) >= v32(p) >= v32(j) >= v64(j) - b(j) for every remaining j:
v64(p) >= max_j v64(j) - b(p) - max_j b(j).  Derived, not tuned; every pick of every row is checked."""
import numpy as np
import pandas as pd
import pytest

from gru4rec_amd import _native
from gru4rec_amd.gru4rec import GRU4Rec

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
_MODELS = {}
# (items, top layer, input): the last one's table row is wider than the kernel's k-chunk of 128 floats
TABLES = {'50x4': (50, 4, 'constrained'), '300x36': (300, 36, 'separate'), '3000x100': (3000, 100, 'onehot'), '300x160': (300, 160, 'constrained')}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def train_some(g, steps):
    assert g.run_epoch(0, max_steps=steps) is not None
    g._download_weights()


def fitted(name, steps=30):
    """A GRU4Rec trained for `steps` mini-batches on synthetic sessions that hold every one of the table's items (ids 10, 13, 16, ...)."""
    if name not in _MODELS:
        n_items, D, mode = TABLES[name]
        rng = np.random.RandomState(D + n_items)
        n_ev = max(2 * n_items, 400)
        items = 10 + 3 * np.concatenate([rng.permutation(n_items), rng.randint(0, n_items, size=n_ev - n_items)])
        sess = np.repeat(np.arange(n_ev // 5), 5)
        data = pd.DataFrame({'SessionId': sess, 'ItemId': items[:len(sess)], 'Time': np.arange(len(sess), dtype=np.int64)})
        g = GRU4Rec(layers=[D], final_act='linear', loss='bpr-max', n_epochs=1, batch_size=32, n_sample=64, learning_rate=0.1,
                    constrained_embedding=mode == 'constrained', embedding=64 if mode == 'separate' else 0)
        g.prepare(data, sample_store=64 * 256)
        assert g.n_items == n_items
        w0 = g.Wy.copy()
        train_some(g, steps)
        assert (g.Wy != w0).any()
        _MODELS[name] = g
    return _MODELS[name]


def table_of(g, space):
    return g.E if (space == 'input' and g.embedding and not g.constrained_embedding) else g.Wy


def histories(g, n, seed):
    ids = g.itemidmap.index.values
    rng = np.random.RandomState(seed)
    return [ids[rng.randint(0, len(ids), size=rng.randint(1, 7))] for _ in range(n)]


def pair_matrix(g, row_items, metric, space):
    """sim[i, j] of a pool: query = the item at position i, candidate = the item at position j, from similar_items.  A pool of distinct
    items: similar_items(pool, k = P - 1, predict_for_item_ids = pool), scattered (the diagonal, never read, stays NaN).  Otherwise
    over the distinct items with exclude_self=False, expanded -- the same bits by similar_items' contract."""
    P = len(row_items)
    uniq, inv = np.unique(row_items, return_inverse=True)
    S = np.full((len(uniq), len(uniq)), np.nan, dtype=np.float32)
    if len(uniq) == P and P > 1:
        it, sc = g.similar_items(uniq, k=P - 1, metric=metric, space=space, predict_for_item_ids=uniq)
    elif len(uniq) < P:
        it, sc = g.similar_items(uniq, k=len(uniq), metric=metric, space=space, predict_for_item_ids=uniq, exclude_self=False)
    else:
        return S
    S[np.arange(len(uniq))[:, None], np.searchsorted(uniq, it)] = sc
    return S[inv][:, inv]


def greedy(s, S, k, trade_off, normalize):
    """The selection of include/gru4rec_hip.h in np.float32: (positions, values)."""
    s = np.asarray(s, dtype=np.float32)
    lam = np.float32(trade_off)
    mu = np.float32(1.0) - lam
    r = s
    if normalize:
        lo, hi = s.min(), s.max()
        r = (s - lo) / (hi - lo) if hi > lo else np.zeros_like(s)
    lr = lam * r
    assert lr.dtype == np.float32 and mu.dtype == np.float32
    free = np.ones(len(s), dtype=bool)
    pos, val, m = [], [], None
    for t in range(k):
        if t == 0:
            v = lr
        else:
            sim = S[pos[-1]]
            m = sim if t == 1 else np.where(sim > m, sim, m)
            v = lr - mu * m
        assert v.dtype == np.float32 and not np.isnan(v[free]).any()
        j = int(np.argmax(np.where(free, v, -np.inf)))      # the first of the largest: the lower position
        pos.append(j)
        val.append(v[j])
        free[j] = False
    return np.array(pos, dtype=np.int32), np.array(val, dtype=np.float32)


def host_loop(g, pool_items, pool_scores, k, trade_off, metric, space, normalize):
    out = [greedy(pool_scores[i], pair_matrix(g, pool_items[i], metric, space), k, trade_off, normalize) for i in range(len(pool_items))]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def check_parity(g, hist, P, k, trade_off, metric, space, normalize, tag, **kw):
    pool_items, pool_scores, H0 = g.recommend_sessions(hist, k=P, return_hidden=True, **kw)
    items, scores, H, pos, values = g.diversify_sessions(hist, k=k, pool=P, trade_off=trade_off, metric=metric, space=space, normalize=normalize,
                                                         return_hidden=True, return_details=True, **kw)
    assert items.shape == scores.shape == pos.shape == values.shape == (len(hist), k)
    assert pos.dtype == np.int32 and values.dtype == np.float32 and scores.dtype == np.float32
    want_pos, want_val = host_loop(g, pool_items, pool_scores, k, trade_off, metric, space, normalize)
    rows = np.arange(len(hist))[:, None]
    bad = np.flatnonzero((pos != want_pos).any(1))
    assert len(bad) == 0, '%s: row %d picks %s, the host loop %s' % (tag, bad[0], pos[bad[0]], want_pos[bad[0]])
    np.testing.assert_array_equal(bits(values), bits(want_val), err_msg=tag)
    np.testing.assert_array_equal(items, pool_items[rows, pos], err_msg=tag)
    np.testing.assert_array_equal(bits(scores), bits(pool_scores[rows, pos]), err_msg=tag)
    for a, b in zip(H, H0):
        np.testing.assert_array_equal(bits(a), bits(b), err_msg=tag)
    # the re-ranker alone, on the same pools and scores
    p2, v2 = g.diversify_lists(pool_items, pool_scores, k, trade_off=trade_off, metric=metric, space=space, normalize=normalize)
    np.testing.assert_array_equal(p2, pos, err_msg=tag)
    np.testing.assert_array_equal(bits(v2), bits(values), err_msg=tag)
    # without the extras: the same first two
    i3, s3 = g.diversify_sessions(hist, k=k, pool=P, trade_off=trade_off, metric=metric, space=space, normalize=normalize, **kw)
    np.testing.assert_array_equal(i3, items)
    np.testing.assert_array_equal(bits(s3), bits(scores))
    return items, scores, pos, values


KS = {'k1-2': (1, 2), 'k10-P': (10, 'P')}
POOLS = (1, 2, 16, 37, 128)


def ks_of(ks, P):
    return sorted({min(P, P if k == 'P' else k) for k in KS[ks]})


# ---- 1. bit parity with the host loop -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ks', sorted(KS))
@pytest.mark.parametrize('name', sorted(TABLES))
def test_parity_with_the_host_loop(name, ks):
    g = fitted(name)
    n_items = TABLES[name][0]
    spaces = ['output'] if TABLES[name][2] == 'onehot' else ['output', 'input']
    rng = np.random.RandomState(5)
    n_cfg = 0
    for P in POOLS:
        if P > n_items:
            continue
        for k in ks_of(ks, P):
            # every (trade_off, metric, normalize, space) over the pools and ks, N = 1 and 3 in turn
            for trade_off in (0, 0.3, 0.7, 1):
                metric, normalize, space = ('cosine', 'dot')[n_cfg % 2], bool((n_cfg // 2) % 2), spaces[(n_cfg // 4) % len(spaces)]
                N = (1, 3)[(n_cfg // 3) % 2]
                check_parity(g, histories(g, N, seed=int(rng.randint(1 << 30))), P, k, trade_off, metric, space, normalize,
                             '%s P=%d k=%d t=%g %s %s norm=%d N=%d' % (name, P, k, trade_off, metric, space, normalize, N))
                n_cfg += 1
    assert n_cfg >= 16


@pytest.mark.parametrize('ks', sorted(KS))
def test_parity_across_chunks_filters_and_scan(ks):
    """N = 600 crosses G4R_REPLAY_CHUNK = 512; exclusions, a candidate list, the bf16 scan and a hidden state handed back."""
    g = fitted('3000x100')
    ids = g.itemidmap.index.values
    P = 37
    k = ks_of(ks, P)[-1] if ks == 'k1-2' else 10
    hist = histories(g, 600, seed=11)
    check_parity(g, hist, P, k, 0.7, 'cosine', 'output', True, 'N=600')
    hist = histories(g, 40, seed=12)
    rng = np.random.RandomState(13)
    per_row = [ids[rng.randint(0, len(ids), size=rng.randint(0, 30))] for _ in hist]
    check_parity(g, hist, P, k, 0.3, 'dot', 'output', False, 'filters', exclude_history=True, exclude=ids[:200], exclude_per_row=per_row)
    sub = ids[rng.permutation(len(ids))[:500]]      # (distinct: the host loop's pair matrix wants a pool of distinct items)
    _, _, pos, _ = check_parity(g, hist, P, k, 0.3, 'cosine', 'output', True, 'candidates', predict_for_item_ids=sub, exclude_history=True)
    check_parity(g, hist, 128, k, 0.7, 'cosine', 'output', True, 'bf16', scan='bf16', oversample=8)
    check_parity(g, hist, 16, min(k, 16), 0.7, 'dot', 'output', True, 'bf16 list', scan='bf16', oversample=2, predict_for_item_ids=sub)
    # diversify(a + b) == diversify(b, hidden = the state after a)
    a, b = histories(g, 40, seed=14), histories(g, 40, seed=15)
    kw = dict(k=k, pool=P, trade_off=0.5, return_hidden=True, return_details=True)
    whole = g.diversify_sessions([np.concatenate(x) for x in zip(a, b)], **kw)
    Ha = g.diversify_sessions(a, **kw)[2]
    rest = g.diversify_sessions(b, hidden=Ha, **kw)
    for x, y in zip(whole[:2] + whole[3:], rest[:2] + rest[3:]):
        np.testing.assert_array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)
    for x, y in zip(whole[2], rest[2]):
        np.testing.assert_array_equal(bits(x), bits(y))


# ---- 2. trade_off = 1 is recommend_sessions -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(TABLES))
def test_trade_off_one_is_recommend_sessions(name):
    g = fitted(name)
    n_items = TABLES[name][0]
    hist = histories(g, 3, seed=21)
    for P in POOLS:
        if P > n_items:
            continue
        for k in sorted({1, min(2, P), min(10, P), P}):
            for normalize in (False, True):
                for metric in ('cosine', 'dot'):
                    items, scores, pos, values = g.diversify_sessions(hist, k=k, pool=P, trade_off=1, metric=metric, normalize=normalize, return_details=True)
                    want_i, want_s = g.recommend_sessions(hist, k=k)
                    np.testing.assert_array_equal(items, want_i)
                    np.testing.assert_array_equal(bits(scores), bits(want_s))
                    np.testing.assert_array_equal(pos, np.tile(np.arange(k, dtype=np.int32), (3, 1)))
                    if not normalize:      # 1 * s - 0 * m
                        np.testing.assert_array_equal(values, want_s)


# ---- 3. every pick against fp64 -------------------------------------------------------------------------------------------------------
def sims64(T, idx, metric):
    """fp64 pair scores of the items idx among themselves and the bound of tests/test_gpu_similar_items.py's module docstring."""
    X = T[idx].astype(np.float64)
    D = T.shape[1]
    ref, S = X @ X.T, np.abs(X) @ np.abs(X).T
    if metric == 'dot':
        return ref, (D + 2) * U * S
    nrm = np.sqrt((X * X).sum(1))
    den = nrm[:, None] * nrm[None, :]
    with np.errstate(divide='ignore', invalid='ignore'):
        ref, S = np.where(den > 0, ref / den, 0.0), np.where(den > 0, S / den, 0.0)
    return ref, (2 * D + 16) * U * S


def check_picks_fp64(g, T, pool_items, pool_scores, pos, trade_off, metric, normalize, tag):
    lam32 = np.float32(trade_off)
    lam, mu = float(lam32), float(np.float32(1.0) - lam32)
    worst = 0.0
    for i in range(len(pool_items)):
        idx = g.itemidmap[pool_items[i]].values
        sim, bsim = sims64(T, idx, metric)
        s = pool_scores[i].astype(np.float64)
        r = s
        if normalize:
            r = (s - s.min()) / (s.max() - s.min()) if s.max() > s.min() else np.zeros_like(s)
        free = np.ones(len(s), dtype=bool)
        for t, p in enumerate(pos[i]):
            assert free[p], '%s row %d: position %d picked twice' % (tag, i, p)
            if t == 0:
                m, bs = np.zeros_like(s), np.zeros_like(s)
            else:
                prev = pos[i][:t]
                which = sim[prev].argmax(0)      # the pick whose similarity is m_j
                m, bs = sim[prev][which, np.arange(len(s))], bsim[prev][which, np.arange(len(s))]
            v = lam * r - (mu * m if t else 0.0)
            b = 4 * U * lam * np.abs(r) + (mu * (bs + U * np.abs(m)) + U * np.abs(v) if t else 0.0)
            best, slack = v[free].max(), b[p] + b[free].max()
            assert v[p] >= best - slack, '%s row %d pick %d: position %d has fp64 value %.9g, the best remaining %.9g, bound %.3g' % (
                tag, i, t, p, v[p], best, slack)
            if best > v[p]:
                worst = max(worst, (best - v[p]) / slack)
            free[p] = False
    return worst


@pytest.mark.parametrize('ks', sorted(KS))
@pytest.mark.parametrize('name', sorted(TABLES))
def test_picks_against_fp64(name, ks):
    g = fitted(name)
    n_items = TABLES[name][0]
    spaces = ['output'] if TABLES[name][2] == 'onehot' else ['output', 'input']
    hist = histories(g, 3, seed=31)
    worst = 0.0
    for P in POOLS:
        if P > n_items:
            continue
        pool_items, pool_scores = g.recommend_sessions(hist, k=P)
        for k in ks_of(ks, P):
            for trade_off in (0, 0.3, 0.7, 1):
                for metric in ('cosine', 'dot'):
                    for normalize in (False, True):
                        for space in spaces:
                            _, _, pos, _ = g.diversify_sessions(hist, k=k, pool=P, trade_off=trade_off, metric=metric, space=space,
                                                                normalize=normalize, return_details=True)
                            worst = max(worst, check_picks_fp64(g, table_of(g, space), pool_items, pool_scores, pos, trade_off, metric, normalize,
                                                                '%s P=%d k=%d t=%g %s %s norm=%d' % (name, P, k, trade_off, metric, space, normalize)))
    print('%s %s: the closest call used %.3f of its bound' % (name, ks, worst))


# ---- 4. supplied lists ----------------------------------------------------------------------------------------------------------------
def test_supplied_lists_ties_zero_rows_and_duplicates():
    g = fitted('300x36')
    keep = g.Wy.copy()
    Wy = keep.copy()
    dup = [5, 100, 101, 299]
    Wy[dup[1:]] = Wy[dup[0]]
    Wy[[7, 200]] = 0.0
    g.Wy = Wy
    g._dev_put(g._ensure_model(), 'Wy', g.Wy)
    try:
        ids = g.itemidmap.index.values
        rng = np.random.RandomState(41)
        other = np.array([i for i in range(300) if i not in dup + [7, 200]])

        def run(idx, rel, k, trade_off, metric, normalize):
            idx, rel = np.atleast_2d(idx), np.atleast_2d(np.asarray(rel, dtype=np.float32))
            pos, val = g.diversify_lists(ids[idx], rel, k, trade_off=trade_off, metric=metric, normalize=normalize)
            want = host_loop(g, ids[idx], rel, k, trade_off, metric, 'output', normalize)
            np.testing.assert_array_equal(pos, want[0])
            np.testing.assert_array_equal(bits(val), bits(want[1]))
            return pos, val
        for metric in ('cosine', 'dot'):
            # duplicated table rows with equal relevance: equal values at every pick, the lower position wins
            idx = np.concatenate([[101, 299, 5, 100], other[:8]])
            rel = np.concatenate([[2.0, 2.0, 2.0, 2.0], np.linspace(1.5, 0.5, 8)])
            pos, val = run(idx, rel, 12, 0.7, metric, False)
            assert pos[0, 0] == 0
            order = [int(np.flatnonzero(pos[0] == j)[0]) for j in range(4)]
            assert order == sorted(order), 'equal (relevance, similarity): the lower position first, got ranks %s' % order
            # the same item listed several times
            idx = np.array([other[3], 5, other[3], 5, other[4], other[3]])
            pos, val = run(idx, [1.0, 1.0, 1.0, 0.5, 0.25, 1.0], 6, 0.5, metric, True)
            assert sorted(pos[0].tolist()) == list(range(6))                   # P == k: a permutation
            assert pos[0, 0] == 0
            # zero rows: similarity 0 to everything, so with equal relevance they follow the first pick in position order
            idx = np.concatenate([other[10:13], [7, 200], other[13:16]])
            pos, val = run(idx, np.ones(8), 8, 0.0, metric, False)
            assert pos[0, 0] == 0
            if metric == 'cosine':      # (under dot a negative product beats 0)
                sim = pair_matrix(g, ids[idx], metric, 'output')
                assert (np.nan_to_num(sim[3]) == 0).all() and (np.nan_to_num(sim[:, 4]) == 0).all()
            # hi == lo: r = 0 whatever the relevance, values = -(mu * m)
            pos, val = run(other[20:57], np.full(37, 3.25), 37, 0.3, metric, True)
            assert val[0, 0] == 0 and sorted(pos[0].tolist()) == list(range(37))
            pos0, val0 = run(other[20:57], np.full(37, -7.5), 37, 0.3, metric, True)
            np.testing.assert_array_equal(pos0, pos)
            np.testing.assert_array_equal(bits(val0), bits(val))
            # many rows at once, P = 128 with duplicates, every k
            idx = rng.randint(0, 300, size=(5, 128))
            rel = rng.randn(5, 128).astype(np.float32)
            rel[:, 5] = rel[:, 90]
            for k in (1, 2, 10, 128):
                pos, val = run(idx, rel, k, 0.7, metric, True)
            assert (np.sort(pos, axis=1) == np.arange(128)).all()
        # one position: itself
        pos, val = run(np.array([[5], [7]]), [[4.0], [-1.0]], 1, 0.3, 'cosine', False)
        assert (pos == 0).all() and val[0, 0] == np.float32(0.3) * np.float32(4.0)
        # the C entry refuses what the Python front end cannot send
        m = g._ensure_model()
        one = np.zeros((1, 4), dtype=np.int32)
        for bad, msg in ((dict(items=np.full((1, 4), 300, dtype=np.int32)), 'item index out of range'), (dict(k=5), 'k must be'), (dict(lam=1.5), 'lam must be'),
                         (dict(lam=float('nan')), 'lam must be'), (dict(rel=np.full((1, 4), np.inf, dtype=np.float32)), 'not finite'),
                         (dict(items=np.zeros((1, 129), dtype=np.int32), rel=np.zeros((1, 129), dtype=np.float32)), 'G4R_DIVERSIFY_POOL_MAX')):
            kw = dict(dict(items=one, rel=np.zeros((1, 4), dtype=np.float32), k=2, lam=0.5), **bad)
            with pytest.raises(_native.NativeError, match=msg):
                m.diversify_lists(**kw)
    finally:
        g.Wy = keep
        g._dev_put(g._ensure_model(), 'Wy', g.Wy)


def test_c_entry_refuses_before_any_launch():
    g = fitted('3000x100')      # one-hot: no input space
    m = g._ensure_model()
    m.set_param('By', g.By.reshape(-1))      # (any upload invalidates the norms: a launch of the cosine path would rebuild them)
    before = m.sim_norms()
    assert not before[1]
    offs, hi = np.array([0, 2], dtype=np.int64), np.array([1, 2], dtype=np.int32)
    for bad, msg in ((dict(pool=129), 'G4R_DIVERSIFY_POOL_MAX'), (dict(k=11), 'k must be'), (dict(k=0), 'k must be'), (dict(lam=-0.5), 'lam must be'),
                     (dict(space='input'), 'one-hot'), (dict(pool=100, oversample=11), 'oversample'),
                     (dict(item_idx=np.arange(5, dtype=np.int32)), 'k exceeds the number of candidates'),
                     (dict(excl_mask=np.full((3000 + 31) // 32, 0xFFFFFFFF, dtype=np.uint32)), 'eligible')):
        kw = dict(dict(hist_offs=offs, hist_items=hi, k=3, pool=10, lam=0.5), **bad)
        with pytest.raises(_native.NativeError, match=msg):
            m.diversify_sessions(**kw)
    assert m.sim_norms() == before
    m.diversify_sessions(offs, hi, k=3, pool=10, lam=0.5)
    assert m.sim_norms() == (before[0], True, before[2] + 1)


# ---- 5. the norm cache follows the weights --------------------------------------------------------------------------------------------
def test_results_follow_the_weights():
    g = fitted('300x36')
    m = g._ensure_model()
    hist = histories(g, 3, seed=51)
    first = check_parity(g, hist, 37, 10, 0.3, 'cosine', 'input', True, 'before')
    builds = m.sim_norms()[2]
    check_parity(g, hist, 37, 10, 0.3, 'cosine', 'input', True, 'again')
    assert m.sim_norms()[1:] == (True, builds)       # nothing changed: nothing rebuilt
    old_E = g.E.copy()
    train_some(g, 20)                                # further steps of fit
    assert not m.sim_norms()[1] and not np.array_equal(old_E, g.E)
    later = check_parity(g, hist, 37, 10, 0.3, 'cosine', 'input', True, 'after fit')
    assert m.sim_norms()[1:] == (True, builds + 1)
    assert not np.array_equal(bits(first[3]), bits(later[3]))
    pool_items, pool_scores = g.recommend_sessions(hist, k=37)
    check_picks_fp64(g, g.E, pool_items, pool_scores, later[2], 0.3, 'cosine', True, 'after fit')


# ---- 6. state -------------------------------------------------------------------------------------------------------------------------
def test_the_prediction_state_and_the_other_entries_are_untouched():
    g = fitted('3000x100')
    ids = g.itemidmap.index.values
    rng = np.random.RandomState(61)
    seq = [(rng.randint(0, 3, size=40), ids[rng.randint(0, len(ids), size=40)]) for _ in range(6)]
    hist = histories(g, 20, seed=62)
    out = []
    for interleave in (False, True):
        g.predict = None
        got = []
        for t, (sid, inp) in enumerate(seq):
            if interleave:
                g.diversify_sessions(histories(g, 30, seed=t), k=10, pool=64, metric='cosine' if t % 2 else 'dot')
                g.diversify_lists(ids[rng.randint(0, len(ids), size=(7, 50))], rng.randn(7, 50), 5)
            if t % 2:
                got.append(g.predict_next_batch(sid, inp, batch=40).values)
            else:
                got.extend(g.recommend_next_batch(sid, inp, k=20, batch=40))
            if t == 3:
                got.extend(g.recommend_sessions(hist, k=50))
                got.extend(g.continue_sessions(hist, steps=3, k=5))
        out.append(got)
    for a, b in zip(*out):
        if a.dtype == np.float32:
            np.testing.assert_array_equal(bits(a), bits(b))
        else:
            np.testing.assert_array_equal(a, b)

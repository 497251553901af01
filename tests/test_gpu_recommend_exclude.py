"""GRU4Rec.recommend_next_batch(exclude_seen=, exclude=, exclude_per_row=) / g4r_recommend_step_filtered against the same-call
predict_next_batch scores with the ineligible positions dropped, in the contract's NumPy order (per row: np.lexsort((np.arange(n),
-S[:, r])) restricted to the eligible positions, first k): items exactly, scores bit for bit."""

import numpy as np
import pandas as pd
import pytest

from gru4rec_amd import _native
from gru4rec_amd.gru4rec import GRU4Rec

pytestmark = pytest.mark.gpu

N_ITEMS = 20000      # > 256 compute units x 32 columns: the column ranges hold several tiles each
XMAX = _native.G4R_EXCLUDE_MAX


def topk_oracle(S, k, eligible=None):
    """S: [rows, n_sel], eligible: bool [rows, n_sel] or None -> (columns, scores) of the k best eligible positions per row."""
    n = S.shape[1]
    out = []
    for r in range(S.shape[0]):
        order = np.lexsort((np.arange(n), -S[r]))
        if eligible is not None:
            order = order[eligible[r][order]]
        assert len(order) >= k
        out.append(order[:k])
    cols = np.stack(out)
    return cols, np.take_along_axis(S, cols, 1)


def assert_same(items, scores, want_items, want_scores):
    np.testing.assert_array_equal(items, want_items)
    assert scores.dtype == np.float32
    np.testing.assert_array_equal(scores.view(np.uint32), np.ascontiguousarray(want_scores, dtype=np.float32).view(np.uint32))


_MODELS = {}


def fitted(final_act, D):
    """A GRU4Rec fitted for one epoch on synthetic sessions that hold every one of N_ITEMS items (ids 10, 13, 16, ...)."""
    key = (final_act, D)
    if key not in _MODELS:
        rng = np.random.RandomState(D + 1)
        items = 10 + 3 * np.concatenate([rng.permutation(N_ITEMS), rng.randint(0, N_ITEMS, size=N_ITEMS)])
        sess = np.repeat(np.arange(len(items) // 5), 5)
        data = pd.DataFrame({'SessionId': sess, 'ItemId': items[:len(sess)], 'Time': np.arange(len(sess), dtype=np.int64)})
        sm = final_act.startswith('softmax')
        g = GRU4Rec(layers=[D], final_act=final_act, loss='cross-entropy' if sm else 'bpr-max', n_epochs=1, batch_size=64,
                    n_sample=0 if sm else 128, learning_rate=0.05)
        g.fit(data, sample_store=0 if sm else 100000)
        assert g.n_items == N_ITEMS
        _MODELS[key] = g
    return _MODELS[key]


def eligible_of(C, rows, exclude=None, exclude_per_row=None):
    """bool [rows, len(C)]: the candidate ids C that no exclusion names."""
    E = np.ones((rows, len(C)), dtype=bool)
    if exclude is not None and len(exclude):
        E &= ~np.isin(C, exclude)[None, :]
    if exclude_per_row is not None:
        for r in range(rows):
            if len(exclude_per_row[r]):
                E[r] &= ~np.isin(C, np.asarray(exclude_per_row[r]))
    return E


def compare_call(g, rows, k, cand, excl, pre_steps=1, seed=0):
    """The same call sequence twice from a fresh prediction state: `pre_steps` predict_next_batch calls, then predict_next_batch
    (the oracle) / recommend_next_batch with the exclusions excl(S, C) -> dict(exclude=, exclude_per_row=) (under test)."""
    rng = np.random.RandomState(seed)
    ids = g.itemidmap.index.values
    seq = [(rng.randint(0, 3, size=rows), ids[rng.randint(0, len(ids), size=rows)]) for _ in range(pre_steps + 1)]
    C = ids if cand is None else np.asarray(cand)
    g.predict = None
    for sid, inp in seq[:-1]:
        g.predict_next_batch(sid, inp, predict_for_item_ids=cand, batch=rows)
    S = g.predict_next_batch(seq[-1][0], seq[-1][1], predict_for_item_ids=cand, batch=rows).values.T.astype(np.float32)
    kw = excl(S, C)
    g.predict = None
    for sid, inp in seq[:-1]:
        g.predict_next_batch(sid, inp, predict_for_item_ids=cand, batch=rows)
    items, scores = g.recommend_next_batch(seq[-1][0], seq[-1][1], k=k, predict_for_item_ids=cand, batch=rows, **kw)
    E = eligible_of(C, rows, **kw)
    cols, want = topk_oracle(S, k, E)
    assert items.shape == scores.shape == (rows, k)
    assert_same(items, scores, C[cols], want)
    return S, E, items


def random_excl(n_row=50, frac=0.01, seed=0):
    def f(S, C):
        rng = np.random.RandomState(seed)
        u = np.unique(C)
        return dict(exclude=rng.choice(u, size=max(1, int(frac * len(u))), replace=False),
                    exclude_per_row=[rng.choice(u, size=min(n_row, len(u) // 4), replace=False) for _ in range(S.shape[0])])
    return f


def own_top_k(k):
    """Row r excludes the items of its own unfiltered top k: it has to return ranks k+1 .. 2k (by item)."""
    def f(S, C):
        cols, _ = topk_oracle(S, k)
        return dict(exclude_per_row=[C[c] for c in cols])
    return f


def subset_with_duplicates(g, n, seed=1):
    rng = np.random.RandomState(seed)
    ids = g.itemidmap.index.values
    c = ids[rng.randint(0, len(ids), size=n)]
    c[5:12] = c[0]            # duplicates: equal scores at different positions
    c[20:24] = c[1]
    return c


@pytest.mark.parametrize('final_act', ['linear', 'elu-0.5', 'relu', 'tanh', 'softmax'])
@pytest.mark.parametrize('D', [64, 100])
def test_exclusions_match_the_oracle(final_act, D):
    g = fitted(final_act, D)
    sub = subset_with_duplicates(g, 400)
    for rows in (1, 5, 130):
        for k in (1, 20, 256):
            compare_call(g, rows, k, None, random_excl(seed=rows + k), seed=rows + k)
        # the duplicated items of the subset are excluded in some rows (every one of their positions goes) and not in others
        dup = lambda S, C: dict(exclude_per_row=[[C[0], C[1]] if r % 2 == 0 else [C[30]] for r in range(S.shape[0])], exclude=[C[40]])
        _, E, items = compare_call(g, rows, 20, sub, dup, seed=rows)
        assert not np.isin(items[0], [sub[0], sub[1]]).any() and E[0, 5:12].sum() == 0
        compare_call(g, rows, 256, sub, random_excl(n_row=30, frac=0.05, seed=rows), seed=rows + 1)


@pytest.mark.parametrize('final_act', ['linear', 'softmax', 'relu'])
def test_excluding_the_own_top_k_gives_the_next_k(final_act):
    g = fitted(final_act, 64)
    for rows, k in ((1, 256), (5, 20), (130, 256), (130, 1)):
        S, E, items = compare_call(g, rows, k, None, own_top_k(k), seed=k + rows)
        cols2, _ = topk_oracle(S, 2 * k)
        np.testing.assert_array_equal(items, g.itemidmap.index.values[cols2[:, k:]])
    sub = subset_with_duplicates(g, 600)
    compare_call(g, 130, 200, sub, own_top_k(200), seed=3)


# ---- adversarial orders on weights set directly (no training)
def _with_weights(final_act, Wy=None, By=None):
    g = fitted(final_act, 64)
    if Wy is not None:
        g.Wy = np.ascontiguousarray(Wy, dtype=np.float32)
    if By is not None:
        g.By = np.ascontiguousarray(By, dtype=np.float32).reshape(-1, 1)
    g.close()
    return g


@pytest.mark.parametrize('final_act', ['linear', 'softmax'])
def test_excluded_nan_rows(final_act):
    Wy = (np.random.RandomState(9).randn(N_ITEMS, 64) * 0.1).astype(np.float32)
    nan_items = [0, 3, 777, N_ITEMS - 1]
    if final_act == 'linear':
        Wy[nan_items] = np.nan
    else:
        Wy[nan_items[0]] = np.nan      # softmax: one NaN poisons the whole row (every score NaN): the order is the column order
    g = _with_weights(final_act, Wy=Wy)
    try:
        ids = g.itemidmap.index.values
        cand = np.concatenate([ids[nan_items], ids[10:200], ids[nan_items[:2]]])
        some_nan = lambda S, C: dict(exclude=ids[nan_items[:1]], exclude_per_row=[ids[nan_items[1 + r % 3:]] for r in range(S.shape[0])])
        for rows in (1, 130):
            S, _, _ = compare_call(g, rows, len(cand) - 6, cand, some_nan, seed=rows)
            assert np.isnan(S).any()
            compare_call(g, rows, 256, None, some_nan, seed=rows + 1)
            compare_call(g, rows, 20, cand, some_nan, seed=rows + 2)
    finally:
        _MODELS.pop((final_act, 64), None)


@pytest.mark.parametrize('final_act', ['linear', 'softmax'])
def test_global_mask_leaving_exactly_k(final_act):
    g = fitted(final_act, 64)
    ids = g.itemidmap.index.values
    rng = np.random.RandomState(4)
    for rows, k in ((5, 256), (130, 20), (1, 1)):
        keep = rng.choice(N_ITEMS, size=k, replace=False)
        rest = np.setdiff1d(np.arange(N_ITEMS), keep)
        _, _, items = compare_call(g, rows, k, None, lambda S, C: dict(exclude=ids[rest]), seed=k)
        for r in range(rows):
            assert set(items[r]) == set(ids[keep])
    # with a row list on top, k left in every row: the global mask takes all but k + 3, each row drops 3 more
    keep = rng.choice(N_ITEMS, size=23, replace=False)
    rest = np.setdiff1d(np.arange(N_ITEMS), keep)
    compare_call(g, 7, 20, None, lambda S, C: dict(exclude=ids[rest], exclude_per_row=[ids[np.roll(keep, r)[:3]] for r in range(7)]))


@pytest.mark.parametrize('final_act', ['linear', 'softmax'])
def test_row_list_of_exactly_the_limit(final_act):
    g = fitted(final_act, 64)
    ids = g.itemidmap.index.values

    def f(S, C):
        cols, _ = topk_oracle(S, 256)
        out = []
        for r in range(S.shape[0]):       # the row's own top 256 plus random others: XMAX distinct items, some twice
            x = np.unique(np.concatenate([C[cols[r]], ids[np.random.RandomState(r).choice(N_ITEMS, size=3 * XMAX, replace=False)]]))
            x = np.setdiff1d(x, C[cols[r]])[:XMAX - 256]
            out.append(np.concatenate([C[cols[r]], x, x[:50]]))
            assert len(np.unique(out[-1])) == XMAX
        return dict(exclude_per_row=out)
    compare_call(g, 130, 256, None, f, seed=2)
    compare_call(g, 3, 20, None, f, seed=3)


@pytest.mark.parametrize('final_act', ['linear', 'relu'])
def test_all_scores_equal_gives_the_first_remaining_positions(final_act):
    g = _with_weights(final_act, Wy=np.zeros((N_ITEMS, 64)), By=np.full(N_ITEMS, -0.25 if final_act == 'relu' else 0.5))
    try:
        ids = g.itemidmap.index.values
        for rows, k in ((1, 1), (5, 20), (130, 256)):
            excl = lambda S, C: dict(exclude=ids[:7], exclude_per_row=[ids[np.arange(r, 300, 2)] for r in range(S.shape[0])])
            S, E, items = compare_call(g, rows, k, None, excl, seed=k)
            assert (S == S[0, 0]).all()
            for r in range(rows):
                np.testing.assert_array_equal(items[r], ids[np.flatnonzero(E[r])[:k]])
            sub = subset_with_duplicates(g, 300)
            compare_call(g, rows, min(k, 200), sub, lambda S, C: dict(exclude=[C[0]], exclude_per_row=[C[r:r + 3] for r in range(S.shape[0])]),
                         seed=k + 1)
    finally:
        _MODELS.pop((final_act, 64), None)


@pytest.mark.parametrize('final_act', ['elu-0.5', 'softmax'])
def test_exclude_seen_over_interleaved_calls(final_act):
    """A random sequence of predict_next_batch / recommend_next_batch(exclude_seen=True) calls with session changes and a batch change,
    against the same sequence made of predict_next_batch calls only, with the seen items tracked here."""
    g = fitted(final_act, 64)
    rng = np.random.RandomState(11)
    ids = g.itemidmap.index.values
    hot = ids[rng.choice(N_ITEMS, size=30, replace=False)]       # inputs drawn from few items: repeats and seen winners
    sub = subset_with_duplicates(g, 400, seed=5)
    calls, sessions = [], np.arange(40)
    for t in range(16):
        if t == 10:
            sessions = np.arange(48)      # a new batch size restarts the prediction state (and the seen-history)
        B = len(sessions)
        sessions = np.where(rng.rand(B) < 0.2, rng.randint(100, 10000, size=B), sessions)
        inp = np.where(rng.rand(B) < 0.7, hot[rng.randint(0, len(hot), size=B)], ids[rng.randint(0, N_ITEMS, size=B)])
        calls.append((sessions.copy(), inp, rng.rand() < 0.6, int(rng.choice([1, 20, 100])), sub if rng.rand() < 0.3 else None, B))
    got, want = [], []
    g.predict = None
    for sid, inp, rec, k, cand, batch in calls:
        if rec:
            got.append(g.recommend_next_batch(sid, inp, k=k, predict_for_item_ids=cand, batch=batch, exclude_seen=True))
        else:
            g.predict_next_batch(sid, inp, predict_for_item_ids=cand, batch=batch)
    g.predict = None
    seen, cur, cur_b = None, None, None
    for sid, inp, rec, k, cand, batch in calls:
        if batch != cur_b:
            seen, cur, cur_b = [set() for _ in range(batch)], np.full(batch, -1), batch
        for r in range(batch):
            if sid[r] != cur[r]:
                seen[r] = set()
            seen[r].add(inp[r])
        cur = sid.copy()
        S = g.predict_next_batch(sid, inp, predict_for_item_ids=cand, batch=batch).values.T.astype(np.float32)
        if rec:
            C = ids if cand is None else cand
            cols, sc = topk_oracle(S, k, eligible_of(C, batch, exclude_per_row=[sorted(x) for x in seen]))
            want.append((C[cols], sc))
    assert len(got) == len(want) > 4
    assert max(len(x) for x in seen) > 1
    for (gi, gs), (wi, ws) in zip(got, want):
        assert_same(gi, gs, wi, ws)


@pytest.mark.parametrize('final_act', ['linear', 'softmax'])
def test_filtered_entry_without_filters_is_the_unfiltered_one(final_act):
    g = fitted(final_act, 64)
    m = g._model if g._model is not None else g._ensure_model()
    rng = np.random.RandomState(1)
    for rows, k, cand in ((5, 20, None), (130, 256, None), (7, 50, rng.randint(0, N_ITEMS, size=300).astype(np.int32))):
        in_idx = rng.randint(0, N_ITEMS, size=rows).astype(np.int32)
        m.predict_begin(rows)
        a = m.recommend_step(in_idx, cand, k)
        m.predict_begin(rows)
        b = m.recommend_step_filtered(in_idx, cand, k, None, None, None)
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    g.predict = None


def test_c_abi_refuses_before_the_state_advances():
    g = fitted('linear', 64)
    m = g._model if g._model is not None else g._ensure_model()
    in_idx = np.array([1, 2, 3], dtype=np.int32)
    mask = np.zeros((N_ITEMS + 31) // 32, dtype=np.uint32)
    mask[:] = 0xFFFFFFFF
    m.predict_begin(3)
    ref = m.recommend_step(in_idx, None, 10)
    m.predict_begin(3)
    offs = np.array([0, 0, XMAX + 1, XMAX + 1], dtype=np.int64)
    with pytest.raises(_native.NativeError, match='row 1 .*G4R_EXCLUDE_MAX'):
        m.recommend_step_filtered(in_idx, None, 10, offs, np.arange(XMAX + 1, dtype=np.int32), None)
    with pytest.raises(_native.NativeError, match='row 0 has 0 eligible'):
        m.recommend_step_filtered(in_idx, None, 10, None, None, mask)
    with pytest.raises(_native.NativeError, match='out of range'):
        m.recommend_step_filtered(in_idx, None, 10, np.array([0, 1, 1, 1]), np.array([N_ITEMS], dtype=np.int32), None)
    with pytest.raises(_native.NativeError, match='monotone'):
        m.recommend_step_filtered(in_idx, None, 10, np.array([0, 2, 1, 2]), np.array([4, 5], dtype=np.int32), None)
    got = m.recommend_step(in_idx, None, 10)      # the refused calls left the hidden state where it was
    np.testing.assert_array_equal(got[0], ref[0])
    np.testing.assert_array_equal(got[1].view(np.uint32), ref[1].view(np.uint32))
    g.predict = None


# ---- large catalogue
def _mem_available_gb():
    try:
        for line in open('/proc/meminfo'):
            if line.startswith('MemAvailable:'):
                return int(line.split()[1]) / 1e6
    except OSError:
        pass
    return 0.0


def test_large_catalogue_10M_items():
    """10,000,000 x 256, 4 rows, k = 100 through the C ABI against predict_step at the same shape and hidden state.  Winners are
    planted through By at item 0, n_items - 1 and either side of the byte offsets 2^31 / 2^32 / 2^33 of Wy; the ones past 2^31
    are excluded -- by the global mask, by one row's list, by another row's list -- and must not come back."""
    I, D, B, k = 10_000_000, 256, 4, 100
    need = I * D * 4 / 1e9
    if _mem_available_gb() < need + 12:
        pytest.skip('needs ~%.0f GB of host memory for the item table' % (need + 12))
    rng = np.random.RandomState(5)
    Wy = np.tile((rng.randn(4093, D) * 0.05).astype(np.float32), (I // 4093 + 1, 1))[:I]
    By = np.zeros(I, dtype=np.float32)
    planted = [0, I - 1]
    for p in (31, 32, 33):
        r = (1 << p) // (D * 4)
        planted += [r - 1, r]
    By[planted] = np.float32(50.0) + np.arange(len(planted), dtype=np.float32)
    m = _native.Model(n_items=I, layers=[D], batch_size=B, n_sample=0, loss=_native.LOSS_IDS['bpr-max'], final_act=_native.ACT_IDS['linear'],
                      hidden_act=_native.ACT_IDS['tanh'], embed_mode=0, embedding=0, learning_rate=0.1, sample_store=0, seed=3,
                      device=0, rank=0, nranks=1, use_graph=0)
    try:
        m.set_param('Wy', Wy)
        del Wy
        m.set_param('By', By)
        m.set_param('Wx', (rng.randn(D, 3 * D) * 0.05).astype(np.float32))
        m.set_param('Wh', (rng.randn(D, D) * 0.05).astype(np.float32))
        m.set_param('Wrz', (rng.randn(D, 2 * D) * 0.05).astype(np.float32))
        m.set_param('Bh', (rng.randn(3 * D) * 0.1).astype(np.float32))
        in_idx = np.array(planted[:B], dtype=np.int32)
        far = planted[3:]                 # past 2^31 bytes of Wy
        masked = [far[0], I - 1]
        lists = [[far[1], far[2]], [far[3], far[2]] + list(rng.randint(0, I, size=XMAX - 2)), [], [far[4], 7, far[1]]]
        offs = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
        mask = np.zeros((I + 31) // 32, dtype=np.uint32)
        for i in masked:
            mask[i >> 5] |= np.uint32(1 << (i & 31))
        m.predict_begin(B)
        S = m.predict_step(in_idx)
        m.predict_begin(B)
        cols, scores = m.recommend_step_filtered(in_idx, None, k, offs, np.concatenate(lists).astype(np.int32), mask)
        E = np.ones(S.shape, dtype=bool)
        E[:, masked] = False
        for r in range(B):
            E[r, lists[r]] = False
        want_cols, want = topk_oracle(S, k, E)
        np.testing.assert_array_equal(cols, want_cols)
        np.testing.assert_array_equal(scores.view(np.uint32), want.view(np.uint32))
        for r in range(B):
            assert set(planted) - set(masked) - set(lists[r]) <= set(cols[r].tolist())
            assert not (set(masked) | set(lists[r])) & set(cols[r].tolist())
    finally:
        m.close()

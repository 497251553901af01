"""GRU4Rec.recommend_next_batch / g4r_recommend_step against the same-call predict_next_batch scores and the contract's NumPy order
(per row: np.lexsort((np.arange(n), -S[:, r]))[:k]): items exactly, scores bit for bit.  Ties are fed on purpose: whole rows of
equal scores (relu zeros, saturated tanh, all-zero item rows), scores that rise with the column (every new score beats the
threshold), NaN item rows, duplicated candidates."""

import numpy as np
import pandas as pd
import pytest

from gru4rec_amd import _native
from gru4rec_amd.gru4rec import GRU4Rec

pytestmark = pytest.mark.gpu

N_ITEMS = 20000      # > 256 compute units x 32 columns: the column ranges hold several tiles each


def topk_oracle(S, k):
    """S: [rows, n_sel] -> (columns, scores) of the k best per row in the contract's order."""
    n = S.shape[1]
    cols = np.stack([np.lexsort((np.arange(n), -S[r]))[:k] for r in range(S.shape[0])])
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
        rng = np.random.RandomState(D)
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


def compare_call(g, rows, k, cand, pre_steps=1, seed=0):
    """The same call sequence twice from a fresh prediction state: `pre_steps` predict_next_batch calls, then predict_next_batch
    (the oracle) / recommend_next_batch (under test)."""
    rng = np.random.RandomState(seed)
    ids = g.itemidmap.index.values
    seq = [(rng.randint(0, 3, size=rows), ids[rng.randint(0, len(ids), size=rows)]) for _ in range(pre_steps + 1)]
    out = []
    for mode in ('predict', 'recommend'):
        g.predict = None
        for sid, inp in seq[:-1]:
            g.predict_next_batch(sid, inp, predict_for_item_ids=cand, batch=rows)
        sid, inp = seq[-1]
        if mode == 'predict':
            out.append(g.predict_next_batch(sid, inp, predict_for_item_ids=cand, batch=rows).values.T.astype(np.float32))
        else:
            out.append(g.recommend_next_batch(sid, inp, k=k, predict_for_item_ids=cand, batch=rows))
    S, (items, scores) = out
    cols, want = topk_oracle(S, k)
    C = g.itemidmap.index.values if cand is None else np.asarray(cand)
    assert items.shape == scores.shape == (rows, k)
    assert_same(items, scores, C[cols], want)
    return S


def subset_with_duplicates(g, n, seed=1):
    rng = np.random.RandomState(seed)
    ids = g.itemidmap.index.values
    c = ids[rng.randint(0, len(ids), size=n)]
    c[5:12] = c[0]            # duplicates: equal scores at different columns
    return c


@pytest.mark.parametrize('final_act', ['linear', 'elu-0.5', 'relu', 'tanh', 'softmax'])
@pytest.mark.parametrize('D', [64, 100])
def test_top_k_matches_predict_next_batch(final_act, D):
    g = fitted(final_act, D)
    if final_act == 'tanh':       # scaled so that many scores saturate to +-1 exactly (ties across the whole row)
        g.Wy = g.Wy * 200.0
        g.close()
    sub = subset_with_duplicates(g, 200)
    for rows in (1, 5, 130):
        for k in (1, 20, 256):
            compare_call(g, rows, k, None, seed=rows + k)
        compare_call(g, rows, 20, sub, seed=rows)
        compare_call(g, rows, len(sub), sub, seed=rows + 1)      # k = n_sel
    if final_act == 'relu':
        # many exact 0 ties: the zeros inside the top 256 come in column order
        S = compare_call(g, 130, 256, None, seed=3)
        assert (S == 0).sum(axis=1).max() > 256


def test_interleaved_calls_keep_the_session_state():
    """One random sequence of predict_next_batch / recommend_next_batch calls with session changes and batch-size changes against the
    same sequence made of predict_next_batch calls only (top k taken on the host)."""
    g = fitted('elu-0.5', 64)
    rng = np.random.RandomState(11)
    ids = g.itemidmap.index.values
    sub = subset_with_duplicates(g, 300, seed=5)
    calls, sessions = [], np.arange(40)
    for t in range(14):
        if t == 9:
            sessions = np.arange(48)      # a new batch size restarts the prediction state
        B = len(sessions)
        sessions = np.where(rng.rand(B) < 0.3, rng.randint(100, 10000, size=B), sessions)      # some sessions change
        calls.append((sessions.copy(), ids[rng.randint(0, len(ids), size=B)], rng.rand() < 0.6, int(rng.choice([1, 20, 100])),
                      sub if rng.rand() < 0.3 else None, B))
    got, want = [], []
    g.predict = None
    for sid, inp, rec, k, cand, batch in calls:
        if rec:
            got.append(g.recommend_next_batch(sid, inp, k=k, predict_for_item_ids=cand, batch=batch))
        else:
            g.predict_next_batch(sid, inp, predict_for_item_ids=cand, batch=batch)
    g.predict = None
    for sid, inp, rec, k, cand, batch in calls:
        S = g.predict_next_batch(sid, inp, predict_for_item_ids=cand, batch=batch).values.T.astype(np.float32)
        if rec:
            cols, sc = topk_oracle(S, k)
            want.append(((ids if cand is None else cand)[cols], sc))
    assert len(got) == len(want) > 3
    for (gi, gs), (wi, ws) in zip(got, want):
        assert_same(gi, gs, wi, ws)


# ---- adversarial orders on weights set directly (no training)
def _with_weights(final_act, Wy=None, By=None):
    g = fitted(final_act, 64)
    if Wy is not None:
        g.Wy = np.ascontiguousarray(Wy, dtype=np.float32)
    if By is not None:
        g.By = np.ascontiguousarray(By, dtype=np.float32).reshape(-1, 1)
    g.close()
    return g


@pytest.mark.parametrize('final_act', ['linear', 'relu'])
def test_all_scores_equal_gives_the_first_columns(final_act):
    """All item rows zero and all biases equal: every score of a row is the same, the result is the first k columns."""
    g = _with_weights(final_act, Wy=np.zeros((N_ITEMS, 64)), By=np.full(N_ITEMS, -0.25 if final_act == 'relu' else 0.5))
    try:
        sub = subset_with_duplicates(g, 250)
        for rows, k in ((1, 1), (5, 20), (130, 256)):
            S = compare_call(g, rows, k, None, seed=k)
            assert (S == S[0, 0]).all()
            items, _ = g.recommend_next_batch(np.arange(rows), g.itemidmap.index.values[:rows], k=k, batch=rows)
            np.testing.assert_array_equal(items, np.broadcast_to(g.itemidmap.index.values[:k], (rows, k)))
            compare_call(g, rows, min(k, len(sub)), sub, seed=k + 1)
    finally:
        _MODELS.pop((final_act, 64), None)


def test_scores_rising_with_the_column():
    """By[i] strictly increasing, zero item rows: each new score beats the running threshold (every tile is a full queue)."""
    By = np.arange(N_ITEMS, dtype=np.float32) * np.float32(1e-3)
    g = _with_weights('linear', Wy=np.zeros((N_ITEMS, 64)), By=By)
    try:
        for rows, k in ((1, 256), (130, 256), (5, 20), (5, 1)):
            compare_call(g, rows, k, None, seed=k)
        cand = np.sort(subset_with_duplicates(g, 256))
        compare_call(g, 130, 256, cand, seed=2)
        # plus a real GRU term on top of the ramp
        g.Wy = (np.random.RandomState(4).randn(N_ITEMS, 64) * 1e-4).astype(np.float32)
        g.close()
        compare_call(g, 130, 256, None, seed=5)
    finally:
        _MODELS.pop(('linear', 64), None)


@pytest.mark.parametrize('final_act', ['linear', 'softmax'])
def test_nan_item_rows_rank_last(final_act):
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
        for rows in (1, 130):
            S = compare_call(g, rows, len(cand), cand, seed=rows)
            assert np.isnan(S).any()
            compare_call(g, rows, 256, None, seed=rows + 1)
            compare_call(g, rows, 20, cand, seed=rows + 2)
    finally:
        _MODELS.pop((final_act, 64), None)


def test_c_abi_refuses_bad_k():
    g = fitted('linear', 64)
    g.predict = None
    g.predict_next_batch(np.arange(3), g.itemidmap.index.values[:3], batch=3)
    m = g._model
    for k, msg in ((0, '256'), (257, '256'), (N_ITEMS + 1, '256')):
        with pytest.raises(_native.NativeError, match=msg):
            m.recommend_step(np.zeros(3, dtype=np.int32), None, k)
    with pytest.raises(_native.NativeError, match='n_sel'):
        m.recommend_step(np.zeros(3, dtype=np.int32), np.arange(4, dtype=np.int32), 5)


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
    """10,000,000 x 256, 8 rows, k = 100 through the C ABI against predict_step at the same shape and hidden state.  Wy is a block of
    4093 random rows repeated, so equal scores recur all over the catalogue (ties across column ranges); winners are planted through
    By at item 0, n_items - 1 and either side of the byte offsets 2^31 / 2^32 / 2^33 of Wy."""
    I, D, B, k = 10_000_000, 256, 8, 100
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
        m.predict_begin(B)
        S = m.predict_step(in_idx)
        m.predict_begin(B)
        cols, scores = m.recommend_step(in_idx, None, k)
        want_cols, want = topk_oracle(S, k)
        np.testing.assert_array_equal(cols, want_cols)
        np.testing.assert_array_equal(scores.view(np.uint32), want.view(np.uint32))
        assert set(planted) <= set(cols[0].tolist())
    finally:
        m.close()

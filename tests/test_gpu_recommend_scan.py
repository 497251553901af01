"""scan='bf16' of GRU4Rec.recommend_next_batch / recommend_sessions (g4r_recommend_step_scan / g4r_recommend_sessions_scan): a bf16 scan
keeps c = k * oversample candidates per row, which are re-ranked by their exact fp32 scores.

What holds for ANY input: every returned score is the same call's predict_next_batch score bit for bit, the list is in the contract's
order (score descending, equal scores by the lower column, NaN last), no column comes twice and no excluded item comes at all.  What
holds when c covers the row's eligible columns: the result IS the exact call's.  And what holds on CERTIFIED rows: with
    e(row, item) = sum_i |h_i w_i| * (2u + u^2 + (D + 2) 2^-24 (1 + u)^2),   u = 2^-8
(both operands rounded to bf16, fp32 accumulation of D products and the bias) a row is certified when every exact top-k item t has
fewer than c items j with s_j + e_j > s_t - e_t: the bf16 candidates then contain the exact top k, so the result must equal the exact
call's bit for bit.  The certified tests assert that ALL their rows are certified, so they cannot pass by skipping."""
import numpy as np
import pytest

from gru4rec_amd import _native
from gru4rec_amd.gru4rec import GRU4Rec
from test_gpu_recommend import N_ITEMS, _MODELS, assert_same, fitted, subset_with_duplicates, topk_oracle

pytestmark = pytest.mark.gpu

U = 2.0 ** -8


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check_invariants(S, cand_ids, items, scores, k, excluded=None):
    """S: [rows, n_sel] predict_next_batch scores of the same call; cand_ids: the candidates' ids in column order.  The j-th
    occurrence of an id in a row is taken to be the j-th lowest column holding it (what the tie rule demands)."""
    rows = S.shape[0]
    assert items.shape == scores.shape == (rows, k) and scores.dtype == np.float32
    cols_of = {}
    for c, i in enumerate(cand_ids):
        cols_of.setdefault(i, []).append(c)
    for r in range(rows):
        seen, prev = {}, None
        for j in range(k):
            i = items[r, j]
            n = seen.get(i, 0)
            assert n < len(cols_of[i]), 'row %d: id %r returned more often than it is a candidate' % (r, i)
            col = cols_of[i][n]
            seen[i] = n + 1
            assert bits(scores[r, j]) == bits(S[r, col]), 'row %d entry %d: not the predict_next_batch bits' % (r, j)
            assert excluded is None or i not in excluded[r], 'row %d: excluded id %r returned' % (r, i)
            key = (1 if np.isnan(scores[r, j]) else 0, -np.float64(0.0 if np.isnan(scores[r, j]) else scores[r, j]), col)
            assert prev is None or prev < key, 'row %d: entries %d, %d out of order' % (r, j - 1, j)
            prev = key


def both_calls(g, rows, k, cand, seed, **kw):
    """predict_next_batch (the oracle) and recommend_next_batch(**kw) as the last call of the same sequence from a fresh state."""
    rng = np.random.RandomState(seed)
    ids = g.itemidmap.index.values
    seq = [(rng.randint(0, 3, size=rows), ids[rng.randint(0, len(ids), size=rows)]) for _ in range(2)]
    out = []
    for mode in ('predict', 'recommend'):
        g.predict = None
        g.predict_next_batch(seq[0][0], seq[0][1], predict_for_item_ids=cand, batch=rows)
        if mode == 'predict':
            out.append(g.predict_next_batch(seq[1][0], seq[1][1], predict_for_item_ids=cand, batch=rows).values.T.astype(np.float32))
        else:
            out.append(g.recommend_next_batch(seq[1][0], seq[1][1], k=k, predict_for_item_ids=cand, batch=rows, **kw))
    return out[0], out[1]


@pytest.mark.parametrize('final_act', ['linear', 'elu-0.5', 'relu', 'tanh'])
@pytest.mark.parametrize('D', [64, 100])
def test_exact_scores_and_contract_order(final_act, D):
    """Test 1: fitted models; the overlap with the exact top k is printed, not asserted."""
    g = fitted(final_act, D)
    ids = g.itemidmap.index.values
    sub = subset_with_duplicates(g, 2000)
    worst = 1.0
    for rows in (1, 5, 130):
        for k, over in ((1, 8), (20, 8), (256, 4)):
            for cand in (None, sub):
                S, (items, scores) = both_calls(g, rows, k, cand, seed=rows + k, scan='bf16', oversample=over)
                C = ids if cand is None else cand
                check_invariants(S, C, items, scores, k)
                cols, _ = topk_oracle(S, k)
                want = C[cols]
                worst = min(worst, min(len(set(a) & set(b)) / k for a, b in zip(items, want)))
    print('fitted %s D=%d: smallest overlap of a row with the exact top k: %.3f' % (final_act, D, worst))


def _with_weights(final_act, D=64, Wy=None, By=None, scale=None):
    g = fitted(final_act, D)
    if Wy is not None:
        g.Wy = np.ascontiguousarray(Wy, dtype=np.float32)
    if scale is not None:
        g.Wy = g.Wy * np.float32(scale)
    if By is not None:
        g.By = np.ascontiguousarray(By, dtype=np.float32).reshape(-1, 1)
    g.close()
    return g


@pytest.mark.parametrize('case', ['fitted', 'relu_zeros', 'tanh_saturated'])
def test_degenerate_equals_the_exact_call(case):
    """Test 2: c >= n_sel: the two-stage result is the exact one, ties and all."""
    if case == 'relu_zeros':
        g, key = _with_weights('relu', Wy=np.zeros((N_ITEMS, 64)), By=np.full(N_ITEMS, -0.25)), ('relu', 64)
    elif case == 'tanh_saturated':
        g, key = _with_weights('tanh', scale=200.0), ('tanh', 64)
    else:
        g, key = fitted('linear', 64), None
    try:
        for n_sel, k, over in ((150, 20, 8), (160, 20, 8), (1000, 256, 4), (40, 40, 1), (7, 1, 8)):
            sub = subset_with_duplicates(g, max(n_sel, 12), seed=n_sel)[:n_sel]
            for rows in (1, 130):
                S, (items, scores) = both_calls(g, rows, k, sub, seed=rows + n_sel, scan='bf16', oversample=over)
                cols, want = topk_oracle(S, k)
                assert_same(items, scores, sub[cols], want)
                if case == 'relu_zeros':
                    assert (S == 0).all()
                elif case == 'tanh_saturated':
                    print('n_sel=%d rows=%d: share of scores saturated to +-1: %.3f' % (n_sel, rows, (np.abs(S) == 1).mean()))
    finally:
        if key:
            _MODELS.pop(key, None)


# ---- certified equality on hand-set weights ---------------------------------------------------------------------------------------
def certified_rows(h, Wy, By, k, c, eligible=None):
    """[rows] bool by the bound of the module docstring (linear final activation); eligible: [rows, n_items] bool or None."""
    h, Wy, By = h.astype(np.float64), Wy.astype(np.float64), By.astype(np.float64).ravel()
    D = Wy.shape[1]
    s = h @ Wy.T + By
    e = (np.abs(h) @ np.abs(Wy).T) * (2 * U + U * U + (D + 2) * 2.0 ** -24 * (1 + U) ** 2)
    ok = np.zeros(len(h), dtype=bool)
    for r in range(len(h)):
        el = np.ones(len(By), dtype=bool) if eligible is None else eligible[r]
        sr, er = s[r][el], e[r][el]
        top = np.argsort(-sr, kind='stable')[:k]
        upper = np.sort(sr + er)
        lower = (sr - er)[top].min()
        ok[r] = len(upper) - np.searchsorted(upper, lower, side='right') < c
    return ok


def native_model(I, D, seed=7):
    rng = np.random.RandomState(seed)
    m = _native.Model(n_items=I, layers=[D], batch_size=32, n_sample=0, loss=_native.LOSS_IDS['bpr-max'], final_act=_native.ACT_IDS['linear'],
                      hidden_act=_native.ACT_IDS['tanh'], embed_mode=0, embedding=0, learning_rate=0.1, sample_store=0, seed=3,
                      device=0, rank=0, nranks=1, use_graph=0)
    Wy = (rng.randn(I, D) * 0.1).astype(np.float32)
    By = (rng.randn(I) * 0.05).astype(np.float32)
    m.set_param('Wy', Wy)
    m.set_param('By', By)
    m.set_param('Wx', (rng.randn(D, 3 * D) * 0.3).astype(np.float32))      # (constrained embedding: the input rows are Wy's)
    m.set_param('Wh', (rng.randn(D, D) * 0.1).astype(np.float32))
    m.set_param('Wrz', (rng.randn(D, 2 * D) * 0.1).astype(np.float32))
    return m, Wy, By, rng


@pytest.mark.parametrize('I, D', [(20000, 64), (20000, 100), (37483, 100)])
def test_certified_rows_equal_the_exact_call(I, D):
    """Test 3, through the C ABI: 130 one-item sessions started from h0 = tanh(N(0, 1)); the bound uses the hidden state the call
    itself returns (the rows the scan scored)."""
    m, Wy, By, rng = native_model(I, D)
    try:
        rows = 130
        offs, hist = np.arange(rows + 1, dtype=np.int64), rng.randint(0, I, size=rows).astype(np.int32)
        h0 = [np.tanh(rng.randn(rows, D)).astype(np.float32)]
        for k, over in ((20, 8), (20, 4), (256, 4), (256, 2)):
            ec, es, H = m.recommend_sessions(offs, hist, None, k, hidden=h0, return_hidden=True)
            sc, ss, H2 = m.recommend_sessions(offs, hist, None, k, hidden=h0, return_hidden=True, oversample=over)
            np.testing.assert_array_equal(bits(H2[0]), bits(H[0]))
            ok = certified_rows(H[0], Wy, By, k, k * over)
            print('I=%d D=%d k=%d oversample=%d: %d of %d rows certified' % (I, D, k, over, ok.sum(), rows))
            assert ok.all(), 'uncertified rows: %s' % np.flatnonzero(~ok)
            np.testing.assert_array_equal(sc, ec)
            np.testing.assert_array_equal(bits(ss), bits(es))
        assert m.scan_table() == (((I + 31) // 32) * 32 * (128 if D <= 128 else 256) * 2, True, 1)
        m.scan_table_release()
        assert m.scan_table() == (0, False, 1)
        sc, ss = m.recommend_sessions(offs, hist, None, 20, hidden=h0, oversample=8)
        ec, es = m.recommend_sessions(offs, hist, None, 20, hidden=h0)
        np.testing.assert_array_equal(sc, ec)
        assert m.scan_table()[1:] == (True, 2)
    finally:
        m.close()


def _hand_set(D=64, seed=21):
    rng = np.random.RandomState(seed)
    g = _with_weights('linear', D, Wy=rng.randn(N_ITEMS, D) * 0.1, By=rng.randn(N_ITEMS) * 0.05)
    return g, rng


def _certify_sessions(g, hists, k, c, excluded_idx=None):
    """All rows of a recommend_sessions call certified?  (hidden state taken from the exact call)"""
    _, _, H = g.recommend_sessions(hists, k=k, return_hidden=True)
    el = None
    if excluded_idx is not None:
        el = np.ones((len(hists), N_ITEMS), dtype=bool)
        for r, x in enumerate(excluded_idx):
            el[r, list(x)] = False
    ok = certified_rows(H[-1], g.Wy, g.By, k, c, el)
    assert ok.all(), 'uncertified rows: %s' % np.flatnonzero(~ok)


def test_exclusions_through_the_scan():
    """Test 4: global and per-row exclusions, on certified inputs equal to the exact filtered call; a row left with exactly k eligible
    items; never an excluded item."""
    g, rng = _hand_set()
    try:
        ids = g.itemidmap.index.values
        idx = g.itemidmap
        rows, k, over = 130, 20, 8
        hists = [[ids[i]] for i in rng.randint(0, N_ITEMS, size=rows)]
        # the exact unfiltered top 40 of every row are excluded per row (so the filter matters), + 3000 items for everybody
        top_items, _ = g.recommend_sessions(hists, k=40)
        glob = ids[rng.choice(N_ITEMS, size=3000, replace=False)]
        per_row = [list(t) + list(ids[rng.randint(0, N_ITEMS, size=30)]) for t in top_items]
        gone = [set(idx[glob].values) | set(idx[p].values) | {idx[h[0]]} for p, h in zip(per_row, hists)]
        _certify_sessions(g, hists, k, k * over, gone)
        kw = dict(exclude=glob, exclude_per_row=per_row, exclude_history=True)
        ei, es = g.recommend_sessions(hists, k=k, **kw)
        si, ss = g.recommend_sessions(hists, k=k, scan='bf16', oversample=over, **kw)
        assert_same(si, ss, ei, es)
        gone_ids = [set(ids[list(x)]) for x in gone]
        assert all(not (set(r) & x) for r, x in zip(si, gone_ids))
        # the stepwise call: one step from a fresh state is the one-item session
        sid, inp = np.arange(rows), np.array([h[0] for h in hists])
        g.predict = None
        ni, ns = g.recommend_next_batch(sid, inp, k=k, batch=rows, exclude_seen=True, exclude=glob, exclude_per_row=per_row, scan='bf16',
                                        oversample=over)
        assert_same(ni, ns, ei, es)
        # a candidate subset that leaves row 0 exactly k eligible positions (c > eligible: degenerate = exact), others more
        sub = ids[rng.choice(N_ITEMS, size=250, replace=False)]
        per_row2 = [list(sub[k:]) if r == 0 else list(sub[:5 * (r % 7)]) for r in range(rows)]
        for scan_kw in (dict(scan='bf16', oversample=13), dict(scan='bf16', oversample=1)):      # c = n_sel = 250, c = k
            a = g.recommend_sessions(hists, k=k, predict_for_item_ids=sub, exclude_per_row=per_row2)
            b = g.recommend_sessions(hists, k=k, predict_for_item_ids=sub, exclude_per_row=per_row2, **scan_kw)
            assert set(b[0][0]) == set(sub[:k])
            assert all(not (set(r) & set(x)) for r, x in zip(b[0], per_row2))
            if scan_kw['oversample'] == 13:
                assert_same(b[0], b[1], a[0], a[1])
            else:       # c = k: only the invariants hold in general; the scores must still be exact ones
                S = g.recommend_sessions(hists, k=len(sub), predict_for_item_ids=sub)
                for r in range(rows):
                    exact = dict(zip(S[0][r], bits(S[1][r])))
                    assert all(exact[i] == s for i, s in zip(b[0][r], bits(b[1][r])))
    finally:
        _MODELS.pop(('linear', 64), None)


def test_stateless_twin_chunks_and_hidden(monkeypatch):
    """Test 5: recommend_sessions(scan='bf16') on ragged histories in several chunks: equal to the exact call where certified
    (hand-set weights), hidden states bit-identical, and equal to the stepwise route's scan."""
    g, rng = _hand_set(seed=22)
    try:
        ids = g.itemidmap.index.values
        lens = rng.randint(1, 12, size=200)
        hists = [ids[rng.randint(0, N_ITEMS, size=n)] for n in lens]
        _certify_sessions(g, hists, 20, 160)
        ei, es, EH = g.recommend_sessions(hists, k=20, return_hidden=True)
        monkeypatch.setenv('G4R_SESSIONS_CHUNK', '37')
        si, ss, SH = g.recommend_sessions(hists, k=20, return_hidden=True, scan='bf16', oversample=8)
        monkeypatch.delenv('G4R_SESSIONS_CHUNK')
        assert_same(si, ss, ei, es)
        for a, b in zip(SH, EH):
            np.testing.assert_array_equal(bits(a), bits(b))
        # stepwise: all but the last items through predict_next_batch, aligned to end together, the last through the scan
        T, N = int(lens.max()), len(hists)
        g.predict = None
        for s in range(T):
            live = [s >= T - len(h) for h in hists]
            sid = np.array([i if a else -2 - i for i, a in enumerate(live)])
            inp = np.array([h[s - (T - len(h))] if a else ids[0] for h, a in zip(hists, live)])
            if s < T - 1:
                g.predict_next_batch(sid, inp, predict_for_item_ids=ids[:1], batch=N)
        ni, ns = g.recommend_next_batch(sid, inp, k=20, batch=N, scan='bf16', oversample=8)
        g.predict = None
        assert_same(ni, ns, si, ss)
    finally:
        _MODELS.pop(('linear', 64), None)


def test_staleness(tmp_path):
    """Test 6: the shadow table follows Wy: a live g4r_set_param, weights assigned + close(), one more fit epoch, loadmodel."""
    g, rng = _hand_set(seed=23)
    try:
        ids = g.itemidmap.index.values
        hists = [[ids[i]] for i in rng.randint(0, N_ITEMS, size=130)]

        def scan_equals_exact(model):
            _certify_sessions(model, hists, 20, 160)
            e = model.recommend_sessions(hists, k=20)
            s = model.recommend_sessions(hists, k=20, scan='bf16', oversample=8)
            assert_same(s[0], s[1], e[0], e[1])
            return s

        first = scan_equals_exact(g)
        m = g._model
        assert m.scan_table()[1:] == (True, 1)
        scan_equals_exact(g)
        assert m.scan_table()[1:] == (True, 1)                          # nothing changed: not rebuilt
        # (a) a live parameter upload
        W2 = (rng.randn(N_ITEMS, 64) * 0.1).astype(np.float32)
        m.set_param('Wy', W2)
        assert m.scan_table()[1:] == (False, 1)
        g.Wy = W2
        second = scan_equals_exact(g)
        assert m.scan_table()[1:] == (True, 2)
        assert not np.array_equal(first[0], second[0])
        # (b) direct assignment + close(): a new device model
        g.Wy = (rng.randn(N_ITEMS, 64) * 0.1).astype(np.float32)
        g.close()
        third = scan_equals_exact(g)
        assert not np.array_equal(third[0], second[0])
        g.savemodel(str(tmp_path / 'hand.pickle'))
    finally:
        _MODELS.pop(('linear', 64), None)
    # (c) one more fit epoch on a fitted model (invariants on any input), with the scan used before and after
    f = fitted('linear', 64)
    try:
        ids = f.itemidmap.index.values
        S, (i0, s0) = both_calls(f, 130, 20, None, seed=1, scan='bf16', oversample=8)
        check_invariants(S, ids, i0, s0, 20)
        items = 10 + 3 * np.concatenate([np.random.RandomState(64).permutation(N_ITEMS), np.random.RandomState(65).randint(0, N_ITEMS, size=N_ITEMS)])
        import pandas as pd
        sess = np.repeat(np.arange(len(items) // 5), 5)
        f.fit(pd.DataFrame({'SessionId': sess, 'ItemId': items[:len(sess)], 'Time': np.arange(len(sess), dtype=np.int64)}), sample_store=100000)
        S1, (i1, s1) = both_calls(f, 130, 20, None, seed=1, scan='bf16', oversample=8)
        assert not np.array_equal(bits(S), bits(S1))
        check_invariants(S1, f.itemidmap.index.values, i1, s1, 20)
    finally:
        _MODELS.pop(('linear', 64), None)
    # (d) loadmodel of the hand-set checkpoint
    h = GRU4Rec.loadmodel(str(tmp_path / 'hand.pickle'))
    try:
        e = h.recommend_sessions(hists, k=20)
        s = h.recommend_sessions(hists, k=20, scan='bf16', oversample=8)
        assert_same(s[0], s[1], e[0], e[1])
        assert_same(s[0], s[1], third[0], third[1])
        assert h._model.scan_table()[1:] == (True, 1)
    finally:
        h.close()


def test_training_marks_the_table_stale():
    """g4r_train_steps after a scan: the debug query shows the table invalid, the next scan rebuilds it."""
    m, Wy, By, rng = native_model(500, 64)
    try:
        I, B, T = 500, 32, 4
        offs, hist = np.arange(9, dtype=np.int64), rng.randint(0, I, size=8).astype(np.int32)
        m.recommend_sessions(offs, hist, None, 5, oversample=4)
        assert m.scan_table()[1:] == (True, 1)
        m.set_plan(dict(in_idx=rng.randint(0, I, size=(T, B)).astype(np.int32), out_idx=rng.randint(0, I, size=(T, B)).astype(np.int32),
                        reset=np.zeros((T, B), dtype=np.uint8), M=np.full(T, B, dtype=np.int32), n_compact=0, compact_steps=None,
                        compact_maps=None))
        m.reset_hidden()
        m.train_steps(0, T)
        assert m.scan_table()[1:] == (False, 1)
        a = m.recommend_sessions(offs, hist, None, 5, oversample=100)        # c = n_items: equal to the exact call on the new weights
        b = m.recommend_sessions(offs, hist, None, 5)
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(bits(a[1]), bits(b[1]))
        assert m.scan_table()[1:] == (True, 2)
    finally:
        m.close()


def test_interleaved_calls_keep_the_session_state():
    """Test 7: a random sequence of predict_next_batch / exact / scan calls with session and batch-size changes against the same
    sequence of predict_next_batch calls only."""
    g = fitted('elu-0.5', 64)
    rng = np.random.RandomState(12)
    ids = g.itemidmap.index.values
    sub = subset_with_duplicates(g, 300, seed=5)
    calls, sessions = [], np.arange(40)
    for t in range(16):
        if t == 9:
            sessions = np.arange(48)
        B = len(sessions)
        sessions = np.where(rng.rand(B) < 0.3, rng.randint(100, 10000, size=B), sessions)
        calls.append((sessions.copy(), ids[rng.randint(0, len(ids), size=B)], rng.choice(['predict', 'fp32', 'bf16'], p=[0.3, 0.3, 0.4]),
                      int(rng.choice([1, 20, 100])), sub if rng.rand() < 0.3 else None, B))
    got = []
    g.predict = None
    for sid, inp, mode, k, cand, batch in calls:
        if mode == 'predict':
            g.predict_next_batch(sid, inp, predict_for_item_ids=cand, batch=batch)
        else:
            got.append(g.recommend_next_batch(sid, inp, k=k, predict_for_item_ids=cand, batch=batch, scan=mode, oversample=4))
    g.predict = None
    n = 0
    for sid, inp, mode, k, cand, batch in calls:
        S = g.predict_next_batch(sid, inp, predict_for_item_ids=cand, batch=batch).values.T.astype(np.float32)
        if mode == 'predict':
            continue
        items, scores = got[n]
        n += 1
        C = ids if cand is None else cand
        if mode == 'fp32':
            cols, sc = topk_oracle(S, k)
            assert_same(items, scores, C[cols], sc)
        else:
            check_invariants(S, C, items, scores, k)
    assert n == len(got) > 5
    g.predict = None


def test_c_abi_refuses_bad_arguments():
    m, Wy, By, rng = native_model(500, 64)
    try:
        m.predict_begin(3)
        inp = np.zeros(3, dtype=np.int32)
        for k, over in ((20, 0), (20, 52), (256, 5)):
            with pytest.raises(_native.NativeError, match='G4R_SCAN_CAND_MAX = 1024'):
                m.recommend_step_filtered(inp, None, k, oversample=over)
        with pytest.raises(_native.NativeError, match='256'):
            m.recommend_step_filtered(inp, None, 257, oversample=1)
        with pytest.raises(_native.NativeError, match='G4R_SCAN_CAND_MAX = 1024'):
            m.recommend_sessions(np.arange(4, dtype=np.int64), inp, None, 20, oversample=0)
    finally:
        m.close()

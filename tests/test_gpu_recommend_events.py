"""evaluation.recommend_gpu / g4r_recommend_events (the top-k list, the target's rank and score at EVERY event of a test set, one
pass over the candidates per step) against the library's own pinned entries: recommend_sessions on every event's prefix (lists, bit
for bit), evaluate_gpu's sums (ranks, exactly), predict_next_batch's scores restated in NumPy (rank and list agree), and the launch
counter of the call (one scan of the candidate columns per step)."""
import numpy as np
import pandas as pd
import pytest

from gru4rec_amd import _native, evaluation

from test_gpu_recommend_sessions import N_ITEMS, assert_bits, fitted

pytestmark = pytest.mark.gpu

BATCH = 48


def make_test_set(g, n_sessions=300, seed=0, max_len=30, repeats=True):
    """Sessions of 2 .. max_len events over the model's items, session ids shuffled so that the table has to be sorted; every third
    session draws from a pool of 6 items, so it repeats items."""
    rng = np.random.RandomState(seed)
    ids = g.itemidmap.index.values
    lens = rng.randint(2, max_len + 1, size=n_sessions)
    sess, items = [], []
    for s, n in enumerate(lens):
        pool = ids[rng.randint(0, len(ids), size=6)] if (repeats and s % 3 == 0) else ids
        items.append(pool[rng.randint(0, len(pool), size=n)])
        sess.append(np.full(n, 1000 + 7 * s))
    data = pd.DataFrame({'SessionId': np.concatenate(sess).astype(np.int32), 'ItemId': np.concatenate(items),
                         'Time': np.arange(int(lens.sum()), dtype=np.int64)})
    return data.iloc[rng.permutation(len(data))].reset_index(drop=True)


def sorted_table(data):
    return data.sort_values(['SessionId', 'Time', 'ItemId']).reset_index(drop=True)


def prefixes(data, rows):
    """The history of every scored event: its session's items up to and including the event at table row `rows[i]`."""
    t = sorted_table(data)
    sess, items = t.SessionId.values, t.ItemId.values
    start = np.zeros(len(t), dtype=np.int64)
    new = np.flatnonzero(np.r_[True, sess[1:] != sess[:-1]])
    start[new] = new
    start = np.maximum.accumulate(start)
    return [items[start[r]:r + 1] for r in rows], t


def check_table_columns(res, data):
    hists, t = prefixes(data, res['row'])
    sess, items = t.SessionId.values, t.ItemId.values
    has_next = np.r_[sess[1:] == sess[:-1], False]
    np.testing.assert_array_equal(res['row'], np.flatnonzero(has_next))      # every event with a successor, none left out
    np.testing.assert_array_equal(res['session'], sess[res['row']])
    np.testing.assert_array_equal(res['target'], items[res['row'] + 1])
    return hists


# ---- 1. lists, bit for bit ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', [1, 20, 256])
@pytest.mark.parametrize('cand', [False, True])
@pytest.mark.parametrize('final_act', ['elu-0.5', 'softmax'])
@pytest.mark.parametrize('embed', ['onehot', 'embedding', 'constrained'])
@pytest.mark.parametrize('layers', [(64,), (100, 64)])
def test_lists_equal_recommend_sessions_of_every_prefix(layers, embed, final_act, cand, k):
    g = fitted(final_act, layers, embed)
    data = make_test_set(g, seed=len(layers) + k)
    ids = g.itemidmap.index.values
    items = ids[np.random.RandomState(k).permutation(len(ids))[:700]] if cand else None
    res = evaluation.recommend_gpu(g, data, k=k, items=items, batch_size=BATCH)
    hists = check_table_columns(res, data)
    assert len(hists) > 2000 and res['items'].shape == res['scores'].shape == (len(hists), k)
    want_items, want_scores = g.recommend_sessions(hists, k=k, predict_for_item_ids=items)
    np.testing.assert_array_equal(res['items'], want_items)
    assert_bits(res['scores'], want_scores)


# ---- 2. ranks against g4r_evaluate ----------------------------------------------------------------------------------------------
def tied_model():
    """relu scores (many exact zeros) and a block of 40 items that share one row of Wy / By: standard, conservative and median differ."""
    g = fitted('relu', (64,), 'onehot')
    if not getattr(g, '_tied', False):
        g.Wy[100:140] = g.Wy[100]
        g.By[100:140] = g.By[100]
        g.close()
        g._tied = True
    return g


@pytest.mark.parametrize('cand', [False, True])
@pytest.mark.parametrize('model', ['tied', 'elu', 'softmax'])
def test_ranks_equal_evaluate_gpu(model, cand):
    g = tied_model() if model == 'tied' else fitted('elu-0.5' if model == 'elu' else 'softmax')
    data = make_test_set(g, seed=11)
    ids = g.itemidmap.index.values
    if model == 'tied':      # half of the targets inside the tied block
        t = data.ItemId.values.copy()
        t[::2] = ids[100 + np.arange(len(t[::2])) % 40]
        data = data.assign(ItemId=t)
    # the candidates hold every target: a target outside them has conservative rank 0 in g4r_evaluate, and 1 / rank is no number
    items = np.unique(np.r_[ids[90:150], data.ItemId.values])[::-1] if cand else None
    cuts = [1, 5, 20, 100]
    titems, item_idxs, offs = evaluation._prepare(g, data.copy(), items, 'SessionId', 'ItemId', 'Time')
    plan = _native.build_plan(offs.astype(np.int32), np.arange(len(offs) - 1), titems, BATCH, 1)
    seen = {}
    for mode in ('standard', 'conservative', 'median', 'tiebreaking'):
        rec_sum, mrr_sum, n = g._ensure_model().evaluate(plan, BATCH, item_idxs, cuts, mode)
        res = evaluation.recommend_gpu(g, data, k=5, items=items, batch_size=BATCH, mode=mode)
        rank = res['rank'].astype(np.float64)
        assert len(rank) == n
        for j, c in enumerate(cuts):
            hit = rank <= c
            print(model, cand, mode, c, int(hit.sum()), rec_sum[j], (1.0 / rank[hit]).sum(), mrr_sum[j])
            assert int(hit.sum()) == int(rec_sum[j]) and rec_sum[j] == int(rec_sum[j])
            assert abs((1.0 / rank[hit]).sum() - mrr_sum[j]) <= 1e-9 * mrr_sum[j]
        m = evaluation.list_metrics(res, cuts)
        want = evaluation.evaluate_gpu(g, data.copy(), items=items, cut_off=cuts, batch_size=BATCH, mode=mode)
        np.testing.assert_allclose(m['recall'], want[0], rtol=1e-12)
        np.testing.assert_allclose(m['mrr'], want[1], rtol=1e-9)
        seen[mode] = rank
    if model == 'tied':
        assert (seen['standard'] != seen['conservative']).any() and (seen['median'] != seen['standard']).any()
        assert (seen['median'] != seen['conservative']).any()


# ---- 3. rank and list agree (standard mode, scores restated from predict_next_batch) ---------------------------------------------
def test_rank_list_and_target_score_agree_with_predict_next_batch():
    g = tied_model()
    k, n_sess, B = 20, 40, 16
    data = make_test_set(g, n_sessions=n_sess, seed=3, max_len=12)
    ids = g.itemidmap.index.values
    t = data.ItemId.values.copy()
    t[::3] = ids[100 + np.arange(len(t[::3])) % 40]
    data = data.assign(ItemId=t)
    res = evaluation.recommend_gpu(g, data, k=k, batch_size=B)
    tab = sorted_table(data)
    sess, items = tab.SessionId.values, tab.ItemId.values
    starts = np.flatnonzero(np.r_[True, sess[1:] != sess[:-1]])
    lens = np.diff(np.r_[starts, len(tab)])
    row_of = {r: i for i, r in enumerate(res['row'])}
    g.predict = None
    checked = 0
    for step in range(lens.max() - 1):
        live = lens - 1 > step
        inp = np.where(live, items[np.minimum(starts + step, len(tab) - 1)], ids[0])
        scores = g.predict_next_batch(np.arange(n_sess), inp, batch=n_sess).values.T      # [session, item]
        for s in np.flatnonzero(live):
            i = row_of[starts[s] + step]
            row = scores[s]
            ts = row[g.itemidmap[res['target'][i]]]
            assert_bits(res['target_score'][i:i + 1], np.array([ts]))
            gt, eq = int((row > ts).sum()), int((row == ts).sum())
            assert res['rank'][i] == gt + 1                      # evaluation.py's standard rule: (others > target).sum() + 1
            where = np.flatnonzero(res['items'][i] == res['target'][i])
            if gt < k:
                assert len(where) == 1 and gt <= where[0] < gt + eq
            else:
                assert len(where) == 0
            checked += 1
    g.predict = None
    assert checked == len(res['row'])


# ---- 4. exclusions --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cand', [False, True])
@pytest.mark.parametrize('final_act', ['elu-0.5', 'softmax'])
def test_exclusions(final_act, cand):
    g = fitted(final_act)
    data = make_test_set(g, seed=21)
    ids = g.itemidmap.index.values
    items = ids[np.random.RandomState(2).permutation(len(ids))[:900]] if cand else None
    plain = evaluation.recommend_gpu(g, data, k=20, items=items, batch_size=BATCH)
    banned = plain['items'][:, 0][:50]                # items that do lead lists
    res = evaluation.recommend_gpu(g, data, k=20, items=items, batch_size=BATCH, exclude_seen=True, exclude=banned)
    hists = check_table_columns(res, data)
    assert any(len(set(h)) < len(h) for h in hists)      # sessions with repeated items are among them
    want_items, want_scores = g.recommend_sessions(hists, k=20, predict_for_item_ids=items, exclude_history=True, exclude=banned)
    np.testing.assert_array_equal(res['items'], want_items)
    assert_bits(res['scores'], want_scores)
    assert not np.isin(res['items'], banned).any()
    assert (res['items'] != plain['items']).any()
    np.testing.assert_array_equal(res['rank'], plain['rank'])      # exclusions shape the list, never the rank
    assert_bits(res['target_score'], plain['target_score'])
    only_seen = evaluation.recommend_gpu(g, data, k=20, items=items, batch_size=BATCH, exclude_seen=True)
    w_items, w_scores = g.recommend_sessions(hists, k=20, predict_for_item_ids=items, exclude_history=True)
    np.testing.assert_array_equal(only_seen['items'], w_items)
    assert_bits(only_seen['scores'], w_scores)


def test_too_few_candidates_left_is_refused_naming_the_session():
    g = fitted('elu-0.5')
    data = make_test_set(g, seed=22)
    tab = sorted_table(data)
    distinct = tab.groupby('SessionId').ItemId.nunique()
    first = distinct.idxmax()                                 # the session with the most distinct items
    own = pd.unique(tab.ItemId.values[tab.SessionId.values == first])
    assert len(own) >= 8
    ids = g.itemidmap.index.values
    items = np.r_[own, np.setdiff1d(ids, tab.ItemId.values)[:18]]      # its own items + 18 candidates no session ever sees
    before = g._ensure_model().events_launches()
    with pytest.raises(ValueError, match='session %d' % first):
        evaluation.recommend_gpu(g, data, k=20, items=items, batch_size=BATCH, exclude_seen=True)
    with pytest.raises(ValueError, match='eligible'):
        evaluation.recommend_gpu(g, data, k=20, items=items[:25], batch_size=BATCH, exclude=items[:10])
    assert g._ensure_model().events_launches() == before      # nothing was launched
    evaluation.recommend_gpu(g, data, k=20, items=items, batch_size=BATCH)


# ---- 5. a large catalogue once: many ranges per row, the lists downloaded in pieces ----------------------------------------------
def test_million_items_against_sampled_prefixes(monkeypatch):
    I, D, B, k = 1000000, 64, 32, 20
    rng = np.random.RandomState(5)
    m = _native.Model(n_items=I, layers=[D], batch_size=32, n_sample=0, loss=_native.LOSS_IDS['bpr-max'], final_act=_native.ACT_IDS['linear'],
                      hidden_act=_native.ACT_IDS['tanh'], embed_mode=0, embedding=0, learning_rate=0.1, sample_store=0, seed=3,
                      device=0, rank=0, nranks=1, use_graph=0)
    block = (rng.randn(8192, D) * 0.1).astype(np.float32)
    Wy = np.tile(block, (I // 8192 + 1, 1))[:I] * (1.0 + 1e-3 * (np.arange(I, dtype=np.float32) % 977))[:, None]
    m.set_param('Wy', Wy.astype(np.float32))
    m.set_param('By', (rng.randn(I) * 0.01).astype(np.float32))
    for name, shape in (('Wx', (D, 3 * D)), ('Wh', (D, D)), ('Wrz', (D, 2 * D)), ('Bh', (3 * D,))):
        m.set_param(name, (rng.randn(*shape) * 0.1).astype(np.float32))
    lens = rng.randint(2, 31, size=200)
    offs = np.r_[0, np.cumsum(lens)].astype(np.int64)
    titems = rng.randint(0, I, size=int(offs[-1])).astype(np.int32)
    plan = _native.build_plan(offs.astype(np.int32), np.arange(len(lens)), titems, B, 1)
    _, table = evaluation.slot_map(offs, B)
    has_next = np.ones(len(titems), dtype=bool)
    has_next[offs[1:] - 1] = False
    rows = np.flatnonzero(has_next)
    number = np.full(len(titems) + 1, -1, dtype=np.int64)
    number[rows] = np.arange(len(rows))
    slot = number[table]
    assert len(rows) > 2000
    one = m.recommend_events(plan, B, None, 'standard', slot, len(rows), k)
    assert m.events_launches()[3] == 1
    monkeypatch.setenv('G4R_EVENTS_PIECE', str(64 * 1024))
    li, ls, rank, ts = m.recommend_events(plan, B, None, 'standard', slot, len(rows), k)
    steps, scans, _, pieces = m.events_launches()
    assert pieces > 3 and scans == steps == plan['T']
    for a, b in zip(one, (li, ls, rank, ts)):
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))      # the pieces change nothing
    pick = rng.choice(len(rows), size=64, replace=False)
    sess = np.searchsorted(offs, rows[pick], side='right') - 1
    hist = [titems[offs[s]:r + 1] for s, r in zip(sess, rows[pick])]
    hoffs = np.r_[0, np.cumsum([len(h) for h in hist])].astype(np.int64)
    cols, scores = m.recommend_sessions(hoffs, np.concatenate(hist), None, k)
    np.testing.assert_array_equal(li[pick], cols)
    assert_bits(ls[pick], scores)
    assert (rank[pick] >= 1).all() and (rank <= I).all()
    m.close()


# ---- 6. one pass ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('exclude_seen', [False, True])
def test_one_scan_of_the_candidates_per_step(exclude_seen):
    g = fitted('elu-0.5')
    data = make_test_set(g, seed=31)
    evaluation.recommend_gpu(g, data, k=20, batch_size=BATCH, exclude_seen=exclude_seen)
    steps, scans, launches, pieces = g._ensure_model().events_launches()
    assert steps > 50 and scans == steps and pieces == 1
    g2 = fitted('softmax')
    evaluation.recommend_gpu(g2, data, k=20, batch_size=BATCH, exclude_seen=exclude_seen)
    s2 = g2._ensure_model().events_launches()
    assert s2[0] == steps and s2[1] == 4 * steps      # softmax: scored, normalised, ranked and selected in passes of their own

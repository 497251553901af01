"""Per-group caps on the device (k_group_cap behind recommend_sessions / continue_sessions, and cap_lists) against the host loop they
replace: recommend_sessions(k=pool) with the same arguments followed by the NumPy statement of the cap rule (tests/group_caps_ref.py).
Item ids, score BITS (pads compared as pads), pool positions, n_kept and the hidden-state bits have to be equal: nothing here is a
tolerance.  The continuation's host loop carries the hidden states, the per-row exclusions as continue_sessions' docstring defines
them, and the prior groups, one recommend_sessions(k=pool) call per step.

Fixture groups: item index i is ungrouped when i % 7 == 0, otherwise its group is i % 5."""
import numpy as np
import pandas as pd
import pytest

import group_caps_ref as ref
from gru4rec_amd import _native
from gru4rec_amd.gru4rec import GRU4Rec

pytestmark = pytest.mark.gpu

_MODELS = {}
# (items, top layer, input, final activation, loss)
TABLES = {'300x36': (300, 36, 'separate', 'linear', 'bpr-max'), '3000x100': (3000, 100, 'onehot', 'linear', 'bpr-max'),
          '300x36-softmax': (300, 36, 'constrained', 'softmax', 'cross-entropy')}
POOLS = (1, 63, 64, 65, 128, 256)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def fixture_groups(n_items):
    i = np.arange(n_items)
    return np.where(i % 7 == 0, -1, i % 5)


def set_groups(g, table):
    """Groups by item index (-1 = ungrouped) through the public call; labels 'G<index>'."""
    ids = g.itemidmap.index.values
    g.set_item_groups({ids[i]: 'G%d' % t for i, t in enumerate(table) if t >= 0})


def fitted(name, steps=30):
    """A GRU4Rec trained for `steps` mini-batches on synthetic sessions that hold every one of the table's items (ids 10, 13, 16, ...),
    with the fixture groups set."""
    if name not in _MODELS:
        n_items, D, mode, final_act, loss = TABLES[name]
        rng = np.random.RandomState(D + n_items)
        n_ev = max(2 * n_items, 400)
        items = 10 + 3 * np.concatenate([rng.permutation(n_items), rng.randint(0, n_items, size=n_ev - n_items)])
        sess = np.repeat(np.arange(n_ev // 5), 5)
        data = pd.DataFrame({'SessionId': sess, 'ItemId': items[:len(sess)], 'Time': np.arange(len(sess), dtype=np.int64)})
        g = GRU4Rec(layers=[D], final_act=final_act, loss=loss, n_epochs=1, batch_size=32, n_sample=64, learning_rate=0.1,
                    constrained_embedding=mode == 'constrained', embedding=64 if mode == 'separate' else 0)
        g.prepare(data, sample_store=64 * 256)
        assert g.n_items == n_items
        w0 = g.Wy.copy()
        assert g.run_epoch(0, max_steps=steps) is not None
        g._download_weights()
        assert (g.Wy != w0).any()
        _MODELS[name] = g
    g = _MODELS[name]
    want = fixture_groups(g.n_items)
    if g.item_groups is None or len(g.group_labels) != 5:
        set_groups(g, want)
    # (labels are numbered in order of first appearance: compare the partition, not the indices)
    assert ((g.item_groups < 0) == (want < 0)).all()
    return g


def histories(g, n, seed, longest=7):
    ids = g.itemidmap.index.values
    rng = np.random.RandomState(seed)
    return [ids[rng.randint(0, len(ids), size=rng.randint(1, longest))] for _ in range(n)]


def native_capped(g, hist, P, k, cap, predict_for_item_ids=None, exclude_history=False, exclude=None, exclude_per_row=None,
                  exclude_groups=None, hidden=None, scan='fp32', oversample=8):
    """g4r_recommend_sessions_capped with the front end's packing: (columns, scores, pool positions, n_kept)."""
    over = g._scan_oversample(scan, oversample, P)
    N, lens, offs, hidx, h0 = g._session_inputs(hist, hidden)
    iidx, cand = g._candidates(predict_for_item_ids)
    excl = g._session_exclusions(N, lens, hidx, P, iidx, exclude_history, exclude, exclude_per_row, exclude_groups=exclude_groups)
    return g._ensure_model().recommend_sessions_capped(offs, hidx, iidx, k, P, cap, *excl, hidden=h0, oversample=over)


def check_capped(g, hist, P, kcaps, tag, **kw):
    """The pool once, then every (k, cap) of kcaps against the NumPy rule over it.  Returns the oracle's n_kept of the last pair."""
    pool_items, pool_scores, H0 = g.recommend_sessions(hist, k=P, return_hidden=True, **kw)
    idx = g.itemidmap[pool_items.ravel()].values.reshape(pool_items.shape)
    rows = np.arange(len(hist))[:, None]
    for k, cap in kcaps:
        t = '%s P=%d k=%d cap=%d' % (tag, P, k, cap)
        pos, kept, _, want_scores = ref.apply_cap(idx, pool_scores, g.item_groups, k, cap)
        pad = pos < 0
        ids, scores, n_kept, H = g.recommend_sessions(hist, k=k, max_per_group=cap, pool=P, return_hidden=True, **kw)
        assert ids.shape == scores.shape == (len(hist), k) and scores.dtype == np.float32 and n_kept.dtype == np.int32
        np.testing.assert_array_equal(n_kept, kept, err_msg=t)
        np.testing.assert_array_equal(ids[~pad], pool_items[rows, np.maximum(pos, 0)][~pad], err_msg=t)
        np.testing.assert_array_equal(bits(scores)[~pad], bits(want_scores)[~pad], err_msg=t)
        assert np.isnan(scores[pad]).all(), t
        for a, b in zip(H, H0):
            np.testing.assert_array_equal(bits(a), bits(b), err_msg=t)
        # the entry itself: the pool positions and the pads
        hid = {x: kw[x] for x in kw if x != 'return_hidden'}
        cols, sc2, pos2, kept2 = native_capped(g, hist, P, k, cap, **hid)
        np.testing.assert_array_equal(pos2, pos, err_msg=t)
        np.testing.assert_array_equal(kept2, kept, err_msg=t)
        assert (cols[pad] == -1).all(), t
        np.testing.assert_array_equal(bits(sc2), bits(scores), err_msg=t)
        if cap >= P:      # nothing can be dropped: recommend_sessions(k) itself
            ri, rs = g.recommend_sessions(hist, k=k, **kw)
            np.testing.assert_array_equal(ids, ri, err_msg=t)
            np.testing.assert_array_equal(bits(scores), bits(rs), err_msg=t)
            assert (n_kept == k).all(), t
        # without the hidden state: the same first three
        out = g.recommend_sessions(hist, k=k, max_per_group=cap, pool=P, **kw)
        assert len(out) == 3
        np.testing.assert_array_equal(out[0][~pad], ids[~pad])
        np.testing.assert_array_equal(bits(out[1]), bits(scores))
        np.testing.assert_array_equal(out[2], n_kept)
    return kept


def kcaps_of(P):
    return [(k, cap) for k in sorted({1, P, min(20, P)}) for cap in sorted({1, 2, 3, P})]


# ---- 1. capped lists against the host loop --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('P', POOLS, ids=['P%d' % p for p in POOLS])
def test_capped_lists_equal_the_host_loop(P):
    g = fitted('3000x100')
    check_capped(g, histories(g, 5, seed=P), P, kcaps_of(P), 'exact')
    if P <= 128:
        check_capped(fitted('300x36'), histories(fitted('300x36'), 3, seed=P + 1), P, kcaps_of(P), '300x36')


def test_all_ungrouped_and_one_group():
    g = fitted('3000x100')
    hist = histories(g, 4, seed=3)
    try:
        set_groups(g, np.full(g.n_items, -1))
        for P in (64, 130):
            kept = check_capped(g, hist, P, [(P, 1), (20, 2)], 'ungrouped')
            assert (kept == 20).all()
        set_groups(g, np.zeros(g.n_items, dtype=np.int64))
        for P in (64, 130):
            for cap in (1, 3, 70):
                kept = check_capped(g, hist, P, [(P, cap)], 'one group')
                assert (kept == min(cap, P)).all()      # n_kept == cap
    finally:
        set_groups(g, fixture_groups(g.n_items))


def test_chunks_and_both_branches_of_the_walk(monkeypatch):
    """N = 700 in chunks of 64 rows, histories of mixed length (the chunk's permutation matters).  A condition on the inputs: with cap 2,
    k 20 and pool 64 the oracle holds rows that fill their list and rows that do not."""
    g = fitted('3000x100')
    monkeypatch.setenv('G4R_SESSIONS_CHUNK', '64')
    kept = check_capped(g, histories(g, 700, seed=7, longest=12), 64, [(20, 2)], 'N=700')
    assert (kept < 20).any() and (kept == 20).any(), np.bincount(kept)


def test_filters_candidates_scan_and_hidden():
    g = fitted('3000x100')
    ids = g.itemidmap.index.values
    rng = np.random.RandomState(13)
    hist = histories(g, 40, seed=12)
    per_row = [ids[rng.randint(0, len(ids), size=rng.randint(0, 30))] for _ in hist]
    kc = [(20, 2), (65, 1)]
    check_capped(g, hist, 65, kc, 'filters', exclude_history=True, exclude=ids[:200], exclude_per_row=per_row, exclude_groups=['G3'])
    # exclude_groups alone: no item of the group comes back, and it equals the equivalent exclude=
    gi = g.group_labels.tolist().index('G3')
    members = ids[g.item_groups == gi]
    a = g.recommend_sessions(hist, k=20, max_per_group=2, pool=65, exclude_groups=['G3'])
    b = g.recommend_sessions(hist, k=20, max_per_group=2, pool=65, exclude=members)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)
    assert not np.isin(a[0][~np.isnan(a[1])], members).any()
    a = g.recommend_sessions(hist, k=20, exclude_groups=['G3', 'G1'])
    b = g.recommend_sessions(hist, k=20, exclude=ids[np.isin(g.item_groups, [gi, g.group_labels.tolist().index('G1')])])
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(bits(a[1]), bits(b[1]))
    # candidates with duplicates: every position is one
    sub = ids[rng.randint(0, len(ids), size=500)]
    assert len(np.unique(sub)) < len(sub)
    check_capped(g, hist, 130, [(20, 2), (130, 3)], 'candidates', predict_for_item_ids=sub, exclude_history=True)
    # the two-stage selection
    check_capped(g, hist, 128, [(20, 2), (128, 1)], 'bf16', scan='bf16', oversample=8)
    check_capped(g, hist, 64, [(20, 2)], 'bf16 list', scan='bf16', oversample=4, predict_for_item_ids=sub)
    # capped(a + b) == capped(b, hidden = the state after a)
    a, b = histories(g, 40, seed=14), histories(g, 40, seed=15)
    kw = dict(k=20, max_per_group=2, pool=100, return_hidden=True)
    whole = g.recommend_sessions([np.concatenate(x) for x in zip(a, b)], **kw)
    Ha = g.recommend_sessions(a, **kw)[3]
    rest = g.recommend_sessions(b, hidden=Ha, **kw)
    live = ~np.isnan(whole[1])
    np.testing.assert_array_equal(whole[0][live], rest[0][live])
    np.testing.assert_array_equal(bits(whole[1]), bits(rest[1]))
    np.testing.assert_array_equal(whole[2], rest[2])
    for x, y in zip(whole[3], rest[3]):
        np.testing.assert_array_equal(bits(x), bits(y))
    check_capped(g, b, 65, [(20, 2)], 'hidden in', hidden=Ha)


def test_softmax_model():
    g = fitted('300x36-softmax')
    hist = histories(g, 6, seed=21)
    check_capped(g, hist, 65, [(20, 2), (65, 1)], 'softmax')
    check_continuation(g, hist, 2, 5, 65, 1, True, False, 'softmax')


# ---- 2. the continuation against the host loop ------------------------------------------------------------------------------------------
def host_continue(g, hist, steps, k, P, cap, no_repeat, count_history, exclude_per_row=None, priors=None, **kw):
    """The loop continue_sessions(max_per_group=) replaces: (ids[N, steps, k] -- -1 in the pads --, scores, n_kept[N, steps], hidden)."""
    N, G = len(hist), g.item_groups
    prior = [[] for _ in hist] if priors is None else [list(p) for p in priors]
    if count_history:
        for i, h in enumerate(hist):
            gh = G[g.itemidmap[np.asarray(h)].values]
            prior[i] += gh[gh >= 0].tolist()
    per_row = [list(x) for x in exclude_per_row] if exclude_per_row is not None else [[] for _ in hist]
    if no_repeat:
        per_row = [p + list(h) for p, h in zip(per_row, hist)]
    ids = np.full((N, steps, k), -1, dtype=np.int64)
    scores = np.full((N, steps, k), np.nan, dtype=np.float32)
    kept = np.zeros((N, steps), dtype=np.int32)
    cur, H = hist, kw.pop('hidden', None)
    for s in range(steps):
        pool_items, pool_scores, H = g.recommend_sessions(cur, k=P, hidden=H, return_hidden=True,
                                                          exclude_per_row=per_row if any(len(p) for p in per_row) else None, **kw)
        idx = g.itemidmap[pool_items.ravel()].values.reshape(pool_items.shape)
        nxt = []
        for i in range(N):
            pos, n = ref.cap_rule(G[idx[i]], k, cap, prior[i])
            kept[i, s] = n
            if n == 0:      # the fallback winner: list position 0
                pos[0], n = 0, 1
            ids[i, s, :n] = pool_items[i, pos[:n]]
            scores[i, s, :n] = pool_scores[i, pos[:n]]
            w = pool_items[i, pos[0]]
            if G[idx[i, pos[0]]] >= 0:
                prior[i].append(int(G[idx[i, pos[0]]]))
            if no_repeat:
                per_row[i].append(w)
            nxt.append([w])
        cur = nxt
    return ids, scores, kept, H


def check_continuation(g, hist, steps, k, P, cap, no_repeat, count_history, tag, **kw):
    t = '%s steps=%d k=%d P=%d cap=%d no_repeat=%d count_history=%d' % (tag, steps, k, P, cap, no_repeat, count_history)
    want = host_continue(g, hist, steps, k, P, cap, no_repeat, count_history, **dict(kw))
    got = g.continue_sessions(hist, steps, k=k, no_repeat=no_repeat, max_per_group=cap, pool=P, count_history=count_history,
                              return_hidden=True, **kw)
    assert got[0].shape == got[1].shape == (len(hist), steps, k) and got[2].shape == (len(hist), steps) and got[2].dtype == np.int32
    np.testing.assert_array_equal(got[2], want[2], err_msg=t)
    live = want[0] >= 0
    np.testing.assert_array_equal(got[0][live], want[0][live], err_msg=t)
    np.testing.assert_array_equal(bits(got[1])[live], bits(want[1])[live], err_msg=t)
    assert np.isnan(got[1][~live]).all(), t
    assert live[:, :, 0].all()      # a winner at every step, kept or fallback
    for a, b in zip(got[3], want[3]):
        np.testing.assert_array_equal(bits(a), bits(b), err_msg=t)
    short = g.continue_sessions(hist, steps, k=k, no_repeat=no_repeat, max_per_group=cap, pool=P, count_history=count_history, **kw)
    assert len(short) == 3
    np.testing.assert_array_equal(bits(short[1]), bits(got[1]))
    np.testing.assert_array_equal(short[2], got[2])
    return want


@pytest.mark.parametrize('P', (16, 80), ids=['P16', 'P80'])
@pytest.mark.parametrize('steps', (1, 2, 5), ids=['s1', 's2', 's5'])
def test_continuation_equals_the_host_loop(steps, P):
    g = fitted('3000x100')
    hist = histories(g, 9, seed=100 + steps)
    n_cfg = 0
    for no_repeat in (True, False):
        for count_history in (False, True):
            for k in (1, 5):
                check_continuation(g, hist, steps, k, P, 1 + n_cfg % 2, no_repeat, count_history, 'loop')
                n_cfg += 1
    check_continuation(g, hist, steps, P, P, 2, True, True, 'k = P')      # the whole pool leaves: every wave's positions are seen


def test_continuation_fallback_filters_scan_and_chunks(monkeypatch):
    g = fitted('3000x100')
    ids = g.itemidmap.index.values
    hist = histories(g, 7, seed=31)
    try:
        # every item in one group, cap 1: step 0 keeps one position, every later step keeps none and feeds list position 0
        set_groups(g, np.zeros(g.n_items, dtype=np.int64))
        for k in (1, 5):
            want = check_continuation(g, hist, 3, k, 70, 1, True, False, 'fallback')
            assert (want[2][:, 0] == 1).all() and (want[2][:, 1:] == 0).all()
        want = check_continuation(g, hist, 3, 5, 70, 1, False, True, 'fallback from step 0')      # the history fills the group
        assert (want[2] == 0).all()
    finally:
        set_groups(g, fixture_groups(g.n_items))
    rng = np.random.RandomState(32)
    per_row = [ids[rng.randint(0, len(ids), size=rng.randint(0, 20))] for _ in hist]
    check_continuation(g, hist, 3, 5, 65, 1, True, True, 'filters', exclude=ids[:100], exclude_per_row=per_row, exclude_groups=['G2'])
    sub = ids[rng.permutation(len(ids))[:400]]
    check_continuation(g, hist, 3, 5, 65, 2, True, False, 'candidates', predict_for_item_ids=sub)
    check_continuation(g, hist, 3, 5, 64, 1, True, True, 'bf16', scan='bf16', oversample=8)
    H = g.recommend_sessions(histories(g, 7, seed=33), k=1, return_hidden=True)[2]
    check_continuation(g, hist, 2, 5, 65, 1, True, False, 'hidden in', hidden=H)
    monkeypatch.setenv('G4R_SESSIONS_CHUNK', '64')
    check_continuation(g, histories(g, 150, seed=34, longest=12), 3, 5, 65, 1, True, True, 'chunks')


@pytest.mark.parametrize('n_prior', (0, 1, 64, 65, 1024))
def test_prior_lists_of_every_length(n_prior):
    """The entry's own prior lists (one step: the prior may be G4R_GROUP_PRIOR_MAX long), one of them filling a group."""
    g = fitted('3000x100')
    m = g._ensure_model()
    hist = histories(g, 6, seed=41, longest=9)
    N, lens, offs, hidx, _ = g._session_inputs(hist, None)
    rng = np.random.RandomState(n_prior)
    priors = [rng.randint(0, 5, size=n_prior) for _ in hist]
    if n_prior:
        priors[0][:] = 3      # fills group 3 for every cap <= n_prior
        priors[1] = np.zeros(0, dtype=np.int64)      # lists of different lengths in one call
    po = np.concatenate([[0], np.cumsum([len(p) for p in priors])]).astype(np.int64)
    pg = np.concatenate(priors).astype(np.int32)
    P, k = 80, 20
    pool_items, pool_scores = g.recommend_sessions(hist, k=P)
    idx = g.itemidmap[pool_items.ravel()].values.reshape(pool_items.shape)
    for cap in (1, 2, 14):
        pos, kept, _, want_scores = ref.apply_cap(idx, pool_scores, g.item_groups, k, cap, priors)
        cols, scores, n_kept = m.continue_sessions_capped(offs, hidx, None, k, P, cap, 1, False, prior_offs=po, prior_groups=pg)
        live = pos >= 0
        live[:, 0] |= kept == 0
        np.testing.assert_array_equal(n_kept[:, 0], kept)
        np.testing.assert_array_equal(cols[:, 0][live], idx[np.arange(N)[:, None], np.maximum(pos, 0)][live])
        np.testing.assert_array_equal(bits(scores[:, 0])[live], bits(pool_scores[np.arange(N)[:, None], np.maximum(pos, 0)])[live])
        assert (cols[:, 0][~live] == -1).all() and np.isnan(scores[:, 0][~live]).all()
        if n_prior >= cap and kept[0]:      # row 0's prior fills group 3: none of it comes back
            assert not (g.item_groups[cols[0, 0][live[0]]] == 3).any()


# ---- 3. supplied lists ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('P', POOLS, ids=['P%d' % p for p in POOLS])
def test_cap_lists_equal_the_rule(P):
    g = fitted('300x36')
    ids = g.itemidmap.index.values
    rng = np.random.RandomState(P)
    N = 9
    idx = rng.randint(0, 60, size=(N, P))      # 60 items in up to 256 positions: duplicates
    assert P < 65 or len(np.unique(idx[0])) < P
    for n_prior in (0, 1, 64, 65, 1024):
        prior_idx = [rng.randint(0, 300, size=n_prior) for _ in range(N)]
        if n_prior:
            prior_idx[0][:] = 3      # one item, n_prior times: its group is full for every cap below
        priors = [g.item_groups[p][g.item_groups[p] >= 0] for p in prior_idx]
        for k in sorted({1, P, min(20, P)}):
            for cap in sorted({1, 2, 3, P}):
                pos, n_kept = g.cap_lists(ids[idx], k, cap, prior=[ids[p] for p in prior_idx] if n_prior else None)
                assert pos.dtype == np.int32 and pos.shape == (N, k) and n_kept.shape == (N,)
                for i in range(N):
                    want_pos, want_n = ref.cap_rule(g.item_groups[idx[i]], k, cap, priors[i])
                    np.testing.assert_array_equal(pos[i], want_pos, err_msg='P=%d k=%d cap=%d prior=%d row %d' % (P, k, cap, n_prior, i))
                    assert n_kept[i] == want_n
    # more rows than a chunk holds
    big = rng.randint(0, 300, size=(4100, P))
    pos, n_kept = g.cap_lists(ids[big], min(20, P), 2)
    for i in (0, 4095, 4096, 4099):
        want_pos, want_n = ref.cap_rule(g.item_groups[big[i]], min(20, P), 2)
        np.testing.assert_array_equal(pos[i], want_pos)
        assert n_kept[i] == want_n


# ---- 4. the C entries -------------------------------------------------------------------------------------------------------------------
def test_c_entries_refuse_before_any_launch():
    g = fitted('3000x100')
    m = g._ensure_model()
    np.testing.assert_array_equal(m.get_item_groups(), g.item_groups)
    offs, hi = np.array([0, 2], dtype=np.int64), np.array([1, 2], dtype=np.int32)
    before = m.get_debug('continue_steps', 2).copy()
    ok = dict(hist_offs=offs, hist_items=hi, k=3, pool=10, cap=1)
    for bad, msg in ((dict(cap=0), 'cap must be'), (dict(pool=257), 'G4R_TOPK_MAX'), (dict(pool=0), 'G4R_TOPK_MAX'), (dict(k=11), 'k must be'),
                     (dict(k=0), 'k must be'), (dict(pool=100, oversample=11), 'oversample'),
                     (dict(item_idx=np.arange(5, dtype=np.int32)), 'k exceeds the number of candidates'),
                     (dict(excl_mask=np.full((3000 + 31) // 32, 0xFFFFFFFF, dtype=np.uint32)), 'eligible')):
        with pytest.raises(_native.NativeError, match=msg):
            m.recommend_sessions_capped(**dict(ok, **bad))
        with pytest.raises(_native.NativeError, match=msg):
            m.continue_sessions_capped(steps=2, **dict(ok, **bad))
    one = np.array([0, 1], dtype=np.int64)
    for bad, msg in ((dict(prior_offs=one, prior_groups=np.array([5], dtype=np.int32)), 'prior group out of range in row 0'),
                     (dict(prior_offs=one, prior_groups=np.array([-1], dtype=np.int32)), 'prior group out of range'),
                     (dict(prior_offs=np.array([0, 1024], dtype=np.int64), prior_groups=np.zeros(1024, dtype=np.int32)), 'G4R_GROUP_PRIOR_MAX'),
                     (dict(steps=1026, no_repeat=False), 'G4R_GROUP_PRIOR_MAX'), (dict(steps=0), 'steps must be')):
        with pytest.raises((_native.NativeError, ValueError), match=msg):
            m.continue_sessions_capped(**dict(dict(ok, steps=2), **bad))
    lists = np.zeros((1, 4), dtype=np.int32)
    for bad, msg in ((dict(items=np.full((1, 4), 3000, dtype=np.int32)), 'item index out of range'), (dict(k=5), 'k must be'), (dict(cap=0), 'cap must be'),
                     (dict(items=np.zeros((1, 257), dtype=np.int32)), 'G4R_TOPK_MAX'),
                     (dict(prior_offs=one, prior_groups=np.array([7], dtype=np.int32)), 'prior group out of range'),
                     (dict(prior_offs=np.array([0, 1025], dtype=np.int64), prior_groups=np.zeros(1025, dtype=np.int32)), 'G4R_GROUP_PRIOR_MAX')):
        with pytest.raises(_native.NativeError, match=msg):
            m.cap_lists(**dict(dict(items=lists, k=2, cap=1), **bad))
    np.testing.assert_array_equal(m.get_debug('continue_steps', 2), before)      # no call got as far as its first launch
    # the table: its checks, clearing it, setting it again
    with pytest.raises(_native.NativeError, match='n_items = 3000'):
        m.set_item_groups(np.zeros(10, dtype=np.int32))
    with pytest.raises(_native.NativeError, match='below -1'):
        m.set_item_groups(np.full(3000, -2, dtype=np.int32))
    np.testing.assert_array_equal(m.get_item_groups(), g.item_groups)
    m.set_item_groups(None)
    for call in (lambda: m.recommend_sessions_capped(**ok), lambda: m.continue_sessions_capped(steps=2, **ok), lambda: m.cap_lists(lists, 2, 1),
                 lambda: m.get_item_groups()):
        with pytest.raises(_native.NativeError, match='no item groups are set'):
            call()
    m.set_item_groups(g.item_groups)
    assert m.recommend_sessions_capped(**ok)[3].shape == (1,)


def test_groups_follow_the_model_and_the_uncapped_calls_are_untouched():
    g = fitted('300x36')
    ids = g.itemidmap.index.values
    hist = histories(g, 12, seed=51)
    # a new device model gets the table (close() drops the old one)
    first = g.recommend_sessions(hist, k=10, max_per_group=1, pool=40)
    g.close()
    again = g.recommend_sessions(hist, k=10, max_per_group=1, pool=40)
    np.testing.assert_array_equal(g._ensure_model().get_item_groups(), g.item_groups)
    for x, y in zip(first[1:], again[1:]):
        np.testing.assert_array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)
    # without max_per_group: what the untouched entries return
    m = g._ensure_model()
    N, lens, offs, hidx, _ = g._session_inputs(hist, None)
    cols, scores = m.recommend_sessions(offs, hidx, None, 20)
    out = g.recommend_sessions(hist, k=20)
    assert len(out) == 2
    np.testing.assert_array_equal(out[0], ids[cols])
    np.testing.assert_array_equal(bits(out[1]), bits(scores))
    xo = np.concatenate([[0], np.cumsum([len(np.unique(h)) for h in hist])]).astype(np.int64)
    xi = np.concatenate([np.unique(g.itemidmap[h].values) for h in hist]).astype(np.int32)
    cols, scores = m.continue_sessions(offs, hidx, None, 5, 3, True, xo, xi)
    out = g.continue_sessions(hist, 3, k=5)
    assert len(out) == 2
    np.testing.assert_array_equal(out[0], ids[cols])
    np.testing.assert_array_equal(bits(out[1]), bits(scores))

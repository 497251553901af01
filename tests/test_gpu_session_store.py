"""GRU4Rec.open_session_store / g4r_store_* against the stateless path, which is existing, tested code: whatever way a session's
events are split over push calls, whatever company they keep and whichever slot they land in, what a push returns equals
recommend_sessions of the session's events so far -- ids equal, scores and hidden states equal bit for bit -- and the seen lists
equal the rule "the first seen_cap distinct items in event order, held sorted" computed on the host."""
import numpy as np
import pandas as pd
import pytest

from gru4rec_amd.gru4rec import GRU4Rec

pytestmark = pytest.mark.gpu

N_ITEMS = 600
_MODELS = {}


def train_data(seed):
    rng = np.random.RandomState(seed)
    items = 10 + 3 * np.concatenate([rng.permutation(N_ITEMS), rng.randint(0, N_ITEMS, size=N_ITEMS)])
    sess = np.repeat(np.arange(len(items) // 5), 5)
    return pd.DataFrame({'SessionId': sess, 'ItemId': items[:len(sess)], 'Time': np.arange(len(sess), dtype=np.int64)})


def fitted(final_act='linear', layers=(100,), cache=True):
    """A GRU4Rec fitted for one epoch on synthetic sessions that hold every one of N_ITEMS items (ids 10, 13, 16, ...)."""
    key = (final_act, tuple(layers))
    if cache and key in _MODELS:
        return _MODELS[key]
    sm = final_act.startswith('softmax')
    g = GRU4Rec(layers=list(layers), final_act=final_act, loss='cross-entropy' if sm else 'bpr-max', n_epochs=1, batch_size=32,
                n_sample=0 if sm else 64, learning_rate=0.05)
    g.fit(train_data(sum(layers) + len(final_act)), sample_store=0 if sm else 100000)
    assert g.n_items == N_ITEMS
    if cache:
        _MODELS[key] = g
    return g


@pytest.fixture
def opened():
    """open_session_store that closes whatever the test left open (one store per device model)."""
    stores = []

    def op(g, capacity, seen_cap=64):
        for st in stores:
            st.close()
        stores.append(g.open_session_store(capacity, seen_cap))
        return stores[-1]
    yield op
    for st in stores:
        st.close()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_bits(a, b):
    assert np.shape(a) == np.shape(b)
    np.testing.assert_array_equal(bits(a), bits(b))


def make_sessions(g, n, seed, lo=1, hi=12):
    rng = np.random.RandomState(seed)
    ids = g.itemidmap.index.values
    return {s: ids[rng.randint(0, len(ids), size=rng.randint(lo, hi + 1))] for s in range(n)}


def make_calls(sessions, rows_plan, seed):
    """Cuts the sessions' events into calls: call c names rows_plan[c] sessions (then 1..40 until every event is out), 1 to 3 events of
    each, the sessions' events interleaved at random with every session's own order kept.  -> list of (session ids, item ids)."""
    rng = np.random.RandomState(seed)
    at = {s: 0 for s in sessions}
    calls = []
    while True:
        left = [s for s in sessions if at[s] < len(sessions[s])]
        if not left:
            return calls
        want = rows_plan[len(calls)] if len(calls) < len(rows_plan) else rng.randint(1, 41)
        pick = rng.permutation(left)[:want]
        take = {s: min(len(sessions[s]) - at[s], rng.randint(1, 4)) for s in pick}
        order = rng.permutation(np.repeat(pick, [take[s] for s in pick]))
        items = []
        for s in order:
            items.append(sessions[s][at[s]])
            at[s] += 1
        calls.append((order.tolist(), np.array(items)))


def first_appearance(sids):
    return list(dict.fromkeys(sids))


def check_call(g, st, seen, sids, items, k, exclude_seen, **kw):
    """One push, checked against recommend_sessions of every row's events so far (seen: session -> list of item ids, updated)."""
    rows, got_items, got_scores, over = st.push(sids, items, k=k, exclude_seen=exclude_seen, **kw)
    assert rows == first_appearance(sids)
    for s, i in zip(sids, items):
        seen.setdefault(s, []).append(i)
    want = g.recommend_sessions([seen[s] for s in rows], k=k, exclude_history=exclude_seen, return_hidden=True, **kw)
    np.testing.assert_array_equal(got_items, want[0])
    assert_bits(got_scores, want[1])
    assert not over.any()
    ex = st.export(rows)
    assert list(ex['session_ids']) == rows
    for h, w in zip(ex['hidden'], want[2]):
        assert_bits(h, w)
    return got_items, got_scores


CONFIGS = {'linear_100_fp32': ('linear', (100,), dict()), 'linear_100_bf16': ('linear', (100,), dict(scan='bf16', oversample=8)),
           'softmax_48_20': ('softmax', (48, 20), dict()), 'elu_50_unaligned': ('elu-0.5', (50,), dict())}


@pytest.mark.parametrize('name', list(CONFIGS))
def test_any_split_equals_the_whole(opened, name):
    final_act, layers, kw = CONFIGS[name]
    g = fitted(final_act, layers)
    sessions = make_sessions(g, 100, seed=3)
    calls = make_calls(sessions, [1, 64, 65, 7], seed=4)
    assert [len(set(c[0])) for c in calls[:3]] == [1, 64, 65]
    assert any(len(c[0]) > len(set(c[0])) for c in calls)      # several events of one session inside one call
    st = opened(g, 128)
    seen = {}
    for c, (sids, items) in enumerate(calls):
        check_call(g, st, seen, sids, items, 10, exclude_seen=(c % 2 == 0), **kw)
    assert len(st) == 100 and all(len(seen[s]) == len(sessions[s]) for s in sessions)


def test_company_chunking_and_slot_order_do_not_matter(opened, monkeypatch):
    g = fitted()
    sessions = make_sessions(g, 12, seed=5)
    calls = make_calls(sessions, [5, 12, 3], seed=6)
    st = opened(g, 64)
    ref = [st.push(sids, items, k=10, exclude_seen=True) for sids, items in calls]
    slots_ref = dict(st._map.slot)
    # again: smaller chunks, unrelated sessions in every call, and other slots (unrelated sessions come and go first)
    monkeypatch.setenv('G4R_SESSIONS_CHUNK', '3')
    st = opened(g, 64)
    ids = g.itemidmap.index.values
    st.push(['u%d' % i for i in range(9)], ids[:9])
    st.end(['u1', 'u4', 'u6'])
    rng = np.random.RandomState(7)
    for (sids, items), (rows, ritems, rscores, _) in zip(calls, ref):
        extra = ['x%d' % i for i in rng.randint(0, 6, size=7)]
        pos = np.sort(rng.randint(0, len(sids) + 1, size=7))
        got = st.push(np.insert(np.array(sids, dtype=object), pos, extra).tolist(), np.insert(items, pos, ids[rng.randint(0, N_ITEMS, size=7)]),
                      k=10, exclude_seen=True)
        at = [got[0].index(s) for s in rows]
        np.testing.assert_array_equal(got[1][at], ritems)
        assert_bits(got[2][at], rscores)
    assert any(st._map.slot[s] != slots_ref[s] for s in sessions)
    a = st.export(list(sessions))
    monkeypatch.delenv('G4R_SESSIONS_CHUNK')
    want = g.recommend_sessions([sessions[s] for s in sessions], k=10, return_hidden=True)
    for h, w in zip(a['hidden'], want[2]):
        assert_bits(h, w)


def test_eviction_follows_the_rule_and_a_reused_slot_leaks_nothing(opened):
    g = fitted()
    ids = g.itemidmap.index.values
    st = opened(g, 8, seen_cap=16)
    rng = np.random.RandomState(8)
    touch, since, evictions = {}, {}, 0      # the host model: last touch (call, row) of every live session; its events since it came
    for c in range(30):
        sids = rng.choice(20, size=rng.randint(1, 5), replace=False).tolist()
        items = ids[rng.randint(0, N_ITEMS, size=len(sids))]
        short = sum(1 for s in sids if s not in touch) - (8 - len(touch))
        want_evicted = sorted((x for x in touch if x not in sids), key=touch.get)[:max(short, 0)]
        for v in want_evicted:
            del touch[v], since[v]
        evictions += len(want_evicted)
        for r, (s, i) in enumerate(zip(sids, items)):
            touch[s] = (c, r)
            since.setdefault(s, []).append(i)
        rows, got_items, got_scores, _ = st.push(sids, items, k=10, exclude_seen=True)
        assert st.pop_evicted() == want_evicted
        assert st.stats()['live'] == len(touch) == len(st) and st.stats()['evictions'] == evictions and st.stats()['capacity'] == 8
        assert all((s in st) == (s in touch) for s in range(20))
        want = g.recommend_sessions([since[s] for s in rows], k=10, exclude_history=True)      # only the events since it (re)entered
        np.testing.assert_array_equal(got_items, want[0])
        assert_bits(got_scores, want[1])
    assert evictions > 5 and st.stats()['device_bytes'] > 0
    # a reused slot: the previous occupant saw exactly the items the newcomer is about to be recommended
    st = opened(g, 1, seen_cap=16)
    hist = ids[[5, 17, 99]]
    want = g.recommend_sessions([hist], k=8, exclude_history=True, return_hidden=True)
    st.push(['old'] * 8, want[0][0])
    rows, got_items, got_scores, over = st.push(['new'] * 3, hist, k=8, exclude_seen=True)
    assert st.pop_evicted() == ['old'] and 'old' not in st and st._map.slot['new'] == 0
    np.testing.assert_array_equal(got_items, want[0])
    assert_bits(got_scores, want[1])
    assert_bits(st.export(['new'])['hidden'][0], want[2][0])
    assert sorted(st.export()['seen_items']) == sorted(hist) and not over.any()


def host_seen(events, cap, itemidmap):
    """The rule: the first `cap` distinct items in event order, sorted by item index; overflow when there are more."""
    first = list(dict.fromkeys(events))
    kept = sorted(first[:cap], key=lambda i: itemidmap[i])
    return kept, len(first) > cap


def test_seen_lists_follow_the_rule(opened):
    g = fitted()
    ids = g.itemidmap.index.values
    st = opened(g, 16, seen_cap=4)
    rng = np.random.RandomState(9)
    pools = {s: ids[rng.randint(0, N_ITEMS, size=2 + s)] for s in range(6)}      # 2 .. 7 distinct-ish items, drawn with repeats
    seen = {}
    for c in range(6):
        sids = rng.randint(0, 6, size=9).tolist()
        items = np.array([pools[s][rng.randint(0, len(pools[s]))] for s in sids])
        for s, i in zip(sids, items):
            seen.setdefault(s, []).append(i)
        rows, got_items, got_scores, over = st.push(sids, items, k=10, exclude_seen=True)
        lists = [host_seen(seen[s], 4, g.itemidmap) for s in rows]
        np.testing.assert_array_equal(over, [o for _, o in lists])
        ex = st.export(rows)
        for r in range(len(rows)):
            assert ex['seen_items'][ex['seen_offs'][r]:ex['seen_offs'][r + 1]].tolist() == lists[r][0]
        np.testing.assert_array_equal(ex['overflow'], over)
        want = g.recommend_sessions([seen[s] for s in rows], k=10, exclude_per_row=[l for l, _ in lists])
        np.testing.assert_array_equal(got_items, want[0])
        assert_bits(got_scores, want[1])
    assert any(host_seen(seen[s], 4, g.itemidmap)[1] for s in seen) and not all(host_seen(seen[s], 4, g.itemidmap)[1] for s in seen)
    assert any(len(seen[s]) > len(set(seen[s])) for s in seen)      # repeats were skipped


def test_a_long_list_crosses_the_run_of_64(opened):
    g = fitted()
    ids = g.itemidmap.index.values      # (in item index order)
    st = opened(g, 4, seen_cap=130)
    s = ids[1 + np.sort(np.random.RandomState(10).choice(N_ITEMS - 1, size=70, replace=False))]
    # 66 insertions at the end, one at the front under a tail of 66 (two runs), two at the end, one in the middle, then repeats
    order = np.concatenate([s[1:67], s[:1], s[68:70], s[67:68], s[30:33]])
    other = ids[[400, 3, 250, 3]]
    rows, got_items, got_scores, over = st.push(['long'] * len(order) + ['other'] * 4, np.concatenate([order, other]), k=10, exclude_seen=True)
    want = g.recommend_sessions([order, other], k=10, exclude_history=True)
    np.testing.assert_array_equal(got_items, want[0])
    assert_bits(got_scores, want[1])
    ex = st.export(['long', 'other'])
    assert ex['seen_offs'].tolist() == [0, 70, 73] and not over.any()
    assert ex['seen_items'][:70].tolist() == s.tolist() and ex['seen_items'][70:].tolist() == ids[[3, 250, 400]].tolist()
    # across calls: one more at the front, under a tail of 70
    low = ids[:1]
    st.push(['long'], low)
    assert sorted(st.export(['long'])['seen_items'].tolist()) == sorted(s.tolist() + low.tolist())


def same_export(a, b):
    assert list(a['session_ids']) == list(b['session_ids'])
    for x, y in zip(a['hidden'], b['hidden']):
        assert_bits(x, y)
    np.testing.assert_array_equal(a['seen_offs'], b['seen_offs'])
    np.testing.assert_array_equal(a['seen_items'], b['seen_items'])
    np.testing.assert_array_equal(a['overflow'], b['overflow'])


def test_recommend_equals_the_last_push_and_changes_nothing(opened):
    g = fitted('linear', (48, 20))
    sessions = make_sessions(g, 70, seed=11)
    st = opened(g, 80, seen_cap=8)
    last = {}
    for sids, items in make_calls(sessions, [70, 20], seed=12):
        rows, ri, rs, ro = st.push(sids, items, k=10, exclude_seen=True)
        for r, s in enumerate(rows):
            last[s] = (ri[r], rs[r], ro[r])
    before = st.export()
    order = list(before['session_ids'])
    who = list(np.random.RandomState(13).permutation(list(sessions)))
    gi, gs, go = st.recommend(who, k=10, exclude_seen=True)
    np.testing.assert_array_equal(gi, [last[s][0] for s in who])
    assert_bits(gs, np.array([last[s][1] for s in who]))
    np.testing.assert_array_equal(go, [last[s][2] for s in who])
    same_export(st.export(), before)
    assert list(st._map.slot) == order      # (no session was touched)
    with pytest.raises(KeyError):
        st.recommend(['nobody'], k=10)


def test_export_load_into_a_fresh_store(opened):
    g = fitted()
    sessions = make_sessions(g, 30, seed=14, lo=4)
    calls = make_calls(sessions, [30, 10], seed=15)
    half = len(calls) // 2
    st = opened(g, 32, seen_cap=6)
    for sids, items in calls[:half]:
        st.push(sids, items)
    saved = st.export()
    ref = [st.push(sids, items, k=10, exclude_seen=True) for sids, items in calls[half:]]
    end = st.export(list(sessions))
    st.close()
    with pytest.raises(RuntimeError):
        st.push([0], g.itemidmap.index.values[:1])
    st = opened(g, 40, seen_cap=6)
    st.load(saved)
    same_export(st.export(), saved)
    for (sids, items), want in zip(calls[half:], ref):
        got = st.push(sids, items, k=10, exclude_seen=True)
        assert got[0] == want[0]
        np.testing.assert_array_equal(got[1], want[1])
        assert_bits(got[2], want[2])
        np.testing.assert_array_equal(got[3], want[3])
    same_export(st.export(list(sessions)), end)


def test_interleaving_with_the_prediction_state_and_fit(opened):
    g = fitted('linear', (100,), cache=False)
    ids = g.itemidmap.index.values
    rng = np.random.RandomState(16)
    steps = [(np.arange(5), ids[rng.randint(0, N_ITEMS, size=5)]) for _ in range(4)]

    def predictions(between):
        g.predict = None
        out = []
        for t, (sid, inp) in enumerate(steps):
            out.append(g.predict_next_batch(sid, inp, batch=5).values if t % 2 == 0 else
                       g.recommend_next_batch(sid, inp, k=10, batch=5, exclude_seen=True))
            between(t)
        g.predict = None
        return out
    want = predictions(lambda t: None)
    st = opened(g, 8)
    seen = {}
    got = predictions(lambda t: check_call(g, st, seen, [t % 2, 7, t % 2], ids[rng.randint(0, N_ITEMS, size=3)], 10, True))
    for a, b in zip(got, want):
        if isinstance(a, tuple):
            np.testing.assert_array_equal(a[0], b[0])
            assert_bits(a[1], b[1])
        else:
            assert_bits(a, b)
    g.fit(train_data(1))
    for call in (lambda: st.push([1], ids[:1]), lambda: st.recommend([1], k=5), st.export, lambda: st.end([1]), lambda: st.load({})):
        with pytest.raises(RuntimeError):
            call()
    st2 = g.open_session_store(4)      # the new device model takes a new store
    with pytest.raises(RuntimeError):
        g.open_session_store(4)
    st2.close()
    g.close()


def test_refusals_change_nothing(opened):
    g = fitted()
    ids = g.itemidmap.index.values
    st = opened(g, 8, seen_cap=64)
    st.push([1, 2, 3, 1], ids[[4, 5, 6, 7]])
    before, order = st.export(), list(st._map.slot)
    with pytest.raises(KeyError):
        st.push([1, 9], [ids[0], -5], k=5)
    with pytest.raises(ValueError, match='conservative'):
        st.push([1, 9], ids[:2], k=10, exclude_seen=True, predict_for_item_ids=ids[:70])
    with pytest.raises(ValueError, match='capacity'):
        st.push(list(range(9)), ids[:9])
    with pytest.raises(ValueError):
        st.push([1], ids[:1], k=0)
    with pytest.raises(ValueError, match='duplicate-free'):
        st.push([1], ids[:1], k=2, exclude_seen=True, predict_for_item_ids=ids[[1, 2, 2, 3] + list(range(100, 200))])
    same_export(st.export(), before)
    assert list(st._map.slot) == order and len(st) == 3 and 9 not in st and st.pop_evicted() == []

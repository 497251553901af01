"""recommend_sessions(nprobe=) over an item index (g4r_ivf_assign / g4r_ivf_set / g4r_recommend_sessions_ivf).

What is approximate is WHICH items a row considers -- those of the nprobe lists whose centroids score best against its final hidden
state; the scores, the order and the tie rule never are.  So, for any input: every returned score is predict_next_batch's bit for bit,
the list is in the contract's order (score descending, equal scores by the lower item, NaN last), no item comes twice and no
excluded item comes at all.  A row's result is a function of its own history: not of the rows around it, the chunking or the work
items it was grouped into.  With nprobe = n_lists the result is scan='bf16''s with the same oversample, ids and bits; and over a
union of probed lists it is scan='bf16''s over exactly those items, which, when c covers the union, is the exact top k over it
(score_candidates_sessions).  The assignment and the probes are checked against the float64 rules of tests/ivf_ref.py."""
import numpy as np
import pandas as pd
import pytest

import ivf_ref
from gru4rec_amd import _native
from gru4rec_amd.gru4rec import GRU4Rec
from test_gpu_recommend import N_ITEMS, fitted

pytestmark = pytest.mark.gpu

SMALL_ITEMS = 1003      # not a multiple of 32
_SMALL = {}
_BUILT = {}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def small():
    """A model of 1,003 items and 36 units, fitted for one epoch."""
    if 'g' not in _SMALL:
        rng = np.random.RandomState(36)
        items = 10 + 3 * np.concatenate([rng.permutation(SMALL_ITEMS), rng.randint(0, SMALL_ITEMS, size=2 * SMALL_ITEMS)])
        sess = np.repeat(np.arange(len(items) // 3), 3)
        data = pd.DataFrame({'SessionId': sess, 'ItemId': items[:len(sess)], 'Time': np.arange(len(sess), dtype=np.int64)})
        g = GRU4Rec(layers=[36], final_act='linear', loss='bpr-max', n_epochs=1, batch_size=32, n_sample=64, learning_rate=0.05)
        g.fit(data, sample_store=10000)
        assert g.n_items == SMALL_ITEMS
        _SMALL['g'] = g
    return _SMALL['g']


MODELS = {'m64': (lambda: fitted('linear', 64), 64), 'm100': (lambda: fitted('linear', 100), 200), 'small': (small, 7)}


def built(name):
    """The model with a k-means index of the model's number of lists (built once; tests that install another index put it back)."""
    g = MODELS[name][0]()
    if name not in _BUILT:
        stats = g.build_item_index(n_lists=MODELS[name][1], iters=4, sample_per_list=32, seed=1)
        _BUILT[name] = (stats, g.item_index())
    elif g.item_index() is None or len(g.item_index()['list_offs']) - 1 != MODELS[name][1]:
        g.build_item_index(index=_BUILT[name][1])
    return g


def hists(g, lens, seed):
    rng = np.random.RandomState(seed)
    ids = g.itemidmap.index.values
    return [ids[rng.randint(0, len(ids), size=n)] for n in lens]


def exact_scores(g, hs):
    """predict_next_batch's scores after every history: [len(hs), n_items] float32, columns in itemidmap order."""
    S = np.empty((len(hs), g.n_items), dtype=np.float32)
    lens = np.array([len(h) for h in hs])
    for L in np.unique(lens):
        rows = np.flatnonzero(lens == L)
        g.predict = None
        for t in range(L):
            out = g.predict_next_batch(np.arange(len(rows)), np.array([hs[r][t] for r in rows]), batch=len(rows))
        S[rows] = out.values.T
    g.predict = None
    return S


def check_invariants(g, S, items, scores, found, k, excluded=None, universe=None):
    """S: exact_scores of the same histories.  universe[r]: the item indices row r may return (None: any)."""
    idx = g.itemidmap[items.ravel()].values.reshape(items.shape)
    assert items.shape == scores.shape == (len(S), k) and scores.dtype == np.float32 and found.dtype == np.int32
    for r in range(len(S)):
        n = found[r]
        assert 0 <= n <= k and np.isnan(scores[r, n:]).all()
        assert len(set(idx[r, :n])) == n, 'row %d: an item twice' % r
        np.testing.assert_array_equal(bits(scores[r, :n]), bits(S[r, idx[r, :n]]), 'row %d: not the predict_next_batch bits' % r)
        order = ivf_ref.topk_by_contract(scores[r, :n], idx[r, :n], n)
        np.testing.assert_array_equal(order, np.arange(n), 'row %d: not in the contract order' % r)
        if excluded is not None:
            assert not set(items[r, :n]) & set(excluded[r]), 'row %d: an excluded item' % r
        if universe is not None:
            assert set(idx[r, :n]) <= set(universe[r]), 'row %d: an item of a list that was not probed' % r


def lists_of(ix, g):
    """The index's lists as arrays of item INDICES."""
    idx = g.itemidmap[ix['list_items']].values
    return [idx[a:b] for a, b in zip(ix['list_offs'][:-1], ix['list_offs'][1:])]


# ---------------------------------------------------------------------------------------------- assignment and partition
@pytest.mark.parametrize('name', ['m64', 'm100', 'small'])
def test_assignment_and_partition(name):
    g = built(name)
    stats, ix = _BUILT[name]
    nl = MODELS[name][1]
    lists = lists_of(ix, g)
    assert stats['n_lists'] == nl == len(lists) and ix['centroids'].shape == (nl, g.layers[-1] + 1)
    allidx = np.concatenate(lists)
    np.testing.assert_array_equal(np.sort(allidx), np.arange(g.n_items))
    assert all((np.diff(l) > 0).all() for l in lists), 'a list is not ascending'
    lens = np.array([len(l) for l in lists])
    assert (stats['list_len_min'], stats['list_len_max'], stats['empty_lists']) == (lens.min(), lens.max(), (lens == 0).sum())
    assert all(stats[key] >= 0 for key in ('seconds_kmeans', 'seconds_assign', 'seconds_upload'))
    assigned = np.empty(g.n_items, dtype=np.int64)
    assigned[allidx] = np.repeat(np.arange(nl), lens)
    ok, amb = ivf_ref.check_assignment(ivf_ref.item_vectors(g.Wy, g.By), ix['centroids'], assigned)
    print('%s: lists %d, lengths %d / %.1f / %d, %d empty, ambiguous items %.5f; k-means %.2f s, assignment %.3f s, upload %.3f s'
          % (name, nl, lens.min(), lens.mean(), lens.max(), (lens == 0).sum(), amb, stats['seconds_kmeans'], stats['seconds_assign'],
             stats['seconds_upload']))
    assert amb <= 0.01, 'the inputs of this test leave too many items with more than one acceptable list'
    assert ok.all(), 'items assigned to a list that is not within 2 tau of the best: %s' % np.flatnonzero(~ok)[:10]
    # centroids= skips k-means and gives the same partition; the native assignment agrees with itself
    g.build_item_index(centroids=ix['centroids'])
    again = g.item_index()
    np.testing.assert_array_equal(again['list_offs'], ix['list_offs'])
    np.testing.assert_array_equal(again['list_items'], ix['list_items'])


# ---------------------------------------------------------------------------------------------- a hand-made partition
HAND_LENS = [0, 1, 31, 32, 33, 64, 65, 2500]


def hand_index(g, priority):
    """Lists of HAND_LENS items each (random items, ascending) and one list of the rest.  The centroids' weights are zero and their
    biases are `priority`: every row's centroid score is the bias itself, so every row probes the lists in the order of `priority`
    (equal values: the lower list first)."""
    rng = np.random.RandomState(7)
    perm = rng.permutation(g.n_items)
    offs = np.concatenate([[0], np.cumsum(HAND_LENS), [g.n_items]]).astype(np.int64)
    lists = [np.sort(perm[a:b]) for a, b in zip(offs[:-1], offs[1:])]
    cen = np.zeros((len(lists), g.layers[-1] + 1), dtype=np.float32)
    cen[:, -1] = priority
    ids = g.itemidmap.index.values
    return dict(centroids=cen, list_offs=offs, list_items=ids[np.concatenate(lists)]), lists


def union_reference(g, hs, union_idx, k, excluded_idx=None):
    """The exact top k of every row over the items union_idx minus the row's excluded ones: score_candidates_sessions over the
    candidates in ascending item index (its tie rule, the lower position, is then the lower item)."""
    ids = g.itemidmap.index.values
    cands = [ids[np.setdiff1d(union_idx, [] if excluded_idx is None else excluded_idx[r])] for r in range(len(hs))]
    assert min(len(c) for c in cands) >= k
    return g.score_candidates_sessions(hs, cands, k=k)


def test_hand_made_partition():
    g = fitted('linear', 64)
    ids = g.itemidmap.index.values
    hs = hists(g, [2, 1, 3, 1, 2] * 7, seed=11)      # 35 rows: two row groups on every probed list
    try:
        # the seven short lists, best first 65, 64, 33, 32, 31, 1, 0: c = 20 * 16 covers their 226 items
        ix, lists = hand_index(g, [1, 2, 3, 4, 5, 6, 7, 0, -1])
        g.build_item_index(index=ix)
        items, scores, found, probes = g.recommend_sessions(hs, k=20, oversample=16, nprobe=7, return_probes=True)
        np.testing.assert_array_equal(probes, np.tile([6, 5, 4, 3, 2, 1, 0], (len(hs), 1)))
        union = np.concatenate(lists[:7])
        assert len(union) == 226 <= 20 * 16 and (found == 20).all()
        w_items, w_scores = union_reference(g, hs, union, 20)
        np.testing.assert_array_equal(items, w_items)
        np.testing.assert_array_equal(bits(scores), bits(w_scores))
        # with exclusions: every row's history, one item everywhere, and the best item of the union per row
        top = [items[r, 0] for r in range(len(hs))]
        glob = ids[lists[4][:5]]
        items, scores, found = g.recommend_sessions(hs, k=20, oversample=16, nprobe=7, exclude_history=True, exclude=glob,
                                                    exclude_per_row=[[t] for t in top])
        excl_ids = [set(hs[r]) | set(glob) | {top[r]} for r in range(len(hs))]
        excl_idx = [g.itemidmap[list(e)].values for e in excl_ids]
        w_items, w_scores = union_reference(g, hs, union, 20, excl_idx)
        assert all(top[r] not in items[r] for r in range(len(hs))) and (found == 20).all()
        np.testing.assert_array_equal(items, w_items)
        np.testing.assert_array_equal(bits(scores), bits(w_scores))
        # equal biases: the lower list first.  Lists 0 (empty) and 1 (one item): the union is shorter than k
        ix, lists = hand_index(g, [5, 5, 0, 0, 0, 0, 0, 0, 0])
        g.build_item_index(index=ix)
        items, scores, found, probes = g.recommend_sessions(hs, k=20, nprobe=2, return_probes=True)
        np.testing.assert_array_equal(probes, np.tile([0, 1], (len(hs), 1)))
        only = ids[lists[1][0]]
        assert (found == 1).all() and (items[:, 0] == only).all() and np.isnan(scores[:, 1:]).all()
        S = exact_scores(g, hs)
        np.testing.assert_array_equal(bits(scores[:, 0]), bits(S[:, lists[1][0]]))
        items, scores, found = g.recommend_sessions(hs, k=20, nprobe=2, exclude=[only])
        assert (found == 0).all() and np.isnan(scores).all()
        per_row = [[only] if r % 2 else [] for r in range(len(hs))]
        items, scores, found = g.recommend_sessions(hs, k=20, nprobe=2, exclude_per_row=per_row)
        np.testing.assert_array_equal(found, [0 if r % 2 else 1 for r in range(len(hs))])
        # the list of 2,500 (several merges of the survivor queues) and the one of 33: the bf16 scan over exactly those items
        ix, lists = hand_index(g, [0, 0, 0, 0, 3, 0, 0, 9, 0])
        g.build_item_index(index=ix)
        for nprobe, over in ((1, 8), (2, 1), (2, 8)):
            items, scores, found, probes = g.recommend_sessions(hs, k=20, oversample=over, nprobe=nprobe, return_probes=True)
            np.testing.assert_array_equal(probes, np.tile([7, 4][:nprobe], (len(hs), 1)))
            union = np.sort(np.concatenate([lists[7], lists[4]][:nprobe]))
            w_items, w_scores = g.recommend_sessions(hs, k=20, predict_for_item_ids=ids[union], scan='bf16', oversample=over)
            assert (found == 20).all()
            np.testing.assert_array_equal(items, w_items)
            np.testing.assert_array_equal(bits(scores), bits(w_scores))
            check_invariants(g, S, items, scores, found, 20, universe=[union] * len(hs))
    finally:
        g.drop_item_index()


# ---------------------------------------------------------------------------------------------- probes
@pytest.mark.parametrize('name, nprobe', [('m64', 8), ('m100', 16), ('small', 3), ('small', 7)])
def test_probes_follow_the_rule(name, nprobe):
    g = built(name)
    hs = hists(g, [1, 2, 3, 4, 5] * 26, seed=3)
    out = g.recommend_sessions(hs, k=5, nprobe=nprobe, return_hidden=True, return_probes=True)
    H, probes = out[3][-1], out[4]
    assert probes.shape == (len(hs), nprobe) and probes.dtype == np.int32
    s, tau = ivf_ref.probe_scores(H, _BUILT[name][1]['centroids'])
    ok, amb = ivf_ref.check_probes(s, tau, probes)
    print('%s nprobe=%d: ambiguous (row, list) pairs %.5f' % (name, nprobe, amb))
    assert amb <= 0.01, 'the inputs of this test leave too many (row, list) pairs on the cut'
    assert ok.all(), 'rows whose probes break the rule: %s' % np.flatnonzero(~ok)[:10]


# ---------------------------------------------------------------------------------------------- nprobe = n_lists: the bf16 scan
# (k, oversample): scan='bf16' takes k * oversample <= 1024, so k = 256 goes with 1 and 4
@pytest.mark.parametrize('name', ['m64', 'm100', 'small'])
def test_all_lists_probed_equals_the_bf16_scan(name):
    g = built(name)
    nl = MODELS[name][1]
    hs = hists(g, [3, 1, 2] * 11, seed=5)
    for k, over in ((1, 1), (1, 8), (20, 1), (20, 8), (256, 1), (256, 4)):
        if nl * min(k * over, 1024) > _native.G4R_IVF_WS_MAX:
            with pytest.raises(ValueError, match='G4R_IVF_WS_MAX'):
                g.recommend_sessions(hs, k=k, oversample=over, nprobe=nl)
            continue
        items, scores, found = g.recommend_sessions(hs, k=k, oversample=over, nprobe=nl, exclude_history=True)
        w_items, w_scores = g.recommend_sessions(hs, k=k, scan='bf16', oversample=over, exclude_history=True)
        assert (found == k).all()
        np.testing.assert_array_equal(items, w_items, 'k=%d oversample=%d' % (k, over))
        np.testing.assert_array_equal(bits(scores), bits(w_scores), 'k=%d oversample=%d' % (k, over))


# ---------------------------------------------------------------------------------------------- row counts and company
@pytest.mark.parametrize('rows', [1, 33, 130])
def test_same_history_in_every_row(rows):
    """nprobe = 1 and one history: every row probes the same list (130 rows: five work items on it) and receives the same answer."""
    g = built('m64')
    h = hists(g, [3], seed=8)[0]
    items, scores, found, probes = g.recommend_sessions([h] * rows, k=20, nprobe=1, return_probes=True)
    assert (probes == probes[0]).all() and (found == found[0]).all()
    assert (items == items[0]).all() and (bits(scores) == bits(scores[0])).all()
    S = exact_scores(g, [h])
    check_invariants(g, np.repeat(S, rows, axis=0), items, scores, found, 20)


def test_distinct_histories_alone_in_company_and_in_small_chunks(monkeypatch):
    g = built('m100')
    hs = hists(g, list(np.random.RandomState(4).randint(1, 7, size=130)), seed=9)
    kw = dict(k=20, oversample=4, nprobe=5, exclude_history=True, return_probes=True)
    full = g.recommend_sessions(hs, **kw)
    S = exact_scores(g, hs)
    lists = lists_of(_BUILT['m100'][1], g)
    universe = [np.concatenate([lists[l] for l in full[3][r]]) for r in range(len(hs))]
    check_invariants(g, S, full[0], full[1], full[2], 20, excluded=hs, universe=universe)
    for sel in ([77], list(range(33)), list(range(129, -1, -1))):
        part = g.recommend_sessions([hs[i] for i in sel], **kw)
        for a, b in zip(part, full):
            np.testing.assert_array_equal(bits(a) if a.dtype == np.float32 else a, (bits(b) if b.dtype == np.float32 else b)[sel])
    monkeypatch.setenv('G4R_SESSIONS_CHUNK', '64')
    chunked = g.recommend_sessions(hs, **kw)
    for a, b in zip(chunked, full):
        np.testing.assert_array_equal(bits(a) if a.dtype == np.float32 else a, bits(b) if b.dtype == np.float32 else b)


def test_an_excluded_item_that_would_top_a_probed_list():
    g = built('m64')
    hs = hists(g, [2, 1, 3, 2] * 8, seed=12)
    items, scores, found = g.recommend_sessions(hs, k=10, nprobe=2)
    tops = [[items[r, 0], items[r, 1]] for r in range(len(hs))]
    items2, scores2, found2 = g.recommend_sessions(hs, k=10, nprobe=2, exclude_per_row=tops)
    S = exact_scores(g, hs)
    check_invariants(g, S, items2, scores2, found2, 10, excluded=tops)
    assert (found2 == 10).all()


# ---------------------------------------------------------------------------------------------- supersets
def test_more_probes_never_lose_a_list_or_an_exact_item():
    """A partition into runs of 100 consecutive items (centroid: the run's mean): c = 128 * 8 covers up to ten lists, so the result
    over the probes is the exact top k over them; the probes of 2 p lists hold those of p, and no row's overlap with the exact top k
    over the whole catalogue falls."""
    g = fitted('linear', 100)
    V = ivf_ref.item_vectors(g.Wy, g.By)
    nl = N_ITEMS // 100
    ix = dict(centroids=V.reshape(nl, 100, -1).mean(axis=1).astype(np.float32), list_offs=np.arange(0, N_ITEMS + 1, 100, dtype=np.int64),
              list_items=g.itemidmap.index.values)
    hs = hists(g, [1, 2, 3] * 11, seed=13)
    S = exact_scores(g, hs)
    k = 128
    exact = [set(ivf_ref.topk_by_contract(S[r], np.arange(N_ITEMS), k)) for r in range(len(hs))]
    try:
        g.build_item_index(index=ix)
        prev = None
        for p in (1, 2, 4, 8):
            items, scores, found, probes = g.recommend_sessions(hs, k=k, oversample=8, nprobe=p, return_probes=True)
            idx = g.itemidmap[items.ravel()].values.reshape(items.shape)
            assert p * 100 <= k * 8 and (found == min(k, p * 100)).all()
            over = np.array([len(exact[r] & set(idx[r, :found[r]])) for r in range(len(hs))])
            for r in range(len(hs)):
                union = np.concatenate([np.arange(100 * l, 100 * l + 100) for l in probes[r]])
                want = union[ivf_ref.topk_by_contract(S[r, union], union, found[r])]
                np.testing.assert_array_equal(idx[r, :found[r]], want)
            if prev is not None:
                assert all(set(prev[0][r]) <= set(probes[r]) for r in range(len(hs)))
                assert (over >= prev[1]).all()
            prev = (probes, over)
        print('overlap with the exact top %d at 8 of %d lists: mean %.3f' % (k, nl, prev[1].mean() / k))
    finally:
        g.drop_item_index()


# ---------------------------------------------------------------------------------------------- other behaviour
def test_hidden_states_as_in_the_exact_call():
    g = built('small')
    hs = hists(g, [4, 2, 6, 2, 3], seed=14)
    a, b = [h[:len(h) // 2] for h in hs], [h[len(h) // 2:] for h in hs]
    _, _, H_exact = g.recommend_sessions(a, k=5, return_hidden=True)
    items_a, scores_a, found_a, H = g.recommend_sessions(a, k=5, nprobe=7, return_hidden=True)
    for x, y in zip(H, H_exact):
        np.testing.assert_array_equal(bits(x), bits(y))
    joined = g.recommend_sessions([np.concatenate([x, y]) for x, y in zip(a, b)], k=5, nprobe=3)
    cont = g.recommend_sessions(b, k=5, nprobe=3, hidden=H)
    for x, y in zip(joined, cont):
        np.testing.assert_array_equal(bits(x) if x.dtype == np.float32 else x, bits(y) if y.dtype == np.float32 else y)


def test_tables_follow_the_weights_and_drop_frees_the_index():
    g = built('small')
    m = g._model
    hs = hists(g, [2, 3, 1], seed=15)
    before = g.recommend_sessions(hs, k=5, nprobe=7)
    nl, nblk, nbytes, valid, builds = m.ivf_info()
    lens = np.diff(_BUILT['small'][1]['list_offs'])
    assert nl == 7 and nblk == ((lens + 31) // 32).sum() and valid and nbytes >= nblk * 32 * 128 * 2
    By = np.asarray(g.By, dtype=np.float32).ravel().copy()
    best = g.itemidmap[before[0][:, 0]].values
    By2 = By.copy()
    By2[best] -= 100.0                         # the rows' best items sink: stale tables would keep returning them first
    try:
        m.set_param('By', By2)
        assert m.ivf_info()[3] is False
        after = g.recommend_sessions(hs, k=5, nprobe=7)
        assert m.ivf_info()[3:] == (True, builds + 1)
        w_items, w_scores = g.recommend_sessions(hs, k=5, scan='bf16', oversample=8)
        np.testing.assert_array_equal(after[0], w_items)
        np.testing.assert_array_equal(bits(after[1]), bits(w_scores))
        assert (after[0][:, 0] != before[0][:, 0]).all()
    finally:
        m.set_param('By', By)
    g.drop_item_index()
    assert m.ivf_info()[:4] == (0, 0, 0, False) and g.item_index() is None
    with pytest.raises(ValueError, match='build_item_index'):
        g.recommend_sessions(hs, k=5, nprobe=1)
    g.build_item_index(index=_BUILT['small'][1])
    again = g.recommend_sessions(hs, k=5, nprobe=7)
    np.testing.assert_array_equal(again[0], before[0])
    np.testing.assert_array_equal(bits(again[1]), bits(before[1]))
    g.close()                                  # a new device model receives the index of this object again
    again = g.recommend_sessions(hs, k=5, nprobe=7)
    np.testing.assert_array_equal(again[0], before[0])


def test_c_abi_refuses_bad_arguments():
    g = built('small')
    m = g._ensure_model()
    ix = g._item_index
    offs, items = np.array([0, 1, 3], dtype=np.int64), np.array([5, 6, 7], dtype=np.int32)
    ok = dict(k=5, oversample=8, nprobe=2)
    for kw, word in ((dict(ok, k=0), 'k must be'), (dict(ok, k=257), 'k must be'), (dict(ok, oversample=0), 'oversample'),
                     (dict(ok, nprobe=0), 'nprobe'), (dict(ok, nprobe=8), 'nprobe'), (dict(k=256, oversample=4, nprobe=7), None)):
        if word is None:
            m.recommend_sessions_ivf(offs, items, **kw)      # 7 * 1024 entries per row: within the limit
            continue
        with pytest.raises(_native.NativeError, match=word):
            m.recommend_sessions_ivf(offs, items, **kw)
    with pytest.raises(_native.NativeError, match='empty'):
        m.recommend_sessions_ivf(np.array([0, 0, 3], dtype=np.int64), items, **ok)
    with pytest.raises(_native.NativeError, match='out of range'):
        m.recommend_sessions_ivf(offs, np.array([5, 6, SMALL_ITEMS], dtype=np.int32), **ok)
    lib, null = _native.lib(), None
    assert lib.g4r_ivf_assign(m.h, null, 3, null) != 0 and b'null' in lib.g4r_last_error()
    assert lib.g4r_ivf_set(m.h, null, 3, null, null) != 0 and b'null' in lib.g4r_last_error()
    assert lib.g4r_recommend_sessions_ivf(m.h, null, null, 1, null, 5, 8, 1, null, null, null, null, null, null, null, null) != 0
    assert lib.g4r_ivf_release(None) != 0
    cen, lo, li = ix['centroids'], ix['list_offs'], ix['list_items']
    with pytest.raises(_native.NativeError, match='n_lists'):
        m.ivf_assign(np.zeros((0, 37), dtype=np.float32))
    with pytest.raises(_native.NativeError, match='finite'):
        m.ivf_assign(np.full((3, 37), np.nan, dtype=np.float32))
    twice = li.copy()
    twice[1] = twice[0]
    down = li.copy()
    a = lo[np.flatnonzero(np.diff(lo) >= 2)[0]]      # the first two items of a list that holds two, swapped
    down[a:a + 2] = li[a + 1], li[a]
    short = lo.copy()
    short[-1] -= 1
    for args, word in (((cen, lo, twice), 'twice'), ((cen, lo, down), 'ascending'), ((cen, short, li), 'list_offs'),
                       ((np.full_like(cen, np.inf), lo, li), 'finite')):
        with pytest.raises(_native.NativeError, match=word):
            m.ivf_set(*args)
    m.ivf_set(cen, lo, li)      # (a refused g4r_ivf_set leaves the index as it was; this one is the same index again)
    g2 = fitted('softmax', 64)
    m2 = g2._ensure_model()
    V = np.zeros((2, 65), dtype=np.float32)
    m2.ivf_set(V, np.array([0, 1, N_ITEMS], dtype=np.int64), np.arange(N_ITEMS, dtype=np.int32))
    try:
        with pytest.raises(_native.NativeError, match='softmax'):
            m2.recommend_sessions_ivf(offs, items, **ok)
    finally:
        m2.ivf_release()

"""GRU4Rec.similar_items / item_neighbors (g4r_similar_items) against fp64 NumPy on the downloaded item table.

Bounds (derived, not tuned).  u = 2^-24, D = the table's width, S(q, j) = sum_d |T[q, d] T[j, d]| (for cosine divided by |T_q| |T_j|
in fp64).  A dot product of D fp32 products accumulated in fp32 in ANY order is within gamma_D S <= (D + 2) u S of the exact value
(Higham, Accuracy and Stability, (3.5); the + 2 covers the second-order terms for every D used here, D u < 2^-13).  An inverse norm is
1 / sqrt(sum of D squares): the sum is within (D + 1) u relative, the square root halves that and adds u, the division adds u --
(D / 2 + 4) u relative with the second-order terms.  cosine = (dot * inv_q) * inv_j adds two inverse norms and two multiplications
to the dot term: (D + 2 + 2 (D / 2 + 4) + 2 + 4) u S = (2 D + 16) u S.
Selection, tie-tolerant: a returned item j either is one of the row's k best by fp64 score, or it displaced one of them, t, that the
device scored no higher: ref(j) + b(j) >= device(j) >= device(t) >= ref(t) - b(t) >= kth - b(t), so ref(j) >= kth - b(j) - max_t b(t):
the row's k-th best fp64 score minus twice the bound, the second one taken as the largest bound among the row's eligible pairs.
Every row of every call is checked."""
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

from gru4rec_amd import _native
from gru4rec_amd.gru4rec import GRU4Rec

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
_MODELS = {}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def train_some(g, steps):
    assert g.run_epoch(0, max_steps=steps) is not None
    g._download_weights()


def fitted(n_items, D, mode, steps=40):
    """A GRU4Rec trained for `steps` mini-batches on synthetic sessions that hold every one of n_items items (ids 10, 13, 16, ...).
    mode: 'constrained' / 'separate' (embedding = 64) / 'onehot'.  steps = 0 (and the catalogue of one item, which has no negatives
    to train on): no training, Wy is edited on the host instead."""
    key = (n_items, D, mode)
    if key not in _MODELS:
        rng = np.random.RandomState(D + n_items)
        n_ev = max(2 * n_items, 400)
        items = 10 + 3 * np.concatenate([rng.permutation(n_items), rng.randint(0, n_items, size=n_ev - n_items)])
        sess = np.repeat(np.arange(n_ev // 5), 5)
        data = pd.DataFrame({'SessionId': sess, 'ItemId': items[:len(sess)], 'Time': np.arange(len(sess), dtype=np.int64)})
        g = GRU4Rec(layers=[D], final_act='linear', loss='bpr-max', n_epochs=1, batch_size=32, n_sample=64 if n_items > 1 else 0,
                    learning_rate=0.1, constrained_embedding=mode == 'constrained', embedding=64 if mode == 'separate' else 0)
        g.prepare(data, sample_store=64 * 256 if n_items > 1 else 0)
        assert g.n_items == n_items
        w0 = g.Wy.copy()
        if n_items > 1 and steps > 0:
            train_some(g, steps)
        else:      # tables that are not the initial draws without training: every row rescaled and shifted, uploaded with set_param
            g._download_weights()
            g.Wy = (g.Wy * rng.uniform(0.3, 3.0, size=(n_items, 1)) + rng.randn(*g.Wy.shape) * 0.02).astype(np.float32)
            g._dev_put(g._model, 'Wy', g.Wy)
        assert (g.Wy != w0).any()
        _MODELS[key] = g
    return _MODELS[key]


def table_of(g, space):
    return g.E if (space == 'input' and g.embedding and not g.constrained_embedding) else g.Wy


def reference(T, qidx, cidx, metric):
    """fp64 scores [len(qidx), len(cidx)] and the bound of the module docstring."""
    T = T.astype(np.float64)
    Q, Cn = T[qidx], T[cidx]
    D = T.shape[1]
    ref, S = Q @ Cn.T, np.abs(Q) @ np.abs(Cn).T
    if metric == 'dot':
        return ref, (D + 2) * U * S
    nq, nc = np.sqrt((Q * Q).sum(1)), np.sqrt((Cn * Cn).sum(1))
    den = nq[:, None] * nc[None, :]
    with np.errstate(divide='ignore', invalid='ignore'):
        ref, S = np.where(den > 0, ref / den, 0.0), np.where(den > 0, S / den, 0.0)
    return ref, (2 * D + 16) * U * S


def check_rows(g, T, query_ids, items, scores, k, metric, cand=None, exclude_self=True, exclude=(), rows_per_block=None, tag=''):
    """Every row of a similar_items result against the fp64 reference (module docstring).  Returns the worst error / bound ratio."""
    ids = g.itemidmap.index.values
    query_ids = np.asarray(query_ids)
    cand_ids = ids if cand is None else np.asarray(cand)
    qidx, cidx = g.itemidmap[query_ids].values, g.itemidmap[cand_ids].values
    xidx = g.itemidmap[list(exclude)].values if len(exclude) else np.zeros(0, dtype=np.int64)
    assert items.shape == scores.shape == (len(qidx), k) and scores.dtype == np.float32
    assert not np.isnan(scores).any()
    worst = 0.0
    pos_of = {}
    for p, i in enumerate(cand_ids):
        pos_of.setdefault(i, []).append(p)
    unique_cand = len(pos_of) == len(cand_ids)
    lookup = pd.Series(np.arange(len(cand_ids)), index=cand_ids) if unique_cand else None
    rows_per_block = rows_per_block or max(16, int(2e7 // len(cidx)))
    for r0 in range(0, len(qidx), rows_per_block):
        q = qidx[r0:r0 + rows_per_block]
        ref, bound = reference(T, q, cidx, metric)
        elig = ~np.isin(cidx, xidx)[None, :] & np.ones((len(q), 1), dtype=bool)
        if exclude_self:
            elig &= cidx[None, :] != q[:, None]
        assert (elig.sum(1) >= k).all()
        kth = -np.partition(np.where(elig, -ref, np.inf), k - 1, axis=1)[:, k - 1]
        bmax = np.where(elig, bound, 0.0).max(1)
        for r in range(len(q)):
            it, sc = items[r0 + r], scores[r0 + r].astype(np.float64)
            if unique_cand:
                cols = lookup[it].values
            else:      # the j-th occurrence of an id in a row is the j-th lowest position holding it (what the tie rule demands)
                seen, cols = {}, []
                for i in it:
                    n = seen.get(i, 0)
                    assert n < len(pos_of[i]), '%s row %d: id %r returned more often than it is a candidate' % (tag, r0 + r, i)
                    cols.append(pos_of[i][n])
                    seen[i] = n + 1
                cols = np.array(cols)
            assert len(set(cols.tolist())) == k, '%s row %d: a candidate position returned twice' % (tag, r0 + r)
            assert elig[r, cols].all(), '%s row %d: an excluded position returned' % (tag, r0 + r)
            err, b = np.abs(sc - ref[r, cols]), bound[r, cols]
            j = int((err - b).argmax())
            assert (err <= b).all(), '%s row %d: score of candidate position %d off by %g, bound %g' % (tag, r0 + r, cols[j], err[j], b[j])
            if (b > 0).any():
                worst = max(worst, float((err[b > 0] / b[b > 0]).max()))
            assert (ref[r, cols] >= kth[r] - b - bmax[r]).all(), '%s row %d: an item outside the tie-tolerant top k returned' % (tag, r0 + r)
            assert (sc[1:] <= sc[:-1]).all(), '%s row %d: scores rise' % (tag, r0 + r)
            same = sc[1:] == sc[:-1]
            assert (cols[1:][same] > cols[:-1][same]).all(), '%s row %d: equal scores not in ascending candidate position' % (tag, r0 + r)
    return worst


def queries(g, n, seed=0):
    ids = g.itemidmap.index.values
    return ids[np.random.RandomState(seed).randint(0, len(ids), size=n)]


# ---- against fp64 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_items,D,mode', [(37483, 100, 'constrained'), (200000, 100, 'separate'), (50, 30, 'onehot'),
                                            (3000, 256, 'constrained'), (3000, 512, 'separate'), (2000, 1024, 'constrained')])
def test_scores_and_selection_against_fp64(n_items, D, mode):
    g = fitted(n_items, D, mode, steps=40 if D <= 256 else 10)
    ids = g.itemidmap.index.values
    assert g.Wy.shape == (n_items, D)
    q = queries(g, 200 if n_items > 50 else 50, seed=D)
    sub = ids[np.random.RandomState(1).permutation(n_items)[:max(n_items // 3, 40)]]
    sub[3:6] = sub[0]      # duplicated candidates
    spaces = ['output'] if mode == 'onehot' else ['output', 'input']
    for space in spaces:
        T = table_of(g, space)
        assert T.shape[1] == (64 if (space == 'input' and mode == 'separate') else D)
        for metric in ('cosine', 'dot'):
            for k in (1, 20, 256):
                if k >= n_items:
                    continue
                items, scores = g.similar_items(q, k=k, metric=metric, space=space)
                w = check_rows(g, T, q, items, scores, k, metric, tag='%s/%s/k=%d' % (space, metric, k))
                print('n=%d D=%d %s %s %s k=%d: worst error / bound = %.3f' % (n_items, D, mode, space, metric, k, w))
            k = min(20, len(sub) - 4)
            items, scores = g.similar_items(q, k=k, metric=metric, space=space, predict_for_item_ids=sub)
            check_rows(g, T, q, items, scores, k, metric, cand=sub, tag='%s/%s/list' % (space, metric))
    if mode == 'onehot':
        with pytest.raises(NotImplementedError, match="space='output'"):
            g.similar_items(q, k=5, space='input')
        with pytest.raises(_native.NativeError, match='one-hot'):
            g._ensure_model().similar_items(np.zeros(1, dtype=np.int32), None, 5, 'cosine', 'input')


def test_whole_catalogue_against_fp64():
    """item_neighbors at 37,483 x 100: every one of its rows is checked, and it is similar_items over the catalogue bit for bit."""
    g = fitted(37483, 100, 'constrained')
    ids = g.itemidmap.index.values
    items, scores = g.item_neighbors(k=20)
    assert items.shape == (37483, 20)
    w = check_rows(g, g.Wy, ids, items, scores, 20, 'cosine', tag='item_neighbors')
    print('item_neighbors 37483 x 100: worst error / bound = %.3f' % w)
    part = np.random.RandomState(3).permutation(len(ids))[:3000]
    it2, sc2 = g.similar_items(ids[part], k=20)
    np.testing.assert_array_equal(it2, items[part])
    np.testing.assert_array_equal(bits(sc2), bits(scores[part]))


def test_catalogue_of_one_item():
    g = fitted(1, 30, 'constrained')
    ids = g.itemidmap.index.values
    for metric in ('cosine', 'dot'):
        items, scores = g.similar_items(ids, k=1, metric=metric, exclude_self=False)
        check_rows(g, g.Wy, ids, items, scores, 1, metric, exclude_self=False)
        assert items[0, 0] == ids[0]
    with pytest.raises(ValueError, match='query 0'):
        g.similar_items(ids, k=1)
    with pytest.raises(_native.NativeError, match='query 0'):
        g._ensure_model().similar_items(np.zeros(1, dtype=np.int32), None, 1)


# ---- ties, zero rows ------------------------------------------------------------------------------------------------------------------
def with_rows(n_items, D, edit):
    """A copy-free variant of the fitted model whose Wy went through edit(Wy) and was uploaded with set_param."""
    g = fitted(n_items, D, 'constrained')
    Wy = g.Wy.copy()
    edit(Wy)
    g.Wy = Wy
    g._dev_put(g._ensure_model(), 'Wy', g.Wy)
    return g


def test_exact_ties_and_zero_rows():
    n = 37483
    keep = fitted(n, 100, 'constrained').Wy.copy()
    dup = [5, 100, 101, 20000, 37482]

    def edit(Wy):
        Wy[dup[1:]] = Wy[dup[0]]
        Wy[[7, 300]] = 0.0
    g = with_rows(n, 100, edit)
    try:
        ids = g.itemidmap.index.values
        for metric in ('cosine', 'dot'):
            items, scores = g.similar_items(ids[[5, 20000]], k=20, metric=metric, exclude_self=False)
            check_rows(g, g.Wy, ids[[5, 20000]], items, scores, 20, metric, exclude_self=False)
            if metric == 'cosine':      # (under dot a longer row may score higher than the row itself)
                for r in range(2):
                    np.testing.assert_array_equal(items[r, :5], ids[dup])      # the duplicates first, the lower position first
                    assert len(set(bits(scores[r, :5]).tolist())) == 1
                assert abs(float(scores[0, 0]) - 1.0) <= (2 * 100 + 16) * U
            # the same through a shuffled candidate list: the duplicates in the list's order
            perm = np.random.RandomState(2).permutation(n)[:5000]
            perm = np.concatenate([perm[~np.isin(perm, dup)], dup])
            np.random.RandomState(4).shuffle(perm)
            it2, sc2 = g.similar_items(ids[[5]], k=20, metric=metric, exclude_self=False, predict_for_item_ids=ids[perm])
            check_rows(g, g.Wy, ids[[5]], it2, sc2, 20, metric, cand=ids[perm], exclude_self=False)
            if metric == 'cosine':
                want = [i for i in perm if i in dup]
                np.testing.assert_array_equal(it2[0, :5], ids[want])
                assert set(bits(sc2[0, :5]).tolist()) == set(bits(scores[0, :1]).tolist())
            # a zero row: 0 against everything, in candidate order; others see it as 0
            items, scores = g.similar_items(ids[[7]], k=20, metric=metric, exclude_self=False)
            assert (scores == 0).all()
            np.testing.assert_array_equal(items[0], ids[:20])
            items, scores = g.similar_items(ids[[7]], k=20, metric=metric)
            np.testing.assert_array_equal(items[0], ids[[i for i in range(21) if i != 7]])
        # duplicate queries give duplicate rows
        items, scores = g.similar_items(ids[[9, 5, 9, 9]], k=20)
        for r in (2, 3):
            np.testing.assert_array_equal(items[r], items[0])
            np.testing.assert_array_equal(bits(scores[r]), bits(scores[0]))
    finally:
        g.Wy = keep
        g._dev_put(g._ensure_model(), 'Wy', g.Wy)


# ---- pair invariance ------------------------------------------------------------------------------------------------------------------
CHILD = """
import sys
import numpy as np
from gru4rec_amd.gru4rec import GRU4Rec
g = GRU4Rec.loadmodel(sys.argv[1])
q = np.load(sys.argv[2], allow_pickle=True)
items, scores = g.similar_items(q, k=int(sys.argv[4]), metric=sys.argv[5])
np.savez(sys.argv[3], items=items, scores=scores)
"""


@pytest.mark.parametrize('metric', ['cosine', 'dot'])
def test_a_pair_scores_the_same_bits_everywhere(metric, tmp_path):
    g = fitted(37483, 100, 'constrained')
    ids = g.itemidmap.index.values
    k = 256
    q = queries(g, 3000, seed=8)
    big_i, big_s = g.similar_items(q, k=k, metric=metric)
    # alone
    for r in (0, 1500, 2999):
        i1, s1 = g.similar_items(q[r:r + 1], k=k, metric=metric)
        np.testing.assert_array_equal(i1[0], big_i[r])
        np.testing.assert_array_equal(bits(s1[0]), bits(big_s[r]))
    # in chunks of 100 rows (a child process: the environment is read per call, but the parent's must stay as it is)
    model, qf, out = str(tmp_path / 'm.pickle'), str(tmp_path / 'q.npy'), str(tmp_path / 'o.npz')
    g.savemodel(model)
    np.save(qf, q)
    r = subprocess.run([sys.executable, '-c', CHILD, model, qf, out, str(k), metric], cwd=ROOT, env=dict(os.environ, G4R_SIM_CHUNK='100'),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    z = np.load(out, allow_pickle=True)
    np.testing.assert_array_equal(z['items'], big_i)
    np.testing.assert_array_equal(bits(z['scores']), bits(big_s))
    # through a shuffled subset of the candidates: every pair that appears in both calls
    sub = ids[np.random.RandomState(5).permutation(len(ids))[:12000]]
    sub_i, sub_s = g.similar_items(q[:300], k=k, metric=metric, predict_for_item_ids=sub)
    shared = 0
    for r in range(300):
        a = dict(zip(big_i[r].tolist(), bits(big_s[r]).tolist()))
        for i, b in zip(sub_i[r].tolist(), bits(sub_s[r]).tolist()):
            if i in a:
                shared += 1
                assert a[i] == b, 'query %r, candidate %r: %08x in the whole catalogue, %08x in the list' % (q[r], i, a[i], b)
    assert shared > 300 * 20
    # in item_neighbors
    all_i, all_s = g.item_neighbors(k=k, metric=metric)
    rows = g.itemidmap[q].values
    np.testing.assert_array_equal(all_i[rows], big_i)
    np.testing.assert_array_equal(bits(all_s[rows]), bits(big_s))


# ---- exclusions -----------------------------------------------------------------------------------------------------------------------
def test_exclusions_remove_exactly_those_positions():
    g = fitted(37483, 100, 'constrained')
    ids = g.itemidmap.index.values
    q = queries(g, 150, seed=12)
    full_i, full_s = g.similar_items(q, k=256, exclude_self=False)
    assert (full_i[:, 0] == q).mean() > 0.99      # cosine: the query itself comes first
    assert np.abs(full_s[:, 0].astype(np.float64) - 1.0).max() <= (2 * 100 + 16) * U
    # exclude_self removes the query and nothing else
    self_i, self_s = g.similar_items(q, k=200)
    ex = np.unique(np.concatenate([full_i[:, 1:9].ravel(), ids[:50]]))      # many of every row's best
    ex_i, ex_s = g.similar_items(q, k=100, exclude=ex)
    for r in range(len(q)):
        keep = full_i[r] != q[r]
        np.testing.assert_array_equal(self_i[r], full_i[r][keep][:200])
        np.testing.assert_array_equal(bits(self_s[r]), bits(full_s[r][keep][:200]))
        keep &= ~np.isin(full_i[r], ex)
        assert keep.sum() >= 100
        np.testing.assert_array_equal(ex_i[r], full_i[r][keep][:100])
        np.testing.assert_array_equal(bits(ex_s[r]), bits(full_s[r][keep][:100]))
    check_rows(g, g.Wy, q, ex_i, ex_s, 100, 'cosine', exclude=ex)
    # a query left with k - 1 eligible positions is refused by name and nothing is launched
    m = g._ensure_model()
    m.set_param('By', g.By.reshape(-1))      # (any upload invalidates the norms: a launch would rebuild them)
    before = m.sim_norms()
    assert not before[1]
    cand = g.itemidmap[ids[[3, 4, 5, 6, 4]]].values.astype(np.int32)
    with pytest.raises(_native.NativeError, match=r'query 1 \(item index 4\) has 3 eligible candidate positions, fewer than k = 4'):
        m.similar_items(np.array([3, 4, 5], dtype=np.int32), cand, 4)
    with pytest.raises(ValueError, match=r'query 1 \(item id %d\) has 3 eligible' % ids[4]):
        g.similar_items(ids[[3, 4, 5]], k=4, predict_for_item_ids=ids[[3, 4, 5, 6, 4]])
    assert m.sim_norms() == before
    for bad in (dict(k=0), dict(k=257), dict(metric='cosine', space='input', k=5, q_idx=np.array([37483], dtype=np.int32))):
        kw = dict(dict(q_idx=np.array([3], dtype=np.int32), item_idx=None, k=5), **bad)
        with pytest.raises(_native.NativeError):
            m.similar_items(**kw)
    # a space or metric the header does not define is refused by the C entry itself, on a constrained model too
    q1, oc, os_ = np.array([3], dtype=np.int32), np.empty(5, dtype=np.int32), np.empty(5, dtype=np.float32)
    for space, metric in ((7, 1), (-1, 0), (0, 2), (1, -1)):
        rc = _native.lib().g4r_similar_items(m.h, space, metric, _native._i32(q1), 1, None, 0, 5, 1, None, _native._i32(oc), _native._f32(os_))
        assert rc != 0 and (b'space must be' if space not in (0, 1) else b'metric must be') in _native.lib().g4r_last_error()
    assert m.sim_norms() == before


# ---- cache, state ---------------------------------------------------------------------------------------------------------------------
def test_norm_cache_follows_the_weights():
    g = fitted(3000, 256, 'separate')
    ids = g.itemidmap.index.values
    m = g._ensure_model()
    q = queries(g, 100, seed=2)
    for space in ('output', 'input'):
        items, scores = g.similar_items(q, k=20, space=space)
    bytes_held, valid, builds = m.sim_norms()
    assert valid and bytes_held == 2 * 3000 * 4
    g.similar_items(q, k=20, metric='dot')
    g.similar_items(q, k=20)
    assert m.sim_norms() == (bytes_held, True, builds)      # nothing changed: nothing rebuilt
    old = g.Wy.copy()
    train_some(g, 20)                                        # further steps of fit
    assert not m.sim_norms()[1] and not np.array_equal(old, g.Wy)
    for space in ('output', 'input'):
        items, scores = g.similar_items(q, k=20, space=space)
        check_rows(g, table_of(g, space), q, items, scores, 20, 'cosine', tag='after fit/' + space)
    assert m.sim_norms() == (bytes_held, True, builds + 2)
    g.Wy = (g.Wy * np.linspace(0.5, 3.0, 3000, dtype=np.float32)[:, None]).astype(np.float32)      # other norms, same directions
    g._dev_put(m, 'Wy', g.Wy)
    assert not m.sim_norms()[1]
    items, scores = g.similar_items(q, k=20)
    check_rows(g, g.Wy, q, items, scores, 20, 'cosine', tag='after set_param')
    assert m.sim_norms() == (bytes_held, True, builds + 3)


def test_the_prediction_state_is_untouched():
    g = fitted(37483, 100, 'constrained')
    ids = g.itemidmap.index.values
    rng = np.random.RandomState(21)
    seq = [(rng.randint(0, 3, size=40), ids[rng.randint(0, len(ids), size=40)]) for _ in range(6)]
    out = []
    for interleave in (False, True):
        g.predict = None
        got = []
        for t, (sid, inp) in enumerate(seq):
            if interleave:
                g.similar_items(queries(g, 300, seed=t), k=20, metric='cosine' if t % 2 else 'dot')
            if t % 2:
                got.append(g.predict_next_batch(sid, inp, batch=40).values)
            else:
                got.extend(g.recommend_next_batch(sid, inp, k=20, batch=40))
        if interleave:
            g.item_neighbors(k=5)
        out.append(got)
    for a, b in zip(*out):
        if a.dtype == np.float32:
            np.testing.assert_array_equal(bits(a), bits(b))
        else:
            np.testing.assert_array_equal(a, b)


# ---- command line ---------------------------------------------------------------------------------------------------------------------
def test_cli_saves_the_neighbour_table(tmp_path):
    from gru4rec_amd import synth
    data = synth.make_sessions(2000, n_items=400, seed=4)
    train, model, nb = str(tmp_path / 'train.tsv'), str(tmp_path / 'model.pickle'), str(tmp_path / 'nb.npz')
    data.to_csv(train, sep='\t', index=False)
    ps = 'loss=bpr-max,final_act=linear,layers=48,batch_size=32,n_sample=128,constrained_embedding=True,n_epochs=1'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'run.py'), train, '-ps', ps, '-s', model, '-ss', str(128 * 64), '--save_neighbors', nb,
                        '--neighbors_k', '7', '--neighbors_metric', 'dot'], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert 'nearest neighbours' in r.stdout
    z = np.load(nb, allow_pickle=True)
    g = GRU4Rec.loadmodel(model)
    items, scores = g.item_neighbors(k=7, metric='dot')
    np.testing.assert_array_equal(z['item_ids'], g.itemidmap.index.values)
    np.testing.assert_array_equal(z['neighbor_ids'], items)
    np.testing.assert_array_equal(bits(z['scores']), bits(scores))
    assert items.shape == (len(g.itemidmap), 7)
    g.close()

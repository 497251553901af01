"""GRU4Rec.score_candidates / score_candidates_sessions (g4r_score_candidates*, k_score_cand) against the routes of their contract,
on twin models that hold identical weights.  Row i must equal, bit for bit, what the existing calls return with
predict_for_item_ids = candidates[i]: column i of predict_next_batch (k=None), row i of recommend_next_batch (k); with an
element-wise final activation also the full-catalogue predict_next_batch score of the item.  The stateless form must equal the
stepwise route of recommend_sessions, and one configuration is checked against the NumPy oracle."""
import pickle

import numpy as np
import pandas as pd
import pytest

from gru4rec_amd import _native
from gru4rec_amd.gru4rec import GRU4Rec
from oracle.model import OracleGRU4Rec

pytestmark = pytest.mark.gpu

N_ITEMS = 3000
_MODELS = {}


def fitted(final_act='linear', layers=(64,), embed='constrained'):
    """A GRU4Rec fitted for one epoch on synthetic sessions that hold every one of N_ITEMS items (ids 10, 13, 16, ...).
    embed: 'onehot', 'embedding' (a separate 32-wide table) or 'constrained'."""
    key = (final_act, tuple(layers), embed)
    if key not in _MODELS:
        rng = np.random.RandomState(sum(layers) + len(final_act))
        items = 10 + 3 * np.concatenate([rng.permutation(N_ITEMS), rng.randint(0, N_ITEMS, size=N_ITEMS)])
        sess = np.repeat(np.arange(len(items) // 5), 5)
        data = pd.DataFrame({'SessionId': sess, 'ItemId': items[:len(sess)], 'Time': np.arange(len(sess), dtype=np.int64)})
        sm = final_act.startswith('softmax')
        g = GRU4Rec(layers=list(layers), final_act=final_act, loss='cross-entropy' if sm else 'bpr-max', n_epochs=1, batch_size=64,
                    n_sample=0 if sm else 128, learning_rate=0.05, constrained_embedding=(embed == 'constrained'),
                    embedding=32 if embed == 'embedding' else 0)
        g.fit(data, sample_store=0 if sm else 100000)
        assert g.n_items == N_ITEMS
        _MODELS[key] = g
    return _MODELS[key]


def twins(g):
    """Two models with g's weights, each with a device model and a prediction state of its own."""
    blob = pickle.dumps(g)
    return pickle.loads(blob), pickle.loads(blob)


def assert_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    assert a.shape == b.shape
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))


def ragged_lists(g, lens, seed=0, dup=False):
    rng = np.random.RandomState(seed)
    ids = g.itemidmap.index.values
    out = []
    for n in lens:
        c = ids[rng.randint(0, len(ids), size=n)]
        if dup and n > 2:
            c[rng.randint(0, n, size=max(1, n // 4))] = c[0]      # repeated items, the first one at the lowest position
        out.append(c)
    return out


def histories(g, lens, seed=0):
    rng = np.random.RandomState(seed)
    ids = g.itemidmap.index.values
    return [ids[rng.randint(0, len(ids), size=n)] for n in lens]


def calls(g, n, steps, seed=0):
    """`steps` consecutive (session ids, input item ids) of n slots, with session changes in between."""
    rng = np.random.RandomState(seed)
    ids = g.itemidmap.index.values
    sid = np.arange(n)
    out = []
    for s in range(steps):
        if s:
            ch = rng.rand(n) < 0.3
            sid = np.where(ch, sid + 1000 * (s + 1), sid)
        out.append((sid.copy(), ids[rng.randint(0, len(ids), size=n)]))
    return out


# ---------------------------------------------------------------------------------------------- element-wise final activations
ELEMENTWISE = [('linear', (100,), 'constrained'), ('linear', (37,), 'embedding'), ('tanh', (64, 48), 'onehot'),
               ('relu', (512,), 'constrained'), ('leaky-0.1', (37,), 'onehot'), ('elu-0.5', (100,), 'embedding')]


@pytest.mark.parametrize('final_act,layers,embed', ELEMENTWISE)
def test_elementwise_scores_equal_the_full_catalogue(final_act, layers, embed):
    a, b = twins(fitted(final_act, layers, embed))
    n = 24
    cand = np.stack(ragged_lists(a, [50] * n, seed=len(layers)))
    col = a.itemidmap[cand.ravel()].values.reshape(n, -1)
    for s, (sid, inp) in enumerate(calls(a, n, 4, seed=1)):
        got = a.score_candidates(sid, inp, cand, batch=n)
        full = b.predict_next_batch(sid, inp, batch=n).values.T          # [n, n_items]
        assert got.shape == cand.shape and got.dtype == np.float32
        assert_bits(got, np.take_along_axis(full, col, axis=1))
    # the hidden states stayed in step: one more call of each route agrees on every item
    sid, inp = calls(a, n, 5, seed=1)[-1]
    assert_bits(a.predict_next_batch(sid, inp, batch=n).values, b.predict_next_batch(sid, inp, batch=n).values)


@pytest.mark.parametrize('final_act', ['linear', 'tanh'])
def test_ragged_elementwise_and_interleaving(final_act):
    a, b = twins(fitted(final_act))
    n = 16
    lens = [1, 31, 32, 33, 257, 2000] + list(np.random.RandomState(2).randint(1, 400, size=n - 6))
    cand = ragged_lists(a, lens, seed=3, dup=True)
    steps = calls(a, n, 4, seed=4)
    for s, (sid, inp) in enumerate(steps):
        if s == 2:      # an interleaved predict_next_batch / recommend_next_batch call on both sides
            assert_bits(a.predict_next_batch(sid, inp, batch=n).values, b.predict_next_batch(sid, inp, batch=n).values)
            continue
        got = a.score_candidates(sid, inp, cand, batch=n)
        full = b.predict_next_batch(sid, inp, batch=n).values.T
        assert isinstance(got, list) and len(got) == n
        for i in range(n):
            assert_bits(got[i], full[i, a.itemidmap[cand[i]].values])
        assert got[0].base is not None and all(x.base is got[0].base for x in got)     # views into one CSR buffer


def per_row_models(g, n):
    """n models with g's weights: model i answers row i's calls with predict_for_item_ids = that row's list (the contract's
    reference); all of them see the same sequence of calls."""
    blob = pickle.dumps(g)
    return [pickle.loads(blob) for _ in range(n)]


# ---------------------------------------------------------------------------------------------- softmax / softmax_logit
@pytest.mark.parametrize('final_act', ['softmax', 'softmax_logit'])
def test_softmax_normalises_over_the_rows_own_list(final_act):
    g = fitted(final_act)
    a = pickle.loads(pickle.dumps(g))
    lens = [1, 31, 32, 33, 257, 1999]
    n = len(lens)
    refs = per_row_models(g, n)
    cand = ragged_lists(g, lens, seed=5, dup=True)
    for sid, inp in calls(g, n, 3, seed=6):
        got = a.score_candidates(sid, inp, cand, batch=n)
        for i, r in enumerate(refs):
            assert_bits(got[i], r.predict_next_batch(sid, inp, predict_for_item_ids=cand[i], batch=n).values[:, i])


# ---------------------------------------------------------------------------------------------- k
@pytest.mark.parametrize('final_act,k', [('linear', 1), ('linear', 20), ('softmax', 20), ('relu', 7)])
def test_topk_equals_recommend_next_batch(final_act, k):
    g = fitted(final_act)
    a = pickle.loads(pickle.dumps(g))
    lens = [20, 31, 33, 256, 300, 2000, 40, 25]
    n = len(lens)
    refs = per_row_models(g, n)
    cand = ragged_lists(g, lens, seed=7, dup=True)
    cand[6][:] = cand[6][0]            # one row of a single item 40 times: every score ties, the lower positions win
    for sid, inp in calls(g, n, 3, seed=8):
        items, scores = a.score_candidates(sid, inp, cand, k=k, batch=n)
        assert items.shape == scores.shape == (n, k)
        for i, r in enumerate(refs):
            wi, ws = r.recommend_next_batch(sid, inp, k=k, predict_for_item_ids=cand[i], batch=n)
            np.testing.assert_array_equal(items[i], wi[i])
            assert_bits(scores[i], ws[i])


@pytest.mark.parametrize('final_act', ['linear', 'softmax_logit'])
def test_topk_k_equals_row_length_and_k_256(final_act):
    g = fitted(final_act)
    lens = [256, 300, 1000, 256]
    n = len(lens)
    cand = ragged_lists(g, lens, seed=9, dup=True)
    sid, inp = calls(g, n, 1, seed=10)[0]
    a = pickle.loads(pickle.dumps(g))
    items, scores = a.score_candidates(sid, inp, cand, k=256, batch=n)
    for i, r in enumerate(per_row_models(g, n)):
        wi, ws = r.recommend_next_batch(sid, inp, k=256, predict_for_item_ids=cand[i], batch=n)
        np.testing.assert_array_equal(items[i], wi[i])
        assert_bits(scores[i], ws[i])
    # k = the row's length: the whole list in the contract's order
    cand2 = np.stack(ragged_lists(g, [12] * n, seed=11, dup=True))
    a, c = twins(g)
    items, scores = a.score_candidates(sid, inp, cand2, k=12, batch=n)
    full = c.score_candidates(sid, inp, cand2, batch=n)
    for i in range(n):
        order = sorted(range(12), key=lambda j: (-full[i, j], j))
        np.testing.assert_array_equal(items[i], cand2[i, order])
        assert_bits(scores[i], full[i, order])


# ---------------------------------------------------------------------------------------------- stateless
def stepwise(g, hists, cand, k):
    """The contract's route: a fresh prediction state, the first T - 1 items of every history through predict_next_batch (histories
    aligned to end together), the last one through score_candidates."""
    N, T = len(hists), max(len(h) for h in hists)
    ids = g.itemidmap.index.values
    g.predict = None
    for s in range(T):
        live = [s >= T - len(h) for h in hists]
        sid = np.array([i if a else -2 - i for i, a in enumerate(live)])
        inp = np.array([h[s - (T - len(h))] if a else ids[0] for h, a in zip(hists, live)])
        if s < T - 1:
            g.predict_next_batch(sid, inp, predict_for_item_ids=ids[:1], batch=N)
    out = g.score_candidates(sid, inp, cand, k=k, batch=N)
    g.predict = None
    return out


@pytest.mark.parametrize('final_act,k', [('linear', None), ('linear', 5), ('softmax', None), ('softmax_logit', 3), ('tanh', None)])
def test_sessions_equal_the_stepwise_route(final_act, k):
    g = fitted(final_act)
    hists = histories(g, [3, 1, 8, 5, 2, 8, 1, 12], seed=12)
    cand = ragged_lists(g, [40, 5, 300, 33, 6, 90, 257, 10], seed=13, dup=True)
    got = g.score_candidates_sessions(hists, cand, k=k)
    want = stepwise(g, hists, cand, k)
    if k is None:
        for x, y in zip(got, want):
            assert_bits(x, y)
    else:
        np.testing.assert_array_equal(got[0], want[0])
        assert_bits(got[1], want[1])


def test_sessions_hidden_continuation_and_return_hidden():
    g = fitted('linear', (100, 64), 'onehot')
    lens_a = [4, 1, 7, 3, 2]
    ha, hb = histories(g, lens_a, seed=14), histories(g, [3, 2, 1, 5, 4], seed=15)
    cand = np.stack(ragged_lists(g, [60] * 5, seed=16))
    s_ab, H_ab = g.score_candidates_sessions([np.concatenate([x, y]) for x, y in zip(ha, hb)], cand, return_hidden=True)
    _, Ha = g.score_candidates_sessions(ha, cand, return_hidden=True)
    s_b, H_b = g.score_candidates_sessions(hb, cand, hidden=Ha, return_hidden=True)
    assert_bits(s_b, s_ab)
    for x, y in zip(H_b, H_ab):
        assert_bits(x, y)
    _, _, H_rec = g.recommend_sessions(ha, k=5, return_hidden=True)
    for x, y in zip(Ha, H_rec):
        assert_bits(x, y)
    it, sc, H_k = g.score_candidates_sessions(ha, cand, k=5, return_hidden=True)
    assert it.shape == sc.shape == (5, 5)
    for x, y in zip(H_k, H_rec):
        assert_bits(x, y)


@pytest.mark.parametrize('final_act', ['linear', 'softmax'])
def test_sessions_many_rows_and_chunking(final_act, monkeypatch):
    g = fitted(final_act)
    N = 700
    rng = np.random.RandomState(17)
    hists = histories(g, list(rng.randint(1, 12, size=N)), seed=18)
    cand = ragged_lists(g, list(rng.randint(1, 300, size=N)), seed=19)
    s0, H0 = g.score_candidates_sessions(hists, cand, return_hidden=True)
    i0, t0 = g.score_candidates_sessions(hists, cand, k=1)
    monkeypatch.setenv('G4R_SESSIONS_CHUNK', '37')
    s1, H1 = g.score_candidates_sessions(hists, cand, return_hidden=True)
    i1, t1 = g.score_candidates_sessions(hists, cand, k=1)
    for x, y in zip(s0, s1):
        assert_bits(x, y)
    for x, y in zip(H0, H1):
        assert_bits(x, y)
    np.testing.assert_array_equal(i0, i1)
    assert_bits(t0, t1)
    # a few rows against the stepwise route
    sel = [0, 1, 511, 512, 699]
    want = stepwise(g, [hists[i] for i in sel], [cand[i] for i in sel], None)
    for j, i in enumerate(sel):
        assert_bits(s0[i], want[j])


# ---------------------------------------------------------------------------------------------- the NumPy oracle
def oracle_of(g):
    o = OracleGRU4Rec(n_items=g.n_items, layers=tuple(g.layers), batch_size=g.batch_size, final_act=g.final_act, hidden_act=g.hidden_act,
                      constrained_embedding=g.constrained_embedding, embedding=g.embedding, dtype=np.float32)
    for n in ('Wx', 'Wh', 'Wrz', 'Bh'):
        setattr(o, n, [np.asarray(x, dtype=np.float32).copy() for x in getattr(g, n)])
    o.Wy = np.asarray(g.Wy, dtype=np.float32).copy()
    o.By = np.asarray(g.By, dtype=np.float32).reshape(-1).copy()
    if g.embedding and not g.constrained_embedding:
        o.E = np.asarray(g.E, dtype=np.float32).copy()
    return o


@pytest.mark.parametrize('final_act', ['tanh', 'softmax'])
def test_against_the_oracle(final_act):
    g = fitted(final_act, (100,), 'embedding')
    o = oracle_of(g)
    hists = histories(g, [3, 1, 6], seed=20)
    cand = ragged_lists(g, [50, 7, 300], seed=21, dup=True)
    got = g.score_candidates_sessions(hists, cand)
    for i, h in enumerate(hists):
        Ho = [np.zeros((1, D), dtype=np.float32) for D in g.layers]
        for x in g.itemidmap[h[:-1]].values:
            _, Ho = o.predict_step(Ho, [x])
        want, _ = o.predict_step(Ho, [g.itemidmap[h[-1]]], item_idx=g.itemidmap[cand[i]].values)
        np.testing.assert_allclose(got[i], np.ravel(want), rtol=2e-4, atol=2e-6)


# ---------------------------------------------------------------------------------------------- a large catalogue
def test_large_catalogue_against_the_union():
    n_items = 2_100_000
    g = GRU4Rec(layers=[64], final_act='linear', loss='bpr-max', batch_size=64, n_sample=0, constrained_embedding=True)
    g.itemidmap = pd.Series(data=np.arange(n_items), index=np.arange(n_items) * 2 + 1, name='ItemIdx')
    g.n_items = n_items
    g.error_during_train = False
    g._init_host_weights()
    g.By = (np.random.RandomState(22).randn(n_items, 1) * 0.1).astype(np.float32)
    a, b = twins(g)
    n = 64
    rng = np.random.RandomState(23)
    ids = g.itemidmap.index.values
    cand = [ids[np.concatenate([rng.randint(0, n_items, size=int(rng.randint(1, 600))), [0, n_items - 1]])] for _ in range(n)]
    union = np.unique(np.concatenate(cand))
    for sid, inp in calls(g, n, 2, seed=24):
        got = a.score_candidates(sid, inp, cand, batch=n)
        full = b.predict_next_batch(sid, inp, predict_for_item_ids=union, batch=n).values.T
        for i in range(n):
            assert_bits(got[i], full[i, np.searchsorted(union, cand[i])])


# ---------------------------------------------------------------------------------------------- refusals on the device
def test_refusals_leave_the_state_alone():
    a, b = twins(fitted('linear'))
    n = 8
    cand = np.stack(ragged_lists(a, [20] * n, seed=25))
    (s0, i0), (s1, i1) = calls(a, n, 2, seed=26)
    a.score_candidates(s0, i0, cand, batch=n)
    b.predict_next_batch(s0, i0, batch=n)
    bad = cand.astype(object)
    bad[3, 4] = -7
    with pytest.raises(KeyError):
        a.score_candidates(s1, i1, bad, batch=n)
    for kw in (dict(k=0), dict(k=21), dict(k=_native.G4R_TOPK_MAX + 1)):
        with pytest.raises(ValueError):
            a.score_candidates(s1, i1, cand, batch=n, **kw)
    with pytest.raises(ValueError):
        a.score_candidates(s1, i1, cand[:-1], batch=n)
    with pytest.raises(ValueError):
        a.score_candidates(s1, i1, [list(c) for c in cand[:-1]] + [[]], batch=n)
    got = a.score_candidates(s1, i1, cand, batch=n)
    full = b.predict_next_batch(s1, i1, batch=n).values.T
    assert_bits(got, np.take_along_axis(full, a.itemidmap[cand.ravel()].values.reshape(n, -1), axis=1))

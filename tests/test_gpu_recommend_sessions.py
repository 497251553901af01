"""GRU4Rec.recommend_sessions / g4r_recommend_sessions against the stepwise route of its contract: a fresh prediction state fed the
first T - 1 items of every history through predict_next_batch, then the last one through recommend_next_batch (same candidates,
exclude_history as exclude_seen).  Items must be equal and scores equal bit for bit; the hidden state that comes back is checked
by continuation (a + b against b from the state after a, bit for bit) and against the NumPy oracle."""
import os

import numpy as np
import pandas as pd
import pytest

from gru4rec_amd import _native
from gru4rec_amd.gru4rec import GRU4Rec, _pad4
from oracle.model import OracleGRU4Rec

pytestmark = pytest.mark.gpu

N_ITEMS = 3000
FINAL_ACTS = ['linear', 'relu', 'tanh', 'leaky-0.1', 'elu-0.5', 'selu-1.0-1.5', 'softmax', 'softmax_logit']
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


def histories(g, lens, seed=0):
    rng = np.random.RandomState(seed)
    ids = g.itemidmap.index.values
    return [ids[rng.randint(0, len(ids), size=n)] for n in lens]


def stepwise(g, hists, k, cand=None, exclude_history=False, exclude=None, exclude_per_row=None):
    """The contract's route: one predict_next_batch slot per history, all histories aligned to end at the last step (a slot holds a
    placeholder session before its own begins; the session change zeroes its state and seen-history), every call before the last
    one with a one-item candidate list, the last one recommend_next_batch."""
    N, T = len(hists), max(len(h) for h in hists)
    ids = g.itemidmap.index.values
    g.predict = None
    for s in range(T):
        live = [s >= T - len(h) for h in hists]
        sid = np.array([i if a else -2 - i for i, a in enumerate(live)])
        inp = np.array([h[s - (T - len(h))] if a else ids[0] for h, a in zip(hists, live)])
        if s < T - 1:
            g.predict_next_batch(sid, inp, predict_for_item_ids=ids[:1], batch=N)
    out = g.recommend_next_batch(sid, inp, k=k, predict_for_item_ids=cand, batch=N, exclude_seen=exclude_history, exclude=exclude,
                                 exclude_per_row=exclude_per_row)
    g.predict = None
    return out


def assert_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    assert a.shape == b.shape
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))


def check(g, hists, k=20, cand=None, **kw):
    items, scores = g.recommend_sessions(hists, k=k, predict_for_item_ids=cand, **kw)
    want_items, want_scores = stepwise(g, hists, k, cand, **kw)
    assert items.shape == scores.shape == (len(hists), k)
    np.testing.assert_array_equal(items, want_items)
    assert_bits(scores, want_scores)
    return items, scores


RAGGED = {'one': lambda n: [1] * n, 'equal': lambda n: [7] * n,
          'ragged': lambda n: list(np.random.RandomState(n).randint(1, 201, size=n)),
          'long_among_ones': lambda n: [1] * (n // 2) + [200] + [1] * (n - n // 2 - 1)}


@pytest.mark.parametrize('final_act', FINAL_ACTS)
def test_final_activations(final_act):
    g = fitted(final_act)
    check(g, histories(g, [3, 1, 8, 5, 2, 8, 1], seed=1), k=20)


@pytest.mark.parametrize('layers', [(64,), (100,), (256,), (100, 64)])
@pytest.mark.parametrize('embed', ['onehot', 'embedding', 'constrained'])
def test_layers_and_inputs(layers, embed):
    g = fitted('linear', layers, embed)
    check(g, histories(g, RAGGED['ragged'](9), seed=2), k=20)


@pytest.mark.parametrize('shape', sorted(RAGGED))
@pytest.mark.parametrize('n', [1, 5, 130])
def test_history_lengths_and_row_counts(shape, n):
    g = fitted('linear')
    check(g, histories(g, RAGGED[shape](n), seed=n), k=20)


@pytest.mark.parametrize('final_act', ['linear', 'softmax'])
def test_thousands_of_sessions_and_a_forced_small_chunk(final_act, monkeypatch):
    g = fitted(final_act)
    lens = list(np.random.RandomState(5).randint(1, 31, size=2500))
    hists = histories(g, lens, seed=5)
    items, scores = check(g, hists, k=20)
    _, _, H = g.recommend_sessions(hists, k=20, return_hidden=True)
    monkeypatch.setenv('G4R_SESSIONS_CHUNK', '37')
    items2, scores2, H2 = g.recommend_sessions(hists, k=20, return_hidden=True)
    np.testing.assert_array_equal(items2, items)
    assert_bits(scores2, scores)
    assert_bits(H2[0], H[0])


def subset_with_duplicates(g, n, seed=1):
    rng = np.random.RandomState(seed)
    ids = g.itemidmap.index.values
    c = ids[rng.randint(0, len(ids), size=n)]
    c[n // 2:n // 2 + 10] = c[:10]
    return c


@pytest.mark.parametrize('final_act', ['linear', 'softmax'])
@pytest.mark.parametrize('k', [1, 20, 256])
def test_candidates_with_duplicates_and_k(final_act, k):
    g = fitted(final_act)
    hists = histories(g, RAGGED['ragged'](6), seed=6)
    check(g, hists, k=k, cand=subset_with_duplicates(g, 700))
    check(g, hists, k=k)


@pytest.mark.parametrize('final_act', ['linear', 'softmax', 'relu'])
@pytest.mark.parametrize('kind', ['history', 'global', 'per_row', 'union'])
def test_exclusions(final_act, kind):
    g = fitted(final_act)
    hists = histories(g, [4, 1, 9, 30, 2, 6], seed=7)
    rng = np.random.RandomState(8)
    ids = g.itemidmap.index.values
    # each row's own unfiltered top 20 among the excluded: the filtered result has to come from below it
    top, _ = g.recommend_sessions(hists, k=20)
    kw = {}
    if kind in ('history', 'union'):
        kw['exclude_history'] = True
    if kind in ('global', 'union'):
        kw['exclude'] = np.concatenate([top[0][:5], rng.choice(ids, size=30, replace=False)])
    if kind in ('per_row', 'union'):
        kw['exclude_per_row'] = [np.concatenate([t[:10], rng.choice(ids, size=20, replace=False)]) for t in top]
    items, _ = check(g, hists, k=20, **kw)
    check(g, hists, k=20, cand=subset_with_duplicates(g, 700), **kw)
    for r, h in enumerate(hists):
        banned = set(kw.get('exclude', [])) | set(kw['exclude_per_row'][r] if 'exclude_per_row' in kw else []) | \
            (set(h) if kw.get('exclude_history') else set())
        assert not banned & set(items[r])


@pytest.mark.parametrize('shape', ['ragged', 'equal'])
def test_hidden_continuation(shape):
    g = fitted('linear', (100, 64))
    rng = np.random.RandomState(9)
    hists = histories(g, RAGGED['ragged'](40) if shape == 'ragged' else [12] * 40, seed=9)
    # b keeps at least one item; 'equal': every a and every b of one length
    split = [rng.randint(0, len(h)) for h in hists] if shape == 'ragged' else [5] * len(hists)
    a = [h[:s] for h, s in zip(hists, split)]
    b = [h[s:] for h, s in zip(hists, split)]
    items, scores, H = g.recommend_sessions(hists, k=20, return_hidden=True)
    # sessions whose a is empty start from zero: give them explicit zero rows
    has_a = [i for i in range(len(a)) if len(a[i])]
    _, _, Ha = g.recommend_sessions([a[i] for i in has_a], k=20, return_hidden=True)
    H0 = [np.zeros((len(hists), D), dtype=np.float32) for D in g.layers]
    for l in range(len(H0)):
        H0[l][has_a] = Ha[l]
    items2, scores2, H2 = g.recommend_sessions(b, k=20, hidden=H0, return_hidden=True)
    np.testing.assert_array_equal(items2, items)
    assert_bits(scores2, scores)
    for l in range(len(H)):
        assert H[l].shape == (len(hists), g.layers[l])
        assert_bits(H2[l], H[l])
    # zero rows given explicitly are the same as hidden=None
    _, s0, h0 = g.recommend_sessions(b, k=20, hidden=[np.zeros_like(x) for x in H0], return_hidden=True)
    _, s1, h1 = g.recommend_sessions(b, k=20, return_hidden=True)
    assert_bits(s0, s1)
    assert_bits(h0[0], h1[0])


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


@pytest.mark.parametrize('shape', ['ragged', 'equal'])
@pytest.mark.parametrize('layers,embed', [((64,), 'constrained'), ((100, 64), 'onehot'), ((256,), 'embedding')])
def test_hidden_out_against_the_oracle(layers, embed, shape):
    g = fitted('linear', layers, embed)
    o = oracle_of(g)
    lens = [1, 2, 3, 4, 5, 6, 3, 1] if shape == 'ragged' else [5] * 8
    hists = histories(g, lens, seed=10)
    _, _, H = g.recommend_sessions(hists, k=5, return_hidden=True)
    for i, h in enumerate(hists):
        Ho = [np.zeros((1, D), dtype=np.float32) for D in g.layers]
        for x in g.itemidmap[h].values:
            _, Ho = o.predict_step(Ho, [x])
        for l in range(len(H)):
            np.testing.assert_allclose(H[l][i], Ho[l][0], atol=2e-6 * len(h), rtol=3e-4)


def test_permuting_the_sessions_permutes_the_outputs():
    g = fitted('softmax')
    hists = histories(g, RAGGED['ragged'](50), seed=11)
    items, scores, H = g.recommend_sessions(hists, k=20, exclude_history=True, return_hidden=True)
    p = np.random.RandomState(12).permutation(50)
    items2, scores2, H2 = g.recommend_sessions([hists[i] for i in p], k=20, exclude_history=True, return_hidden=True)
    np.testing.assert_array_equal(items2, items[p])
    assert_bits(scores2, scores[p])
    assert_bits(H2[0], H[0][p])


def test_interleaving_leaves_predict_and_recommend_unchanged():
    g = fitted('linear')
    ids = g.itemidmap.index.values
    rng = np.random.RandomState(13)
    seq = [(rng.randint(0, 3, size=6), ids[rng.randint(0, len(ids), size=6)]) for _ in range(5)]
    hists = histories(g, [3, 9, 1], seed=14)

    def run(interleave):
        g.predict = None
        out, side = [], []
        for t, (sid, inp) in enumerate(seq):
            if t % 2:
                out.append(g.predict_next_batch(sid, inp, batch=6).values)
            else:
                out.append(g.recommend_next_batch(sid, inp, k=10, batch=6, exclude_seen=True))
            if interleave:
                side.append(g.recommend_sessions(hists, k=10, exclude_history=True))
        return out, side
    plain, _ = run(False)
    mixed, side = run(True)
    for x, y in zip(plain, mixed):
        if isinstance(x, tuple):
            np.testing.assert_array_equal(x[0], y[0])
            assert_bits(x[1], y[1])
        else:
            assert_bits(x, y)
    g.predict = None
    want = g.recommend_sessions(hists, k=10, exclude_history=True)
    for items, scores in side:
        np.testing.assert_array_equal(items, want[0])
        assert_bits(scores, want[1])


def test_right_after_fit_and_after_loadmodel(tmp_path):
    g = fitted('tanh', (100,), 'embedding')
    hists = histories(g, [5, 1, 12], seed=15)
    g.predict = None
    items, scores = g.recommend_sessions(hists, k=20)          # no predict call before it
    fn = str(tmp_path / 'm.pickle')
    g.savemodel(fn)
    g2 = GRU4Rec.loadmodel(fn)
    items2, scores2 = g2.recommend_sessions(hists, k=20)
    np.testing.assert_array_equal(items2, items)
    assert_bits(scores2, scores)
    check(g2, hists, k=20)
    g2.close()


def test_refused_calls_on_the_device():
    g = fitted('linear')
    ids = g.itemidmap.index.values
    with pytest.raises(ValueError):
        g.recommend_sessions([ids[:3], []])
    with pytest.raises(KeyError):
        g.recommend_sessions([[ids[0], 1]])
    with pytest.raises(ValueError):
        g.recommend_sessions([ids[:3]], hidden=[np.zeros((1, g.layers[0]), dtype=np.float64)])
    m = g._model
    with pytest.raises(_native.NativeError):      # the C entry's own checks: an empty history, an item out of range
        m.recommend_sessions(np.array([0, 2, 2]), np.array([1, 2], dtype=np.int32), k=5)
    with pytest.raises(_native.NativeError):
        m.recommend_sessions(np.array([0, 1]), np.array([N_ITEMS], dtype=np.int32), k=5)
    check(g, histories(g, [2, 3], seed=16), k=5)      # and the model still works
    assert _pad4(g.layers[0]) == g.layers[0]
    assert os.environ.get('G4R_SESSIONS_CHUNK') is None

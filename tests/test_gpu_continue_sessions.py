"""GRU4Rec.continue_sessions / g4r_continue_sessions against the loop of its contract: recommend_sessions on the histories, then
steps - 1 times recommend_sessions on the one-item histories [[previous winner]] from the returned hidden state, the generated items
(and the history) added to exclude_per_row with no_repeat.  Items must be equal, scores and hidden states equal bit for bit."""
import numpy as np
import pandas as pd
import pytest

from gru4rec_amd.gru4rec import GRU4Rec

pytestmark = pytest.mark.gpu

N_ITEMS = 1003          # a partial last 32-column tile
LENS = [1, 2, 3, 6, 1, 4, 7]     # both parities in one chunk: the rollout start has rows to bring across
_MODELS = {}


def fitted(final_act='linear', layers=(30,), embed='constrained'):
    """A GRU4Rec fitted for one epoch on synthetic sessions that hold every one of N_ITEMS items (ids 10, 13, 16, ...)."""
    key = (final_act, tuple(layers), embed)
    if key not in _MODELS:
        rng = np.random.RandomState(sum(layers) + len(final_act))
        items = 10 + 3 * np.concatenate([rng.permutation(N_ITEMS), rng.randint(0, N_ITEMS, size=N_ITEMS)])
        sess = np.repeat(np.arange(len(items) // 5), 5)
        data = pd.DataFrame({'SessionId': sess, 'ItemId': items[:len(sess)], 'Time': np.arange(len(sess), dtype=np.int64)})
        sm = final_act.startswith('softmax')
        g = GRU4Rec(layers=list(layers), final_act=final_act, loss='cross-entropy' if sm else 'bpr-max', n_epochs=1, batch_size=32,
                    n_sample=0 if sm else 64, learning_rate=0.05, constrained_embedding=(embed == 'constrained'),
                    embedding=16 if embed == 'embedding' else 0)
        g.fit(data, sample_store=0 if sm else 100000)
        assert g.n_items == N_ITEMS
        _MODELS[key] = g
    return _MODELS[key]


def histories(g, lens, seed=0, pool=None):
    rng = np.random.RandomState(seed)
    ids = g.itemidmap.index.values if pool is None else pool
    return [ids[rng.randint(0, len(ids), size=n)] for n in lens]


def loop(g, hists, steps, k=1, no_repeat=True, cand=None, exclude=None, xpr=None, hidden=None, scan='fp32', oversample=8):
    """The contract's route, out of calls that exist without continue_sessions."""
    N = len(hists)
    kw = dict(k=k, exclude=exclude, predict_for_item_ids=cand, return_hidden=True, scan=scan, oversample=oversample)
    ids, sc, H = g.recommend_sessions(hists, exclude_history=no_repeat, exclude_per_row=xpr, hidden=hidden, **kw)
    all_ids, all_sc = [ids], [sc]
    gen = [[] for _ in hists]
    for s in range(1, steps):
        for i in range(N):
            gen[i].append(ids[i, 0])
        xs = [(list(hists[i]) + gen[i] if no_repeat else []) + (list(xpr[i]) if xpr is not None else []) for i in range(N)]
        if not any(len(x) for x in xs):
            xs = None
        ids, sc, H = g.recommend_sessions([[gen[i][-1]] for i in range(N)], exclude_per_row=xs, hidden=H, **kw)
        all_ids.append(ids)
        all_sc.append(sc)
    return np.stack(all_ids, axis=1), np.stack(all_sc, axis=1), H


def assert_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    assert a.shape == b.shape
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))


def check(g, hists, steps, k=1, no_repeat=True, cand=None, exclude=None, xpr=None, hidden=None, scan='fp32', oversample=8):
    items, scores, H = g.continue_sessions(hists, steps, k=k, no_repeat=no_repeat, predict_for_item_ids=cand, exclude=exclude,
                                           exclude_per_row=xpr, hidden=hidden, return_hidden=True, scan=scan, oversample=oversample)
    want_items, want_scores, want_H = loop(g, hists, steps, k, no_repeat, cand, exclude, xpr, hidden, scan, oversample)
    assert items.shape == scores.shape == (len(hists), steps, k) and scores.dtype == np.float32
    np.testing.assert_array_equal(items, want_items)
    assert_bits(scores, want_scores)
    assert len(H) == len(want_H) == len(g.layers)
    for a, b in zip(H, want_H):
        assert_bits(a, b)
    return items, scores, H


def assert_nothing_recurs(hists, items, xpr=None):
    """no_repeat: row i's lists never hold an item of its history, of its exclude_per_row, or one it has been fed before."""
    for i, h in enumerate(hists):
        gone = set(np.asarray(h).tolist()) | (set(xpr[i]) if xpr is not None else set())
        for s in range(items.shape[1]):
            assert not gone & set(items[i, s].tolist()), 'row %d step %d returns an excluded item' % (i, s)
            gone.add(items[i, s, 0])
        assert len(set(items[i, :, 0].tolist())) == items.shape[1]


@pytest.mark.parametrize('k', [1, 5])
@pytest.mark.parametrize('steps', [1, 2, 6])
def test_lengths_and_parities(steps, k):
    g = fitted()
    hists = histories(g, LENS, seed=1)
    items, scores, H = check(g, hists, steps, k=k)
    assert_nothing_recurs(hists, items)
    if steps == 1:
        ids1, sc1, H1 = g.recommend_sessions(hists, k=k, exclude_history=True, return_hidden=True)
        np.testing.assert_array_equal(items[:, 0], ids1)
        assert_bits(scores[:, 0], sc1)
        assert_bits(H[0], H1[0])


@pytest.mark.parametrize('layers', [(30,), (24, 12)])
@pytest.mark.parametrize('embed', ['onehot', 'embedding', 'constrained'])
def test_layers_and_inputs(layers, embed):
    g = fitted('linear', layers, embed)
    check(g, histories(g, LENS, seed=2), 4, k=5)


@pytest.mark.parametrize('final_act', ['linear', 'tanh', 'softmax', 'softmax_logit'])
def test_final_activations(final_act):
    g = fitted(final_act)
    check(g, histories(g, LENS, seed=3), 4, k=5)


def high_low(g):
    """(history pool, candidates): every candidate sorts above every history item, so a row's first generated item sorts above its
    whole exclusion list."""
    ids = g.itemidmap.index.values
    return ids[:500], ids[N_ITEMS - 40:]


@pytest.mark.parametrize('no_repeat', [True, False])
def test_no_repeat(no_repeat):
    g = fitted()
    pool, cand = high_low(g)
    hists = histories(g, LENS, seed=4, pool=pool)
    items, _, _ = check(g, hists, 6, k=30, no_repeat=no_repeat, cand=cand)      # True: the last step keeps 35 of 40 eligible
    if no_repeat:
        assert_nothing_recurs(hists, items)


@pytest.mark.parametrize('no_repeat', [True, False])
def test_no_repeat_over_all_items(no_repeat):
    g = fitted()
    hists = histories(g, LENS, seed=5)
    items, _, _ = check(g, hists, 6, k=5, no_repeat=no_repeat)
    if no_repeat:
        assert_nothing_recurs(hists, items)


@pytest.mark.parametrize('final_act', ['linear', 'softmax'])
def test_exclusions_with_no_repeat(final_act):
    g = fitted(final_act)
    ids = g.itemidmap.index.values
    hists = histories(g, LENS, seed=6)
    rng = np.random.RandomState(6)
    first = g.recommend_sessions(hists, k=8)[0]
    exclude = np.unique(first[:, :2])                                      # items that would otherwise be returned
    xpr = [list(first[i, 2:5]) + list(ids[rng.randint(0, N_ITEMS, size=i)]) for i in range(len(hists))]
    items, _, _ = check(g, hists, 5, k=5, exclude=exclude, xpr=xpr)
    assert_nothing_recurs(hists, items, xpr)
    assert not set(exclude.tolist()) & set(items.ravel().tolist())
    # the mask and the lists without no_repeat: nothing grows, the static lists still apply
    items, _, _ = check(g, hists, 5, k=5, exclude=exclude, xpr=xpr, no_repeat=False)
    assert not set(exclude.tolist()) & set(items.ravel().tolist())
    check(g, hists, 3, k=5, exclude=exclude)                               # a mask, and lists that start as the history alone


@pytest.mark.parametrize('no_repeat', [True, False])
def test_running_the_candidates_dry(no_repeat):
    g = fitted()
    ids = g.itemidmap.index.values
    pool, cand = ids[:500], ids[N_ITEMS - 12:]                             # 12 candidates, none of them in a history
    hists = histories(g, LENS, seed=7, pool=pool)
    items, scores, _ = check(g, hists, 8, k=5, no_repeat=no_repeat, cand=cand)      # True: the last step has exactly k eligible
    assert set(items.ravel().tolist()) <= set(cand.tolist())
    cols, _ = g._ensure_model().continue_sessions(*session_csr(g, hists), item_idx=g.itemidmap[cand].values, k=5, steps=8,
                                                  no_repeat=no_repeat, **history_lists(g, hists, no_repeat))
    assert cols.min() >= 0 and cols.max() < 12, 'a pad (column 0xFFFFFFFF) was returned'
    if no_repeat:
        assert_nothing_recurs(hists, items)
        for i in range(len(hists)):
            assert set(items[i, 7].tolist()) == set(cand.tolist()) - set(items[i, :7, 0].tolist())


def session_csr(g, hists):
    lens = [len(h) for h in hists]
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), g.itemidmap[np.concatenate(hists)].values.astype(np.int32)


def history_lists(g, hists, on):
    if not on:
        return {}
    rows = [np.unique(g.itemidmap[h].values) for h in hists]
    return dict(excl_offs=np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64),
                excl_items=np.concatenate(rows).astype(np.int32))


def test_a_forced_small_chunk_gives_the_same_bits(monkeypatch):
    g = fitted()
    hists = histories(g, LENS, seed=8)
    items, scores, H = g.continue_sessions(hists, 5, k=5, return_hidden=True)
    monkeypatch.setenv('G4R_SESSIONS_CHUNK', '3')
    items2, scores2, H2 = g.continue_sessions(hists, 5, k=5, return_hidden=True)
    np.testing.assert_array_equal(items2, items)
    assert_bits(scores2, scores)
    assert_bits(H2[0], H[0])
    check(g, hists, 5, k=5)                 # and the loop, chunked the same way


@pytest.mark.parametrize('final_act', ['linear', 'softmax'])
def test_more_than_one_row_block(final_act):
    g = fitted(final_act)
    lens = list(np.random.RandomState(9).randint(1, 8, size=130))
    hists = histories(g, lens, seed=9)
    items, _, _ = check(g, hists, 3, k=5)
    assert_nothing_recurs(hists, items)


@pytest.mark.parametrize('layers', [(30,), (24, 12)])
def test_hidden_in_and_out_compose(layers):
    g = fitted('linear', layers)
    hists = histories(g, LENS, seed=10)
    a, b = 3, 4
    items, scores, H = g.continue_sessions(hists, a + b, k=5, return_hidden=True)
    items_a, scores_a, H_a = check(g, hists, a, k=5)
    np.testing.assert_array_equal(items_a, items[:, :a])
    assert_bits(scores_a, scores[:, :a])
    xpr = [list(h) + list(items[i, :a, 0]) for i, h in enumerate(hists)]
    # H_a has not consumed the winner of step a - 1: fed as a one-item history, step 0 of the second call is step a of the first
    items_c, scores_c, H_c = g.continue_sessions([[items[i, a - 1, 0]] for i in range(len(hists))], b, k=5, hidden=H_a,
                                                 exclude_per_row=xpr, return_hidden=True)
    np.testing.assert_array_equal(items_c, items[:, a:])
    assert_bits(scores_c, scores[:, a:])
    for x, y in zip(H_c, H):
        assert_bits(x, y)


def test_two_stage_scan():
    g = fitted()
    hists = histories(g, LENS, seed=11)
    # k * oversample >= the number of candidates: every eligible item reaches stage 2, the result is the exact one
    items, scores, H = g.continue_sessions(hists, 4, k=5, scan='bf16', oversample=204, return_hidden=True)
    items32, scores32, H32 = g.continue_sessions(hists, 4, k=5, return_hidden=True)
    np.testing.assert_array_equal(items, items32)
    assert_bits(scores, scores32)
    assert_bits(H[0], H32[0])
    check(g, hists, 4, k=5, scan='bf16', oversample=8)                     # against the bf16 loop
    check(g, hists, 4, k=5, scan='bf16', oversample=8, no_repeat=False)

"""GRU4Rec.beam_sessions / g4r_beam_sessions against the host loop of its contract (loop, below): recommend_sessions on the histories
with k = beams, then per step ONE recommend_sessions call over all N x beams beams -- the one-item history [[last item]] from the
beam's own returned state, its own exclusion list -- and the beams x beams candidates of every session combined, ordered and rescaled
in NumPy float32 (combine_scores, best_extensions, rescale: the rule itself, tested on hand-made values in
test_beam_sessions_args.py).  Item ids, score bits and scale_exp must be equal."""
import numpy as np
import pandas as pd
import pytest

from gru4rec_amd.gru4rec import GRU4Rec

pytestmark = pytest.mark.gpu

N_ITEMS = 251           # a partial last 32-column tile
LENS = [1, 2, 3, 6, 1, 4, 5]     # both parities in one chunk: k_beam_expand reads both halves
SOFTMAX, ELU = ('softmax', (16,)), ('elu-0.5', (12, 20))      # (final_act, layers): one layer / two unaligned layers
_MODELS = {}
TINY = np.float32(2.0 ** -126)


def fitted(final_act='softmax', layers=(16,), variant=0):
    """A GRU4Rec fitted for one epoch on synthetic sessions that hold every one of N_ITEMS items (ids 10, 13, 16, ...); `variant`
    keys a copy of its own (a test that edits the weights)."""
    key = (final_act, tuple(layers), variant)
    if key not in _MODELS:
        rng = np.random.RandomState(sum(layers) + len(final_act))
        items = 10 + 3 * np.concatenate([rng.permutation(N_ITEMS), rng.randint(0, N_ITEMS, size=3 * N_ITEMS)])
        sess = np.repeat(np.arange(len(items) // 4), 4)
        data = pd.DataFrame({'SessionId': sess, 'ItemId': items[:len(sess)], 'Time': np.arange(len(sess), dtype=np.int64)})
        sm = final_act.startswith('softmax')
        g = GRU4Rec(layers=list(layers), final_act=final_act, loss='cross-entropy' if sm else 'bpr-max', n_epochs=1, batch_size=32,
                    n_sample=0 if sm else 64, learning_rate=0.05, constrained_embedding=True)
        g.fit(data, sample_store=0 if sm else 100000)
        assert g.n_items == N_ITEMS
        _MODELS[key] = g
    return _MODELS[key]


def histories(g, lens, seed=0, pool=None):
    rng = np.random.RandomState(seed)
    ids = g.itemidmap.index.values if pool is None else pool
    return [ids[rng.randint(0, len(ids), size=n)] for n in lens]


# ---- the rule, in NumPy float32 -------------------------------------------------------------------------------------------------------
def combine_scores(cum, x, combine):
    """Path score of an extension: 'sum' fl32(cum + x); 'product' fl32(cum * x), a magnitude below 2^-126 (NaN is not) -> 0.0."""
    cum, x = np.asarray(cum, dtype=np.float32), np.asarray(x, dtype=np.float32)
    with np.errstate(all='ignore'):
        if combine == 'sum':
            return np.add(cum, x, dtype=np.float32)
        p = np.multiply(cum, x, dtype=np.float32)
        return np.where(np.abs(p) < TINY, np.float32(0.0), p).astype(np.float32)


def best_extensions(p, w):
    """The w best positions of the path scores p: score descending, equal scores (-0.0 == 0.0) by the lower position, NaN last."""
    p = np.asarray(p, dtype=np.float32)
    return sorted(range(len(p)), key=lambda c: (1, 0.0, c) if np.isnan(p[c]) else (0, -float(p[c]), c))[:w]


def rescale(p):
    """'product', after a selection: m = p[0]; finite and > 0: m = g 2^e, 1 <= g < 2 -> (p 2^-e, e); otherwise (p, 0)."""
    p = np.asarray(p, dtype=np.float32)
    m = p[0]
    if not (np.isfinite(m) and m > 0):
        return p, 0
    _, x = np.frexp(m)
    e = int(x) - 1
    return np.ldexp(p, -e).astype(np.float32), e


# ---- the contract --------------------------------------------------------------------------------------------------------------------
def loop(g, hists, steps, beams, no_repeat=True, combine=None, cand=None, exclude=None, xpr=None, hidden=None, scan='fp32', oversample=8):
    """The host loop, out of recommend_sessions and NumPy alone: (paths, path_scores, step_scores, scale_exp,
    parents[steps - 1][N][beams], the number of selections in which two extensions of DIFFERENT beams with equal path scores were
    ranked next to each other among the winners and the first loser)."""
    N, W = len(hists), beams
    if combine is None:
        combine = 'product' if g.final_act.startswith('softmax') else 'sum'
    kw = dict(k=W, exclude=exclude, predict_for_item_ids=cand, return_hidden=True, scan=scan, oversample=oversample)
    ids, sc, H = g.recommend_sessions(hists, exclude_history=no_repeat, exclude_per_row=xpr, hidden=hidden, **kw)
    paths = [[[ids[n, i]] for i in range(W)] for n in range(N)]
    sscores = [[[sc[n, i]] for i in range(W)] for n in range(N)]
    cum = sc.astype(np.float32).copy()
    scale = np.zeros(N, dtype=np.int32)
    H = [np.repeat(h, W, axis=0) for h in H]              # beam (n, i) is row n W + i
    parents, ties = [], 0

    def rescale_all():
        if combine == 'product':
            for n in range(N):
                cum[n], e = rescale(cum[n])
                scale[n] += e
    rescale_all()
    for s in range(1, steps):
        rows = [[paths[n][b][-1]] for n in range(N) for b in range(W)]
        xs = [(list(hists[n]) + paths[n][b] if no_repeat else []) + (list(xpr[n]) if xpr is not None else []) for n in range(N) for b in range(W)]
        if not any(len(x) for x in xs):
            xs = None
        ids, sc, Hn = g.recommend_sessions(rows, exclude_per_row=xs, hidden=H, **kw)
        take, par = [], []
        for n in range(N):
            p = np.concatenate([combine_scores(cum[n, b], sc[n * W + b], combine) for b in range(W)])
            win = best_extensions(p, W)
            edge = best_extensions(p, W + 1)
            ties += any(p[c] == p[d] and c // W != d // W for c, d in zip(edge, edge[1:]))
            cum[n] = p[win]
            par.append([c // W for c in win])
            paths[n] = [paths[n][c // W] + [ids[n * W + c // W, c % W]] for c in win]
            sscores[n] = [sscores[n][c // W] + [sc[n * W + c // W, c % W]] for c in win]
            take += [n * W + c // W for c in win]
        H = [h[take] for h in Hn]
        parents.append(par)
        rescale_all()
    return np.array(paths), cum, np.array(sscores, dtype=np.float32), scale, np.array(parents).reshape(steps - 1, N, W), ties


def assert_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    assert a.shape == b.shape
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))


def check(g, hists, steps, beams, reparents=None, **kw):
    """beam_sessions == loop.  reparents True: the REFERENCE must re-parent somewhere (a beam whose parent is not the beam of the same
    rank), or the case says nothing about k_beam_advance's gather."""
    got = g.beam_sessions(hists, steps, beams=beams, **kw)
    want = loop(g, hists, steps, beams, **{{'predict_for_item_ids': 'cand', 'exclude_per_row': 'xpr'}.get(k, k): v for k, v in kw.items()})
    if reparents:
        assert (want[4] != np.arange(beams)).any(), 'no step of the reference re-parents: pick another seed'
    paths, path_scores, step_scores, scale_exp = got
    N = len(hists)
    assert paths.shape == step_scores.shape == (N, beams, steps) and path_scores.shape == (N, beams) and scale_exp.shape == (N,)
    assert path_scores.dtype == step_scores.dtype == np.float32 and scale_exp.dtype == np.int32
    np.testing.assert_array_equal(paths, want[0])
    assert_bits(path_scores, want[1])
    assert_bits(step_scores, want[2])
    np.testing.assert_array_equal(scale_exp, want[3])
    return got, want


def assert_paths_are_fresh(hists, paths, xpr=None):
    """no_repeat: no path holds an item of its session's history (or exclude_per_row) or an item twice."""
    for n, h in enumerate(hists):
        gone = set(np.asarray(h).tolist()) | (set(xpr[n]) if xpr is not None else set())
        for b in range(paths.shape[1]):
            p = paths[n, b].tolist()
            assert not gone & set(p), 'session %d beam %d holds an excluded item' % (n, b)
            assert len(set(p)) == len(p), 'session %d beam %d repeats an item' % (n, b)


# ---- equality with the loop ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('steps', [1, 2, 5])
@pytest.mark.parametrize('beams', [1, 3, 8])
@pytest.mark.parametrize('model', [SOFTMAX, ELU], ids=['softmax', 'elu'])
def test_lengths_beams_and_steps(model, beams, steps):
    g = fitted(*model)
    hists = histories(g, LENS, seed=1)
    (paths, _, _, scale_exp), _ = check(g, hists, steps, beams, reparents=(beams > 1 and steps == 5))
    assert_paths_are_fresh(hists, paths)
    if model is ELU:
        assert not scale_exp.any()


@pytest.mark.parametrize('no_repeat', [True, False])
@pytest.mark.parametrize('model,combine', [(SOFTMAX, 'product'), (SOFTMAX, 'sum'), (ELU, 'sum'), (('softmax', (12, 20)), 'product')],
                         ids=['softmax-product', 'softmax-sum', 'elu-sum', 'softmax2-product'])
def test_combine_modes_and_no_repeat(model, combine, no_repeat):
    g = fitted(*model)
    hists = histories(g, LENS, seed=2)
    (paths, _, _, _), _ = check(g, hists, 5, 3, reparents=True, combine=combine, no_repeat=no_repeat)
    if no_repeat:
        assert_paths_are_fresh(hists, paths)


@pytest.mark.parametrize('model', [SOFTMAX, ELU], ids=['softmax', 'elu'])
def test_candidates_exclusions_and_hidden(model):
    g = fitted(*model)
    ids = g.itemidmap.index.values
    hists = histories(g, LENS, seed=3)
    rng = np.random.RandomState(3)
    first = g.recommend_sessions(hists, k=8)[0]
    exclude = np.unique(first[:, :2])                                      # items that would otherwise be returned
    xpr = [list(first[n, 2:5]) + list(ids[rng.randint(0, N_ITEMS, size=n)]) for n in range(len(hists))]
    (paths, _, _, _), _ = check(g, hists, 4, 3, reparents=True, exclude=exclude, exclude_per_row=xpr)
    assert_paths_are_fresh(hists, paths, xpr)
    assert not set(exclude.tolist()) & set(paths.ravel().tolist())
    # the mask and the lists without no_repeat: the beams of a session share its one list
    (paths, _, _, _), _ = check(g, hists, 4, 3, exclude=exclude, exclude_per_row=xpr, no_repeat=False)
    assert not set(exclude.tolist()) & set(paths.ravel().tolist())
    check(g, hists, 3, 3, exclude=exclude, no_repeat=False)                # a mask alone
    cand = ids[rng.permutation(N_ITEMS)[:90]]                              # candidates in an order of their own
    (paths, _, _, _), _ = check(g, hists, 4, 3, predict_for_item_ids=cand)
    assert set(paths.ravel().tolist()) <= set(cand.tolist())
    check(g, hists, 4, 3, predict_for_item_ids=cand, exclude=exclude, exclude_per_row=xpr, no_repeat=False)
    hidden = [(rng.randn(len(hists), D) * 0.5).astype(np.float32) for D in g.layers]
    check(g, hists, 4, 3, hidden=hidden)


# ---- cross-checks ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('model', [SOFTMAX, ELU], ids=['softmax', 'elu'])
def test_one_beam_is_the_greedy_continuation(model):
    g = fitted(*model)
    hists = histories(g, LENS, seed=4)
    paths, path_scores, step_scores, _ = g.beam_sessions(hists, 5, beams=1)
    items, scores = g.continue_sessions(hists, 5, k=1)
    np.testing.assert_array_equal(paths[:, 0], items[:, :, 0])
    assert_bits(step_scores[:, 0], scores[:, :, 0])
    check(g, hists, 5, 1)


@pytest.mark.parametrize('model', [SOFTMAX, ELU], ids=['softmax', 'elu'])
def test_one_step_is_recommend_sessions(model):
    g = fitted(*model)
    hists = histories(g, LENS, seed=5)
    paths, path_scores, step_scores, scale_exp = g.beam_sessions(hists, 1, beams=8, combine='sum')
    ids, sc = g.recommend_sessions(hists, k=8, exclude_history=True)
    np.testing.assert_array_equal(paths[:, :, 0], ids)
    assert_bits(step_scores[:, :, 0], sc)
    assert_bits(path_scores, sc)
    assert not scale_exp.any()


# ---- chunks, ties, long products, dry candidates, the two-stage scan -------------------------------------------------------------------------
@pytest.mark.parametrize('chunk', ['3', '2'])
def test_a_forced_small_chunk_gives_the_same_bits(chunk, monkeypatch):
    g = fitted(*SOFTMAX)
    hists = histories(g, LENS, seed=6)
    one = g.beam_sessions(hists, 4, beams=3)
    monkeypatch.setenv('G4R_SESSIONS_CHUNK', chunk)                        # 7 sessions: chunks of 3 + 3 + 1, of 2 + 2 + 2 + 1
    many = g.beam_sessions(hists, 4, beams=3)
    np.testing.assert_array_equal(many[0], one[0])
    assert_bits(many[1], one[1])
    assert_bits(many[2], one[2])
    np.testing.assert_array_equal(many[3], one[3])
    check(g, hists, 4, 3)                                                  # and the loop, chunked the same way


@pytest.mark.parametrize('no_repeat', [False, True])
@pytest.mark.parametrize('model', [SOFTMAX, ELU], ids=['softmax', 'elu'])
def test_equal_path_scores_follow_the_position_rule(model, no_repeat):
    """For every session, item b is made a copy of item a (output row, bias and, the embedding being constrained, input row), a the
    session's best next item and b its second best: the beams through a and through b carry equal path scores and equal candidates,
    so which of two equal extensions is ranked first -- or survives the cut -- is decided by b * beams + j alone."""
    g = fitted(*model, variant=1)
    hists = histories(g, LENS, seed=7)
    if not getattr(g, '_twins', None):
        Wy, By, used = g.Wy.copy(), g.By.copy(), set()
        for top in g.recommend_sessions(hists, k=2)[0]:
            a, b = g.itemidmap[top].values
            if not {a, b} & used:
                Wy[b], By[b] = Wy[a], By[a]
                used |= {a, b}
        g.Wy, g.By = Wy, By
        g._dev_put(g._ensure_model(), 'Wy', g.Wy)
        g._dev_put(g._ensure_model(), 'By', g.By.reshape(-1))
        g._twins = used
    for beams in (2, 3):
        _, want = check(g, hists, 3, beams, no_repeat=no_repeat)
        assert want[5] > 0, 'no selection of the reference had to order two equal extensions of different beams'


def test_a_long_product_stays_representable():
    g = fitted(*SOFTMAX)
    hists = histories(g, LENS, seed=8)
    (_, path_scores, _, scale_exp), want = check(g, hists, 24, 3, reparents=True)
    assert (want[3] < -126).all(), 'the plain product would still be a normal float32: %s' % want[3]
    assert ((path_scores[:, 0] >= 1) & (path_scores[:, 0] < 2)).all()


def test_running_the_candidates_nearly_dry():
    g = fitted(*SOFTMAX)
    ids = g.itemidmap.index.values
    pool, cand = ids[:150], ids[N_ITEMS - 12:]                             # 12 candidates, none of them in a history: 8 + 5 - 1
    hists = histories(g, LENS, seed=9, pool=pool)
    (paths, _, _, _), _ = check(g, hists, 5, 8, reparents=True, predict_for_item_ids=cand)
    assert set(paths.ravel().tolist()) <= set(cand.tolist())
    assert_paths_are_fresh(hists, paths)
    with pytest.raises(ValueError, match='eligible'):
        g.beam_sessions(hists, 6, beams=8, predict_for_item_ids=cand)


def test_two_stage_scan():
    g = fitted(*ELU)
    hists = histories(g, LENS, seed=10)
    check(g, hists, 4, 3, reparents=True, scan='bf16', oversample=8)       # against the loop run with scan='bf16'
    check(g, hists, 4, 3, scan='bf16', oversample=8, no_repeat=False)

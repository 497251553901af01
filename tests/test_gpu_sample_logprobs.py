"""Log-probabilities and nucleus sampling of GRU4Rec.sample_sessions, and GRU4Rec.session_log_partition, on the device against the
contract (the docstring of sample_sessions; the host twin is tests/logprob_ref.py).
  terms        g4r_debug_lse_terms against the float64 twin;
  Q            session_log_partition's raw (zeta, Q) equal, AS INTEGERS, to the twin's sum of the device terms over the eligible
               positions of z = score_candidates_sessions' bits;
  values       lse and logprobs against a float64 evaluation on the same z bits (softmax models: z recomputed from the weights);
  host loop    sampling_ref.host_loop extended by zeta, the terms, Q / C_t / m: items, score bits and hidden bits equal, logprobs
               within 1 ulp (the device's log against NumPy's);
  identities, invariance (chunks, row blocks, chaining), and the distribution inside a nucleus."""
import numpy as np
import pandas as pd
import pytest

import logprob_ref as lref
import sampling_ref as ref
from gru4rec_amd.gru4rec import GRU4Rec
from test_gpu_continue_sessions import LENS, N_ITEMS, assert_bits, fitted, histories

pytestmark = pytest.mark.gpu

TEMPERATURES = (1.0, 0.5, 3.0, 0.004)


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x)).astype(np.float32)).astype(np.float64)


def inv_t32(temperature):
    return np.float32(1.0) / np.float32(temperature)


def device_terms(g):
    m = g._ensure_model()
    return lambda z, zeta, inv_t: m.debug_lse_terms(z, zeta, inv_t)


def device_noise(g):
    m = g._ensure_model()
    return lambda seed, q, step, items: m.debug_gumbel(seed, q, step, items)


# ------------------------------------------------------------------------------------------------ 1. terms
def test_terms():
    g = fitted()
    terms = device_terms(g)
    d = -np.linspace(0.0, 30.0, 4001).astype(np.float32)
    q = terms(d, 0.0, 1.0)
    assert q.dtype == np.uint64 and int(q[0]) == 2 ** 39, 'd = 0 must give 2^39 exactly'
    assert (np.diff(q.astype(np.int64)) <= 0).all(), 'the terms rise somewhere as d falls'
    assert (q[d < -28.0] == 0).all() and (q[d > -26.0] > 0).all()
    # the bound: expf to 1 ulp, doubled as noise_bound doubles, + the rounding to an integer
    worst = 0.0
    rng = np.random.RandomState(0)
    for z, zeta, inv_t in ((d, np.float32(0.0), np.float32(1.0)),
                           (rng.randn(4096).astype(np.float32), np.float32(3.25), inv_t32(3.0)),
                           (rng.randn(4096).astype(np.float32) * 0.01, np.float32(0.031), inv_t32(0.004)),
                           (rng.randn(4096).astype(np.float32) * 5, rng.randn(4096).astype(np.float32) + 20, inv_t32(0.7))):
        want = lref.q64(lref.d32(z, zeta, inv_t))                 # d: the twin's two float32 roundings
        err = np.abs(terms(z, zeta, inv_t).astype(np.float64) - want)
        bound = want * (2 * 2.0 ** -23) + 0.5
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), 'largest error %.6g at %d' % (err.max(), err.argmax())
    print('terms: largest error / bound = %.3f' % worst)
    bad = terms(np.array([np.nan, -np.inf, 1.0, -np.inf], dtype=np.float32), np.array([0.0, 0.0, np.nan, -np.inf], dtype=np.float32), 1.0)
    assert bad.tolist() == [0, 0, 0, 0]                           # (-inf - -inf is NaN too)


# ------------------------------------------------------------------------------------------------ 2. Q is exact
def raw_partition(g, hists, temperature=1.0, cand=None, exclude_history=False, exclude=None, xpr=None, hidden=None):
    """(zeta, Q) as the device returns them: session_log_partition's own packing, without its last line."""
    N, lens, offs, hidx, h0 = g._session_inputs(hists, hidden)
    iidx, _ = g._candidates(cand)
    excl = g._session_exclusions(N, lens, hidx, 1, iidx, exclude_history, exclude, xpr)
    return g._ensure_model().session_log_partition(offs, hidx, iidx, float(np.float32(temperature)), *excl, hidden=h0)


def check_partition(g, hists, cand=None, exclude_history=False, exclude=None, xpr=None, hidden=None, temperatures=TEMPERATURES):
    cand_ids = g.itemidmap.index.values if cand is None else np.asarray(cand)
    Z = np.asarray(g.score_candidates_sessions(hists, np.tile(cand_ids, (len(hists), 1)), hidden=hidden), dtype=np.float32)
    on = lref.eligibility(g, hists, cand_ids, exclude_history, exclude, xpr)
    terms = device_terms(g)
    kw = dict(cand=cand, exclude_history=exclude_history, exclude=exclude, xpr=xpr, hidden=hidden)
    for t in temperatures:
        zeta, Q = raw_partition(g, hists, t, **kw)
        assert zeta.dtype == np.float32 and Q.dtype == np.uint64
        lse = g.session_log_partition(hists, temperature=t, predict_for_item_ids=cand, exclude_history=exclude_history, exclude=exclude,
                                      exclude_per_row=xpr, hidden=hidden)
        for i in range(len(hists)):
            want_zeta = Z[i][ref.order(Z[i], on[i])[0]]
            assert_bits(zeta[i], want_zeta)
            want_Q = lref.total(terms(Z[i], want_zeta, inv_t32(t))[on[i]])
            assert int(Q[i]) == want_Q, 'T = %g, session %d: Q = %d, the eligible terms sum to %d (difference %d)' % (
                t, i, int(Q[i]), want_Q, int(Q[i]) - want_Q)
            assert_bits(lse[i], lref.lse(want_zeta, inv_t32(t), want_Q))


def _lists(g, seed=5):
    ids = g.itemidmap.index.values
    rng = np.random.RandomState(seed)
    return rng.permutation(ids)[:200], [rng.permutation(ids)[:n] for n in (0, 5, 40, 1, 0, 300, 2)]


def test_q_without_exclusions():
    g = fitted()
    check_partition(g, histories(g, LENS, seed=21))


def test_q_with_the_history_excluded():
    g = fitted()
    check_partition(g, histories(g, LENS, seed=22), exclude_history=True)


def test_q_with_a_mask_and_lists():
    g = fitted()
    exclude, xpr = _lists(g)
    check_partition(g, histories(g, LENS, seed=23), exclude=exclude, xpr=xpr)
    check_partition(g, histories(g, LENS, seed=23), xpr=xpr, temperatures=(1.0,))


def test_q_with_lists_at_the_edges_of_the_catalogue():
    """Item index 1002 closes a list (the partial last tile: columns 992 .. 1002), item index 0 opens one, and lists take the first and
    the last column of a 32-column tile."""
    g = fitted()
    ids = g.itemidmap.index.values
    xpr = [ids[[5, 500, 1002]], ids[[0, 31, 32]], ids[[0, 1002]], ids[[991, 992]], [], ids[np.arange(960, 1003)], ids[[63, 64, 1001]]]
    check_partition(g, histories(g, LENS, seed=24), xpr=xpr)
    check_partition(g, histories(g, LENS, seed=24), xpr=xpr, exclude_history=True, exclude=ids[[1, 1002]], temperatures=(0.5,))


def test_q_over_candidate_lists():
    g = fitted()
    ids = g.itemidmap.index.values
    rng = np.random.RandomState(25)
    cand = rng.permutation(ids)[:333]                      # ten full tiles and a partial one
    exclude, xpr = _lists(g, seed=26)
    hists = histories(g, LENS, seed=25, pool=cand)
    check_partition(g, hists, cand=cand)
    check_partition(g, hists, cand=cand, exclude_history=True, exclude=exclude[:50], xpr=xpr)
    # a list that names one item twice: both positions count (or both go)
    dup = np.concatenate([cand[:40], cand[7:8], cand[40:70], cand[69:70]])
    check_partition(g, hists, cand=dup, temperatures=(1.0, 0.5))
    check_partition(g, hists, cand=dup, xpr=[cand[[7, 69]], cand[[7]], [], cand[[69, 3]], [], cand[:30], []], temperatures=(1.0, 3.0))


def test_q_from_a_supplied_hidden_state():
    g = fitted('linear', (24, 12))
    rng = np.random.RandomState(27)
    H0 = [rng.randn(len(LENS), D).astype(np.float32) * 0.3 for D in g.layers]
    check_partition(g, histories(g, LENS, seed=27), hidden=H0, exclude_history=True, temperatures=(1.0, 0.5))


# ------------------------------------------------------------------------------------------------ 3. float values
def value_bound(n_e, d_c, value):
    """|device - float64| allowed.  Two fp32 roundings of d on terms that still count (|d| <= 27.1: 2 * 27.1 * 2^-24 = 3.2e-6) and expf
    to 1 ulp (1.2e-7): 3.5e-6 relative on every term, so on the sum and absolute on its logarithm; n_E 2^-39 for the quantisation and
    the dropped terms (each at most 1 in units of 2^-39, against a sum of at least 2^39 of them); 2^-23 |d_c| for the two roundings of
    the chosen d; the final rounding; a margin factor of 2."""
    return 2 * (3.5e-6 + n_e * 2.0 ** -39 + 2.0 ** -23 * np.abs(d_c)) + ulp32(value)


@pytest.mark.parametrize('temperature', TEMPERATURES)
def test_values_against_float64(temperature):
    g = fitted('elu-0.5')
    ids = g.itemidmap.index.values
    hists = histories(g, LENS, seed=31)
    it = np.float64(inv_t32(temperature))
    Z = np.asarray(g.score_candidates_sessions(hists, np.tile(ids, (len(hists), 1))), dtype=np.float32)
    on = lref.eligibility(g, hists, ids, True, None, None)
    x = Z.astype(np.float64) * it

    def lse64(i, keep):
        v = x[i][keep]
        return v.max() + np.log(np.exp(v - v.max()).sum())
    lse = g.session_log_partition(hists, temperature=temperature, exclude_history=True)
    worst = 0.0
    for i in range(len(hists)):
        want = lse64(i, on[i])
        err, bound = abs(float(lse[i]) - want), value_bound(on[i].sum(), 0.0, want)
        worst = max(worst, err / bound)
        assert err <= bound, 'lse of session %d: %.9g against %.9g' % (i, lse[i], want)
    # one step, so that every draw's eligible set is the session's: untruncated, top_k, top_k + top_p
    S = 4
    for top_k, top_p in ((None, None), (20, None), (20, 0.7)):
        items, scores, lp = g.sample_sessions(hists, 1, samples=S, temperature=temperature, top_k=top_k, top_p=top_p, seed=5, return_logprobs=True)
        for i in range(len(hists)):
            keep = on[i]
            if top_k is not None:
                best = ref.order(Z[i], on[i])[:top_k]
                m = top_k
                if top_p is not None:
                    p = np.exp(x[i][best] - lse64(i, on[i]))
                    reached = np.flatnonzero(np.cumsum(p) >= np.float64(np.float32(top_p)))
                    m = int(reached[0]) + 1 if len(reached) else top_k
                    # (the device may cut one entry earlier or later where the mass meets top_p within the error: not at these shapes)
                    assert abs(np.cumsum(p)[m - 1] - np.float32(top_p)) > 1e-4
                keep = np.zeros(len(ids), dtype=bool)
                keep[best[:m]] = True
            for j in range(S):
                c = int(g.itemidmap[items[i, j, 0]])
                assert keep[c]
                want = x[i, c] - lse64(i, keep)
                d_c = x[i, c] - x[i][on[i]].max()
                err, bound = abs(float(lp[i, j, 0]) - want), value_bound(keep.sum(), d_c, want)
                worst = max(worst, err / bound)
                assert err <= bound, 'draw (%d, %d) top_k %s top_p %s: logprob %.9g against %.9g' % (i, j, top_k, top_p, lp[i, j, 0], want)
    print('T = %g: largest error / bound = %.3f' % (temperature, worst))


@pytest.mark.parametrize('final_act', ['softmax', 'softmax_logit'])
def test_values_of_softmax_models(final_act):
    """z is the pre-activation value, which no public call returns: recomputed in float64 from the weights and the returned state as in
    test_softmax_models_sample_on_the_logit, the bound widened by that test's dot-product bound on the chosen z and on the others."""
    g = fitted(final_act)
    D = g.layers[-1]
    Wy, By = g.Wy.astype(np.float64), g.By.reshape(-1).astype(np.float64)
    hists = histories(g, [1, 2, 3, 6, 1, 4, 7] * 3, seed=32)
    S, temperature = 2, 0.5
    it = np.float64(inv_t32(temperature))
    worst = 0.0
    for steps in (1, 3):
        items, scores, H, lp = g.sample_sessions(hists, steps, samples=S, temperature=temperature, seed=78, return_hidden=True, return_logprobs=True)
        s = steps - 1
        for i, h in enumerate(hists):
            for j in range(S):
                prod = Wy * H[-1][i, j].astype(np.float64)[None, :]
                z64 = prod.sum(axis=1) + By
                e = it * (D + 2) * 2.0 ** -24 * (np.abs(prod).sum(axis=1) + np.abs(By))
                gone = set(np.asarray(h).tolist()) | set(items[i, j, :s].tolist())
                on = ~np.isin(g.itemidmap.index.values, list(gone))
                c = int(g.itemidmap[items[i, j, s]])
                v = z64[on] * it
                want = z64[c] * it - (v.max() + np.log(np.exp(v - v.max()).sum()))
                err = abs(float(lp[i, j, s]) - want)
                bound = value_bound(on.sum(), z64[c] * it - v.max(), want) + e[c] + e[on].max()
                worst = max(worst, err / bound)
                assert err <= bound, 'draw (%d, %d): logprob %.9g against %.9g' % (i, j, lp[i, j, s], want)
    print('%s: largest error / bound = %.3f' % (final_act, worst))


# ------------------------------------------------------------------------------------------------ 4. the host-loop twin
def check(g, hists, steps, samples=1, temperature=1.0, top_k=None, top_p=None, seed=3, first_step=0, no_repeat=True, cand=None, exclude=None,
          xpr=None, hidden=None):
    kw = dict(samples=samples, temperature=temperature, top_k=top_k, top_p=top_p, seed=seed, first_step=first_step, no_repeat=no_repeat,
              exclude=exclude, hidden=hidden)
    items, scores, H, lp = g.sample_sessions(hists, steps, predict_for_item_ids=cand, exclude_per_row=xpr, return_hidden=True,
                                             return_logprobs=True, **kw)
    want_items, want_scores, want_H, want_lp = lref.host_loop(g, hists, steps, cand=cand, xpr=xpr, noise=device_noise(g), terms=device_terms(g),
                                                              **kw)
    assert items.shape == scores.shape == lp.shape == (len(hists), samples, steps) and lp.dtype == np.float32
    np.testing.assert_array_equal(items, want_items)
    assert_bits(scores, want_scores)
    for a, b in zip(H, want_H):
        assert_bits(a, b)
    assert (np.abs(lp.astype(np.float64) - want_lp.astype(np.float64)) <= ulp32(want_lp)).all(), \
        'logprobs more than 1 ulp from the twin: largest difference %.3g' % np.abs(lp.astype(np.float64) - want_lp).max()
    assert (lp <= 0).all()
    if top_p is None:      # the log-probabilities change nothing else
        plain = g.sample_sessions(hists, steps, predict_for_item_ids=cand, exclude_per_row=xpr, return_hidden=True, **dict(kw, top_p=None))
        np.testing.assert_array_equal(items, plain[0])
        assert_bits(scores, plain[1])
        for a, b in zip(H, plain[2]):
            assert_bits(a, b)
    return items, scores, H, lp


MODES = [(None, None), (1, None), (5, None), (256, None)] + [(t, p) for t in (5, 256) for p in (0.3, 0.9, 1.0)]


@pytest.mark.parametrize('temperature', [0.5, 0.004])
@pytest.mark.parametrize('top_k,top_p', MODES)
def test_host_loop(top_k, top_p, temperature):
    g = fitted()
    hists = histories(g, LENS, seed=41)
    for steps in (1, 2, 5):
        for samples in (1, 3):
            for no_repeat in (True, False):
                check(g, hists, steps, samples=samples, temperature=temperature, top_k=top_k, top_p=top_p, no_repeat=no_repeat,
                      seed=1000 * steps + samples)


def test_host_loop_with_candidates_lists_and_hidden():
    g = fitted()
    ids = g.itemidmap.index.values
    rng = np.random.RandomState(42)
    cand = rng.permutation(ids)[:333]
    hists = histories(g, LENS, seed=42, pool=cand)
    exclude, xpr = _lists(g, seed=43)
    check(g, hists, 3, samples=2, cand=cand)
    check(g, hists, 3, samples=2, cand=cand, top_k=9, top_p=0.6, exclude=exclude[:50], xpr=xpr, first_step=7)
    check(g, hists, 2, samples=2, exclude=exclude, xpr=xpr, no_repeat=False)
    H0 = [rng.randn(len(LENS), D).astype(np.float32) * 0.3 for D in g.layers]
    check(g, histories(g, LENS, seed=44), 2, samples=2, hidden=H0, top_k=30, top_p=0.5)


# ------------------------------------------------------------------------------------------------ 5. identities
def _same(a, b):
    assert len(a) == len(b)
    np.testing.assert_array_equal(a[0], b[0])
    assert_bits(a[1], b[1])
    for x, y in zip(a[2], b[2]):
        assert_bits(x, y)
    assert_bits(a[3], b[3])


def test_identities():
    g = fitted()
    hists = histories(g, LENS, seed=51)
    kw = dict(samples=3, temperature=0.5, seed=17, return_hidden=True, return_logprobs=True)
    for t in (5, 256):
        _same(g.sample_sessions(hists, 5, top_k=t, top_p=1.0, **kw), g.sample_sessions(hists, 5, top_k=t, **kw))
    a = g.sample_sessions(hists, 5, top_k=40, top_p=1e-6, **kw)
    b = g.sample_sessions(hists, 5, top_k=1, **kw)
    _same(a[:3] + (a[3] * 0,), b[:3] + (b[3] * 0,))
    assert (a[3] == 0.0).all() and (b[3] == 0.0).all()
    c = g.continue_sessions(hists, 5, k=1)
    np.testing.assert_array_equal(a[0][:, 0], c[0][..., 0])


# ------------------------------------------------------------------------------------------------ 6. invariance
@pytest.mark.parametrize('top_k,top_p', [(None, None), (5, None), (40, 0.8)])
def test_the_call_twice_and_in_chunks(monkeypatch, top_k, top_p):
    g = fitted()
    hists = histories(g, LENS, seed=61)
    kw = dict(samples=3, temperature=0.5, seed=41, top_k=top_k, top_p=top_p, return_hidden=True, return_logprobs=True)
    a = g.sample_sessions(hists, 5, **kw)
    _same(a, g.sample_sessions(hists, 5, **kw))
    for chunk in ('3', '1'):
        monkeypatch.setenv('G4R_SESSIONS_CHUNK', chunk)
        _same(a, g.sample_sessions(hists, 5, **kw))
    monkeypatch.delenv('G4R_SESSIONS_CHUNK')


def test_a_session_alone_and_among_130():
    g = fitted()
    hists = histories(g, [1 + (i * 7) % 5 for i in range(130)], seed=62)
    for t in (1.0, 0.004):
        zeta, Q = raw_partition(g, hists, t, exclude_history=True)
        for i in (0, 77, 129):
            z1, Q1 = raw_partition(g, hists[i:i + 1], t, exclude_history=True)
            assert_bits(z1[0], zeta[i])
            assert int(Q1[0]) == int(Q[i])
    lse = g.session_log_partition(hists, exclude_history=True)
    assert_bits(g.session_log_partition(hists[77:78], exclude_history=True), lse[77:78])


_BIG = {}


def big_model():
    if 'g' not in _BIG:
        n_items = 4099
        rng = np.random.RandomState(12)
        ev = 10 + 3 * np.concatenate([rng.permutation(n_items), rng.randint(0, n_items, size=n_items)])
        sess = np.repeat(np.arange(len(ev) // 5), 5)
        data = pd.DataFrame({'SessionId': sess, 'ItemId': ev[:len(sess)], 'Time': np.arange(len(sess), dtype=np.int64)})
        g = GRU4Rec(layers=[30], final_act='linear', loss='bpr-max', n_epochs=1, batch_size=32, n_sample=64, learning_rate=0.05)
        g.fit(data, sample_store=100000)
        assert g.n_items == n_items
        _BIG['g'] = g
    return _BIG['g']


@pytest.mark.parametrize('top_k,top_p', [(None, None), (50, 0.9)])
def test_several_tiles_per_range_and_row_blocks(monkeypatch, top_k, top_p):
    """4,099 items, 130 sessions x 3 samples = 390 draw rows: 4 row blocks, several 32-column tiles per range -- against one session per
    chunk (other ranges: another order of the same integer sum) and against the twin."""
    g = big_model()
    hists = histories(g, [1 + (i * 7) % 5 for i in range(130)], seed=12)
    a = check(g, hists, 2, samples=3, temperature=0.5, seed=99, top_k=top_k, top_p=top_p)
    monkeypatch.setenv('G4R_SESSIONS_CHUNK', '1')
    b = g.sample_sessions(hists, 2, samples=3, temperature=0.5, seed=99, top_k=top_k, top_p=top_p, return_hidden=True, return_logprobs=True)
    monkeypatch.delenv('G4R_SESSIONS_CHUNK')
    _same(a, b)


@pytest.mark.parametrize('top_k,top_p', [(None, None), (5, None), (30, 0.9)])
def test_chaining(top_k, top_p):
    g = fitted()
    a, b, S = 2, 3, 3
    hists = histories(g, LENS, seed=11)
    kw = dict(temperature=0.5, seed=2 ** 33 + 7, top_k=top_k, top_p=top_p, return_hidden=True, return_logprobs=True)
    items, scores, H, lp = g.sample_sessions(hists, a + b, samples=S, **kw)
    items_a, scores_a, H_a, lp_a = g.sample_sessions(hists, a, samples=S, **kw)
    np.testing.assert_array_equal(items_a, items[..., :a])
    assert_bits(lp_a, lp[..., :a])
    N = len(hists)
    flat = items.reshape(N * S, a + b)
    xpr = [list(hists[q // S]) + flat[q, :a].tolist() for q in range(N * S)]
    items_b, scores_b, H_b, lp_b = g.sample_sessions([[x] for x in flat[:, a - 1]], b, samples=1, first_step=a, no_repeat=True, exclude_per_row=xpr,
                                                     hidden=[h.reshape(N * S, -1) for h in H_a], **kw)
    np.testing.assert_array_equal(items_b.reshape(N, S, b), items[..., a:])
    assert_bits(scores_b.reshape(N, S, b), scores[..., a:])
    assert_bits(lp_b.reshape(N, S, b), lp[..., a:])
    for x, y in zip(H_b, H):
        assert_bits(x.reshape(N, S, -1), y)


# ------------------------------------------------------------------------------------------------ 7. distribution
CHI2_999 = {1: 10.83, 2: 13.82, 3: 16.27, 4: 18.47, 5: 20.52, 6: 22.46, 7: 24.32}      # chi-square quantiles at p = 0.001 by degrees of freedom


@pytest.mark.parametrize('seed', [1, 2 ** 33 + 9])
def test_distribution_inside_the_nucleus(seed):
    g = fitted()
    ids = g.itemidmap.index.values
    cand = ids[[5, 100, 333, 334, 640, 801, 900, 1002]]
    cidx = g.itemidmap[cand].values
    hist = [[ids[17]]]
    z = np.asarray(g.score_candidates_sessions(hist, cand[None, :]), dtype=np.float32)[0]
    on = np.ones(8, dtype=bool)
    by_z = ref.order(z, on)
    qb = [int(x) for x in device_terms(g)(z[by_z], z[by_z[0]], 1.0)]
    m, _ = lref.nucleus(qb, 0.8, sum(qb))
    assert 2 <= m, 'the nucleus is a single item: nothing to test'
    nuc = np.zeros(8, dtype=bool)
    nuc[by_z[:m]] = True
    items, _ = g.sample_sessions(hist * 512, 1, samples=8, seed=seed, no_repeat=False, predict_for_item_ids=cand, top_k=8, top_p=0.8)
    counts = np.array([(items == c).sum() for c in cand])
    assert counts.sum() == 4096
    assert counts[~nuc].sum() == 0, 'draws outside the nucleus: %s, nucleus %s' % (counts.tolist(), nuc.tolist())
    p = ref.softmax64(z[nuc])
    want = np.zeros(8, dtype=np.int64)
    for q in range(4096):
        want[ref.choose(z, ref.g64(seed, q, 0, cidx).astype(np.float32), np.float32(1.0), nuc)] += 1
    chi, chi_ref = ref.chi_square(counts[nuc], p), ref.chi_square(want[nuc], p)
    print('seed %d: nucleus of %d, p %s\n device %s chi-square %.2f\n reference %s chi-square %.2f' % (
        seed, m, np.round(p, 4).tolist(), counts[nuc].tolist(), chi, want[nuc].tolist(), chi_ref))
    assert chi_ref <= CHI2_999[m - 1]
    assert chi <= CHI2_999[m - 1]

"""GRU4Rec.audience_sessions / g4r_audience_sessions -- for each of M items the k sessions with the largest value -- against host loops
over existing calls.  by='score': the N x M matrix of score_candidates_sessions, ineligible pairs removed, one stable sort per column;
sessions, value bits and counts must be equal.  by='logprob': the twin is session_log_likelihood on every history followed by the item
(its last event), whose float64 logarithm may differ from the device's in the last place, so values are compared within one float32
ulp and the selection is checked against the returned values themselves.  Both: the result does not depend on the chunking, on how
the sessions are split over calls or on their order; `hidden` continues a session; the prediction state is left alone."""
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
N_ITEMS = 301      # no multiple of 4 or 64
_MODELS = {}
_CACHE = {}


def fitted(final_act='linear', layers=(20,), str_ids=False):
    """A GRU4Rec fitted for one epoch on synthetic sessions that hold every one of N_ITEMS items (ids 10, 13, 16, ...; str_ids: as
    strings, what run.py reads from a file)."""
    key = (final_act, tuple(layers), str_ids)
    if key not in _MODELS:
        rng = np.random.RandomState(sum(layers) + len(final_act))
        items = 10 + 3 * np.concatenate([rng.permutation(N_ITEMS), rng.randint(0, N_ITEMS, size=N_ITEMS)])
        sess = np.repeat(np.arange(len(items) // 5), 5)
        data = pd.DataFrame({'SessionId': sess, 'ItemId': items[:len(sess)], 'Time': np.arange(len(sess), dtype=np.int64)})
        if str_ids:
            data['ItemId'] = data['ItemId'].astype(str)
        sm = final_act.startswith('softmax')
        g = GRU4Rec(layers=list(layers), final_act=final_act, loss='cross-entropy' if sm else 'bpr-max', n_epochs=1, batch_size=32,
                    n_sample=0 if sm else 64, learning_rate=0.05)
        g.fit(data, sample_store=0 if sm else 10000)
        assert g.n_items == N_ITEMS
        _MODELS[key] = g
    return _MODELS[key]


def histories(n, seed=0, duplicates=True):
    """n histories of 1 to 9 items over the ids of the fitted models.  duplicates: every seventh history from index 3 on repeats the
    history 3 before it, and the last ones repeat the first ones -- equal values in one chunk and across chunk boundaries; without them
    the histories hold 3 to 9 items and are distinct."""
    rng = np.random.RandomState(100 + seed)
    ids = 10 + 3 * np.arange(N_ITEMS)
    h = [list(ids[rng.randint(0, N_ITEMS, size=rng.randint(1 if duplicates else 3, 10))]) for _ in range(n)]
    if duplicates:
        for i in range(3, n, 7):
            h[i] = list(h[i - 3])
        for i in range(min(5, n // 2)):
            h[n - 1 - i] = list(h[i])
    else:
        assert len(set(map(tuple, h))) == n
    return h


def item_list(M, seed=0):
    """M item ids with a duplicate position (M >= 5) and, first, ids that lie in many histories."""
    rng = np.random.RandomState(200 + seed)
    it = list(10 + 3 * rng.permutation(N_ITEMS)[:M])
    if M >= 5:
        it[4] = it[1]
    return it


def order(vals, idx):
    """positions sorted value descending (float ==), then index ascending, NaN last"""
    nan = np.isnan(vals)
    return np.lexsort((idx, np.where(nan, 0, -vals), nan))


def host_audience(V, elig, k):
    """the host loop: column j of the value matrix V[N, M] without the ineligible sessions, sorted, cut at k and padded"""
    N, M = V.shape
    S = np.full((M, k), -1, dtype=np.int64)
    W = np.full((M, k), np.nan, dtype=np.float32)
    C = np.zeros(M, dtype=np.int32)
    for j in range(M):
        idx = np.flatnonzero(elig[:, j])
        o = idx[order(V[idx, j], idx)][:k]
        C[j] = len(o)
        S[j, :len(o)] = o
        W[j, :len(o)] = V[o, j]
    return S, W, C


def held(hists, items):
    """held[i, j]: history i holds items[j]"""
    return np.array([[it in set(h) for it in items] for h in hists], dtype=bool)


def score_matrix(g, hists, items, tag):
    key = ('score', id(g), tag)
    if key not in _CACHE:
        _CACHE[key] = g.score_candidates_sessions(hists, np.tile(np.asarray(items), (len(hists), 1)))
    return _CACHE[key]


def assert_same(got, want):
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(np.ascontiguousarray(got[1]).view(np.uint32), np.ascontiguousarray(want[1]).view(np.uint32))
    np.testing.assert_array_equal(got[2], want[2])
    assert got[0].dtype == np.int64 and got[1].dtype == np.float32 and got[2].dtype == np.int32


SCORE_MODELS = [('linear', (20,)), ('tanh', (20,)), ('relu', (20,)), ('linear', (24, 16)), ('relu', (24, 16))]


# ---- by='score' ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,chunk', [(1, None), (37, None), (600, None), (600, 16)])      # 600: the native 512-row boundary, a forced one
@pytest.mark.parametrize('final_act,layers', SCORE_MODELS)
def test_scores_equal_the_host_loop(final_act, layers, N, chunk, monkeypatch):
    g = fitted(final_act, layers)
    hists = histories(N, seed=N)
    all_items = item_list(70)
    V = score_matrix(g, hists, all_items, (N, 70))
    H = held(hists, all_items)
    if chunk is not None:
        monkeypatch.setenv('G4R_SESSIONS_CHUNK', str(chunk))
    for M in (1, 5, 70):
        for k in (1, 7, 300, N + 5):
            for excl in (False, True):
                got = g.audience_sessions(hists, all_items[:M], k, by='score', exclude_history=excl)
                want = host_audience(V[:, :M], ~H[:, :M] if excl else np.ones((N, M), dtype=bool), k)
                assert_same(got, want)


def test_lists_longer_than_one_merge_tile(monkeypatch):
    """k above 1024 entries: a list is merged by several workgroups (k_audience_merge places 1024 list entries per workgroup)"""
    g = fitted('linear')
    N = 2600
    hists, items = histories(N, seed=N), item_list(5)[:3]
    V = score_matrix(g, hists, items, (N, 3))
    H = held(hists, items)
    for chunk in (None, 37):
        if chunk:
            monkeypatch.setenv('G4R_SESSIONS_CHUNK', str(chunk))
        for k in (1024, 1025, 2500, N + 5):
            for excl in (False, True):
                got = g.audience_sessions(hists, items, k, by='score', exclude_history=excl)
                assert_same(got, host_audience(V, ~H if excl else np.ones((N, 3), dtype=bool), k))
    lp37 = g.audience_sessions(hists, items, 2500, by='logprob', temperature=0.7, exclude_history=True)
    monkeypatch.delenv('G4R_SESSIONS_CHUNK')
    lp = g.audience_sessions(hists, items, 2500, by='logprob', temperature=0.7, exclude_history=True)
    assert_same(lp37, lp)
    for j in range(3):
        n = int(lp[2][j])
        assert n == min(2500, int((~H[:, j]).sum())) and not H[lp[0][j, :n], j].any()
        np.testing.assert_array_equal(order(lp[1][j, :n], lp[0][j, :n]), np.arange(n))


def test_equal_histories_come_back_in_index_order_across_chunks(monkeypatch):
    g = fitted('linear')
    hists = histories(600, seed=600)
    same = [i for i in range(600) if hists[i] == hists[0]]
    assert same[0] == 0 and same[-1] == 599      # a twin in the first chunk and one behind the 512-row boundary
    for chunk in (None, 16):
        if chunk:
            monkeypatch.setenv('G4R_SESSIONS_CHUNK', str(chunk))
        s, v, c = g.audience_sessions(hists, item_list(5), 605, by='score')
        for j in range(5):
            pos = [int(np.flatnonzero(s[j] == i)[0]) for i in same]
            assert pos == list(range(pos[0], pos[0] + len(same)))      # adjacent (equal values), lower index first
            assert len(set(v[j, pos].view(np.uint32).tolist())) == 1


# ---- by='logprob' ----------------------------------------------------------------------------------------------------------------
def twin(g, hists, items, temperature, excl, tag):
    """(logprob[N, M], eligible[N, M]) of session_log_likelihood's last events of histories[i] + [items[j]]"""
    key = ('lp', id(g), tag, temperature, excl)
    if key not in _CACHE:
        rows = [list(h) + [it] for h in hists for it in items]
        _, offs, res = g.session_log_likelihood(rows, temperature=temperature, exclude_seen=excl, return_details=True)
        last = offs[1:] - 1
        shape = (len(hists), len(items))
        _CACHE[key] = (res['logprob'][last].reshape(shape), np.asarray(res['eligible'])[last].reshape(shape).astype(bool))
    return _CACHE[key]


def check_logprob(got, T, E, k):
    s, v, c = got
    N, M = T.shape
    assert s.shape == v.shape == (M, k) and c.shape == (M,)
    with np.errstate(all='ignore'):
        ulp = np.spacing(np.abs(T).astype(np.float32))      # (an ineligible pair's twin is -inf; never indexed below)
    for j in range(M):
        n = int(c[j])
        assert n == min(k, int(E[:, j].sum()))                                                  # (d)
        assert (s[j, n:] == -1).all() and np.isnan(v[j, n:]).all()
        sj, vj = s[j, :n], v[j, :n]
        assert len(set(sj.tolist())) == n and E[sj, j].all()                                    # (d): no ineligible session, none twice
        assert (np.abs(vj.astype(np.float64) - T[sj, j].astype(np.float64)) <= ulp[sj, j]).all()   # (a)
        np.testing.assert_array_equal(order(vj, sj), np.arange(n))                              # (b)
        if n == k:                                                                              # (c)
            out = np.setdiff1d(np.flatnonzero(E[:, j]), sj)
            if len(out):
                assert (T[out, j].astype(np.float64) <= np.float64(vj[-1]) + ulp[out, j]).all()


LOGPROB_MODELS = [('linear', (20,)), ('softmax', (24, 16))]


@pytest.mark.parametrize('excl', [False, True])
@pytest.mark.parametrize('temperature', [1.0, 0.7])
@pytest.mark.parametrize('N,M', [(1, 5), (37, 70), (600, 5)])
@pytest.mark.parametrize('final_act,layers', LOGPROB_MODELS)
def test_logprobs_against_the_log_likelihood_twin(final_act, layers, N, M, temperature, excl, monkeypatch):
    g = fitted(final_act, layers)
    hists = histories(N, seed=N)
    items = item_list(M)
    T, E = twin(g, hists, items, temperature, excl, (N, M))
    if not excl:
        assert E.all()
    else:
        np.testing.assert_array_equal(E, ~held(hists, items))
    for chunk in ((None, 16) if N == 600 else (None,)):
        if chunk:
            monkeypatch.setenv('G4R_SESSIONS_CHUNK', str(chunk))
        for m in sorted({1, 5, M}):
            for k in (1, 7, 300, N + 5):
                got = g.audience_sessions(hists, items[:m], k, by='logprob', temperature=temperature, exclude_history=excl)
                check_logprob(got, T[:, :m], E[:, :m], k)


# ---- properties of both modes ----------------------------------------------------------------------------------------------------
MODES = [('linear', (20,), 'score'), ('relu', (24, 16), 'score'), ('linear', (20,), 'logprob'), ('softmax', (24, 16), 'logprob')]


@pytest.mark.parametrize('excl', [False, True])
@pytest.mark.parametrize('final_act,layers,by', MODES)
def test_the_result_does_not_depend_on_the_chunking(final_act, layers, by, excl, monkeypatch):
    g = fitted(final_act, layers)
    hists, items = histories(600, seed=600), item_list(70)
    for k in (7, 300, 605):
        monkeypatch.delenv('G4R_SESSIONS_CHUNK', raising=False)
        want = g.audience_sessions(hists, items, k, by=by, temperature=0.7, exclude_history=excl)
        for chunk in (16, 37):
            monkeypatch.setenv('G4R_SESSIONS_CHUNK', str(chunk))
            assert_same(g.audience_sessions(hists, items, k, by=by, temperature=0.7, exclude_history=excl), want)


@pytest.mark.parametrize('final_act,layers,by', MODES)
def test_splitting_the_sessions_over_two_calls(final_act, layers, by):
    g = fitted(final_act, layers)
    hists, items = histories(600, seed=600), item_list(5)
    A, B = hists[:250], hists[250:]
    for k in (7, 300):
        whole = g.audience_sessions(hists, items, k, by=by, exclude_history=True)
        a, b = g.audience_sessions(A, items, k, by=by, exclude_history=True), g.audience_sessions(B, items, k, by=by, exclude_history=True)
        S = np.full((5, k), -1, dtype=np.int64)
        W = np.full((5, k), np.nan, dtype=np.float32)
        C = np.zeros(5, dtype=np.int32)
        for j in range(5):
            idx = np.concatenate([a[0][j, :a[2][j]], b[0][j, :b[2][j]] + 250])
            val = np.concatenate([a[1][j, :a[2][j]], b[1][j, :b[2][j]]])
            o = order(val, idx)[:k]
            C[j] = len(o)
            S[j, :len(o)], W[j, :len(o)] = idx[o], val[o]
        assert_same(whole, (S, W, C))


@pytest.mark.parametrize('final_act,layers,by', [MODES[0], MODES[2]])
def test_permuting_the_sessions_permutes_the_indices(final_act, layers, by, monkeypatch):
    g = fitted(final_act, layers)
    hists, items = histories(600, seed=7, duplicates=False), item_list(5)
    # tie-free inputs: distinct histories may still share a float32 value for an item; such sessions are left out (a session's value
    # does not depend on the others)
    s0, v0, _ = g.audience_sessions(hists, items, 600, by=by)
    tied = set()
    for j in range(5):
        bits = v0[j].view(np.uint32)
        _, inv, cnt = np.unique(bits, return_inverse=True, return_counts=True)
        tied.update(s0[j, cnt[inv] > 1].tolist())
    hists = [h for i, h in enumerate(hists) if i not in tied]
    N = len(hists)
    assert N > 520
    monkeypatch.setenv('G4R_SESSIONS_CHUNK', '37')
    s, v, c = g.audience_sessions(hists, items, 300, by=by)
    assert all(len(set(v[j].view(np.uint32).tolist())) == 300 for j in range(5))
    p = np.random.RandomState(3).permutation(N)      # new position q holds old session p[q]
    s2, v2, c2 = g.audience_sessions([hists[i] for i in p], items, 300, by=by)
    assert_same((p[s2], v2, c2), (s, v, c))


def test_hidden_continues_a_session():
    g = fitted('linear', (24, 16))
    a, b, items = histories(37, seed=1), histories(37, seed=2), item_list(5)
    _, _, H = g.recommend_sessions(a, k=1, return_hidden=True)
    want = g.audience_sessions([x + y for x, y in zip(a, b)], items, 10, by='score')
    assert_same(g.audience_sessions(b, items, 10, by='score', hidden=H), want)
    assert not np.array_equal(g.audience_sessions(b, items, 10, by='score')[1], want[1])


def test_the_prediction_state_is_left_alone():
    g = fitted('linear')
    ids = 10 + 3 * np.arange(N_ITEMS)
    sid, in1, in2 = np.arange(8), ids[5:13], ids[40:48]
    hists, items = histories(37, seed=37), item_list(5)

    def run(between):
        g.predict = None
        p1 = g.predict_next_batch(sid, in1, batch=8)
        if between:
            g.audience_sessions(hists, items, 7, by='score')
            g.audience_sessions(hists, items, 7, by='logprob', exclude_history=True)
        r = g.recommend_next_batch(sid, in2, k=10, batch=8)
        p2 = g.predict_next_batch(sid, in1, batch=8)
        g.predict = None
        return np.asarray(p1), r[0], r[1], np.asarray(p2)

    for x, y in zip(run(False), run(True)):
        np.testing.assert_array_equal(x, y)


def test_the_c_entry_refuses_before_any_launch_and_the_next_call_is_correct():
    g = fitted('linear')
    m = g._ensure_model()
    hists, items = histories(37, seed=37), item_list(5)
    want = g.audience_sessions(hists, items, 7)
    offs, hi = np.array([0, 2], dtype=np.int64), np.array([1, 2], dtype=np.int32)
    ok = dict(hist_offs=offs, hist_items=hi, items=np.array([3], dtype=np.int32), k=2)
    m.profile(True)
    try:
        for bad, msg in ((dict(items=np.array([N_ITEMS], dtype=np.int32)), 'item index out of range'), (dict(items=np.array([-1], dtype=np.int32)), 'item index'),
                         (dict(hist_items=np.array([1, N_ITEMS], dtype=np.int32)), 'history item index out of range'),
                         (dict(hist_offs=np.array([0, 0], dtype=np.int64)), 'is empty'), (dict(temperature=0.0), 'temperature'),
                         (dict(temperature=float('nan')), 'temperature'), (dict(hidden=[np.zeros((1, 20), dtype=np.float32)] * 2), 'hidden')):
            with pytest.raises((_native.NativeError, ValueError), match=msg):
                m.audience_sessions(**dict(ok, **bad))
        lib, i32p = _native.lib(), _native.i32p
        out = np.zeros(4, dtype=np.int32)
        val = np.zeros(4, dtype=np.float32)
        raw = lambda n_items, k, by: lib.g4r_audience_sessions(m.h, offs.ctypes.data_as(_native.i64p), hi.ctypes.data_as(i32p), 1, None,
                                                               ok['items'].ctypes.data_as(i32p), n_items, k, by, 1.0, 0, out.ctypes.data_as(i32p),
                                                               val.ctypes.data_as(_native.f32p), out.ctypes.data_as(i32p))
        for args in ((0, 2, 1), (_native.G4R_AUDIENCE_ITEMS_MAX + 1, 2, 1), (1, 0, 1), (1, _native.G4R_AUDIENCE_MAX + 1, 1), (1, 2, 2), (1, 2, -1),
                     (4096, 4096, 1)):
            assert raw(*args) == -1, args
        assert not any(name.startswith('k_audience') for name in m.kernel_times())      # no call got as far as its first launch
        assert_same(g.audience_sessions(hists, items, 7), want)
        kt = m.kernel_times()
        assert kt['k_audience_keys'][1] == kt['k_audience_merge'][1] == 1      # one chunk
    finally:
        m.profile(False)
    sm = fitted('softmax', (24, 16))._ensure_model()
    with pytest.raises(_native.NativeError, match='G4R_AUDIENCE_LOGPROB'):
        sm.audience_sessions(by='score', **ok)


def test_run_py_saves_the_audience(tmp_path):
    g = fitted('linear', str_ids=True)
    model, test, items, out = (str(tmp_path / n) for n in ('model.pickle', 'test.tsv', 'items.txt', 'audience.npz'))
    g.savemodel(model)
    hists = [[str(i) for i in h] for h in histories(640, seed=45) if len(h) >= 2]      # (the evaluation in front wants 512 sessions of 2 events)
    assert len(hists) >= 512
    sids = 1000 + 7 * np.arange(len(hists))
    rows = [(sid, it, t) for sid, h in zip(sids, hists) for t, it in enumerate(h)]
    pd.DataFrame(rows, columns=['SessionId', 'ItemId', 'Time']).to_csv(test, sep='\t', index=False)
    ids = [str(i) for i in item_list(5)]
    with open(items, 'w') as f:
        f.write('\n'.join(ids) + '\n')
    for by in ('score', 'logprob'):
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'run.py'), model, '-l', '-t', test, '--save_audience', out, '--audience_items', items,
                            '--audience_k', '40', '--audience_by', by], cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
        s, v, c = g.audience_sessions(hists, ids, 40, by=by)
        with np.load(out) as z:
            assert z['item_ids'].tolist() == ids
            np.testing.assert_array_equal(z['counts'], c)
            np.testing.assert_array_equal(z['values'].view(np.uint32), v.view(np.uint32))
            np.testing.assert_array_equal(z['session_ids'], np.where(s >= 0, sids[np.maximum(s, 0)], -1))

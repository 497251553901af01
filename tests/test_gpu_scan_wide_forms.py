"""The bf16 scan on top layers wider than 128 units: k_scan_bf16<4> (129 .. 256 units) and k_scan_bf16<8> (257 .. 512), each with fixed
exclusion lists (TkExcl: g4r_recommend_sessions_scan) and with lists that grow on the device (TkGrow: g4r_continue_sessions).  The other
scan tests run models of at most 128 units, which take k_scan_bf16<2>.

Oracles, the ones tests/test_gpu_recommend_scan.py and tests/test_gpu_continue_sessions.py use:
  fixed lists    c = k * oversample covers every candidate -> the result IS the exact (fp32) filtered call's, bit for bit; and with
                 c below the candidate count, on rows CERTIFIED by the bf16 error bound (certified_rows), it is again the exact call's
  growing lists  continue_sessions(oversample) == the loop of recommend_sessions(oversample) calls that appends every row's best item
                 to its history and to its exclusion list -- the same c, so stage 1 has to keep the same candidates in both
Shapes: 1 row and 129 rows (a second, nearly empty row block); 33 and 65 candidates; k = 1 and k = every position left eligible in the
fullest row; a row with an empty list and a row with a full list (G4R_EXCLUDE_MAX items, less the slack the growing lists need)."""
import numpy as np
import pytest

from test_gpu_recommend_scan import bits, certified_rows, native_model

pytestmark = pytest.mark.gpu

I = 2000
EXCLUDE_MAX = 1024      # G4R_EXCLUDE_MAX
X_ROW, X_MASK = 7, 2    # candidate positions the fullest row's list / the global mask take
_MODELS = {}


def model(D):
    if D not in _MODELS:
        _MODELS[D] = native_model(I, D, seed=D)[:3]
    return _MODELS[D]


@pytest.fixture(scope='module', autouse=True)
def close_models():
    yield
    while _MODELS:
        _MODELS.popitem()[1][0].close()


def inputs(D, rows, n_cand, full_len, seed):
    """One-item sessions from h0 = tanh(N(0, 1)); n_cand distinct candidates; row 0 excludes nothing, the last row full_len items
    (X_ROW of them candidates), the rows between a few; the mask takes the first X_MASK candidates and 100 other items."""
    rng = np.random.RandomState(seed)
    cand = rng.permutation(I)[:n_cand].astype(np.int32)
    others = np.setdiff1d(np.arange(I), cand)
    lists = []
    for r in range(rows):
        if r == rows - 1:
            row = np.concatenate([cand[X_MASK:X_MASK + X_ROW], rng.permutation(others)[:full_len - X_ROW]])
        elif r == 0:
            row = np.zeros(0, dtype=np.int64)
        else:
            row = np.concatenate([rng.permutation(cand[X_MASK:])[:rng.randint(0, X_ROW + 1)], rng.permutation(others)[:rng.randint(0, 20)]])
        lists.append(rng.permutation(row).astype(np.int32))
    mask = np.zeros((I + 31) // 32, dtype=np.uint32)
    for i in np.concatenate([cand[:X_MASK], rng.permutation(others)[:100]]):
        mask[i >> 5] |= np.uint32(1) << np.uint32(i & 31)
    hist = [[int(i)] for i in rng.randint(0, I, size=rows)]
    h0 = [np.tanh(rng.randn(rows, D)).astype(np.float32)]
    return cand, lists, mask, hist, h0


def csr(lists):
    offs = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    flat = np.concatenate([np.asarray(x, dtype=np.int32) for x in lists]) if offs[-1] else np.zeros(0, dtype=np.int32)
    return offs, flat.astype(np.int32)


def assert_equal(got, want):
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(bits(got[1]), bits(want[1]))


@pytest.mark.parametrize('k_all', [False, True])
@pytest.mark.parametrize('n_cand', [33, 65])
@pytest.mark.parametrize('rows', [1, 129])
@pytest.mark.parametrize('D', [160, 264])
def test_fixed_lists_every_candidate_kept_is_the_exact_call(D, rows, n_cand, k_all):
    m = model(D)[0]
    k = n_cand - X_ROW - X_MASK if k_all else 1
    over = -(-n_cand // k)      # c = min(n_cand, k * over) = n_cand
    for full_len in (EXCLUDE_MAX, 0) if rows == 1 else (EXCLUDE_MAX,):      # (one row: once with the full list, once with none)
        cand, lists, mask, hist, h0 = inputs(D, rows, n_cand, full_len, seed=D + rows + n_cand)
        if full_len == 0:
            lists = [np.zeros(0, dtype=np.int32)]
        ho, hi = csr(hist)
        xo, xi = csr(lists)
        exact = m.recommend_sessions(ho, hi, cand, k, xo, xi, mask, hidden=h0)
        scan = m.recommend_sessions(ho, hi, cand, k, xo, xi, mask, hidden=h0, oversample=over)
        assert_equal(scan, exact)
        gone = [set(x) for x in lists]
        assert all(not (set(cand[scan[0][r]]) & gone[r]) and scan[0][r].min() >= X_MASK for r in range(rows))


@pytest.mark.parametrize('D', [160, 264])
def test_fixed_lists_certified_rows_are_the_exact_call(D):
    """c = 24 of 65 candidates: stage 1 has to rank by the bf16 scores; every row is certified, so the result is the exact one."""
    m, Wy, By = model(D)
    rows, n_cand, k, over = 129, 65, 3, 8
    cand, lists, mask, hist, h0 = inputs(D, rows, n_cand, EXCLUDE_MAX, seed=D)
    ho, hi = csr(hist)
    xo, xi = csr(lists)
    exact = m.recommend_sessions(ho, hi, cand, k, xo, xi, mask, hidden=h0, return_hidden=True)
    scan = m.recommend_sessions(ho, hi, cand, k, xo, xi, mask, hidden=h0, oversample=over)
    eligible = np.ones((rows, n_cand), dtype=bool)
    eligible[:, :X_MASK] = False
    for r in range(rows):
        eligible[r, np.isin(cand, lists[r])] = False
    ok = certified_rows(exact[2][0], Wy[cand], By[cand], k, k * over, eligible)
    print('D=%d: %d of %d rows certified' % (D, ok.sum(), rows))
    assert ok.all(), 'uncertified rows: %s' % np.flatnonzero(~ok)
    assert_equal(scan, exact[:2])


@pytest.mark.parametrize('k_all', [False, True])
@pytest.mark.parametrize('n_cand', [33, 65])
@pytest.mark.parametrize('rows', [1, 129])
@pytest.mark.parametrize('D', [160, 264])
def test_growing_lists_equal_the_loop_of_scans(D, rows, n_cand, k_all):
    m = model(D)[0]
    steps = 3
    k = n_cand - X_ROW - X_MASK - (steps - 1) if k_all else 1      # every generated item takes one eligible position
    over = 1 if k_all else 2                                       # c = k, c = 2: below the candidate count
    for full_len in (EXCLUDE_MAX - (steps - 1), 0) if rows == 1 else (EXCLUDE_MAX - (steps - 1),):
        cand, lists, mask, hist, h0 = inputs(D, rows, n_cand, full_len, seed=D + rows + n_cand + 1)
        if full_len == 0:
            lists = [np.zeros(0, dtype=np.int32)]
        ho, hi = csr(hist)
        xo, xi = csr(lists)
        cols, scores, H = m.continue_sessions(ho, hi, cand, k, steps, True, xo, xi, mask, hidden=h0, return_hidden=True, oversample=over)
        assert cols.shape == scores.shape == (rows, steps, k)
        hs, xs = [list(h) for h in hist], [list(x) for x in lists]
        for s in range(steps):
            ho, hi = csr(hs)
            xo, xi = csr(xs)
            wc, ws, wH = m.recommend_sessions(ho, hi, cand, k, xo, xi, mask, hidden=h0, return_hidden=True, oversample=over)
            assert_equal((cols[:, s], scores[:, s]), (wc, ws))
            for r in range(rows):
                hs[r].append(int(cand[wc[r, 0]]))
                xs[r].append(int(cand[wc[r, 0]]))
        np.testing.assert_array_equal(bits(H[0]), bits(wH[0]))

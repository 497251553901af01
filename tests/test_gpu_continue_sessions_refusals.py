"""The host checks of the C entry g4r_continue_sessions, reached through _native.Model without the Python layer's own checks in front:
a call they refuse raises NativeError and enqueues nothing (g4r_get_debug "continue_steps": calls that passed every check, (chunk,
step) chains enqueued -- neither moves), and the boundaries they allow run: a list that grows to exactly G4R_EXCLUDE_MAX items on
the device, candidates that run dry at the last step."""
import numpy as np
import pytest

from gru4rec_amd import _native

pytestmark = pytest.mark.gpu

I, D = 3000, 32
XMAX = _native.G4R_EXCLUDE_MAX


@pytest.fixture(scope='module')
def model():
    rng = np.random.RandomState(0)
    m = _native.Model(n_items=I, layers=[D], batch_size=32, n_sample=0, loss=_native.LOSS_IDS['bpr-max'], final_act=_native.ACT_IDS['linear'],
                      hidden_act=_native.ACT_IDS['tanh'], embed_mode=0, embedding=0, learning_rate=0.1, sample_store=0, seed=1, device=0,
                      rank=0, nranks=1, use_graph=0)
    m.set_param('Wy', (rng.randn(I, D) * 0.1).astype(np.float32))
    m.set_param('By', (rng.randn(I) * 0.1).astype(np.float32))
    m.set_param('Wx', (rng.randn(D, 3 * D) * 0.05).astype(np.float32))
    m.set_param('Wh', (rng.randn(D, D) * 0.05).astype(np.float32))
    m.set_param('Wrz', (rng.randn(D, 2 * D) * 0.05).astype(np.float32))
    m.set_param('Bh', (rng.randn(3 * D) * 0.1).astype(np.float32))
    yield m
    m.close()


OFFS = np.array([0, 2, 3], dtype=np.int64)          # two sessions: items (5, 6) and (7)
HIST = np.array([5, 6, 7], dtype=np.int32)


def counters(m):
    return m.get_debug('continue_steps', 2).tolist()


def refused(m, match, **kw):
    before = counters(m)
    with pytest.raises(_native.NativeError, match=match):
        m.continue_sessions(OFFS, HIST, **kw)
    assert counters(m) == before, 'a refused call enqueued work'


def test_lists_that_would_outgrow_the_maximum_are_refused_with_and_without_lists(model):
    m = model
    # no lists passed: every row starts empty and gains steps - 1 items on the device
    refused(m, 'G4R_EXCLUDE_MAX', k=1, steps=XMAX + 2, no_repeat=True)
    refused(m, 'G4R_EXCLUDE_MAX', k=1, steps=1100, no_repeat=True)
    # lists passed: row 1 holds 1,000 distinct items, 24 more fit
    xo = np.array([0, 1, 1001], dtype=np.int64)
    xi = np.concatenate([[5], np.arange(100, 1100)]).astype(np.int32)
    refused(m, 'row 1', k=1, steps=26, no_repeat=True, excl_offs=xo, excl_items=xi)
    before = counters(m)
    cols, _ = m.continue_sessions(OFFS, HIST, k=1, steps=25, no_repeat=True, excl_offs=xo, excl_items=xi)     # 1,000 + 24 == the maximum
    assert counters(m) == [before[0] + 1, before[1] + 25]
    assert cols.shape == (2, 25, 1)
    for r in range(2):
        path = cols[r, :, 0].tolist()
        assert len(set(path)) == 25 and not set(path) & set(xi[xo[r]:xo[r + 1]].tolist())
    # without no_repeat nothing grows: the same lists and many more steps are fine for the check (run short here)
    m.continue_sessions(OFFS, HIST, k=1, steps=30, no_repeat=False, excl_offs=xo, excl_items=xi)


def test_a_list_grows_to_exactly_the_maximum_on_the_device(model):
    m = model
    before = counters(m)
    cols, scores = m.continue_sessions(OFFS, HIST, k=3, steps=XMAX + 1, no_repeat=True)      # empty lists + 1,024 generated items
    assert counters(m) == [before[0] + 1, before[1] + XMAX + 1]
    assert cols.shape == (2, XMAX + 1, 3) and cols.min() >= 0 and cols.max() < I
    for r in range(2):
        gone = set()
        for s in range(XMAX + 1):
            assert not gone & set(cols[r, s].tolist()), 'row %d step %d returns an item it has generated' % (r, s)
            gone.add(int(cols[r, s, 0]))
        assert len(gone) == XMAX + 1
    assert np.isfinite(scores).all()


def test_duplicate_candidates_are_refused_with_no_repeat_only(model):
    m = model
    cand = np.array([40, 7, 40, 3, 9, 11, 12, 13], dtype=np.int32)
    refused(m, 'duplicate-free', item_idx=cand, k=2, steps=2, no_repeat=True)
    refused(m, 'duplicate-free', item_idx=cand, k=2, steps=1, no_repeat=True)
    cols, _ = m.continue_sessions(OFFS, HIST, item_idx=cand, k=2, steps=3, no_repeat=False)
    assert cols.shape == (2, 3, 2) and cols.min() >= 0 and cols.max() < len(cand)


def test_the_eligible_count_boundary(model):
    m = model
    cand = np.arange(100, 112, dtype=np.int32)                       # 12 candidates
    refused(m, 'row 0', item_idx=cand, k=5, steps=9, no_repeat=True)             # 12 - 8 < 5
    cols, _ = m.continue_sessions(OFFS, HIST, item_idx=cand, k=5, steps=8, no_repeat=True)      # 12 - 7 == 5: the last list is all that is left
    assert cols.min() >= 0 and cols.max() < 12, 'a pad (column 0xFFFFFFFF) was returned'
    for r in range(2):
        assert set(cols[r, 7].tolist()) == set(range(12)) - set(cols[r, :7, 0].tolist())
    # row 1 lists two of the candidates: 10 eligible
    xo = np.array([0, 0, 2], dtype=np.int64)
    xi = np.array([100, 101], dtype=np.int32)
    refused(m, 'row 1', item_idx=cand, k=5, steps=7, no_repeat=True, excl_offs=xo, excl_items=xi)
    cols, _ = m.continue_sessions(OFFS, HIST, item_idx=cand, k=5, steps=6, no_repeat=True, excl_offs=xo, excl_items=xi)
    assert cols.min() >= 0 and not {0, 1} & set(cols[1].ravel().tolist())
    # a mask takes positions too
    mask = np.zeros((I + 31) // 32, dtype=np.uint32)
    for i in (102, 103, 104):
        mask[i >> 5] |= np.uint32(1 << (i & 31))
    refused(m, 'row 0', item_idx=cand, k=5, steps=6, no_repeat=True, excl_mask=mask)          # 9 - 5 < 5
    m.continue_sessions(OFFS, HIST, item_idx=cand, k=5, steps=5, no_repeat=True, excl_mask=mask)


def test_other_refusals(model):
    m = model
    before = counters(m)
    with pytest.raises((ValueError, _native.NativeError)):
        m.continue_sessions(OFFS, HIST, k=1, steps=0)
    with pytest.raises(_native.NativeError):
        m.continue_sessions(OFFS, HIST, k=0, steps=2)
    with pytest.raises(_native.NativeError):
        m.continue_sessions(OFFS, HIST, k=1, steps=2, oversample=-1)
    with pytest.raises(_native.NativeError):
        m.continue_sessions(OFFS, np.array([5, 6, I], dtype=np.int32), k=1, steps=2)      # a history item out of range
    with pytest.raises(_native.NativeError):
        m.continue_sessions(OFFS, HIST, item_idx=np.array([1, I], dtype=np.int32), k=1, steps=1)
    assert counters(m) == before

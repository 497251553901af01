"""The grow-only device arrays of the inference entries (DevBuf, g4r_host_model.hpp) over a model's life: every entry is called
small, then large, then small again on ONE model, so each array is allocated, outgrown in mid-life and then reused at a smaller size.
Every call is replayed on a fresh twin (same configuration, seed and weights) for which it is the first call of its kind, with
arrays of exactly the call's size.  Both sides run the same kernels with the same geometry: columns and score bits must be equal."""
import numpy as np
import pytest

from gru4rec_amd import _native

pytestmark = pytest.mark.gpu

N_ITEMS, D, PB = 300, 64, 130
# rows (one past the 128-row block in the large shape), k, candidates (None: all items), items per exclusion list
SMALL = dict(rows=3, k=1, n_cand=40, n_excl=2)
LARGE = dict(rows=130, k=33, n_cand=None, n_excl=20)


def make(final_act):
    sm = final_act.startswith('softmax')
    m = _native.Model(n_items=N_ITEMS, layers=[D], batch_size=32, n_sample=0, loss=_native.LOSS_IDS['cross-entropy' if sm else 'bpr-max'],
                      final_act=_native.ACT_IDS[final_act], hidden_act=_native.ACT_IDS['tanh'], embed_mode=0, embedding=0,
                      learning_rate=0.1, sample_store=0, seed=1, device=0, rank=0, nranks=1, use_graph=0)
    rng = np.random.RandomState(5)
    m.set_param('Wy', (rng.randn(N_ITEMS, D) * 0.1).astype(np.float32))
    m.set_param('By', (rng.randn(N_ITEMS) * 0.1).astype(np.float32))
    m.set_param('Wx', (rng.randn(D, 3 * D) * 0.05).astype(np.float32))
    m.set_param('Wh', (rng.randn(D, D) * 0.05).astype(np.float32))
    m.set_param('Wrz', (rng.randn(D, 2 * D) * 0.05).astype(np.float32))
    m.set_param('Bh', (rng.randn(3 * D) * 0.1).astype(np.float32))
    return m


def inputs(shape, seed):
    """The arguments of one round of calls at `shape`."""
    rng = np.random.RandomState(seed)
    rows, n_excl = shape['rows'], shape['n_excl']
    cand = None if shape['n_cand'] is None else rng.permutation(N_ITEMS)[:shape['n_cand']].astype(np.int32)      # duplicate-free (no_repeat)
    lens = rng.randint(1, 6, size=rows)
    mask = np.zeros((N_ITEMS + 31) // 32, dtype=np.uint32)
    mask[1] = 0x00010010
    return dict(k=shape['k'], cand=cand, in_idx=rng.randint(0, N_ITEMS, size=rows).astype(np.int32),
                xoffs=np.arange(rows + 1, dtype=np.int64) * n_excl, xitems=rng.randint(0, N_ITEMS, size=rows * n_excl).astype(np.int32), mask=mask,
                hoffs=np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), hitems=rng.randint(0, N_ITEMS, size=int(lens.sum())).astype(np.int32),
                coffs=np.arange(rows + 1, dtype=np.int64) * (shape['n_cand'] or N_ITEMS),
                citems=np.concatenate([rng.permutation(N_ITEMS)[:shape['n_cand'] or N_ITEMS] for _ in range(rows)]).astype(np.int32),
                q=rng.randint(0, N_ITEMS, size=rows).astype(np.int32))


def stateful(fn):
    """A call on the prediction state, from a zero state of PB rows on whichever model runs it."""
    def run(m, a):
        m.predict_begin(PB)
        return fn(m, a)
    return run


CALLS = [
    ('recommend_step', stateful(lambda m, a: m.recommend_step(a['in_idx'], a['cand'], a['k']))),
    ('recommend_step_filtered', stateful(lambda m, a: m.recommend_step_filtered(a['in_idx'], a['cand'], a['k'], a['xoffs'], a['xitems'], a['mask']))),
    ('recommend_step_scan', stateful(lambda m, a: m.recommend_step_filtered(a['in_idx'], a['cand'], a['k'], a['xoffs'], a['xitems'], None, oversample=8))),
    ('recommend_sessions', lambda m, a: m.recommend_sessions(a['hoffs'], a['hitems'], a['cand'], a['k'], a['xoffs'], a['xitems'], None)),
    ('continue_sessions', lambda m, a: m.continue_sessions(a['hoffs'], a['hitems'], a['cand'], a['k'], 3, True, a['xoffs'], a['xitems'], None)),
    ('score_candidates', stateful(lambda m, a: m.score_candidates(a['in_idx'], a['coffs'], a['citems'], a['k']))),
    ('similar_items', lambda m, a: m.similar_items(a['q'], a['cand'], a['k'], 'cosine', 'output', True, a['mask'])),
]


@pytest.mark.parametrize('final_act', ['linear', 'softmax'])
def test_grown_and_reused_buffers_give_a_fresh_models_bits(final_act):
    a_model = make(final_act)
    rounds = [inputs(SMALL, 1), inputs(LARGE, 2), inputs(SMALL, 3)]
    try:
        for name, call in CALLS:
            if name == 'recommend_step_scan' and final_act != 'linear':
                continue      # (the bf16 scan refuses softmax)
            for i, args in enumerate(rounds):
                got = call(a_model, args)
                fresh = make(final_act)
                try:
                    want = call(fresh, args)
                finally:
                    fresh.close()
                where = '%s, round %d' % (name, i)
                assert got[0].shape == want[0].shape and got[1].shape == want[1].shape, where
                np.testing.assert_array_equal(got[0], want[0], err_msg=where)
                np.testing.assert_array_equal(np.ascontiguousarray(got[1], dtype=np.float32).view(np.uint32),
                                              np.ascontiguousarray(want[1], dtype=np.float32).view(np.uint32), err_msg=where)
    finally:
        a_model.close()

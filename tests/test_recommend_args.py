"""GRU4Rec.recommend_next_batch refuses a bad k before any device work (no GPU needed): k = 0, k > 256 (G4R_TOPK_MAX) and k above
the number of candidates raise ValueError; the model is never created."""
import numpy as np
import pandas as pd
import pytest

from gru4rec_amd.gru4rec import GRU4Rec


def _model_without_device(n_items=300):
    g = GRU4Rec(layers=[64], final_act='linear')
    # what fit() would leave behind (fitting needs a GPU): the item id map; the device model is never to be created here
    g.itemidmap = pd.Series(data=np.arange(n_items), index=np.arange(1000, 1000 + n_items), name='ItemIdx')
    g.n_items = n_items
    g.error_during_train = False

    def no_device():
        raise AssertionError('recommend_next_batch touched the device before checking k')
    g._ensure_model = no_device
    return g


@pytest.mark.parametrize('k', [0, -1, 257, 1000])
def test_k_out_of_range_all_items(k):
    g = _model_without_device()
    with pytest.raises(ValueError, match='k = '):
        g.recommend_next_batch(np.array([1, 2]), np.array([1000, 1001]), k=k)


def test_k_above_the_candidate_count():
    g = _model_without_device()
    cand = np.array([1000, 1005, 1005, 1007])       # duplicates count: 4 candidates
    with pytest.raises(ValueError, match='number of candidates = 4'):
        g.recommend_next_batch(np.array([1]), np.array([1000]), k=5, predict_for_item_ids=cand)
    g2 = _model_without_device(n_items=10)
    with pytest.raises(ValueError):
        g2.recommend_next_batch(np.array([1]), np.array([1000]), k=11)


def test_non_integer_k():
    g = _model_without_device()
    with pytest.raises(ValueError):
        g.recommend_next_batch(np.array([1]), np.array([1000]), k=2.5)


def test_valid_k_reaches_the_device():
    """A valid k goes on to the device model (here: the stand-in that refuses), so the checks above are not vacuous."""
    g = _model_without_device()
    with pytest.raises(AssertionError, match='touched the device'):
        g.recommend_next_batch(np.array([1]), np.array([1000]), k=256)
    with pytest.raises(AssertionError, match='touched the device'):
        g.recommend_next_batch(np.array([1]), np.array([1000]), k=4, predict_for_item_ids=np.array([1000, 1005, 1005, 1007]))


class _KRecorder:
    """Stand-in for the device model that records the k it is handed."""

    def __init__(self):
        self.k = []

    def predict_begin(self, batch):
        pass

    def predict_hidden(self, zero_mask=None):
        pass

    def recommend_step(self, in_idx, item_idx=None, k=20):
        self.k.append(k)
        return np.tile(np.arange(k, dtype=np.int32), (len(in_idx), 1)), np.zeros((len(in_idx), k), dtype=np.float32)


def test_what_k_is_taken_as():
    """True counts as 1 and 2.0 as 2 (the device receives an int); 2.5, 0 and number of candidates + 1 are refused with the call's own
    message; a string and None fail inside int(), with int's own error."""
    g = _model_without_device()
    rec = _KRecorder()
    g._ensure_model = lambda: rec
    cand = np.array([1000, 1005, 1005, 1007, 1009])
    for k, want in ((True, 1), (2.0, 2)):
        items, scores = g.recommend_next_batch(np.array([1]), np.array([1000]), k=k, predict_for_item_ids=cand, batch=1)
        assert rec.k[-1] == want and type(rec.k[-1]) is int and items.shape == scores.shape == (1, want)
    for k in (2.5, 0, 6):
        with pytest.raises(ValueError, match='k = %r: it must be an integer in' % (k,)):
            g.recommend_next_batch(np.array([1]), np.array([1000]), k=k, predict_for_item_ids=cand, batch=1)
    with pytest.raises(ValueError, match='invalid literal'):
        g.recommend_next_batch(np.array([1]), np.array([1000]), k='a', predict_for_item_ids=cand, batch=1)
    with pytest.raises(TypeError):
        g.recommend_next_batch(np.array([1]), np.array([1000]), k=None, predict_for_item_ids=cand, batch=1)
    assert len(rec.k) == 2

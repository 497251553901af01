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

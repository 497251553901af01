"""GRU4Rec.diversify_sessions / diversify_lists refuse bad arguments before any device work (no GPU needed): a bad k, pool, trade_off,
metric or space and ragged or non-finite lists raise ValueError, an unknown item id KeyError, space='input' on a one-hot model
NotImplementedError; the model is never created.  Header, binding and exported symbols agree on the two new entries."""
import os
import re

import numpy as np
import pandas as pd
import pytest

from gru4rec_amd import _native
from gru4rec_amd import build as g4r_build
from gru4rec_amd.gru4rec import GRU4Rec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model_without_device(n_items=300, **kw):
    g = GRU4Rec(layers=[64], final_act='linear', **kw)
    # what fit() would leave behind (fitting needs a GPU): the item id map; the device model is never to be created here
    g.itemidmap = pd.Series(data=np.arange(n_items), index=np.arange(1000, 1000 + n_items), name='ItemIdx')
    g.n_items = n_items
    g.error_during_train = False

    def no_device():
        raise AssertionError('diversify touched the device before checking its arguments')
    g._ensure_model = no_device
    return g


HIST = [[1000, 1001], [1005]]
LISTS = np.array([[1000, 1001, 1002, 1003], [1003, 1003, 1004, 1005]])
REL = np.array([[0.5, 0.25, 0.125, 0.0], [1.0, 1.0, -2.0, 3.0]])


@pytest.mark.parametrize('k', [0, -1, 11, 2.5, True, 'a', None])
def test_k_out_of_range(k):
    g = _model_without_device()
    with pytest.raises(ValueError, match='k = '):
        g.diversify_sessions(HIST, k=k, pool=10)
    with pytest.raises(ValueError, match='k = '):
        g.diversify_lists(LISTS, REL, k=k if k != 11 else 5)


@pytest.mark.parametrize('pool', [0, -3, 129, 256, 2.5, True])
def test_pool_out_of_range(pool):
    g = _model_without_device()
    with pytest.raises(ValueError, match='pool = '):
        g.diversify_sessions(HIST, k=1, pool=pool)


def test_pool_above_the_candidate_count():
    g = _model_without_device()
    with pytest.raises(ValueError, match='pool = 5.*number of candidates = 4'):
        g.diversify_sessions(HIST, k=2, pool=5, predict_for_item_ids=np.array([1000, 1005, 1005, 1007]))
    with pytest.raises(ValueError, match='pool = 100.*number of candidates = 50'):
        _model_without_device(n_items=50).diversify_sessions(HIST, k=2)
    with pytest.raises(ValueError, match='k = 5'):
        g.diversify_sessions(HIST, k=5, pool=4)


def test_pool_needs_that_many_eligible_positions():
    g = _model_without_device(n_items=20)
    with pytest.raises(ValueError, match='row 0 has 18 eligible candidate positions, fewer than k = 19'):
        g.diversify_sessions(HIST, k=2, pool=19, exclude_history=True)
    with pytest.raises(AssertionError, match='touched the device'):
        g.diversify_sessions(HIST, k=2, pool=18, exclude_history=True)


@pytest.mark.parametrize('t', [-0.01, 1.5, float('nan'), float('inf'), 'x', None, True])
def test_trade_off_out_of_range(t):
    g = _model_without_device()
    with pytest.raises(ValueError, match='trade_off = '):
        g.diversify_sessions(HIST, k=2, pool=10, trade_off=t)
    with pytest.raises(ValueError, match='trade_off = '):
        g.diversify_lists(LISTS, REL, k=2, trade_off=t)


@pytest.mark.parametrize('kw', [dict(metric='euclid'), dict(metric=None), dict(space='hidden'), dict(space=0)])
def test_bad_metric_or_space(kw):
    g = _model_without_device()
    with pytest.raises(ValueError, match='metric = |space = '):
        g.diversify_sessions(HIST, k=2, pool=10, **kw)
    with pytest.raises(ValueError, match='metric = |space = '):
        g.diversify_lists(LISTS, REL, k=2, **kw)


def test_bad_scan_arguments():
    g = _model_without_device()
    with pytest.raises(ValueError, match='scan = '):
        g.diversify_sessions(HIST, k=2, pool=10, scan='fp16')
    with pytest.raises(ValueError, match='k \\* oversample = 100 \\* 11'):
        g.diversify_sessions(HIST, k=2, pool=100, scan='bf16', oversample=11)
    with pytest.raises(AssertionError, match='touched the device'):
        g.diversify_sessions(HIST, k=2, pool=100, scan='bf16', oversample=10)


def test_input_space_of_a_one_hot_model():
    g = _model_without_device()      # embedding = 0, constrained_embedding = False: one-hot input
    with pytest.raises(NotImplementedError, match="space='output'"):
        g.diversify_sessions(HIST, k=2, pool=10, space='input')
    with pytest.raises(NotImplementedError, match="space='output'"):
        g.diversify_lists(LISTS, REL, k=2, space='input')
    for kw in (dict(embedding=32), dict(constrained_embedding=True)):
        with pytest.raises(AssertionError, match='touched the device'):
            _model_without_device(**kw).diversify_sessions(HIST, k=2, pool=10, space='input')
        with pytest.raises(AssertionError, match='touched the device'):
            _model_without_device(**kw).diversify_lists(LISTS, REL, k=2, space='input')


def test_unknown_item_ids():
    g = _model_without_device()
    with pytest.raises(KeyError):
        g.diversify_sessions([[1000, 7]], k=2, pool=10)
    with pytest.raises(KeyError):
        g.diversify_sessions(HIST, k=2, pool=3, predict_for_item_ids=[1001, 1002, 8])
    with pytest.raises(KeyError):
        g.diversify_sessions(HIST, k=2, pool=10, exclude=[9])
    with pytest.raises(KeyError):
        g.diversify_lists(np.array([[1000, 1001, 5]]), np.zeros((1, 3)), k=2)
    with pytest.raises(ValueError, match='empty'):
        g.diversify_sessions([], k=2, pool=10)
    with pytest.raises(ValueError, match='history 1 is empty'):
        g.diversify_sessions([[1000], []], k=2, pool=10)


def test_ragged_or_non_finite_lists():
    g = _model_without_device()
    with pytest.raises(ValueError, match='ragged'):
        g.diversify_lists([[1000, 1001], [1002]], [[1.0, 2.0], [3.0]], k=1)
    with pytest.raises(ValueError, match='one shape'):
        g.diversify_lists(LISTS, REL[:, :3], k=1)
    with pytest.raises(ValueError, match='one shape'):
        g.diversify_lists(LISTS[0], REL[0], k=1)
    with pytest.raises(ValueError, match='one shape'):
        g.diversify_lists(np.zeros((0, 4), dtype=np.int64), np.zeros((0, 4)), k=1)
    for bad in (np.nan, np.inf, -np.inf, 1e39):      # (1e39 is finite as a double, infinite as the float32 the device reads)
        rel = REL.copy()
        rel[1, 2] = bad
        with pytest.raises(ValueError, match='not finite'):
            g.diversify_lists(LISTS, rel, k=1)
    wide = np.full((1, 129), 1000)
    with pytest.raises(ValueError, match='P = 129'):
        g.diversify_lists(wide, np.zeros(wide.shape), k=1)
    with pytest.raises(ValueError, match='P = 0'):
        g.diversify_lists(np.zeros((2, 0), dtype=np.int64), np.zeros((2, 0)), k=1)


def test_valid_arguments_reach_the_device():
    """Valid calls go on to the device model (here: the stand-in that refuses), so the checks above are not vacuous."""
    g = _model_without_device()
    for kw in (dict(), dict(k=128, pool=128), dict(k=1, pool=1, trade_off=0), dict(k=3, pool=4, trade_off=1, metric='dot', normalize=False,
                                                                                 predict_for_item_ids=np.array([1000, 1005, 1005, 1007, 1009])),
               dict(k=20, pool=100, exclude=[1001, 1002], exclude_history=True, return_details=True, return_hidden=True),
               dict(k=2.0, pool=10.0, trade_off=np.float32(0.3))):
        with pytest.raises(AssertionError, match='touched the device'):
            g.diversify_sessions(HIST, **kw)
    for kw in (dict(k=4), dict(k=1, trade_off=0.0, metric='dot'), dict(k=2, trade_off=1, normalize=False)):
        with pytest.raises(AssertionError, match='touched the device'):
            g.diversify_lists(LISTS, REL, **kw)
        with pytest.raises(AssertionError, match='touched the device'):
            g.diversify_lists(LISTS.tolist(), REL.tolist(), **kw)


def test_header_binding_and_library_agree():
    text = open(os.path.join(ROOT, 'include', 'gru4rec_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    lib = _native.lib()
    for name, nargs in (('g4r_diversify_lists', 12), ('g4r_diversify_sessions', 22)):
        decl = re.search(r'int\s+%s\s*\(([^;]*)\)\s*;' % name, code)
        assert decl, '%s is not declared in the header' % name
        args = [a.strip() for a in decl.group(1).split(',')]
        assert len(args) == nargs
        assert name in _native.SYMBOLS
        assert hasattr(lib, name) and len(getattr(lib, name).argtypes) == nargs
    assert re.search(r'#define\s+G4R_DIVERSIFY_POOL_MAX\s+128\b', code)
    assert _native.G4R_DIVERSIFY_POOL_MAX == 128
    assert callable(_native.Model.diversify_lists) and callable(_native.Model.diversify_sessions)


def test_mutant_24_is_listed():
    assert 24 in g4r_build.MUTANTS and 'OVERWRITTEN' in g4r_build.MUTANTS[24]

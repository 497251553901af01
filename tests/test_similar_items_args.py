"""GRU4Rec.similar_items / item_neighbors refuse bad arguments before any device work (no GPU needed): a bad k, metric or space and a
query with too few eligible candidates raise ValueError, an unknown item id KeyError, space='input' on a one-hot model
NotImplementedError; the model is never created.  Header, binding and exported symbol agree on g4r_similar_items, and g4r_config keeps
its size."""
import ctypes
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
        raise AssertionError('similar_items touched the device before checking its arguments')
    g._ensure_model = no_device
    return g


@pytest.mark.parametrize('k', [0, -1, 257, 1000, 2.5, True])
def test_k_out_of_range(k):
    g = _model_without_device()
    with pytest.raises(ValueError, match='k = '):
        g.similar_items([1000, 1001], k=k)
    with pytest.raises(ValueError, match='k = '):
        g.item_neighbors(k=k)


def test_k_above_the_candidate_count():
    g = _model_without_device()
    cand = np.array([1000, 1005, 1005, 1007])       # duplicates count: 4 candidates
    with pytest.raises(ValueError, match='number of candidates = 4'):
        g.similar_items([1000], k=5, predict_for_item_ids=cand)
    with pytest.raises(ValueError, match='number of candidates = 10'):
        _model_without_device(n_items=10).similar_items([1000], k=11)


@pytest.mark.parametrize('kw', [dict(metric='euclid'), dict(metric=None), dict(space='hidden'), dict(space=0)])
def test_bad_metric_or_space(kw):
    g = _model_without_device()
    with pytest.raises(ValueError, match='metric = |space = '):
        g.similar_items([1000], k=5, **kw)
    with pytest.raises(ValueError, match='metric = |space = '):
        g.item_neighbors(k=5, **kw)


def test_unknown_item_ids():
    g = _model_without_device()
    with pytest.raises(KeyError):
        g.similar_items([1000, 7], k=5)
    with pytest.raises(KeyError):
        g.similar_items([1000], k=2, predict_for_item_ids=[1001, 1002, 8])
    with pytest.raises(KeyError):
        g.similar_items([1000], k=2, exclude=[9])
    with pytest.raises(ValueError, match='empty'):
        g.similar_items([], k=2)


def test_input_space_of_a_one_hot_model():
    g = _model_without_device()      # embedding = 0, constrained_embedding = False: one-hot input
    with pytest.raises(NotImplementedError, match="space='output'"):
        g.similar_items([1000], k=5, space='input')
    with pytest.raises(NotImplementedError, match="space='output'"):
        g.item_neighbors(k=5, space='input')
    for kw in (dict(embedding=32), dict(constrained_embedding=True)):
        with pytest.raises(AssertionError, match='touched the device'):
            _model_without_device(**kw).similar_items([1000], k=5, space='input')


def test_too_few_eligible_candidates_names_the_query():
    g = _model_without_device(n_items=10)
    ids = g.itemidmap.index.values
    with pytest.raises(ValueError, match=r'query 0 \(item id 1000\) has 9 eligible candidate positions, fewer than k = 10'):
        g.similar_items([1000], k=10)                                   # the query itself is skipped
    with pytest.raises(ValueError, match=r'query 2 \(item id 1003\) has 7 eligible'):
        g.similar_items([1000, 1001, 1003], k=8, exclude=[1000, 1001])  # queries 0, 1 are excluded anyway: 8 left for them
    cand = np.array([1004, 1005, 1005, 1005, 1006])
    with pytest.raises(ValueError, match=r'query 1 \(item id 1005\) has 2 eligible'):
        g.similar_items([1004, 1005], k=3, predict_for_item_ids=cand)   # every position holding the query counts
    with pytest.raises(ValueError, match=r'query 0 .* has 3 eligible'):
        g.similar_items([1004], k=4, predict_for_item_ids=cand, exclude_self=False, exclude=[1004, 1006, 1006])
    with pytest.raises(ValueError, match='query 0'):
        g.item_neighbors(k=10)
    # the same calls with one neighbour fewer go on to the device
    for call in (lambda: g.similar_items([1000], k=9), lambda: g.similar_items([1000], k=10, exclude_self=False),
                 lambda: g.similar_items([1004, 1005], k=2, predict_for_item_ids=cand), lambda: g.item_neighbors(k=9),
                 lambda: g.similar_items(ids, k=7, exclude=[1000, 1001])):
        with pytest.raises(AssertionError, match='touched the device'):
            call()


def test_valid_arguments_reach_the_device():
    """Valid calls go on to the device model (here: the stand-in that refuses), so the checks above are not vacuous."""
    g = _model_without_device()
    for kw in (dict(k=256), dict(k=1, metric='dot'), dict(k=4, predict_for_item_ids=np.array([1000, 1005, 1005, 1007, 1009])),
               dict(k=20, space='output', exclude=[1001, 1002])):
        with pytest.raises(AssertionError, match='touched the device'):
            g.similar_items(np.array([1000, 1000, 1003]), **kw)


def test_header_binding_and_library_agree():
    text = open(os.path.join(ROOT, 'include', 'gru4rec_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    decl = re.search(r'int\s+g4r_similar_items\s*\(([^;]*)\)\s*;', code)
    assert decl, 'g4r_similar_items is not declared in the header'
    args = [a.strip() for a in decl.group(1).split(',')]
    assert len(args) == 12
    assert 'g4r_similar_items' in _native.SYMBOLS
    lib = _native.lib()
    assert hasattr(lib, 'g4r_similar_items') and len(lib.g4r_similar_items.argtypes) == len(args)
    for name, value in (('G4R_SIM_DOT', 0), ('G4R_SIM_COSINE', 1), ('G4R_SPACE_OUTPUT', 0), ('G4R_SPACE_INPUT', 1)):
        assert re.search(r'#define\s+%s\s+%d\b' % (name, value), code), name
    assert _native.SIM_METRICS == {'dot': 0, 'cosine': 1} and _native.SIM_SPACES == {'output': 0, 'input': 1}
    assert callable(_native.Model.similar_items) and callable(_native.Model.sim_norms)


def test_config_struct_size_is_unchanged():
    assert ctypes.sizeof(_native.G4RConfig) == _native.lib().g4r_sizeof_config() == 184


def test_mutant_13_is_listed():
    assert 13 in g4r_build.MUTANTS and 'POSITION' in g4r_build.MUTANTS[13]


def test_what_k_is_taken_as():
    """2.0 counts as 2; True, 2.5, 0 and number of candidates + 1 are refused with the call's own message; a string and None fail
    inside int(), with int's own error."""
    g = _model_without_device()
    cand = np.array([1000, 1005, 1005, 1007, 1009])
    with pytest.raises(AssertionError, match='touched the device'):
        g.similar_items([1001], k=2.0, predict_for_item_ids=cand)
    for k in (True, 2.5, 0, 6):
        with pytest.raises(ValueError, match='k = %r: it must be an integer in' % (k,)):
            g.similar_items([1001], k=k, predict_for_item_ids=cand)
    with pytest.raises(ValueError, match='invalid literal'):
        g.similar_items([1001], k='a', predict_for_item_ids=cand)
    with pytest.raises(TypeError):
        g.similar_items([1001], k=None, predict_for_item_ids=cand)
    with pytest.raises(ValueError, match='invalid literal'):
        g.item_neighbors(k='a')
    with pytest.raises(TypeError):
        g.item_neighbors(k=None)

"""The item-index keywords of GRU4Rec (build_item_index, item_index, drop_item_index, recommend_sessions(nprobe=, return_probes=)) are
checked before any device work (no GPU needed; the device is stubbed out as in test_recommend_scan_args.py): every refusal is raised
with the model never created, index= is validated, nprobe=None goes on to the unchanged entries."""
import os

import numpy as np
import pandas as pd
import pytest

from gru4rec_amd import _native
from gru4rec_amd import build as g4r_build
from gru4rec_amd.gru4rec import GRU4Rec

N_ITEMS, D, N_LISTS = 3000, 64, 12
HISTS = [[1000, 1001], [1002]]


def _no_device():
    raise AssertionError('the call touched the device before its checks')


def _model_without_device(final_act='linear', index=True):
    g = GRU4Rec(layers=[D], final_act=final_act)
    g.itemidmap = pd.Series(data=np.arange(N_ITEMS), index=np.arange(1000, 1000 + N_ITEMS), name='ItemIdx')
    g.n_items = N_ITEMS
    g.error_during_train = False
    g.Wy = np.zeros((N_ITEMS, D), dtype=np.float32)
    g.By = np.zeros((N_ITEMS, 1), dtype=np.float32)
    g._ensure_model = _no_device
    if index:
        g._item_index = _index_by_indices()
    return g


def _index_by_indices():
    offs = np.linspace(0, N_ITEMS, N_LISTS + 1).astype(np.int64)
    return dict(centroids=np.zeros((N_LISTS, D + 1), dtype=np.float32), list_offs=offs, list_items=np.arange(N_ITEMS, dtype=np.int32))


def _index_by_ids(**over):
    ix = _index_by_indices()
    ix['list_items'] = 1000 + ix['list_items'].astype(np.int64)
    ix.update(over)
    return ix


def test_the_limits_are_the_headers():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'gru4rec_hip.h')).read()
    assert _native.G4R_IVF_WS_MAX == 65536 and '#define G4R_IVF_WS_MAX 65536' in text
    assert '#define G4R_IVF_NPROBE_MAX %d' % _native.G4R_IVF_NPROBE_MAX in text
    assert '#define G4R_IVF_LISTS_MAX %d' % _native.G4R_IVF_LISTS_MAX in text


def test_no_index_is_refused_by_name():
    g = _model_without_device(index=False)
    with pytest.raises(ValueError, match='build_item_index'):
        g.recommend_sessions(HISTS, nprobe=1)
    assert g.item_index() is None


@pytest.mark.parametrize('nprobe', [0, -1, N_LISTS + 1, 2.0, True, '3'])
def test_nprobe_out_of_range(nprobe):
    with pytest.raises(ValueError, match=r'nprobe = .*\[1, n_lists = %d\]' % N_LISTS):
        _model_without_device().recommend_sessions(HISTS, nprobe=nprobe)


def test_nprobe_over_the_probe_limit():
    g = _model_without_device()
    offs = np.concatenate([np.arange(300), [N_ITEMS]]).astype(np.int64)
    g._item_index = dict(centroids=np.zeros((300, D + 1), dtype=np.float32), list_offs=offs, list_items=np.arange(N_ITEMS, dtype=np.int32))
    with pytest.raises(ValueError, match='G4R_IVF_NPROBE_MAX = 256'):
        g.recommend_sessions(HISTS, k=1, oversample=1, nprobe=257)


@pytest.mark.parametrize('kw, word', [(dict(scan='bf16'), "scan='bf16'"), (dict(predict_for_item_ids=[1000, 1001, 1002] * 10), 'predict_for_item_ids'),
                                      (dict(max_per_group=2), 'max_per_group')])
def test_nprobe_with_an_excluded_companion(kw, word):
    with pytest.raises(ValueError, match=word):
        _model_without_device().recommend_sessions(HISTS, nprobe=2, **kw)


def test_unknown_scan_name_keeps_its_message():
    with pytest.raises(ValueError, match="'fp32' or 'bf16'"):
        _model_without_device().recommend_sessions(HISTS, nprobe=2, scan='bf8')


@pytest.mark.parametrize('final_act', ['softmax', 'softmax_logit'])
def test_softmax_is_refused(final_act):
    with pytest.raises(NotImplementedError, match='nprobe'):
        _model_without_device(final_act=final_act).recommend_sessions(HISTS, nprobe=2)


@pytest.mark.parametrize('k, oversample, nprobe', [(256, 4, 65), (128, 8, 65), (20, 8, 410), (256, 100, 65)])
def test_workspace_limit_is_named(k, oversample, nprobe):
    g = _model_without_device()
    offs = np.concatenate([np.arange(500), [N_ITEMS]]).astype(np.int64)
    g._item_index = dict(centroids=np.zeros((500, D + 1), dtype=np.float32), list_offs=offs, list_items=np.arange(N_ITEMS, dtype=np.int32))
    _native_max = _native.G4R_IVF_NPROBE_MAX
    if nprobe > _native_max:
        with pytest.raises(ValueError, match='G4R_IVF_NPROBE_MAX'):
            g.recommend_sessions(HISTS, k=k, oversample=oversample, nprobe=nprobe)
        return
    with pytest.raises(ValueError, match='G4R_IVF_WS_MAX = 65536'):
        g.recommend_sessions(HISTS, k=k, oversample=oversample, nprobe=nprobe)


@pytest.mark.parametrize('oversample', [0, -3, 2.5, True])
def test_bad_oversample(oversample):
    with pytest.raises(ValueError, match='oversample = '):
        _model_without_device().recommend_sessions(HISTS, nprobe=2, oversample=oversample)


def test_the_k_check_comes_first_and_return_probes_needs_nprobe():
    with pytest.raises(ValueError, match='k = '):
        _model_without_device().recommend_sessions(HISTS, k=257, nprobe=2)
    with pytest.raises(ValueError, match='return_probes'):
        _model_without_device().recommend_sessions(HISTS, return_probes=True)


@pytest.mark.parametrize('k, oversample, nprobe', [(20, 8, 1), (20, 8, N_LISTS), (256, 4, N_LISTS), (256, 100, 12), (1, 1, 5)])
def test_valid_values_reach_the_device(k, oversample, nprobe):
    with pytest.raises(AssertionError, match='touched the device'):
        _model_without_device().recommend_sessions(HISTS, k=k, oversample=oversample, nprobe=nprobe)


class _Recorder:
    """Stands in for the native model: records which entry a call is routed to."""
    layers = [D]
    h = 1

    def __init__(self):
        self.calls = []

    def recommend_sessions(self, hist_offs, hist_items, item_idx=None, k=20, excl_offs=None, excl_items=None, excl_mask=None, hidden=None,
                           return_hidden=False, **kw):
        self.calls.append(('recommend_sessions', dict(kw)))
        n = len(hist_offs) - 1
        return np.zeros((n, k), dtype=np.int32), np.zeros((n, k), dtype=np.float32)

    def recommend_sessions_ivf(self, hist_offs, hist_items, k, oversample, nprobe, excl_offs=None, excl_items=None, excl_mask=None, hidden=None,
                               return_hidden=False, return_probes=False):
        self.calls.append(('recommend_sessions_ivf', dict(k=k, oversample=oversample, nprobe=nprobe, lists=excl_offs is not None)))
        n = len(hist_offs) - 1
        out = (np.zeros((n, k), dtype=np.int32), np.zeros((n, k), dtype=np.float32), np.full(n, k, dtype=np.int32))
        return out + ((np.zeros((n, nprobe), dtype=np.int32),) if return_probes else ())

    def ivf_set(self, centroids, list_offs, list_items):
        self.calls.append(('ivf_set', dict(n_lists=len(centroids), first=list(list_items[:3]))))

    def ivf_release(self):
        self.calls.append(('ivf_release', {}))


def test_nprobe_none_takes_the_unchanged_entries_and_an_integer_the_new_one():
    g = _model_without_device()
    rec = _Recorder()
    g._ensure_model = lambda: rec
    g._model = rec
    a = g.recommend_sessions(HISTS, k=5)
    g.recommend_sessions(HISTS, k=5, scan='bf16', oversample=2)
    assert len(a) == 2 and rec.calls == [('recommend_sessions', {}), ('recommend_sessions', {'oversample': 2})]
    rec.calls.clear()
    out = g.recommend_sessions(HISTS, k=5, nprobe=3, exclude_history=True, return_probes=True)
    assert [c[0] for c in rec.calls] == ['ivf_set', 'recommend_sessions_ivf']      # a device model without the index receives it first
    assert rec.calls[1][1] == dict(k=5, oversample=8, nprobe=3, lists=True)
    assert len(out) == 4 and out[0].shape == (2, 5) and out[2].dtype == np.int32 and out[3].shape == (2, 3)
    rec.calls.clear()
    g.recommend_sessions(HISTS, k=5, nprobe=3)
    assert [c[0] for c in rec.calls] == ['recommend_sessions_ivf']
    g.drop_item_index()
    assert rec.calls[-1][0] == 'ivf_release' and g.item_index() is None
    with pytest.raises(ValueError, match='build_item_index'):
        g.recommend_sessions(HISTS, k=5, nprobe=3)


def test_default_n_lists():
    f = GRU4Rec._index_n_lists
    assert f(None, 10 ** 7) == 12649 and f(None, 37483) == 774 and f(None, 20000) == 566 and f(None, 1) == 1 and f(None, 3) == 3
    assert f(7, 1003) == 7 and f(65536, 10 ** 7) == 65536
    for bad, n in ((0, 100), (65537, 10 ** 7), (101, 100), (2.5, 100), (True, 100)):
        with pytest.raises(ValueError, match='n_lists = '):
            f(bad, n)


def test_build_needs_a_model_and_checks_its_arguments_first():
    with pytest.raises(ValueError, match='fitted or loaded'):
        GRU4Rec(layers=[D]).build_item_index()
    g = _model_without_device(index=False)
    for kw in (dict(n_lists=0), dict(n_lists=N_ITEMS + 1), dict(iters=-1), dict(sample_per_list=0),
               dict(centroids=np.zeros((4, D), dtype=np.float32)), dict(centroids=np.zeros((4, D + 1))),
               dict(centroids=np.full((4, D + 1), np.nan, dtype=np.float32))):
        with pytest.raises(ValueError):
            g.build_item_index(**kw)
    with pytest.raises(AssertionError, match='touched the device'):
        g.build_item_index(n_lists=4)


def test_index_argument_is_validated():
    g = _model_without_device(index=False)
    ids = _index_by_ids()['list_items']
    twice = ids.copy()
    twice[5] = twice[4]
    offs = _index_by_ids()['list_offs']
    down = offs.copy()
    down[3], down[4] = offs[4], offs[3]
    cases = [({'list_items': twice}, 'permutation'), ({'list_items': ids[:-1]}, 'permutation'), ({'list_offs': offs[:-1]}, 'list_offs'),
             ({'list_offs': down}, 'monoton'), ({'list_offs': offs + 1}, 'list_offs'),
             ({'centroids': np.zeros((N_LISTS, D), dtype=np.float32)}, 'centroids'), ({'centroids': np.zeros((N_LISTS, D + 1))}, 'centroids'),
             ({'centroids': np.full((N_LISTS, D + 1), np.inf, dtype=np.float32)}, 'finite')]
    for over, word in cases:
        with pytest.raises(ValueError, match=word):
            g.build_item_index(index=_index_by_ids(**over))
    with pytest.raises(ValueError, match='dict'):
        g.build_item_index(index=[1, 2, 3])
    with pytest.raises(KeyError):
        g.build_item_index(index=_index_by_ids(list_items=ids + 10 ** 6))
    with pytest.raises(AssertionError, match='touched the device'):
        g.build_item_index(index=_index_by_ids())


def test_index_argument_round_trip_through_the_stub():
    g = _model_without_device(index=False)
    rec = _Recorder()
    g._ensure_model = lambda: rec
    g._model = rec
    ix = _index_by_ids()
    ix['list_items'] = ix['list_items'][::-1].copy()      # the order within a list carries nothing: every list is sorted again
    ix['list_offs'] = (N_ITEMS - ix['list_offs'][::-1]).copy()
    stats = g.build_item_index(index=ix)
    assert rec.calls == [('ivf_set', dict(n_lists=N_LISTS, first=[2750, 2751, 2752]))]
    assert stats['n_lists'] == N_LISTS and stats['list_len_min'] == stats['list_len_max'] == 250 and stats['empty_lists'] == 0
    assert set(stats) == {'n_lists', 'list_len_min', 'list_len_mean', 'list_len_max', 'empty_lists', 'seconds_kmeans', 'seconds_assign',
                          'seconds_upload'}
    back = g.item_index()
    assert back['list_items'][0] == 3750 and back['list_offs'].dtype == np.int64 and back['centroids'].shape == (N_LISTS, D + 1)
    assert not any(key.startswith('_item_index') for key in g.__getstate__())      # savemodel does not pickle the index


def test_native_binding_declares_the_new_entries_and_the_mutant():
    lib = _native.lib()
    for name in ('g4r_ivf_assign', 'g4r_ivf_set', 'g4r_ivf_release', 'g4r_recommend_sessions_ivf'):
        assert name in _native.SYMBOLS and hasattr(lib, name)
    assert 31 in g4r_build.MUTANTS and 'last block' in g4r_build.MUTANTS[31]

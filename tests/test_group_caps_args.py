"""Item groups and per-group caps without a GPU: set_item_groups' semantics and its pickle round trip; max_per_group / pool /
count_history / exclude_groups / cap_lists refuse bad arguments before any device work (the model is never created); the NumPy
statement of the cap rule equals the plain walk with one counter per group; exclude_groups packs what the equivalent exclude= packs;
header, binding and exported symbols agree on the new entries."""
import os
import re

import numpy as np
import pandas as pd
import pytest

import group_caps_ref as ref
from gru4rec_amd import _native
from gru4rec_amd import build as g4r_build
from gru4rec_amd.gru4rec import GRU4Rec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model_without_device(n_items=300, groups=True, **kw):
    g = GRU4Rec(layers=[64], final_act='linear', **kw)
    # what fit() would leave behind (fitting needs a GPU): the item id map; the device model is never to be created here
    g.itemidmap = pd.Series(data=np.arange(n_items), index=np.arange(1000, 1000 + n_items), name='ItemIdx')
    g.n_items = n_items
    g.error_during_train = False
    if groups:      # item index i: ungrouped when i % 7 == 0, otherwise group 'g<i % 5>'
        g.set_item_groups({1000 + i: 'g%d' % (i % 5) for i in range(n_items) if i % 7})

    def no_device():
        raise AssertionError('the call touched the device before checking its arguments')
    g._ensure_model = no_device
    return g


HIST = [[1000, 1001], [1005]]
LISTS = np.array([[1000, 1001, 1002, 1003], [1003, 1003, 1004, 1005]])


# ---- set_item_groups ------------------------------------------------------------------------------------------------------------------
def test_set_item_groups_semantics():
    g = _model_without_device(n_items=20, groups=False)
    assert g.item_groups is None and g.group_labels is None
    g.set_item_groups({1003: 'b', 1001: 'a', 1010: 'b', 1019: ('tuple', 1)})
    assert g.item_groups.dtype == np.int32 and g.item_groups.shape == (20,)
    want = np.full(20, -1)
    want[[3, 10]] = 0      # dense indices in the order the labels first appear
    want[1] = 1
    want[19] = 2
    np.testing.assert_array_equal(g.item_groups, want)
    assert list(g.group_labels) == ['b', 'a', ('tuple', 1)]
    g.set_item_groups(pd.Series({1000: 7, 1002: 9, 1004: 7}))
    np.testing.assert_array_equal(g.item_groups[:5], [0, -1, 1, -1, 0])
    assert (g.item_groups[5:] == -1).all() and g.group_labels.tolist() == [7, 9]
    with pytest.raises(KeyError):
        g.set_item_groups({1000: 'a', 5: 'a'})
    np.testing.assert_array_equal(g.item_groups[:5], [0, -1, 1, -1, 0])      # a refused call changes nothing
    with pytest.raises(ValueError, match='dict'):
        g.set_item_groups([1, 2, 3])
    g.set_item_groups({})
    assert (g.item_groups == -1).all() and len(g.group_labels) == 0
    g.set_item_groups(None)
    assert g.item_groups is None and g.group_labels is None
    with pytest.raises(ValueError, match='item id map'):
        GRU4Rec(layers=[8]).set_item_groups({1: 'a'})


def test_groups_are_pickled_with_the_model(tmp_path):
    g = _model_without_device(n_items=40)
    del g._ensure_model
    g.Wy = np.zeros((40, 64), dtype=np.float32)
    path = str(tmp_path / 'model.pickle')
    g.savemodel(path)
    h = GRU4Rec.loadmodel(path)
    np.testing.assert_array_equal(h.item_groups, g.item_groups)
    assert h.item_groups.dtype == np.int32 and list(h.group_labels) == list(g.group_labels)
    g.set_item_groups(None)
    g.savemodel(path)
    h = GRU4Rec.loadmodel(path)
    assert h.item_groups is None and h.group_labels is None
    # a state without the attributes (a pickle of an earlier version, or of the reference)
    st = g.__getstate__()
    del st['item_groups'], st['group_labels']
    old = GRU4Rec.__new__(GRU4Rec)
    old.__setstate__(st)
    assert old.item_groups is None and old.group_labels is None


def test_run_py_item_groups_option(tmp_path):
    import importlib.util
    spec = importlib.util.spec_from_file_location('run_py_for_groups', os.path.join(ROOT, 'run.py'))
    run = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(run)
    o = run.build_parser().parse_args(['model.pickle', '-l'])
    assert o.item_groups is None
    o = run.build_parser().parse_args(['model.pickle', '-l', '--item_groups', 'groups.tsv', '-s', 'out.pickle'])
    assert o.item_groups == 'groups.tsv'
    g = _model_without_device(n_items=10, groups=False)
    path = tmp_path / 'groups.tsv'
    path.write_text('1001\tacme\n1003\tzenith\n1004\tacme\n77\tnot in the model\n1003\tacme\n')      # (the last row of an item wins)
    run.set_item_groups(g, str(path))
    np.testing.assert_array_equal(g.item_groups, [-1, 0, -1, 0, 0, -1, -1, -1, -1, -1])
    assert g.group_labels.tolist() == ['acme']


# ---- the cap rule ---------------------------------------------------------------------------------------------------------------------
def test_numpy_rule_equals_the_counter_walk():
    rng = np.random.RandomState(3)
    seen_short = seen_full = 0
    for _ in range(400):
        P = int(rng.randint(1, 70))
        n_groups = int(rng.randint(1, 8))
        g = rng.randint(-1, n_groups, size=P)
        k = int(rng.randint(1, P + 1))
        cap = int(rng.randint(1, 5))
        prior = rng.randint(0, n_groups, size=rng.randint(0, 6))
        pos, n = ref.cap_rule(g, k, cap, prior)
        pos2, n2 = ref.cap_walk(g, k, cap, prior)
        np.testing.assert_array_equal(pos, pos2)
        assert n == n2 and (pos[:n] >= 0).all() and (pos[n:] == -1).all() and (np.diff(pos[:n]) > 0).all()
        seen_short += n < k
        seen_full += n == k
    assert seen_short > 20 and seen_full > 20
    # by hand: groups 0 0 1 0 -1 1 1, cap 2, a prior that holds one 1
    pos, n = ref.cap_rule([0, 0, 1, 0, -1, 1, 1], 7, 2, [1])
    assert pos.tolist() == [0, 1, 2, 4, -1, -1, -1] and n == 4
    pos, n = ref.cap_rule([0, 0, 1, 0, -1, 1, 1], 3, 2, [1])
    assert pos.tolist() == [0, 1, 2] and n == 3
    pos, n = ref.cap_rule([2, 2], 2, 1, [2])      # the prior already fills the group
    assert pos.tolist() == [-1, -1] and n == 0


# ---- refusals, all before the device ------------------------------------------------------------------------------------------------------
def test_no_group_table():
    g = _model_without_device(groups=False)
    with pytest.raises(ValueError, match='set_item_groups'):
        g.recommend_sessions(HIST, k=2, max_per_group=1)
    with pytest.raises(ValueError, match='set_item_groups'):
        g.continue_sessions(HIST, 2, max_per_group=1)
    with pytest.raises(ValueError, match='set_item_groups'):
        g.cap_lists(LISTS, 2, 1)
    for call in (lambda: g.recommend_sessions(HIST, k=2, exclude_groups=['g1']), lambda: g.continue_sessions(HIST, 2, exclude_groups=['g1']),
                 lambda: g.diversify_sessions(HIST, k=2, pool=10, exclude_groups=['g1'])):
        with pytest.raises(ValueError, match='set_item_groups'):
            call()


@pytest.mark.parametrize('cap', [0, -1, 1.5, True, 'a', 2 ** 31])
def test_cap_out_of_range(cap):
    g = _model_without_device()
    with pytest.raises(ValueError, match='max_per_group = '):
        g.recommend_sessions(HIST, k=2, max_per_group=cap)
    with pytest.raises(ValueError, match='max_per_group = '):
        g.continue_sessions(HIST, 2, max_per_group=cap)
    with pytest.raises(ValueError, match='max_per_group = '):
        g.cap_lists(LISTS, 2, cap)
    with pytest.raises(ValueError, match='max_per_group = '):
        g.cap_lists(LISTS, 2, None)


@pytest.mark.parametrize('pool', [0, -3, 257, 301, 2.5, True, 'x'])
def test_pool_out_of_range(pool):
    g = _model_without_device()
    with pytest.raises(ValueError, match='pool = '):
        g.recommend_sessions(HIST, k=1, max_per_group=1, pool=pool)
    with pytest.raises(ValueError, match='pool = '):
        g.continue_sessions(HIST, 2, max_per_group=1, pool=pool)


def test_pool_k_and_the_options_that_need_max_per_group():
    g = _model_without_device()
    with pytest.raises(ValueError, match='k = 5.*pool = 4'):
        g.recommend_sessions(HIST, k=5, max_per_group=1, pool=4)
    with pytest.raises(ValueError, match='k = 5.*pool = 4'):
        g.continue_sessions(HIST, 2, k=5, max_per_group=1, pool=4)
    with pytest.raises(ValueError, match='pool = 5.*number of candidates = 4'):
        g.recommend_sessions(HIST, k=2, max_per_group=1, pool=5, predict_for_item_ids=np.array([1000, 1005, 1005, 1007]))
    with pytest.raises(ValueError, match='max_per_group, which is None'):
        g.recommend_sessions(HIST, k=2, pool=10)
    with pytest.raises(ValueError, match='max_per_group, which is None'):
        g.continue_sessions(HIST, 2, count_history=True)
    # the scan's limit counts the pool
    with pytest.raises(ValueError, match='k \\* oversample = 100 \\* 11'):
        g.recommend_sessions(HIST, k=2, max_per_group=1, pool=100, scan='bf16', oversample=11)
    # cap_lists: P, k, ragged lists, the prior's length, unknown ids
    with pytest.raises(ValueError, match='k = 5'):
        g.cap_lists(LISTS, 5, 1)
    with pytest.raises(ValueError, match='P = 257'):
        g.cap_lists(np.full((1, 257), 1000), 1, 1)
    with pytest.raises(ValueError, match='ragged'):
        g.cap_lists([[1000, 1001], [1002]], 1, 1)
    with pytest.raises(ValueError, match='prior holds 1 lists'):
        g.cap_lists(LISTS, 2, 1, prior=[[1000]])
    with pytest.raises(KeyError):
        g.cap_lists(LISTS, 2, 1, prior=[[1000], [5]])
    with pytest.raises(KeyError):
        g.cap_lists(np.array([[1000, 7]]), 1, 1)
    with pytest.raises(KeyError, match='unknown group label'):
        g.recommend_sessions(HIST, k=2, exclude_groups=['g1', 'nope'])


def test_default_pool_and_the_eligible_positions_it_needs():
    g = _model_without_device(n_items=20)
    # pool = min(256, candidates, 4 k) = 20 > the 18 eligible positions of row 0
    with pytest.raises(ValueError, match='row 0 has 18 eligible candidate positions, fewer than k = 20'):
        g.recommend_sessions(HIST, k=5, max_per_group=1, exclude_history=True)
    with pytest.raises(ValueError, match='row 0 has 18 eligible candidate positions, fewer than k = 19'):
        g.recommend_sessions(HIST, k=5, max_per_group=1, pool=19, exclude_history=True)
    with pytest.raises(AssertionError, match='touched the device'):
        g.recommend_sessions(HIST, k=5, max_per_group=1, pool=18, exclude_history=True)
    # continuation: pool + steps - 1 eligible positions
    with pytest.raises(ValueError, match='row 0 has 18 eligible candidate positions, fewer than k \\+ steps - 1 = 19'):
        g.continue_sessions(HIST, 4, k=2, max_per_group=1, pool=16)
    with pytest.raises(AssertionError, match='touched the device'):
        g.continue_sessions(HIST, 3, k=2, max_per_group=1, pool=16)


def test_prior_list_too_long():
    g = _model_without_device()
    long_hist = [[1001] * 1024, [1005]]      # (item index 1: grouped)
    with pytest.raises(ValueError, match='row 0 has 1024 prior groups and gains steps - 1 = 1 more, more than G4R_GROUP_PRIOR_MAX = 1024'):
        g.continue_sessions(long_hist, 2, max_per_group=2, count_history=True)
    with pytest.raises(AssertionError, match='touched the device'):
        g.continue_sessions(long_hist, 1, max_per_group=2, count_history=True)
    with pytest.raises(AssertionError, match='touched the device'):
        g.continue_sessions([[1000] * 2000, [1005]], 2, max_per_group=2, count_history=True)      # ungrouped items do not count
    with pytest.raises(ValueError, match='row 1 has 1025 prior groups, more than'):
        g.cap_lists(LISTS, 2, 1, prior=[[1000], [1001] * 1025])
    with pytest.raises(ValueError, match='more than G4R_GROUP_PRIOR_MAX'):
        g.continue_sessions(HIST, 1026, max_per_group=2, no_repeat=False)


def test_valid_arguments_reach_the_device():
    g = _model_without_device()
    for kw in (dict(k=2, max_per_group=1), dict(k=20, max_per_group=3, pool=256), dict(k=1, max_per_group=2 ** 31 - 1, pool=1),
               dict(k=5, max_per_group=2, pool=100, scan='bf16', oversample=10, exclude_groups=['g1'], exclude_history=True, return_hidden=True),
               dict(k=3, max_per_group=1, predict_for_item_ids=np.array([1000, 1005, 1005, 1007, 1009]))):
        with pytest.raises(AssertionError, match='touched the device'):
            g.recommend_sessions(HIST, **kw)
    for kw in (dict(max_per_group=1), dict(k=5, max_per_group=2, pool=64, count_history=True, no_repeat=False), dict(exclude_groups=['g0', 'g2'])):
        with pytest.raises(AssertionError, match='touched the device'):
            g.continue_sessions(HIST, 3, **kw)
    for kw in (dict(), dict(prior=[[1001, 1002], []]), dict(prior=[np.array([1001]), np.array([], dtype=np.int64)])):
        with pytest.raises(AssertionError, match='touched the device'):
            g.cap_lists(LISTS, 2, 1, **kw)
    with pytest.raises(AssertionError, match='touched the device'):
        g.diversify_sessions(HIST, k=2, pool=10, exclude_groups=['g3'])


# ---- exclude_groups is exclude= ---------------------------------------------------------------------------------------------------------------
def test_exclude_groups_packs_what_the_equivalent_exclude_packs():
    g = _model_without_device(n_items=120)
    ids = g.itemidmap.index.values
    labels = ['g1', 'g4']
    members = ids[np.isin(g.item_groups, [g.group_labels.tolist().index(x) for x in labels])]
    assert len(members) == sum(1 for i in range(120) if i % 7 and i % 5 in (1, 4))
    gidx, mask = g._global_exclude(None, labels)
    gidx2, mask2 = g._global_exclude(members)
    np.testing.assert_array_equal(gidx, gidx2)
    np.testing.assert_array_equal(mask, mask2)
    # merged with exclude=
    extra = ids[[0, 7, 11]]
    gidx, mask = g._global_exclude(extra, labels)
    gidx2, mask2 = g._global_exclude(np.concatenate([members, extra]))
    np.testing.assert_array_equal(gidx, gidx2)
    np.testing.assert_array_equal(mask, mask2)
    gidx, mask = g._global_exclude(None, [])
    assert len(gidx) == 0 and mask is None
    # the eligibility arithmetic sees it: the same packed lists, the same counts in the refusal
    for cand in (None, ids[np.r_[0:60, 0:10]]):
        cidx = None if cand is None else g.itemidmap[cand].values
        per_row = [ids[[1, 2, 3]], ids[[6, 9]]]
        a = g._pack_exclusions(2, 5, cidx, None, 'x', None, per_row, exclude_groups=labels)
        b = g._pack_exclusions(2, 5, cidx, None, 'x', members, per_row)
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)
        msgs = []
        for kw in (dict(exclude_groups=labels), dict(exclude=members)):
            with pytest.raises(ValueError, match='eligible candidate positions') as e:
                g.recommend_sessions(HIST, k=len(ids) if cand is None else len(cand), predict_for_item_ids=cand, exclude_history=True, **kw)
            msgs.append(str(e.value))
        assert msgs[0] == msgs[1]


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree():
    text = open(os.path.join(ROOT, 'include', 'gru4rec_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    lib = _native.lib()
    for name, nargs in (('g4r_set_item_groups', 3), ('g4r_get_item_groups', 3), ('g4r_recommend_sessions_capped', 19),
                        ('g4r_continue_sessions_capped', 22), ('g4r_cap_lists', 10)):
        decl = re.search(r'int\s+%s\s*\(([^;]*)\)\s*;' % name, code)
        assert decl, '%s is not declared in the header' % name
        args = [a.strip() for a in decl.group(1).split(',')]
        assert len(args) == nargs
        assert name in _native.SYMBOLS
        assert hasattr(lib, name) and len(getattr(lib, name).argtypes) == nargs
    assert re.search(r'#define\s+G4R_GROUP_PRIOR_MAX\s+1024\b', code)
    assert _native.G4R_GROUP_PRIOR_MAX == 1024
    for name in ('set_item_groups', 'get_item_groups', 'recommend_sessions_capped', 'continue_sessions_capped', 'cap_lists'):
        assert callable(getattr(_native.Model, name))


def test_mutant_26_is_listed():
    assert 26 in g4r_build.MUTANTS and 'OWN wave' in g4r_build.MUTANTS[26]

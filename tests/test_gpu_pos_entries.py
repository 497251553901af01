"""The per-item (last + 1, R - first, count) entries of a step written once per window, by position (k_owner_window's entry ring, debug
keys pos_entries / pos_entries_ring), against the form that builds them inside every step with atomics in k_gru_v / k_score_s and
takes them back in k_update_l (G4R_POS_ENTRIES=0, read at create): the same values feed the same branches, so the same bits -- losses,
item tables, accumulators, velocities, dense parameters, H.
(a) after one 16-step window every slot of the ring equals the host rule (test_pos_entries_rule.py) for that step's plan row and store
    row -- both table rules, -1 positions, a hot item whose counts are far past 15;
(b) T = 23 steps (a 16-step replay, a 4-step replay and three eager steps where the sample store lets a run go that far), graph and
    eager, as one call and as 9 + 14, at the shapes of tests/test_gpu_owner_window.py and its doctored plans; a list just past the
    form's LDS cap reports pos_entries == 0 and still matches; per-kernel profiling switched on in the middle of a run -- plain, and with
    the split update, which falls back to the in-step form for those steps -- leaves the bits alone, against the run without it and
    against the same profiled run under G4R_POS_ENTRIES=0."""
import numpy as np
import pytest

from test_gpu_parity import make_pair
from test_gpu_owner_window import BPR, CASES, RING, T, _env, _plan, _same_bits, _state
from test_owner_window_rule import occurrences
from test_pos_entries_rule import check_entries

# R = 2 * 32 + 5398 = 5462: one id more than the 8192-slot hash of k_owner_window holds at 1.5 slots per id (R <= 5461)
PAST_CAP = (2000, 32, 5398, 24, None, 0, dict(BPR, layers=(16,)))
ALL = dict(CASES, past_the_lds_cap=PAST_CAP)


def _make(case, graph, entries):
    I, B, ns, store_rows, hot, empty, kw = ALL[case]
    support = None
    if hot is not None:
        support = np.ones(I)
        support[0] = hot
    with _env(G4R_POS_ENTRIES=None if entries else '0', G4R_OWNER_WINDOW=None, G4R_OWNER_SCAN=None):      # (read at create)
        return make_pair(I, B, ns, store_rows=store_rows, support=support, use_graph=graph, **dict(kw))


def _run(case, graph, entries, calls=(T,), profile_at=None):
    """profile_at = (call index, mode): per-kernel profiling in that mode for that call alone."""
    I, B, ns, store_rows, hot, empty, kw = ALL[case]
    o, m = _make(case, graph, entries)
    try:
        assert int(m.get_debug('lean', 4)[3]) == 1, 'k_update_l was not chosen for %s' % case
        assert int(m.get_debug('owner_window', 1)[0]) == 1
        assert int(m.get_debug('pos_entries', 1)[0]) == (1 if entries and case != 'past_the_lds_cap' else 0)
        m.set_plan(_plan(I, B, T, o.ST if ns else None, empty))
        t = 0
        for i, n in enumerate(calls):
            if profile_at and profile_at[0] == i:
                m.profile(profile_at[1])
            m.train_steps(t, n)
            if profile_at and profile_at[0] == i:
                m.profile(False)
            t += n
        assert t == T
        out = _state(m, I, kw, T)
        for l, Dl in enumerate(kw['layers']):
            out['H%d' % l] = m.get_param('H', (B, Dl), l).copy()
        return out
    finally:
        m.close()


_REF = {}


def _ref(case, graph):
    """The in-step form (G4R_POS_ENTRIES=0), one call: computed once per (case, graph) and left alone."""
    if (case, graph) not in _REF:
        _REF[case, graph] = _run(case, graph, entries=False)
        assert np.isfinite(_REF[case, graph]['loss']).all()
    return _REF[case, graph]


@pytest.mark.gpu
@pytest.mark.parametrize('graph', [0, 1])
@pytest.mark.parametrize('case', sorted(ALL))
def test_entries_by_position_bit_identical_to_the_entries_built_in_the_step(case, graph):
    ref = _ref(case, graph)
    _same_bits(_run(case, graph, entries=True), ref)
    _same_bits(_run(case, graph, entries=True, calls=(9, 14)), ref)


@pytest.mark.gpu
@pytest.mark.parametrize('mode', [True, 2])
def test_profiling_in_the_middle_of_a_run_leaves_the_bits_alone(mode):
    """Steps 9 .. 13 run eagerly under per-kernel profiling: mode 2 times the split update, whose steps take the null slot (entries
    through occ_fl, owner table from the pre-scan in k_loss_rows), between replays that take theirs from the ring.  The split update of
    a step that ends in k_update_l is k_update_l's own two halves as two launches (dense tiles; bookkeeping + row workgroups): the same
    code on the same operands, hence the same bits.  (Timed as k_dense_grad<32> + k_sparse_update, whose tiles add the batch up in
    another order, the five profiled steps left 5 of the 23 losses off by 1 ulp and 14 tensors different.)"""
    case = 'cfg2_shape_refill_at_12'
    _same_bits(_run(case, 1, entries=True, calls=(9, 5, 9), profile_at=(1, mode)), _ref(case, 1))


@pytest.mark.gpu
@pytest.mark.parametrize('mode', [True, 2])
def test_profiled_steps_fall_back_to_the_same_bits(mode):
    """The same run -- profiling for steps 9 .. 13 -- with the entries by position and with G4R_POS_ENTRIES=0: bit for bit, in mode 2
    too (its steps run the in-step form either way; the replays around them switch forms and find occ_fl all zero)."""
    case = 'cfg2_shape_refill_at_12'
    _same_bits(_run(case, 1, entries=True, calls=(9, 5, 9), profile_at=(1, mode)),
               _run(case, 1, entries=False, calls=(9, 5, 9), profile_at=(1, mode)))


RING_CASES = {
    # name: (I, B, ns, store_rows, hot, M = 0 steps at the end, kwargs); 16 steps, no refill inside them
    'cfg2_shape': (RING['I'], RING['B'], RING['ns'], RING['store_rows'], None, 0, dict(BPR, layers=(100,))),
    'two_tables': CASES['two_tables'],
    'hot_item': CASES['hot_item'],
    'ragged_tail_then_empty_steps': CASES['ragged_tail_then_empty_steps'],
    'no_samples': CASES['no_samples'],
}


def check_every_slot(name):
    """One 16-step graph window: the entries of EVERY slot of the ring against the host rule for that step's plan row and store row.
    Returns the number of positions, over the window, of repeated items that occur only among the sampled negatives."""
    I, B, ns, rows, hot, empty, kw = RING_CASES[name]
    n_steps = 16
    support = None
    if hot is not None:
        support = np.ones(I)
        support[0] = hot
    with _env(G4R_POS_ENTRIES=None, G4R_OWNER_WINDOW=None, G4R_OWNER_SCAN=None):
        o, m = make_pair(I, B, ns, store_rows=rows, support=support, use_graph=1, **dict(kw))
    try:
        assert int(m.get_debug('pos_entries', 1)[0]) == 1
        plan = _plan(I, B, n_steps, o.ST if ns else None, empty)
        m.set_plan(plan)
        m.train_steps(0, n_steps)
        assert int(m.get_debug('graph_mode', 1)[0]) == 1
        R = 2 * B + ns
        Rp = (R + 3) // 4 * 4
        ring = m.get_debug('pos_entries_ring', (16 * Rp * 4,)).view(np.int32).reshape(16, Rp, 4)
        constrained = bool(kw['constrained_embedding'])
        negatives_only = 0
        for t in range(n_steps):
            occ = occurrences(plan, o.ST if ns else None, t, t % rows if ns else 0, B, ns)
            negatives_only += check_entries(ring[t], occ, B, constrained)
        if empty:
            assert not ring[n_steps - empty:].any()      # M = 0: every position holds -1, every entry zeros
        occ_dev = m.get_debug('occ_idx', (R,)).view(np.int32)
        np.testing.assert_array_equal(occ_dev[:int(plan['M'][-1])], plan['in_idx'][-1, :int(plan['M'][-1])])      # occ_idx keeps its contents
        return negatives_only
    finally:
        m.close()


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(RING_CASES))
def test_every_slot_of_the_ring_holds_its_steps_entries(name):
    n = check_every_slot(name)
    if name in ('cfg2_shape', 'two_tables', 'ragged_tail_then_empty_steps'):      # (hot_item: 8 items, every one of them also in X | Y)
        assert n > 0, 'no repeated item among the negatives alone: the case does not reach what the owner tables never look at'

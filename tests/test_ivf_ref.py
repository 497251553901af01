"""The float64 helpers of the item-index tests (tests/ivf_ref.py) on hand-made cases, and the share of ambiguous answers on random
tables shaped like the GPU test models (no GPU needed)."""
import numpy as np
import pytest

import ivf_ref


def test_objective_and_tau_by_hand():
    V = np.array([[3.0, 4.0, 0.0], [0.0, 0.0, 2.0]])
    cen = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, 2.0, 0.0]])
    J, tau = ivf_ref.assign_objective(V, cen)
    np.testing.assert_allclose(J, [[3 - 0.5, 0 - 0.5, 8 - 2.0], [-0.5, 2 - 0.5, -2.0]])
    np.testing.assert_allclose(tau[0], 5 * 2.0 ** -24 * np.array([5 * 1 + 0.5, 5 * 1 + 0.5, 5 * 2 + 2.0]))
    ok, amb = ivf_ref.check_assignment(V, cen, [2, 1])
    assert ok.all() and amb == 0.0
    ok, _ = ivf_ref.check_assignment(V, cen, [0, 1])
    assert list(ok) == [False, True]


def test_a_tie_accepts_both_lists_and_counts_as_ambiguous():
    V = np.array([[1.0, 1.0, 0.0]])
    cen = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0]])      # J = 0.5, 0.5, -1.5
    for lst, want in ((0, True), (1, True), (2, False)):
        ok, amb = ivf_ref.check_assignment(V, cen, [lst])
        assert ok[0] == want and amb == 1.0


def test_a_gap_of_a_few_ulps_is_within_the_bound_and_a_real_gap_is_not():
    V = np.array([[1.0, 0.0, 0.0]])
    J, tau = ivf_ref.assign_objective(V, np.array([[1.0, 0.0, 0.0], [1.0 - 2.0 ** -23, 0.0, 0.0], [0.9, 0.0, 0.0]]))
    acc = ivf_ref.acceptable(J, tau)
    assert list(acc[0]) == [True, True, False]


def test_probe_rule_by_hand():
    H = np.array([[1.0, 2.0], [0.0, 0.0]])
    cen = np.array([[1.0, 0.0, 0.5], [0.0, 1.0, 0.0], [0.0, 0.0, 0.25], [-1.0, -1.0, 0.0]])
    s, tau = ivf_ref.probe_scores(H, cen)
    np.testing.assert_allclose(s, [[1.5, 2.0, 0.25, -3.0], [0.5, 0.0, 0.25, 0.0]])
    np.testing.assert_allclose(tau[0], 5 * 2.0 ** -24 * np.array([np.sqrt(5) + 0.5, np.sqrt(5), 0.25, np.sqrt(10)]))
    ok, amb = ivf_ref.check_probes(s, tau, [[1, 0], [0, 2]])
    assert ok.all() and amb == 0.0
    for bad in ([[0, 1], [0, 2]], [[1, 0], [0, 1]], [[1, 1], [0, 2]], [[1, 0], [2, 0]], [[1, 4], [0, 2]]):
        assert not ivf_ref.check_probes(s, tau, bad)[0].all(), bad
    # row 1: lists 1 and 3 tie at 0.0 exactly, and the cut of three probes falls between them: either is acceptable, both are counted
    ok, amb = ivf_ref.check_probes(s, tau, [[1, 0, 2], [0, 2, 3]])
    assert ok.all() and amb == 1 / 8.0


def test_topk_by_contract():
    sc = np.array([1.0, np.nan, 2.0, 1.0, -0.0, 0.0], dtype=np.float32)
    items = np.array([9, 1, 5, 3, 8, 7])
    assert list(ivf_ref.topk_by_contract(sc, items, 6)) == [2, 3, 0, 5, 4, 1]      # 1.0: item 3 before 9; -0.0 == 0.0: item 7 before 8
    assert list(ivf_ref.topk_by_contract(sc, items, 2)) == [2, 3]


@pytest.mark.parametrize('n, D, n_lists', [(20000, 64, 64), (20000, 100, 200), (1003, 36, 7)])
def test_random_tables_are_hardly_ever_ambiguous(n, D, n_lists):
    rng = np.random.RandomState(D)
    V = rng.randn(n, D + 1) * 0.3
    cen = V[rng.choice(n, n_lists, replace=False)] * 0.8
    _, amb = ivf_ref.check_assignment(V, cen, np.zeros(n, dtype=int))
    H = np.tanh(rng.randn(130, D))
    s, tau = ivf_ref.probe_scores(H, cen)
    order = np.argsort(-s, axis=1, kind='stable')
    ok, amb_p = ivf_ref.check_probes(s, tau, order[:, :min(4, n_lists)])
    print('%d x %d, %d lists: ambiguous items %.5f, ambiguous (row, list) pairs %.5f' % (n, D, n_lists, amb, amb_p))
    assert ok.all() and amb <= 0.01 and amb_p <= 0.01

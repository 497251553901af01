"""The cases of tests/test_gpu_loss_rows.py without a device: the FLOAT32 oracle stands in for the kernel and goes through the same
comparison against the float64 oracle, so the inputs are known to keep the reference alone inside the bounds, and the harness is
known to be right, before either sees a GPU.  The distances measured on the way justify the coefficients: A_ORD and A_EXT must be
at least 8 x the float32 oracle's largest distance and at most 1e-4.  And the per-row losses of loss_fwd_bwd(per_row=True) sum to
what the function returns without it, for every loss."""
import numpy as np
import pytest

import test_gpu_loss_rows as lr
from oracle.model import final_act_fwd, loss_fwd_bwd, parse_act

@pytest.fixture(scope='module')
def oracle32_runs():
    """Every case once, the float32 oracle in the device's place: ({case: names of what failed}, {kind: largest distance}).  Shared by
    the tests below, so each of them stands on its own whatever is selected and in whatever order."""
    failed, measured = {}, {}

    def measure(kind, value):
        measured[kind] = max(measured.get(kind, 0.0), value)

    for ftag, gtag in lr.CASES:
        _, _, B, N, ld, _, _ = lr.GEO[gtag]
        errs = []
        lr.run_case(ftag, gtag, lambda cfg, X, M, B=B, N=N: lr.oracle32_as_device(cfg, X, B, N, M), errs, measure=measure)
        failed[(ftag, gtag)] = errs
    return failed, measured


@pytest.mark.parametrize('ftag,gtag', lr.CASES, ids=['%s-%s' % c for c in lr.CASES])
def test_float32_oracle_passes_every_case(oracle32_runs, ftag, gtag):
    assert not oracle32_runs[0][(ftag, gtag)]


def test_coefficients_are_eight_times_the_measured_distances(oracle32_runs):
    """Each coefficient covers 8 x the float32 oracle's largest distance over ALL its cases and stays under the cap; the ordinary one is
    the derived value itself, to the three digits it is written with."""
    measured = oracle32_runs[1]
    assert len(lr.CASES) == len(set(lr.CASES))
    assert 8.0 * measured['ordinary'] <= lr.A_ORD <= 8.0 * measured['ordinary'] * 1.001 and lr.A_ORD <= lr.A_CAP, measured
    for group, a in lr.A_EXT.items():
        assert a == max(8.0 * lr.EXT_MEASURED[group], lr.A_ORD) and lr.EXT_MEASURED[group] >= measured[group] and a <= lr.A_CAP, (group, measured)


def test_every_family_meets_every_form():
    for ftag, _, _, _ in lr.FAMILIES:
        forms = {lr.GEO[g][1] for f, g in lr.CASES if f == ftag}
        assert forms == {'v1', 'v4', 'long'}, (ftag, forms)
        assert all((ftag, g) in lr.CASES for g in lr.EVERY_FAMILY)
    for tag, _, B, N, ld, Ms, _ in lr.GEOMS:
        assert ld == (N + 15) // 16 * 16 and all(1 <= M <= B for M in Ms)


@pytest.mark.parametrize('loss', ['cross-entropy', 'xe_logit', 'bpr', 'top1', 'bpr-max', 'top1-max'])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_row_losses_sum_to_the_cost(loss, dtype):
    M, n = 7, 30
    s = (np.random.RandomState(3).randn(M, n) * 2).astype(dtype)
    colmask = np.ones(n, dtype=bool)
    fa = parse_act('softmax' if loss == 'cross-entropy' else 'softmax_logit' if loss == 'xe_logit' else 'tanh')
    yhat = final_act_fwd(*fa, s, colmask).astype(dtype)
    for smoothing in ((0.0, 0.2) if loss in ('cross-entropy', 'xe_logit') else (0.0,)):
        total, d0 = loss_fwd_bwd(loss, yhat, M, np.arange(M), colmask, 0.5, smoothing)
        rows, d1 = loss_fwd_bwd(loss, yhat, M, np.arange(M), colmask, 0.5, smoothing, per_row=True)
        assert rows.shape == (M,) and rows.dtype == np.dtype(dtype) and np.array_equal(d0, d1)
        np.testing.assert_allclose(rows.sum(dtype=np.float64), float(total), rtol=4 * np.finfo(dtype).eps * M)

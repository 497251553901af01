"""The host code that launches a training step (g4r_host_step.hpp: step mode, window loop, step_head / step_tail) against records taken
before it was restructured (tests/golden/step_launches.json, written by tools/record_step_launches.py): per case of
step_launch_cases.CASES the kernel choice (`kernels` debug key), the launches per kernel slot of a profiled 37-step run and the bits
of an unprofiled one (SHA-256 over losses, Wy, acc_Wy and layer 0's Wx / Wh / Wrz) must be what they were.  The table as a whole has
to reach every kernel family the step dispatches on, read from the `kernels` key: a case that drifts off its path fails loudly."""
import json

import pytest

import step_launch_cases as slc

GOLDEN = json.load(open(slc.GOLDEN))
ML = slc.ML
# enumerators of GruFwdKind, GruBwdKind, ScoreFwdKind, ScoreBwdKind, UpdateKind (g4r_host_model.hpp)
N_FWD, N_BWD, N_SFWD, N_SBWD, N_UPDATE = 5, 5, 6, 5, 3


def test_the_golden_file_covers_the_case_table():
    assert sorted(GOLDEN) == sorted(slc.CASES)
    assert [n for n in slc.MANDATORY if GOLDEN[n]['digest'] is None] == []


def test_the_case_table_reaches_every_kernel_family():
    fwd, bwd, sf, sb, up, chunks, mom = set(), set(), set(), set(), set(), set(), set()
    for name, g in GOLDEN.items():
        k, L = g['kernels'], len(slc.CASES[name]['layers'])
        fwd |= set(k[:L])
        bwd |= set(k[ML:ML + L])
        sf.add(k[4 * ML])
        sb.add(k[4 * ML + 4])
        up.add(k[4 * ML + 8])
        chunks.add(k[4 * ML + 9])
        mom.add(slc.CASES[name].get('momentum', 0.0) > 0)
    assert fwd == set(range(N_FWD)) and bwd == set(range(N_BWD)), (fwd, bwd)
    assert sf == set(range(N_SFWD)) and sb == set(range(N_SBWD)), (sf, sb)
    assert up == set(range(N_UPDATE)) and chunks == {1, 2, 4} and mom == {False, True}, (up, chunks, mom)


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(slc.CASES))
def test_kernel_choice_launch_counts_and_bits_are_the_recorded_ones(name):
    want = GOLDEN[name]
    kernels, n_cu = slc.describe(name)
    if n_cu != want['n_cu']:
        pytest.skip('the goldens were recorded on a device of %d CUs, this one has %d' % (want['n_cu'], n_cu))
    assert kernels == want['kernels']
    got = slc.record(name)
    assert got['kernels'] == want['kernels']
    assert got.get('launches') == want.get('launches')
    assert got.get('launches_split') == want.get('launches_split')
    if want['digest'] is not None:
        assert got['digest'] == want['digest']

"""The beam-search tests must be able to FAIL: mutant 15 (gru4rec_amd/build.py MUTANTS, -DG4R_MUTATE=15 in g4r_beam_kernels.cuh) makes
k_beam_advance read the hidden state of beam row i itself instead of the row of its parent -- the classic beam-search bug: wherever
the selection re-parents, a beam carries on from the wrong state.  Chosen tests of test_gpu_beam_sessions.py whose reference
re-parents (they assert it) run in a child process with G4R_LIB pointing at it and have to come back red; the beams=1 tests stay
green on it (the only parent is the row itself), and on the product library all of them are green."""
import os
import subprocess
import sys

import pytest

from gru4rec_amd import build as g4r_build

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 'tests/test_gpu_beam_sessions.py::'
REPARENTING_TESTS = [T + 'test_lengths_beams_and_steps[softmax-3-5]', T + 'test_combine_modes_and_no_repeat[elu-sum-True]']
ONE_BEAM_TESTS = [T + 'test_lengths_beams_and_steps[softmax-1-5]', T + 'test_lengths_beams_and_steps[elu-1-5]',
                  T + 'test_one_beam_is_the_greedy_continuation[softmax]']


@pytest.fixture(scope='module')
def mutant15():
    path = g4r_build.mutant_path(15)
    if not os.path.exists(path) or any(os.path.getmtime(path) < os.path.getmtime(d) for d in g4r_build.DEPS):
        os.makedirs(os.path.dirname(path), exist_ok=True)
        g4r_build.build(out=path, defs=['G4R_MUTATE=15'])
    return path


def _run(sels, lib=None):
    env = dict(os.environ)
    if lib:
        env['G4R_LIB'] = lib
    return subprocess.run([sys.executable, '-m', 'pytest'] + list(sels) + ['-x', '-q', '-p', 'no:cacheprovider'], cwd=ROOT, env=env,
                          capture_output=True, text=True, timeout=900)


@pytest.mark.parametrize('sel', REPARENTING_TESTS)
def test_mutant_15_turns_the_reparenting_tests_red(mutant15, sel):
    r = _run([sel], mutant15)
    assert r.returncode == 1, 'mutant 15 passed %s:\n%s' % (sel, (r.stdout + r.stderr)[-3000:])
    assert 'AssertionError' in r.stdout + r.stderr


def test_mutant_15_passes_the_one_beam_tests(mutant15):
    r = _run(ONE_BEAM_TESTS, mutant15)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]


def test_product_library_passes_the_beam_tests():
    r = _run(REPARENTING_TESTS + ONE_BEAM_TESTS)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]

"""The sampling tests must be able to FAIL: mutant 20 (gru4rec_amd/build.py MUTANTS, -DG4R_MUTATE=20 in g4r_device.cuh) makes
gumbel_noise ignore the decoding step, so every step of a draw gets the noise of step 0.  The replay tests of
test_gpu_sample_sessions.py with steps >= 2 run in a child process with G4R_LIB pointing at it and have to come back red; their
steps = 1 cases and the noise test at step 0 stay green on it (step 0 is all they use), and on the product library all of them are
green."""
import os
import subprocess
import sys

import pytest

from gru4rec_amd import build as g4r_build

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 'tests/test_gpu_sample_sessions.py::'
LATER_STEPS = [T + 'test_exact_replay[2-1]', T + 'test_exact_replay[5-3]']
STEP_0 = [T + 'test_exact_replay[1-1]', T + 'test_exact_replay[1-3]', T + 'test_noise[0]']


@pytest.fixture(scope='module')
def mutant20():
    path = g4r_build.mutant_path(20)
    if not os.path.exists(path) or any(os.path.getmtime(path) < os.path.getmtime(d) for d in g4r_build.DEPS):
        os.makedirs(os.path.dirname(path), exist_ok=True)
        g4r_build.build(out=path, defs=['G4R_MUTATE=20'])
    return path


def _run(sels, lib=None):
    env = dict(os.environ)
    if lib:
        env['G4R_LIB'] = lib
    return subprocess.run([sys.executable, '-m', 'pytest'] + list(sels) + ['-x', '-q', '-p', 'no:cacheprovider'], cwd=ROOT, env=env,
                          capture_output=True, text=True, timeout=900)


@pytest.mark.parametrize('sel', LATER_STEPS)
def test_mutant_20_turns_the_later_steps_red(mutant20, sel):
    r = _run([sel], mutant20)
    assert r.returncode == 1, 'mutant 20 passed %s:\n%s' % (sel, (r.stdout + r.stderr)[-3000:])
    assert 'AssertionError' in r.stdout + r.stderr


def test_mutant_20_passes_what_uses_step_0_alone(mutant20):
    r = _run(STEP_0, mutant20)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]


def test_product_library_passes_the_sampling_tests():
    r = _run(LATER_STEPS + STEP_0)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]

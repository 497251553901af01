"""The continuation tests must be able to FAIL: mutant 14 (gru4rec_amd/build.py MUTANTS, -DG4R_MUTATE=14 in g4r_rollout_kernels.cuh)
makes k_rollout_feed's sorted insertion drop an item that sorts above every item already in its row's exclusion list, so that item is
never excluded and can be returned again.  Chosen no_repeat=True tests of test_gpu_continue_sessions.py (candidates that sort above
every history item: each row's first generated item is such an item) run in a child process with G4R_LIB pointing at it and have to
come back red; their no_repeat=False twins stay green on it (nothing is inserted), and on the product library all of them are green."""
import os
import subprocess
import sys

import pytest

from gru4rec_amd import build as g4r_build

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 'tests/test_gpu_continue_sessions.py::'
NO_REPEAT_TESTS = [T + 'test_no_repeat[True]', T + 'test_running_the_candidates_dry[True]']
REPEAT_TESTS = [T + 'test_no_repeat[False]', T + 'test_running_the_candidates_dry[False]', T + 'test_no_repeat_over_all_items[False]']


@pytest.fixture(scope='module')
def mutant14():
    path = g4r_build.mutant_path(14)
    if not os.path.exists(path) or any(os.path.getmtime(path) < os.path.getmtime(d) for d in g4r_build.DEPS):
        os.makedirs(os.path.dirname(path), exist_ok=True)
        g4r_build.build(out=path, defs=['G4R_MUTATE=14'])
    return path


def _run(sels, lib=None):
    env = dict(os.environ)
    if lib:
        env['G4R_LIB'] = lib
    return subprocess.run([sys.executable, '-m', 'pytest'] + list(sels) + ['-x', '-q', '-p', 'no:cacheprovider'], cwd=ROOT, env=env,
                          capture_output=True, text=True, timeout=900)


@pytest.mark.parametrize('sel', NO_REPEAT_TESTS)
def test_mutant_14_turns_the_no_repeat_tests_red(mutant14, sel):
    r = _run([sel], mutant14)
    assert r.returncode == 1, 'mutant 14 passed %s:\n%s' % (sel, (r.stdout + r.stderr)[-3000:])
    assert 'AssertionError' in r.stdout + r.stderr


def test_mutant_14_passes_the_tests_without_no_repeat(mutant14):
    r = _run(REPEAT_TESTS, mutant14)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]


def test_product_library_passes_the_continuation_tests():
    r = _run(NO_REPEAT_TESTS + REPEAT_TESTS)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]

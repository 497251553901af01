"""The replay tests must be able to FAIL: mutant 10 (gru4rec_amd/build.py MUTANTS, -DG4R_MUTATE=10 in g4r_topk_kernels.cuh) makes
k_replay_final read every row's final state from the ping-pong buffer of its chunk's LONGEST history.  Chosen ragged-length tests of
test_gpu_recommend_sessions.py run in a child process with G4R_LIB pointing at it and have to come back red; their equal-length
twins stay green on it (there every row's parity is the longest's), and on the product library all of them are green."""
import os
import subprocess
import sys

import pytest

from gru4rec_amd import build as g4r_build

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 'tests/test_gpu_recommend_sessions.py::'
RAGGED_TESTS = [T + 'test_hidden_continuation[ragged]', T + 'test_hidden_out_against_the_oracle[layers0-constrained-ragged]',
                T + 'test_hidden_out_against_the_oracle[layers1-onehot-ragged]']
EQUAL_TESTS = [T + 'test_hidden_continuation[equal]', T + 'test_hidden_out_against_the_oracle[layers0-constrained-equal]']


@pytest.fixture(scope='module')
def mutant10():
    path = g4r_build.mutant_path(10)
    if not os.path.exists(path) or any(os.path.getmtime(path) < os.path.getmtime(d) for d in g4r_build.DEPS):
        os.makedirs(os.path.dirname(path), exist_ok=True)
        g4r_build.build(out=path, defs=['G4R_MUTATE=10'])
    return path


def _run(sels, lib=None):
    env = dict(os.environ)
    if lib:
        env['G4R_LIB'] = lib
    return subprocess.run([sys.executable, '-m', 'pytest'] + list(sels) + ['-x', '-q', '-p', 'no:cacheprovider'], cwd=ROOT, env=env,
                          capture_output=True, text=True, timeout=900)


@pytest.mark.parametrize('sel', RAGGED_TESTS)
def test_mutant_10_turns_the_ragged_tests_red(mutant10, sel):
    r = _run([sel], mutant10)
    assert r.returncode == 1, 'mutant 10 passed %s:\n%s' % (sel, (r.stdout + r.stderr)[-3000:])
    assert 'AssertionError' in r.stdout + r.stderr


def test_mutant_10_passes_the_equal_length_tests(mutant10):
    r = _run(EQUAL_TESTS, mutant10)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]


def test_product_library_passes_the_replay_tests():
    r = _run(RAGGED_TESTS + EQUAL_TESTS)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]

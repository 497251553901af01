"""The scan tests must be able to FAIL: mutant 12 (gru4rec_amd/build.py MUTANTS, -DG4R_MUTATE=12 in g4r_host_topk.hpp) skips the
fp32 re-scoring of the two-stage top-k, so its second stage ranks -- and returns -- the approximate bf16 scores of the first.  The
tests that compare returned scores with predict_next_batch bit for bit, and the certified-equality test, run in a child process with
G4R_LIB pointing at it and have to come back red; the argument test, which launches nothing, stays green on it, and on the product
library all of them are green."""
import os
import subprocess
import sys

import pytest

from gru4rec_amd import build as g4r_build

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 'tests/test_gpu_recommend_scan.py::'
RED_TESTS = [T + 'test_exact_scores_and_contract_order[64-linear]', T + 'test_certified_rows_equal_the_exact_call[20000-64]',
             T + 'test_degenerate_equals_the_exact_call[fitted]']
GREEN_TESTS = [T + 'test_c_abi_refuses_bad_arguments']


@pytest.fixture(scope='module')
def mutant12():
    path = g4r_build.mutant_path(12)
    if not os.path.exists(path) or any(os.path.getmtime(path) < os.path.getmtime(d) for d in g4r_build.DEPS):
        os.makedirs(os.path.dirname(path), exist_ok=True)
        g4r_build.build(out=path, defs=['G4R_MUTATE=12'])
    return path


def _run(sels, lib=None):
    env = dict(os.environ)
    if lib:
        env['G4R_LIB'] = lib
    return subprocess.run([sys.executable, '-m', 'pytest'] + list(sels) + ['-x', '-q', '-p', 'no:cacheprovider'], cwd=ROOT, env=env,
                          capture_output=True, text=True, timeout=900)


@pytest.mark.parametrize('sel', RED_TESTS)
def test_mutant_12_turns_the_score_tests_red(mutant12, sel):
    r = _run([sel], mutant12)
    assert r.returncode == 1, 'mutant 12 passed %s:\n%s' % (sel, (r.stdout + r.stderr)[-3000:])
    assert 'AssertionError' in r.stdout + r.stderr


def test_mutant_12_passes_the_argument_test(mutant12):
    r = _run(GREEN_TESTS, mutant12)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]


def test_product_library_passes_the_scan_tests():
    r = _run(RED_TESTS + GREEN_TESTS)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]

"""The top-k tie tests must be able to FAIL: mutant 7 (gru4rec_amd/build.py MUTANTS, -DG4R_MUTATE=7 in g4r_topk_kernels.cuh) breaks
equal scores by the higher column instead of the lower one.  The tie tests of test_gpu_recommend.py run in a child process with
G4R_LIB pointing at it and have to come back red; on the product library the same selection is green."""
import os
import subprocess
import sys

import pytest

from gru4rec_amd import build as g4r_build

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIE_TESTS = ['tests/test_gpu_recommend.py::test_all_scores_equal_gives_the_first_columns[linear]',
             'tests/test_gpu_recommend.py::test_all_scores_equal_gives_the_first_columns[relu]',
             'tests/test_gpu_recommend.py::test_top_k_matches_predict_next_batch[64-relu]',
             'tests/test_gpu_recommend.py::test_top_k_matches_predict_next_batch[64-tanh]']


@pytest.fixture(scope='module')
def mutant7():
    path = g4r_build.mutant_path(7)
    if not os.path.exists(path) or any(os.path.getmtime(path) < os.path.getmtime(d) for d in g4r_build.DEPS):
        os.makedirs(os.path.dirname(path), exist_ok=True)
        g4r_build.build(out=path, defs=['G4R_MUTATE=7'])
    return path


def _run(sels, lib=None):
    env = dict(os.environ)
    if lib:
        env['G4R_LIB'] = lib
    return subprocess.run([sys.executable, '-m', 'pytest'] + list(sels) + ['-x', '-q', '-p', 'no:cacheprovider'], cwd=ROOT, env=env,
                          capture_output=True, text=True, timeout=900)


@pytest.mark.parametrize('sel', TIE_TESTS)
def test_mutant_7_turns_the_tie_tests_red(mutant7, sel):
    r = _run([sel], mutant7)
    assert r.returncode == 1, 'mutant 7 passed %s:\n%s' % (sel, (r.stdout + r.stderr)[-3000:])
    assert 'AssertionError' in r.stdout + r.stderr


def test_product_library_passes_the_tie_tests():
    r = _run(TIE_TESTS)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]

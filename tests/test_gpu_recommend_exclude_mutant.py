"""The exclusion tests must be able to FAIL: mutant 9 (gru4rec_amd/build.py MUTANTS, -DG4R_MUTATE=9 in g4r_topk_kernels.cuh) makes the
merge-time search of a row's sorted exclusion list miss its last item.  Chosen tests of test_gpu_recommend_exclude.py run in a child
process with G4R_LIB pointing at it and have to come back red; on the product library the same selection is green."""
import os
import subprocess
import sys

import pytest

from gru4rec_amd import build as g4r_build

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXCL_TESTS = ['tests/test_gpu_recommend_exclude.py::test_excluding_the_own_top_k_gives_the_next_k[linear]',
              'tests/test_gpu_recommend_exclude.py::test_excluding_the_own_top_k_gives_the_next_k[softmax]',
              'tests/test_gpu_recommend_exclude.py::test_excluding_the_own_top_k_gives_the_next_k[relu]']


@pytest.fixture(scope='module')
def mutant9():
    path = g4r_build.mutant_path(9)
    if not os.path.exists(path) or any(os.path.getmtime(path) < os.path.getmtime(d) for d in g4r_build.DEPS):
        os.makedirs(os.path.dirname(path), exist_ok=True)
        g4r_build.build(out=path, defs=['G4R_MUTATE=9'])
    return path


def _run(sels, lib=None):
    env = dict(os.environ)
    if lib:
        env['G4R_LIB'] = lib
    return subprocess.run([sys.executable, '-m', 'pytest'] + list(sels) + ['-x', '-q', '-p', 'no:cacheprovider'], cwd=ROOT, env=env,
                          capture_output=True, text=True, timeout=900)


@pytest.mark.parametrize('sel', EXCL_TESTS)
def test_mutant_9_turns_the_exclusion_tests_red(mutant9, sel):
    r = _run([sel], mutant9)
    assert r.returncode == 1, 'mutant 9 passed %s:\n%s' % (sel, (r.stdout + r.stderr)[-3000:])
    assert 'AssertionError' in r.stdout + r.stderr


def test_product_library_passes_the_exclusion_tests():
    r = _run(EXCL_TESTS)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]

"""The item-index tests must be able to FAIL: mutant 31 (gru4rec_amd/build.py MUTANTS, -DG4R_MUTATE=31 in g4r_ivf_kernels.cuh) makes
k_ivf_scan leave out the last block of every list whose length is not a multiple of 32, so the items of that block never become
candidates.  The hand-made-partition test (lists of 1, 31, 33, 65 and 2,500 items) and the nprobe = n_lists test run in a child process
with G4R_LIB pointing at it and have to come back red; the argument test, which scans nothing, stays green on it, and on the product
library all of them are green."""
import os
import subprocess
import sys

import pytest

from gru4rec_amd import build as g4r_build

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 'tests/test_gpu_item_index.py::'
RED_TESTS = [T + 'test_hand_made_partition', T + 'test_all_lists_probed_equals_the_bf16_scan[small]']
GREEN_TESTS = ['tests/test_item_index_args.py', T + 'test_c_abi_refuses_bad_arguments']


@pytest.fixture(scope='module')
def mutant31():
    path = g4r_build.mutant_path(31)
    if not os.path.exists(path) or any(os.path.getmtime(path) < os.path.getmtime(d) for d in g4r_build.DEPS):
        os.makedirs(os.path.dirname(path), exist_ok=True)
        g4r_build.build(out=path, defs=['G4R_MUTATE=31'])
    return path


def _run(sels, lib=None):
    env = dict(os.environ)
    if lib:
        env['G4R_LIB'] = lib
    return subprocess.run([sys.executable, '-m', 'pytest'] + list(sels) + ['-x', '-q', '-p', 'no:cacheprovider'], cwd=ROOT, env=env,
                          capture_output=True, text=True, timeout=900)


@pytest.mark.parametrize('sel', RED_TESTS)
def test_mutant_31_turns_the_scan_tests_red(mutant31, sel):
    r = _run([sel], mutant31)
    assert r.returncode == 1, 'mutant 31 passed %s:\n%s' % (sel, (r.stdout + r.stderr)[-3000:])
    assert 'AssertionError' in r.stdout + r.stderr


def test_mutant_31_passes_the_argument_test(mutant31):
    r = _run(GREEN_TESTS, mutant31)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]


def test_product_library_passes_the_scan_tests():
    r = _run(RED_TESTS + GREEN_TESTS)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]

"""The diversify tests must be able to FAIL: mutant 24 (gru4rec_amd/build.py MUTANTS, -DG4R_MUTATE=24 in g4r_mmr_kernels.cuh) overwrites a
position's largest similarity to the picks by its similarity to the LAST pick from the second update on, instead of taking the maximum.
The first two picks, and every pick with trade_off = 1 (the similarity term is multiplied by 0), are the product's, so those tests and
the argument tests stay green on it; from the third pick on an item close to an early pick comes back too soon, and the parity and fp64
tests with k >= 3 and trade_off < 1 run in a child process with G4R_LIB pointing at it and have to come back red.  On the product
library all of them are green."""
import os
import subprocess
import sys

import pytest

from gru4rec_amd import build as g4r_build

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 'tests/test_gpu_diversify.py::'
RED_TESTS = [T + 'test_parity_with_the_host_loop[3000x100-k10-P]', T + 'test_parity_with_the_host_loop[300x160-k10-P]',
             T + 'test_picks_against_fp64[300x36-k10-P]', T + 'test_parity_across_chunks_filters_and_scan[k10-P]']
GREEN_TESTS = [T + 'test_trade_off_one_is_recommend_sessions', T + 'test_parity_with_the_host_loop[3000x100-k1-2]',
               T + 'test_picks_against_fp64[300x36-k1-2]', T + 'test_parity_across_chunks_filters_and_scan[k1-2]', 'tests/test_diversify_args.py']


@pytest.fixture(scope='module')
def mutant24():
    path = g4r_build.mutant_path(24)
    if not os.path.exists(path) or any(os.path.getmtime(path) < os.path.getmtime(d) for d in g4r_build.DEPS):
        os.makedirs(os.path.dirname(path), exist_ok=True)
        g4r_build.build(out=path, defs=['G4R_MUTATE=24'])
    return path


def _run(sels, lib=None):
    env = dict(os.environ)
    if lib:
        env['G4R_LIB'] = lib
    return subprocess.run([sys.executable, '-m', 'pytest'] + list(sels) + ['-x', '-q', '-p', 'no:cacheprovider'], cwd=ROOT, env=env,
                          capture_output=True, text=True, timeout=900)


@pytest.mark.parametrize('sel', RED_TESTS)
def test_mutant_24_turns_the_later_picks_red(mutant24, sel):
    r = _run([sel], mutant24)
    assert r.returncode == 1, 'mutant 24 passed %s:\n%s' % (sel, (r.stdout + r.stderr)[-3000:])
    assert 'AssertionError' in r.stdout + r.stderr


def test_mutant_24_passes_the_first_two_picks_and_the_argument_tests(mutant24):
    r = _run(GREEN_TESTS, mutant24)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]


def test_product_library_passes_the_diversify_tests():
    r = _run(RED_TESTS + GREEN_TESTS)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]

"""The neighbour tests must be able to FAIL: mutant 13 (gru4rec_amd/build.py MUTANTS, -DG4R_MUTATE=13 in g4r_sim_kernels.cuh) reads the
candidate's inverse norm at the candidate's POSITION instead of at its item index.  Over the whole catalogue the two coincide, so those
tests and the argument tests stay green on it; with a candidate list every cosine score is scaled by another item's norm, and the tests
that pass predict_for_item_ids run in a child process with G4R_LIB pointing at it and have to come back red.  On the product library
all of them are green."""
import os
import subprocess
import sys

import pytest

from gru4rec_amd import build as g4r_build

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 'tests/test_gpu_similar_items.py::'
RED_TESTS = [T + 'test_scores_and_selection_against_fp64[50-30-onehot]', T + 'test_scores_and_selection_against_fp64[3000-256-constrained]',
             T + 'test_exact_ties_and_zero_rows']
GREEN_TESTS = [T + 'test_norm_cache_follows_the_weights', T + 'test_catalogue_of_one_item', 'tests/test_similar_items_args.py']


@pytest.fixture(scope='module')
def mutant13():
    path = g4r_build.mutant_path(13)
    if not os.path.exists(path) or any(os.path.getmtime(path) < os.path.getmtime(d) for d in g4r_build.DEPS):
        os.makedirs(os.path.dirname(path), exist_ok=True)
        g4r_build.build(out=path, defs=['G4R_MUTATE=13'])
    return path


def _run(sels, lib=None):
    env = dict(os.environ)
    if lib:
        env['G4R_LIB'] = lib
    return subprocess.run([sys.executable, '-m', 'pytest'] + list(sels) + ['-x', '-q', '-p', 'no:cacheprovider'], cwd=ROOT, env=env,
                          capture_output=True, text=True, timeout=900)


@pytest.mark.parametrize('sel', RED_TESTS)
def test_mutant_13_turns_the_candidate_list_tests_red(mutant13, sel):
    r = _run([sel], mutant13)
    assert r.returncode == 1, 'mutant 13 passed %s:\n%s' % (sel, (r.stdout + r.stderr)[-3000:])
    assert 'AssertionError' in r.stdout + r.stderr


def test_mutant_13_passes_the_whole_catalogue_and_argument_tests(mutant13):
    r = _run(GREEN_TESTS, mutant13)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]


def test_product_library_passes_the_neighbour_tests():
    r = _run(RED_TESTS + GREEN_TESTS)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]

"""The candidate tests must be able to FAIL: mutant 11 (gru4rec_amd/build.py MUTANTS, -DG4R_MUTATE=11 in g4r_cand_kernels.cuh)
makes every work item of k_score_cand past a row's first slice (CS_SLICE = 256 positions) score the items of the row's first
slice instead of its own.  Chosen tests of test_gpu_candidates.py whose rows are longer than one slice run in a child process with
G4R_LIB pointing at it and have to come back red; twins whose rows all fit in one slice stay green on it, and on the product
library all of them are green."""
import os
import subprocess
import sys

import pytest

from gru4rec_amd import build as g4r_build

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 'tests/test_gpu_candidates.py::'
LONG_TESTS = [T + 'test_ragged_elementwise_and_interleaving[linear]', T + 'test_softmax_normalises_over_the_rows_own_list[softmax]',
              T + 'test_topk_equals_recommend_next_batch[linear-20]', T + 'test_against_the_oracle[tanh]']
SHORT_TESTS = [T + 'test_elementwise_scores_equal_the_full_catalogue[linear-layers0-constrained]',
               T + 'test_sessions_hidden_continuation_and_return_hidden']


@pytest.fixture(scope='module')
def mutant11():
    path = g4r_build.mutant_path(11)
    if not os.path.exists(path) or any(os.path.getmtime(path) < os.path.getmtime(d) for d in g4r_build.DEPS):
        os.makedirs(os.path.dirname(path), exist_ok=True)
        g4r_build.build(out=path, defs=['G4R_MUTATE=11'])
    return path


def _run(sels, lib=None):
    env = dict(os.environ)
    if lib:
        env['G4R_LIB'] = lib
    return subprocess.run([sys.executable, '-m', 'pytest'] + list(sels) + ['-x', '-q', '-p', 'no:cacheprovider'], cwd=ROOT, env=env,
                          capture_output=True, text=True, timeout=900)


@pytest.mark.parametrize('sel', LONG_TESTS)
def test_mutant_11_turns_the_long_row_tests_red(mutant11, sel):
    r = _run([sel], mutant11)
    assert r.returncode == 1, 'mutant 11 passed %s:\n%s' % (sel, (r.stdout + r.stderr)[-3000:])
    assert 'AssertionError' in r.stdout + r.stderr


def test_mutant_11_passes_the_one_slice_tests(mutant11):
    r = _run(SHORT_TESTS, mutant11)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]


def test_product_library_passes_the_candidate_tests():
    r = _run(LONG_TESTS + SHORT_TESTS)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]

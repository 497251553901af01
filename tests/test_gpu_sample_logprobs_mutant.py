"""The row-normaliser tests must be able to FAIL: mutant 25 (gru4rec_amd/build.py MUTANTS, -DG4R_MUTATE=25 in g4r_topk_kernels.cuh) never
marks the LAST item of a row's sorted list as ineligible, so that item's term is counted in Q.  The exact-Q tests of
test_gpu_sample_logprobs.py whose rows have lists run in a child process with G4R_LIB pointing at it and have to come back red; the
case without exclusions and the terms test stay green on it (no list is read), and on the product library all of them are green."""
import os
import subprocess
import sys

import pytest

from gru4rec_amd import build as g4r_build

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 'tests/test_gpu_sample_logprobs.py::'
WITH_LISTS = [T + 'test_q_with_the_history_excluded', T + 'test_q_with_a_mask_and_lists', T + 'test_q_with_lists_at_the_edges_of_the_catalogue']
WITHOUT = [T + 'test_q_without_exclusions', T + 'test_terms']


@pytest.fixture(scope='module')
def mutant25():
    path = g4r_build.mutant_path(25)
    if not os.path.exists(path) or any(os.path.getmtime(path) < os.path.getmtime(d) for d in g4r_build.DEPS):
        os.makedirs(os.path.dirname(path), exist_ok=True)
        g4r_build.build(out=path, defs=['G4R_MUTATE=25'])
    return path


def _run(sels, lib=None):
    env = dict(os.environ)
    if lib:
        env['G4R_LIB'] = lib
    return subprocess.run([sys.executable, '-m', 'pytest'] + list(sels) + ['-x', '-q', '-p', 'no:cacheprovider'], cwd=ROOT, env=env,
                          capture_output=True, text=True, timeout=900)


@pytest.mark.parametrize('sel', WITH_LISTS)
def test_mutant_25_turns_the_rows_with_lists_red(mutant25, sel):
    r = _run([sel], mutant25)
    assert r.returncode == 1, 'mutant 25 passed %s:\n%s' % (sel, (r.stdout + r.stderr)[-3000:])
    assert 'AssertionError' in r.stdout + r.stderr and 'the eligible terms sum to' in r.stdout + r.stderr


def test_mutant_25_passes_what_reads_no_list(mutant25):
    r = _run(WITHOUT, mutant25)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]


def test_product_library_passes_the_normaliser_tests():
    r = _run(WITH_LISTS + WITHOUT)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]

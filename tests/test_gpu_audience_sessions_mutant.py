"""The audience tests must be able to FAIL: mutant 28 (gru4rec_amd/build.py MUTANTS, -DG4R_MUTATE=28 in g4r_audience_kernels.cuh) files a
session under its index within its chunk -- the chunk's first session is not added.  Calls of one chunk (at most 512 sessions, no
G4R_SESSIONS_CHUNK) have a first session of 0 and stay correct, so those tests and the argument tests stay green on it; from the second
chunk on the lists name sessions of the first chunk, and the multi-chunk parity tests run in a child process with G4R_LIB pointing at
it and have to come back red.  On the product library all of them are green."""
import os
import subprocess
import sys

import pytest

from gru4rec_amd import build as g4r_build

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 'tests/test_gpu_audience_sessions.py::'
RED_TESTS = [T + 'test_scores_equal_the_host_loop[linear-layers0-600-None]', T + 'test_scores_equal_the_host_loop[relu-layers4-600-16]',
             T + 'test_logprobs_against_the_log_likelihood_twin[linear-layers0-600-5-1.0-True]',
             T + 'test_the_result_does_not_depend_on_the_chunking[linear-layers0-score-False]',
             T + 'test_splitting_the_sessions_over_two_calls[softmax-layers3-logprob]']
GREEN_TESTS = [T + 'test_scores_equal_the_host_loop[linear-layers0-1-None]', T + 'test_scores_equal_the_host_loop[linear-layers0-37-None]',
               T + 'test_logprobs_against_the_log_likelihood_twin[linear-layers0-37-70-0.7-True]', T + 'test_hidden_continues_a_session',
               T + 'test_the_c_entry_refuses_before_any_launch_and_the_next_call_is_correct', 'tests/test_audience_sessions_args.py']


@pytest.fixture(scope='module')
def mutant28():
    path = g4r_build.mutant_path(28)
    if not os.path.exists(path) or any(os.path.getmtime(path) < os.path.getmtime(d) for d in g4r_build.DEPS):
        os.makedirs(os.path.dirname(path), exist_ok=True)
        g4r_build.build(out=path, defs=['G4R_MUTATE=28'])
    return path


def _run(sels, lib=None):
    env = dict(os.environ)
    env.pop('G4R_SESSIONS_CHUNK', None)
    if lib:
        env['G4R_LIB'] = lib
    return subprocess.run([sys.executable, '-m', 'pytest'] + list(sels) + ['-x', '-q', '-p', 'no:cacheprovider'], cwd=ROOT, env=env,
                          capture_output=True, text=True, timeout=900)


@pytest.mark.parametrize('sel', RED_TESTS)
def test_mutant_28_turns_the_multi_chunk_calls_red(mutant28, sel):
    r = _run([sel], mutant28)
    assert r.returncode == 1, 'mutant 28 passed %s:\n%s' % (sel, (r.stdout + r.stderr)[-3000:])
    assert 'AssertionError' in r.stdout + r.stderr


def test_mutant_28_passes_the_one_chunk_calls_and_the_argument_tests(mutant28):
    r = _run(GREEN_TESTS, mutant28)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]


def test_product_library_passes_the_audience_tests():
    r = _run(RED_TESTS + GREEN_TESTS)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]

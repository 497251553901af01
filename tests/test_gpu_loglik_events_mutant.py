"""The log-likelihood tests must be able to FAIL: mutant 27 (gru4rec_amd/build.py MUTANTS, -DG4R_MUTATE=27 in g4r_topk_kernels.cuh) takes a
session item as seen only when its first occurrence is BEFORE the input event, so the input event's own item, first shown there, stays
in the row normaliser Q.  The exclude_seen tests of test_gpu_loglik_events.py run in a child process with G4R_LIB pointing at it and
have to come back red; the prefix-loop test without exclusions stays green on it (no session list is read), and on the product library
all of them are green."""
import os
import subprocess
import sys

import pytest

from gru4rec_amd import build as g4r_build

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 'tests/test_gpu_loglik_events.py::'
WITH_SEEN = [T + 'test_exclusions', T + 'test_agrees_with_sample_sessions']
WITHOUT = [T + 'test_equals_the_prefix_loop', '-k', 'constrained and 0.5']


@pytest.fixture(scope='module')
def mutant27():
    path = g4r_build.mutant_path(27)
    if not os.path.exists(path) or any(os.path.getmtime(path) < os.path.getmtime(d) for d in g4r_build.DEPS):
        os.makedirs(os.path.dirname(path), exist_ok=True)
        g4r_build.build(out=path, defs=['G4R_MUTATE=27'])
    return path


def _run(sels, lib=None):
    env = dict(os.environ)
    if lib:
        env['G4R_LIB'] = lib
    return subprocess.run([sys.executable, '-m', 'pytest'] + list(sels) + ['-x', '-q', '-p', 'no:cacheprovider'], cwd=ROOT, env=env,
                          capture_output=True, text=True, timeout=900)


@pytest.mark.parametrize('sel', WITH_SEEN)
def test_mutant_27_turns_the_seen_exclusions_red(mutant27, sel):
    r = _run([sel], mutant27)
    assert r.returncode == 1, 'mutant 27 passed %s:\n%s' % (sel, (r.stdout + r.stderr)[-3000:])
    assert 'AssertionError' in r.stdout + r.stderr


def test_mutant_27_passes_what_reads_no_session_list(mutant27):
    r = _run(WITHOUT, mutant27)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]


def test_product_library_passes_them():
    r = _run(WITH_SEEN + WITHOUT)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]

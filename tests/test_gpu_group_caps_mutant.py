"""The group-cap tests must be able to FAIL: mutant 26 (gru4rec_amd/build.py MUTANTS, -DG4R_MUTATE=26 in g4r_group_kernels.cuh) counts a
position's earlier same-group positions from the start of its own wave only, so the positions of earlier waves are forgotten.  Lists
of at most 64 positions lie in one wave and stay correct, so those tests and the argument tests stay green on it; a longer list keeps
positions whose group was already full in an earlier wave, and the parity tests with more than 64 positions run in a child process
with G4R_LIB pointing at it and have to come back red.  On the product library all of them are green."""
import os
import subprocess
import sys

import pytest

from gru4rec_amd import build as g4r_build

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 'tests/test_gpu_group_caps.py::'
RED_TESTS = [T + 'test_capped_lists_equal_the_host_loop[P65]', T + 'test_capped_lists_equal_the_host_loop[P128]',
             T + 'test_capped_lists_equal_the_host_loop[P256]', T + 'test_cap_lists_equal_the_rule[P128]',
             T + 'test_continuation_equals_the_host_loop[s2-P80]']
GREEN_TESTS = [T + 'test_capped_lists_equal_the_host_loop[P1]', T + 'test_capped_lists_equal_the_host_loop[P63]',
               T + 'test_capped_lists_equal_the_host_loop[P64]', T + 'test_cap_lists_equal_the_rule[P64]',
               T + 'test_continuation_equals_the_host_loop[s2-P16]', T + 'test_c_entries_refuse_before_any_launch', 'tests/test_group_caps_args.py']


@pytest.fixture(scope='module')
def mutant26():
    path = g4r_build.mutant_path(26)
    if not os.path.exists(path) or any(os.path.getmtime(path) < os.path.getmtime(d) for d in g4r_build.DEPS):
        os.makedirs(os.path.dirname(path), exist_ok=True)
        g4r_build.build(out=path, defs=['G4R_MUTATE=26'])
    return path


def _run(sels, lib=None):
    env = dict(os.environ)
    if lib:
        env['G4R_LIB'] = lib
    return subprocess.run([sys.executable, '-m', 'pytest'] + list(sels) + ['-x', '-q', '-p', 'no:cacheprovider'], cwd=ROOT, env=env,
                          capture_output=True, text=True, timeout=900)


@pytest.mark.parametrize('sel', RED_TESTS)
def test_mutant_26_turns_the_long_lists_red(mutant26, sel):
    r = _run([sel], mutant26)
    assert r.returncode == 1, 'mutant 26 passed %s:\n%s' % (sel, (r.stdout + r.stderr)[-3000:])
    assert 'AssertionError' in r.stdout + r.stderr


def test_mutant_26_passes_the_one_wave_lists_and_the_argument_tests(mutant26):
    r = _run(GREEN_TESTS, mutant26)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]


def test_product_library_passes_the_group_cap_tests():
    r = _run(RED_TESTS + GREEN_TESTS)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]

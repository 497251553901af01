"""The checks of the per-position entries must be able to FAIL: mutant 32 (gru4rec_amd/build.py MUTANTS, -DG4R_MUTATE=32 in
g4r_update_kernels.cuh) lets k_owner_window count a repeated item whose occurrences are all sampled negatives one too low -- items the
owner tables never look at.  The every-slot check of the entry ring and the bit comparison with the in-step form
(tests/test_gpu_pos_entries.py) run in a child process with G4R_LIB pointing at it and have to come back red; on the product library
the same selections are green."""
import os
import subprocess
import sys

import pytest

from gru4rec_amd import build as g4r_build

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLOT_TEST = 'tests/test_gpu_pos_entries.py::test_every_slot_of_the_ring_holds_its_steps_entries[cfg2_shape]'
BITS_TEST = 'tests/test_gpu_pos_entries.py::test_entries_by_position_bit_identical_to_the_entries_built_in_the_step[cfg2_shape_refill_at_12-1]'


@pytest.fixture(scope='module')
def mutant32():
    path = g4r_build.mutant_path(32)
    if not os.path.exists(path) or any(os.path.getmtime(path) < os.path.getmtime(d) for d in g4r_build.DEPS):
        os.makedirs(os.path.dirname(path), exist_ok=True)
        g4r_build.build(out=path, defs=['G4R_MUTATE=32'])
    return path


def _run(sels, lib=None):
    env = dict(os.environ)
    if lib:
        env['G4R_LIB'] = lib
    return subprocess.run([sys.executable, '-m', 'pytest'] + list(sels) + ['-x', '-q', '-p', 'no:cacheprovider'], cwd=ROOT, env=env,
                          capture_output=True, text=True, timeout=900)


@pytest.mark.parametrize('sel', [SLOT_TEST, BITS_TEST])
def test_mutant_32_turns_the_check_red(mutant32, sel):
    r = _run([sel], mutant32)
    assert r.returncode == 1, 'mutant 32 passed %s:\n%s' % (sel, (r.stdout + r.stderr)[-3000:])
    assert 'AssertionError' in r.stdout + r.stderr


def test_product_library_passes_both_checks():
    r = _run([SLOT_TEST, BITS_TEST])
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]

"""The every-slot check of the owner ring must be able to FAIL: mutant 21 (gru4rec_amd/build.py MUTANTS, -DG4R_MUTATE=21 in
g4r_update_kernels.cuh) lets k_owner_window take the sample-store row of every step of its window from the window's first global step.
tests/test_gpu_owner_window.py::test_every_slot_of_the_ring_holds_its_steps_owner_rows runs in a child process with G4R_LIB pointing
at it and has to come back red; on the product library the same selection is green."""
import os
import subprocess
import sys

import pytest

from gru4rec_amd import build as g4r_build

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLOT_TEST = 'tests/test_gpu_owner_window.py::test_every_slot_of_the_ring_holds_its_steps_owner_rows'


@pytest.fixture(scope='module')
def mutant21():
    path = g4r_build.mutant_path(21)
    if not os.path.exists(path) or any(os.path.getmtime(path) < os.path.getmtime(d) for d in g4r_build.DEPS):
        os.makedirs(os.path.dirname(path), exist_ok=True)
        g4r_build.build(out=path, defs=['G4R_MUTATE=21'])
    return path


def _run(sels, lib=None):
    env = dict(os.environ)
    if lib:
        env['G4R_LIB'] = lib
    return subprocess.run([sys.executable, '-m', 'pytest'] + list(sels) + ['-x', '-q', '-p', 'no:cacheprovider'], cwd=ROOT, env=env,
                          capture_output=True, text=True, timeout=900)


def test_mutant_21_turns_the_every_slot_check_red(mutant21):
    r = _run([SLOT_TEST], mutant21)
    assert r.returncode == 1, 'mutant 21 passed %s:\n%s' % (SLOT_TEST, (r.stdout + r.stderr)[-3000:])
    assert 'AssertionError' in r.stdout + r.stderr


def test_product_library_passes_the_every_slot_check():
    r = _run([SLOT_TEST])
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]

"""The session-store tests must be able to FAIL: mutant 33 (gru4rec_amd/build.py MUTANTS, -DG4R_MUTATE=33 in g4r_store_kernels.cuh) makes
k_store_save read every row's final state from the ping-pong half the chunk's LONGEST row selects.  The tests below push calls whose
rows mix odd and even event counts and then read the stored states back (export, a later push, recommend): in a child process with
G4R_LIB pointing at the mutant they have to come back red; their twins, in which every row of a call has the same count, stay green on
it, and on the product library all of them are green."""
import os
import subprocess
import sys

import numpy as np
import pytest

from gru4rec_amd import build as g4r_build

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 'tests/test_gpu_session_store_mutant.py::'
MIXED_TESTS = [T + 'test_stored_state_after_counts[mixed]', T + 'test_next_push_continues_after_counts[mixed]']
EQUAL_TESTS = [T + 'test_stored_state_after_counts[equal]', T + 'test_next_push_continues_after_counts[equal]']
COUNTS = {'mixed': [1, 2, 3, 2, 4, 1, 5], 'equal': [3, 3, 3, 3, 3, 3, 3]}


def _store(counts):
    from test_gpu_session_store import fitted
    g = fitted()
    ids = g.itemidmap.index.values
    rng = np.random.RandomState(33)
    hists = [ids[rng.randint(0, len(ids), size=n)] for n in counts]
    st = g.open_session_store(16)
    st.push(np.repeat(np.arange(len(counts)), counts), np.concatenate(hists))
    return g, st, hists


@pytest.mark.parametrize('counts', list(COUNTS))
def test_stored_state_after_counts(counts):
    from test_gpu_session_store import assert_bits
    g, st, hists = _store(COUNTS[counts])
    try:
        want = g.recommend_sessions(hists, k=10, return_hidden=True)
        for h, w in zip(st.export(list(range(len(hists))))['hidden'], want[2]):
            assert_bits(h, w)
        got = st.recommend(list(range(len(hists))), k=10)
        np.testing.assert_array_equal(got[0], want[0])
        assert_bits(got[1], want[1])
    finally:
        st.close()


@pytest.mark.parametrize('counts', list(COUNTS))
def test_next_push_continues_after_counts(counts):
    from test_gpu_session_store import assert_bits
    g, st, hists = _store(COUNTS[counts])
    try:
        nxt = g.itemidmap.index.values[40:40 + len(hists)]
        rows, items, scores, _ = st.push(list(range(len(hists))), nxt, k=10)
        want = g.recommend_sessions([np.append(h, x) for h, x in zip(hists, nxt)], k=10)
        np.testing.assert_array_equal(items, want[0])
        assert_bits(scores, want[1])
    finally:
        st.close()


@pytest.fixture(scope='module')
def mutant33():
    path = g4r_build.mutant_path(33)
    if not os.path.exists(path) or any(os.path.getmtime(path) < os.path.getmtime(d) for d in g4r_build.DEPS):
        os.makedirs(os.path.dirname(path), exist_ok=True)
        g4r_build.build(out=path, defs=['G4R_MUTATE=33'])
    return path


def _run(sels, lib=None):
    env = dict(os.environ)
    if lib:
        env['G4R_LIB'] = lib
    return subprocess.run([sys.executable, '-m', 'pytest'] + list(sels) + ['-x', '-q', '-p', 'no:cacheprovider'], cwd=ROOT, env=env,
                          capture_output=True, text=True, timeout=900)


@pytest.mark.parametrize('sel', MIXED_TESTS)
def test_mutant_33_turns_the_mixed_count_tests_red(mutant33, sel):
    r = _run([sel], mutant33)
    assert r.returncode == 1, 'mutant 33 passed %s:\n%s' % (sel, (r.stdout + r.stderr)[-3000:])
    assert 'AssertionError' in r.stdout + r.stderr


def test_mutant_33_passes_the_equal_count_twins(mutant33):
    r = _run(EQUAL_TESTS, mutant33)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]


def test_product_library_passes_the_count_tests():
    r = _run(MIXED_TESTS + EQUAL_TESTS)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]

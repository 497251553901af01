"""The parity suite must be able to FAIL.  Three deliberately wrong builds of the library (gru4rec_amd/build.py: build_mutants,
-DG4R_MUTATE=k in g4r_device.cuh) are run through a handful of the parity tests in a child process with G4R_LIB pointing at the
mutant; every one of those runs has to come back red, and the tensor it names has to be the one the mutation damages:

  mutant 1  every per-occurrence sparse accumulator increment x 1.01   -> acc_Wy / acc_By (1 % of an accumulator of ~1e-7)
  mutant 2  every sparse Adagrad step x 1.01                             -> dWy / dBy (1 % of a step)
  mutant 3  every dense accumulator increment x 1.01                     -> acc_Wx / acc_Wh / ...
  mutant 5  the 1 / nranks factor of the exact-replica joint update x 1.01 -> the REDUCE / MEAN oracle-as-replicas tests
  mutant 6  the Adagrad step of ONE item row per step x 1.5 (the item of score column 0) -> dWy: a single wrong row must fail, also in
            the exact-shape tests that compare the rows of kink items apart (round 5 left those rows out; now they are bounded)
  mutant 8  k_update_l's owner scan skips the last id of every 1024-id slice after the first -> dWy of the hot-item case of
            test_gpu_lean_edges.py (an item with > 1024 earlier occurrences in a step loses one of them)
  mutant 16 k_sparse_update_generic's owner walk drops the first hit of every pass after the first -> dWy of the hot rows of
            test_gpu_generic_edges.py::test_hot_items (an item with > 64 earlier occurrences loses one per later pass)
  mutant 17 opt_rule's new second statistic x 1.01 -> acc2_* of an adadelta and of an adam case; rmsprop (no such statistic) passes
  mutant 18 k_loss_rows' grp_fast takes the quad whose last column is the first inactive one as wholly active -> ds of the M = 35 run
            of a four-column case of test_gpu_loss_rows.py; the M = 36 run of the same case passes
  mutant 19 k_loss_rows' first pass starts its loop past the prefetched groups one STEP late -> ds at N = 12301; N = 4099 (no such
            trip) passes
  mutant 22 hidden_act_bwd decides the branch of leaky / elu / selu on the VALUE of the stored candidate c, not on its sign bit -> dV (da)
            of the sign-bit cases of test_gpu_hidden_act.py for elu and selu, lean (k_gru_da) and wide (k_gru_bwd_pre); leaky (p0 * a is
            not zero) and the one-step cases of every activation pass
  mutant 23 hidden_act_bwd's negative-branch slope of leaky / elu / selu x 1.01 -> dV0 (da) and dWx0 of their one-step cases, lean and
            wide; the tanh and relu rows pass
  mutant 29 finish_rows leaves out the sixteenth K-slice plane of layer 0's dy -> dWy / acc_Wy (the input rows' update) of the 16-slice case
            of test_gpu_wide_edges.py; the 12-slice case passes
  mutant 30 k_gru_p1s keys its embedding-dropout mask by the k offset inside the K slice -> the two-input-slice case (embedding 144) of
            test_gpu_wide_edges.py; the one-slice case (embedding 80, slice start 0) passes
  mutant 34 k_score_all leaves out By in the row tiles past the first 128 rows -> the 129-, 130- and 257-row cases of
            test_gpu_predict_edges.py; its 37- and 128-row cases and test_predict_and_ranks (40 rows) pass
  mutant 35 k_gru_p1 at prediction takes the third K chunk onward as zeros -> the cases of test_gpu_predict_edges.py with K = IN + D > 512;
            its K = 400 and K = 340 cases and test_gpu_hidden_act.py::test_predict_step (K <= 512) pass

(Round 2's `atol = 1e-4` on every tensor let an accumulator that is wrong by 100 x pass.)  The same selection runs green on the
product library in the ordinary suite."""
import os
import subprocess
import sys

import pytest

from gru4rec_amd import build as g4r_build

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SELECTION = ['tests/test_gpu_parity.py::test_first_step_intermediates[bprmax_elu]',
             'tests/test_gpu_baseline_configs.py::test_cfg4_exact_shape',
             'tests/test_gpu_parity.py::test_baseline_config2_shape_few_steps',
             'tests/test_gpu_golden.py::test_product_reproduces_reference_run[bprmax_constrained]']
# one step from zero accumulators: what must fail and what must still pass (p1 = the first-step test's tag)
FIRST_STEP = {1: (('p1 acc_Wy', 'p1 acc_By'), ('p1 acc_Wx0', 'p1 acc_Wh0', 'p1 dWx0')),
              2: (('p1 dWy', 'p1 dBy'), ('p1 acc_Wy', 'p1 acc_By', 'p1 acc_Wx0', 'p1 dWx0')),
              3: (('p1 acc_Wx0', 'p1 acc_Wh0', 'p1 acc_Wrz0', 'p1 acc_Bh0'), ('p1 acc_Wy', 'p1 acc_By', 'p1 dWy')),
              6: (('p1 dWy',), ('p1 acc_Wy', 'p1 acc_By', 'p1 acc_Wx0', 'p1 dWx0'))}


@pytest.fixture(scope='module')
def mutants():
    paths = g4r_build.build_mutants()
    assert all(os.path.exists(p) for p in paths)
    return dict(zip(sorted(g4r_build.MUTANTS), paths))


@pytest.mark.parametrize('k', sorted(FIRST_STEP))      # (mutant 4, the stale-register pipeline, has its own test: test_gpu_stress.py)
def test_mutant_turns_the_parity_tests_red(mutants, k, tmp_path):
    for i, sel in enumerate(SELECTION):
        rep = str(tmp_path / ('report%d.txt' % i))
        env = dict(os.environ, G4R_LIB=mutants[k], G4R_PARITY_REPORT=rep)
        r = subprocess.run([sys.executable, '-m', 'pytest', sel, '-x', '-q', '-p', 'no:cacheprovider'], cwd=ROOT, env=env,
                           capture_output=True, text=True, timeout=900)
        out = r.stdout + r.stderr
        assert r.returncode == 1, 'mutant %d (%s) passed %s:\n%s' % (k, g4r_build.MUTANTS[k], sel, out[-3000:])
        if i == 0:
            # the per-tensor report of the child: the damaged tensors are red, the others still green
            lines = open(rep).read().splitlines()
            state = {ln[:28].strip(): ln.rstrip().endswith('FAIL') for ln in lines if 'worst/tol' in ln}
            must_fail, must_pass = FIRST_STEP[k]
            assert all(state[n] for n in must_fail), (k, {n: state[n] for n in must_fail})
            assert not any(state[n] for n in must_pass), (k, {n: state[n] for n in must_pass})


EXACT_SELECTION = ['tests/test_gpu_exact_replicas.py::test_reduce_form_against_the_oracle_run_as_replicas[bprmax_constrained]',
                   'tests/test_gpu_exact_replicas.py::test_mean_form_against_the_oracle_run_as_replicas[bprmax_constrained]']


def test_mutant_5_turns_the_exact_replica_parity_red(mutants, tmp_path):
    """The 1 / nranks factor of the joint update x 1.01 (REDUCE: the gradient scale; MEAN: the mean over the touching ranks): the
    oracle-as-replicas tests of the forms that carry it must fail, the SUM form (no such factor) must still pass."""
    for i, (sel, want_rc) in enumerate([(s_, 1) for s_ in EXACT_SELECTION] +
                                       [('tests/test_gpu_exact_replicas.py::test_exact_mode_against_the_oracle_run_as_replicas[bprmax_constrained]', 0)]):
        env = dict(os.environ, G4R_LIB=mutants[5], G4R_PARITY_REPORT=str(tmp_path / ('x%d.txt' % i)))
        r = subprocess.run([sys.executable, '-m', 'pytest', sel, '-x', '-q', '-p', 'no:cacheprovider'], cwd=ROOT, env=env,
                           capture_output=True, text=True, timeout=900)
        assert r.returncode == want_rc, 'mutant 5 on %s: rc %d\n%s' % (sel, r.returncode, (r.stdout + r.stderr)[-3000:])


def test_mutant_8_turns_the_hot_item_case_red(mutants, tmp_path):
    """The owner scan of k_update_l loses one occurrence per later 1024-id slice: the hot-item case must fail on dWy; a shape whose owners never reach a second slice must still pass."""
    for i, (sel, want_rc) in enumerate([('tests/test_gpu_lean_edges.py::test_hot_item_past_1024[0.0]', 1),
                                        ('tests/test_gpu_lean_edges.py::test_partial_16_tiles[20-17-0.0]', 0)]):
        rep = str(tmp_path / ('hot%d.txt' % i))
        env = dict(os.environ, G4R_LIB=mutants[8], G4R_PARITY_REPORT=rep)
        r = subprocess.run([sys.executable, '-m', 'pytest', sel, '-x', '-q', '-p', 'no:cacheprovider'], cwd=ROOT, env=env,
                           capture_output=True, text=True, timeout=900)
        assert r.returncode == want_rc, 'mutant 8 on %s: rc %d\n%s' % (sel, r.returncode, (r.stdout + r.stderr)[-3000:])
        if want_rc:
            lines = open(rep).read().splitlines()
            state = {ln[:28].strip(): ln.rstrip().endswith('FAIL') for ln in lines if 'worst/tol' in ln}
            assert state['hot dWy'], state


def _child(lib, sel, rep):
    env = dict(os.environ, G4R_LIB=lib, G4R_PARITY_REPORT=rep)
    r = subprocess.run([sys.executable, '-m', 'pytest', sel, '-x', '-q', '-p', 'no:cacheprovider'], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=900)
    lines = open(rep).read().splitlines() if os.path.exists(rep) else []
    return r, {ln[:28].strip(): ln[:ln.find('(hot row')].rstrip().endswith('FAIL') if '(hot row' in ln else ln.rstrip().endswith('FAIL')
               for ln in lines if 'worst/tol' in ln or 'counters:' in ln}


def test_mutant_16_turns_the_generic_hot_item_case_red(mutants, tmp_path):
    """The owner walk of k_sparse_update_generic loses the first hit of its second and third pass: the hot-item case must fail on
    dWy of the hot rows (item 0 loses two of ~150 occurrences, item 1 one of ~85); a width-boundary case in which no item has more
    than 64 occurrences must still pass."""
    r, state = _child(mutants[16], 'tests/test_gpu_generic_edges.py::test_hot_items[40-sgd_mom]', str(tmp_path / 'hot.txt'))
    assert r.returncode == 1, 'mutant 16 passed the hot-item case:\n%s' % (r.stdout + r.stderr)[-3000:]
    assert state['hot sgd_mom D=40 dWy hot0'] and state['hot sgd_mom D=40 dWy hot1'], state
    r, state = _child(mutants[16], 'tests/test_gpu_generic_edges.py::test_row_width[64-rmsprop]', str(tmp_path / 'width.txt'))
    assert r.returncode == 0, 'mutant 16 on a case without a second pass: rc %d\n%s' % (r.returncode, (r.stdout + r.stderr)[-3000:])


def test_mutant_17_turns_the_second_statistic_red(mutants, tmp_path):
    """opt_rule's new second statistic x 1.01: an adadelta and an adam case must fail on acc2_* (sparse rows and dense tensors: one rule),
    a rmsprop case (no second statistic) must still pass."""
    for opt in ('adadelta', 'adam'):
        r, state = _child(mutants[17], 'tests/test_gpu_generic_edges.py::test_row_width[260-%s]' % opt, str(tmp_path / (opt + '.txt')))
        assert r.returncode == 1, 'mutant 17 passed the %s case:\n%s' % (opt, (r.stdout + r.stderr)[-3000:])
        tag = '%s D=260' % opt
        assert state[tag + ' acc2_Wy'] and state[tag + ' acc2_By'] and state[tag + ' acc2_Wh0'], state
    r, state = _child(mutants[17], 'tests/test_gpu_generic_edges.py::test_row_width[260-rmsprop]', str(tmp_path / 'rms.txt'))
    assert r.returncode == 0, 'mutant 17 on rmsprop: rc %d\n%s' % (r.returncode, (r.stdout + r.stderr)[-3000:])


def test_mutant_18_turns_the_quad_that_ends_on_column_M_red(mutants, tmp_path):
    """k_loss_rows takes a quad whose last column is the first inactive in-batch column as wholly active: at B = 37 the run with
    M = 35 (quad [32, 36)) must fail on ds; the runs with M = 36 and M = 34 of the same case, where no quad ends on column M, pass."""
    r, state = _child(mutants[18], 'tests/test_gpu_loss_rows.py::test_loss_rows[elubm-q4099]', str(tmp_path / 'm18.txt'))
    assert r.returncode == 1, 'mutant 18 passed the four-column case:\n%s' % (r.stdout + r.stderr)[-3000:]
    assert state['elubm q4099 M=35 ds'], state
    assert not state['elubm q4099 M=36 ds'] and not state['elubm q4099 M=34 ds'] and not state['elubm q4099 M=36 loss'], state


def test_mutant_19_turns_the_first_trip_past_the_prefetch_red(mutants, tmp_path):
    """k_loss_rows' first pass skips the first loop trip past the prefetched groups: N = 12301 (columns 8192 .. 12287 of every row)
    must fail on ds; N = 4099, where the prefetched groups hold the whole row, passes."""
    r, state = _child(mutants[19], 'tests/test_gpu_loss_rows.py::test_loss_rows[elubm-q12301]', str(tmp_path / 'm19a.txt'))
    assert r.returncode == 1, 'mutant 19 passed N = 12301:\n%s' % (r.stdout + r.stderr)[-3000:]
    assert state['elubm q12301 M=37 ds'], state
    r, state = _child(mutants[19], 'tests/test_gpu_loss_rows.py::test_loss_rows[elubm-q4099]', str(tmp_path / 'm19b.txt'))
    assert r.returncode == 0, 'mutant 19 on N = 4099: rc %d\n%s' % (r.returncode, (r.stdout + r.stderr)[-3000:])


HIDDEN = 'tests/test_gpu_hidden_act.py::'
HIDDEN_FAMILIES = ('lean', 'wide_w4')      # a k_gru_da site and a k_gru_bwd_pre site
HIDDEN_ACTS = ('tanh', 'relu', 'linear', 'leaky-0.2', 'elu-0.5', 'selu-1.0507-1.6733')


def _hidden_children(lib, ids, rep):
    """The test ids of tests/test_gpu_hidden_act.py in one child process on library `lib`: (return code, output, per test -- in the
    order of its `--- hidden_act ...` header in the report -- {report line name: failed})."""
    env = dict(os.environ, G4R_LIB=lib, G4R_PARITY_REPORT=rep)
    r = subprocess.run([sys.executable, '-m', 'pytest'] + [HIDDEN + i for i in ids] + ['-q', '-p', 'no:cacheprovider'], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=900)
    sections = {}
    for ln in (open(rep).read().splitlines() if os.path.exists(rep) else []):
        if ln.startswith('--- hidden_act'):
            cur = sections.setdefault(ln.split(':')[0], {})
        elif 'worst/tol' in ln:
            cur[ln[:28].strip()] = ln.rstrip().endswith('FAIL')
    return r.returncode, (r.stdout + r.stderr)[-3000:], sections


def _one_step_ids():
    return ['test_one_step_against_the_float64_oracle[%s-%s-bprmax-dh0.00]' % (f, a) for f in HIDDEN_FAMILIES for a in HIDDEN_ACTS]


def test_mutant_22_turns_the_sign_bit_cases_red(mutants, tmp_path):
    """The branch decided on c >= 0: where the forward returned -0.0 (elu / selu of a = -1e-9) the backward takes the positive slope.  The
    sign-bit cases of elu and selu must fail on da, at a k_gru_da site (lean) and at a k_gru_bwd_pre site (wide); leaky, whose p0 * a
    is not zero, and the one-step cases of every activation (no candidate rounds to zero there) must pass."""
    ids = ['test_branch_travels_in_the_sign_bit_of_the_stored_candidate[%s-%s]' % (f, a) for f in HIDDEN_FAMILIES
           for a in ('elu-0.5', 'selu-1.0507-1.6733', 'leaky-0.2')]
    rc, out, sec = _hidden_children(mutants[22], ids, str(tmp_path / 'm22c.txt'))
    assert rc == 1, 'mutant 22 on the sign-bit cases: rc %d\n%s' % (rc, out)
    for f in HIDDEN_FAMILIES:
        for a in ('elu-0.5', 'selu-1.0507-1.6733'):
            assert sec['--- hidden_act sign bit %s %s' % (f, a)]['sb dV0 da'], (f, a, sec)
        assert not any(sec['--- hidden_act sign bit %s leaky-0.2' % f].values()), (f, sec)
    rc, out, sec = _hidden_children(mutants[22], _one_step_ids(), str(tmp_path / 'm22a.txt'))
    assert rc == 0, 'mutant 22 on the one-step cases: rc %d\n%s' % (rc, out)
    assert len(sec) == len(HIDDEN_FAMILIES) * len(HIDDEN_ACTS), sorted(sec)


def test_mutant_23_turns_the_negative_slope_red(mutants, tmp_path):
    """The negative-branch slope of leaky / elu / selu x 1.01: their one-step cases must fail on dV0 (da) and on dWx0, lean and wide; the
    tanh and relu rows (and linear) must pass."""
    rc, out, sec = _hidden_children(mutants[23], _one_step_ids(), str(tmp_path / 'm23.txt'))
    assert rc == 1, 'mutant 23 on the one-step cases: rc %d\n%s' % (rc, out)
    for f in HIDDEN_FAMILIES:
        for a in HIDDEN_ACTS:
            state = sec['--- hidden_act one step %s-%s-bprmax-dh0.00' % (f, a)]
            if a in ('tanh', 'relu', 'linear'):
                assert not any(state.values()), (f, a, state)
            else:
                assert state['ha dV0 da'] and state['ha dWx0'], (f, a, state)
                assert not state['ha r0'] and not state['ha z0'] and not state['ha c0'] and not state['ha dV0 dzp'], (f, a, state)


WIDE = 'tests/test_gpu_wide_edges.py::'


def test_mutant_29_turns_the_sixteenth_dy_plane_red(mutants, tmp_path):
    """finish_rows adds up min(nsl, 15) planes: the case with 16 dy slices (D = 512, slices of 96) must fail on the input rows' update --
    dWy and, through g^2, acc_Wy (the embedding is constrained: the input rows are rows of Wy) --; the case with 12 slices must pass."""
    r, state = _child(mutants[29], WIDE + 'test_dy_16_slices', str(tmp_path / 'm29a.txt'))
    assert r.returncode == 1, 'mutant 29 passed the 16-slice case:\n%s' % (r.stdout + r.stderr)[-3000:]
    assert state['dy16 dWy'] and state['dy16 acc_Wy'], state
    r, state = _child(mutants[29], WIDE + 'test_two_stage_slices', str(tmp_path / 'm29b.txt'))
    assert r.returncode == 0, 'mutant 29 on 12 slices: rc %d\n%s' % (r.returncode, (r.stdout + r.stderr)[-3000:])


def test_mutant_30_turns_the_second_input_slice_red(mutants, tmp_path):
    """k_gru_p1s draws the embedding-dropout mask of input slice s from the k offset inside the slice: with two input slices (embedding 144:
    80 + 64) the second slice is masked by the first one's bits, which is neither the oracle's mask nor the one finish_rows regenerates: the
    case must fail; with one slice (embedding 80, slice start 0) nothing changes and the case must pass."""
    r, state = _child(mutants[30], WIDE + 'test_input_width[144]', str(tmp_path / 'm30a.txt'))
    assert r.returncode == 1, 'mutant 30 passed the two-slice case:\n%s' % (r.stdout + r.stderr)[-3000:]
    assert state['loss curve'] and state['in144 dE'], state
    r, state = _child(mutants[30], WIDE + 'test_input_width[80]', str(tmp_path / 'm30b.txt'))
    assert r.returncode == 0, 'mutant 30 on one input slice: rc %d\n%s' % (r.returncode, (r.stdout + r.stderr)[-3000:])


EDGES = 'tests/test_gpu_predict_edges.py::'


def _edge_children(lib, ids, rep):
    """Test ids in one child process on library `lib`: (return code, output, {report line name: failed})."""
    env = dict(os.environ, G4R_LIB=lib, G4R_PARITY_REPORT=rep)
    r = subprocess.run([sys.executable, '-m', 'pytest'] + list(ids) + ['-q', '-p', 'no:cacheprovider'], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=900)
    lines = open(rep).read().splitlines() if os.path.exists(rep) else []
    return r.returncode, (r.stdout + r.stderr)[-3000:], {ln[:28].strip(): ln.rstrip().endswith('FAIL') for ln in lines if 'worst/tol' in ln}


def test_mutant_34_turns_the_rows_past_the_first_score_tile_red(mutants, tmp_path):
    """k_score_all without By in the row tiles past the first: every candidate case of test_gpu_predict_edges.py (130 rows) and the 129-
    and 257-row cases must fail, on every step; the 128-row case, the width cases (37 rows) and test_predict_and_ranks (40 rows) must
    pass -- no prediction test before test_gpu_predict_edges.py had a row past the first 128."""
    acts = ('linear', 'relu', 'tanh', 'elu-0.5', 'softmax', 'softmax_logit')
    widths = ('d260', 'd320', 'd512_geo0', 'd512_geo1', 'd768', 'd1024')
    ids = [EDGES + 'test_candidate_lists[%s]' % a for a in acts] + [EDGES + 'test_rows[%d]' % pb for pb in (128, 129, 257)] + \
          [EDGES + 'test_widths[%s]' % w for w in widths]
    rc, out, state = _edge_children(mutants[34], ids, str(tmp_path / 'm34a.txt'))
    assert rc == 1, 'mutant 34 on the prediction edge cases: rc %d\n%s' % (rc, out)
    for a in acts:
        assert all(state['c %s s%d' % (a, i)] for i in (0, 3, 5)), (a, state)
    assert all(state['r %d s%d' % (pb, i)] for pb in (129, 257) for i in range(4)), state
    assert not any(state['r 128 s%d' % i] for i in range(4)), state
    assert not any(state['w %s s%d' % (w, i)] for w in widths for i in range(4)), state
    rc, out, _ = _edge_children(mutants[34], ['tests/test_gpu_parity.py::test_predict_and_ranks'], str(tmp_path / 'm34b.txt'))
    assert rc == 0, 'mutant 34 on test_predict_and_ranks: rc %d\n%s' % (rc, out)


def test_mutant_35_turns_the_third_k_chunk_red(mutants, tmp_path):
    """k_gru_p1 at prediction without its K chunks from the third on (k >= 512 of K = IN + D adds zeros): the width cases and the two
    stacks with a 512 layer of test_gpu_predict_edges.py must fail.  Where the lost columns are hidden-state columns only (D <= 512) the
    first step, from a zero state, still passes and the second fails; at D = 768 and 1024 input columns go as well and the first step
    fails.  D = 260 is among the failures: its K = 520 leaves 8 hidden columns in a third chunk.  K = 400 (embedding 100 + D 300), the one-hot
    D = 340 (K = 340) and test_gpu_hidden_act.py::test_predict_step (K <= 512) must pass -- no prediction test before
    test_gpu_predict_edges.py had a third chunk."""
    zero_ok = ('w d260', 'w d320', 'w d512_geo0', 'w d512_geo1', 'i s36_512', 'i s512_36')
    ids = [EDGES + 'test_widths[%s]' % w for w in ('d260', 'd320', 'd512_geo0', 'd512_geo1', 'd768', 'd1024')] + \
          [EDGES + 'test_input_widths[%s]' % w for w in ('s36_512', 's512_36', 'e100_d300', 'onehot340')]
    rc, out, state = _edge_children(mutants[35], ids, str(tmp_path / 'm35a.txt'))
    assert rc == 1, 'mutant 35 on the prediction edge cases: rc %d\n%s' % (rc, out)
    for tag in zero_ok:
        assert not state[tag + ' s0'] and state[tag + ' s1'] and state[tag + ' s3'], (tag, state)
    for tag in ('w d768', 'w d1024'):
        assert state[tag + ' s0'] and state[tag + ' s1'], (tag, state)
    assert not any(state['i %s s%d' % (w, i)] for w in ('e100_d300', 'onehot340') for i in range(4)), state
    rc, out, _ = _edge_children(mutants[35], ['tests/test_gpu_hidden_act.py::test_predict_step'], str(tmp_path / 'm35b.txt'))
    assert rc == 0, 'mutant 35 on test_gpu_hidden_act.py::test_predict_step: rc %d\n%s' % (rc, out)


def test_product_library_is_not_a_mutant():
    from gru4rec_amd import _native
    assert 'G4R_LIB' not in os.environ or '_variants' not in os.environ['G4R_LIB']
    assert '_variants' not in _native.LIB_PATH

"""bench.py's N > 1 code path, driven on the CPU with a stand-in for the device model.

No multi-GPU box has ever run `bench.py --gpus N`: the driver's SCALE run would be the first.  Everything the RCCL ranks need below
`bench.main()` -- the model handle and the collectives on it -- is replaced by a fake that answers as rank 0 of a world of two (every
collective returns this rank's own value), so that the Python of the path is executed: plan per rank, timed region with the
on-stream reconciliation, per-kernel pass, the reconciliation measurement, `value` / `value_step_only` / `value_source`, the
`multi_gpu` object, the ONE JSON line on stdout.  What it cannot check is RCCL itself.  The same fake, as a single rank, drives
`--dump-outputs`: what the timed steps computed, read back right behind them, from inputs that do not change between runs."""
import glob
import json
import os
import sys
import tempfile

import numpy as np
import pytest

import bench
from gru4rec_amd import _native, launch, synth


class FakeModel:
    """The methods bench.py calls on _native.Model, with plausible answers and no device."""
    instances = []

    def __init__(self, **kw):
        self.kw = kw
        self.sync_k = 0
        self.calls = []
        self.profile_mode = 0
        self.inputs = {}
        FakeModel.instances.append(self)

    def comm_init(self, uid, nranks, rank): self.comm = (uid, nranks, rank)
    def comm_nranks(self): return self.kw['nranks']
    def set_param(self, name, arr, layer=0): self.inputs[(name, layer)] = np.array(arr)
    def set_popularity(self, *a, **k): self.inputs['popularity'] = [None if x is None else np.array(x) for x in a]

    def set_plan(self, plan):
        self.T = int(plan['T'])
        self.inputs['plan'] = {k: np.array(plan[k]) for k in ('in_idx', 'out_idx', 'reset', 'M')}

    def get_param(self, name, shape, layer=0):
        self.calls.append(('get', name, layer))
        return (np.arange(int(np.prod(shape)), dtype=np.float32) + 1000 * layer).reshape(shape)
    def reset_hidden(self): pass

    def train_steps(self, t0, n):
        assert 0 <= t0 and t0 + n <= self.T, 'step range outside the plan'
        self.calls.append((t0, n, self.sync_k, self.profile_mode))

    def get_losses(self, t0, n): return np.full(n, 0.7, dtype=np.float32)
    def profile(self, mode): self.profile_mode = int(mode)

    def kernel_times(self):
        names = ('k_gru_fwd', 'k_score_fwd', 'k_loss_rows', 'k_score_bwd', 'k_gru_bwd', 'k_update', 'rccl_allreduce', 'k_dense_apply')
        return {n: (0.005 * 300, 300) for n in names}

    def set_sync_every(self, k):
        self.sync_k = int(k)
        return True      # small item tables: the library reconciles on the stream

    def comm_sync_sparse(self): self.calls.append(('sync',))
    def comm_max(self, v): return int(v)
    def p2p_active(self): return False

    def get_debug(self, name, shape):
        return np.array([{'dense_count': 60300.0, 'graph_mode': 1.0, 'dev_syncs': 3.0}.get(name, 0.0)], dtype=np.float32)

    def close(self): pass


@pytest.mark.parametrize('extra', [[], ['--sparse-exact']], ids=['gpu_local_rows', 'exact_replicas'])
def test_bench_main_as_rank_0_of_2(monkeypatch, capsys, extra):
    FakeModel.instances.clear()
    monkeypatch.setenv('RANK', '0')
    monkeypatch.setenv('LOCAL_RANK', '0')
    monkeypatch.setenv('WORLD_SIZE', '2')
    monkeypatch.delenv('G4R_FORCE_STAGED', raising=False)
    monkeypatch.setattr(_native, 'device_count', lambda: 2)
    monkeypatch.setattr(_native, 'Model', FakeModel)
    monkeypatch.setattr(launch, 'unique_id', lambda rank, world, **kw: b'\0' * 128)
    monkeypatch.setattr(launch, 'cleanup', lambda rank: None)
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '2', '--steps', '20', '--warmup', '5', '--full', '--no-cpu-baseline', '--no-micro',
                                      '--profile-steps', '16'] + extra)
    bench.main()
    lines = [l for l in capsys.readouterr().out.splitlines() if l.strip()]
    assert len(lines) == 1, 'rank 0 prints ONE JSON line'
    out = json.loads(lines[0])
    for k in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling', 'vs_baseline', 'dtype', 'data', 'config'):
        assert k in out
    assert out['n_gpus'] == 2 and out['steps'] == 20 and out['warmup'] == 5 and out['scaling'] == 'weak' and out['unit'] == 'mini-batches/s'
    assert out['config']['global_batch'] == 2 * bench.CONFIGS['cfg2']['batch_size']
    assert out['value'] > 0 and np.isfinite(out['value'])
    assert 'multi_gpu' in out and out['multi_gpu']['ncclCommCount'] == 2 and len(out['multi_gpu']['rank_ms_per_step']) == 2
    m = FakeModel.instances[0]
    assert m.kw['rank'] == 0 and m.kw['nranks'] == 2
    timed = [c for c in m.calls if c[0] == 5 and c[1] == 20]
    assert len(timed) == 1, 'the timed region is ONE call over exactly --steps plan steps behind the warmup'
    if extra:
        assert m.kw['sparse_exact'] == 3 and timed[0][2] == 0 and 'value_source' not in out      # nothing to reconcile in this mode
        assert out['config']['item_rows'].startswith('exact replicas')
    else:
        # GPU-local rows: the timed region runs WITH the reconciliation every sync_every steps (4 at two ranks), the bare step is reported next to it
        assert m.kw['sparse_exact'] == 0 and timed[0][2] == 4
        assert 'reconciles the GPU-local item tables every 4 steps' in out['value_source']
        assert out['value_step_only'] > 0
        assert out['multi_gpu']['reconciliation']['timed_region_includes_reconciliation'] is True
        assert all(c[2] == 0 for c in m.calls if len(c) == 4 and c[3] != 0), 'the per-kernel passes time the bare step'


def _boom(name):
    def f(*a, **k):
        raise AssertionError('a plain run must not reach %s' % name)
    return f


MOVED_KEYS = ('long_run', 'kernels', 'kernel_time_sum_us_per_step', 'dominant_kernel', 'roofline', 'roofline_gather_scatter', 'gather_scatter_micro',
              'large_catalogue', 'cpu_baseline', 'projection_8_gpus', 'reconciliation_one_rank_communicator', 'value_step_only')


def test_plain_run_times_its_steps_and_nothing_else(monkeypatch, capsys, tmp_path):
    """Without --full: warm-up, the timed steps, the dump, the result line.  No other step, no per-kernel pass, no micro-benchmark, no
    child run, no CPU baseline -- with none of the --no-... switches given -- and no file of an earlier run read."""
    monkeypatch.setattr(bench, 'cpu_baseline', _boom('cpu_baseline'))
    monkeypatch.setattr(bench, 'large_catalogue_legs', _boom('large_catalogue_legs'))
    monkeypatch.setattr(_native, 'bench_rows', _boom('bench_rows'))
    d = str(tmp_path / 'plain')
    with monkeypatch.context() as mp:
        mp.setattr(np, 'load', _boom('np.load'))
        mp.setattr(np, 'savez', _boom('np.savez'))
        out, m = _run_one_rank(mp, capsys, ['--steps', '7', '--warmup', '3', '--long-steps', '50', '--dump-outputs', d], flags=[])
    assert out['full'] is False and out['steps'] == 7 and out['warmup'] == 3
    for k in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step', 'n_gpus', 'config', 'events_per_s', 'loss_first', 'loss_last', 'dump_outputs'):
        assert k in out
    assert out['unit'] == 'mini-batches/s' and out['higher_is_better'] is True and out['dtype'] == 'f32'
    assert out['value'] > 0 and abs(out['value'] * out['ms_per_step'] - 1000.0) < 1e-6 * 1000.0
    assert not [k for k in MOVED_KEYS if k in out]
    assert [c for c in m.calls if c[0] != 'get'] == [(0, 3, 0, 0), (3, 7, 0, 0)], 'warm-up, then the timed steps, then nothing'
    assert m.profile_mode == 0
    # the same arguments with --full: the same plan, weights and popularity go in, the same arrays come out
    d2 = str(tmp_path / 'full')
    out2, m2 = _run_one_rank(monkeypatch, capsys, ['--steps', '7', '--warmup', '3', '--long-steps', '50', '--full', '--dump-outputs', d2])
    assert out2['full'] is True and 'long_run' in out2 and 'kernels' in out2
    steps2 = [c for c in m2.calls if len(c) == 4]
    assert steps2[:2] == [(0, 3, 0, 0), (3, 7, 0, 0)] and len(steps2) > 2
    assert out2['metric'] == out['metric'] and out2['config'] == out['config']
    assert sorted(m.inputs, key=str) == sorted(m2.inputs, key=str)
    for k, v in m.inputs.items():
        w = m2.inputs[k]
        for x, y in (zip(v.values(), w.values()) if isinstance(v, dict) else zip(v, w) if isinstance(v, list) else [(v, w)]):
            assert (x is None and y is None) or np.array_equal(x, y)
    got, got2 = _dumped(d), _dumped(d2)
    assert sorted(got) == sorted(got2)
    for k in got:
        np.testing.assert_array_equal(got[k], got2[k])


@pytest.mark.parametrize('extra', [[], ['--sparse-exact']], ids=['gpu_local_rows', 'exact_replicas'])
def test_plain_run_as_rank_0_of_2(monkeypatch, capsys, extra):
    """N > 1 without --full: the timed region as ever (with the on-stream reconciliation for GPU-local rows), no step behind it."""
    FakeModel.instances.clear()
    monkeypatch.setenv('RANK', '0')
    monkeypatch.setenv('LOCAL_RANK', '0')
    monkeypatch.setenv('WORLD_SIZE', '2')
    monkeypatch.delenv('G4R_FORCE_STAGED', raising=False)
    monkeypatch.setattr(_native, 'device_count', lambda: 2)
    monkeypatch.setattr(_native, 'Model', FakeModel)
    monkeypatch.setattr(launch, 'unique_id', lambda rank, world, **kw: b'\0' * 128)
    monkeypatch.setattr(launch, 'cleanup', lambda rank: None)
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '2', '--steps', '20', '--warmup', '5', '--long-steps', '50', '--profile-steps', '16'] + extra)
    bench.main()
    lines = [l for l in capsys.readouterr().out.splitlines() if l.strip()]
    assert len(lines) == 1
    out = json.loads(lines[0])
    m = FakeModel.instances[0]
    k = 0 if extra else 4
    assert m.calls == [(0, 5, k, 0), (5, 20, k, 0)]
    assert out['n_gpus'] == 2 and out['full'] is False and out['value'] > 0 and out['multi_gpu']['ncclCommCount'] == 2
    assert ('value_source' in out) == (not extra) and not [k for k in MOVED_KEYS if k in out]
    assert out['multi_gpu']['reconciliation'] is None


def test_synth_cache_is_opt_in(monkeypatch, tmp_path):
    """make_plan keeps the generated sessions only in a directory the caller names, and a plan read from there equals a generated one."""
    cfg = bench.CONFIGS['cfg1']
    monkeypatch.setattr(tempfile, 'tempdir', str(tmp_path / 'tmp'))
    os.makedirs(tempfile.gettempdir())
    fresh, sup = bench.make_plan(cfg, 40, 0, 1)
    assert os.listdir(tempfile.gettempdir()) == []
    shared = str(tmp_path / 'shared')
    first, _ = bench.make_plan(cfg, 40, 0, 1, cache_dir=shared)
    assert len(os.listdir(shared)) == 1 and os.listdir(tempfile.gettempdir()) == []
    monkeypatch.setattr(synth, 'make_sessions', _boom('the generator when the sessions are in the directory'))
    again, sup2 = bench.make_plan(cfg, 40, 0, 1, cache_dir=shared)
    for k in ('in_idx', 'out_idx', 'reset', 'M'):
        np.testing.assert_array_equal(fresh[k], first[k])
        np.testing.assert_array_equal(fresh[k], again[k])
    np.testing.assert_array_equal(sup, sup2)


def _run_one_rank(monkeypatch, capsys, argv, flags=('--no-cpu-baseline', '--no-micro')):
    FakeModel.instances.clear()
    for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'G4R_FORCE_STAGED'):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(_native, 'device_count', lambda: 1)
    monkeypatch.setattr(_native, 'Model', FakeModel)
    monkeypatch.setattr(launch, 'unique_id', lambda rank, world, **kw: None)
    monkeypatch.setattr(launch, 'cleanup', lambda rank: None)
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '1'] + list(flags) + argv)
    bench.main()
    lines = [l for l in capsys.readouterr().out.splitlines() if l.strip()]
    assert len(lines) == 1
    return json.loads(lines[0]), FakeModel.instances[0]


def _dumped(d):
    return {os.path.basename(p)[:-4]: np.load(p) for p in sorted(glob.glob(os.path.join(d, '*')))}


def test_bench_dump_outputs_reads_back_the_timed_steps(monkeypatch, capsys, tmp_path):
    runs = []
    for name in ('a', 'b'):
        d = str(tmp_path / name)
        out, m = _run_one_rank(monkeypatch, capsys, ['--steps', '7', '--warmup', '3', '--full', '--profile-steps', '16', '--long-steps', '50',
                                                     '--dump-outputs', d])
        runs.append((out, m, _dumped(d)))
    (out, m, got), (_, m2, got2) = runs
    assert out['steps'] == 7 and out['ms_per_step'] > 0
    steps = [c for c in m.calls if len(c) == 4]
    assert steps[1][:2] == (3, 7), 'the timed region is ONE call over exactly --steps plan steps behind the warmup'
    # every read lies between the timed call and the next step: the dump is the model right after the last timed step
    i_timed = m.calls.index(steps[1])
    reads = [i for i, c in enumerate(m.calls) if c[0] == 'get']
    assert reads and min(reads) == i_timed + 1 and max(reads) < m.calls.index(steps[2])
    D, B, I = 100, 128, 37483
    shapes = {'losses': (7,), 'Wx_0': (D, 3 * D), 'Wh_0': (D, D), 'Wrz_0': (D, 2 * D), 'Bh_0': (3 * D,), 'H_0': (B, D), 'Wy': (I, D), 'By': (I,)}
    assert {k: v.shape for k, v in got.items()} == shapes
    assert all(v.dtype in (np.float32, np.float64) for v in got.values())
    assert sum(os.path.getsize(p) for p in glob.glob(str(tmp_path / 'a' / '*'))) <= 64 * 10 ** 6
    assert out['dump_outputs']['arrays'] == {k: list(v) for k, v in shapes.items()}
    np.testing.assert_array_equal(got['Wy'], m.get_param('Wy', (I, D)))
    # the same arguments give the same inputs, and so the same outputs
    assert sorted(m.inputs, key=str) == sorted(m2.inputs, key=str)
    for k, v in m.inputs.items():
        w = m2.inputs[k]
        if isinstance(v, dict):
            for kk in v:
                np.testing.assert_array_equal(v[kk], w[kk])
        elif isinstance(v, list):
            for x, y in zip(v, w):
                assert (x is None and y is None) or np.array_equal(x, y)
        else:
            np.testing.assert_array_equal(v, w)
    for k in got:
        np.testing.assert_array_equal(got[k], got2[k])


def test_bench_dump_outputs_samples_item_rows_beyond_the_budget(monkeypatch, capsys, tmp_path):
    monkeypatch.setattr(bench, 'DUMP_BYTES', 2 * 10 ** 6)
    d = str(tmp_path / 'd')
    out, m = _run_one_rank(monkeypatch, capsys, ['--config', 'cfg1', '--steps', '5', '--warmup', '2', '--profile-steps', '0',
                                                 '--long-steps', '0', '--dump-outputs', d])
    got = _dumped(d)
    D, I = 100, 37483
    rows = got['Wy_rows'].astype(np.int64)
    assert got['Wy_rows'].dtype == np.float64 and (np.diff(rows) > 0).all() and rows.max() < I
    assert sum(v.nbytes for v in got.values()) <= 2 * 10 ** 6
    assert len(rows) > 1000
    plan = m.inputs['plan']
    assert set(plan['in_idx'][6]) | set(plan['out_idx'][6]) <= set(rows), 'the rows the last timed step gathered are kept'
    np.testing.assert_array_equal(got['Wy'], m.get_param('Wy', (I, D))[rows])
    np.testing.assert_array_equal(got['By'], m.get_param('By', (I,))[rows])


def test_bench_refuses_zero_steps(monkeypatch):
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--steps', '0'])
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 2

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

import numpy as np
import pytest

import bench
from gru4rec_amd import _native, launch


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
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '2', '--steps', '20', '--warmup', '5', '--no-cpu-baseline', '--no-micro',
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


def _run_one_rank(monkeypatch, capsys, argv):
    FakeModel.instances.clear()
    for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'G4R_FORCE_STAGED'):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(_native, 'device_count', lambda: 1)
    monkeypatch.setattr(_native, 'Model', FakeModel)
    monkeypatch.setattr(launch, 'unique_id', lambda rank, world, **kw: None)
    monkeypatch.setattr(launch, 'cleanup', lambda rank: None)
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '1', '--no-cpu-baseline', '--no-micro'] + argv)
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
        out, m = _run_one_rank(monkeypatch, capsys, ['--steps', '7', '--warmup', '3', '--profile-steps', '16', '--long-steps', '50',
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

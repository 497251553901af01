"""Host side of evaluation.recommend_gpu / list_metrics (no device): the metrics against a direct restatement, the slot map from the
plan builder's arange trick against a brute-force walk, the seen-item tables against sets, argument validation, run.py's options."""
import importlib.util
import os

import numpy as np
import pandas as pd
import pytest

from gru4rec_amd import _native, evaluation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_list_metrics_against_a_direct_restatement():
    rank = np.array([1, 3, 7, 2.5, 21, 5, 1, 400], dtype=np.float32)
    items = np.array([[1, 2, 3, 4, 5, 6], [1, 2, 9, 9, 9, 9], [7, 2, 3, 4, 5, 8]] + [[1, 2, 3, 4, 5, 6]] * 5)
    res = dict(rank=rank, items=items)
    cuts = [1, 5, 6]
    m = evaluation.list_metrics(res, cuts, n_items=50)
    import math
    for j, c in enumerate(cuts):
        rs = [float(r) for r in rank]                 # (float32 ranks hold these values exactly)
        rec = sum(1 for r in rs if r <= c) / len(rs)
        mrr = sum(1.0 / r for r in rs if r <= c) / len(rs)
        ndcg = sum(1.0 / math.log2(1.0 + r) for r in rs if r <= c) / len(rs)
        cov = len(set(items[:, :c].ravel().tolist())) / 50.0
        assert m['recall'][j] == pytest.approx(rec, rel=1e-12) and m['mrr'][j] == pytest.approx(mrr, rel=1e-12)
        assert m['ndcg'][j] == pytest.approx(ndcg, rel=1e-12) and m['coverage'][j] == pytest.approx(cov, rel=1e-12)
    assert evaluation.list_metrics(res, 5)['coverage'] == [None]
    assert evaluation.list_metrics(res, [1], n_items=50)['coverage'] == [2 / 50.0]
    with pytest.raises(ValueError):
        evaluation.list_metrics(res, [7], n_items=50)


@pytest.mark.parametrize('batch', [1, 3, 8])
def test_slot_map_against_a_walk_of_the_plan(batch):
    rng = np.random.RandomState(batch)
    lens = rng.randint(1, 9, size=11)
    lens[:8] = np.maximum(lens[:8], 2)
    offs = np.r_[0, np.cumsum(lens)].astype(np.int64)
    titems = rng.randint(0, 50, size=int(offs[-1])).astype(np.int32)
    plan = _native.build_plan(offs.astype(np.int32), np.arange(len(lens)), titems, batch, 1)
    rows, table = evaluation.slot_map(offs, batch)
    assert rows['T'] == plan['T'] and table.shape == (plan['T'], batch)
    np.testing.assert_array_equal(rows['M'], plan['M'])
    sess = np.repeat(np.arange(len(lens)), lens)
    used = []
    for t in range(plan['T']):
        for r in range(batch):
            if r >= plan['M'][t]:
                assert table[t, r] == -1
                continue
            row = table[t, r]
            # the input event of (t, r) is table row `row`, and its successor in the same session is the step's target
            assert plan['in_idx'][t, r] == titems[row]
            assert sess[row + 1] == sess[row] and plan['out_idx'][t, r] == titems[row + 1]
            used.append(row)
    has_next = np.r_[sess[1:] == sess[:-1], False]
    assert sorted(used) == np.flatnonzero(has_next).tolist()      # each row that has a successor appears exactly once


def test_seen_tables_against_sets():
    rng = np.random.RandomState(4)
    lens = rng.randint(1, 40, size=30)
    offs = np.r_[0, np.cumsum(lens)].astype(np.int64)
    titems = rng.randint(0, 12, size=int(offs[-1]))
    t = evaluation.seen_tables(titems, offs)
    assert t['offs'][0] == 0 and len(t['offs']) == len(lens) + 1 and len(t['items']) == len(t['first']) == t['offs'][-1]
    for s in range(len(lens)):
        ev = titems[offs[s]:offs[s + 1]]
        lst, first = t['items'][t['offs'][s]:t['offs'][s + 1]], t['first'][t['offs'][s]:t['offs'][s + 1]]
        assert lst.tolist() == sorted(set(ev.tolist()))
        assert first.tolist() == [ev.tolist().index(i) for i in lst]
        for p in range(len(ev)):      # the rule of the kernel: found with first <= position  <=>  seen up to and including p
            assert set(lst[first <= p].tolist()) == set(ev[:p + 1].tolist())


class _NoDevice:
    """As much of a GRU4Rec as recommend_gpu's checks need; creating the device model fails the test."""
    error_during_train = False
    itemidmap = pd.Series(np.arange(30), index=np.arange(100, 130))

    def _ensure_model(self):
        raise AssertionError('the checks come before any device work')


def _table(n_sessions=4):
    return pd.DataFrame({'SessionId': np.repeat(np.arange(n_sessions), 3), 'ItemId': 100 + np.arange(3 * n_sessions) % 30,
                         'Time': np.arange(3 * n_sessions)})


@pytest.mark.parametrize('k', [0, -1, 31, 2.5, True, _native.G4R_TOPK_MAX + 1])
def test_k_is_checked_before_anything_else(k):
    with pytest.raises(ValueError, match='k = '):
        evaluation.recommend_gpu(_NoDevice(), _table(), k=k, batch_size=2)


def test_other_arguments_are_checked_without_a_device():
    g = _NoDevice()
    with pytest.raises(ValueError, match='k = '):
        evaluation.recommend_gpu(g, _table(), k=6, items=np.arange(100, 105), batch_size=2)      # more than the candidates
    with pytest.raises(NotImplementedError):
        evaluation.recommend_gpu(g, _table(), k=5, mode='optimistic', batch_size=2)
    with pytest.raises(ValueError, match='batch_size'):
        evaluation.recommend_gpu(g, _table(), k=5, batch_size=0)
    with pytest.raises(IndexError):
        evaluation.recommend_gpu(g, _table(4), k=5, batch_size=5)
    with pytest.raises(KeyError):
        evaluation.recommend_gpu(g, _table(), k=5, batch_size=2, exclude=[999])
    g.error_during_train = True
    with pytest.raises(Exception):
        evaluation.recommend_gpu(g, _table(), k=5, batch_size=2)


def _run_py():
    spec = importlib.util.spec_from_file_location('g4r_run_py', os.path.join(ROOT, 'run.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_run_py_accepts_the_new_options_and_keeps_the_old_ones():
    run = _run_py()
    longs = [o[1] for o in run.OPTIONS]
    before = ['--parameter_string', '--parameter_file', '--load_model', '--save_model', '--test', '--measure', '--eval_type',
              '--sample_store_size', '--sample_store_on_cpu', '--gru4rec_model', '--item_key', '--session_key', '--time_key',
              '--primary_metric', '--log_primary_metric', '--sparse_exact', '--gpus']
    assert [x for x in longs if x not in ('--save_recs', '--recs_k')] == before
    ap = run.build_parser()
    o = ap.parse_args(['model.pickle', '-l', '-t', 'test.tsv'])
    assert o.save_recs is None and o.recs_k == 20 and o.measure == [20] and o.eval_type == 'standard' and o.gpus == 1
    o = ap.parse_args(['model.pickle', '-l', '-t', 'test.tsv', '--save_recs', 'recs.npz', '--recs_k', '50'])
    assert o.save_recs == 'recs.npz' and o.recs_k == 50

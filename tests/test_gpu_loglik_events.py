"""evaluation.loglik_gpu / g4r_loglik_events (the log-probability of the logged next item at EVERY event of a test set) against the
library's own pinned entries on every event's prefix: session_log_partition's raw (zeta, Q) and its lse bits, the target's z from
score_candidates_sessions (softmax models: from the partition of the one-candidate list), the float64 formulas of tests/logprob_ref.py,
and sample_sessions' own log-probabilities along a drawn path.  Q is an exact integer, so everything but the last is bit for bit."""
import os
import re
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

import logprob_ref as lref
from gru4rec_amd import evaluation, synth
from gru4rec_amd.gru4rec import GRU4Rec
from test_gpu_continue_sessions import LENS, N_ITEMS, assert_bits, fitted, histories
from test_gpu_recommend_events import BATCH, make_test_set, prefixes
from test_gpu_sample_logprobs import big_model, raw_partition, ulp32

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ('row', 'session', 'target', 'logprob', 'lse', 'target_logit', 'zeta', 'Q', 'eligible')


def inv_t32(temperature):
    return np.float32(1.0) / np.float32(temperature)


def same(a, b):
    """Two loglik_gpu results, bit for bit."""
    for key in KEYS:
        x, y = np.asarray(a[key]), np.asarray(b[key])
        assert x.dtype == y.dtype and x.shape == y.shape, key
        if x.dtype == np.float32:
            assert_bits(x, y)
        else:
            np.testing.assert_array_equal(x, y, err_msg=key)


def want_eligible(hists, targets, items, exclude_seen, exclude):
    gone = set() if exclude is None else set(np.asarray(exclude).tolist())
    listed = None if items is None else set(np.asarray(items).tolist())
    return np.array([(listed is None or t in listed) and t not in gone and not (exclude_seen and t in set(np.asarray(h).tolist()))
                     for h, t in zip(hists, targets)], dtype=bool)


def check_columns(res, data):
    assert tuple(sorted(res)) == tuple(sorted(KEYS))
    hists, t = prefixes(data, res['row'])
    sess, items = t.SessionId.values, t.ItemId.values
    np.testing.assert_array_equal(res['row'], np.flatnonzero(np.r_[sess[1:] == sess[:-1], False]))
    np.testing.assert_array_equal(res['session'], sess[res['row']])
    np.testing.assert_array_equal(res['target'], items[res['row'] + 1])
    assert res['logprob'].dtype == res['lse'].dtype == res['target_logit'].dtype == res['zeta'].dtype == np.float32
    assert res['Q'].dtype == np.uint64 and res['eligible'].dtype == bool
    return hists


def check_prefix_loop(g, data, res, temperature, items=None, exclude_seen=False, exclude=None, pick=None, z_t=None):
    """The partition of every (picked) event against the prefix loop; with z_t (the picked events' oracle target logits) the
    target's columns too."""
    hists = check_columns(res, data)
    pick = np.arange(len(hists)) if pick is None else np.asarray(pick)
    hs = [hists[i] for i in pick]
    zeta, Q = raw_partition(g, hs, temperature, cand=items, exclude_history=exclude_seen, exclude=exclude)
    assert_bits(res['zeta'][pick], zeta)
    np.testing.assert_array_equal(res['Q'][pick], Q)
    lse = g.session_log_partition(hs, temperature=temperature, predict_for_item_ids=items, exclude_history=exclude_seen, exclude=exclude)
    assert_bits(res['lse'][pick], lse)
    if z_t is None:
        return
    on = want_eligible(hs, res['target'][pick], items, exclude_seen, exclude)
    np.testing.assert_array_equal(res['eligible'][pick], on)
    assert_bits(res['target_logit'][pick], z_t)
    assert np.isfinite(res['target_logit'][pick]).all()
    with np.errstate(all='ignore'):
        lp = np.where(on, lref.logprob(lref.d32(z_t, zeta, inv_t32(temperature)), Q), np.float32(-np.inf)).astype(np.float32)
    assert_bits(res['logprob'][pick], lp)
    assert (res['logprob'][pick][on] <= 0).all() and np.isfinite(res['logprob'][pick][on]).all()


def score_targets(g, hists, targets):
    return np.asarray(g.score_candidates_sessions(hists, [[t] for t in targets]), dtype=np.float32).reshape(-1)


def logit_targets(g, hists, targets):
    """softmax models: the pre-activation z of a target is the zeta of the partition over the one-candidate list [target]."""
    return np.array([raw_partition(g, [h], 1.0, cand=[t])[0][0] for h, t in zip(hists, targets)], dtype=np.float32)


# ---- 1. the prefix loop, bit for bit ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('temperature', [1.0, 0.5, 0.004])
@pytest.mark.parametrize('cand', [False, True])
@pytest.mark.parametrize('embed', ['onehot', 'embedding', 'constrained'])
@pytest.mark.parametrize('layers', [(30,), (100, 64)])
def test_equals_the_prefix_loop(layers, embed, cand, temperature):
    g = fitted('linear', layers, embed)
    assert g.n_items == N_ITEMS
    data = make_test_set(g, n_sessions=60, seed=len(layers) + int(cand), max_len=12)
    ids = g.itemidmap.index.values
    # the candidates hold most targets, not all, and fill a partial last tile
    items = ids[np.random.RandomState(7).permutation(len(ids))[:701]] if cand else None
    res = evaluation.loglik_gpu(g, data, items=items, temperature=temperature, batch_size=BATCH)
    hists, _ = prefixes(data, res['row'])
    assert len(hists) > 250
    z_t = score_targets(g, hists, res['target'])
    check_prefix_loop(g, data, res, temperature, items=items, z_t=z_t)
    assert res['eligible'].all() == (not cand) and res['eligible'].any()      # (701 of 1003 items: some targets are not listed)
    rec = evaluation.recommend_gpu(g, data, k=1, items=items, batch_size=BATCH)
    np.testing.assert_array_equal(rec['row'], res['row'])
    assert_bits(rec['target_score'], res['target_logit'])


# ---- 2. softmax models, and two scans per step whatever the final activation -----------------------------------------------------
@pytest.mark.parametrize('cand', [False, True])
@pytest.mark.parametrize('final_act', ['softmax', 'softmax_logit'])
def test_softmax_models(final_act, cand):
    g = fitted(final_act)
    data = make_test_set(g, n_sessions=60, seed=5, max_len=12)
    ids = g.itemidmap.index.values
    items = ids[np.random.RandomState(8).permutation(len(ids))[:701]] if cand else None
    res = evaluation.loglik_gpu(g, data, items=items, temperature=0.5, batch_size=BATCH)
    steps, scans, _, pieces = g._ensure_model().events_launches()
    assert steps > 5 and scans == 2 * steps and pieces == 1
    check_prefix_loop(g, data, res, 0.5, items=items)
    hists, _ = prefixes(data, res['row'])
    pick = np.random.RandomState(9).choice(len(hists), size=64, replace=False)
    z_t = logit_targets(g, [hists[i] for i in pick], res['target'][pick])
    check_prefix_loop(g, data, res, 0.5, items=items, pick=pick, z_t=z_t)


def test_two_scans_per_step_with_an_elementwise_activation():
    g = fitted('elu-0.5')
    data = make_test_set(g, n_sessions=60, seed=6, max_len=12)
    for kw in (dict(), dict(exclude_seen=True)):
        evaluation.loglik_gpu(g, data, batch_size=BATCH, **kw)
        steps, scans, _, pieces = g._ensure_model().events_launches()
        assert steps > 5 and scans == 2 * steps and pieces == 1


# ---- 3. exclusions ---------------------------------------------------------------------------------------------------------------
def with_repeats(g, data):
    """`data` plus hand-made [a, b, a, c, b]-shaped sessions: events whose target the session has shown are certain to occur."""
    ids = g.itemidmap.index.values
    rng = np.random.RandomState(3)
    rows = []
    for s in range(6):
        a, b, c = ids[rng.choice(len(ids), size=3, replace=False)]
        rows += [(5 + s, x, 10 ** 6 + 10 * s + j) for j, x in enumerate([a, b, a, c, b])]
    extra = pd.DataFrame(rows, columns=['SessionId', 'ItemId', 'Time']).astype({'SessionId': np.int32, 'Time': np.int64})
    return pd.concat([data, extra], ignore_index=True)


def test_exclusions():
    g = fitted('elu-0.5')
    data = with_repeats(g, make_test_set(g, n_sessions=60, seed=21, max_len=12))
    ids = g.itemidmap.index.values
    plain = evaluation.loglik_gpu(g, data, batch_size=BATCH)
    assert plain['eligible'].all()
    hists, _ = prefixes(data, plain['row'])
    shown = np.array([t in set(h.tolist()) for h, t in zip(hists, plain['target'])])
    fresh = plain['target'][~shown]
    banned = np.unique(np.r_[fresh[::9], ids[[0, 31, 32, 1002]]])       # some targets, both ends of the catalogue and of a tile
    z_t = score_targets(g, hists, plain['target'])
    res = evaluation.loglik_gpu(g, data, temperature=0.5, exclude_seen=True, exclude=banned, batch_size=BATCH)
    check_prefix_loop(g, data, res, 0.5, exclude_seen=True, exclude=banned, z_t=z_t)
    out = ~res['eligible']
    assert (out & shown).any() and (out & ~shown).any() and (out == (shown | np.isin(res['target'], banned))).all()
    assert res['eligible'].any()
    assert (res['logprob'][out] == -np.inf).all() and np.isfinite(res['target_logit'][out]).all()
    # candidates that name one id twice (both positions count, or both go) and lack some targets
    rng = np.random.RandomState(4)
    items = rng.permutation(ids)[:600]
    items = np.r_[items, items[17:18], items[300:301]]
    res = evaluation.loglik_gpu(g, data, items=items, temperature=0.5, exclude_seen=True, exclude=banned, batch_size=BATCH)
    check_prefix_loop(g, data, res, 0.5, items=items, exclude_seen=True, exclude=banned, z_t=z_t)
    assert (~np.isin(res['target'], items) & ~shown & ~np.isin(res['target'], banned)).any()
    assert (res['logprob'][~np.isin(res['target'], items)] == -np.inf).all()


# ---- 4. two row blocks, several tiles per range ----------------------------------------------------------------------------------
def test_row_blocks_and_several_tiles_per_range():
    g = big_model()
    data = make_test_set(g, n_sessions=130, seed=41, max_len=12)
    a = evaluation.loglik_gpu(g, data, temperature=0.5, exclude_seen=True, batch_size=130)
    b = evaluation.loglik_gpu(g, data, temperature=0.5, exclude_seen=True, batch_size=7)
    same(a, b)
    hists, _ = prefixes(data, a['row'])
    pick = np.random.RandomState(42).choice(len(hists), size=64, replace=False)
    z_t = score_targets(g, [hists[i] for i in pick], a['target'][pick])
    check_prefix_loop(g, data, a, 0.5, exclude_seen=True, pick=pick, z_t=z_t)


# ---- 5. pieces and batch sizes change nothing ------------------------------------------------------------------------------------
def test_pieces_and_batch_sizes(monkeypatch):
    g = fitted('elu-0.5')
    data = make_test_set(g, n_sessions=60, seed=51, max_len=12)
    ids = g.itemidmap.index.values
    kw = dict(temperature=0.5, exclude_seen=True, exclude=ids[:40])
    one = evaluation.loglik_gpu(g, data, batch_size=BATCH, **kw)
    assert g._ensure_model().events_launches()[3] == 1
    same(one, evaluation.loglik_gpu(g, data, **kw))                    # batch_size=None: min(512, the sessions)
    monkeypatch.setenv('G4R_EVENTS_PIECE', '256')
    for batch in (BATCH, 7, 60):
        res = evaluation.loglik_gpu(g, data, batch_size=batch, **kw)
        steps, scans, _, pieces = g._ensure_model().events_launches()
        assert pieces > 3 and scans == 2 * steps
        same(one, res)


# ---- 6. sample_sessions' own log-probabilities -----------------------------------------------------------------------------------
def test_agrees_with_sample_sessions():
    g = fitted()
    hists = histories(g, LENS, seed=61)
    steps, S = 4, 2
    items, scores, lp = g.sample_sessions(hists, steps, samples=S, temperature=0.5, no_repeat=True, return_logprobs=True)
    full = [list(h) + list(items[i, j]) for i, h in enumerate(hists) for j in range(S)]
    got, offs, det = g.session_log_likelihood(full, temperature=0.5, exclude_seen=True, return_details=True)
    at = np.array([[offs[i * S + j] + len(h) - 1 + s for s in range(steps)] for i, h in enumerate(hists) for j in range(S)])
    assert det['eligible'][at].all()
    np.testing.assert_array_equal(det['target'][at].reshape(items.shape), items)
    assert_bits(det['target_logit'][at].reshape(scores.shape), scores)
    err = np.abs(got[at].reshape(lp.shape).astype(np.float64) - lp.astype(np.float64))
    print('largest |logprob - sample_sessions| / ulp = %.3f' % (err / ulp32(lp)).max())
    assert (err <= ulp32(lp)).all(), 'more than 1 ulp from sample_sessions: largest difference %.3g' % err.max()


# ---- 7. the list form ------------------------------------------------------------------------------------------------------------
def test_session_log_likelihood_equals_loglik_gpu():
    g = fitted('elu-0.5')
    ids = g.itemidmap.index.values
    hists = histories(g, [5, 1, 2, 9, 3, 12, 2], seed=71, pool=ids[:40])
    table = pd.DataFrame({'SessionId': np.repeat(np.arange(len(hists)), [len(h) for h in hists]).astype(np.int32),
                          'ItemId': np.concatenate(hists), 'Time': np.arange(sum(len(h) for h in hists), dtype=np.int64)})
    table = table[table.SessionId != 1]                                 # (the one-item session scores nothing)
    for kw in (dict(), dict(temperature=0.5, exclude_seen=True, exclude=ids[3:6])):
        want = evaluation.loglik_gpu(g, table, **kw)
        g.predict = 'sentinel'
        lp, offs = g.session_log_likelihood(hists, **kw)
        assert g.predict is None
        assert lp.dtype == np.float32 and offs.dtype == np.int64
        np.testing.assert_array_equal(offs, np.r_[0, np.cumsum([len(h) - 1 for h in hists])])
        assert_bits(lp, want['logprob'])
        det = g.session_log_likelihood(hists, return_details=True, **kw)[2]
        np.testing.assert_array_equal(det['session'], want['session'])
        np.testing.assert_array_equal(det['target'], want['target'])
        np.testing.assert_array_equal(det['Q'], want['Q'])
    assert not want['eligible'].all() and want['eligible'].any()
    # a refused call launches nothing
    before = g._ensure_model().events_launches()
    own = pd.unique(hists[5][:-1])                                      # all shown by the session's last INPUT event
    with pytest.raises(ValueError, match='session 5'):
        g.session_log_likelihood(hists, predict_for_item_ids=own, exclude_seen=True)
    with pytest.raises(ValueError, match='eligible'):
        g.session_log_likelihood(hists, predict_for_item_ids=ids[:10], exclude=ids[:10])
    with pytest.raises(KeyError):
        g.session_log_likelihood([[ids[0], -5]])
    assert g._ensure_model().events_launches() == before


# ---- 8. the command line ---------------------------------------------------------------------------------------------------------
def test_cli_prints_the_metrics(tmp_path):
    data = synth.make_sessions(6000, n_items=300, seed=8)              # > 512 test sessions: run.py evaluates with batch_size=512
    train, test = synth.train_test_split(data, test_frac=0.1)
    paths = [str(tmp_path / 'train.tsv'), str(tmp_path / 'test.tsv'), str(tmp_path / 'model.pickle')]
    train.to_csv(paths[0], sep='\t', index=False)
    test.to_csv(paths[1], sep='\t', index=False)
    ps = 'loss=bpr-max,final_act=elu-0.5,layers=32,batch_size=32,n_sample=256,constrained_embedding=True,learning_rate=0.1,n_epochs=1'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'run.py'), paths[0], '-ps', ps, '-ss', str(256 * 64), '-s', paths[2], '-t', paths[1],
                        '--loglik', '--loglik_temperature', '0.5'], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    at = [i for i, ln in enumerate(lines) if ln.startswith('NLL: ')]
    assert len(at) == 1 and lines[at[0] - 1].startswith('Recall@20')
    hit = re.fullmatch(r'NLL: ([0-9.]+) Perplexity: ([0-9.]+) Events: (\d+) Ineligible: (\d+)', lines[at[0]])
    assert hit, lines[at[0]]
    g = GRU4Rec.loadmodel(paths[2])
    events = pd.read_csv(paths[1], sep='\t', dtype={'SessionId': 'int32', 'ItemId': 'str'})
    m = evaluation.loglik_metrics(evaluation.loglik_gpu(g, events, temperature=0.5))
    assert hit.groups() == ('%.6f' % m['nll'], '%.6f' % m['perplexity'], str(m['n']), str(m['n_ineligible']))
    assert m['n'] > 1000 and m['n_ineligible'] == 0 and m['nll'] > 0 and np.isfinite(m['perplexity'])

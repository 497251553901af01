"""Recall@N / MRR@N on the device: same signature and results as the reference's
`evaluation.evaluate_gpu` (evaluation.py:15-147), without the Theano graph.

`evaluate_gpu` hands the whole test loop to the device in ONE call (`g4r_evaluate`): the session-parallel schedule
of evaluation.py:96-139 is the schedule of `fit` (same author, same loop), so the C++ plan builder produces it; every
step runs the GRU forward, scores all / the given items (final activation applied in fp32 as the reference does), ranks
the targets with the > / >= / == counts of :62-65 (mode 'tiebreaking': scores + uniform * 1e-10 in fp32 first, :55, from a Philox
stream keyed by the model seed, evaluation step, row and candidate column) and adds the hits and reciprocal ranks of every cut-off into device
accumulators; hidden rows of finished sessions are zeroed / dropped on the device.  `evaluate_gpu_stepwise` is the
host-driven variant (one `g4r_predict_step` + `g4r_rank_targets` per step), kept as a cross-check.

Not in the reference: `recommend_gpu` runs the same loop (`g4r_recommend_events`) and returns, for every scored event, its top-k
list, the rank of its target and the target's score; `list_metrics` turns that into recall, MRR, NDCG and item coverage.
`loglik_gpu` runs it once more (`g4r_loglik_events`) for the log-probability the model gives to the item that actually came next at
every event -- sample_sessions' distribution, its exact integer normaliser formed on the device -- and `loglik_metrics` turns that
into the held-out negative log-likelihood, the perplexity and per-session sequence likelihoods.
"""
import numpy as np
import pandas as pd


def _prepare_categorical(gru, test_data, items, session_key, item_key, time_key, want_sessions=False):
    """_prepare for tables from eventio.read_events: the inner join on the item id, the (session, time, item id) ordering and
    the session sizes of evaluation.py:86-95 as linear passes over integer arrays."""
    from . import datatools, eventio
    col = test_data[item_key]
    idx = eventio.lookup_item_index(col, gru.itemidmap)
    keep = idx >= 0                                   # how='inner': events of items the model does not know are dropped
    sess, tm = test_data[session_key].values[keep], test_data[time_key].values[keep]
    idx, codes = idx[keep], np.asarray(col.cat.codes.values)[keep]
    n = len(idx)
    ordered = n < 2 or bool(np.all((sess[1:] > sess[:-1]) | ((sess[1:] == sess[:-1]) & (tm[1:] > tm[:-1]))))
    if not ordered:
        # ties on (session, time) are broken by the item id *string*, as sort_values on a str column does
        cats = np.asarray(col.cat.categories.values, dtype=object).astype(str)
        lex = np.empty(len(cats), dtype=np.int64)
        lex[np.argsort(cats, kind='stable')] = np.arange(len(cats))
        order = np.lexsort((lex[codes], tm, sess))
        sess, idx = sess[order], idx[order]
    item_idxs = None if items is None else gru.itemidmap[items].values.astype(np.int32)
    offs = datatools.compute_offset(pd.DataFrame({session_key: sess}, copy=False), session_key).astype(np.int64)
    if want_sessions:
        return idx.astype(np.int32), item_idxs, offs, sess
    return idx.astype(np.int32), item_idxs, offs


def _prepare(gru, test_data, items, session_key, item_key, time_key, want_sessions=False):
    """(item index of every event of the sorted test table, candidate item indices or None, session offsets); want_sessions: + the
    session id of every event."""
    if isinstance(test_data[item_key].dtype, pd.CategoricalDtype):
        return _prepare_categorical(gru, test_data, items, session_key, item_key, time_key, want_sessions)
    lookup = pd.DataFrame({'ItemIdx': gru.itemidmap.values, item_key: gru.itemidmap.index})
    test_data = pd.merge(test_data, lookup, on=item_key, how='inner')
    test_data.sort_values([session_key, time_key, item_key], inplace=True)
    titems = test_data.ItemIdx.values.astype(np.int32)
    item_idxs = None if items is None else gru.itemidmap[items].values.astype(np.int32)
    sizes = test_data.groupby(session_key).size().values
    offs = np.zeros(len(sizes) + 1, dtype=np.int64)
    offs[1:] = np.cumsum(sizes)
    if want_sessions:
        return titems, item_idxs, offs, test_data[session_key].values
    return titems, item_idxs, offs


def evaluate_gpu(gru, test_data, items=None, session_key='SessionId', item_key='ItemId', time_key='Time',
                 cut_off=[20], batch_size=100, mode='standard'):
    """Returns (recall list, mrr list) -- one entry per cut-off, like the reference.  One device call for the whole test."""
    from . import _native
    if gru.error_during_train:
        raise Exception
    if mode not in ('standard', 'conservative', 'median', 'tiebreaking'):
        raise NotImplementedError
    multi = isinstance(cut_off, (list, tuple))
    cuts = list(cut_off) if multi else [cut_off]
    print('Measuring Recall@{} and MRR@{}'.format(','.join(str(c) for c in cuts), ','.join(str(c) for c in cuts)))
    model = gru._ensure_model()
    titems, item_idxs, offs = _prepare(gru, test_data, items, session_key, item_key, time_key)
    n_sessions = len(offs) - 1
    if n_sessions < batch_size:
        raise IndexError('fewer test sessions ({}) than batch_size ({})'.format(n_sessions, batch_size))
    # sessions in id order (evaluation.py:90-95); n_sample = 1 selects "run until no session is left" (:124-127)
    plan = _native.build_plan(offs.astype(np.int32), np.arange(n_sessions), titems, batch_size, 1)
    rec, mrr, n = model.evaluate(plan, batch_size, item_idxs, cuts, mode)
    # the evaluation used the model's prediction state; predict_next_batch starts afresh afterwards (the reference's
    # evaluate_gpu keeps an H of its own, evaluation.py:54)
    gru.predict = None
    return (rec / n).tolist(), (mrr / n).tolist()


def evaluate_gpu_stepwise(gru, test_data, items=None, session_key='SessionId', item_key='ItemId', time_key='Time',
                          cut_off=[20], batch_size=100, mode='standard'):
    """Host-driven variant of evaluate_gpu: the loop of evaluation.py:96-139 in Python, one device step at a time."""
    if gru.error_during_train:
        raise Exception
    if mode not in ('standard', 'conservative', 'median', 'tiebreaking'):
        raise NotImplementedError
    multi = isinstance(cut_off, (list, tuple))
    cuts = list(cut_off) if multi else [cut_off]
    print('Measuring Recall@{} and MRR@{}'.format(','.join(str(c) for c in cuts), ','.join(str(c) for c in cuts)))
    model = gru._ensure_model()
    lookup = pd.DataFrame({'ItemIdx': gru.itemidmap.values, item_key: gru.itemidmap.index})
    test_data = pd.merge(test_data, lookup, on=item_key, how='inner')
    test_data.sort_values([session_key, time_key, item_key], inplace=True)
    titems = test_data.ItemIdx.values.astype(np.int32)
    item_idxs = None if items is None else gru.itemidmap[items].values.astype(np.int32)
    sizes = test_data.groupby(session_key).size().values
    n_sessions = len(sizes)
    offs = np.zeros(n_sessions + 1, dtype=np.int64)
    offs[1:] = np.cumsum(sizes)
    if n_sessions < batch_size:
        raise IndexError('fewer test sessions ({}) than batch_size ({})'.format(n_sessions, batch_size))
    rec = np.zeros(len(cuts))
    mrr = np.zeros(len(cuts))
    n = 0
    model.predict_begin(batch_size)
    slot = np.arange(batch_size)
    next_free = batch_size - 1
    first = offs[slot].copy()
    last = offs[slot + 1].copy()
    while True:
        run = int((last - first).min())
        for i in range(run - 1):
            cur_in = titems[first + i]
            cur_out = titems[first + i + 1]
            m = len(slot)
            if item_idxs is None:
                model.predict_step(cur_in, None, want_scores=False)
                ranks = model.rank_targets(cur_out, 0, mode)
            else:
                model.predict_step(cur_in, np.concatenate([cur_out, item_idxs]), want_scores=False)
                ranks = model.rank_targets(np.arange(m, dtype=np.int32), m, mode)
            for j, c in enumerate(cuts):
                hit = ranks <= c
                rec[j] += hit.sum()
                mrr[j] += (hit / ranks).sum()
            n += m
        first = first + run - 1
        done = (last - first) <= 1
        n_done = int(done.sum())
        slot[done] = next_free + 1 + np.arange(n_done)
        next_free += n_done
        valid = slot < n_sessions
        if not valid.any():
            break
        refill = done & valid
        first[refill] = offs[slot[refill]]
        last[refill] = offs[slot[refill] + 1]
        # hidden rows of restarted slots are zeroed, rows of exhausted slots dropped (evaluation.py:134-139)
        keep = np.nonzero(valid)[0].astype(np.int32)
        model.predict_hidden(zero_mask=refill.astype(np.uint8) if len(refill) == batch_size else
                             np.pad(refill.astype(np.uint8), (0, batch_size - len(refill))),
                             keep_rows=keep if len(keep) < len(valid) else None)
        slot, first, last = slot[valid], first[valid], last[valid]
    gru.predict = None      # see evaluate_gpu
    rec = (rec / n).tolist()
    mrr = (mrr / n).tolist()
    return rec, mrr


# ---------------------------------------------------------------------------------------------- per-event lists (not in the reference)
def slot_map(offs, batch_size):
    """(plan, rows): the evaluation plan of sessions with offsets `offs` and, for every (step, row) of it, the row of the sorted
    test table that is the step's INPUT event (-1 for padding).  The plan builder run on arange(n_rows) in place of the item
    indices returns exactly that as its in_idx."""
    from . import _native
    offs = np.asarray(offs, dtype=np.int64)
    n_sessions, n_rows = len(offs) - 1, int(offs[-1])
    rows = _native.build_plan(offs.astype(np.int32), np.arange(n_sessions), np.arange(n_rows, dtype=np.int32), batch_size, 1)
    T = rows['T']
    table = rows['in_idx'].astype(np.int64).reshape(T, batch_size)
    table[np.arange(batch_size)[None, :] >= rows['M'][:T, None]] = -1
    return rows, table


def seen_tables(titems, offs):
    """The seen-item tables of g4r_recommend_events, linear in the number of events: per session the sorted distinct item indices
    and, beside each, the position in the session of its first occurrence.  Returns dict(offs int64[n_sessions + 1], items int32,
    first int32)."""
    titems = np.asarray(titems, dtype=np.int64)
    offs = np.asarray(offs, dtype=np.int64)
    n_sessions = len(offs) - 1
    sess = np.repeat(np.arange(n_sessions), np.diff(offs))
    pos = np.arange(len(titems)) - offs[sess]
    order = np.lexsort((pos, titems, sess))          # by session, then item, then position: the first of every (session, item) run
    s, it, p = sess[order], titems[order], pos[order]
    head = np.ones(len(order), dtype=bool)
    head[1:] = (s[1:] != s[:-1]) | (it[1:] != it[:-1])
    counts = np.bincount(s[head], minlength=n_sessions)
    return dict(offs=np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), items=it[head].astype(np.int32),
                first=p[head].astype(np.int32))


def _events_inputs(gru, titems, offs, sess_ids, batch_size, exclude_seen, exclude):
    """What recommend_gpu and loglik_gpu hand to the device besides the candidates: (device model, plan, slot int64[T, batch], rows =
    the scored events' rows of the sorted table, exclusion mask or None, seen tables or None, the session id of every session)."""
    from . import _native
    n_sessions = len(offs) - 1
    if n_sessions < batch_size:
        raise IndexError('fewer test sessions ({}) than batch_size ({})'.format(n_sessions, batch_size))
    mask = None
    if exclude is not None:
        ex = exclude if isinstance(exclude, np.ndarray) else list(exclude)
        if len(ex):
            gidx = np.unique(gru.itemidmap[np.ravel(ex)].values.astype(np.int64))
            mask = np.zeros((len(gru.itemidmap) + 31) // 32, dtype=np.uint32)
            np.bitwise_or.at(mask, gidx >> 5, np.left_shift(1, gidx & 31).astype(np.uint32))
    first_sess = sess_ids[offs[:-1]] if n_sessions else np.zeros(0)
    seen = None
    if exclude_seen:
        seen = seen_tables(titems, offs)
        big = np.flatnonzero(np.diff(seen['offs']) > _native.G4R_EXCLUDE_MAX)
        if len(big):
            raise ValueError('exclude_seen: session %s holds %d distinct items, more than G4R_EXCLUDE_MAX = %d'
                             % (first_sess[big[0]], np.diff(seen['offs'])[big[0]], _native.G4R_EXCLUDE_MAX))
    model = gru._ensure_model()
    plan = _native.build_plan(offs.astype(np.int32), np.arange(n_sessions), titems, batch_size, 1)
    _, table = slot_map(offs, batch_size)
    # scored events in table order: every row with a successor in its session; slot = its number among them
    has_next = np.ones(len(titems), dtype=bool)
    has_next[offs[1:] - 1] = False
    rows = np.flatnonzero(has_next)
    number = np.full(len(titems) + 1, -1, dtype=np.int64)
    number[rows] = np.arange(len(rows))
    slot = number[table]                       # (table == -1 reads the spare last entry: -1)
    if seen is not None:
        row_sess = np.repeat(np.arange(n_sessions), np.diff(offs))
        safe = np.maximum(table, 0)
        seen['sess'] = row_sess[safe].astype(np.int32)
        seen['pos'] = (safe - offs[row_sess[safe]]).astype(np.int32)
    return model, plan, slot, rows, mask, seen, first_sess


def _events_refusal(e, first_sess):
    """The device call's refusals that are the caller's doing, as ValueError (the session by its id); anything else returns."""
    import re
    hit = re.search(r'session (\d+) has', str(e))
    if hit:
        raise ValueError('session %s: %s' % (first_sess[int(hit.group(1))], e)) from None
    if 'eligible candidate positions' in str(e):
        raise ValueError(str(e)) from None


def recommend_gpu(gru, test_data, k=20, items=None, session_key='SessionId', item_key='ItemId', time_key='Time', batch_size=100,
                  mode='standard', exclude_seen=False, exclude=None):
    """The top-k list and the target's rank at EVERY event of a test set, in one device call (g4r_recommend_events): the loop of
    evaluate_gpu -- same preparation, same plan, same ranks -- that keeps what evaluate_gpu folds into two sums.

    Returns a dict of NumPy arrays with one entry per scored event (every event of the sorted test table that has a successor in
    its session), in the order of that table:
      row           index of the input event in the sorted test table (events of unknown items dropped, sorted by session, time, item)
      session       its session id
      target        item id of the next event of the session
      rank          the target's rank among the candidates (`mode` as in evaluate_gpu): sum(rank <= c) / n is evaluate_gpu's recall@c
      target_score  the target's score
      items         [n, k] item ids, best first: what recommend_sessions returns for the session's prefix up to the input event
      scores        [n, k] float32, predict_next_batch's bit patterns
    items: candidate item ids (default: all); the list is chosen among them, the rank counts them (the target itself is ranked
    whether listed or not, as in evaluate_gpu).  exclude_seen: an event's list leaves out the items its session has shown up to and
    including the input event (recommend_sessions' exclude_history); exclude: item ids left out of every list.  Exclusions never
    change `rank`.  A session with more than G4R_EXCLUDE_MAX distinct items, or exclusions that leave fewer than k candidates at
    some event, raise ValueError naming the session before anything runs."""
    from . import _native
    if gru.error_during_train:
        raise Exception
    if mode not in ('standard', 'conservative', 'median', 'tiebreaking'):
        raise NotImplementedError
    n_sel = len(gru.itemidmap) if items is None else len(items)
    if isinstance(k, bool) or int(k) != k or not 1 <= k <= min(n_sel, _native.G4R_TOPK_MAX):
        raise ValueError('k = %r: it must be an integer in [1, min(number of candidates = %d, %d)]' % (k, n_sel, _native.G4R_TOPK_MAX))
    k = int(k)
    if isinstance(batch_size, bool) or int(batch_size) != batch_size or batch_size < 1:
        raise ValueError('batch_size = %r: it must be a positive integer' % (batch_size,))
    titems, item_idxs, offs, sess_ids = _prepare(gru, test_data, items, session_key, item_key, time_key, want_sessions=True)
    model, plan, slot, rows, mask, seen, first_sess = _events_inputs(gru, titems, offs, sess_ids, batch_size, exclude_seen, exclude)
    try:
        li, ls, rank, ts = model.recommend_events(plan, batch_size, item_idxs, mode, slot, len(rows), k, mask, seen)
    except _native.NativeError as e:
        _events_refusal(e, first_sess)
        raise
    finally:
        gru.predict = None      # the call used the model's prediction state (see evaluate_gpu)
    ids = gru.itemidmap.index.values
    return dict(row=rows, session=np.asarray(sess_ids)[rows], target=ids[titems[rows + 1]], rank=rank, target_score=ts,
                items=ids[li], scores=ls)


def list_metrics(result, cut_off=[5, 10, 20], n_items=None):
    """Metrics of a recommend_gpu result, per cut-off: dict(recall, mrr, ndcg, coverage), each a list with one entry per cut-off.
    recall / mrr are evaluate_gpu's (from `rank`); ndcg = mean of 1 / log2(1 + rank) over the events with rank <= cut (one
    relevant item per event: the ideal DCG is 1); coverage = distinct items in the first `cut` columns of `items` / n_items
    (None without n_items).  A cut-off above the list length k is refused for coverage only when n_items is given."""
    cuts = list(cut_off) if isinstance(cut_off, (list, tuple, np.ndarray)) else [cut_off]
    rank = np.asarray(result['rank'], dtype=np.float64)
    n = max(len(rank), 1)
    out = dict(recall=[], mrr=[], ndcg=[], coverage=[])
    for c in cuts:
        hit = rank <= c
        out['recall'].append(float(hit.sum()) / n)
        out['mrr'].append(float((1.0 / rank[hit]).sum()) / n)
        out['ndcg'].append(float((1.0 / np.log2(1.0 + rank[hit])).sum()) / n)
        if n_items is None:
            out['coverage'].append(None)
        else:
            lists = np.asarray(result['items'])
            if c > lists.shape[1]:
                raise ValueError('coverage at cut-off %d needs lists of at least that length (k = %d)' % (c, lists.shape[1]))
            out['coverage'].append(len(np.unique(lists[:, :c])) / float(n_items))
    return out


# ---------------------------------------------------------------------------------------------- per-event log-likelihood (not in the reference)
def _loglik_events(gru, titems, item_idxs, offs, sess_ids, batch_size, t32, exclude_seen, exclude):
    """loglik_gpu behind its preparation (GRU4Rec.session_log_likelihood enters here): one g4r_loglik_events call, then the two
    float64 formulas of the contract in NumPy."""
    from . import _native
    model, plan, slot, rows, mask, seen, first_sess = _events_inputs(gru, titems, offs, sess_ids, batch_size, exclude_seen, exclude)
    try:
        z, zeta, Q, eligible = model.loglik_events(plan, batch_size, item_idxs, slot, len(rows), float(t32), mask, seen)
    except _native.NativeError as e:
        _events_refusal(e, first_sess)
        raise
    finally:
        gru.predict = None      # the call used the model's prediction state (see evaluate_gpu)
    inv_t = np.float32(1) / t32
    with np.errstate(all='ignore'):
        logq = np.log(Q.astype(np.float64) * 2.0 ** -39)
        lse = (zeta.astype(np.float64) * np.float64(inv_t) + logq).astype(np.float32)
        d = ((z - zeta).astype(np.float32) * inv_t).astype(np.float32)
        logprob = np.where(eligible, (d.astype(np.float64) - logq).astype(np.float32), np.float32(-np.inf)).astype(np.float32)
    ids = gru.itemidmap.index.values
    return dict(row=rows, session=np.asarray(sess_ids)[rows], target=ids[titems[rows + 1]], logprob=logprob, lse=lse, target_logit=z,
                zeta=zeta, Q=Q, eligible=eligible)


def loglik_gpu(gru, test_data, items=None, temperature=1.0, exclude_seen=False, exclude=None, session_key='SessionId', item_key='ItemId',
               time_key='Time', batch_size=None):
    """The log-probability the model gives to the item that actually came next, at EVERY event of a test set, in one device call
    (g4r_loglik_events): held-out negative log-likelihood / perplexity (loglik_metrics), the target-policy propensity
    pi(logged item | prefix) of off-policy evaluation, per-session sequence likelihoods.  Same preparation, plan and seen tables as
    recommend_gpu, and the distribution is sample_sessions': softmax(z / temperature) over the event's eligible candidate positions.

    Returns a dict of NumPy arrays with one entry per scored event, in the order of the sorted test table; row / session / target
    are recommend_gpu's, so the two results join on `row`:
      logprob       float32: fl32(d_t - log(Q * 2^-39)) in float64, d_t = fl32(fl32(z_t - zeta) / temperature); -inf when the target
                    holds no eligible position
      lse           float32: fl32(zeta / temperature + log(Q * 2^-39)), session_log_partition's bits for the session's prefix
      target_logit  float32 z_t: the target's predict_next_batch score, the pre-activation value for final_act softmax / softmax_logit
                    (reported for ineligible targets too)
      zeta, Q       the largest eligible z of the event and the exact integer normaliser (uint64), as sample_sessions defines them
      eligible      bool: the target holds an eligible position
    Eligible positions of an event: all items, or the positions of `items` (a duplicate id counts once per position), minus
    `exclude`, minus -- exclude_seen -- the items its session has shown up to and including the input event: the positions
    recommend_gpu's list may hold under the same arguments.  Every value is a function of exact device outputs, so it does not depend
    on batch_size (None: min(512, number of sessions)).  An unknown id raises KeyError; a session with more than G4R_EXCLUDE_MAX
    distinct items, or an event left without an eligible position, ValueError naming the session; more than 2^24 candidate positions
    or a bad temperature ValueError; fewer sessions than an explicit batch_size IndexError -- all before anything runs."""
    from .gru4rec import _check_lse_candidates, _check_temperature
    if gru.error_during_train:
        raise Exception
    t32 = _check_temperature(temperature)
    if batch_size is not None and (isinstance(batch_size, bool) or int(batch_size) != batch_size or batch_size < 1):
        raise ValueError('batch_size = %r: it must be a positive integer or None' % (batch_size,))
    n_sel = len(gru.itemidmap) if items is None else len(items)
    if n_sel < 1:
        raise ValueError('items is empty: at least one candidate is needed')
    _check_lse_candidates(n_sel)
    titems, item_idxs, offs, sess_ids = _prepare(gru, test_data, items, session_key, item_key, time_key, want_sessions=True)
    if batch_size is None:
        batch_size = max(1, min(512, len(offs) - 1))
    return _loglik_events(gru, titems, item_idxs, offs, sess_ids, int(batch_size), t32, exclude_seen, exclude)


def loglik_metrics(result):
    """Metrics of a loglik_gpu result: dict(n = scored events, n_ineligible = those whose target held no eligible position, nll = the
    float64 mean of -logprob over the eligible events, perplexity = exp(nll), sessions = the distinct session ids, session_logprob =
    the float64 sum of logprob over every session's eligible events, session_events = their number).  nll and perplexity are nan
    when no event is eligible."""
    lp = np.asarray(result['logprob'], dtype=np.float64)
    ok = np.asarray(result['eligible'], dtype=bool)
    n_ok = int(ok.sum())
    nll = float(-lp[ok].sum() / n_ok) if n_ok else float('nan')
    sessions, inv = np.unique(np.asarray(result['session']), return_inverse=True)
    inv = np.ravel(inv)
    return dict(n=len(lp), n_ineligible=len(lp) - n_ok, nll=nll, perplexity=float(np.exp(nll)), sessions=sessions,
                session_logprob=np.bincount(inv[ok], weights=lp[ok], minlength=len(sessions)).astype(np.float64),
                session_events=np.bincount(inv[ok], minlength=len(sessions)).astype(np.int64))

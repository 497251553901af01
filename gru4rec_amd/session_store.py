"""The device-resident session store behind GRU4Rec.open_session_store (not in the reference): every live session's hidden state and
seen items stay on the device between calls (g4r_store_*, include/gru4rec_hip.h), so a serving process pushes one new click and asks
"what next?" without replaying the history or carrying the state.  The device side is slot-level; this module keeps the map from
session id to slot and the eviction rule, and packs the arguments -- one packer per argument family, as gru4rec.py's front end:
pack_events (the events of a call as CSR rows), SlotMap (ids, slots, least-recently-touched eviction), SessionStore._selection (the
selection arguments and their refusals)."""
import heapq
from collections import OrderedDict

import numpy as np


def _id_list(session_ids):
    """Session ids as a list of hashables (NumPy scalars become Python ones, so 3 and np.int64(3) are the same session)."""
    if isinstance(session_ids, np.ndarray):
        return session_ids.tolist() if session_ids.ndim == 1 else [session_ids.tolist()] if session_ids.ndim == 0 else list(map(tuple, session_ids.tolist()))
    return [s.item() if isinstance(s, np.generic) else s for s in session_ids]


def pack_events(session_ids, item_idx):
    """The events of one push, taken in the given order, as CSR rows: (sessions, offsets int64[U + 1], item indices int32).  The U
    distinct sessions, in order of first appearance, are the rows; row u holds session u's events in their order."""
    sids = _id_list(session_ids)
    item_idx = np.ravel(np.asarray(item_idx, dtype=np.int32))
    if len(sids) != len(item_idx):
        raise ValueError('session_ids holds %d entries and item_ids %d: one item per event is needed' % (len(sids), len(item_idx)))
    if not sids:
        raise ValueError('a push needs at least one event')
    row_of, rows = {}, np.empty(len(sids), dtype=np.int64)
    for e, s in enumerate(sids):
        r = row_of.get(s)
        if r is None:
            r = row_of[s] = len(row_of)
        rows[e] = r
    order = np.argsort(rows, kind='stable')
    offs = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=len(row_of)))]).astype(np.int64)
    return list(row_of), offs, np.ascontiguousarray(item_idx[order])


class SlotMap:
    """Session id -> slot, with the eviction rule.  A session is touched by every call that names it (push, load); the order of
    touches is the order of the calls and, within a call, the order of its rows, so the rule is deterministic.  When a new session
    finds no free slot, the least-recently-touched session NOT in the current call gives up its slot.  Free slots are handed out
    lowest first: the slots given back by release() (a heap), then the slots never used."""

    def __init__(self, capacity):
        self.capacity = int(capacity)
        self.slot = OrderedDict()      # id -> slot, least recently touched first
        self.released = []             # heap of slots given back
        self.unused = 0                # slots [unused, capacity) were never handed out
        self.evictions = 0
        self.evicted = []

    def n_free(self):
        return len(self.released) + self.capacity - self.unused

    def plan(self, sessions):
        """What a call over these distinct sessions will do, computed without changing anything: (slots int32, fresh int32, evicted
        ids, number of released slots taken)."""
        if len(sessions) > self.capacity:
            raise ValueError('the call names %d distinct sessions, more than the store holds (capacity = %d)' % (len(sessions), self.capacity))
        n_new = sum(1 for s in sessions if s not in self.slot)
        short = n_new - self.n_free()
        evicted = []
        if short > 0:
            here = set(sessions)
            for s in self.slot:      # least recently touched first
                if s not in here:
                    evicted.append(s)
                    if len(evicted) == short:
                        break
        rel = heapq.nsmallest(min(n_new, len(self.released)), self.released)
        pool = iter(rel + list(range(self.unused, min(self.capacity, self.unused + n_new - len(rel)))) + [self.slot[s] for s in evicted])
        slots, fresh = [], []
        for s in sessions:
            known = s in self.slot
            slots.append(self.slot[s] if known else next(pool))
            fresh.append(0 if known else 1)
        return np.array(slots, dtype=np.int32), np.array(fresh, dtype=np.int32), evicted, len(rel)

    def commit(self, sessions, slots, evicted, n_released):
        """Makes a planned call happen in the map."""
        for s in evicted:
            del self.slot[s]
        self.evictions += len(evicted)
        self.evicted.extend(evicted)
        for _ in range(n_released):
            heapq.heappop(self.released)
        for s, sl in zip(sessions, slots):
            if s in self.slot:
                self.slot.move_to_end(s)
            else:
                self.slot[s] = int(sl)
                self.unused = max(self.unused, int(sl) + 1)

    def release(self, sessions):
        for s in sessions:
            heapq.heappush(self.released, self.slot.pop(s))


class SessionStore:
    """`capacity` slots in device memory, each holding one session's hidden state (all layers), its sorted, duplicate-free list of
    seen items (at most seen_cap) and an overflow flag.  Returned by GRU4Rec.open_session_store; bound to the device model it was
    opened on: fit, prepare, run_epoch, close or anything else that drops or retrains that model closes the store, and a closed
    store's calls raise RuntimeError -- states computed under old weights are never served.  Not pickled with the model."""

    def __init__(self, gru, model, capacity, seen_cap):
        self._g, self._m = gru, model
        self.capacity, self.seen_cap = int(capacity), int(seen_cap)
        self._map = SlotMap(capacity)
        self._closed = False
        self._bytes = 0

    # ------------------------------------------------------------------ state of the store itself
    def _live(self):
        if self._closed or self._g._model is not self._m or not getattr(self._m, 'h', None):
            self._closed = True
            raise RuntimeError('the session store is closed (close(), or the device model it was opened on was dropped or retrained: '
                               'fit / prepare / run_epoch / close); open a new one with open_session_store')
        if self._g.error_during_train:
            raise Exception
        return self._m

    def _invalidate(self):
        """The model's weights change or the model goes: the store closes, its device memory is freed where the model lives on."""
        if not self._closed:
            self._closed = True
            if getattr(self._m, 'h', None):
                self._m.store_close()
        if getattr(self._g, '_store', None) is self:
            self._g._store = None

    def close(self):
        """Frees the slots; every later call raises RuntimeError.  The model may open a new store afterwards."""
        self._invalidate()

    @property
    def closed(self):
        return self._closed or self._g._model is not self._m or not getattr(self._m, 'h', None)

    def __len__(self):
        return len(self._map.slot)

    def __contains__(self, session_id):
        return (session_id.item() if isinstance(session_id, np.generic) else session_id) in self._map.slot

    def stats(self):
        """dict(live: sessions held, capacity, seen_cap, evictions: sessions evicted so far, device_bytes: what the slots hold)."""
        return dict(live=len(self._map.slot), capacity=self.capacity, seen_cap=self.seen_cap, evictions=self._map.evictions,
                    device_bytes=self._bytes)

    def pop_evicted(self):
        """The ids evicted since this was last called, in eviction order."""
        out, self._map.evicted = self._map.evicted, []
        return out

    # ------------------------------------------------------------------ the selection arguments
    def _selection(self, k, exclude_seen, exclude, exclude_groups, predict_for_item_ids, scan, oversample):
        """Checks and packs the selection arguments of push / recommend, before any device work: (k, candidate indices or None, their
        ids, mask, oversample or None).  The refusals of recommend_sessions for k / scan / oversample / exclude; with exclude_seen the
        candidates must be duplicate-free (as no_repeat requires) and k + seen_cap + (globally excluded candidates) <= candidates."""
        g = self._g
        from .gru4rec import _check_k
        k = _check_k(k, g._n_candidates(predict_for_item_ids), bools=True)
        over = g._scan_oversample(scan, oversample, k)
        iidx, cand = g._candidates(predict_for_item_ids)
        mask = None
        if exclude is not None or exclude_groups is not None:      # (one row stands for all: nothing here is per row)
            _, _, mask = g._pack_exclusions(1, k, iidx, None, '', exclude, None, exclude_groups=exclude_groups)
        if exclude_seen:
            if self.seen_cap == 0:
                raise ValueError('exclude_seen=True needs seen lists: the store was opened with seen_cap = 0')
            if iidx is not None and len(np.unique(iidx)) != len(iidx):
                raise ValueError('exclude_seen needs duplicate-free predict_for_item_ids: every seen item must take exactly one candidate '
                                 'position')
            gidx, _ = g._global_exclude(exclude, exclude_groups)
            n_cand = len(g.itemidmap) if iidx is None else len(iidx)
            n_masked = len(gidx) if iidx is None else int(np.isin(iidx, gidx).sum())
            if k + self.seen_cap + n_masked > n_cand:
                raise ValueError('k = %d with exclude_seen needs k + seen_cap + globally excluded candidates <= candidates (%d + %d + %d > %d): '
                                 'the seen lists live on the device, so this bound is conservative -- every list counts as full'
                                 % (k, k, self.seen_cap, n_masked, n_cand))
        return k, iidx, cand, mask, over

    # ------------------------------------------------------------------ push / recommend
    def push(self, session_ids, item_ids, k=None, exclude_seen=False, exclude=None, exclude_groups=None, predict_for_item_ids=None,
             scan='fp32', oversample=8):
        """Pushes (session id, item id) events, taken in the given order; any number of events per session.  The distinct sessions, in
        order of first appearance, are the rows of the call: U rows.  Every row's events advance its stored state -- from zero for a
        session the store does not hold -- and its distinct items are merged into its seen list (the first seen_cap distinct items of
        the session in event order; a session that shows more gets its overflow flag set).

        k=None: nothing is selected; returns sessions[U].  Otherwise (sessions[U], item_ids[U, k], scores[U, k] float32,
        seen_overflow[U] bool), computed after each session's last event: row u equals, ids and score bits,
        recommend_sessions(<all events of the session since it entered the store>, k, ...) with the same predict_for_item_ids /
        exclude / exclude_groups / scan / oversample.  exclude_seen: the stored list, this call's inputs included, is excluded
        (recommend_next_batch's exclude_seen rule; with seen_overflow[u] the list no longer holds everything the session saw).

        When a new session finds no free slot, the least-recently-touched session not in this call is evicted (pop_evicted());
        touches count calls, not time.  An evicted session that comes back is a new session.  Everything is checked before any
        device work and before the id map changes: an unknown item raises KeyError; a bad k / scan / oversample, more distinct
        sessions than capacity, exclude_seen with seen_cap = 0, with duplicate candidates or with k + seen_cap + globally excluded
        candidates > candidates (a conservative bound) raise ValueError.  The prediction state is neither read nor changed."""
        m = self._live()
        sel = None
        if k is not None:
            sel = self._selection(k, exclude_seen, exclude, exclude_groups, predict_for_item_ids, scan, oversample)
        idx = self._g.itemidmap[np.ravel(item_ids) if isinstance(item_ids, np.ndarray) else list(item_ids)].values
        sessions, offs, ev = pack_events(session_ids, idx)
        slots, fresh, evicted, nrel = self._map.plan(sessions)
        if sel is None:
            m.store_push(offs, ev, slots, fresh)
            self._map.commit(sessions, slots, evicted, nrel)
            return sessions
        k, iidx, cand, mask, over = sel
        cols, scores, flags = m.store_push(offs, ev, slots, fresh, iidx, k, exclude_seen, mask, over)
        self._map.commit(sessions, slots, evicted, nrel)
        return sessions, cand[cols], scores, flags.astype(bool)

    def recommend(self, session_ids, k=20, exclude_seen=False, exclude=None, exclude_groups=None, predict_for_item_ids=None, scan='fp32',
                  oversample=8):
        """The top-k of stored sessions from their stored state: (item_ids[n, k], scores[n, k], seen_overflow[n]), what the session's
        last push would have returned with these arguments.  Nothing advances, nothing changes, no session is touched.  The session
        ids must be distinct; an unknown one raises KeyError."""
        m = self._live()
        k, iidx, cand, mask, over = self._selection(k, exclude_seen, exclude, exclude_groups, predict_for_item_ids, scan, oversample)
        slots = self._slots_of(session_ids)
        cols, scores, flags = m.store_peek(slots, iidx, k, exclude_seen, mask, over)
        return cand[cols], scores, flags.astype(bool)

    def _slots_of(self, session_ids):
        sids = _id_list(session_ids)
        if not sids:
            raise ValueError('at least one session is needed')
        for s in sids:
            if s not in self._map.slot:
                raise KeyError(s)
        if len(set(sids)) != len(sids):
            raise ValueError('a session is named twice')
        return np.array([self._map.slot[s] for s in sids], dtype=np.int32)

    # ------------------------------------------------------------------ export / load / end
    def export(self, session_ids=None):
        """The stored sessions (None: all, least recently touched first) as a dict of NumPy arrays: session_ids; hidden: one float32
        array [n, layers[l]] per layer (the layout of recommend_sessions' hidden=); seen_offs int64[n + 1] and seen_items (item IDS,
        every list in stored order: ascending item index); overflow bool[n]; seen_cap.  Nothing changes.  load() accepts it."""
        m = self._live()
        sids = list(self._map.slot) if session_ids is None else _id_list(session_ids)
        ids = np.empty(len(sids), dtype=object)
        ids[:] = sids
        layers = self._g.layers
        if not sids:
            return dict(session_ids=ids, hidden=[np.zeros((0, D), dtype=np.float32) for D in layers], seen_offs=np.zeros(1, dtype=np.int64),
                        seen_items=self._g.itemidmap.index.values[:0], overflow=np.zeros(0, dtype=bool), seen_cap=self.seen_cap)
        H, seen, ln, fl = m.store_read(self._slots_of(sids), self.seen_cap)
        keep = np.arange(self.seen_cap)[None, :] < ln[:, None]
        return dict(session_ids=ids, hidden=self._g._unpad_hidden(H), seen_offs=np.concatenate([[0], np.cumsum(ln)]).astype(np.int64),
                    seen_items=self._g.itemidmap.index.values[seen[keep]], overflow=fl.astype(bool), seen_cap=self.seen_cap)

    def load(self, state):
        """Takes the sessions of an export() dict (of this store, an earlier one or another process's, same model and weights) into
        the store: a session it holds is overwritten, another takes a slot as in push (the call touches them in order, eviction
        included).  Checked before anything changes: the layer shapes, lists no longer than this store's seen_cap, known items."""
        from .gru4rec import _pad_cols, _pad4
        m = self._live()
        g = self._g
        sids = _id_list(state['session_ids'])
        n = len(sids)
        if len(set(sids)) != n:
            raise ValueError('a session is named twice')
        hidden = state['hidden']
        if not isinstance(hidden, (list, tuple)) or len(hidden) != len(g.layers):
            raise ValueError('hidden must be a list of %d arrays, one per layer' % len(g.layers))
        for l, (h, D) in enumerate(zip(hidden, g.layers)):
            if not isinstance(h, np.ndarray) or h.dtype != np.float32 or h.shape != (n, D):
                raise ValueError('hidden[%d] must be a float32 array of shape (%d, %d)' % (l, n, D))
        offs = np.asarray(state['seen_offs'], dtype=np.int64)
        over = np.asarray(state['overflow']).astype(np.int32)
        if len(offs) != n + 1 or len(over) != n or (n and (offs[0] != 0 or (np.diff(offs) < 0).any())):
            raise ValueError('seen_offs must hold n + 1 monotone offsets from 0 and overflow n flags')
        ln = np.diff(offs).astype(np.int32)
        if n == 0:
            return
        if ln.max() > self.seen_cap:
            raise ValueError('session %r has %d seen items, more than this store keeps (seen_cap = %d)' % (sids[int(ln.argmax())], ln.max(), self.seen_cap))
        items = np.ravel(state['seen_items'])
        if len(items) != offs[-1]:
            raise ValueError('seen_items must hold seen_offs[-1] = %d ids' % offs[-1])
        idx = g.itemidmap[items].values.astype(np.int64) if len(items) else np.zeros(0, dtype=np.int64)
        rows = np.repeat(np.arange(n), ln)
        order = np.lexsort((idx, rows))
        idx = idx[order]
        if len(idx) > 1 and ((np.diff(idx) == 0) & (np.diff(rows) == 0)).any():
            raise ValueError('a seen list names an item twice')
        seen = np.zeros((n, self.seen_cap), dtype=np.int32)
        seen[rows, np.arange(len(idx)) - offs[:-1][rows]] = idx
        slots, _, evicted, nrel = self._map.plan(sids)
        m.store_write(slots, [_pad_cols(h, 1, D, _pad4(D)) for h, D in zip(hidden, g.layers)], seen, ln, over)
        self._map.commit(sids, slots, evicted, nrel)

    def end(self, session_ids):
        """Frees the slots of these sessions (they are not counted as evicted).  An unknown session raises KeyError, before any goes."""
        self._live()
        sids = _id_list(session_ids)
        for s in sids:
            if s not in self._map.slot:
                raise KeyError(s)
        self._map.release(list(dict.fromkeys(sids)))

"""GRU4Rec.open_session_store without a GPU: the id map and its least-recently-touched rule against a brute-force model over random
call sequences, the CSR packing of a push's events into rows (distinct sessions in order of first appearance), every refusal -- raised
before the device model (a recording stand-in) is called and before the id map changes -- and the closed-store behaviour."""
import pickle

import numpy as np
import pandas as pd
import pytest

from gru4rec_amd import _native
from gru4rec_amd.gru4rec import GRU4Rec
from gru4rec_amd.session_store import SlotMap, pack_events

BASE = 1000     # item id of item index 0


class Recorder:
    """Stand-in for the device model: records every store call; a selection returns positions 0 .. k - 1 and zero scores."""

    def __init__(self, n_items, layers):
        self.n_items, self.layers, self.calls, self.h, self.open = n_items, layers, [], 1, None

    def store_open(self, capacity, seen_cap):
        assert self.open is None
        self.open = (capacity, seen_cap)
        self.calls.append(('open', capacity, seen_cap))

    def store_close(self):
        self.open = None
        self.calls.append(('close',))

    def store_info(self):
        return (self.open[0], self.open[1], 4096)

    def _out(self, n, k):
        return np.tile(np.arange(k, dtype=np.int32), (n, 1)), np.zeros((n, k), dtype=np.float32), np.zeros(n, dtype=np.int32)

    def store_push(self, ev_offs, ev_items, slots, fresh, item_idx=None, k=0, exclude_seen=False, excl_mask=None, oversample=None):
        cp = (lambda a: None if a is None else np.asarray(a).copy())
        self.calls.append(('push', dict(offs=cp(ev_offs), items=cp(ev_items), slots=cp(slots), fresh=cp(fresh), item_idx=cp(item_idx), k=k,
                                        exclude_seen=exclude_seen, mask=cp(excl_mask), oversample=oversample)))
        return self._out(len(slots), k) if k else None

    def store_peek(self, slots, item_idx=None, k=20, exclude_seen=False, excl_mask=None, oversample=None):
        self.calls.append(('peek', dict(slots=np.asarray(slots).copy(), k=k, exclude_seen=exclude_seen, oversample=oversample)))
        return self._out(len(slots), k)

    def close(self):
        self.h = None


def _model(n_items=300, layers=(50,), final_act='linear'):
    g = GRU4Rec(layers=list(layers), final_act=final_act)
    g.itemidmap = pd.Series(data=np.arange(n_items), index=np.arange(BASE, BASE + n_items), name='ItemIdx')
    g.n_items = n_items
    g.error_during_train = False
    g.Wy = np.zeros((n_items, layers[-1]), dtype=np.float32)
    g._model = Recorder(n_items, [(D + 3) // 4 * 4 for D in layers])
    return g


def ids(*idx):
    return [BASE + i for i in idx]


# ------------------------------------------------------------------ packing
def test_events_become_rows_in_order_of_first_appearance():
    sessions, offs, items = pack_events(['b', 'a', 'b', ('c', 1), 'a', 'b'], [5, 6, 7, 8, 9, 10])
    assert sessions == ['b', 'a', ('c', 1)]
    assert offs.dtype == np.int64 and offs.tolist() == [0, 3, 5, 6]
    assert items.dtype == np.int32 and items.tolist() == [5, 7, 10, 6, 9, 8]
    sessions, offs, items = pack_events(np.array([3, 3, 2]), np.array([1, 2, 3]))
    assert sessions == [3, 2] and all(type(s) is int for s in sessions) and offs.tolist() == [0, 2, 3] and items.tolist() == [1, 2, 3]
    with pytest.raises(ValueError, match='one item per event'):
        pack_events([1, 2], [1])
    with pytest.raises(ValueError, match='at least one event'):
        pack_events([], [])


def test_push_packs_rows_slots_and_fresh_marks():
    g = _model()
    st = g.open_session_store(4, seen_cap=8)
    assert g._model.calls[-1] == ('open', 4, 8) and st.stats() == dict(live=0, capacity=4, seen_cap=8, evictions=0, device_bytes=4096)
    assert st.push(['x', 'y', 'x'], ids(3, 4, 5)) == ['x', 'y']
    c = g._model.calls[-1][1]
    assert c['offs'].tolist() == [0, 2, 3] and c['items'].tolist() == [3, 5, 4] and c['slots'].tolist() == [0, 1] and c['fresh'].tolist() == [1, 1]
    assert c['k'] == 0
    rows, items, scores, over = st.push(['y', 'z'], ids(6, 7), k=3, exclude_seen=True, exclude=ids(0), scan='bf16', oversample=4,
                                        predict_for_item_ids=ids(*range(10, 100)))
    c = g._model.calls[-1][1]
    assert rows == ['y', 'z'] and c['slots'].tolist() == [1, 2] and c['fresh'].tolist() == [0, 1] and c['k'] == 3 and c['exclude_seen']
    assert c['oversample'] == 4 and c['item_idx'].tolist() == list(range(10, 100)) and c['mask'][0] == 1
    assert items.tolist() == [ids(10, 11, 12)] * 2 and scores.shape == (2, 3) and over.dtype == bool
    assert len(st) == 3 and 'x' in st and 'w' not in st
    gi, gs, go = st.recommend(['z', 'x'], k=2)
    assert g._model.calls[-1][0] == 'peek' and g._model.calls[-1][1]['slots'].tolist() == [2, 0] and gi.shape == (2, 2)
    st.end(['x'])
    assert 'x' not in st and st.push(['n'], ids(1)) == ['n'] and g._model.calls[-1][1]['slots'].tolist() == [0]      # lowest free slot first


# ------------------------------------------------------------------ the id map against a brute-force model
def test_slot_map_against_a_brute_force_lru_model():
    rng = np.random.RandomState(0)
    for capacity in (1, 3, 8):
        mp = SlotMap(capacity)
        touch, slot_of, clock, evictions = {}, {}, 0, 0
        for c in range(300):
            if touch and rng.rand() < 0.15:
                gone = [s for s in touch if rng.rand() < 0.3]
                mp.release(gone)
                for s in gone:
                    del touch[s], slot_of[s]
                continue
            sessions = rng.choice(12, size=rng.randint(1, min(capacity, 5) + 1), replace=False).tolist()
            slots, fresh, evicted, nrel = mp.plan(sessions)
            state = (list(mp.slot.items()), list(mp.released), mp.unused)
            assert mp.plan(sessions)[2] == evicted and state == (list(mp.slot.items()), list(mp.released), mp.unused)      # plan changes nothing
            # the model: evict the least recently touched sessions not in the call, as many as there are new sessions without a free slot
            short = sum(1 for s in sessions if s not in touch) - (capacity - len(touch))
            want = sorted((s for s in touch if s not in sessions), key=touch.get)[:max(short, 0)]
            assert evicted == want
            assert fresh.tolist() == [0 if s in touch else 1 for s in sessions]
            for s in want:
                del touch[s], slot_of[s]
            mp.commit(sessions, slots, evicted, nrel)
            evictions += len(want)
            for s, sl in zip(sessions, slots):
                assert slot_of.setdefault(s, int(sl)) == sl      # a live session keeps its slot
                clock += 1
                touch[s] = clock
            assert sorted(slot_of.values()) == sorted(set(slot_of.values())) and all(0 <= v < capacity for v in slot_of.values())
            assert dict(mp.slot) == slot_of and mp.evictions == evictions and mp.n_free() == capacity - len(touch)
            assert list(mp.slot) == sorted(touch, key=touch.get)
        with pytest.raises(ValueError, match='capacity'):
            mp.plan(list(range(100, 101 + capacity)))


def test_eviction_through_the_store_and_pop_evicted():
    g = _model()
    st = g.open_session_store(2, seen_cap=0)
    st.push([1, 2], ids(1, 2))
    st.push([1], ids(3))
    st.push([3], ids(4))                                   # 2 is the least recently touched
    assert st.pop_evicted() == [2] and st.pop_evicted() == [] and 2 not in st and st.stats()['evictions'] == 1
    st.push([2, 3], ids(5, 6))                             # 1 goes; 3 is in the call
    c = g._model.calls[-1][1]
    assert st.pop_evicted() == [1] and c['fresh'].tolist() == [1, 0] and sorted(c['slots'].tolist()) == [0, 1]


# ------------------------------------------------------------------ refusals
def test_open_refusals():
    g = _model()
    for bad in (0, -1, 2 ** 31, 1.5, True, '3'):
        with pytest.raises(ValueError, match='capacity'):
            g.open_session_store(bad)
    for bad in (-1, _native.G4R_EXCLUDE_MAX + 1, 2.0, False):
        with pytest.raises(ValueError, match='seen_cap'):
            g.open_session_store(4, seen_cap=bad)
    assert g._model.calls == []
    st = g.open_session_store(4)
    with pytest.raises(RuntimeError, match='open on this model already'):
        g.open_session_store(4)
    st.close()
    g.open_session_store(4, seen_cap=0)
    with pytest.raises(ValueError, match='fitted or loaded'):
        GRU4Rec().open_session_store(4)


def test_push_refusals_come_before_the_device_and_the_map():
    g = _model()
    st = g.open_session_store(3, seen_cap=64)
    st.push(['a', 'b'], ids(1, 2))
    n_calls, order = len(g._model.calls), list(st._map.slot)
    with pytest.raises(KeyError):
        st.push(['a', 'c'], [BASE + 1, 5], k=5)
    with pytest.raises(ValueError, match='more than the store holds'):
        st.push(list('wxyz'), ids(1, 2, 3, 4))
    for bad in (0, 257, 301, 1.5):
        with pytest.raises(ValueError, match='k = '):
            st.push(['a'], ids(1), k=bad)
    with pytest.raises(ValueError, match="must be 'fp32' or 'bf16'"):
        st.push(['a'], ids(1), k=5, scan='fp16')
    with pytest.raises(ValueError, match='oversample'):
        st.push(['a'], ids(1), k=5, scan='bf16', oversample=0)
    with pytest.raises(ValueError, match='conservative'):
        st.push(['a'], ids(1), k=237, exclude_seen=True)                    # 237 + 64 > 300
    st.push(['a'], ids(1), k=236, exclude_seen=True)                        # 236 + 64 = 300
    n_calls, order = n_calls + 1, list(st._map.slot)
    with pytest.raises(ValueError, match='conservative'):
        st.push(['a'], ids(1), k=236, exclude_seen=True, exclude=ids(7))    # one globally excluded candidate more
    with pytest.raises(ValueError, match='duplicate-free'):
        st.recommend(['a'], k=2, exclude_seen=True, predict_for_item_ids=ids(*([1, 1] + list(range(100, 200)))))
    with pytest.raises(ValueError, match='fewer than k'):
        st.push(['a'], ids(1), k=5, exclude=ids(1, 2), predict_for_item_ids=ids(1, 2, 3, 4, 5, 6))
    with pytest.raises(KeyError):
        st.recommend(['nobody'], k=5)
    with pytest.raises(ValueError, match='named twice'):
        st.recommend(['a', 'a'], k=5)
    with pytest.raises(KeyError):
        st.end(['a', 'nobody'])
    with pytest.raises(ValueError, match='one item per event'):
        st.push(['a', 'b'], ids(1))
    assert len(g._model.calls) == n_calls and list(st._map.slot) == order and st.pop_evicted() == []
    g2 = _model()
    st0 = g2.open_session_store(3, seen_cap=0)
    with pytest.raises(ValueError, match='seen_cap = 0'):
        st0.push(['a'], ids(1), k=5, exclude_seen=True)
    st0.push(['a'], ids(1), k=5)


# ------------------------------------------------------------------ closed stores
def test_a_closed_store_refuses_every_call():
    for how in ('close', 'model_close', 'prepare', 'replaced'):
        g = _model()
        st = g.open_session_store(3)
        st.push(['a'], ids(1))
        if how == 'close':
            st.close()
            assert g._model.calls[-1] == ('close',)
        elif how == 'model_close':
            g.close()
        elif how == 'prepare':
            g._drop_session_store()      # what prepare (so fit) and run_epoch call before the weights change
            assert g._model.calls[-1] == ('close',)
        else:
            g._model = Recorder(300, [52])
        assert st.closed and g._store is None or how == 'replaced'
        for call in (lambda: st.push(['a'], ids(1)), lambda: st.recommend(['a'], k=2), st.export, lambda: st.load({}), lambda: st.end(['a'])):
            with pytest.raises(RuntimeError, match='closed'):
                call()
        assert len(st) == 1      # (the host side can still be inspected)
        if how != 'model_close':
            g.open_session_store(2).close()


def test_the_store_is_not_pickled():
    g = _model()
    g.open_session_store(3)
    model, g._model = g._model, None
    g2 = pickle.loads(pickle.dumps(g))
    g._model = model
    assert getattr(g2, '_store', None) is None and g._store is not None


def test_mutant_33_is_registered():
    from gru4rec_amd import build as g4r_build
    assert 33 in g4r_build.MUTANTS and 'LONGEST' in g4r_build.MUTANTS[33]

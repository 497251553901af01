"""_native.Model without a device and without the shared object: `_native.lib` is replaced by a fake whose g4r_* entries copy out what
they are handed (every array read back through its pointer, so with the pointer's own element type), fill every output array with
1, 2, 3, ... and return 0.  Pinned per inference / plan entry: which entry is called, the position of every argument, the integer
values, the contents and dtype of every array, which pointers are NULL, the shapes and dtypes of what returns -- and every
ValueError this layer raises, with its text."""
import ctypes as C
import re

import numpy as np
import pytest

from gru4rec_amd import _native
from gru4rec_amd._native import Model, NativeError

HANDLE = 0x5EED
N_ITEMS, LAYERS = 70, (8, 4)
WORDS = (N_ITEMS + 31) // 32
MASK_TEXT = 'excl_mask must hold ceil(n_items / 32) words'
HIST_TEXT = 'hist_offs must hold n + 1 >= 2 offsets into hist_items'

# One line per C entry: its arguments in the order of include/gru4rec_hip.h.  'name' is an integer (or the handle, or bytes);
# 'name*len' an input array of `len` elements; 'name>len' an output array; 'name**rows' / 'name>>rows' an array of one float pointer
# per layer, [rows, layers[l]] each; 'name@' an integer passed by reference (the fake stores 77).  `len` is an expression over the
# integer arguments of the same call and over Fake.env.
_SESS = ('h', 'hist_offs*n+1', 'hist_items*nh', 'n', 'hidden**n', 'item_idx*n_sel', 'n_sel')
_EXCL = ('excl_offs*n+1', 'excl_items*nx', 'excl_mask*W')
_PLAN = ('h', 'in_idx*T*B', 'out_idx*T*B', 'reset*T*B', 'M*T', 'T')
SPECS = {
    'g4r_predict_step': ('h', 'in_idx*n', 'n', 'item_idx*n_sel', 'n_sel', 'out>n*n_sel'),
    'g4r_recommend_step': ('h', 'in_idx*n', 'n', 'item_idx*n_sel', 'n_sel', 'k', 'cols>n*k', 'scores>n*k'),
    'g4r_recommend_step_filtered': ('h', 'in_idx*n', 'n', 'item_idx*n_sel', 'n_sel', 'k') + _EXCL + ('cols>n*k', 'scores>n*k'),
    'g4r_recommend_step_scan': ('h', 'in_idx*n', 'n', 'item_idx*n_sel', 'n_sel', 'k', 'oversample') + _EXCL + ('cols>n*k', 'scores>n*k'),
    'g4r_recommend_sessions': _SESS + ('k',) + _EXCL + ('cols>n*k', 'scores>n*k', 'hout>>n'),
    'g4r_recommend_sessions_scan': _SESS + ('k', 'oversample') + _EXCL + ('cols>n*k', 'scores>n*k', 'hout>>n'),
    'g4r_continue_sessions': _SESS + ('k', 'oversample', 'steps', 'no_repeat') + _EXCL + ('cols>n*steps*k', 'scores>n*steps*k', 'hout>>n'),
    'g4r_beam_sessions': _SESS + ('beams', 'oversample', 'steps', 'no_repeat', 'combine') + _EXCL + (
        'parent>n*steps*beams', 'cols>n*steps*beams', 'step_scores>n*steps*beams', 'path_scores>n*beams', 'scale_exp>n'),
    'g4r_similar_items': ('h', 'space', 'metric', 'q_idx*n', 'n', 'item_idx*n_sel', 'n_sel', 'k', 'exclude_self', 'excl_mask*W',
                          'cols>n*k', 'scores>n*k'),
    'g4r_score_candidates': ('h', 'in_idx*n', 'n', 'cand_offs*n+1', 'cand_items*ncand', 'k', 'scores>n*k if k else ncand', 'pos>n*k'),
    'g4r_score_candidates_sessions': ('h', 'hist_offs*n+1', 'hist_items*nh', 'n', 'hidden**n', 'cand_offs*n+1', 'cand_items*ncand', 'k',
                                      'scores>n*k if k else ncand', 'pos>n*k', 'hout>>n'),
    'g4r_set_plan': _PLAN + ('compact_steps*nc', 'compact_maps*nc*B', 'nc'),
    'g4r_evaluate': _PLAN + ('B', 'compact_steps*max(nc,1)', 'compact_maps*max(nc,1)*B', 'nc', 'items*n_it', 'n_it', 'cutoffs*n_cut',
                             'n_cut', 'mode', 'recall>n_cut', 'mrr>n_cut', 'n_events@'),
    'g4r_recommend_events': _PLAN + ('B', 'compact_steps*max(nc,1)', 'compact_maps*max(nc,1)*B', 'nc', 'items*n_it', 'n_it', 'mode',
                                     'slot*T*B', 'n_slots', 'k', 'excl_mask*W', 'seen_offs*ns+1', 'seen_items*nseen', 'seen_first*nseen',
                                     'ns', 'sess*T*B', 'pos*T*B', 'out_items>n_slots*k', 'out_scores>n_slots*k', 'rank>n_slots',
                                     'target_score>n_slots'),
    'g4r_p2p_attach': ('h', 'blob', 'nranks', 'rank'),
    'g4r_debug_loss_rows': ('h', 'scores>count', 'count', 'M', 'lossrow>B'),
}


def _read(p, n):
    """A copy of the n elements behind a ctypes pointer, in the pointer's element type."""
    return np.ctypeslib.as_array(p, shape=(n,)).copy() if n else np.zeros(0, dtype=np.dtype(p._type_))


def _fill(p, n):
    if n:
        a = np.ctypeslib.as_array(p, shape=(n,))
        a[:] = np.arange(1, n + 1)


class Fake:
    """Stand-in for the loaded library.  calls: [(entry, {argument name: value})]; a NULL pointer is recorded as None."""

    def __init__(self):
        self.calls, self.rc, self.env = [], 0, {}
        self.error = b'the fake refused'

    def g4r_last_error(self):
        return self.error

    def g4r_destroy(self, h):
        self.calls.append(('g4r_destroy', {}))

    def __getattr__(self, name):
        if name not in SPECS:
            raise AttributeError(name)

        def entry(*args):
            spec = SPECS[name]
            assert len(args) == len(spec), '%s takes %d arguments, %d given' % (name, len(spec), len(args))
            got, ints = {}, dict(self.env, W=WORDS)
            for s, a in zip(spec, args):
                if not re.search(r'[*>@]', s):
                    got[s] = a.value if isinstance(a, C.c_void_p) else a
                    if isinstance(a, int):
                        ints[s] = a
            for s, a in zip(spec, args):
                m = re.match(r'(\w+)(\*\*|>>|\*|>|@)(.*)', s)
                if not m:
                    continue
                key, kind, expr = m.groups()
                if a is None:
                    got[key] = None
                elif kind == '@':
                    a._obj.value = 77
                    got[key] = '@'
                else:
                    n = int(eval(expr, {}, ints))
                    if kind in ('**', '>>'):
                        assert len(a) == len(LAYERS) and a._type_ is C.POINTER(C.c_float)
                        got[key] = [_read(a[l], n * D).reshape(n, D) for l, D in enumerate(LAYERS)]
                        if kind == '>>':
                            for l, D in enumerate(LAYERS):
                                _fill(a[l], n * D)
                    else:
                        got[key] = _read(a, n)
                        if kind == '>':
                            _fill(a, n)
            self.calls.append((name, got))
            return self.rc
        return entry

    def only(self):
        assert len(self.calls) == 1, [c[0] for c in self.calls]
        return self.calls.pop()


@pytest.fixture
def fake(monkeypatch):
    f = Fake()
    monkeypatch.setattr(_native, 'lib', lambda: f)
    return f


@pytest.fixture
def m(fake):
    mod = Model.__new__(Model)
    mod.cfg = _native.G4RConfig()
    mod.cfg.n_items = N_ITEMS
    mod.layers, mod.h, mod.T = list(LAYERS), C.c_void_p(HANDLE), 0
    yield mod
    mod.h = None      # nothing to destroy


def same(a, values, dtype):
    assert a is not None and a.dtype == np.dtype(dtype), (a, dtype)
    assert a.tolist() == list(values)


def filled(a, shape, dtype):
    """An output array the fake has written: the array that returns is the one whose pointer was handed over, at that size."""
    assert a.shape == tuple(shape) and a.dtype == np.dtype(dtype)
    assert a.ravel().tolist() == list(range(1, a.size + 1))


def raises(text):
    return pytest.raises(ValueError, match='^' + re.escape(text) + '$')


HIST = dict(hist_offs=[0, 2, 3, 6], hist_items=[5, 6, 7, 1, 2, 3])           # n = 3 sessions
EXCL = dict(excl_offs=[0, 1, 1, 3], excl_items=[9, 4, 8], excl_mask=[1, 2, 0x30])
MASK = np.array([7, 0, 0x21], dtype=np.uint64)


def hidden(n=3, dtype=np.float32):
    return [np.arange(n * D, dtype=dtype).reshape(n, D) + 100 * l for l, D in enumerate(LAYERS)]


def check_hist(c):
    same(c['hist_offs'], HIST['hist_offs'], np.int64)
    same(c['hist_items'], HIST['hist_items'], np.int32)
    assert c['h'] == HANDLE and c['n'] == 3


def check_excl(c, supplied):
    if supplied:
        same(c['excl_offs'], EXCL['excl_offs'], np.int64)
        same(c['excl_mask'], EXCL['excl_mask'], np.uint32)
    else:
        assert c['excl_offs'] is None and c['excl_mask'] is None
    same(c['excl_items'], EXCL['excl_items'] if supplied else [], np.int32)      # never NULL: an empty array without exclusions


def check_hidden_in(c, supplied):
    if not supplied:
        assert c['hidden'] is None
        return
    for got, want in zip(c['hidden'], hidden()):
        assert got.dtype == np.float32
        np.testing.assert_array_equal(got, want)


def check_hout(c, out, returned):
    if not returned:
        assert c['hout'] is None
        return
    assert isinstance(out, list) and len(out) == len(LAYERS)
    for h, D in zip(out, LAYERS):
        filled(h, (3, D), np.float32)


# ---------------------------------------------------------------------------------------------------- the stepwise entries
def test_predict_step(m, fake):
    out = m.predict_step([3, 4], [7, 8, 9])
    name, c = fake.only()
    assert name == 'g4r_predict_step' and c['h'] == HANDLE and c['n'] == 2 and c['n_sel'] == 3
    same(c['in_idx'], [3, 4], np.int32)
    same(c['item_idx'], [7, 8, 9], np.int32)
    filled(out, (2, 3), np.float32)
    out = m.predict_step(np.array([3, 4, 5], dtype=np.int64))
    name, c = fake.only()
    assert c['item_idx'] is None and c['n_sel'] == N_ITEMS and c['n'] == 3
    filled(out, (3, N_ITEMS), np.float32)
    assert m.predict_step([3], want_scores=False) is None
    name, c = fake.only()
    assert name == 'g4r_predict_step' and c['out'] is None and c['item_idx'] is None and c['n_sel'] == N_ITEMS


def test_recommend_step(m, fake):
    cols, scores = m.recommend_step([3, 4], [7, 8, 9], 2)
    name, c = fake.only()
    assert name == 'g4r_recommend_step' and c['h'] == HANDLE and (c['n'], c['n_sel'], c['k']) == (2, 3, 2)
    same(c['in_idx'], [3, 4], np.int32)
    same(c['item_idx'], [7, 8, 9], np.int32)
    filled(cols, (2, 2), np.int32)
    filled(scores, (2, 2), np.float32)
    cols, scores = m.recommend_step([3])
    name, c = fake.only()
    assert c['item_idx'] is None and (c['n'], c['n_sel'], c['k']) == (1, N_ITEMS, 20)
    filled(cols, (1, 20), np.int32)


@pytest.mark.parametrize('oversample', [None, 4])
def test_recommend_step_filtered(m, fake, oversample):
    fake.env = dict(nx=3)
    cols, scores = m.recommend_step_filtered([3, 4, 5], [7, 8, 9, 10], 2, oversample=oversample, **EXCL)
    name, c = fake.only()
    assert name == ('g4r_recommend_step_filtered' if oversample is None else 'g4r_recommend_step_scan')
    assert c['h'] == HANDLE and (c['n'], c['n_sel'], c['k']) == (3, 4, 2) and c.get('oversample') == oversample
    same(c['in_idx'], [3, 4, 5], np.int32)
    same(c['item_idx'], [7, 8, 9, 10], np.int32)
    check_excl(c, True)
    filled(cols, (3, 2), np.int32)
    filled(scores, (3, 2), np.float32)
    fake.env = dict(nx=0)
    cols, scores = m.recommend_step_filtered([3, 4, 5], oversample=oversample)
    name, c = fake.only()
    assert c['item_idx'] is None and (c['n'], c['n_sel'], c['k']) == (3, N_ITEMS, 20)
    check_excl(c, False)
    filled(cols, (3, 20), np.int32)
    fake.env = dict(nx=0)
    m.recommend_step_filtered([3], excl_mask=MASK, oversample=oversample)      # a mask alone; any integer dtype is converted
    same(fake.only()[1]['excl_mask'], MASK.tolist(), np.uint32)


def test_recommend_step_filtered_refusals(m, fake):
    text = 'excl_offs must hold rows + 1 offsets into excl_items'
    for offs, items in (([0, 1, 3], [1, 2, 3]), ([0, 1, 1, 4], [1, 2, 3]), ([-1, 1, 1, 3], [1, 2, 3]), ([0, 0, 0, 1], None)):
        with raises(text):
            m.recommend_step_filtered([3, 4, 5], None, 2, offs, items)
    with raises(MASK_TEXT):
        m.recommend_step_filtered([3, 4, 5], None, 2, excl_mask=[0, 0])
    with raises(text):                                                      # the list check comes first
        m.recommend_step_filtered([3, 4, 5], None, 2, [0], [], excl_mask=[0, 0])
    assert not fake.calls


# ---------------------------------------------------------------------------------------------------- the session entries
@pytest.mark.parametrize('oversample', [None, 4])
def test_recommend_sessions(m, fake, oversample):
    fake.env = dict(nh=6, nx=3)
    out = m.recommend_sessions(item_idx=[7, 8, 9, 10], k=2, hidden=hidden(), return_hidden=True, oversample=oversample, **HIST, **EXCL)
    name, c = fake.only()
    assert name == ('g4r_recommend_sessions' if oversample is None else 'g4r_recommend_sessions_scan')
    check_hist(c)
    assert (c['n_sel'], c['k']) == (4, 2) and c.get('oversample') == oversample
    same(c['item_idx'], [7, 8, 9, 10], np.int32)
    check_excl(c, True)
    check_hidden_in(c, True)
    assert len(out) == 3
    filled(out[0], (3, 2), np.int32)
    filled(out[1], (3, 2), np.float32)
    check_hout(c, out[2], True)
    fake.env = dict(nh=6, nx=0)
    out = m.recommend_sessions(HIST['hist_offs'], HIST['hist_items'], oversample=oversample)
    name, c = fake.only()
    check_hist(c)
    assert c['item_idx'] is None and (c['n_sel'], c['k']) == (N_ITEMS, 20)
    check_excl(c, False)
    check_hidden_in(c, False)
    check_hout(c, None, False)
    assert len(out) == 2
    filled(out[0], (3, 20), np.int32)
    filled(out[1], (3, 20), np.float32)


def test_hidden_is_converted_to_float32(m, fake):
    fake.env = dict(nh=6, nx=0)
    m.recommend_sessions(hidden=hidden(dtype=np.float64), **HIST)
    check_hidden_in(fake.only()[1], True)


def test_continue_sessions(m, fake):
    fake.env = dict(nh=6, nx=3)
    out = m.continue_sessions(item_idx=[7, 8, 9, 10], k=2, steps=3, no_repeat=False, hidden=hidden(), return_hidden=True, oversample=4,
                              **HIST, **EXCL)
    name, c = fake.only()
    assert name == 'g4r_continue_sessions'
    check_hist(c)
    assert (c['n_sel'], c['k'], c['oversample'], c['steps'], c['no_repeat']) == (4, 2, 4, 3, 0)
    same(c['item_idx'], [7, 8, 9, 10], np.int32)
    check_excl(c, True)
    check_hidden_in(c, True)
    assert len(out) == 3
    filled(out[0], (3, 3, 2), np.int32)
    filled(out[1], (3, 3, 2), np.float32)
    check_hout(c, out[2], True)
    fake.env = dict(nh=6, nx=0)
    out = m.continue_sessions(HIST['hist_offs'], HIST['hist_items'])
    name, c = fake.only()
    check_hist(c)
    assert c['item_idx'] is None and (c['n_sel'], c['k'], c['oversample'], c['steps'], c['no_repeat']) == (N_ITEMS, 1, 0, 1, 1)
    check_excl(c, False)
    check_hidden_in(c, False)
    check_hout(c, None, False)
    assert len(out) == 2
    filled(out[0], (3, 1, 1), np.int32)
    filled(out[1], (3, 1, 1), np.float32)


def test_beam_sessions(m, fake):
    fake.env = dict(nh=6, nx=3)
    out = m.beam_sessions(item_idx=[7, 8, 9, 10], beams=2, steps=3, no_repeat=False, combine='product', hidden=hidden(), oversample=4,
                          **HIST, **EXCL)
    name, c = fake.only()
    assert name == 'g4r_beam_sessions'
    check_hist(c)
    assert (c['n_sel'], c['beams'], c['oversample'], c['steps'], c['no_repeat'], c['combine']) == (4, 2, 4, 3, 0, 1)
    same(c['item_idx'], [7, 8, 9, 10], np.int32)
    check_excl(c, True)
    check_hidden_in(c, True)
    assert len(out) == 5
    filled(out[0], (3, 3, 2), np.int32)
    filled(out[1], (3, 3, 2), np.int32)
    filled(out[2], (3, 3, 2), np.float32)
    filled(out[3], (3, 2), np.float32)
    filled(out[4], (3,), np.int32)
    fake.env = dict(nh=6, nx=0)
    out = m.beam_sessions(HIST['hist_offs'], HIST['hist_items'])
    name, c = fake.only()
    check_hist(c)
    assert c['item_idx'] is None
    assert (c['n_sel'], c['beams'], c['oversample'], c['steps'], c['no_repeat'], c['combine']) == (N_ITEMS, 4, 0, 1, 1, 0)
    check_excl(c, False)
    check_hidden_in(c, False)
    filled(out[0], (3, 1, 4), np.int32)
    filled(out[3], (3, 4), np.float32)


def test_score_candidates_sessions(m, fake):
    fake.env = dict(nh=6, ncand=5)
    out = m.score_candidates_sessions(cand_offs=[0, 2, 3, 5], cand_items=[9, 8, 7, 6, 5], k=1, hidden=hidden(), return_hidden=True, **HIST)
    name, c = fake.only()
    assert name == 'g4r_score_candidates_sessions'
    check_hist(c)
    assert c['k'] == 1
    same(c['cand_offs'], [0, 2, 3, 5], np.int64)
    same(c['cand_items'], [9, 8, 7, 6, 5], np.int32)
    check_hidden_in(c, True)
    (pos, scores), hout = out
    filled(pos, (3, 1), np.int32)
    filled(scores, (3, 1), np.float32)
    check_hout(c, hout, True)
    scores = m.score_candidates_sessions(HIST['hist_offs'], HIST['hist_items'], [0, 2, 3, 5], [9, 8, 7, 6, 5])
    name, c = fake.only()
    assert c['k'] == 0 and c['pos'] is None
    check_hidden_in(c, False)
    check_hout(c, None, False)
    filled(scores, (5,), np.float32)
    scores, hout = m.score_candidates_sessions(HIST['hist_offs'], HIST['hist_items'], [0, 2, 3, 5], [9, 8, 7, 6, 5], return_hidden=True)
    name, c = fake.only()
    filled(scores, (5,), np.float32)
    check_hout(c, hout, True)


SESSION_CALLS = {
    'recommend_sessions': lambda m, **kw: m.recommend_sessions(**kw),
    'continue_sessions': lambda m, **kw: m.continue_sessions(**kw),
    'beam_sessions': lambda m, **kw: m.beam_sessions(**kw),
    'score_candidates_sessions': lambda m, **kw: m.score_candidates_sessions(cand_offs=[0, 1, 2, 3], cand_items=[1, 2, 3], **kw),
}


@pytest.mark.parametrize('call', sorted(SESSION_CALLS))
def test_session_refusals_histories_and_hidden(m, fake, call):
    f = SESSION_CALLS[call]
    for offs, items in (([0], [1, 2]), ([], [1, 2]), ([-1, 1, 2], [1, 2]), ([0, 1, 3], [1, 2])):
        with raises(HIST_TEXT):
            f(m, hist_offs=offs, hist_items=items)
    with raises('hidden holds 1 arrays, one per layer (2) is needed'):
        f(m, hidden=hidden()[:1], **HIST)
    with raises('hidden holds 3 arrays, one per layer (2) is needed'):
        f(m, hidden=hidden() + hidden()[:1], **HIST)
    with raises('hidden[0] has shape (2, 8), (3, 8) is needed'):
        f(m, hidden=hidden(2), **HIST)
    with raises('hidden[1] has shape (3, 8), (3, 4) is needed'):
        f(m, hidden=[hidden()[0], hidden()[0]], **HIST)
    assert not fake.calls


@pytest.mark.parametrize('call', ['recommend_sessions', 'continue_sessions', 'beam_sessions'])
def test_session_refusals_exclusions(m, fake, call):
    f = SESSION_CALLS[call]
    text = 'excl_offs must hold n + 1 offsets into excl_items'
    for offs, items in (([0, 1, 3], [1, 2, 3]), ([0, 1, 1, 4], [1, 2, 3]), ([-1, 1, 1, 3], [1, 2, 3]), ([0, 0, 0, 1], None)):
        with raises(text):
            f(m, excl_offs=offs, excl_items=items, **HIST)
    with raises(MASK_TEXT):
        f(m, excl_mask=[0, 0], **HIST)
    with raises(text):                                                      # the order of the checks: lists, mask, hidden
        f(m, excl_offs=[0], excl_mask=[0, 0], hidden=[], **HIST)
    with raises(MASK_TEXT):
        f(m, excl_mask=[0, 0], hidden=[], **HIST)
    with raises(HIST_TEXT):                                                 # and the histories before everything else
        f(m, hist_offs=[0], hist_items=[], excl_offs=[0], excl_mask=[0, 0], hidden=[])
    assert not fake.calls


def test_steps_and_beams_refusals(m, fake):
    with raises('steps must be at least 1'):
        m.continue_sessions(steps=0, **HIST)
    with raises('steps must be at least 1'):
        m.beam_sessions(steps=-2, **HIST)
    for beams in (0, -1, _native.G4R_BEAM_MAX + 1):
        with raises('beams must be in [1, %d]' % _native.G4R_BEAM_MAX):
            m.beam_sessions(beams=beams, **HIST)
    with raises('steps must be at least 1'):                                # steps before beams, both before the exclusions
        m.beam_sessions(steps=0, beams=0, excl_mask=[0], **HIST)
    with raises('steps must be at least 1'):
        m.continue_sessions(steps=0, excl_mask=[0], **HIST)
    with raises(HIST_TEXT):
        m.beam_sessions(hist_offs=[0], hist_items=[], steps=0)
    assert not fake.calls
    fake.env = dict(nh=6, nx=0)
    m.beam_sessions(beams=_native.G4R_BEAM_MAX, steps=1.0, **HIST)          # the bounds themselves pass, as integers
    c = fake.only()[1]
    assert c['beams'] == _native.G4R_BEAM_MAX and c['steps'] == 1 and isinstance(c['steps'], int)


# ---------------------------------------------------------------------------------------------------- similar_items, candidates
def test_similar_items(m, fake):
    cols, scores = m.similar_items([3, 4], [7, 8, 9], 2, 'dot', 'input', False, MASK)
    name, c = fake.only()
    assert name == 'g4r_similar_items' and c['h'] == HANDLE
    assert (c['space'], c['metric'], c['n'], c['n_sel'], c['k'], c['exclude_self']) == (1, 0, 2, 3, 2, 0)
    same(c['q_idx'], [3, 4], np.int32)
    same(c['item_idx'], [7, 8, 9], np.int32)
    same(c['excl_mask'], MASK.tolist(), np.uint32)
    filled(cols, (2, 2), np.int32)
    filled(scores, (2, 2), np.float32)
    cols, scores = m.similar_items([3])
    name, c = fake.only()
    assert c['item_idx'] is None and c['excl_mask'] is None
    assert (c['space'], c['metric'], c['n'], c['n_sel'], c['k'], c['exclude_self']) == (0, 1, 1, N_ITEMS, 20, 1)
    filled(cols, (1, 20), np.int32)
    with raises(MASK_TEXT):
        m.similar_items([3], excl_mask=[0, 0])
    assert not fake.calls


def test_score_candidates(m, fake):
    fake.env = dict(ncand=5)
    pos, scores = m.score_candidates([3, 4, 5], [0, 2, 3, 5], [9, 8, 7, 6, 5], 1)
    name, c = fake.only()
    assert name == 'g4r_score_candidates' and c['h'] == HANDLE and (c['n'], c['k']) == (3, 1)
    same(c['in_idx'], [3, 4, 5], np.int32)
    same(c['cand_offs'], [0, 2, 3, 5], np.int64)
    same(c['cand_items'], [9, 8, 7, 6, 5], np.int32)
    filled(pos, (3, 1), np.int32)
    filled(scores, (3, 1), np.float32)
    scores = m.score_candidates([3, 4, 5], [0, 2, 3, 5], [9, 8, 7, 6, 5])
    name, c = fake.only()
    assert c['k'] == 0 and c['pos'] is None
    filled(scores, (5,), np.float32)
    fake.env = dict(ncand=6)
    scores = m.score_candidates([3, 4], [1, 2, 5], [9, 8, 7, 6, 5, 4])      # a CSR that does not start at 0: offs[-1] - offs[0] scores
    fake.only()
    assert scores.shape == (4,)


def test_cand_offs_refusals(m, fake):
    for offs, items in (([0, 1, 2], [1, 2, 3]), ([0, 1, 2, 4], [1, 2, 3]), ([-1, 1, 2, 3], [1, 2, 3])):
        with raises('cand_offs must hold rows + 1 = 4 offsets into cand_items'):
            m.score_candidates([3, 4, 5], offs, items)
        with raises('cand_offs must hold rows + 1 = 4 offsets into cand_items'):
            m.score_candidates_sessions(cand_offs=offs, cand_items=items, **HIST)
    with raises(HIST_TEXT):                                                 # the histories first, the hidden state last
        m.score_candidates_sessions([0], [], [0], [])
    with raises('cand_offs must hold rows + 1 = 4 offsets into cand_items'):
        m.score_candidates_sessions(cand_offs=[0], cand_items=[], hidden=[], **HIST)
    assert not fake.calls


# ---------------------------------------------------------------------------------------------------- plans
T_, B_ = 3, 2


def plan(nc):
    p = dict(T=T_, n_compact=nc,
             in_idx=np.arange(T_ * B_, dtype=np.int32).reshape(T_, B_) + 10, out_idx=np.arange(T_ * B_, dtype=np.int32).reshape(T_, B_) + 20,
             reset=np.array([[1, 1], [0, 1], [0, 0]], dtype=np.uint8), M=np.array([2, 2, 1], dtype=np.int32),
             compact_steps=np.array([2, 1][:nc], dtype=np.int64), compact_maps=np.array([[0, -1], [1, 0]][:nc], dtype=np.int32).reshape(nc, B_))
    return p


def check_plan(c, p):
    assert c['h'] == HANDLE and c['T'] == T_ and c['nc'] == p['n_compact']
    same(c['in_idx'], p['in_idx'].ravel(), np.int32)
    same(c['out_idx'], p['out_idx'].ravel(), np.int32)
    same(c['reset'], p['reset'].ravel(), np.uint8)
    same(c['M'], p['M'], np.int32)


def check_compact(c, p, dummies):
    """n_compact > 0: the tables; 0: NULL from set_plan, one zeroed entry / row from evaluate and recommend_events."""
    if p['n_compact']:
        same(c['compact_steps'], p['compact_steps'], np.int64)
        same(c['compact_maps'], p['compact_maps'].ravel(), np.int32)
    elif dummies:
        same(c['compact_steps'], [0], np.int64)
        same(c['compact_maps'], [0] * B_, np.int32)
    else:
        assert c['compact_steps'] is None and c['compact_maps'] is None


@pytest.mark.parametrize('nc', [0, 2])
def test_set_plan(m, fake, nc):
    fake.env = dict(B=B_)
    p = plan(nc)
    assert m.set_plan(p) is None and m.T == T_
    name, c = fake.only()
    assert name == 'g4r_set_plan'
    check_plan(c, p)
    check_compact(c, p, dummies=False)
    q = {k: (v.astype(np.int64) if isinstance(v, np.ndarray) else v) for k, v in p.items() if k != 'n_compact'}
    m.set_plan(q)                                                           # set_plan converts; without 'n_compact' there are no tables
    name, c = fake.only()
    check_plan(c, dict(p, n_compact=0))
    assert c['compact_steps'] is None and c['compact_maps'] is None


@pytest.mark.parametrize('nc', [0, 2])
def test_evaluate(m, fake, nc):
    p = plan(nc)
    rec, mrr, n = m.evaluate(p, B_, [7, 8, 9], [1, 5, 20], 'conservative')
    name, c = fake.only()
    assert name == 'g4r_evaluate'
    check_plan(c, p)
    check_compact(c, p, dummies=True)
    assert (c['B'], c['n_it'], c['n_cut'], c['mode']) == (B_, 3, 3, 1) and c['n_events'] == '@' and n == 77
    same(c['items'], [7, 8, 9], np.int32)
    same(c['cutoffs'], [1, 5, 20], np.int32)
    filled(rec, (3,), np.float64)
    filled(mrr, (3,), np.float64)
    rec, mrr, n = m.evaluate(p, B_, None, [20], 'standard')
    name, c = fake.only()
    assert c['items'] is None and (c['n_it'], c['n_cut'], c['mode']) == (0, 1, 0)
    filled(rec, (1,), np.float64)


def seen_tables():
    return dict(offs=[0, 2, 3], items=[4, 5, 6], first=[0, 1, 0], sess=np.array([[0, 1], [0, 1], [0, -1]]), pos=np.arange(T_ * B_).reshape(T_, B_))


@pytest.mark.parametrize('nc', [0, 2])
def test_recommend_events(m, fake, nc):
    p = plan(nc)
    slot = np.array([[0, 1], [2, 3], [4, -1]])
    fake.env = dict(nseen=3)
    oi, os_, rk, ts = m.recommend_events(p, B_, [7, 8, 9], 'median', slot, 5, 2, excl_mask=MASK, seen=seen_tables())
    name, c = fake.only()
    assert name == 'g4r_recommend_events'
    check_plan(c, p)
    check_compact(c, p, dummies=True)
    assert (c['B'], c['n_it'], c['mode'], c['n_slots'], c['k'], c['ns']) == (B_, 3, 2, 5, 2, 2)
    same(c['items'], [7, 8, 9], np.int32)
    same(c['slot'], slot.ravel(), np.int64)
    same(c['excl_mask'], MASK.tolist(), np.uint32)
    same(c['seen_offs'], [0, 2, 3], np.int64)
    same(c['seen_items'], [4, 5, 6], np.int32)
    same(c['seen_first'], [0, 1, 0], np.int32)
    same(c['sess'], [0, 1, 0, 1, 0, -1], np.int32)
    same(c['pos'], range(T_ * B_), np.int32)
    filled(oi, (5, 2), np.int32)
    filled(os_, (5, 2), np.float32)
    filled(rk, (5,), np.float32)
    filled(ts, (5,), np.float32)
    oi, os_, rk, ts = m.recommend_events(p, B_, None, 'standard', slot, 5, 2, want_lists=False)
    name, c = fake.only()
    assert c['items'] is None and c['excl_mask'] is None and (c['n_it'], c['mode'], c['ns']) == (0, 0, 0)
    assert all(c[key] is None for key in ('seen_offs', 'seen_items', 'seen_first', 'sess', 'pos', 'out_items', 'out_scores'))
    assert oi is None and os_ is None
    filled(rk, (5,), np.float32)
    filled(ts, (5,), np.float32)


def test_recommend_events_refusals(m, fake):
    p = plan(0)
    slot = np.zeros((T_, B_), dtype=np.int64)
    with raises('slot must hold T * batch = 6 entries'):
        m.recommend_events(p, B_, None, 'standard', slot[:2], 5, 2)
    with raises(MASK_TEXT):
        m.recommend_events(p, B_, None, 'standard', slot, 5, 2, excl_mask=[0, 0])
    text = 'seen tables: sess / pos must hold T * batch entries, items / first one entry per offset'
    for key, bad in (('sess', np.zeros((2, B_))), ('pos', np.zeros((T_, B_ + 1))), ('first', [0, 1]), ('offs', [0, 2, 4])):
        with raises(text):
            m.recommend_events(p, B_, None, 'standard', slot, 5, 2, seen=dict(seen_tables(), **{key: bad}))
    with raises('slot must hold T * batch = 6 entries'):                    # the order: slot, mask, seen
        m.recommend_events(p, B_, None, 'standard', slot[:2], 5, 2, excl_mask=[0, 0], seen=dict(seen_tables(), first=[0]))
    with raises(MASK_TEXT):
        m.recommend_events(p, B_, None, 'standard', slot, 5, 2, excl_mask=[0, 0], seen=dict(seen_tables(), first=[0]))
    assert not fake.calls


# ---------------------------------------------------------------------------------------------------- the rest
def test_p2p_attach(m, fake):
    m.p2p_attach([b'a' * 64, b'b' * 64], 2, 1)
    name, c = fake.only()
    assert name == 'g4r_p2p_attach' and c == dict(h=HANDLE, blob=b'a' * 64 + b'b' * 64, nranks=2, rank=1)
    with raises('p2p_attach: 2 handles of 64 bytes expected'):
        m.p2p_attach([b'a' * 64, b'b' * 63], 2, 0)
    with raises('p2p_attach: 3 handles of 64 bytes expected'):
        m.p2p_attach([b'a' * 64, b'b' * 64], 3, 0)
    assert not fake.calls


def test_debug_loss_rows(m, fake):
    fake.env = dict(B=3)
    scores = np.arange(12, dtype=np.float64).reshape(3, 4) + 0.5
    ds, lossrow = m.debug_loss_rows(scores, 2)
    name, c = fake.only()
    assert name == 'g4r_debug_loss_rows' and c['h'] == HANDLE and (c['count'], c['M']) == (12, 2)
    same(c['scores'], scores.ravel(), np.float32)                           # in: the caller's values, converted
    same(c['lossrow'], [0, 0, 0], np.float32)
    filled(ds, (3, 4), np.float32)                                          # out: the same buffer, a copy of the caller's array
    filled(lossrow, (3,), np.float32)
    assert scores[0, 0] == 0.5
    with raises('scores must be a [batch_size, ldSc] matrix'):
        m.debug_loss_rows(np.zeros(12), 2)
    assert not fake.calls


def test_a_failed_call_raises_the_library_error(m, fake):
    fake.rc, fake.error = 3, 'k is too large (the fake said so)'.encode()
    fake.env = dict(nh=6, nx=0, ncand=3, B=B_)
    calls = [lambda: m.predict_step([3]), lambda: m.recommend_step([3]), lambda: m.recommend_step_filtered([3]),
             lambda: m.recommend_step_filtered([3], oversample=2), lambda: m.recommend_sessions(**HIST),
             lambda: m.recommend_sessions(oversample=2, **HIST), lambda: m.continue_sessions(**HIST), lambda: m.beam_sessions(**HIST),
             lambda: m.similar_items([3]), lambda: m.score_candidates([3], [0, 3], [1, 2, 3]),
             lambda: m.score_candidates_sessions(cand_offs=[0, 1, 2, 3], cand_items=[1, 2, 3], **HIST), lambda: m.set_plan(plan(0)),
             lambda: m.evaluate(plan(0), B_, None, [20], 'standard'),
             lambda: m.recommend_events(plan(0), B_, None, 'standard', np.zeros((T_, B_)), 5, 2), lambda: m.p2p_attach([b'a' * 64], 1, 0),
             lambda: m.debug_loss_rows(np.zeros((B_, 4)), 1)]
    for f in calls:
        with pytest.raises(NativeError, match=re.escape('k is too large (the fake said so)')):
            f()
    assert len(fake.calls) == len(calls)
    assert m.T == 0                                                         # a refused plan is not recorded

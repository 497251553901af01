"""The case table of tests/test_gpu_step_launches.py and of its recorder (tools/record_step_launches.py): shapes and switches that between
them reach every kernel family a training step dispatches on (choose_kernels, g4r_host_model.hpp), and what is recorded of a case --
the `kernels` debug key, n_cu, the launches per kernel slot of a profiled run, a bit digest of an unprofiled run.  Every case runs
T = 37 steps in one call: two 16-step graph replays, one 4-step replay and one eager step where nothing cuts the run shorter."""
import hashlib
import os

import numpy as np

from gru4rec_amd import _native

T = 37
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'step_launches.json')
ML = 8      # G4R_MAX_LAYERS: the `kernels` key holds 4 * ML per-layer values, then 12 scalars
BPR = dict(loss='bpr-max', final_act='elu', final_act_p0=0.5, bpreg=1.0)
XE = dict(loss='cross-entropy', final_act='softmax')
LEAN = dict(BPR, I=700, layers=(32,), B=17, ns=5)


def _case(base, env=None, **kw):
    c = dict(base, **kw)
    c['env'] = dict(env or {})
    return c


# name: I items, layers, B, ns negatives, store_rows (default 64: no refill within T), compact (plan steps), env (read at create),
# ranks (virtual ranks: handles), the other keys are g4r_config fields
CASES = {
    'lean_eager': _case(LEAN, use_graph=0),
    'lean_graph': _case(LEAN),
    'lean_eager_owner_window': _case(LEAN, {'G4R_OWNER_WINDOW': '1'}, use_graph=0),
    'lean_graph_owner_window': _case(LEAN, {'G4R_OWNER_WINDOW': '1'}),
    'lean_two_layers_momentum_dropout_xe_logq': _case(LEAN, layers=(32, 48), momentum=0.3, dropout_p_embed=0.3, logq=1.0, **XE),
    'lean_store_of_5_rows': _case(LEAN, store_rows=5),
    'lean_store_of_5_rows_eager_owner_window': _case(LEAN, {'G4R_OWNER_WINDOW': '1'}, store_rows=5, use_graph=0),
    'lean_two_compactions': _case(LEAN, compact=(9, 22)),
    'no_lean': _case(LEAN, {'G4R_NO_LEAN': '1'}),
    'no_lean_eager': _case(LEAN, {'G4R_NO_LEAN': '1'}, use_graph=0),
    'no_lean_no_merge': _case(LEAN, {'G4R_NO_LEAN': '1', 'G4R_NO_MERGE': '1'}, momentum=0.2),
    'no_lean_deferred': _case(LEAN, {'G4R_NO_LEAN': '1', 'G4R_DEFER': '1', 'G4R_LEAN_UPDATE': '0'}),
    'deferred_eager': _case(LEAN, {'G4R_DEFER': '1', 'G4R_LEAN_UPDATE': '0'}, use_graph=0),
    'mid_width': _case(BPR, I=900, layers=(160,), B=48, ns=64),
    'wide_256': _case(BPR, I=3000, layers=(256,), B=64, ns=1024),
    'wide_512': _case(BPR, I=3000, layers=(512,), B=64, ns=1024),
    'score_bwd2': _case(BPR, I=4000, layers=(64,), B=192, ns=1856),
    'score_t2_bwd_w': _case(BPR, I=6000, layers=(48,), B=256, ns=3840),
    'score_k64': _case(BPR, I=6000, layers=(36,), B=256, ns=3840),
    'score_mt_bmt': _case(BPR, I=9000, layers=(256,), B=512, ns=8192),
    'onehot': _case(XE, I=700, layers=(64,), B=32, ns=0, embed_mode=2),
    'embedding_260': _case(BPR, I=700, layers=(64,), B=32, ns=32, embed_mode=1, embedding=260),
    'embedding_516_momentum': _case(BPR, I=700, layers=(64,), B=32, ns=32, embed_mode=1, embedding=516, momentum=0.2),
    'generic_rmsprop': _case(LEAN, adapt='rmsprop', adapt_p0=0.9, adapt_p1=1e-6),
    'generic_adam': _case(LEAN, adapt='adam', adapt_p0=0.9, adapt_p1=0.999, learning_rate=0.01),
    'generic_adagrad_grad_cap': _case(LEAN, grad_cap=0.5),
    'generic_adagrad_grad_cap_eager': _case(LEAN, grad_cap=0.5, use_graph=0),
    'staged_local': _case(LEAN, {'G4R_FORCE_STAGED': '1'}),
    'virtual_ranks': _case(LEAN, ranks=2),
    'virtual_ranks_exact': _case(LEAN, ranks=2, sparse_exact=3),
}
# the cases whose digest has to exist (a run at the parent commit repeats its bits)
MANDATORY = [n for n in CASES if n.startswith(('lean', 'no_lean', 'mid_', 'wide_', 'generic_', 'staged_'))]
_SWITCHES = ('G4R_OWNER_WINDOW', 'G4R_OWNER_SCAN', 'G4R_NO_LEAN', 'G4R_NO_MERGE', 'G4R_DEFER', 'G4R_LEAN_UPDATE', 'G4R_FORCE_STAGED',
             'G4R_NO_MT', 'G4R_NO_BMT', 'G4R_WIDE2', 'G4R_P2_GEO', 'G4R_BA_GEO', 'G4R_SKIP_KN', 'G4R_TRACE', 'G4R_SCORE_B_SPLIT')


class _env:
    """The switches g4r_create reads: those of the case set, every other one unset; put back afterwards."""
    def __init__(self, kv):
        self.kv = {k: kv.get(k) for k in _SWITCHES}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        self._set(self.kv)

    def __exit__(self, *a):
        self._set(self.old)

    @staticmethod
    def _set(kv):
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _shapes(c):
    D = list(c['layers'])
    mode = c.get('embed_mode', 0)
    ein = D[-1] if mode == 0 else (c['embedding'] if mode == 1 else 3 * D[0])
    ins = [0 if mode == 2 else ein] + D[:-1]
    return D, ins, ein


def make_model(name, rank=0):
    """The device model of case `name` (handle `rank` of its virtual ranks) with seeded random weights and its plan uploaded."""
    c = CASES[name]
    I, B, ns, nranks = c['I'], c['B'], c['ns'], c.get('ranks', 1)
    D, ins, ein = _shapes(c)
    rows = c.get('store_rows', 64)
    with _env(c['env']):
        m = _native.Model(
            n_items=I, layers=D, batch_size=B, n_sample=ns, loss=_native.LOSS_IDS[c['loss']], final_act=_native.ACT_IDS[c['final_act']],
            final_act_p0=c.get('final_act_p0', 0.0), hidden_act=_native.ACT_IDS['tanh'], embed_mode=c.get('embed_mode', 0),
            embedding=c.get('embedding', 0), learning_rate=c.get('learning_rate', 0.05), momentum=c.get('momentum', 0.0),
            bpreg=c.get('bpreg', 0.0), logq=c.get('logq', 0.0), adapt=_native.ADAPT_IDS[c.get('adapt', 'adagrad')],
            adapt_p0=c.get('adapt_p0', 0.0), adapt_p1=c.get('adapt_p1', 0.0), grad_cap=c.get('grad_cap', 0.0), sample_alpha=0.5,
            dropout_p_embed=c.get('dropout_p_embed', 0.0), sample_store=rows * ns, seed=3, device=0, rank=rank, nranks=nranks,
            use_graph=c.get('use_graph', 1), sparse_exact=c.get('sparse_exact', 0))
    try:
        rng = np.random.RandomState(5)      # (every rank the same weights; its own plan below)

        def rnd(*shape):
            return ((rng.rand(*shape) - 0.5) * (2.0 * np.sqrt(6.0 / sum(shape)))).astype(np.float32)
        for l, (Dl, INl) in enumerate(zip(D, ins)):
            if INl:
                m.set_param('Wx', rnd(INl, 3 * Dl), l)
            m.set_param('Wh', rnd(Dl, Dl), l)
            m.set_param('Wrz', rnd(Dl, 2 * Dl), l)
            m.set_param('Bh', (rng.randn(3 * Dl) * 0.1).astype(np.float32), l)
            m.set_param('H', (rng.randn(B, Dl) * 0.3).astype(np.float32), l)
        m.set_param('Wy', rnd(I, D[-1]))
        m.set_param('By', (rng.randn(I) * 0.1).astype(np.float32))
        if c.get('embed_mode', 0):
            m.set_param('E', rnd(I, ein))
        support = rng.randint(1, 40, size=I).astype(np.float64)
        pop = support ** 0.5
        pop = pop.cumsum() / pop.sum()
        pop[-1] = 1
        m.set_popularity(pop.astype(np.float32), np.log(support).astype(np.float32), np.log(support ** 0.5).astype(np.float32))
        prng = np.random.RandomState(100 + rank)
        M = np.full(T, B, dtype=np.int32)
        M[T // 2:] = max(1, B - 3)      # a ragged tail
        plan = dict(in_idx=prng.randint(0, I, size=(T, B)).astype(np.int32), out_idx=prng.randint(0, I, size=(T, B)).astype(np.int32),
                    reset=(prng.rand(T, B) < 0.25).astype(np.uint8), M=M, T=T, n_compact=0, compact_steps=np.zeros(0, dtype=np.int64),
                    compact_maps=np.zeros((0, B), dtype=np.int32))
        plan['out_idx'][:, 1] = plan['out_idx'][:, 0]      # an item twice among the targets, one in both lists: owners with lists
        plan['in_idx'][:, 2] = plan['out_idx'][:, 3]
        steps = c.get('compact', ())
        if steps:
            plan['n_compact'] = len(steps)
            plan['compact_steps'] = np.asarray(steps, dtype=np.int64)
            plan['compact_maps'] = np.stack([prng.permutation(B) for _ in steps]).astype(np.int32)
        m.set_plan(plan)
        return m
    except Exception:
        m.close()
        raise


def _run(name, profile):
    c = CASES[name]
    ms = [make_model(name, r) for r in range(c.get('ranks', 1))]
    try:
        if profile:
            ms[0].profile(profile)
        if len(ms) > 1:
            _native.virtual_train_steps(ms, 0, T)
        else:
            ms[0].train_steps(0, T)
        if profile:
            return {k: int(v[1]) for k, v in ms[0].kernel_times().items()}
        D, ins, ein = _shapes(c)
        h = hashlib.sha256()
        for m in ms:
            arrs = [m.get_losses(0, T), m.get_param('Wy', (c['I'], D[-1])), m.get_param('acc_Wy', (c['I'], D[-1])),
                    m.get_param('Wx', (ins[0] or c['I'], 3 * D[0]), 0), m.get_param('Wh', (D[0], D[0]), 0),
                    m.get_param('Wrz', (D[0], 2 * D[0]), 0)]
            for a in arrs:
                h.update(np.ascontiguousarray(a, dtype=np.float32).tobytes())
        return h.hexdigest()
    finally:
        for m in ms:
            m.close()


def describe(name):
    """(`kernels` key as a list of ints, n_cu) of case `name`."""
    m = make_model(name)
    try:
        return [int(v) for v in m.get_debug('kernels', 4 * ML + 12)], int(m.get_debug('n_cu', 1)[0])
    finally:
        m.close()


def merged_update(kernels):
    return kernels[4 * ML + 8] != 2      # UpdateKind: not UP_SPLIT


def record(name):
    """What the golden file holds of case `name`, from this library: one unprofiled run (the digest), one with profile(1) and, where
    the update is one merged launch, one with profile(2).  Virtual ranks do no profiling."""
    kernels, n_cu = describe(name)
    rec = {'kernels': kernels, 'n_cu': n_cu, 'digest': _run(name, 0)}
    if CASES[name].get('ranks', 1) == 1:
        rec['launches'] = _run(name, 1)
        if merged_update(kernels):
            rec['launches_split'] = _run(name, 2)
    return rec

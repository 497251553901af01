"""GRU4Rec on MI355X: the reference's `GRU4Rec` class surface over hand-written gfx950 kernels.

Mirrors hidasib/GRU4Rec `gru4rec.py` (class GRU4Rec :27; __init__ :97-135; set_params :162-187;
fit :515-664; predict_next_batch :665-728; savemodel/loadmodel :742-781) so that `run.py -g
gru4rec_amd.gru4rec` / `evaluation.evaluate_gpu` keep working, but nothing here builds a Theano graph:
`fit` turns the session-parallel loop into an epoch plan (host scheduler, C++), uploads it once and
lets the device run whole epochs without a host round trip (libgru4rec_hip.so through ctypes).

There is deliberately no CPU fallback.
"""
import os
import pickle
import sys
import time
from collections import OrderedDict  # noqa: F401  (kept: parameter files use it)

import numpy as np
import pandas as pd

from . import _native, datatools, eventio
from .plan import build_rank_plan, pad_plan

_PLAIN_ACTS = ('linear', 'relu', 'tanh', 'softmax')


def _parse_act(name, allow_softmax):
    """'elu-0.5' -> (act id, p0, p1); unknown names raise NotImplementedError (gru4rec.py:144-161)."""
    if name in _PLAIN_ACTS:
        if name == 'softmax' and not allow_softmax:
            raise NotImplementedError
        return _native.ACT_IDS[name], 0.0, 0.0
    if name == 'softmax_logit' and allow_softmax:      # final activation only (gru4rec.py:149)
        return _native.ACT_IDS[name], 0.0, 0.0
    for prefix, npar in (('leaky-', 1), ('elu-', 1), ('selu-', 2)):
        if name.startswith(prefix):
            p = [float(x) for x in name.split('-')[1:]]
            if len(p) < npar:
                raise NotImplementedError
            return _native.ACT_IDS[prefix[:-1]], p[0], (p[1] if npar == 2 else 0.0)
    raise NotImplementedError


def _pad4(n):
    return (int(n) + 3) // 4 * 4


def _pad_cols(a, nblk, D, Dp):
    """(…, nblk * D) -> (…, nblk * Dp): every one of the nblk column blocks gets Dp - D zero columns."""
    if D == Dp:
        return a
    a = np.asarray(a)
    out = np.zeros(a.shape[:-1] + (nblk * Dp,), dtype=a.dtype)
    for b in range(nblk):
        out[..., b * Dp:b * Dp + D] = a[..., b * D:(b + 1) * D]
    return out


def _strip_cols(a, nblk, D, Dp):
    if D == Dp:
        return a
    return np.concatenate([a[..., b * Dp:b * Dp + D] for b in range(nblk)], axis=-1)


def _markers(*names):
    """Methods that only carry a name (a bound method pickles as getattr(obj, __name__))."""
    out = []
    for name in names:
        def f(self, *a, **k):
            raise NotImplementedError('symbolic Theano expression in the reference; computed by the HIP kernels here')
        f.__name__ = name
        f.__qualname__ = 'GRU4Rec.' + name
        out.append(f)
    return out


def _check_k(k, n_sel=None, name='k', cap=_native.G4R_TOPK_MAX, bools=False, own_errors=False):
    """The k (or beams) of a selection, checked, as an int: an integer in [1, min(n_sel, cap)]; n_sel None (score_candidates*, whose
    lists have their own lengths and whose k may also be None): in [1, cap].  bools: True counts as 1.  own_errors: what int() itself
    refuses (a string, None) is refused with this message too; otherwise int's own ValueError / TypeError is let through."""
    try:
        ok = (bools or not isinstance(k, bool)) and int(k) == k and 1 <= k <= (cap if n_sel is None else min(n_sel, cap))
    except (TypeError, ValueError):
        if not own_errors:
            raise
        ok = False
    if not ok and n_sel is None:
        raise ValueError('%s = %r: it must be None or an integer in [1, %d]' % (name, k, cap))
    if not ok:
        raise ValueError('%s = %r: it must be an integer in [1, min(number of candidates = %d, %d)]' % (name, k, n_sel, cap))
    return int(k)


def _check_steps(steps):
    try:
        ok = not isinstance(steps, bool) and int(steps) == steps and steps >= 1
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError('steps = %r: it must be an integer >= 1' % (steps,))
    return int(steps)


def _check_temperature(temperature):
    """The temperature of sample_sessions / session_log_partition, checked, as a float32."""
    try:
        with np.errstate(all='ignore'):
            t32 = np.float32(temperature) if not isinstance(temperature, (bool, str)) else np.float32('nan')
            ok = bool(np.isfinite(t32) and t32 > 0 and np.isfinite(np.float32(1) / t32))
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError('temperature = %r: it must be a finite float > 0 (as a float32, with a finite reciprocal); the greedy limit '
                         'temperature -> 0 is continue_sessions(k=1)' % (temperature,))
    return t32


LSE_CAND_MAX = 2 ** 24      # G4R_LSE_CAND_MAX: with more candidate positions the exact 64-bit row normaliser could overflow


def _check_lse_candidates(n_cand):
    if n_cand > LSE_CAND_MAX:
        raise ValueError('%d candidate positions: log-probabilities, top_p and session_log_partition take at most 2^24 (the row '
                         'normaliser is an exact 64-bit integer)' % n_cand)


def _scan_kw(over):      # the keyword of the device model's two-stage selection; the exact one is called without it
    return {} if over is None else dict(oversample=over)


class GRU4Rec:
    """Same constructor arguments and defaults as the reference (gru4rec.py:97-101)."""

    accepts_categorical_items = True      # fit / evaluate_gpu take tables from eventio.read_events (run.py asks)

    def __init__(self, loss='bpr-max', final_act='linear', hidden_act='tanh', layers=[100],
                 n_epochs=10, batch_size=32, dropout_p_hidden=0.0, dropout_p_embed=0.0, learning_rate=0.1,
                 momentum=0.0, lmbd=0.0, embedding=0, n_sample=2048, sample_alpha=0.75, smoothing=0.0,
                 constrained_embedding=False, adapt='adagrad', adapt_params=[], grad_cap=0.0, bpreg=1.0, logq=0.0,
                 sigma=0.0, init_as_normal=False, train_random_order=False, time_sort=True,
                 session_key='SessionId', item_key='ItemId', time_key='Time'):
        self.layers = layers
        self.n_epochs = n_epochs
        self.batch_size = batch_size
        self.dropout_p_hidden = dropout_p_hidden
        self.dropout_p_embed = dropout_p_embed
        self.learning_rate = learning_rate
        self.adapt_params = adapt_params
        self.momentum = momentum
        self.sigma = sigma
        self.init_as_normal = init_as_normal
        self.session_key = session_key
        self.item_key = item_key
        self.time_key = time_key
        self.grad_cap = grad_cap
        self.bpreg = bpreg
        self.logq = logq
        self.train_random_order = train_random_order
        self.lmbd = lmbd
        self.embedding = self.layers[0] if embedding == 'layersize' else embedding
        self.constrained_embedding = constrained_embedding
        self.time_sort = time_sort
        self.adapt = adapt
        self.loss = loss
        self.set_loss_function(self.loss)
        self.final_act = final_act
        self.set_final_activation(self.final_act)
        self.hidden_act = hidden_act
        self.set_hidden_activation(self.hidden_act)
        self.n_sample = n_sample
        self.sample_alpha = sample_alpha
        self.smoothing = smoothing
        # ---- MI355X-path extras (not in the reference)
        self.seed = 12345            # Philox key (the reference's MRG default seed is 12345 as well)
        self.device = 0
        self.use_graph = True
        self.steps_per_call = 16384  # plan steps per C-ABI call (NaN check granularity)
        # multi-GPU runs: the GPU-local item tables are reconciled every `sync_every` steps and at the end of every epoch.  Measured
        # with virtual ranks (profiles/r03_virtual_ranks.json): reconciling only per epoch lets the replicas'
        # embedding spaces drift apart under the shared (all-reduced) GRU weights -- Recall@20 0.41 -> 0.15 at two ranks.  'auto':
        # 4 steps at two ranks (every 16: 0.20, every 4: 0.40 against 0.41 on one rank), 16 from three ranks on (four / eight ranks lose
        # 0.01 - 0.015 against every 4 and the exchange moves about the whole table each time); an integer is taken as given, 0 / None
        # reconciles at the end of the epoch only
        self.sync_every = 'auto'
        # multi-GPU runs, the other way to keep the replicas together: sparse_exact = True all-gathers every rank's per-occurrence
        # gradient rows of the gathered item rows EVERY step and every rank applies all of them in rank order with the reference's
        # duplicate semantics (gru4rec.py:335-340,407-431 over the concatenated occurrence list): the item tables never diverge, there
        # is nothing to reconcile and no sync_every to choose (SURVEY 8e option 3).  Costs an all-gather of R x D floats per rank and
        # step and needs nranks x (2 batch_size + n_sample) list entries in LDS: for small-catalogue shapes.
        # All ranks then draw the SAME negatives (one sample stream: the global batch shares its row of negatives, as the reference's
        # batch does, gru4rec.py:436-437).  True / 'reduce': the gradient rows of the shared negatives are SUMMED over the ranks (what
        # an all-reduce would give), the ranks' input / target occurrences are listed one rank behind the other, everything scaled to
        # the global batch -- the occurrence list of ONE batch of nranks x batch_size rows, updated as the reference updates its batch
        # EXCEPT that a row is scored against its own rank's batch_size in-batch negatives only (the hidden states live on their
        # ranks), not against all nranks x batch_size targets.  Kept for the A/B of DESIGN.md section 7: 'mean' (every rank's occurrences listed, an item's increment = the mean
        # over the ranks touching it) and 'sum' (every occurrence of every rank applied like a duplicate: diverges from four ranks on)
        self.sparse_exact = False
        # single GPU, Adagrad without momentum / lmbd: row updates whose item is not gathered again inside the current window of 16 steps
        # wait for ONE flush launch per window (g4r_config::defer_updates).  Results are bit-identical to the immediate update on the same
        # (merged k_update) kernel; where the default immediate mode takes the lean k_update_l instead (batches of <= 128 rows, item rows
        # of <= 256 floats), it sums the dense gradients in another order, so the two modes agree to fp32 rounding, not to the bit.  The
        # flush launch runs at ~60 % of the HBM peak at BASELINE configs[2] -- and the step gets 2-5 % slower: off
        # unless asked for
        self.defer_updates = False
        # item groups (set_item_groups): int32[n_items] aligned with itemidmap, -1 = ungrouped, and the labels in group-index order
        self.item_groups = None
        self.group_labels = None
        self._model = None
        self._store = None      # the open session store (open_session_store)
        self._dist = None
        self._cpu_store = False
        self.loss_history = []
        self.optimizer_state = None   # filled by savemodel(fname, optimizer_state=True); read by fit(resume=True)
        self.epochs_done = 0

    # ------------------------------------------------------------------ validation of names
    # The reference keeps its loss / activation as bound methods (`self.loss_function = self.bpr_max`, gru4rec.py:136-161)
    # and pickles them with the model (:742-756).  The same attribute names are kept here so that checkpoints travel both
    # ways (a pickle written by either implementation names `gru4rec.GRU4Rec` and these methods); the methods themselves
    # are markers: the arithmetic lives in the HIP kernels (k_loss_rows, act_fwd).
    linear, tanh, softmax, softmax_logit, softmax_neg, relu, sigmoid = _markers(
        'linear', 'tanh', 'softmax', 'softmax_logit', 'softmax_neg', 'relu', 'sigmoid')
    cross_entropy, cross_entropy_logits, bpr, bpr_max, top1, top1_max = _markers(
        'cross_entropy', 'cross_entropy_logits', 'bpr', 'bpr_max', 'top1', 'top1_max')

    class Selu:
        def __init__(self, lmbd, alpha):
            self.lmbd, self.alpha = lmbd, alpha

        def execute(self, X):
            raise NotImplementedError

    class Elu:
        def __init__(self, alpha):
            self.alpha = alpha

        def execute(self, X):
            raise NotImplementedError

    class LeakyReLU:
        def __init__(self, leak):
            self.leak = leak

        def execute(self, X):
            raise NotImplementedError

    _LOSS_METHODS = {'cross-entropy': 'cross_entropy', 'bpr': 'bpr', 'bpr-max': 'bpr_max', 'top1': 'top1',
                     'top1-max': 'top1_max', 'xe_logit': 'cross_entropy_logits'}

    def _act_callable(self, name):
        if name in ('linear', 'relu', 'tanh', 'softmax', 'softmax_logit'):
            return getattr(self, name)
        p = [float(x) for x in name.split('-')[1:]]
        if name.startswith('leaky-'):
            return self.LeakyReLU(p[0]).execute
        if name.startswith('elu-'):
            return self.Elu(p[0]).execute
        return self.Selu(*p).execute

    def set_loss_function(self, loss):
        if loss in _native.LOSS_IDS:         # gru4rec.py:136-143
            self._loss_id = _native.LOSS_IDS[loss]
            self.loss_function = getattr(self, self._LOSS_METHODS[loss])
        else:
            raise NotImplementedError

    def set_final_activation(self, final_act):
        self._final = _parse_act(final_act, True)
        self.final_activation = self._act_callable(final_act)

    def set_hidden_activation(self, hidden_act):
        self._hidden = _parse_act(hidden_act, False)
        self.hidden_activation = self._act_callable(hidden_act)

    def set_params(self, **kvargs):
        """String -> typed coercion against the current attribute type, as gru4rec.py:162-187."""
        kw = max(len(str(k)) for k in kvargs.keys())
        vw = max(len(str(v)) for v in kvargs.values())

        def show(k):
            val = getattr(self, k)
            print('SET   {}{}TO   {}{}(type: {})'.format(k, ' ' * (kw - len(k) + 3), val,
                                                          ' ' * (vw - len(str(val)) + 3), type(val)))
        for k, v in kvargs.items():
            if not hasattr(self, k) or k.startswith('_'):
                print('Unkown attribute: {}'.format(k))
                raise NotImplementedError
            cur = getattr(self, k)
            if isinstance(v, str):
                if k == 'adapt_params':
                    v = [float(x) for x in v.split('/')]
                elif isinstance(cur, list):
                    v = [int(x) for x in v.split('/')]
                elif isinstance(cur, bool):
                    if v in ('True', '1'):
                        v = True
                    elif v in ('False', '0'):
                        v = False
                    else:
                        print('Invalid value for boolean parameter: {}'.format(v))
                        raise NotImplementedError
            if k == 'embedding' and v == 'layersize':
                self.embedding = 'layersize'
            setattr(self, k, type(getattr(self, k))(v))
            if k == 'loss':
                self.set_loss_function(self.loss)
            if k == 'final_act':
                self.set_final_activation(self.final_act)
            if k == 'hidden_act':
                self.set_hidden_activation(self.hidden_act)
            show(k)
        if self.embedding == 'layersize':
            self.embedding = self.layers[0]
            show('embedding')
        self._check_limits()      # shapes the MI355X path does not serve are refused here, with the limit, not deep inside fit()

    # Shape limits of the HIP path (the reference has none of them; DESIGN.md section 5 "Limits" says where each comes from)
    MAX_WIDTH = 1024            # units of a GRU layer / of the item embedding: one gathered row = at most four 16-byte quads per lane
    LDS_BYTES = 156 * 1024      # what a workgroup of the step kernels may take of a CU's 160 KB

    def _check_limits(self):
        """NotImplementedError (the reference's way of refusing a configuration, gru4rec.py:143-177) naming the limit."""
        for D in self.layers:
            if _pad4(int(D)) > self.MAX_WIDTH:
                raise NotImplementedError('layers={}: the MI355X path serves GRU layers of up to {} units'.format(self.layers, self.MAX_WIDTH))
        if self.embedding and self.embedding != 'layersize' and _pad4(int(self.embedding)) > self.MAX_WIDTH:
            raise NotImplementedError('embedding={}: the MI355X path serves item embeddings of up to {} units'.format(self.embedding, self.MAX_WIDTH))
        if not self.constrained_embedding and not self.embedding and 3 * _pad4(int(self.layers[0])) > self.MAX_WIDTH:
            raise NotImplementedError('one-hot input (embedding=0, constrained_embedding=False) with layers[0]={}: the rows of Wx[0] are 3 * layers[0] wide '
                                      'and the MI355X path serves rows of up to {} floats (layers[0] <= {}); use constrained_embedding=True or '
                                      'embedding=<size> for wider first layers'.format(self.layers[0], self.MAX_WIDTH, self.MAX_WIDTH // 3 // 4 * 4))
        # one copy of a score row (k_loss_rows) and the step's occurrence list + partial rows (sparse update) live in LDS
        B, ns = int(self.batch_size), int(self.n_sample)
        ld = (B + ns + 15) // 16 * 16
        width = max([_pad4(int(self.layers[-1]))] + ([_pad4(int(self.embedding))] if (self.embedding and self.embedding != 'layersize') else [])
                    + ([3 * _pad4(int(self.layers[0]))] if (not self.constrained_embedding and not self.embedding) else []))
        rpad = ((2 * B + ns + 255) // 256) * 256 + 256
        need = max(4 * (ld + 288), 4 * rpad + 2112 + 32 * (width + 4))
        if need > self.LDS_BYTES:
            raise NotImplementedError('batch_size={} with n_sample={}: the MI355X path keeps a score row ({} columns) and the step\'s list of '
                                      '{} gathered rows in the 160 KB of LDS of a compute unit; that holds about 38,000 rows / columns '
                                      '(e.g. batch_size 512 with n_sample 36,000), fewer with rows wider than 512 units'.format(B, ns, B + ns, 2 * B + ns))

    # ------------------------------------------------------------------ weights (gru4rec.py:252-294)
    def _init_matrix(self, shape):
        sigma = self.sigma if self.sigma != 0 else np.sqrt(6.0 / (shape[0] + shape[1]))
        if self.init_as_normal:
            return np.asarray(np.random.randn(*shape) * sigma, dtype=np.float32)
        return np.asarray(np.random.rand(*shape) * sigma * 2 - sigma, dtype=np.float32)

    def _init_host_weights(self):
        """Same RNG draw order as the reference after np.random.seed(42): [E], per layer 3 Wx blocks, Wh,
        2 Wrz blocks, finally Wy -- so both implementations start from identical weights."""
        np.random.seed(42)
        L = self.layers
        if self.constrained_embedding:
            n_features = L[-1]
        elif self.embedding:
            self.E = self._init_matrix((self.n_items, self.embedding))
            n_features = self.embedding
        else:
            n_features = self.n_items
        self.Wx, self.Wh, self.Wrz, self.Bh, self.H = [], [], [], [], []
        for i, D in enumerate(L):
            n_in = L[i - 1] if i > 0 else n_features
            self.Wx.append(np.hstack([self._init_matrix((n_in, D)) for _ in range(3)]))
            self.Wh.append(self._init_matrix((D, D)))
            self.Wrz.append(np.hstack([self._init_matrix((D, D)) for _ in range(2)]))
            self.Bh.append(np.zeros(3 * D, dtype=np.float32))
            self.H.append(np.zeros((self.batch_size, D), dtype=np.float32))
        self.Wy = self._init_matrix((self.n_items, L[-1]))
        self.By = np.zeros((self.n_items, 1), dtype=np.float32)

    # ------------------------------------------------------------------ native model management
    def _check_supported(self):
        need = {'rmsprop': 1, 'adadelta': 1, 'adam': 2}.get(self.adapt, 0)
        if len(self.adapt_params) < need:
            raise IndexError('adapt={} needs {} value(s) in adapt_params'.format(self.adapt, need))     # the reference indexes adapt_params[0..1]
        if self.smoothing and self.loss not in ('cross-entropy', 'xe_logit'):
            raise NotImplementedError('smoothing is only defined for cross-entropy / xe_logit (gru4rec.py:226-235)')
        self._check_limits()

    def _create_model(self, sample_store, batch_size=None):
        self._check_supported()
        if self.adapt == 'adadelta' and self.learning_rate != 1.0:      # gru4rec.py:362-364
            print('Warn: learning_rate is not 1.0 while using adadelta. Setting learning_rate to 1.0')
            self.learning_rate = 1.0
        nranks = self._dist['nranks'] if self._dist else 1
        rank = self._dist['rank'] if self._dist else 0
        m = _native.Model(
            n_items=int(self.n_items), layers=[_pad4(D) for D in self.layers], batch_size=int(batch_size or self.batch_size),
            n_sample=int(self.n_sample), loss=self._loss_id,
            final_act=self._final[0], final_act_p0=self._final[1], final_act_p1=self._final[2],
            hidden_act=self._hidden[0], hidden_act_p0=self._hidden[1], hidden_act_p1=self._hidden[2],
            embed_mode=_native.EMBED_CONSTRAINED if self.constrained_embedding else (
                _native.EMBED_SEPARATE if self.embedding else _native.EMBED_ONEHOT),
            embedding=_pad4(self.embedding or 0), learning_rate=self.learning_rate, momentum=self.momentum,
            lmbd=self.lmbd, bpreg=self.bpreg, logq=self.logq, sample_alpha=self.sample_alpha, smoothing=float(self.smoothing),
            adapt=_native.ADAPT_IDS.get(self.adapt, _native.ADAPT_IDS[None]),      # any other value: plain SGD (gru4rec.py:392-399 fall through)
            adapt_p0=float(self.adapt_params[0]) if len(self.adapt_params) > 0 else 0.0,
            adapt_p1=float(self.adapt_params[1]) if len(self.adapt_params) > 1 else 0.0, grad_cap=float(self.grad_cap),
            dropout_p_hidden=self.dropout_p_hidden, dropout_p_embed=self.dropout_p_embed,
            # sample stream: every rank its own (GPU-local mode: more distinct negatives per global step), or -- exact-replica mode --
            # ONE stream for all ranks: the global batch then shares one row of negatives per step, as the reference's batch does
            # (gru4rec.py:436-437), and every sampled item is touched by all ranks, whose increments are averaged
            sample_store=int(sample_store), seed=int(self.seed) + (0 if self.sparse_exact else 7919 * rank), device=int(self.device),
            rank=rank, nranks=nranks, use_graph=1 if self.use_graph else 0,
            sparse_exact=({'sum': 1, 'mean': 2, 'reduce': 3}.get(self.sparse_exact, 3) if (self.sparse_exact and nranks > 1) else 0),
            defer_updates=1 if getattr(self, 'defer_updates', False) else 0)
        if getattr(self, 'defer_updates', False) and not m.get_debug('defer_stats', 4)[2]:
            import warnings
            warnings.warn('defer_updates is set but cannot apply to this model (it needs a single GPU, Adagrad without momentum, lmbd = 0, '
                          'no grad_cap): row updates are applied every step as usual')
        if self._dist and self._dist['unique_id'] is not None:
            m.comm_init(self._dist['unique_id'], nranks, rank)
            if nranks > 1:
                # every rank holds the communicator once this max-reduce returns: the rendezvous file has done its job and goes
                # now, not after fit() (a crash during training must not leave an id behind for the next run to read)
                from . import launch
                launch.barrier(m)
                launch.cleanup(rank)
            if os.environ.get('G4R_P2P') == '1' and nranks <= 8:
                # the switch next to the RCCL all-reduce: every rank reads its peers' gradients over xGMI itself (g4r_p2p_enable)
                m.p2p_enable()
        if getattr(self, 'item_groups', None) is not None:
            m.set_item_groups(self.item_groups)
        return m

    # ---- device layout: the library wants layer / embedding widths that are multiples of 4 (16-byte rows).  Other widths are
    # padded with zero columns / rows on the way to the device and stripped on the way back.  A padded unit has zero weights in
    # and out, so its activation is act(0) = 0, its state stays 0, and every gradient, accumulator and update that touches it
    # is exactly 0 (g = 0 gives a zero step under every `adapt`): the computation on the real units is unchanged.
    def _dev_spec(self, name, layer):
        """(rows, padded rows, column blocks, block width, padded block width) of a parameter array; rows = None for vectors."""
        base = name.split('_', 1)[1] if name.split('_', 1)[0] in ('acc', 'vel', 'acc2', 'cnt') else name
        L = self.layers
        D = L[layer] if base in ('Wx', 'Wh', 'Wrz', 'Bh', 'H') else L[-1]
        if base == 'Wx':
            if layer > 0:
                n_in = L[layer - 1]
            elif self.constrained_embedding:
                n_in = L[-1]
            elif self.embedding:
                n_in = self.embedding
            else:
                return self.n_items, self.n_items, 3, D, _pad4(D)      # one-hot input: Wx[0] is the (n_items, 3D) row table
            return n_in, _pad4(n_in), 3, D, _pad4(D)
        if base == 'Wh':
            return D, _pad4(D), 1, D, _pad4(D)
        if base == 'Wrz':
            return D, _pad4(D), 2, D, _pad4(D)
        if base == 'Bh':
            return None, None, 3, D, _pad4(D)
        if base == 'H':
            return None, None, 1, D, _pad4(D)      # rows = batch: taken from the array
        if base == 'Wy':
            return self.n_items, self.n_items, 1, D, _pad4(D)
        if base == 'E':
            return self.n_items, self.n_items, 1, self.embedding, _pad4(self.embedding)
        if base == 'By':
            return None, None, 1, 1, 1
        raise KeyError(name)

    def _dev_put(self, m, name, arr, layer=0):
        rows, rows_p, nblk, D, Dp = self._dev_spec(name, layer)
        a = _pad_cols(np.asarray(arr, dtype=np.float32), nblk, D, Dp) if name.split('_')[-1] != 'By' else np.asarray(arr, dtype=np.float32).reshape(-1)
        if rows is not None and rows_p != rows:
            a = np.concatenate([a, np.zeros((rows_p - rows, a.shape[1]), dtype=np.float32)])
        m.set_param(name, a, layer)

    def _dev_get(self, m, name, shape, layer=0):
        rows, rows_p, nblk, D, Dp = self._dev_spec(name, layer)
        if name.split('_')[-1] == 'By':
            return m.get_param(name, (self.n_items,), layer).reshape(shape)
        if rows is None:
            pshape = tuple(shape[:-1]) + (nblk * Dp,)
        else:
            pshape = (rows_p, nblk * Dp)
        a = _strip_cols(m.get_param(name, pshape, layer), nblk, D, Dp)
        if rows is not None and rows_p != rows:
            a = a[:rows]
        return np.ascontiguousarray(a).reshape(shape)

    def _upload_weights(self, m):
        for i in range(len(self.layers)):
            self._dev_put(m, 'Wx', self.Wx[i], i)
            self._dev_put(m, 'Wh', self.Wh[i], i)
            self._dev_put(m, 'Wrz', self.Wrz[i], i)
            self._dev_put(m, 'Bh', self.Bh[i], i)
        self._dev_put(m, 'Wy', self.Wy)
        self._dev_put(m, 'By', self.By.reshape(-1))
        if not self.constrained_embedding and self.embedding:
            self._dev_put(m, 'E', self.E)

    def _download_weights(self):
        m = self._model
        L = self.layers
        for i, D in enumerate(L):
            n_in = self.Wx[i].shape[0]
            self.Wx[i] = self._dev_get(m, 'Wx', (n_in, 3 * D), i)
            self.Wh[i] = self._dev_get(m, 'Wh', (D, D), i)
            self.Wrz[i] = self._dev_get(m, 'Wrz', (D, 2 * D), i)
            self.Bh[i] = self._dev_get(m, 'Bh', (3 * D,), i)
            self.H[i] = self._dev_get(m, 'H', (m.cfg.batch_size, D), i)
        self.Wy = self._dev_get(m, 'Wy', (self.n_items, L[-1]))
        self.By = self._dev_get(m, 'By', (self.n_items,)).reshape(-1, 1)
        if not self.constrained_embedding and self.embedding:
            self.E = self._dev_get(m, 'E', (self.n_items, self.embedding))

    # ---- optimizer state ("plus new optimizer-state save"; the reference's pickles hold the weights only)
    def _opt_tables(self):
        """(name, layer, shape) of every optimizer-state array the device keeps for this configuration."""
        pre = ['acc_']
        if self.momentum > 0:
            pre.append('vel_')
        if self.adapt in ('adadelta', 'adam'):
            pre.append('acc2_')
        if self.adapt == 'adam':
            pre.append('cnt_')
        if self.adapt not in ('adagrad', 'rmsprop', 'adadelta', 'adam'):
            pre = [p for p in pre if p == 'vel_']      # plain SGD keeps no statistics
        out = []
        L = self.layers
        for p in pre:
            for i, D in enumerate(L):
                out += [(p + 'Wx', i, (self.Wx[i].shape[0], 3 * D)), (p + 'Wh', i, (D, D)), (p + 'Wrz', i, (D, 2 * D)), (p + 'Bh', i, (3 * D,))]
            out += [(p + 'Wy', 0, (self.n_items, L[-1])), (p + 'By', 0, (self.n_items,))]
            if not self.constrained_embedding and self.embedding:
                out.append((p + 'E', 0, (self.n_items, self.embedding)))
        return out

    def _download_optimizer_state(self):
        m = self._model
        # np_random_state: the session order of train_random_order comes from NumPy's global stream (np.random.permutation per
        # epoch, gru4rec.py:593), seeded by the weight initialisation; a resumed run has to continue THAT stream
        st = {'arrays': {}, 'global_step': m.global_step(), 'refills': m.refills(), 'np_random_state': np.random.get_state(),
              'config': self._opt_config()}
        for name, layer, shape in self._opt_tables():
            st['arrays'][(name, layer)] = self._dev_get(m, name, shape, layer)
        return st

    def _opt_config(self):
        """What the saved optimizer state is a function of: resuming under another value of any of these would either not find its
        arrays or silently drop some (e.g. the velocities when momentum goes to 0)."""
        return dict(adapt=self.adapt, adapt_params=[float(x) for x in self.adapt_params], momentum=float(self.momentum),
                    layers=[int(x) for x in self.layers], embedding=int(self.embedding or 0),
                    constrained_embedding=bool(self.constrained_embedding), batch_size=int(self.batch_size), n_sample=int(self.n_sample))

    def _upload_optimizer_state(self, m, st):
        for name, layer, shape in self._opt_tables():
            self._dev_put(m, name, st['arrays'][(name, layer)], layer)
        m.set_step_counters(st['global_step'], st['refills'])

    def set_distributed(self, rank, nranks, unique_id):
        """One process per GPU: sessions are sharded round-robin over ranks, dense GRU gradients are
        all-reduced with RCCL every step, embedding rows stay GPU-local.
        unique_id = None: a virtual rank (gru4rec_amd/virtual_ranks.py: several handles of ONE process stand in for the ranks; no
        communicator is created and the caller steps the handles together)."""
        # (a one-rank layout with an id: the N > 1 data path on a one-rank communicator, G4R_FORCE_STAGED=1 -- tests)
        self._dist = dict(rank=int(rank), nranks=int(nranks), unique_id=unique_id) if (nranks > 1 or unique_id is not None) else None

    # ------------------------------------------------------------------ training (gru4rec.py:515-664)
    def prepare(self, data, sample_store=10000000, store_type='gpu', resume=False):
        """Everything fit() does before its epoch loop: item map, sort, offsets, weights, popularity tables,
        device model.  Split out so that benchmarks can time the epoch loop alone (the reference's own
        mb/s excludes these as well).  resume=True keeps the weights on this object (a loaded checkpoint) instead of
        initialising them, and restores the optimizer state / step counters saved next to them."""
        if store_type not in ('gpu', 'cpu'):
            print('Invalid store type {}'.format(store_type))
            raise NotImplementedError
        if resume and store_type == 'cpu' and self.n_sample:
            # before anything is built (the reference validates store_type first as well, gru4rec.py:546-555)
            raise NotImplementedError('resume=True with store_type="cpu": the host sampler interleaves its draws with the session '
                                      'order on NumPy\'s global random stream; only the device store (store_type="gpu") resumes')
        self.predict = None
        self.error_during_train = False
        self._drop_session_store()      # the model is replaced
        self.drop_item_index()      # the item map may change
        item_col = data[self.item_key]
        if eventio.is_categorical(item_col):
            # table from eventio.read_events: the category codes already are the indices (no hash join over the events)
            itemids, item_idx = eventio.first_appearance_index(item_col)
            itemidmap = pd.Series(data=np.arange(len(itemids)), index=itemids, name='ItemIdx')
            data['ItemIdx'] = item_idx
        else:
            itemids = item_col.unique()
            itemidmap = pd.Series(data=np.arange(len(itemids)), index=itemids, name='ItemIdx')
            data['ItemIdx'] = itemidmap[item_col.values].values
        if resume:
            if not hasattr(self, 'Wy') or getattr(self, 'optimizer_state', None) is None:
                raise ValueError('resume=True needs a model saved with savemodel(fname, optimizer_state=True)')
            if len(itemids) != self.n_items or not np.array_equal(np.asarray(itemidmap.index), np.asarray(self.itemidmap.index)):
                raise ValueError('resume=True: the training data does not produce the item map of the checkpoint')
            saved_cfg = self.optimizer_state.get('config')
            if saved_cfg is not None and saved_cfg != self._opt_config():
                diff = sorted(k for k in saved_cfg if saved_cfg[k] != self._opt_config().get(k))
                raise ValueError('resume=True: %s differ(s) from the checkpoint (%s), its optimizer state does not apply' % (
                    ', '.join(diff), ', '.join('%s=%r' % (k, saved_cfg[k]) for k in diff)))
            if self.train_random_order and self.optimizer_state.get('np_random_state') is None:
                raise ValueError('resume=True with train_random_order: the checkpoint does not hold the random stream of the session order')
        if getattr(self, 'item_groups', None) is not None and not (
                len(itemids) == len(self.item_groups) and np.array_equal(np.asarray(itemidmap.index), np.asarray(self.itemidmap.index))):
            self.item_groups = self.group_labels = None      # groups of another item map: set them again after fit
        self.n_items = len(itemids)
        self.itemidmap = itemidmap
        datatools.sort_if_needed(data, [self.session_key, self.time_key])
        self._offsets = datatools.compute_offset(data, self.session_key)
        if not resume:
            self._init_host_weights()
            self.optimizer_state = None
            self.epochs_done = 0
        # events per item in itemidmap order: data.groupby(item_key).size()[itemidmap.index] of gru4rec.py:540-541
        support = np.bincount(data['ItemIdx'].values, minlength=self.n_items)
        if self._model is not None:
            self._model.close()
        self._model = self._create_model(sample_store)
        m = self._model
        self._upload_weights(m)
        self._cpu_store = bool(store_type == 'cpu' and self.n_sample)
        if self.n_sample and m.sample_store_rows() <= 1:
            print('No example store was used')      # negatives are then drawn anew for every step (gru4rec.py:548-550,614-615)
        lq_t = lq_s = None
        if self.logq:
            p0 = support.astype(np.float32)
            lq_t = np.log(p0)
            lq_s = np.log(p0 ** np.float32(self.sample_alpha))
        pop = support.astype(np.float64) ** self.sample_alpha
        pop = pop.cumsum() / pop.sum()
        pop[-1] = 1
        self._pop64 = pop
        if self._cpu_store:
            # store_type='cpu' (gru4rec.py:551-554): the reference's own host sampler, on NumPy's global stream right behind the
            # weight initialisation -- the negatives are the reference's, draw for draw
            m.set_sample_store(self._cpu_samples(m.sample_store_rows()))
        m.set_popularity(pop.astype(np.float32), lq_t, lq_s)
        if self.n_sample and m.sample_store_rows() > 1:
            print('Created sample store with {} batches of samples (type={})'.format(m.sample_store_rows(), 'CPU' if self._cpu_store else 'GPU'))
        if resume:
            self._upload_optimizer_state(m, self.optimizer_state)
            if self.optimizer_state.get('np_random_state') is not None:
                np.random.set_state(self.optimizer_state['np_random_state'])      # continue the stream of np.random.permutation (:593)
        if self.time_sort:
            # data is ordered by (session, time): a session's first row holds its minimum time (the groupby().min() of
            # gru4rec.py:585-586, sessions in ascending id order)
            self._base_order = np.argsort(data[self.time_key].values[self._offsets[:-1]])
        else:
            self._base_order = np.arange(len(self._offsets) - 1)
        self._data_items = data.ItemIdx.values.astype(np.int32)
        self._plan_key = None
        if not resume:
            self.loss_history = []
        self.step_costs = []          # per-epoch arrays of the per-mini-batch cost (gru4rec.py:623)

    def _cpu_samples(self, length):
        """generate_neg_samples, gru4rec.py:507-514: searchsorted (side='left') in the float64 cumulative table, or a uniform
        choice when sample_alpha == 0; `length` rows of n_sample."""
        if self.sample_alpha:
            sample = np.searchsorted(self._pop64, np.random.rand(self.n_sample * length))
        else:
            sample = np.random.choice(self.n_items, size=self.n_sample * length)
        return sample.reshape(length, self.n_sample).astype(np.int32)

    def _epoch_plan(self):
        n_sessions = len(self._offsets) - 1
        order_all = np.random.permutation(n_sessions) if self.train_random_order else self._base_order
        key = None if self.train_random_order else 'static'
        if key is not None and self._plan_key == key:
            return self._plan
        if self._dist:
            plan = build_rank_plan(self._offsets, order_all, self._data_items, self.batch_size, self.n_sample,
                                   self._dist['rank'], self._dist['nranks'])
            # every rank must issue the same number of all-reduces: the shorter plans are padded with M = 0 steps
            plan = pad_plan(plan, self._model.comm_max(plan['T']))
        else:
            plan = build_rank_plan(self._offsets, order_all, self._data_items, self.batch_size, self.n_sample)
        self._model.set_plan(plan)
        self._plan = plan
        self._plan_key = key
        return plan

    def sync_steps(self, nranks=None):
        """Steps between two reconciliations of the GPU-local item tables for `nranks` ranks (default: this object's layout): the
        `sync_every` attribute, 'auto' resolved as documented there; 0 = only at the end of an epoch."""
        if nranks is None:
            nranks = self._dist['nranks'] if self._dist else 1
        if self.sparse_exact:
            return 0      # exact replicas: nothing to reconcile
        k = self.sync_every
        if k == 'auto':
            # catalogues too large for the on-stream dense reconciliation (item tables > 64 MB per group: the packed-parts exchange moves
            # the rows touched since the last call): every 64 steps.  Measured at a configs[3]-like shape (1 M items, layers [256],
            # B = 512, 8192 negatives, 8 virtual ranks; profiles/r04_virtual_ranks_large.json): Recall@20 0.092 / 0.094 / 0.093 / 0.091 at
            # every 4 / 16 / 64 steps / epoch end -- the ranks' rows rarely collide on a catalogue of that size, what is lost against
            # one rank (0.385) is the 8 x larger global batch (one rank at B = 4096: 0.098) -- while a reconciliation moves 0.20 / 0.55 /
            # 1.21 / 1.57 M rows: 64 keeps the exchange at ~19 K rows per step.
            width = max(_pad4(int(self.layers[-1])), 1)
            if getattr(self, 'n_items', 0) and int(self.n_items) * (2 * width + 2 + 1) * 4 > 64 * 1024 * 1024:
                return 64
            return 4 if nranks == 2 else 16
        if not k:
            return 0
        k = int(k)
        if k < 0:
            raise ValueError('sync_every must be a number of steps, 0 / None or "auto"')
        return k

    def run_epoch(self, epoch, max_steps=None):
        """One pass of the reference's epoch body (gru4rec.py:587-661).  Returns (costs, M per step) or None on NaN."""
        m = self._model
        self._drop_session_store()      # the weights change
        t0 = time.time()
        plan = self._epoch_plan()
        m.reset_hidden()
        T = plan['T'] if max_steps is None else min(plan['T'], max_steps)
        costs = np.empty(T, dtype=np.float32)
        done = 0
        since_sync = 0
        # small item tables are reconciled inside the library (every sync_every steps, between two steps, on the stream); otherwise
        # the calls are cut at those points and g4r_comm_sync_sparse runs in between
        sync_k = self.sync_steps()
        host_sync = bool(self._dist and sync_k) and not m.set_sync_every(sync_k)
        while done < T:
            n = min(self.steps_per_call, T - done)
            if host_sync:
                n = min(n, sync_k - since_sync)      # every rank cuts at the same steps: plans have one common length
            if self._cpu_store:
                # host sample store: the row pointer is the global step modulo the store length; a new store is drawn when it
                # wraps (gru4rec.py:609-613), so no device call runs across that point
                g, gl = m.global_step(), m.sample_store_rows()
                if g > 0 and g % gl == 0:
                    m.set_sample_store(self._cpu_samples(gl))
                n = min(n, gl - g % gl)
            m.train_steps(done, n)
            c = m.get_losses(done, n)
            costs[done:done + n] = c
            bad = bool(np.isnan(c).any())
            if self._dist:
                bad = bool(m.comm_max(int(bad)))      # all ranks leave together: a lone return would hang the others' all-reduce
            if bad:
                print(str(epoch) + ': NaN error!')
                self.error_during_train = True
                return None
            done += n
            since_sync += n
            if host_sync and since_sync >= sync_k and done < T:
                m.comm_sync_sparse()
                since_sync = 0
        cc = plan['M'][:T]
        avgc = np.sum(costs * cc) / max(np.sum(cc), 1)
        bad = bool(np.isnan(avgc))
        if self._dist:
            bad = bool(m.comm_max(int(bad)))      # collective like the per-chunk exit: a lone return would hang the other ranks
        if bad:
            print('Epoch {}: NaN error!'.format(str(epoch)))
            self.error_during_train = True
            return None
        dt = time.time() - t0
        print('Epoch{} --> loss: {:.6f} \t({:.2f}s) \t[{:.2f} mb/s | {:.0f} e/s]'.format(epoch + 1, avgc, dt, T / dt, np.sum(cc) / dt))
        self.loss_history.append(float(avgc))
        self.step_costs.append(costs)
        self.last_epoch_stats = dict(steps=int(T), events=int(np.sum(cc)), seconds=dt, loss=float(avgc))
        return costs, cc

    def fit(self, data, sample_store=10000000, store_type='gpu', resume=False):
        """Trains the network; same contract as the reference's fit (gru4rec.py:515-664): mutates `data`
        (adds ItemIdx, may sort in place), sets n_items / itemidmap / error_during_train.
        resume=True (not in the reference): continue a model loaded from savemodel(fname, optimizer_state=True) on the same
        training data from the epoch it stopped at, up to n_epochs -- bit-identical to the uninterrupted run."""
        self.prepare(data, sample_store=sample_store, store_type=store_type, resume=resume)
        for epoch in range(self.epochs_done if resume else 0, self.n_epochs):
            if self.run_epoch(epoch) is None:
                return
            if self._dist:
                self._model.comm_sync_sparse()
            self.epochs_done = epoch + 1
        self._download_weights()

    def close(self):
        """Releases the device model (parameters stay on the host object); the next predict / fit creates a new one."""
        self._drop_session_store()
        if self._model is not None:
            self._model.close()
            self._model = None
        self._item_index_on = None      # (the index itself stays on this object: the next device model receives it again)
        self.predict = None

    # ------------------------------------------------------------------ prediction (gru4rec.py:665-728)
    def _ensure_model(self):
        if self._model is None:
            self._model = self._create_model(0)
            self._upload_weights(self._model)
        return self._model

    def _predict_plan(self, session_ids, input_item_ids, batch):
        """What _predict_rows will do for this call, computed without changing anything: (restart, session ids, changed, input item
        indices).  restart: the prediction state starts over (first call, new `batch`, or reset by fit / loadmodel / evaluate_gpu)."""
        in_idxs = self.itemidmap[input_item_ids].values
        session_ids = np.asarray(session_ids)
        restart = getattr(self, 'predict', None) is None or self.predict_batch != batch
        changed = session_ids != (np.ones(batch) * -1 if restart else self.current_session)
        return restart, session_ids, changed, in_idxs

    def _predict_rows(self, session_ids, input_item_ids, batch, plan=None):
        """Session bookkeeping of a prediction call (gru4rec.py:712-717), shared by predict_next_batch / recommend_next_batch: (re)starts
        the prediction state for `batch`, zeroes the hidden rows of changed sessions, records the inputs in the seen-history;
        returns (device model, input item indices).  plan: this call's _predict_plan, when the caller has made it already."""
        restart, session_ids, changed, in_idxs = plan if plan is not None else self._predict_plan(session_ids, input_item_ids, batch)
        m = self._ensure_model()
        if restart:
            self.predict_batch = batch
            m.predict_begin(batch)
            self.current_session = np.ones(batch) * -1
            self.predict = True
            self._seen_start(batch)
        if changed.any():
            m.predict_hidden(zero_mask=changed.astype(np.uint8))
            self.current_session = session_ids.copy()
        self._seen_record(changed, in_idxs)
        return m, in_idxs

    # seen-history of recommend_next_batch(exclude_seen=True): the item indices input to every slot since its session began, in a
    # [batch, _SEEN_CAP] buffer with fill counts.  A slot that fills its row is compacted (sorted, de-duplicated) in one vectorised pass;
    # a slot with more than G4R_EXCLUDE_MAX distinct items is marked overflowed (only its later exclude_seen calls refuse).
    _SEEN_CAP = 2 * _native.G4R_EXCLUDE_MAX

    @staticmethod
    def _row_mask(changed, batch):
        out = np.zeros(batch, dtype=bool)
        v = np.ravel(changed)[:batch]
        out[:len(v)] = v
        return out

    def _seen_start(self, batch):
        self._seen = np.zeros((batch, self._SEEN_CAP), dtype=np.int32)
        self._seen_n = np.zeros(batch, dtype=np.int32)
        self._seen_over = np.zeros(batch, dtype=bool)

    def _seen_record(self, changed, in_idxs):
        if getattr(self, '_seen', None) is None or len(self._seen) != self.predict_batch:
            self._seen_start(self.predict_batch)
        reset = self._row_mask(changed, self.predict_batch)
        self._seen_n[reset] = 0
        self._seen_over[reset] = False
        x = np.asarray(in_idxs, dtype=np.int32).ravel()[:self.predict_batch]
        r = len(x)
        if (self._seen_n[:r] >= self._SEEN_CAP).any():
            self._seen_compact()
        self._seen[np.arange(r), self._seen_n[:r]] = x
        self._seen_n[:r] += 1

    def _seen_compact(self):
        pad = np.iinfo(np.int32).max
        s = np.where(np.arange(self._SEEN_CAP) < self._seen_n[:, None], self._seen, pad)
        s.sort(axis=1)
        tail = s[:, 1:]
        tail[tail == s[:, :-1]] = pad
        s.sort(axis=1)
        n = (s != pad).sum(axis=1)
        over = n > _native.G4R_EXCLUDE_MAX
        self._seen_over |= over
        n[over] = 0
        self._seen, self._seen_n = s, n.astype(np.int32)

    def _seen_after(self, plan):
        """(rows, item indices) the seen-history will hold for this call's rows once the call is made (its inputs included)."""
        restart, _, changed, in_idxs = plan
        x = np.asarray(in_idxs, dtype=np.int64).ravel()
        r = len(x)
        rows, items = [np.arange(r)], [x]
        if not restart and getattr(self, '_seen', None) is not None and len(self._seen) >= r:
            fresh = self._row_mask(changed, len(self._seen))[:r]
            over = np.flatnonzero(self._seen_over[:r] & ~fresh)
            if len(over):
                raise ValueError('exclude_seen: row %d has seen more than G4R_EXCLUDE_MAX = %d distinct items in its session'
                                 % (over[0], _native.G4R_EXCLUDE_MAX))
            keep = (np.arange(self._SEEN_CAP) < self._seen_n[:r, None]) & ~fresh[:, None]
            rr, cc = np.nonzero(keep)
            rows.append(rr)
            items.append(self._seen[rr, cc].astype(np.int64))
        return np.concatenate(rows), np.concatenate(items)

    def _exclusions(self, plan, k, cand_idx, exclude_seen, exclude, exclude_per_row):
        """Checks and packs the exclusions of a recommend_next_batch call: (excl_offs, excl_items, excl_mask) of
        g4r_recommend_step_filtered (None where there is nothing to exclude).  Raises before anything changes."""
        seen = self._seen_after(plan) if exclude_seen else None
        return self._pack_exclusions(len(np.ravel(plan[3])), k, cand_idx, seen, 'the items seen', exclude, exclude_per_row)

    def _pack_exclusions(self, rows, k, cand_idx, extra, extra_name, exclude, exclude_per_row, grow=0, exclude_groups=None):
        """_exclusions for `rows` rows; extra: (rows, item indices) the call adds to the per-row lists (the items seen, the
        histories) or None; extra_name names them in the G4R_EXCLUDE_MAX error.  grow (continue_sessions with no_repeat): the items
        every row's list gains on the device, one eligible candidate position each.  exclude_groups: group labels whose items join
        `exclude`."""
        n_items = len(self.itemidmap)
        pr, pi = [np.zeros(0, dtype=np.int64)], [np.zeros(0, dtype=np.int64)]
        if exclude_per_row is not None:
            if len(exclude_per_row) != rows:
                raise ValueError('exclude_per_row holds %d lists, one per row (%d) is needed' % (len(exclude_per_row), rows))
            lists = [x if isinstance(x, np.ndarray) else list(x) for x in exclude_per_row]
            lens = np.array([len(x) for x in lists], dtype=np.int64)
            if lens.sum():
                pr.append(np.repeat(np.arange(rows), lens))
                pi.append(self.itemidmap[np.concatenate([np.ravel(x) for x in lists if len(x)])].values.astype(np.int64))
        if extra is not None:
            pr.append(np.asarray(extra[0], dtype=np.int64))
            pi.append(np.asarray(extra[1], dtype=np.int64))
        gidx, mask = self._global_exclude(exclude, exclude_groups)
        key = np.unique(np.concatenate(pr) * n_items + np.concatenate(pi))
        r, it = key // n_items, key % n_items
        counts = np.bincount(r, minlength=rows)
        big = np.flatnonzero(counts > _native.G4R_EXCLUDE_MAX)
        if len(big):
            raise ValueError('row %d excludes %d distinct items (exclude_per_row and %s), more than G4R_EXCLUDE_MAX = %d'
                             % (big[0], counts[big[0]], extra_name, _native.G4R_EXCLUDE_MAX))
        # eligible candidate positions per row (duplicate positions count): all - masked positions - positions of the row's other items
        if cand_idx is None:
            n_cand, n_masked, per_item = n_items, len(gidx), np.ones(len(it))
        else:
            n_cand, n_masked = len(cand_idx), int(np.isin(cand_idx, gidx).sum())
            uc, cc = np.unique(cand_idx, return_counts=True)
            pos = np.minimum(np.searchsorted(uc, it), max(len(uc) - 1, 0))
            per_item = np.where(uc[pos] == it, cc[pos], 0) if len(uc) else np.zeros(len(it))
        own = ~np.isin(it, gidx)
        elig = n_cand - n_masked - np.bincount(r[own], weights=per_item[own], minlength=rows).astype(np.int64)
        short = np.flatnonzero(elig < k)
        if len(short):
            raise ValueError('row %d has %d eligible candidate positions, fewer than k = %d' % (short[0], elig[short[0]], k))
        if grow:
            big = np.flatnonzero(counts + grow > _native.G4R_EXCLUDE_MAX)
            if len(big):
                raise ValueError('row %d excludes %d distinct items (exclude_per_row and %s) and generates steps - 1 = %d more, more than '
                                 'G4R_EXCLUDE_MAX = %d' % (big[0], counts[big[0]], extra_name, grow, _native.G4R_EXCLUDE_MAX))
            short = np.flatnonzero(elig - grow < k)
            if len(short):
                raise ValueError('row %d has %d eligible candidate positions, fewer than k + steps - 1 = %d (every generated item takes '
                                 'one)' % (short[0], elig[short[0]], k + grow))
        offs = items = None
        if extra is not None or exclude_per_row is not None:
            offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
            items = it.astype(np.int32)
        return offs, items, mask

    def _global_exclude(self, exclude, exclude_groups=None):
        """`exclude`, the item ids excluded in every row, and `exclude_groups`, the group labels all of whose items are, as (their
        distinct item indices, sorted, int64; the bit mask of g4r_recommend_step_filtered over them, None when there are none)."""
        gidx, mask = np.zeros(0, dtype=np.int64), None
        if exclude is not None:
            ex = exclude if isinstance(exclude, np.ndarray) else list(exclude)
            if len(ex):
                gidx = np.unique(self.itemidmap[np.ravel(ex)].values.astype(np.int64))
        if exclude_groups is not None:
            gi = self._group_indices(exclude_groups, 'exclude_groups')
            gidx = np.union1d(gidx, np.flatnonzero(np.isin(self.item_groups, gi))).astype(np.int64)
        if len(gidx):
            mask = np.zeros((len(self.itemidmap) + 31) // 32, dtype=np.uint32)
            np.bitwise_or.at(mask, gidx >> 5, np.left_shift(1, gidx & 31).astype(np.uint32))
        return gidx, mask

    def _session_exclusions(self, N, lens, hidx, k, iidx, history, exclude, exclude_per_row, steps=None, exclude_groups=None):
        """_pack_exclusions for a stateless call over N histories (lengths lens, item indices hidx).  history: every row's list holds
        its own history (exclude_history, no_repeat).  steps (None: the call generates nothing): with history, every row's list gains
        steps - 1 generated items on the device, which needs duplicate-free candidates."""
        if steps is not None and history and iidx is not None and len(np.unique(iidx)) != len(iidx):
            raise ValueError('no_repeat needs duplicate-free predict_for_item_ids: every generated item must take exactly one candidate '
                             'position')
        if not history and exclude is None and exclude_per_row is None and exclude_groups is None:
            return None, None, None
        hist_rows = (np.repeat(np.arange(N), lens), hidx) if history else None
        return self._pack_exclusions(N, k, iidx, hist_rows, 'the history', exclude, exclude_per_row,
                                     grow=steps - 1 if steps is not None and history else 0, exclude_groups=exclude_groups)

    def _n_candidates(self, predict_for_item_ids):
        return len(self.itemidmap) if predict_for_item_ids is None else len(predict_for_item_ids)

    def _candidates(self, predict_for_item_ids):
        """The candidates of a call: (their item indices, None for all items; their ids in candidate order).  An unknown id raises
        KeyError here, which is why the k check, which comes first, takes the count from _n_candidates."""
        if predict_for_item_ids is None:
            return None, self.itemidmap.index.values
        return self.itemidmap[predict_for_item_ids].values, np.asarray(predict_for_item_ids)

    def _unpad_hidden(self, H):      # the states a device call returned (4-padded columns) in the layout of `hidden`
        return [np.ascontiguousarray(_strip_cols(h, 1, D, _pad4(D))) for h, D in zip(H, self.layers)]

    def predict_next_batch(self, session_ids, input_item_ids, predict_for_item_ids=None, batch=100):
        """Scores for the next item of every session in the batch.  Rows: items, columns: batch events."""
        if self.error_during_train:
            raise Exception
        m, in_idxs = self._predict_rows(session_ids, input_item_ids, batch)
        if predict_for_item_ids is not None:
            iidx = self.itemidmap[predict_for_item_ids].values
            preds = m.predict_step(in_idxs, iidx).T
            return pd.DataFrame(data=preds, index=predict_for_item_ids)
        preds = m.predict_step(in_idxs).T
        return pd.DataFrame(data=preds, index=self.itemidmap.index)

    def _scan_oversample(self, scan, oversample, k):
        """The checks of scan / oversample (recommend_next_batch, recommend_sessions), after the k check: None for scan='fp32', the
        checked oversample for scan='bf16'."""
        if scan not in ('fp32', 'bf16'):
            raise ValueError("scan = %r: it must be 'fp32' or 'bf16'" % (scan,))
        cmax = _native.G4R_SCAN_CAND_MAX
        if isinstance(oversample, bool) or int(oversample) != oversample or oversample < 1:
            raise ValueError('oversample = %r: it must be an integer in [1, %d // k]' % (oversample, cmax))
        if scan == 'fp32':
            return None
        if int(k) * int(oversample) > cmax:
            raise ValueError('k * oversample = %d * %d: it must be at most G4R_SCAN_CAND_MAX = %d' % (k, oversample, cmax))
        if self.final_act.startswith('softmax'):
            raise NotImplementedError("scan='bf16' is not implemented for final_act=%r: a softmax value needs the whole row's maximum "
                                      "and sum, which is the fp32 scan again" % self.final_act)
        return int(oversample)

    def recommend_next_batch(self, session_ids, input_item_ids, k=20, predict_for_item_ids=None, batch=100,
                             exclude_seen=False, exclude=None, exclude_per_row=None, scan='fp32', oversample=8):
        """Top-k next items of every session: (item_ids[len(session_ids), k], scores[len(session_ids), k] float32).
        Not in the reference.  Row r holds the k largest entries of column r of what predict_next_batch would return for the same
        call (score descending, equal scores by the lower candidate position, NaN last), the scores bit-identical to it; the
        candidates are all items in itemidmap order, or predict_for_item_ids in the given order.  The hidden state advances as in
        predict_next_batch, so calls of the two may be interleaved.  Selection runs on the device: only k entries per row return.

        Exclusions (the union of the three; by item: every candidate position holding an excluded item is skipped):
          exclude_seen     row r never receives an item input to slot r since that slot's session began (a new session id at that
                           position, a new prediction state: first call, new `batch`, fit / loadmodel / evaluate_gpu), this call's
                           input and inputs of predict_next_batch calls included;
          exclude          item ids excluded in every row;
          exclude_per_row  len(session_ids) iterables of item ids, one per row.
        The rest keep their order and their predict_next_batch scores: softmax / softmax_logit scores are NOT renormalised over them.
        A call is checked before anything changes (hidden state, current_session, seen-history): an unknown item id raises
        KeyError; a row with more than G4R_EXCLUDE_MAX = 1024 distinct items in exclude_per_row plus the items seen, or with fewer
        than k eligible candidate positions (duplicates count), raises ValueError.

        scan='bf16' (opt-in; 'fp32', the default, is the exact selection above) is a two-stage selection for LARGE catalogues
        (millions of items, where the fp32 scoring of every item dominates the call; on catalogues of tens of thousands of items
        the exact call is already bound by its merge and the option gains nothing).  A scan in bf16 (h and Wy rounded to bf16, fp32
        accumulation, bias and activation) keeps c = min(number of candidates, k * oversample) candidates per row, exclusions
        applied; those are scored again in fp32 and the k best returned.  Every returned score still is predict_next_batch's, bit
        for bit, and the order and tie rule are unchanged; only WHICH items were considered is approximate: an item whose bf16 score
        is not among the row's c best cannot appear.  With c >= the row's eligible candidates the result equals scan='fp32'
        exactly.  oversample is an integer >= 1 with k * oversample <= G4R_SCAN_CAND_MAX = 1024 (ValueError otherwise); final_act
        softmax / softmax_logit raise NotImplementedError (their values need the whole row: out of scope).  The hidden state
        advances exactly as with scan='fp32'.  The bf16 copy of Wy is built on the first such call and after every change of Wy."""
        if self.error_during_train:
            raise Exception
        k = _check_k(k, self._n_candidates(predict_for_item_ids), bools=True)
        over = self._scan_oversample(scan, oversample, k)
        plan = self._predict_plan(session_ids, input_item_ids, batch)
        iidx, cand = self._candidates(predict_for_item_ids)
        filtered = exclude_seen or exclude is not None or exclude_per_row is not None
        excl = self._exclusions(plan, k, iidx, exclude_seen, exclude, exclude_per_row) if filtered else ()
        m, in_idxs = self._predict_rows(session_ids, input_item_ids, batch, plan=plan)
        if filtered or over is not None:
            cols, scores = m.recommend_step_filtered(in_idxs, iidx, k, *excl, **_scan_kw(over))
        else:
            cols, scores = m.recommend_step(in_idxs, iidx, k)      # (the unfiltered exact selection is an entry of its own)
        return cand[cols], scores

    # ------------------------------------------------------------------ item index (IVF) of recommend_sessions(nprobe=)
    @staticmethod
    def _index_n_lists(n_lists, n_items):
        """The checked number of lists of an item index over n_items items; None: round(4 * sqrt(n_items))."""
        if n_lists is None:
            n_lists = min(max(int(round(4.0 * np.sqrt(n_items))), 1), n_items, _native.G4R_IVF_LISTS_MAX)
        if isinstance(n_lists, bool) or int(n_lists) != n_lists or not 1 <= n_lists <= min(_native.G4R_IVF_LISTS_MAX, n_items):
            raise ValueError('n_lists = %r: it must be an integer in [1, min(%d, n_items = %d)]' % (n_lists, _native.G4R_IVF_LISTS_MAX, n_items))
        return int(n_lists)

    def _index_checked(self, index):
        """index= of build_item_index (a dict as item_index() returns it), validated: (centroids float32[n_lists, D + 1], list_offs
        int64[n_lists + 1], list_items as item INDICES int32, every list ascending)."""
        n_items, W = len(self.itemidmap), self.layers[-1] + 1
        if not isinstance(index, dict) or not all(key in index for key in ('centroids', 'list_offs', 'list_items')):
            raise ValueError("index must be a dict with 'centroids', 'list_offs' and 'list_items', as item_index() returns it")
        cen = np.asarray(index['centroids'])
        if cen.ndim != 2 or cen.shape[1] != W or cen.dtype != np.float32:
            raise ValueError('index: centroids must be a float32 array [n_lists, %d], not %s %s' % (W, cen.dtype, cen.shape))
        n_lists = self._index_n_lists(cen.shape[0], n_items)
        if not np.isfinite(cen).all():
            raise ValueError('index: centroids must be finite')
        offs = np.asarray(index['list_offs'])
        if offs.ndim != 1 or len(offs) != n_lists + 1 or not np.issubdtype(offs.dtype, np.integer):
            raise ValueError('index: list_offs must hold n_lists + 1 = %d integers' % (n_lists + 1))
        offs = offs.astype(np.int64)
        if offs[0] != 0 or offs[-1] != n_items or (np.diff(offs) < 0).any():
            raise ValueError('index: list_offs must rise monotonically from 0 to n_items = %d' % n_items)
        ids = np.ravel(index['list_items'])
        if len(ids) != n_items:
            raise ValueError('index: list_items must be a permutation of all %d items, it holds %d' % (n_items, len(ids)))
        idx = self.itemidmap[ids].values.astype(np.int64)
        if (np.bincount(idx, minlength=n_items) != 1).any():
            raise ValueError('index: list_items must be a permutation of all %d items (an item is listed twice)' % n_items)
        lst = np.repeat(np.arange(n_lists), np.diff(offs))
        idx = idx[np.lexsort((idx, lst))]      # every list in ascending item index: the order within a list carries nothing
        return np.ascontiguousarray(cen), offs, idx.astype(np.int32)

    def _kmeans(self, n_lists, iters, sample_per_list, seed):
        """Plain Lloyd k-means on the host over a deterministic sample of at most sample_per_list * n_lists item vectors [Wy[i], By[i]]
        (float32); assignment maximises v.c - |c|^2 / 2, equal objectives to the lower list; empty clusters keep their centroid."""
        n = len(self.itemidmap)
        rng = np.random.RandomState(seed)
        S = min(n, int(sample_per_list) * n_lists)
        rows = np.sort(rng.choice(n, S, replace=False)) if S < n else np.arange(n)
        X = np.concatenate([np.asarray(self.Wy, dtype=np.float32)[rows], np.asarray(self.By, dtype=np.float32).reshape(-1, 1)[rows]], axis=1)
        cen = X[np.sort(rng.choice(S, n_lists, replace=False))].copy()
        for _ in range(int(iters)):
            half = 0.5 * (cen.astype(np.float64) ** 2).sum(axis=1).astype(np.float32)
            a = np.empty(S, dtype=np.int64)
            for r0 in range(0, S, 16384):
                a[r0:r0 + 16384] = np.argmax(X[r0:r0 + 16384] @ cen.T - half, axis=1)
            cnt = np.bincount(a, minlength=n_lists)
            sums = np.stack([np.bincount(a, weights=X[:, j], minlength=n_lists) for j in range(X.shape[1])], axis=1)
            full = cnt > 0
            cen[full] = (sums[full] / cnt[full, None]).astype(np.float32)
        return cen

    def build_item_index(self, n_lists=None, iters=10, sample_per_list=64, seed=0, centroids=None, index=None):
        """Builds the item index (an inverted file over the item table) that recommend_sessions(nprobe=) probes.  Not in the reference.
        It needs a fitted or loaded model.  Item i is indexed by v_i = [Wy[i], By[i]] (dimension D + 1): its inner product with [h, 1]
        is the item's logit.  The items are clustered into n_lists lists (None: round(4 * sqrt(n_items)); an integer in [1, 65536], at
        most n_items) by plain Lloyd k-means on the host -- `iters` rounds over a deterministic sample (`seed`) of at most
        sample_per_list * n_lists items, assignment by the largest v.c - |c|^2 / 2, empty clusters keep their centroid -- and every
        item is then assigned to its best list on the device (equal objectives to the lower list).  A list holds its items in
        ascending item index.

          centroids   a float32 array [n_lists, D + 1]: k-means is skipped, only the device assignment runs.
          index       a dict as item_index() returns it: both are skipped.  It is validated (ValueError): list_items must be a
                      permutation of all items, list_offs must hold n_lists + 1 monotone offsets from 0 to n_items, centroids must
                      have the right shape and be finite.  The order of the items within a list carries nothing.

        Returns the statistics of the build: n_lists, list_len_min / list_len_mean / list_len_max, empty_lists, and the seconds spent
        on k-means, on the assignment and on the upload (seconds_kmeans, seconds_assign, seconds_upload).  A work item of the scan
        walks a whole list, so list_len_max against list_len_mean is the skew a probe of the longest list pays for.

        The index lives until fit / prepare (the item map may change), drop_item_index or the end of this object; savemodel does not
        pickle it: keep item_index() and pass it back as index= after loadmodel.  When Wy / By change on the device afterwards
        (further training steps), the index's device tables are rebuilt from the current weights on the next call while the centroids
        and the partition stay as they were built.  That costs recall, never correctness: every returned score stays exact."""
        import time
        if getattr(self, 'error_during_train', False):
            raise Exception
        if getattr(self, 'itemidmap', None) is None or getattr(self, 'Wy', None) is None:
            raise ValueError('build_item_index needs a fitted or loaded model')
        n_items, W = len(self.itemidmap), self.layers[-1] + 1
        t = dict(seconds_kmeans=0.0, seconds_assign=0.0, seconds_upload=0.0)
        if index is not None:
            cen, offs, items = self._index_checked(index)
            m = self._ensure_model()
        else:
            if centroids is not None:
                cen = np.asarray(centroids)
                if cen.ndim != 2 or cen.shape[1] != W or cen.dtype != np.float32 or not np.isfinite(cen).all():
                    raise ValueError('centroids must be a finite float32 array [n_lists, %d]' % W)
                self._index_n_lists(cen.shape[0], n_items)
                cen = np.ascontiguousarray(cen)
                m = self._ensure_model()
            else:
                n_lists = self._index_n_lists(n_lists, n_items)
                if isinstance(iters, bool) or int(iters) != iters or iters < 0:
                    raise ValueError('iters = %r: it must be an integer >= 0' % (iters,))
                if isinstance(sample_per_list, bool) or int(sample_per_list) != sample_per_list or sample_per_list < 1:
                    raise ValueError('sample_per_list = %r: it must be an integer >= 1' % (sample_per_list,))
                m = self._ensure_model()
                t0 = time.perf_counter()
                cen = self._kmeans(n_lists, iters, sample_per_list, seed)
                t['seconds_kmeans'] = time.perf_counter() - t0
            t0 = time.perf_counter()
            lst = m.ivf_assign(cen)
            items = np.argsort(lst, kind='stable').astype(np.int32)      # stable: every list in ascending item index
            offs = np.concatenate([[0], np.cumsum(np.bincount(lst, minlength=len(cen)))]).astype(np.int64)
            t['seconds_assign'] = time.perf_counter() - t0
        t0 = time.perf_counter()
        m.ivf_set(cen, offs, items)
        t['seconds_upload'] = time.perf_counter() - t0
        self._item_index = dict(centroids=cen, list_offs=offs, list_items=items)
        self._item_index_on = m
        lens = np.diff(offs)
        return dict(n_lists=len(cen), list_len_min=int(lens.min()), list_len_mean=float(lens.mean()), list_len_max=int(lens.max()),
                    empty_lists=int((lens == 0).sum()), **t)

    def item_index(self):
        """The item index as dict(centroids float32[n_lists, D + 1], list_offs int64[n_lists + 1], list_items: item ids in list
        order), or None without one.  Passed back as build_item_index(index=...) it re-creates the index without training it again."""
        ix = getattr(self, '_item_index', None)
        if ix is None:
            return None
        return dict(centroids=ix['centroids'].copy(), list_offs=ix['list_offs'].copy(),
                    list_items=self.itemidmap.index.values[ix['list_items']])

    def drop_item_index(self):
        """Frees the host and device copies of the item index; recommend_sessions(nprobe=) then raises until one is built again."""
        m = getattr(self, '_item_index_on', None)
        if m is not None and m is getattr(self, '_model', None) and getattr(m, 'h', None):
            m.ivf_release()
        self._item_index = None
        self._item_index_on = None

    def _index_model(self):
        """The device model, holding the item index (a model created since the index was built receives it here)."""
        m = self._ensure_model()
        if getattr(self, '_item_index_on', None) is not m:
            ix = self._item_index
            m.ivf_set(ix['centroids'], ix['list_offs'], ix['list_items'])
            self._item_index_on = m
        return m

    def _check_nprobe(self, nprobe, return_probes, k, oversample, scan, predict_for_item_ids, max_per_group):
        """The refusals of recommend_sessions(nprobe=), after the k check and before any device work: (nprobe, oversample) checked."""
        if nprobe is None:
            if return_probes:
                raise ValueError('return_probes=True needs nprobe: without it no list is probed')
            return None
        ix = getattr(self, '_item_index', None)
        if ix is None:
            raise ValueError('nprobe needs an item index: call build_item_index first')
        n_lists = len(ix['list_offs']) - 1
        if isinstance(nprobe, bool) or not isinstance(nprobe, (int, np.integer)) or not 1 <= nprobe <= n_lists:
            raise ValueError('nprobe = %r: it must be an integer in [1, n_lists = %d]' % (nprobe, n_lists))
        if nprobe > _native.G4R_IVF_NPROBE_MAX:
            raise ValueError('nprobe = %d: a row probes at most G4R_IVF_NPROBE_MAX = %d lists' % (nprobe, _native.G4R_IVF_NPROBE_MAX))
        if scan != 'fp32':
            self._scan_oversample(scan, oversample, k)      # (an unknown name is refused as ever)
            raise ValueError("nprobe and scan='bf16' exclude each other: the index is a first stage of its own (its scan is the bf16 one)")
        if predict_for_item_ids is not None:
            raise ValueError('nprobe and predict_for_item_ids exclude each other: the index holds all items')
        if max_per_group is not None:
            raise ValueError('nprobe and max_per_group exclude each other')
        self._scan_oversample('fp32', oversample, k)
        if self.final_act.startswith('softmax'):
            raise NotImplementedError("nprobe is not implemented for final_act=%r, as scan='bf16' is not: a softmax value needs the whole "
                                      "row's maximum and sum" % self.final_act)
        c = min(int(k) * int(oversample), _native.G4R_SCAN_CAND_MAX)
        if int(nprobe) * c > _native.G4R_IVF_WS_MAX:
            raise ValueError('nprobe * min(k * oversample, %d) = %d * %d: it must be at most G4R_IVF_WS_MAX = %d (the first stage keeps that '
                             'many entries per row)' % (_native.G4R_SCAN_CAND_MAX, nprobe, c, _native.G4R_IVF_WS_MAX))
        return int(nprobe), int(oversample)

    def _session_inputs(self, histories, hidden):
        """Checks and packs the histories and the initial hidden state of a stateless call (recommend_sessions,
        score_candidates_sessions): (N, lengths, offsets int64[N + 1], item indices int32, per-layer padded states or None)."""
        hist = [np.ravel(h) if isinstance(h, np.ndarray) else list(h) for h in histories]
        N = len(hist)
        if N < 1:
            raise ValueError('histories is empty: at least one session is needed')
        lens = np.array([len(h) for h in hist], dtype=np.int64)
        if (lens == 0).any():
            raise ValueError('history %d is empty' % np.flatnonzero(lens == 0)[0])
        hidx = self.itemidmap[np.concatenate(hist)].values.astype(np.int32)
        offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        h0 = None
        if hidden is not None:
            if not isinstance(hidden, (list, tuple)) or len(hidden) != len(self.layers):
                raise ValueError('hidden must be a list of %d arrays, one per layer' % len(self.layers))
            h0 = []
            for l, (h, D) in enumerate(zip(hidden, self.layers)):
                if not isinstance(h, np.ndarray) or h.dtype != np.float32 or h.shape != (N, D):
                    raise ValueError('hidden[%d] must be a float32 array of shape (%d, %d), not %s %s' % (
                        l, N, D, getattr(h, 'dtype', type(h).__name__), getattr(h, 'shape', '')))
                h0.append(_pad_cols(h, 1, D, _pad4(D)))
        return N, lens, offs, hidx, h0

    def recommend_sessions(self, histories, k=20, predict_for_item_ids=None, exclude_history=False, exclude=None, exclude_per_row=None,
                           hidden=None, return_hidden=False, scan='fp32', oversample=8, max_per_group=None, pool=None, exclude_groups=None,
                           nprobe=None, return_probes=False):
        """Top-k next items of N whole sessions in one stateless call: (item_ids[N, k], scores[N, k] float32), plus the new hidden
        state with return_hidden=True.  Not in the reference.

          nprobe           None: nothing changes.  An integer in [1, n_lists] (at most 256; it needs build_item_index): approximate
                           top-k over the item index.  Row i probes the nprobe lists whose centroids score best against its final
                           hidden state (equal values to the lower list) and only their items are considered: a bf16 scan (as
                           scan='bf16', exclusions applied) keeps c = min(k * oversample, 1024) of them, those are scored again in fp32
                           and the k best returned.  Every returned score is predict_next_batch's bit for bit, the order and the tie
                           rule (the lower item first) are the exact call's; only WHICH items are considered is approximate.  The call
                           returns (item_ids[N, k], scores[N, k], n_found[N] int32), then the hidden state with return_hidden=True,
                           then with return_probes=True an int32 array [N, nprobe] of list numbers, best first.  n_found[i] < k only
                           when row i's probed lists hold fewer than k eligible items; entries at and after it have score NaN and
                           an unspecified id.  A row's result does not depend on the other rows of the call; with nprobe = n_lists it
                           is scan='bf16''s with the same oversample; when c covers the eligible items of the probed lists it is the
                           exact top-k over them.  Refused (ValueError) together with scan='bf16', predict_for_item_ids or
                           max_per_group, without an index, out of range, or with nprobe * c over G4R_IVF_WS_MAX = 65536; softmax /
                           softmax_logit raise NotImplementedError.  The exclusions, hidden and return_hidden work as without it.

          histories        N >= 1 non-empty sequences of item ids; row i belongs to histories[i].  Any N, independent of batch_size.
          hidden           None: every session starts from zero (a new session).  Otherwise a list with one float32 array
                           [N, layers[l]] per layer (the layout of H[l]): history i is replayed from row i.
          return_hidden    also return that list after the last item of every history (to be passed back as `hidden` later).
          exclude_history  row i never receives an item of histories[i].  Items seen before a supplied `hidden` are unknown to the
                           call: pass them in exclude_per_row.
          predict_for_item_ids, exclude, exclude_per_row, k: as in recommend_next_batch (exclude_per_row: N lists).
          scan, oversample as in recommend_next_batch: scan='bf16' is the two-stage selection (bf16 scan, exact fp32 re-rank); the
                           replay, and so the returned hidden state, is the same either way.
          exclude_groups   group labels (set_item_groups): every item of these groups joins `exclude`.
          max_per_group    None: nothing changes.  An integer c >= 1 (it needs set_item_groups): a row receives at most c items of one
                           group, and the call returns (item_ids[N, k], scores[N, k], n_kept[N] int32), plus the hidden state when
                           asked.  The row's pool is what this call returns with k = pool and max_per_group=None; the walk down the
                           pool keeps an item iff it is ungrouped or fewer than c items of its group were kept before it, and
                           stops after k kept items (the cap rule of include/gru4rec_hip.h, on the device behind the selection).
                           n_kept[i] <= k is the number kept; entries at and after it have score NaN and an unspecified id (that
                           of candidate 0).  Scores are recommend_sessions' bit patterns.  A row is exact over the WHOLE catalogue
                           when n_kept[i] == k -- the walk finished inside the pool, so a longer pool would not change it -- and
                           when pool equals the row's eligible candidate positions; otherwise a longer pool may add items.
          pool             the pool of max_per_group, k <= pool <= min(number of candidates, G4R_TOPK_MAX = 256); None:
                           min(G4R_TOPK_MAX, number of candidates, 4 * k).  The k / exclusion / oversample checks then apply with
                           k = pool: every session needs `pool` eligible candidate positions.

        Row i equals, items and score bits, what recommend_next_batch returns for a session whose first T - 1 items went through
        predict_next_batch from a fresh prediction state and whose last item is the recommend_next_batch input (exclude_history as
        exclude_seen); the returned state is the one that stepping leaves.  So recommend_sessions(a + b) equals
        recommend_sessions(b, hidden=<state after a>).  The history is replayed on the device and the catalogue scored once per
        session.  The prediction state (predict_next_batch / recommend_next_batch, current_session, their seen-history) is neither
        read nor changed.  Everything is checked before any device work: an empty history or a bad `hidden` (layer count, shape,
        dtype) raises ValueError, an unknown item id KeyError, and the k / exclusion checks are those of recommend_next_batch."""
        if self.error_during_train:
            raise Exception
        k = _check_k(k, self._n_candidates(predict_for_item_ids), bools=True)
        probe = self._check_nprobe(nprobe, return_probes, k, oversample, scan, predict_for_item_ids, max_per_group)
        if probe is not None:
            N, lens, offs, hidx, h0 = self._session_inputs(histories, hidden)
            excl = self._session_exclusions(N, lens, hidx, k, None, exclude_history, exclude, exclude_per_row, exclude_groups=exclude_groups)
            out = self._index_model().recommend_sessions_ivf(offs, hidx, k, probe[1], probe[0], *excl, hidden=h0, return_hidden=return_hidden,
                                                             return_probes=return_probes)
            res = (self.itemidmap.index.values[out[0]], out[1], out[2])
            if return_hidden:
                res += (self._unpad_hidden(out[3]),)
            return res + (out[-1],) if return_probes else res
        cap, pool = self._cap_args(max_per_group, pool, k, self._n_candidates(predict_for_item_ids))
        ksel = k if cap is None else pool      # what the selection returns per row
        over = self._scan_oversample(scan, oversample, ksel)
        N, lens, offs, hidx, h0 = self._session_inputs(histories, hidden)
        iidx, cand = self._candidates(predict_for_item_ids)
        excl = self._session_exclusions(N, lens, hidx, ksel, iidx, exclude_history, exclude, exclude_per_row, exclude_groups=exclude_groups)
        m = self._ensure_model()
        if cap is not None:
            out = m.recommend_sessions_capped(offs, hidx, iidx, k, pool, cap, *excl, hidden=h0, return_hidden=return_hidden, oversample=over)
            res = (cand[np.maximum(out[0], 0)], out[1], out[3])
            return res + (self._unpad_hidden(out[4]),) if return_hidden else res
        out = m.recommend_sessions(offs, hidx, iidx, k, *excl, hidden=h0, return_hidden=return_hidden, **_scan_kw(over))
        if not return_hidden:
            return cand[out[0]], out[1]
        return cand[out[0]], out[1], self._unpad_hidden(out[2])

    # ------------------------------------------------------------------ session store (gru4rec_amd/session_store.py)
    def _drop_session_store(self):
        """Every path that drops, replaces or retrains the device model comes through here (prepare -- so fit --, run_epoch, close):
        an open session store is closed, its states belong to the old weights."""
        st = getattr(self, '_store', None)
        if st is not None:
            st._invalidate()
        self._store = None

    def open_session_store(self, capacity, seen_cap=64):
        """Opens the device-resident session store of this model and returns it (a session_store.SessionStore).  Not in the reference.
        It holds `capacity` sessions: every session's hidden state and its sorted list of seen items (at most seen_cap, an integer in
        [0, G4R_EXCLUDE_MAX = 1024]; 0: no lists are kept, and exclude_seen=True is refused) stay on the device between calls, so a
        service pushes a click and receives the next top-k without replaying a history or carrying a state: store.push /
        store.recommend / store.export / store.load / store.end.  One open store per device model: a second open raises
        RuntimeError until the first is closed.  The store is bound to the device model: fit, prepare, run_epoch and close close
        it (its calls then raise RuntimeError), and it is not pickled.  It needs a fitted or loaded model."""
        from .session_store import SessionStore
        if getattr(self, 'error_during_train', False):
            raise Exception
        if getattr(self, 'itemidmap', None) is None:
            raise ValueError('open_session_store needs a fitted or loaded model')
        if isinstance(capacity, bool) or not isinstance(capacity, (int, np.integer)) or not 1 <= capacity < 2 ** 31:
            raise ValueError('capacity = %r: it must be an integer in [1, 2^31 - 1]' % (capacity,))
        if isinstance(seen_cap, bool) or not isinstance(seen_cap, (int, np.integer)) or not 0 <= seen_cap <= _native.G4R_EXCLUDE_MAX:
            raise ValueError('seen_cap = %r: it must be an integer in [0, G4R_EXCLUDE_MAX = %d]' % (seen_cap, _native.G4R_EXCLUDE_MAX))
        st = getattr(self, '_store', None)
        if st is not None and not st.closed:
            raise RuntimeError('a session store is open on this model already (one per device model): close it first')
        m = self._ensure_model()
        m.store_open(int(capacity), int(seen_cap))
        self._store = SessionStore(self, m, capacity, seen_cap)
        self._store._bytes = m.store_info()[2]
        return self._store

    def continue_sessions(self, histories, steps, k=1, no_repeat=True, predict_for_item_ids=None, exclude=None, exclude_per_row=None,
                          hidden=None, return_hidden=False, scan='fp32', oversample=8, max_per_group=None, pool=None, count_history=False,
                          exclude_groups=None):
        """The next `steps` items of N whole sessions in one stateless call: (item_ids[N, steps, k], scores[N, steps, k] float32),
        plus the hidden state with return_hidden=True.  Not in the reference.

        The histories are replayed as in recommend_sessions (from zero, or from `hidden`); step 0 selects every row's k best next
        items; the best one, [:, s, 0], is fed back as the row's next input and step s + 1 selects again: `steps` selections,
        steps - 1 fed-back items.  [:, :, 0] is the continuation, the other k - 1 columns are the alternatives at that step.  The
        feedback runs on the device: between steps nothing returns to the host.

        The result equals, item ids, score bits and hidden-state bits, a loop of recommend_sessions calls: the histories with
        exclude_history=no_repeat first, then steps - 1 times the one-item histories [[previous winner]] from the returned hidden
        state, with exclude_per_row = (history + generated items so far, when no_repeat) + the caller's exclude_per_row.

          no_repeat        row i never receives an item of histories[i] nor an item it has generated itself.  False: only exclude /
                           exclude_per_row apply, and a row may loop.
          return_hidden    also return the state that produced the LAST step's scores: after the history and the steps - 1 fed-back
                           items (the last winner has not been consumed).  So continue_sessions(h, a + b)[:, a:] equals
                           continue_sessions([[path[i, a - 1]]], b, hidden=H_a, exclude_per_row=h_i + path[i, :a]).
          k, predict_for_item_ids, exclude, exclude_per_row, hidden, scan, oversample: as in recommend_sessions, with its refusals.
                           softmax / softmax_logit scores are not renormalised over the remaining items.
          exclude_groups   as in recommend_sessions.
          max_per_group    None: nothing changes.  An integer c >= 1 (it needs set_item_groups): at most c items of one group along a
                           row's path, and the call returns (item_ids[N, steps, k], scores[N, steps, k], n_kept[N, steps] int32),
                           plus the hidden state when asked.  Every step selects `pool` items (pool as in recommend_sessions, the
                           checks with k = pool) and recommend_sessions' walk keeps up to k of them, counting on top of the row's
                           prior: the groups of the winners of the steps before, plus the groups of histories[i] with
                           count_history=True.  [:, s, 0], the first kept item, is the winner that is fed back.  n_kept[i, s] == 0
                           marks a fallback step: the pool held no item the cap allows, column 0 is then the unconstrained best (it
                           is fed back, and its group counts like any winner's) and the other columns are pads.  The walk, the
                           prior and the feedback stay on the device.  The result equals the loop of recommend_sessions(k=pool)
                           calls described above with the walk on the host between them.  A row's prior plus steps - 1 may not
                           exceed G4R_GROUP_PRIOR_MAX = 1024 groups.

        Everything is checked before any device work and the prediction state is neither read nor changed.  steps must be an integer
        >= 1.  With no_repeat, predict_for_item_ids must be duplicate-free (every fed-back item then removes exactly one eligible
        position), every row's distinct excluded items plus steps - 1 must not exceed G4R_EXCLUDE_MAX, and every row must keep at least
        k eligible candidate positions at the last step (eligible - (steps - 1) >= k: no list ever holds a pad); each failure raises
        ValueError naming the row."""
        if self.error_during_train:
            raise Exception
        steps = _check_steps(steps)
        k = _check_k(k, self._n_candidates(predict_for_item_ids), bools=True)
        cap, pool = self._cap_args(max_per_group, pool, k, self._n_candidates(predict_for_item_ids), count_history)
        ksel = k if cap is None else pool
        over = self._scan_oversample(scan, oversample, ksel)
        N, lens, offs, hidx, h0 = self._session_inputs(histories, hidden)
        iidx, cand = self._candidates(predict_for_item_ids)
        excl = self._session_exclusions(N, lens, hidx, ksel, iidx, no_repeat, exclude, exclude_per_row, steps=steps, exclude_groups=exclude_groups)
        if cap is not None:
            prior = self._prior_groups(N, (np.repeat(np.arange(N), lens), hidx) if count_history else None, steps - 1)
            m = self._ensure_model()
            out = m.continue_sessions_capped(offs, hidx, iidx, k, pool, cap, steps, bool(no_repeat), *excl, *prior, hidden=h0,
                                             return_hidden=return_hidden, oversample=over)
            res = (cand[np.maximum(out[0], 0)], out[1], out[2])
            return res + (self._unpad_hidden(out[3]),) if return_hidden else res
        m = self._ensure_model()
        out = m.continue_sessions(offs, hidx, iidx, k, steps, bool(no_repeat), *excl, hidden=h0, return_hidden=return_hidden, oversample=over)
        if not return_hidden:
            return cand[out[0]], out[1]
        return cand[out[0]], out[1], self._unpad_hidden(out[2])

    def beam_sessions(self, histories, steps, beams=4, no_repeat=True, predict_for_item_ids=None, exclude=None, exclude_per_row=None,
                      hidden=None, combine=None, scan='fp32', oversample=8):
        """Beam search over the next `steps` items of N whole sessions in one stateless call: (paths[N, beams, steps] item ids, best
        path first, path_scores[N, beams] float32, step_scores[N, beams, steps] float32 -- the step score of every item on the path
        -- and scale_exp[N] int32).  Not in the reference.  continue_sessions feeds back only the best item of every step; this call
        keeps `beams` partial paths per session alive and scores each path as a whole.

        The result equals, item ids, score bits and scale_exp, a host loop of recommend_sessions calls.  Step 0 is
        recommend_sessions(histories, k=beams, exclude_history=no_repeat, ...): beam i is column i, its path score that score.  At
        every later step each beam b is one recommend_sessions([[its last item]], k=beams, hidden=<its own state>) row, excluded
        items as below; candidate (b, j) with step score x has the path score
          combine='sum'      fl32(cum_b + x)   (the default, except for softmax scores);
          combine='product'  fl32(cum_b * x), a result of magnitude below 2^-126 replaced by 0.0; allowed only, and the default,
                             for final_act softmax / softmax_logit, whose scores are probabilities;
        and the `beams` best of the session's beams x beams candidates -- path score descending, equal scores by the lower
        b * beams + j, NaN last -- become the new beams, each with its parent's path plus the item and the state its parent's call
        returned.  'product' rescales after every selection: with m the new beam 0's path score (finite, > 0) = g * 2^e, 1 <= g < 2,
        the session's path scores are multiplied by 2^-e and e is added to scale_exp, so path probability = path_scores *
        2.0 ** scale_exp however many steps there are ('sum': scale_exp is 0).  softmax scores are not renormalised over the
        remaining items.

          no_repeat        a path never holds an item of its session's history nor an item twice: a beam's exclusions are the
                           caller's plus the history and its own path.  False: only exclude / exclude_per_row apply.
          beams            an integer in [1, min(number of candidates, G4R_BEAM_MAX = 32)].
          predict_for_item_ids, exclude, exclude_per_row, hidden, scan, oversample: as in continue_sessions with k = beams, with its
                           refusals (duplicate-free candidates under no_repeat, excluded items + steps - 1 <= G4R_EXCLUDE_MAX, at
                           least beams eligible positions left at the last step, a bad `hidden`, an empty history: ValueError
                           naming the row where there is one; an unknown id: KeyError).

        beams=1 is continue_sessions(k=1)'s path; steps=1 is recommend_sessions(k=beams).  Everything is checked before any device
        work and the prediction state is neither read nor changed.  The paths are rebuilt on the host from the back-pointers the
        device returns (_native.beam_backtrack)."""
        if self.error_during_train:
            raise Exception
        steps = _check_steps(steps)
        beams = _check_k(beams, self._n_candidates(predict_for_item_ids), name='beams', cap=_native.G4R_BEAM_MAX, own_errors=True)
        softmax = self._final[0] in (_native.ACT_IDS['softmax'], _native.ACT_IDS['softmax_logit'])      # (is_softmax of the C side)
        if combine is None:
            combine = 'product' if softmax else 'sum'
        if combine not in ('sum', 'product'):
            raise ValueError("combine = %r: it must be None, 'sum' or 'product'" % (combine,))
        if combine == 'product' and not softmax:
            raise ValueError("combine='product' multiplies probabilities: it needs final_act softmax / softmax_logit, not %r" % self.final_act)
        over = self._scan_oversample(scan, oversample, beams)
        N, lens, offs, hidx, h0 = self._session_inputs(histories, hidden)
        iidx, cand = self._candidates(predict_for_item_ids)
        excl = self._session_exclusions(N, lens, hidx, beams, iidx, no_repeat, exclude, exclude_per_row, steps=steps)
        m = self._ensure_model()
        parent, cols, sscores, path_scores, scale_exp = m.beam_sessions(offs, hidx, iidx, beams, steps, bool(no_repeat), combine, *excl,
                                                                        hidden=h0, oversample=over)
        paths, step_scores = _native.beam_backtrack(parent, cols, sscores)
        return cand[paths], path_scores, step_scores, scale_exp

    def session_log_partition(self, histories, temperature=1.0, predict_for_item_ids=None, exclude_history=False, exclude=None,
                              exclude_per_row=None, hidden=None):
        """lse float32[N]: the logarithm of the sum of exp(z / temperature) over every session's eligible candidates, formed on the
        device in one stateless call.  Not in the reference.  For a model whose score is the logit (every final_act but softmax /
        softmax_logit), fl32(z / temperature) - lse is the log-probability, under softmax(z / temperature) over the eligible
        candidates, of any score z that recommend_sessions or score_candidates_sessions returns for the same arguments; for softmax
        models z is the pre-activation value, as in sample_sessions.  Arguments, eligibility and refusals are recommend_sessions' with
        k = 1, temperature is sample_sessions'; at most 2^24 candidate positions.  The value is sample_sessions' normaliser:
        lse = fl32(zeta / temperature + log(Q * 2^-39)) in float64, zeta and the exact integer Q as its docstring defines them, so the
        same session gives the same bits alone or among others."""
        if self.error_during_train:
            raise Exception
        t32 = _check_temperature(temperature)
        _check_k(1, self._n_candidates(predict_for_item_ids), bools=True)
        _check_lse_candidates(self._n_candidates(predict_for_item_ids))
        N, lens, offs, hidx, h0 = self._session_inputs(histories, hidden)
        iidx, cand = self._candidates(predict_for_item_ids)
        excl = self._session_exclusions(N, lens, hidx, 1, iidx, exclude_history, exclude, exclude_per_row)
        m = self._ensure_model()
        zeta, Q = m.session_log_partition(offs, hidx, iidx, float(t32), *excl, hidden=h0)
        inv_t = np.float64(np.float32(1) / t32)
        with np.errstate(all='ignore'):
            return (zeta.astype(np.float64) * inv_t + np.log(Q.astype(np.float64) * 2.0 ** -39)).astype(np.float32)

    def session_log_likelihood(self, histories, temperature=1.0, predict_for_item_ids=None, exclude_seen=False, exclude=None,
                               return_details=False):
        """Teacher forcing over N sessions given as lists of item ids, in one device call: (logprobs float32[sum(len_i - 1)], offsets
        int64[N + 1]).  Not in the reference.  Event t of row i has input histories[i][t] and target histories[i][t + 1];
        logprobs[offsets[i] + t] is the log-probability sample_sessions' distribution -- softmax(z / temperature) over the eligible
        candidate positions after the prefix histories[i][:t + 1] -- gives that target, -inf when the target holds no eligible
        position (excluded, already shown with exclude_seen, or not among predict_for_item_ids).  The contract, the arguments'
        meaning and the refusals are evaluation.loglik_gpu's (exclude_seen: its exclude_seen, which is sample_sessions' no_repeat);
        the histories are checked as recommend_sessions checks them.  A one-item history contributes no event; no scored event at all
        is a ValueError.  return_details: a third value, loglik_gpu's dict for the same events (session = the row i)."""
        from . import evaluation
        if self.error_during_train:
            raise Exception
        t32 = _check_temperature(temperature)
        n_cand = self._n_candidates(predict_for_item_ids)
        _check_k(1, n_cand, bools=True)
        _check_lse_candidates(n_cand)
        N, lens, offs, hidx, _ = self._session_inputs(histories, None)
        iidx, _ = self._candidates(predict_for_item_ids)
        out_offs = np.concatenate([[0], np.cumsum(lens - 1)]).astype(np.int64)
        if out_offs[-1] == 0:
            raise ValueError('no scored event: every history holds a single item')
        keep = np.flatnonzero(lens > 1)                       # (a one-item session has no event to score and takes no row of the plan)
        on = np.repeat(lens > 1, lens)
        koffs = np.concatenate([[0], np.cumsum(lens[keep])]).astype(np.int64)
        res = evaluation._loglik_events(self, hidx[on], None if iidx is None else iidx.astype(np.int32), koffs, np.repeat(keep, lens[keep]),
                                        int(min(512, len(keep))), t32, exclude_seen, exclude)
        if return_details:
            return res['logprob'], out_offs, res
        return res['logprob'], out_offs

    def audience_sessions(self, histories, item_ids, k, by='logprob', temperature=1.0, exclude_history=False, hidden=None):
        """Which sessions for this item?  For each of M items the k sessions with the largest value, selected on the device in one
        stateless call: (sessions int64[M, k], values float32[M, k], counts int32[M]).  Not in the reference.

          histories, hidden  as in recommend_sessions: N >= 1 non-empty sequences of item ids, any N, and the optional initial state.
          item_ids           M >= 1 item ids, at most G4R_AUDIENCE_ITEMS_MAX = 4096; duplicates are allowed, every position gets its
                             own list.
          k                  the audience size per item, 1 <= k <= G4R_AUDIENCE_MAX = 65536 with M * k <= 2^23.  It is not bounded by
                             G4R_TOPK_MAX and may exceed N.
          by='score'         the value is the item's full-catalogue predict_next_batch score after the session's history: the bits
                             score_candidates_sessions returns for an element-wise final activation.  Scores of different sessions are
                             on one scale only where the model's loss puts them there, and softmax / softmax_logit models raise
                             NotImplementedError: use by='logprob'.
          by='logprob'       the value is the log-probability that softmax(z / temperature) over the session's eligible items -- the
                             whole catalogue, at most 2^24 items -- gives the item; z is the predict_next_batch score, for softmax
                             models the pre-activation value, as in loglik_gpu.  It is session_log_likelihood's value for the history
                             followed by the item: fl32((double)d - log((double)Q * 2^-39)), d = fl32(fl32(z - zeta) / temperature),
                             zeta and the exact integer Q of session_log_partition.
          temperature        as in sample_sessions; read with by='logprob' only.
          exclude_history    a session whose history holds the item is not eligible for that item and is never listed; with
                             by='logprob' the history's items also leave the session's normaliser (session_log_partition's
                             exclude_history, loglik_gpu's exclude_seen; a history of at most G4R_EXCLUDE_MAX = 1024 distinct items).

        Row j holds the counts[j] <= k eligible sessions with the largest value for item_ids[j], as indices into `histories`, ordered
        by value descending, then by the lower index, NaN last; entries at and after counts[j] have session -1 and value NaN.  The
        result depends on nothing else: not on how the call is chunked (G4R_SESSIONS_CHUNK) nor on the company a session keeps.  The
        histories are replayed 512 a chunk and the running lists stay on the device, so M * k entries reach the host whatever N is.
        The prediction state is neither read nor changed.  Everything is checked before any device work: the histories and `hidden`
        as in recommend_sessions, an unknown item id raises KeyError.
        Deliberately left out: predict_for_item_ids, exclude, exclude_per_row, scan='bf16', return_hidden; group-level affinity (a
        segment per item group); per-session caps across items."""
        if self.error_during_train:
            raise Exception
        if by not in _native.AUDIENCE_BY:
            raise ValueError("by = %r: it must be 'score' or 'logprob'" % (by,))
        softmax = self._final[0] in (_native.ACT_IDS['softmax'], _native.ACT_IDS['softmax_logit'])
        if by == 'score' and softmax:
            raise NotImplementedError("by='score' is not implemented for final_act=%r (a softmax score is normalised over its own row and "
                                      "the pre-activation values of different sessions are not on one scale): use by='logprob'" % self.final_act)
        t32 = _check_temperature(temperature) if by == 'logprob' else np.float32(1)
        ids = np.ravel(item_ids) if isinstance(item_ids, np.ndarray) else list(item_ids)
        M = len(ids)
        if not 1 <= M <= _native.G4R_AUDIENCE_ITEMS_MAX:
            raise ValueError('item_ids holds %d items: between 1 and G4R_AUDIENCE_ITEMS_MAX = %d are needed' % (M, _native.G4R_AUDIENCE_ITEMS_MAX))
        try:
            ok = not isinstance(k, bool) and int(k) == k and 1 <= k <= _native.G4R_AUDIENCE_MAX
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError('k = %r: it must be an integer in [1, G4R_AUDIENCE_MAX = %d]' % (k, _native.G4R_AUDIENCE_MAX))
        k = int(k)
        if M * k >_native.G4R_AUDIENCE_ENTRIES_MAX:
            raise ValueError('%d items x k = %d is more than G4R_AUDIENCE_ENTRIES_MAX = 2^23 list entries' % (M, k))
        if by == 'logprob':
            _check_lse_candidates(self.n_items)
        N, lens, offs, hidx, h0 = self._session_inputs(histories, hidden)
        iidx = self.itemidmap[ids].values.astype(np.int32)
        m = self._ensure_model()
        sessions, values, counts = m.audience_sessions(offs, hidx, iidx, k, by=by, temperature=float(t32), exclude_history=bool(exclude_history),
                                                       hidden=h0)
        return np.asarray(sessions).astype(np.int64), np.asarray(values, dtype=np.float32), np.asarray(counts, dtype=np.int32)

    def sample_sessions(self, histories, steps, samples=1, temperature=1.0, top_k=None, seed=0, first_step=0, no_repeat=True,
                        predict_for_item_ids=None, exclude=None, exclude_per_row=None, hidden=None, return_hidden=False, top_p=None,
                        return_logprobs=False):
        """Stochastic continuations of N whole sessions in one stateless call: `samples` independent draws per session of `steps`
        items each, drawn from the model's own next-item distribution.  Returns (item_ids[N, samples, steps], scores[N, samples,
        steps] float32), plus the hidden state with return_hidden=True.  Not in the reference.  continue_sessions and beam_sessions are
        deterministic; this call gives varied continuations of one history, several independent roll-outs per session, or simulated
        sessions for offline policy evaluation, without a score row ever leaving the device.

        Draw (i, j) -- session i, sample j -- starts from the state after histories[i] (replayed from zero, or from hidden[i]).  At
        step s it draws ONE item from softmax(z / temperature) over its eligible candidates, where z is a candidate's logit; the item
        is fed back on the device as the draw's next input and, with no_repeat, joins the draw's own exclusions: continue_sessions'
        feedback on N * samples rows.  The draw is an argmax (the Gumbel-max trick):
          z       the predict_next_batch score, bit for bit; for final_act softmax / softmax_logit the PRE-activation value
                  h . Wy_i + By_i, of which those scores are the softmax;
          g       -log(-log(u)), u uniform in (0, 1) from the counter-based generator: Philox4x32-10 keyed by `seed`, counter (item
                  index >> 2, row id i * samples + j, first_step + s, a stream id of its own), lane item index & 3;
          chosen  the eligible candidate with the largest fl32(fl32(z / temperature) + g), equal values to the lower position.
        So a draw depends on (seed, i, j, first_step + s, the items' logits) and on nothing else: not on N, the batch, the order of
        the rows or how the call is chunked.  `scores` holds the chosen items' z, not the perturbed values: for softmax models that
        is the LOGIT, not the probability predict_next_batch returns.

          samples          an integer in [1, G4R_SAMPLE_MAX = 64]: draws per session.
          temperature      a finite float > 0.  Below 1 sharpens, above 1 flattens.  The greedy limit (temperature -> 0) is
                           continue_sessions(k=1).
          top_k            None, or an integer in [1, min(number of candidates, G4R_TOPK_MAX = 256)]: the eligible candidates are
                           first cut to the top_k best by z (recommend_sessions' exact order, the same exclusions) and the draw is
                           made among those.  top_k=1 is continue_sessions(k=1)'s path for every seed.
          seed             an integer in [0, 2^64): the key of the noise.
          first_step       the step number of the call's first draw, >= 0 with first_step + steps <= 2^31 - 1.  It lets a roll-out be
                           carried on: sample_sessions(h, a + b)[..., a:] equals sample_sessions(<the N * samples one-item histories
                           of the a-th drawn items>, b, samples=1, first_step=a, hidden=<the returned state reshaped to [N * samples,
                           layers[l]]>, exclude_per_row=<history + the first a drawn items, when no_repeat>).
          no_repeat        draw (i, j) never receives an item of histories[i] nor one it has drawn itself.  False: only exclude /
                           exclude_per_row apply.
          return_hidden    also return a list of float32 [N, samples, layers[l]] arrays: the state that produced the LAST step's
                           scores, the same moment as in continue_sessions.
          predict_for_item_ids, exclude, exclude_per_row, hidden: as in continue_sessions with k = top_k (1 without it), with its
                           refusals, each naming its row: duplicate-free candidates under no_repeat, excluded items + steps - 1 <=
                           G4R_EXCLUDE_MAX, at least k eligible positions at the last step.

        Everything is checked before any device work and the prediction state is neither read nor changed.  N * samples must not
        exceed 2^31 - 1.  The two-stage scan='bf16' selection is not offered here.

          return_logprobs  True: logprobs[N, samples, steps] float32, the log-probability with which every item was drawn, is appended
                           as the LAST element of the returned tuple (after the hidden state, if that is returned too).  Items, scores
                           and hidden state are, bit for bit, those of the call without it.
          top_p            None, or a float with 0 < fl32(top_p) <= 1; it needs top_k.  Nucleus sampling: the draw is made among the
                           shortest prefix of the top_k best whose mass reaches top_p of the WHOLE eligible set's.

        Both rest on a row normaliser formed on the device in the scan of the catalogue, exactly, in 64-bit fixed point, so that they
        keep the promise above (no dependence on N, the batch, the row order or the chunking).  For one draw at one step, over its
        eligible candidate positions E (with predict_for_item_ids every position counts, a duplicate once each):
          zeta     the largest z over E in the selection's order;
          d_n      fl32(fl32(z_n - zeta) * fl32(1 / temperature)): two roundings, no FMA;
          q_n      round_to_uint64(2^39 * expf(d_n)), 0 for a NaN d_n: the argmax has 2^39 exactly, terms more than about 27 nats
                   below it are 0;
          Q        the sum of q_n over E, an exact integer (more than 2^24 candidate positions are refused with these options);
          logprob  fl32(float64(d_c) - log(float64(Den) * 2^-39)) of the chosen c, Den the integer mass of the set drawn from: Q when
                   untruncated; C_t, the sum of q over the top_k best (zeta is then their first z), with top_k alone; C_m with top_p;
          nucleus  the top_k best in the selection's order, C_j the integer prefix sums of their q: m is the smallest j with
                   float64(C_j) >= float64(fl32(top_p)) * float64(Q), or top_k if there is none, and the draw is the usual argmax
                   over the first m entries.  So top_p=1.0 gives top_p=None bit for bit, and a top_p below the first entry's share
                   gives top_k=1's path with every logprob == 0.0.
        The untruncated logprob costs a second scan of the catalogue per step (zeta first, then the sum), top_p one more scan;
        top_k with return_logprobs alone costs none.  Scores that are not finite (zeta NaN or infinite) give undefined
        log-probabilities.  session_log_partition returns the normaliser itself."""
        if self.error_during_train:
            raise Exception
        steps = _check_steps(steps)
        try:
            ok = not isinstance(samples, bool) and int(samples) == samples and 1 <= samples <= _native.G4R_SAMPLE_MAX
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError('samples = %r: it must be an integer in [1, G4R_SAMPLE_MAX = %d]' % (samples, _native.G4R_SAMPLE_MAX))
        samples = int(samples)
        t32 = _check_temperature(temperature)
        if top_k is not None:
            top_k = _check_k(top_k, self._n_candidates(predict_for_item_ids), name='top_k', own_errors=True)
        if top_p is not None:
            try:
                with np.errstate(all='ignore'):
                    p32 = np.float32(top_p) if not isinstance(top_p, (bool, np.bool_, str)) and np.ndim(top_p) == 0 else np.float32('nan')
                    ok = bool(0 < p32 <= 1)
            except (TypeError, ValueError):
                ok = False
            if not ok:
                raise ValueError('top_p = %r: it must be None or a float in (0, 1] (as a float32)' % (top_p,))
            if top_k is None:
                raise ValueError('top_p = %r needs top_k: the nucleus is sought among the top_k best' % (top_p,))
            top_p = float(p32)
        if not isinstance(return_logprobs, (bool, np.bool_)):
            raise ValueError('return_logprobs = %r: it must be True or False' % (return_logprobs,))
        return_logprobs = bool(return_logprobs)
        if top_p is not None or return_logprobs:
            _check_lse_candidates(self._n_candidates(predict_for_item_ids))
        try:
            ok = not isinstance(seed, bool) and int(seed) == seed and 0 <= seed < 2 ** 64
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError('seed = %r: it must be an integer in [0, 2^64)' % (seed,))
        try:
            ok = not isinstance(first_step, bool) and int(first_step) == first_step and first_step >= 0 and first_step + steps <= 2 ** 31 - 1
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError('first_step = %r: it must be an integer >= 0 with first_step + steps <= 2^31 - 1' % (first_step,))
        k = top_k or 1
        N, lens, offs, hidx, h0 = self._session_inputs(histories, hidden)
        if N * samples > 2 ** 31 - 1:
            raise ValueError('N * samples = %d * %d exceeds 2^31 - 1' % (N, samples))
        iidx, cand = self._candidates(predict_for_item_ids)
        excl = self._session_exclusions(N, lens, hidx, k, iidx, no_repeat, exclude, exclude_per_row, steps=steps)
        m = self._ensure_model()
        opts = dict(top_p=top_p, return_logprobs=return_logprobs) if top_p is not None or return_logprobs else {}      # (none: the old entry)
        out = m.sample_sessions(offs, hidx, iidx, steps, samples, top_k, float(t32), int(seed), int(first_step), bool(no_repeat), *excl,
                                hidden=h0, return_hidden=return_hidden, **opts)
        res = (cand[out[0]], out[1])
        if return_hidden:
            res += ([h.reshape(N, samples, -1) for h in self._unpad_hidden(out[2])],)
        if return_logprobs:
            res += (out[-1],)
        return res

    # ------------------------------------------------------------------ per-row candidate lists (not in the reference)
    def _candidate_csr(self, candidates, rows, k):
        """Checks and packs the `candidates` argument of score_candidates*: (offsets int64[rows + 1], item indices int32, the
        candidate ids in CSR order, C for a 2-D array / None for ragged lists, k or 0).  Raises before anything changes."""
        if isinstance(candidates, np.ndarray) and candidates.ndim == 2:
            if candidates.shape[0] != rows:
                raise ValueError('candidates has %d rows, one per row (%d) is needed' % (candidates.shape[0], rows))
            width = candidates.shape[1]
            if width < 1:
                raise ValueError('candidate list 0 is empty')
            flat = candidates.ravel()
            lens = np.full(rows, width, dtype=np.int64)
        else:
            if isinstance(candidates, (str, bytes)) or not hasattr(candidates, '__len__'):
                raise ValueError('candidates must be a 2-D array or a list of sequences of item ids')
            lists = [np.ravel(x) if isinstance(x, np.ndarray) else list(x) for x in candidates]
            if len(lists) != rows:
                raise ValueError('candidates holds %d lists, one per row (%d) is needed' % (len(lists), rows))
            lens = np.array([len(x) for x in lists], dtype=np.int64)
            if (lens == 0).any():
                raise ValueError('candidate list %d is empty' % np.flatnonzero(lens == 0)[0])
            flat = np.concatenate([np.asarray(x) for x in lists])
            width = None
        if lens.sum() > _native.G4R_CAND_MAX:
            raise ValueError('%d candidate positions in one call: at most G4R_CAND_MAX = %d' % (lens.sum(), _native.G4R_CAND_MAX))
        if k is not None:
            k = _check_k(k)
            short = np.flatnonzero(lens < k)
            if len(short):
                raise ValueError('candidate list %d holds %d positions, fewer than k = %d' % (short[0], lens[short[0]], k))
        cidx = self.itemidmap[flat].values.astype(np.int32)
        offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        return offs, cidx, flat, width, k or 0

    @staticmethod
    def _candidate_result(out, offs, flat, width, k):
        if k == 0:
            return out.reshape(-1, width) if width is not None else [out[offs[i]:offs[i + 1]] for i in range(len(offs) - 1)]
        pos, scores = out
        return flat[offs[:-1, None] + pos], scores

    def score_candidates(self, session_ids, input_item_ids, candidates, k=None, batch=100):
        """Scores of every session's OWN candidate list (the re-ranking stage behind a retrieval stage).  Not in the reference.

          candidates  one list per row: a 2-D array [n, C] of item ids, or n non-empty sequences of item ids (lengths may differ).
                      Duplicates are allowed; every position is scored.
          k=None      the scores in the caller's order: float32 [n, C] for a 2-D array, else a list of n float32 arrays (views into
                      one CSR buffer).
          k           (item_ids[n, k], scores[n, k]): the k best of each row's own list in the recommend_next_batch order (score
                      descending, equal scores by the lower position in the list, NaN last); 1 <= k <= G4R_TOPK_MAX and every list
                      holds at least k positions.

        Row i is bit for bit what the existing calls return with predict_for_item_ids = candidates[i]: column i of
        predict_next_batch for k=None, row i of recommend_next_batch for k.  So softmax / softmax_logit normalise over the row's own
        list; with an element-wise final activation a score equals the full-catalogue predict_next_batch score of that item.  The
        prediction state advances as in predict_next_batch (changed sessions zeroed, the seen-history recorded), so calls may be
        interleaved with predict_next_batch / recommend_next_batch.  Not supported, as the caller controls each list: exclusions
        (exclude_seen, exclude, exclude_per_row) and predict_for_item_ids.  Everything is checked before the state changes: an
        unknown item id raises KeyError; an empty list, a wrong number of lists, a bad k or more than G4R_CAND_MAX positions in all
        raise ValueError."""
        if self.error_during_train:
            raise Exception
        plan = self._predict_plan(session_ids, input_item_ids, batch)
        n = len(np.ravel(plan[3]))
        if not 1 <= n <= batch:
            raise ValueError('%d input items: between 1 and batch = %d are needed' % (n, batch))
        offs, cidx, flat, width, kk = self._candidate_csr(candidates, n, k)
        m, in_idxs = self._predict_rows(session_ids, input_item_ids, batch, plan=plan)
        out = m.score_candidates(in_idxs, offs, cidx, kk)
        return self._candidate_result(out, offs, flat, width, kk)

    def score_candidates_sessions(self, histories, candidates, k=None, hidden=None, return_hidden=False):
        """score_candidates for N whole sessions in one stateless call.  Not in the reference.

          histories, hidden, return_hidden   as in recommend_sessions (any N, replayed on the device in chunks; the prediction state
                                             is neither read nor changed).
          candidates, k                      as in score_candidates, one list per history.
        Returns what score_candidates returns; with return_hidden=True the list of hidden states is appended (k=None: (scores,
        hidden); k: (item_ids, scores, hidden)).  Row i equals, bit for bit, the stepwise route of recommend_sessions: the first
        T - 1 items through predict_next_batch from a fresh state, the last through score_candidates.  Not supported: exclusions and
        predict_for_item_ids.  Everything is checked before any device work (KeyError for an unknown item id, ValueError for an
        empty history or list, a wrong number of lists, a bad k, a bad hidden or more than G4R_CAND_MAX positions)."""
        if self.error_during_train:
            raise Exception
        N, _, hoffs, hidx, h0 = self._session_inputs(histories, hidden)
        offs, cidx, flat, width, kk = self._candidate_csr(candidates, N, k)
        m = self._ensure_model()
        out = m.score_candidates_sessions(hoffs, hidx, offs, cidx, kk, hidden=h0, return_hidden=return_hidden)
        if not return_hidden:
            return self._candidate_result(out, offs, flat, width, kk)
        res = self._candidate_result(out[0], offs, flat, width, kk)
        H = self._unpad_hidden(out[1])
        return (res, H) if kk == 0 else (res[0], res[1], H)

    # ------------------------------------------------------------------ item-to-item neighbours (not in the reference)
    def similar_items(self, item_ids, k=20, metric='cosine', space='output', predict_for_item_ids=None, exclude_self=True, exclude=None):
        """The k items most similar to each of item_ids in the model's own embedding space:
        (item_ids[len(item_ids), k], scores[len(item_ids), k] float32).  Not in the reference.

          item_ids   the query items, any number >= 1, duplicates allowed (they give duplicate rows).
          space      'output': the rows of Wy (layers[-1] wide), the space the sessions' hidden states are scored in.  'input': the
                     input embedding -- E when embedding > 0, Wy again with constrained_embedding; a one-hot input model has none
                     (NotImplementedError: use space='output').
          metric     'dot': sum_d T[q, d] * T[j, d] in fp32.  'cosine': (dot * inv[q]) * inv[j], inv = 1 / sqrt(sum of squares) in
                     fp32; a zero row has inv = 0 and scores 0 against everything, itself included.
          predict_for_item_ids  the candidates in the given order (duplicates allowed); None: all items in itemidmap order.
          exclude_self          skip every candidate position that holds the query item itself.
          exclude               item ids never returned for any query.

        Row r holds the k best candidates of item_ids[r]: score descending, equal scores by the lower candidate position, NaN last
        (the order of recommend_next_batch).  The score of a (query, candidate) pair depends on the two rows alone, so it is
        bit-identical in every call the pair appears in, whatever the other queries, the candidate list or the size of the call.
        Scoring and selection run on the device: only k entries per row return.  The call is stateless: the prediction state
        (predict_next_batch / recommend_next_batch) is neither read nor changed.  The items' inverse norms are kept on the device and
        rebuilt after fit / a parameter upload.  Everything is checked before any device work: an unknown item id raises KeyError; a
        bad k, metric or space, or a query with fewer than k eligible candidate positions (duplicates count), raises ValueError."""
        if self.error_during_train:
            raise Exception
        n_sel = self._n_candidates(predict_for_item_ids)
        k = _check_k(k, n_sel)
        if metric not in _native.SIM_METRICS:
            raise ValueError("metric = %r: it must be 'cosine' or 'dot'" % (metric,))
        if space not in _native.SIM_SPACES:
            raise ValueError("space = %r: it must be 'output' or 'input'" % (space,))
        if space == 'input' and not self.constrained_embedding and not self.embedding:
            raise NotImplementedError("space='input': a one-hot input model has no input embedding (layer 0 reads a row of Wx per item, "
                                      "three gates wide); use space='output'")
        ids = np.ravel(item_ids) if isinstance(item_ids, np.ndarray) else list(item_ids)
        if len(ids) < 1:
            raise ValueError('item_ids is empty: at least one query item is needed')
        qidx = self.itemidmap[ids].values.astype(np.int32)
        iidx, cand = self._candidates(predict_for_item_ids)
        if iidx is not None:
            iidx = iidx.astype(np.int32)
        gidx, mask = self._global_exclude(exclude)
        # eligible candidate positions per query: all - positions of excluded items - (exclude_self) positions of its own item
        if iidx is None:
            n_masked, own = len(gidx), np.ones(len(qidx), dtype=np.int64)
        else:
            n_masked = int(np.isin(iidx, gidx).sum())
            own = np.bincount(iidx, minlength=len(self.itemidmap))[qidx]
        elig = n_sel - n_masked - (np.where(np.isin(qidx, gidx), 0, own) if exclude_self else 0) * np.ones(len(qidx), dtype=np.int64)
        short = np.flatnonzero(elig < k)
        if len(short):
            raise ValueError('query %d (item id %r) has %d eligible candidate positions, fewer than k = %d'
                             % (short[0], getattr(ids[short[0]], 'item', lambda: ids[short[0]])(), elig[short[0]], k))
        m = self._ensure_model()
        cols, scores = m.similar_items(qidx, iidx, k, metric, space, bool(exclude_self), mask)
        return cand[cols], scores

    def item_neighbors(self, k=20, metric='cosine', space='output', exclude=None):
        """The k nearest neighbours of EVERY item: (neighbor_ids[n_items, k], scores[n_items, k] float32), rows in itemidmap order.
        Not in the reference.  It is similar_items(itemidmap.index, k, metric, space, exclude_self=True, exclude=exclude), bit for
        bit: the whole n_items x n_items product is scored and selected on the device in chunks of rows, and only the lists return."""
        return self.similar_items(self.itemidmap.index.values, k=k, metric=metric, space=space, exclude=exclude)

    # ------------------------------------------------------------------ diversified top-k (not in the reference)
    def _mmr_args(self, trade_off, metric, space):
        """The checks diversify_sessions and diversify_lists share; the trade-off as the float32 the device uses."""
        try:
            ok = not isinstance(trade_off, bool) and 0.0 <= float(trade_off) <= 1.0
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError('trade_off = %r: it must be a number in [0, 1]' % (trade_off,))
        if metric not in _native.SIM_METRICS:
            raise ValueError("metric = %r: it must be 'cosine' or 'dot'" % (metric,))
        if space not in _native.SIM_SPACES:
            raise ValueError("space = %r: it must be 'output' or 'input'" % (space,))
        if space == 'input' and not self.constrained_embedding and not self.embedding:
            raise NotImplementedError("space='input': a one-hot input model has no input embedding (layer 0 reads a row of Wx per item, "
                                      "three gates wide); use space='output'")
        return float(np.float32(trade_off))

    def diversify_sessions(self, histories, k=20, pool=100, trade_off=0.7, metric='cosine', space='output', normalize=True,
                           predict_for_item_ids=None, exclude_history=False, exclude=None, exclude_per_row=None, hidden=None,
                           return_hidden=False, scan='fp32', oversample=8, return_details=False, exclude_groups=None):
        """Diversified top-k next items of N whole sessions in one stateless call: (item_ids[N, k], scores[N, k] float32).  Not in
        the reference.  Maximal marginal relevance: the pool of a session is what recommend_sessions(k=pool) returns for it with the
        same histories, candidates, exclusions, hidden and scan arguments; k of the pool are picked greedily on the device, each pick
        the position with the largest

            trade_off * r_j - (1 - trade_off) * max over the picks so far of sim(pick -> j)

          r_j         the pool score, with normalize rescaled to [0, 1] over the pool: (s_j - lo) / (hi - lo), 0 when all are equal;
          sim         similar_items' score of the pair (metric, space as there), bit for bit;
          trade_off   1: relevance alone -- recommend_sessions(k) exactly; 0: the best item, then the items least similar to the picks.
        Equal values go to the lower pool position; all arithmetic is fp32 in a fixed order (include/gru4rec_hip.h), so the result
        equals the host loop over recommend_sessions and similar_items it replaces.  The returned scores are the model's scores of
        the chosen items -- recommend_sessions' bit patterns -- in pick order, so they need not descend.  return_hidden appends the
        hidden state as in recommend_sessions; return_details appends (pool_pos[N, k] int32, values[N, k] float32): every pick's
        position in the pool and the value it won with.  Only N x k entries leave the device; the prediction state is neither read
        nor changed.  Everything is checked before any device work: ValueError for a k outside [1, pool], a pool outside
        [1, min(number of candidates, G4R_DIVERSIFY_POOL_MAX = 128)], a trade_off outside [0, 1], a bad metric or space, and
        recommend_sessions' own refusals with k = pool (every session needs `pool` eligible candidate positions); KeyError for an
        unknown item id; NotImplementedError for space='input' on a one-hot input model.  exclude_groups: as in recommend_sessions."""
        if self.error_during_train:
            raise Exception
        pool = _check_k(pool, self._n_candidates(predict_for_item_ids), name='pool', cap=_native.G4R_DIVERSIFY_POOL_MAX)
        k = self._mmr_k(k, pool)
        lam = self._mmr_args(trade_off, metric, space)
        over = self._scan_oversample(scan, oversample, pool)
        N, lens, offs, hidx, h0 = self._session_inputs(histories, hidden)
        iidx, cand = self._candidates(predict_for_item_ids)
        excl = self._session_exclusions(N, lens, hidx, pool, iidx, exclude_history, exclude, exclude_per_row, exclude_groups=exclude_groups)
        m = self._ensure_model()
        out = m.diversify_sessions(offs, hidx, iidx, k, pool, lam, metric, space, bool(normalize), *excl, hidden=h0,
                                   return_hidden=return_hidden, **_scan_kw(over))
        res = (cand[out[0]], out[1])
        if return_hidden:
            res += (self._unpad_hidden(out[4]),)
        if return_details:
            res += (out[2], out[3])
        return res

    @staticmethod
    def _mmr_k(k, pool):
        try:
            ok = not isinstance(k, bool) and int(k) == k and 1 <= k <= pool
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError('k = %r: it must be an integer in [1, pool = %d]' % (k, pool))
        return int(k)

    def diversify_lists(self, item_lists, relevance, k, trade_off=0.7, metric='cosine', space='output', normalize=True):
        """The re-ranker of diversify_sessions for lists from any source (score_candidates, another model, a retrieval stage):
        (pos[N, k] int32, values[N, k] float32).  Not in the reference.

          item_lists  [N, P] item ids, 1 <= P <= G4R_DIVERSIFY_POOL_MAX = 128; duplicates allowed, every position is a candidate.
          relevance   [N, P] finite numbers (taken as float32), the relevance of every position.
        Row i picks k of its P positions as diversify_sessions picks from a pool (same arithmetic, same tie rule: the lower
        position); pos holds the picked positions in pick order, values what each pick won with.  Stateless.  Everything is checked
        before any device work: ragged lists, shapes that differ, a P or k out of range, a relevance that is not finite, a bad
        trade_off, metric or space raise ValueError, an unknown item id KeyError, space='input' on a one-hot input model
        NotImplementedError."""
        if self.error_during_train:
            raise Exception
        try:
            ids = np.asarray(item_lists)
            rel = np.asarray(relevance, dtype=np.float64)
        except (TypeError, ValueError):
            ids = rel = None
        if ids is None or ids.dtype == object or ids.ndim != 2 or rel.shape != ids.shape or ids.shape[0] < 1:
            raise ValueError('item_lists and relevance must be two [N, P] arrays of one shape, N >= 1 (ragged lists are not supported)')
        P = ids.shape[1]
        if not 1 <= P <= _native.G4R_DIVERSIFY_POOL_MAX:
            raise ValueError('the lists hold P = %d items: between 1 and G4R_DIVERSIFY_POOL_MAX = %d are needed' % (P, _native.G4R_DIVERSIFY_POOL_MAX))
        k = self._mmr_k(k, P)
        lam = self._mmr_args(trade_off, metric, space)
        with np.errstate(over='ignore'):      # (a double beyond float32's range becomes inf, which is refused below)
            rel32 = rel.astype(np.float32)
        if not np.isfinite(rel32).all():
            raise ValueError('relevance holds a value that is not finite (as float32)')
        idx = self.itemidmap[ids.ravel()].values.astype(np.int32).reshape(ids.shape)
        m = self._ensure_model()
        return m.diversify_lists(idx, rel32, k, lam, metric, space, bool(normalize))

    # ------------------------------------------------------------------ item groups, per-group caps (not in the reference)
    def set_item_groups(self, groups):
        """Gives the items their groups (a brand, an artist, a category, a parent product): a dict or pandas.Series mapping item id ->
        group label, any hashable; None clears them.  Items of the model that are not mentioned are ungrouped and never capped; an id
        the model does not know raises KeyError, a call before the model has an itemidmap (before fit / loadmodel) ValueError.
        Stores item_groups (int32[n_items] aligned with itemidmap, -1 = ungrouped, otherwise a dense group index) and group_labels
        (the labels in group-index order); both are pickled with the model and uploaded to the device model, now if there is one.
        Used by max_per_group / exclude_groups of recommend_sessions, continue_sessions, diversify_sessions and by cap_lists.  fit on
        data with another item map drops them."""
        if groups is None:
            self.item_groups = self.group_labels = None
            if self._model is not None:
                self._model.set_item_groups(None)
            return
        if getattr(self, 'itemidmap', None) is None:
            raise ValueError('set_item_groups needs the item id map of a fitted or loaded model')
        if isinstance(groups, pd.Series):
            ids, labels = groups.index.values, groups.tolist()
        elif isinstance(groups, dict):
            ids, labels = list(groups.keys()), list(groups.values())
        else:
            raise ValueError('groups must be a dict or a pandas.Series mapping item id -> group label, or None')
        idx = self.itemidmap[ids].values.astype(np.int64) if len(ids) else np.zeros(0, dtype=np.int64)
        index_of = {}
        table = np.full(len(self.itemidmap), -1, dtype=np.int32)
        table[idx] = [index_of.setdefault(lab, len(index_of)) for lab in labels]
        arr = np.empty(len(index_of), dtype=object)
        for lab, i in index_of.items():
            arr[i] = lab
        try:
            plain = np.asarray(list(index_of))
            if plain.shape == arr.shape and plain.dtype != object and plain.tolist() == list(index_of):
                arr = plain      # labels of one plain type: an array of that type
        except (TypeError, ValueError):
            pass
        self.item_groups, self.group_labels = table, arr
        if self._model is not None:
            self._model.set_item_groups(table)

    def _group_indices(self, labels, name):
        """Group labels -> their group indices (int64); ValueError without groups, KeyError for an unknown label."""
        if getattr(self, 'item_groups', None) is None:
            raise ValueError('%s needs item groups: call set_item_groups first' % name)
        index_of = {lab: i for i, lab in enumerate(self.group_labels.tolist())}
        lab = labels.tolist() if isinstance(labels, np.ndarray) else list(labels)
        missing = [x for x in lab if x not in index_of]
        if missing:
            raise KeyError('%s: unknown group label %r' % (name, missing[0]))
        return np.array([index_of[x] for x in lab], dtype=np.int64)

    def _cap_args(self, max_per_group, pool, k, n_cand, count_history=False):
        """The checks of max_per_group / pool (after the k check): (cap, pool) as ints, (None, None) without max_per_group."""
        if max_per_group is None:
            if pool is not None or count_history:
                raise ValueError('pool and count_history belong to max_per_group, which is None')
            return None, None
        if getattr(self, 'item_groups', None) is None:
            raise ValueError('max_per_group needs item groups: call set_item_groups first')
        try:
            ok = not isinstance(max_per_group, bool) and int(max_per_group) == max_per_group and 1 <= max_per_group <= 2 ** 31 - 1
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError('max_per_group = %r: it must be None or an integer >= 1' % (max_per_group,))
        if pool is None:
            pool = min(_native.G4R_TOPK_MAX, n_cand, 4 * k)
        else:
            pool = _check_k(pool, n_cand, name='pool', own_errors=True)
            if k > pool:
                raise ValueError('k = %r: it must be an integer in [1, pool = %d]' % (k, pool))
        return int(max_per_group), pool

    def _prior_groups(self, N, extra, grow):
        """The prior lists of N rows as (offsets int64[N + 1], group indices int32): the groups of `extra` = (rows, item indices),
        ungrouped items dropped (None: every list is empty).  grow: the groups every list gains on the device."""
        counts, gg = np.zeros(N, dtype=np.int64), np.zeros(0, dtype=np.int32)
        if extra is not None:
            rows, g = np.asarray(extra[0], dtype=np.int64), self.item_groups[np.asarray(extra[1], dtype=np.int64)]
            order = np.argsort(rows[g >= 0], kind='stable')
            gg = g[g >= 0][order].astype(np.int32)
            counts = np.bincount(rows[g >= 0], minlength=N)
        big = np.flatnonzero(counts + grow > _native.G4R_GROUP_PRIOR_MAX)
        if len(big):
            raise ValueError('row %d has %d prior groups%s, more than G4R_GROUP_PRIOR_MAX = %d' % (
                big[0], counts[big[0]], ' and gains steps - 1 = %d more' % grow if grow else '', _native.G4R_GROUP_PRIOR_MAX))
        return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), gg

    def cap_lists(self, item_lists, k, max_per_group, prior=None):
        """The walk of recommend_sessions(max_per_group=) for lists from any source: (pos[N, k] int32, n_kept[N] int32).  Not in the
        reference.

          item_lists     [N, P] item ids in rank order, 1 <= P <= G4R_TOPK_MAX = 256; duplicates allowed, every position counts.
          max_per_group  the cap c >= 1 (it needs set_item_groups).
          prior          None, or N sequences of item ids whose groups count against the cap before the list starts (what a page
                         already shows); at most G4R_GROUP_PRIOR_MAX = 1024 grouped items per row.
        Row i keeps position j iff its item is ungrouped or fewer than c positions of its group lie in the prior and ahead of j in
        the list; pos[i] holds the first k kept positions in list order, then -1, n_kept[i] their number.  Stateless.  Everything is
        checked before any device work: ragged lists, a P, k or max_per_group out of range, a prior of the wrong length raise
        ValueError, an unknown item id KeyError."""
        if self.error_during_train:
            raise Exception
        try:
            ids = np.asarray(item_lists)
        except (TypeError, ValueError):
            ids = None
        if ids is None or ids.dtype == object or ids.ndim != 2 or ids.shape[0] < 1:
            raise ValueError('item_lists must be an [N, P] array, N >= 1 (ragged lists are not supported)')
        N, P = ids.shape
        if not 1 <= P <= _native.G4R_TOPK_MAX:
            raise ValueError('the lists hold P = %d items: between 1 and G4R_TOPK_MAX = %d are needed' % (P, _native.G4R_TOPK_MAX))
        k = self._mmr_k(k, P)
        if max_per_group is None:
            raise ValueError('max_per_group = None: it must be an integer >= 1')
        cap, _ = self._cap_args(max_per_group, P, k, P)
        idx = self.itemidmap[ids.ravel()].values.astype(np.int32).reshape(ids.shape)
        extra = None
        if prior is not None:
            if len(prior) != N:
                raise ValueError('prior holds %d lists, one per row (%d) is needed' % (len(prior), N))
            lists = [np.ravel(x) if isinstance(x, np.ndarray) else list(x) for x in prior]
            lens = np.array([len(x) for x in lists], dtype=np.int64)
            flat = np.concatenate([np.asarray(x) for x in lists if len(x)]) if lens.sum() else np.zeros(0, dtype=np.int64)
            extra = (np.repeat(np.arange(N), lens), self.itemidmap[flat].values if len(flat) else flat)
        po, pg = self._prior_groups(N, extra, 0)
        m = self._ensure_model()
        return m.cap_lists(idx, k, cap, po, pg)

    def symbolic_predict(self, X, Y, M, items, batch_size):
        raise NotImplementedError('symbolic_predict builds a Theano graph (gru4rec.py:729-741); the MI355X path '
                                  'exposes the same computation through gru4rec_amd.evaluation.evaluate_gpu')

    # ------------------------------------------------------------------ (de)serialisation (gru4rec.py:742-781)
    _EXTRAS = dict(seed=12345, device=0, use_graph=True, steps_per_call=16384, sync_every='auto', sparse_exact=False, defer_updates=False)     # attributes the reference does not have

    def __getstate__(self):
        st = dict(self.__dict__)
        for k in ('_model', '_plan', '_plan_key', '_data_items', '_offsets', '_base_order', '_dist', '_loss_id', '_final', '_hidden', '_pop64', '_cpu_store', '_seen', '_seen_n', '_seen_over', '_item_index', '_item_index_on', '_store'):
            st.pop(k, None)
        st['predict'] = None
        return st

    def __setstate__(self, st):
        """Accepts pickles of this class and of the reference's (whose state lacks the MI355X extras)."""
        self.__dict__.update(st)
        for k, v in self._EXTRAS.items():
            self.__dict__.setdefault(k, v)
        self.__dict__.setdefault('loss_history', [])
        self.__dict__.setdefault('optimizer_state', None)
        self.__dict__.setdefault('epochs_done', 0)
        self.__dict__.setdefault('error_during_train', False)
        self.__dict__.setdefault('item_groups', None)
        self.__dict__.setdefault('group_labels', None)
        self.set_loss_function(self.loss)
        self.set_final_activation(self.final_act)
        self.set_hidden_activation(self.hidden_act)
        if hasattr(self, 'By') and self.By is not None:
            self.By = np.asarray(self.By, dtype=np.float32).reshape(-1, 1)
        self._model = None
        self._dist = None
        self.predict = None

    def savemodel(self, fname, optimizer_state=False):
        """Pickle with the reference's attribute names / array layouts (Wx[i] (in,3D)=[cand|r|z], Wrz[i] (D,2D)=[r|z],
        Wh[i], Bh[i], H[i], Wy (n_items,D), By (n_items,1), E, itemidmap).  optimizer_state=True adds, under attributes the
        reference's loadmodel never looks at (`optimizer_state`, `epochs_done`), what fit(resume=True) needs to continue: the
        accumulator / velocity arrays, the global step and the sample-store refill count.  The file stays loadable by the
        reference (gru4rec.py:768-781 touches the weight attributes only)."""
        if self._model is not None and not self.error_during_train:
            self._download_weights()
        keep = getattr(self, 'optimizer_state', None)
        if optimizer_state:
            if self._model is None:
                raise ValueError('optimizer_state=True needs the trained device model (call savemodel before close())')
            self.optimizer_state = self._download_optimizer_state()
        else:
            self.optimizer_state = None
        try:
            with open(fname, 'wb') as f:
                pickle.dump(self, f)
        finally:
            if not optimizer_state:
                self.optimizer_state = keep

    @classmethod
    def loadmodel(cls, fname):
        """gru4rec.py:768-781.  Reads checkpoints written by this class and by the reference's `savemodel` (both name the
        class `gru4rec.GRU4Rec`; the reference's arrays are plain NumPy in the pickle, :744-756)."""
        class _Opaque:
            """Stand-in for Theano / pygpu objects inside a reference pickle (sample store, RNG state, compiled
            functions left on the object after fit): they are rebuilt by fit() / predict here, never read."""
            def __init__(self, *a, **k):
                pass

            def __setstate__(self, st):
                pass

        class _Unpickler(pickle.Unpickler):
            def find_class(self, module, name):
                if module.split('.')[0] in ('theano', 'pygpu'):
                    return _Opaque
                if module in ('gru4rec', 'gru4rec_amd.gru4rec'):
                    obj = sys.modules[cls.__module__] if cls.__module__ in sys.modules else None
                    target = cls
                    parts = name.split('.')
                    if parts[0] == 'GRU4Rec':
                        for part in parts[1:]:
                            target = getattr(target, part)
                        return target
                    if obj is not None and hasattr(obj, name):
                        return getattr(obj, name)
                return super().find_class(module, name)
        with open(fname, 'rb') as f:
            gru = _Unpickler(f).load()
        for k in [k for k, v in gru.__dict__.items() if isinstance(v, _Opaque)]:
            del gru.__dict__[k]
        gru._model = None
        gru.predict = None
        return gru


# Checkpoints name the class `gru4rec.GRU4Rec`, exactly like the reference's (gru4rec.py:755), so they load on either side;
# `gru4rec.py` at the repository root re-exports this class under that module name.
GRU4Rec.__module__ = 'gru4rec'
GRU4Rec.__qualname__ = 'GRU4Rec'
for _c in (GRU4Rec.Selu, GRU4Rec.Elu, GRU4Rec.LeakyReLU):
    _c.__module__ = 'gru4rec'
sys.modules.setdefault('gru4rec', sys.modules[__name__])     # so pickle can resolve the name without the root shim

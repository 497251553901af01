"""ctypes binding of libgru4rec_hip.so (C ABI: include/gru4rec_hip.h).

The library is built in-tree by `__graft_entry__.build()` / `python -m gru4rec_amd.build`.  There is no
CPU fallback: if the shared object is missing, or no MI355X is visible, the product path raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('G4R_LIB') or os.path.join(_HERE, 'libgru4rec_hip.so')   # G4R_LIB: developer override

G4R_MAX_LAYERS = 8
G4R_TOPK_MAX = 256      # largest k of g4r_recommend_step
G4R_BEAM_MAX = 32       # widest beam of g4r_beam_sessions
G4R_SAMPLE_MAX = 64     # most draws per session of g4r_sample_sessions
G4R_AUDIENCE_MAX = 65536           # largest k of g4r_audience_sessions,
G4R_AUDIENCE_ITEMS_MAX = 4096      # most items of one call,
G4R_AUDIENCE_ENTRIES_MAX = 2 ** 23 # and the most items x k
AUDIENCE_BY = {'score': 0, 'logprob': 1}      # G4R_AUDIENCE_*
G4R_STREAM_GUMBEL = 0x47554D42      # Philox stream id (counter word 3) of its noise
BEAM_COMBINE = {'sum': 0, 'product': 1}      # G4R_BEAM_*
G4R_EXCLUDE_MAX = 1024  # most distinct items one row of g4r_recommend_step_filtered may exclude
G4R_CAND_MAX = 2 ** 31 - 256  # most candidate positions of one g4r_score_candidates* call
G4R_DIVERSIFY_POOL_MAX = 128  # largest pool of g4r_diversify_lists / g4r_diversify_sessions
G4R_GROUP_PRIOR_MAX = 1024  # most prior groups of one row of g4r_continue_sessions_capped / g4r_cap_lists
G4R_SCAN_CAND_MAX = 1024  # most candidates per row (k * oversample) of g4r_recommend_step_scan / g4r_recommend_sessions_scan
G4R_IVF_LISTS_MAX = 65536   # most lists of an item index (g4r_ivf_set)
G4R_IVF_NPROBE_MAX = 256    # most lists one row of g4r_recommend_sessions_ivf probes
G4R_IVF_WS_MAX = 65536      # largest nprobe * candidates per row of that entry (its stage-1 lists: rows * nprobe * c * 8 bytes)
LOSS_IDS = {'cross-entropy': 0, 'bpr-max': 1, 'top1-max': 2, 'bpr': 3, 'top1': 4, 'xe_logit': 5}
ACT_IDS = {'linear': 0, 'relu': 1, 'tanh': 2, 'leaky': 3, 'elu': 4, 'selu': 5, 'softmax': 6, 'softmax_logit': 7}
ADAPT_IDS = {'adagrad': 0, 'rmsprop': 1, 'adadelta': 2, 'adam': 3, None: 4}
RANK_MODES = {'standard': 0, 'conservative': 1, 'median': 2, 'tiebreaking': 3}
EMBED_CONSTRAINED, EMBED_SEPARATE, EMBED_ONEHOT = 0, 1, 2
SIM_METRICS = {'dot': 0, 'cosine': 1}      # G4R_SIM_*
SIM_SPACES = {'output': 0, 'input': 1}     # G4R_SPACE_*


class G4RConfig(C.Structure):
    _fields_ = [
        ('n_items', C.c_int32), ('n_layers', C.c_int32), ('layers', C.c_int32 * G4R_MAX_LAYERS),
        ('batch_size', C.c_int32), ('n_sample', C.c_int32), ('loss', C.c_int32),
        ('final_act', C.c_int32), ('final_act_p0', C.c_float), ('final_act_p1', C.c_float),
        ('hidden_act', C.c_int32), ('hidden_act_p0', C.c_float), ('hidden_act_p1', C.c_float),
        ('embed_mode', C.c_int32), ('embedding', C.c_int32),
        ('learning_rate', C.c_float), ('momentum', C.c_float), ('lmbd', C.c_float), ('bpreg', C.c_float),
        ('logq', C.c_float), ('sample_alpha', C.c_float),
        ('dropout_p_hidden', C.c_float), ('dropout_p_embed', C.c_float),
        ('sample_store', C.c_int64), ('seed', C.c_uint64),
        ('device', C.c_int32), ('rank', C.c_int32), ('nranks', C.c_int32), ('use_graph', C.c_int32),
        ('smoothing', C.c_float), ('adapt', C.c_int32), ('adapt_p0', C.c_float), ('adapt_p1', C.c_float),
        ('grad_cap', C.c_float), ('sparse_exact', C.c_int32), ('defer_updates', C.c_int32),
    ]


# every symbol include/gru4rec_hip.h declares (checked by tests/test_abi.py)
SYMBOLS = [
    'g4r_device_count', 'g4r_last_error', 'g4r_version', 'g4r_sizeof_config', 'g4r_create', 'g4r_destroy', 'g4r_set_param',
    'g4r_get_param', 'g4r_set_popularity', 'g4r_set_sample_store', 'g4r_get_sample_store',
    'g4r_sample_store_rows', 'g4r_build_plan', 'g4r_set_plan', 'g4r_train_steps', 'g4r_get_losses',
    'g4r_synchronize', 'g4r_global_step', 'g4r_refills', 'g4r_set_step_counters', 'g4r_kernel_time', 'g4r_profile', 'g4r_reset_hidden',
    'g4r_predict_begin', 'g4r_predict_hidden', 'g4r_predict_step', 'g4r_recommend_step', 'g4r_recommend_step_filtered', 'g4r_recommend_sessions', 'g4r_recommend_step_scan', 'g4r_recommend_sessions_scan', 'g4r_continue_sessions', 'g4r_store_open', 'g4r_store_close', 'g4r_store_push', 'g4r_store_peek', 'g4r_store_read', 'g4r_store_write', 'g4r_beam_sessions', 'g4r_sample_sessions', 'g4r_sample_sessions_lp', 'g4r_session_log_partition', 'g4r_audience_sessions', 'g4r_scan_table_release', 'g4r_ivf_assign', 'g4r_ivf_set', 'g4r_ivf_release', 'g4r_recommend_sessions_ivf', 'g4r_similar_items', 'g4r_diversify_lists', 'g4r_diversify_sessions', 'g4r_set_item_groups', 'g4r_get_item_groups', 'g4r_recommend_sessions_capped', 'g4r_continue_sessions_capped', 'g4r_cap_lists', 'g4r_score_candidates', 'g4r_score_candidates_sessions', 'g4r_rank_targets', 'g4r_evaluate', 'g4r_recommend_events', 'g4r_loglik_events', 'g4r_comm_unique_id',
    'g4r_comm_init', 'g4r_virtual_train_steps', 'g4r_virtual_sync_dense', 'g4r_comm_sync_sparse', 'g4r_sync_set_rule', 'g4r_set_sync_every', 'g4r_comm_min_i64', 'g4r_comm_max_i64', 'g4r_comm_nranks', 'g4r_p2p_enable', 'g4r_p2p_export', 'g4r_p2p_attach', 'g4r_p2p_active', 'g4r_sync_enable', 'g4r_sync_row_floats', 'g4r_sync_export', 'g4r_sync_import', 'g4r_get_debug', 'g4r_debug_loss_rows', 'g4r_debug_gumbel', 'g4r_debug_lse_terms', 'g4r_stress_start', 'g4r_stress_stop', 'g4r_selftest_mfma', 'g4r_bench_rows',
    'g4r_events_load', 'g4r_events_rows', 'g4r_events_items', 'g4r_events_item_bytes', 'g4r_events_time_kind',
    'g4r_events_copy', 'g4r_events_free',
]

# the pointer types of the ABI
f32p, f64p, i32p, i64p, u8p, u32p = (C.POINTER(t) for t in (C.c_float, C.c_double, C.c_int32, C.c_int64, C.c_uint8, C.c_uint32))
f32pp = C.POINTER(f32p)      # one float array per layer
u64p = C.POINTER(C.c_uint64)

_lib = None


def beam_backtrack(parent, cols, step_scores):
    """The paths of g4r_beam_sessions' final beams out of its back-pointer records ([n, steps, beams] each: beam i of step s extends
    beam parent[n, s, i] of step s - 1 by cols[n, s, i], scored step_scores[n, s, i]): (paths[n, beams, steps] in the dtype of cols,
    scores float32[n, beams, steps]), final beam i read backwards from the last step."""
    parent, cols, step_scores = np.asarray(parent), np.asarray(cols), np.asarray(step_scores)
    n, steps, beams = parent.shape
    paths = np.empty((n, beams, steps), dtype=cols.dtype)
    scores = np.empty((n, beams, steps), dtype=np.float32)
    row = np.arange(n)[:, None]
    cur = np.tile(np.arange(beams), (n, 1))
    for s in range(steps - 1, -1, -1):
        paths[:, :, s] = cols[row, s, cur]
        scores[:, :, s] = step_scores[row, s, cur]
        cur = parent[row, s, cur]
    return paths, scores


class NativeError(RuntimeError):
    pass


def lib():
    """Load the shared library (once).  Raises NativeError when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeError('libgru4rec_hip.so is not built (%s). Run `python -c "import __graft_entry__ as g; '
                          'g.build()"` -- the MI355X path has no CPU fallback.' % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    L.g4r_device_count.restype = C.c_int
    L.g4r_last_error.restype = C.c_char_p
    L.g4r_version.restype = C.c_char_p
    L.g4r_create.argtypes = [C.POINTER(G4RConfig), C.POINTER(vp)]
    L.g4r_destroy.argtypes = [vp]
    L.g4r_destroy.restype = None
    L.g4r_set_param.argtypes = [vp, C.c_char_p, i32, f32p, i64]
    L.g4r_get_param.argtypes = [vp, C.c_char_p, i32, f32p, i64]
    L.g4r_set_popularity.argtypes = [vp, f32p, f32p, f32p, i64]
    L.g4r_set_sample_store.argtypes = [vp, i32p, i64]
    L.g4r_get_sample_store.argtypes = [vp, i32p, i64]
    L.g4r_sample_store_rows.argtypes = [vp]
    L.g4r_sample_store_rows.restype = i64
    L.g4r_build_plan.argtypes = [i32p, i64, i64p, i32p, i32, i32, i32p, i32p, u8p, i32p, i64p, i32p, i64, i64, i64p]
    L.g4r_build_plan.restype = i64
    L.g4r_set_plan.argtypes = [vp, i32p, i32p, u8p, i32p, i64, i64p, i32p, i64]
    L.g4r_train_steps.argtypes = [vp, i64, i64]
    L.g4r_get_losses.argtypes = [vp, i64, i64, f32p]
    L.g4r_synchronize.argtypes = [vp]
    L.g4r_global_step.argtypes = [vp]
    L.g4r_global_step.restype = i64
    L.g4r_refills.argtypes, L.g4r_refills.restype = [vp], i64
    L.g4r_set_step_counters.argtypes = [vp, i64, i64]
    L.g4r_kernel_time.argtypes = [vp, i32, C.POINTER(C.c_char_p), f64p, i64p]
    L.g4r_profile.argtypes = [vp, i32]
    L.g4r_reset_hidden.argtypes = [vp]
    L.g4r_predict_begin.argtypes = [vp, i32]
    L.g4r_predict_hidden.argtypes = [vp, u8p, i32, i32p, i32]
    L.g4r_predict_step.argtypes = [vp, i32p, i32, i32p, i64, f32p]
    L.g4r_recommend_step.argtypes = [vp, i32p, i32, i32p, i64, i32, i32p, f32p]
    L.g4r_recommend_step_filtered.argtypes = [vp, i32p, i32, i32p, i64, i32, i64p, i32p, u32p, i32p, f32p]
    L.g4r_recommend_sessions.argtypes = [vp, i64p, i32p, i32, f32pp, i32p, i64, i32, i64p, i32p, u32p, i32p, f32p, f32pp]
    L.g4r_recommend_step_scan.argtypes = [vp, i32p, i32, i32p, i64, i32, i32, i64p, i32p, u32p, i32p, f32p]
    L.g4r_recommend_sessions_scan.argtypes = [vp, i64p, i32p, i32, f32pp, i32p, i64, i32, i32, i64p, i32p, u32p, i32p, f32p,
                                              f32pp]
    L.g4r_continue_sessions.argtypes = [vp, i64p, i32p, i32, f32pp, i32p, i64, i32, i32, i32, i32, i64p, i32p, u32p, i32p, f32p, f32pp]
    L.g4r_store_open.argtypes = [vp, i64, i32]
    L.g4r_store_close.argtypes = [vp]
    L.g4r_store_push.argtypes = [vp, i64p, i32p, i32p, i32p, i32, i32p, i64, i32, i32, i32, u32p, i32p, f32p, i32p]
    L.g4r_store_peek.argtypes = [vp, i32p, i32, i32p, i64, i32, i32, i32, u32p, i32p, f32p, i32p]
    L.g4r_store_read.argtypes = [vp, i32p, i32, f32pp, i32p, i32p, i32p]
    L.g4r_store_write.argtypes = [vp, i32p, i32, f32pp, i32p, i32p, i32p]
    L.g4r_beam_sessions.argtypes = [vp, i64p, i32p, i32, f32pp, i32p, i64, i32, i32, i32, i32, i32, i64p, i32p, u32p, i32p, i32p,
                                    f32p, f32p, i32p]
    L.g4r_sample_sessions.argtypes = [vp, i64p, i32p, i32, f32pp, i32p, i64, i32, i32, i64p, i32p, u32p, i32, i32, C.c_float, C.c_uint64, i32,
                                      i32p, f32p, f32pp]
    L.g4r_sample_sessions_lp.argtypes = L.g4r_sample_sessions.argtypes + [C.c_float, f32p]
    L.g4r_session_log_partition.argtypes = [vp, i64p, i32p, i32, f32pp, i32p, i64, i64p, i32p, u32p, C.c_float, f32p, u64p]
    L.g4r_audience_sessions.argtypes = [vp, i64p, i32p, i32, f32pp, i32p, i32, i32, i32, C.c_float, i32, i32p, f32p, i32p]
    L.g4r_scan_table_release.argtypes = [vp]
    L.g4r_ivf_assign.argtypes = [vp, f32p, i32, i32p]
    L.g4r_ivf_set.argtypes = [vp, f32p, i32, i64p, i32p]
    L.g4r_ivf_release.argtypes = [vp]
    L.g4r_recommend_sessions_ivf.argtypes = [vp, i64p, i32p, i32, f32pp, i32, i32, i32, i64p, i32p, u32p, i32p, f32p, i32p, f32pp, i32p]
    L.g4r_similar_items.argtypes = [vp, i32, i32, i32p, i64, i32p, i64, i32, i32, u32p, i32p, f32p]
    L.g4r_diversify_lists.argtypes = [vp, i32, i32, i32p, f32p, i64, i32, i32, C.c_float, i32, i32p, f32p]
    L.g4r_diversify_sessions.argtypes = [vp, i64p, i32p, i32, f32pp, i32p, i64, i32, i32, i32, i64p, i32p, u32p, i32, i32, C.c_float, i32,
                                         i32p, f32p, i32p, f32p, f32pp]
    L.g4r_set_item_groups.argtypes = [vp, i32p, i64]
    L.g4r_get_item_groups.argtypes = [vp, i32p, i64]
    L.g4r_recommend_sessions_capped.argtypes = [vp, i64p, i32p, i32, f32pp, i32p, i64, i32, i32, i32, i64p, i32p, u32p, i32, i32p, f32p, i32p,
                                                i32p, f32pp]
    L.g4r_continue_sessions_capped.argtypes = [vp, i64p, i32p, i32, f32pp, i32p, i64, i32, i32, i32, i32, i32, i64p, i32p, u32p, i32, i64p,
                                               i32p, i32p, f32p, i32p, f32pp]
    L.g4r_cap_lists.argtypes = [vp, i32p, i64, i32, i32, i32, i64p, i32p, i32p, i32p]
    L.g4r_score_candidates.argtypes = [vp, i32p, i32, i64p, i32p, i32, f32p, i32p]
    L.g4r_score_candidates_sessions.argtypes = [vp, i64p, i32p, i32, f32pp, i64p, i32p, i32, f32p, i32p, f32pp]
    L.g4r_rank_targets.argtypes = [vp, i32p, i32, i64, i32, f32p]
    L.g4r_evaluate.argtypes = [vp, i32p, i32p, u8p, i32p, i64, i32, i64p, i32p, i64, i32p, i64, i32p, i32, i32, f64p, f64p, i64p]
    L.g4r_recommend_events.argtypes = [vp, i32p, i32p, u8p, i32p, i64, i32, i64p, i32p, i64, i32p, i64, i32, i64p, i64, i32,
                                       u32p, i64p, i32p, i32p, i64, i32p, i32p, i32p, f32p, f32p, f32p]
    L.g4r_loglik_events.argtypes = [vp, i32p, i32p, u8p, i32p, i64, i32, i64p, i32p, i64, i32p, i64, i64p, i64,
                                    u32p, i64p, i32p, i32p, i64, i32p, i32p, C.c_float, f32p, f32p, u64p, u8p]
    L.g4r_comm_unique_id.argtypes = [C.c_char_p]
    L.g4r_comm_init.argtypes = [vp, C.c_char_p, i32, i32]
    L.g4r_comm_sync_sparse.argtypes = [vp]
    L.g4r_virtual_train_steps.argtypes = [C.POINTER(vp), i32, i64, i64]
    L.g4r_virtual_sync_dense.argtypes = [C.POINTER(vp), i32]
    L.g4r_sync_set_rule.argtypes = [vp, i32, i32]
    L.g4r_set_sync_every.argtypes = [vp, i32]
    L.g4r_comm_min_i64.argtypes = [vp, i64p]
    L.g4r_comm_max_i64.argtypes = [vp, i64p]
    L.g4r_comm_nranks.argtypes = [vp]
    L.g4r_p2p_enable.argtypes = [vp]
    L.g4r_p2p_export.argtypes = [vp, C.c_char_p]
    L.g4r_p2p_attach.argtypes = [vp, C.c_char_p, i32, i32]
    L.g4r_p2p_active.argtypes = [vp]
    L.g4r_sync_enable.argtypes = [vp]
    L.g4r_sync_row_floats.argtypes, L.g4r_sync_row_floats.restype = [vp, i32], i64
    L.g4r_sync_export.argtypes, L.g4r_sync_export.restype = [vp, i32, i32p, f32p, i64], i64
    L.g4r_sync_import.argtypes = [vp, i32, i32, i64p, C.POINTER(i32p), f32pp]
    L.g4r_get_debug.argtypes = [vp, C.c_char_p, f32p, i64]
    L.g4r_debug_loss_rows.argtypes = [vp, f32p, i64, i32, f32p]
    L.g4r_debug_gumbel.argtypes = [vp, C.c_uint64, C.c_uint32, C.c_uint32, i32p, i64, f32p]
    L.g4r_debug_lse_terms.argtypes = [vp, f32p, f32p, i64, C.c_float, u64p]
    L.g4r_selftest_mfma.argtypes = [f32p]
    L.g4r_stress_start.argtypes = [i32, i64, i32, C.POINTER(vp)]
    L.g4r_stress_stop.argtypes = [vp]
    L.g4r_bench_rows.argtypes = [i32, i64, i32, i64, i32, i32, C.c_uint64, f64p, f64p]
    L.g4r_events_load.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, i32, C.POINTER(vp)]
    for fn in (L.g4r_events_rows, L.g4r_events_items, L.g4r_events_item_bytes):
        fn.argtypes, fn.restype = [vp], i64
    L.g4r_events_time_kind.argtypes, L.g4r_events_time_kind.restype = [vp], i32
    L.g4r_events_copy.argtypes = [vp, i32p, i32p, vp, i64p, C.c_char_p]
    L.g4r_events_free.argtypes, L.g4r_events_free.restype = [vp], None
    if L.g4r_sizeof_config() != C.sizeof(G4RConfig):
        raise NativeError('g4r_config layout mismatch between the header and the ctypes binding')
    _lib = L
    return L


def device_count():
    return int(lib().g4r_device_count())


def _chk(rc):
    if rc != 0:
        raise NativeError(lib().g4r_last_error().decode())


def _ptr(ptr):
    """The converter of an array to a pointer of type ptr to its data; None stays None (NULL)."""
    return lambda a: None if a is None else a.ctypes.data_as(ptr)


_f32, _f64, _i32, _i64, _u8, _u32, _u64 = (_ptr(t) for t in (f32p, f64p, i32p, i64p, u8p, u32p, u64p))


# -- the argument families of the inference entries.  Every array a packer returns has to stay referenced until the C call returns.
def _arr(a, dtype):
    return None if a is None else np.ascontiguousarray(a, dtype=dtype)


def _cand(item_idx, n_items):
    """item_idx as (int32 array or None, number of candidates): without it the candidates are all items."""
    if item_idx is None:
        return None, n_items
    it = np.ascontiguousarray(item_idx, dtype=np.int32)
    return it, len(it)


def _hist(hist_offs, hist_items):
    """The history CSR of the session entries: (offsets int64[n + 1], item indices int32, n)."""
    offs = np.ascontiguousarray(hist_offs, dtype=np.int64)
    items = np.ascontiguousarray(hist_items, dtype=np.int32)
    n = len(offs) - 1
    if n < 1 or offs[0] < 0 or offs[-1] > len(items):
        raise ValueError('hist_offs must hold n + 1 >= 2 offsets into hist_items')
    return offs, items, n


def _mask(excl_mask, n_items):
    mask = _arr(excl_mask, np.uint32)
    if mask is not None and len(mask) < (n_items + 31) // 32:
        raise ValueError('excl_mask must hold ceil(n_items / 32) words')
    return mask


def _excl(rows, excl_offs, excl_items, excl_mask, n_items, rows_word):
    """The exclusions of a call with `rows` rows: (offsets int64[rows + 1] or None, item indices int32 -- empty without lists,
    never None --, mask words uint32 or None).  rows_word: what the refusal calls the rows ('rows' / 'n')."""
    offs = _arr(excl_offs, np.int64)
    items = np.ascontiguousarray(np.zeros(0) if excl_items is None else excl_items, dtype=np.int32)
    if offs is not None and (len(offs) != rows + 1 or offs[-1] > len(items) or offs[0] < 0):
        raise ValueError('excl_offs must hold %s + 1 offsets into excl_items' % rows_word)
    return offs, items, _mask(excl_mask, n_items)


def _layer_pointers(arrays):
    return (f32p * len(arrays))(*[_f32(a) for a in arrays])


def _hidden_in(hidden, n, layers):
    """The initial hidden state of a session entry: (float32 arrays [n, layers[l]], float*[len(layers)] over them); (None, None)
    without one."""
    if hidden is None:
        return None, None
    if len(hidden) != len(layers):
        raise ValueError('hidden holds %d arrays, one per layer (%d) is needed' % (len(hidden), len(layers)))
    h0 = [np.ascontiguousarray(h, dtype=np.float32) for h in hidden]
    for l, h in enumerate(h0):
        if h.shape != (n, layers[l]):
            raise ValueError('hidden[%d] has shape %s, (%d, %d) is needed' % (l, h.shape, n, layers[l]))
    return h0, _layer_pointers(h0)


def _hidden_out(n, layers, want):
    """Room for the hidden state a session entry returns, as _hidden_in; (None, None) when it is not wanted."""
    if not want:
        return None, None
    hout = [np.empty((n, D), dtype=np.float32) for D in layers]
    return hout, _layer_pointers(hout)


def _topk_out(shape):
    return np.empty(shape, dtype=np.int32), np.empty(shape, dtype=np.float32)


def _plan(plan, dummy_batch=None):
    """The arrays of a plan for g4r_set_plan / g4r_evaluate / g4r_recommend_events, in the order the entries take them: (in_idx,
    out_idx, reset, M, compact_steps, compact_maps, n_compact).  A plan without compaction tables (n_compact == 0) has None (NULL)
    for the two -- what g4r_set_plan takes -- or, with dummy_batch, one zeroed entry and one zeroed row of that width, which the
    other two entries want."""
    nc = int(plan.get('n_compact', 0))
    if nc:
        cs, cm = np.ascontiguousarray(plan['compact_steps'], dtype=np.int64), np.ascontiguousarray(plan['compact_maps'], dtype=np.int32)
    elif dummy_batch is None:
        cs = cm = None
    else:
        cs, cm = np.zeros(1, dtype=np.int64), np.zeros((1, dummy_batch), dtype=np.int32)
    ii, oi, mm = (np.ascontiguousarray(plan[key], dtype=np.int32) for key in ('in_idx', 'out_idx', 'M'))
    return ii, oi, np.ascontiguousarray(plan['reset'], dtype=np.uint8), mm, cs, cm, nc


IO_UNSUPPORTED = 1      # G4R_IO_UNSUPPORTED


def load_events(path, session_col, item_col, time_col=None, threads=0):
    """Native TSV parse (g4r_events_load): dict(session int32[n], item_idx int32[n], time int64|float64[n] or None,
    item_ids list[str] in index order = order of first appearance), or None when the file needs pandas' general parser."""
    L = lib()
    h = C.c_void_p()
    rc = L.g4r_events_load(os.fsencode(path), session_col.encode(), item_col.encode(),
                           None if time_col is None else time_col.encode(), threads, C.byref(h))
    if rc == IO_UNSUPPORTED:
        return None
    _chk(rc)
    try:
        n, k, nb, kind = L.g4r_events_rows(h), L.g4r_events_items(h), L.g4r_events_item_bytes(h), L.g4r_events_time_kind(h)
        session = np.empty(n, dtype=np.int32)
        item_idx = np.empty(n, dtype=np.int32)
        time = None if kind == 0 else np.empty(n, dtype=np.int64 if kind == 1 else np.float64)
        off = np.empty(k + 1, dtype=np.int64)
        raw = C.create_string_buffer(max(int(nb), 1))
        _chk(L.g4r_events_copy(h, _i32(session), _i32(item_idx), _ptr(C.c_void_p)(time),
                               _i64(off), raw))
    finally:
        L.g4r_events_free(h)
    try:
        blob = raw.raw[:nb].decode('utf-8')
    except UnicodeDecodeError:
        return None      # item ids in another encoding: pandas' reader decides how to read them
    lo = off.tolist()
    if len(blob) == nb:      # pure ASCII: byte offsets are character offsets
        ids = [blob[lo[i]:lo[i + 1]] for i in range(k)]
    else:
        rb = raw.raw
        ids = [rb[lo[i]:lo[i + 1]].decode('utf-8') for i in range(k)]
    return dict(session=session, item_idx=item_idx, time=time, item_ids=ids)


def build_plan(offset_sessions, session_order, data_items, batch_size, n_sample):
    """Host scheduler (no GPU): the (X, Y, M, R) stream of one epoch, gru4rec.py:594-651."""
    L = lib()
    off = np.ascontiguousarray(offset_sessions, dtype=np.int32)
    order = np.ascontiguousarray(session_order, dtype=np.int64)
    items = np.ascontiguousarray(data_items, dtype=np.int32)
    n_sess = len(off) - 1
    nc = C.c_int64(0)
    T = L.g4r_build_plan(_i32(off), n_sess, _i64(order), _i32(items), batch_size, n_sample,
                         None, None, None, None, None, None, 0, 0, C.byref(nc))
    if T < 0:
        raise NativeError(L.g4r_last_error().decode())
    B = batch_size
    plan = dict(in_idx=np.zeros((max(T, 1), B), dtype=np.int32), out_idx=np.zeros((max(T, 1), B), dtype=np.int32),
                reset=np.zeros((max(T, 1), B), dtype=np.uint8), M=np.zeros(max(T, 1), dtype=np.int32),
                compact_steps=np.zeros(max(nc.value, 1), dtype=np.int64),
                compact_maps=np.full((max(nc.value, 1), B), -1, dtype=np.int32))
    nc2 = C.c_int64(0)
    T2 = L.g4r_build_plan(_i32(off), n_sess, _i64(order), _i32(items), batch_size, n_sample,
                          _i32(plan['in_idx']), _i32(plan['out_idx']), _u8(plan['reset']), _i32(plan['M']),
                          _i64(plan['compact_steps']), _i32(plan['compact_maps']), max(T, 1), max(nc.value, 1),
                          C.byref(nc2))
    if T2 != T:
        raise NativeError('plan builder is not deterministic: %s' % L.g4r_last_error().decode())
    plan['T'] = int(T)
    plan['n_compact'] = int(nc.value)
    for k in ('in_idx', 'out_idx', 'reset', 'M'):
        plan[k] = plan[k][:T]
    plan['compact_steps'] = plan['compact_steps'][:nc.value]
    plan['compact_maps'] = plan['compact_maps'][:nc.value]
    return plan


class Model:
    """Thin RAII wrapper over a g4r_model handle."""

    def __init__(self, **kw):
        L = lib()
        if L.g4r_device_count() <= 0:
            raise NativeError('no MI355X / HIP device visible: the gfx950 path has no CPU fallback')
        cfg = G4RConfig()
        layers = list(kw.pop('layers'))
        cfg.n_layers = len(layers)
        for i, d in enumerate(layers):
            cfg.layers[i] = int(d)
        for k, v in kw.items():
            setattr(cfg, k, v)
        self.cfg = cfg
        self.layers = layers
        self.h = C.c_void_p()
        _chk(L.g4r_create(C.byref(cfg), C.byref(self.h)))
        self.T = 0

    def close(self):
        if getattr(self, 'h', None):
            lib().g4r_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- parameters
    def set_param(self, name, arr, layer=0):
        a = np.ascontiguousarray(arr, dtype=np.float32)
        _chk(lib().g4r_set_param(self.h, name.encode(), layer, _f32(a), a.size))

    def get_param(self, name, shape, layer=0):
        a = np.empty(shape, dtype=np.float32)
        _chk(lib().g4r_get_param(self.h, name.encode(), layer, _f32(a), a.size))
        return a

    def scan_table(self):
        """State of the bf16 shadow table of the two-stage top-k: (bytes held, valid, builds so far)."""
        a = self.get_debug('scan_table', 3)
        return int(a[0]), bool(a[1]), int(a[2])

    def scan_table_release(self):
        _chk(lib().g4r_scan_table_release(self.h))

    def get_debug(self, name, shape):
        a = np.empty(shape, dtype=np.float32)
        _chk(lib().g4r_get_debug(self.h, name.encode(), _f32(a), a.size))
        return a

    def debug_loss_rows(self, scores, M):
        """The loss launch of a training step on the score rows `scores` ([batch_size, ldSc], a copy is taken) with M active rows
        (g4r_debug_loss_rows): (d cost / d s float32[batch_size, ldSc], row losses float32[batch_size], rows < M written)."""
        ds = np.array(scores, dtype=np.float32, order='C')
        if ds.ndim != 2:
            raise ValueError('scores must be a [batch_size, ldSc] matrix')
        lossrow = np.zeros(ds.shape[0], dtype=np.float32)
        _chk(lib().g4r_debug_loss_rows(self.h, _f32(ds), ds.size, int(M), _f32(lossrow)))
        return ds, lossrow

    # -- sampling
    def set_popularity(self, cum_p, lq_tgt=None, lq_smp=None):
        p = np.ascontiguousarray(cum_p, dtype=np.float32)
        a, b = _arr(lq_tgt, np.float32), _arr(lq_smp, np.float32)
        _chk(lib().g4r_set_popularity(self.h, _f32(p), _f32(a), _f32(b), p.size))

    def sample_store_rows(self):
        return int(lib().g4r_sample_store_rows(self.h))

    def set_sample_store(self, st):
        a = np.ascontiguousarray(st, dtype=np.int32)
        _chk(lib().g4r_set_sample_store(self.h, _i32(a), a.shape[0]))

    def get_sample_store(self, n_sample):
        rows = self.sample_store_rows()
        a = np.empty((rows, n_sample), dtype=np.int32)
        _chk(lib().g4r_get_sample_store(self.h, _i32(a), rows))
        return a

    # -- plan + training
    def set_plan(self, plan):
        in_idx, out_idx, reset, M, cs, cm, nc = _plan(plan)
        _chk(lib().g4r_set_plan(self.h, _i32(in_idx), _i32(out_idx), _u8(reset), _i32(M), len(M), _i64(cs), _i32(cm), nc))
        self.T = len(M)

    def train_steps(self, t0, n):
        _chk(lib().g4r_train_steps(self.h, t0, n))

    def get_losses(self, t0, n):
        a = np.empty(n, dtype=np.float32)
        _chk(lib().g4r_get_losses(self.h, t0, n, _f32(a)))
        return a

    def reset_hidden(self):
        _chk(lib().g4r_reset_hidden(self.h))

    def global_step(self):
        return int(lib().g4r_global_step(self.h))

    def refills(self):
        return int(lib().g4r_refills(self.h))

    def set_step_counters(self, global_step, refills):
        _chk(lib().g4r_set_step_counters(self.h, int(global_step), int(refills)))

    def profile(self, enable):
        """False / True, or 2: profile with the update launch split into its two roles (k_dense_grad, k_sparse_update)."""
        _chk(lib().g4r_profile(self.h, 2 if enable == 2 else (1 if enable else 0)))

    def kernel_times(self):
        out = {}
        i = 0
        while True:
            name = C.c_char_p()
            ms = C.c_double()
            n = C.c_int64()
            if lib().g4r_kernel_time(self.h, i, C.byref(name), C.byref(ms), C.byref(n)) != 0:
                break
            if n.value:
                out[name.value.decode()] = (ms.value, n.value)
            i += 1
        return out

    # -- prediction
    def predict_begin(self, batch):
        _chk(lib().g4r_predict_begin(self.h, batch))

    def predict_hidden(self, zero_mask=None, keep_rows=None):
        z, k = _arr(zero_mask, np.uint8), _arr(keep_rows, np.int32)
        _chk(lib().g4r_predict_hidden(self.h, _u8(z), 0 if z is None else len(z), _i32(k), 0 if k is None else len(k)))

    def predict_step(self, in_idx, item_idx=None, want_scores=True):
        ii = np.ascontiguousarray(in_idx, dtype=np.int32)
        it, n_sel = _cand(item_idx, self.cfg.n_items)
        out = np.empty((len(ii), n_sel), dtype=np.float32) if want_scores else None
        _chk(lib().g4r_predict_step(self.h, _i32(ii), len(ii), _i32(it), n_sel, _f32(out)))
        return out

    def recommend_step(self, in_idx, item_idx=None, k=20):
        """The k best candidates of every row of the scores predict_step would return (g4r_recommend_step; same hidden-state
        update): (cols int32[rows, k], scores float32[rows, k]); cols are positions in item_idx (item indices without it)."""
        ii = np.ascontiguousarray(in_idx, dtype=np.int32)
        it, n_sel = _cand(item_idx, self.cfg.n_items)
        cols, scores = _topk_out((len(ii), k))
        _chk(lib().g4r_recommend_step(self.h, _i32(ii), len(ii), _i32(it), n_sel, k, _i32(cols), _f32(scores)))
        return cols, scores

    def recommend_step_filtered(self, in_idx, item_idx=None, k=20, excl_offs=None, excl_items=None, excl_mask=None, oversample=None):
        """recommend_step without the excluded items (g4r_recommend_step_filtered): row r never receives a candidate whose item index
        is in excl_items[excl_offs[r]:excl_offs[r + 1]] (excl_offs: rows + 1 offsets) or has its bit set in excl_mask (uint32 words,
        bit i & 31 of word i >> 5).  None: no such exclusion.  Same return value as recommend_step.
        oversample (an integer >= 1): the two-stage selection instead (g4r_recommend_step_scan): a bf16 scan keeps k * oversample
        candidates per row, which are re-ranked by their exact fp32 scores."""
        ii = np.ascontiguousarray(in_idx, dtype=np.int32)
        it, n_sel = _cand(item_idx, self.cfg.n_items)
        xo, xi, mask = _excl(len(ii), excl_offs, excl_items, excl_mask, self.cfg.n_items, 'rows')
        cols, scores = _topk_out((len(ii), k))
        head = (self.h, _i32(ii), len(ii), _i32(it), n_sel, k)
        tail = (_i64(xo), _i32(xi), _u32(mask), _i32(cols), _f32(scores))
        if oversample is None:
            _chk(lib().g4r_recommend_step_filtered(*head, *tail))
        else:
            _chk(lib().g4r_recommend_step_scan(*head, int(oversample), *tail))
        return cols, scores

    def recommend_sessions(self, hist_offs, hist_items, item_idx=None, k=20, excl_offs=None, excl_items=None, excl_mask=None,
                           hidden=None, return_hidden=False, oversample=None):
        """Top-k after replaying whole session histories, without the prediction state (g4r_recommend_sessions): session i is
        hist_items[hist_offs[i]:hist_offs[i + 1]] (item indices), started from hidden (a list of float32[n, layers[l]], None = zeros).
        Exclusions as in recommend_step_filtered, one list per session.  Returns (cols, scores), + the list of hidden states after
        the last items with return_hidden=True.  oversample: as in recommend_step_filtered (g4r_recommend_sessions_scan)."""
        offs, hi, n = _hist(hist_offs, hist_items)
        it, n_sel = _cand(item_idx, self.cfg.n_items)
        xo, xi, mask = _excl(n, excl_offs, excl_items, excl_mask, self.cfg.n_items, 'n')
        h0, h0p = _hidden_in(hidden, n, self.layers)
        hout, houtp = _hidden_out(n, self.layers, return_hidden)
        cols, scores = _topk_out((n, k))
        head = (self.h, _i64(offs), _i32(hi), n, h0p, _i32(it), n_sel, k)
        tail = (_i64(xo), _i32(xi), _u32(mask), _i32(cols), _f32(scores), houtp)
        if oversample is None:
            _chk(lib().g4r_recommend_sessions(*head, *tail))
        else:
            _chk(lib().g4r_recommend_sessions_scan(*head, int(oversample), *tail))
        return (cols, scores, hout) if return_hidden else (cols, scores)

    # -- session store (slot-level; the id map lives in gru4rec_amd/session_store.py)
    def store_open(self, capacity, seen_cap):
        _chk(lib().g4r_store_open(self.h, int(capacity), int(seen_cap)))

    def store_close(self):
        _chk(lib().g4r_store_close(self.h))

    def store_info(self):
        """(capacity, seen_cap, bytes the slots hold) of the open session store; zeros without one."""
        a = self.get_debug('session_store', 3)
        return int(a[0]), int(a[1]), int(a[2])

    def store_push(self, ev_offs, ev_items, slots, fresh, item_idx=None, k=0, exclude_seen=False, excl_mask=None, oversample=None):
        """The events of n rows through the slots of the session store (g4r_store_push): row r is ev_items[ev_offs[r]:ev_offs[r + 1]]
        (item indices) of the session in slot slots[r], started from zero with an empty list where fresh[r].  k = 0: returns None;
        otherwise (cols int32[n, k], scores float32[n, k], overflow int32[n]) after every row's last event, the slot's seen list
        excluded with exclude_seen.  oversample: as in recommend_step_filtered."""
        offs, ev, n = _hist(ev_offs, ev_items)
        sl, fr = np.ascontiguousarray(slots, dtype=np.int32), np.ascontiguousarray(fresh, dtype=np.int32)
        if len(sl) != n or len(fr) != n:
            raise ValueError('slots and fresh must hold one entry per row (n)')
        it, n_sel = _cand(item_idx, self.cfg.n_items)
        mask = _mask(excl_mask, self.cfg.n_items)
        cols, scores = _topk_out((n, k))
        over = np.zeros(n, dtype=np.int32)
        _chk(lib().g4r_store_push(self.h, _i64(offs), _i32(ev), _i32(sl), _i32(fr), n, _i32(it), n_sel, int(k), int(oversample or 0),
                                  int(bool(exclude_seen)), _u32(mask), _i32(cols), _f32(scores), _i32(over)))
        return (cols, scores, over) if k else None

    def store_peek(self, slots, item_idx=None, k=20, exclude_seen=False, excl_mask=None, oversample=None):
        """store_push's selection from what the slots hold (g4r_store_peek): nothing is stepped or written."""
        sl = np.ascontiguousarray(slots, dtype=np.int32)
        it, n_sel = _cand(item_idx, self.cfg.n_items)
        mask = _mask(excl_mask, self.cfg.n_items)
        cols, scores = _topk_out((len(sl), k))
        over = np.zeros(len(sl), dtype=np.int32)
        _chk(lib().g4r_store_peek(self.h, _i32(sl), len(sl), _i32(it), n_sel, int(k), int(oversample or 0), int(bool(exclude_seen)), _u32(mask),
                                  _i32(cols), _f32(scores), _i32(over)))
        return cols, scores, over

    def store_read(self, slots, seen_cap):
        """The slots' rows (g4r_store_read): (hidden: float32[n, layers[l]] per layer, seen int32[n, seen_cap], len int32[n], flag int32[n])."""
        sl = np.ascontiguousarray(slots, dtype=np.int32)
        n = len(sl)
        hout, houtp = _hidden_out(n, self.layers, True)
        seen, ln, fl = np.zeros((n, seen_cap), dtype=np.int32), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
        _chk(lib().g4r_store_read(self.h, _i32(sl), n, houtp, _i32(seen), _i32(ln), _i32(fl)))
        return hout, seen, ln, fl

    def store_write(self, slots, hidden, seen, ln, flag):
        """The reverse of store_read (g4r_store_write); seen: int32[n, seen_cap], every row strictly ascending up to its length."""
        sl = np.ascontiguousarray(slots, dtype=np.int32)
        n = len(sl)
        h0, h0p = _hidden_in(hidden, n, self.layers)
        seen, ln, fl = (np.ascontiguousarray(a, dtype=np.int32) for a in (seen, ln, flag))
        if seen.ndim != 2 or seen.shape[0] != n or len(ln) != n or len(fl) != n:
            raise ValueError('seen must be [n, seen_cap], len and flag [n]')
        _chk(lib().g4r_store_write(self.h, _i32(sl), n, h0p, _i32(seen), _i32(ln), _i32(fl)))

    # -- item index (IVF)
    def ivf_assign(self, centroids):
        """The list of every item for float32 centroids [n_lists, layers[-1] + 1] (g4r_ivf_assign): int32[n_items]."""
        cen = np.ascontiguousarray(centroids, dtype=np.float32)
        if cen.ndim != 2 or cen.shape[1] != self.layers[-1] + 1:
            raise ValueError('centroids must be a [n_lists, %d] matrix' % (self.layers[-1] + 1))
        out = np.empty(self.cfg.n_items, dtype=np.int32)
        _chk(lib().g4r_ivf_assign(self.h, _f32(cen), cen.shape[0], _i32(out)))
        return out

    def ivf_set(self, centroids, list_offs, list_items):
        """Installs an item index and builds its device tables (g4r_ivf_set)."""
        cen = np.ascontiguousarray(centroids, dtype=np.float32)
        offs = np.ascontiguousarray(list_offs, dtype=np.int64)
        items = np.ascontiguousarray(list_items, dtype=np.int32)
        if cen.ndim != 2 or cen.shape[1] != self.layers[-1] + 1 or len(offs) != cen.shape[0] + 1 or len(items) != self.cfg.n_items:
            raise ValueError('an item index is centroids [n_lists, %d], list_offs [n_lists + 1] and list_items [n_items]' % (self.layers[-1] + 1))
        _chk(lib().g4r_ivf_set(self.h, _f32(cen), cen.shape[0], _i64(offs), _i32(items)))

    def ivf_release(self):
        _chk(lib().g4r_ivf_release(self.h))

    def ivf_info(self):
        """State of the item index: (lists, blocks of 32 positions, bytes its device tables hold, valid, builds so far)."""
        a = self.get_debug('ivf_index', 5)
        return int(a[0]), int(a[1]), int(a[2]), bool(a[3]), int(a[4])

    def recommend_sessions_ivf(self, hist_offs, hist_items, k=20, oversample=8, nprobe=1, excl_offs=None, excl_items=None, excl_mask=None,
                               hidden=None, return_hidden=False, return_probes=False):
        """recommend_sessions over the nprobe best lists of the item index (g4r_recommend_sessions_ivf): (items int32[n, k], scores
        float32[n, k], found int32[n]), + the hidden states with return_hidden=True, + the probed lists int32[n, nprobe] with
        return_probes=True.  Entries at and after found[i] hold item 0 and score NaN."""
        offs, hi, n = _hist(hist_offs, hist_items)
        xo, xi, mask = _excl(n, excl_offs, excl_items, excl_mask, self.cfg.n_items, 'n')
        h0, h0p = _hidden_in(hidden, n, self.layers)
        hout, houtp = _hidden_out(n, self.layers, return_hidden)
        cols, scores = _topk_out((n, k))
        found = np.empty(n, dtype=np.int32)
        probes = np.empty((n, max(int(nprobe), 1)), dtype=np.int32) if return_probes else None
        _chk(lib().g4r_recommend_sessions_ivf(self.h, _i64(offs), _i32(hi), n, h0p, k, int(oversample), int(nprobe), _i64(xo), _i32(xi), _u32(mask),
                                              _i32(cols), _f32(scores), _i32(found), houtp, _i32(probes)))
        return (cols, scores, found) + ((hout,) if return_hidden else ()) + ((probes,) if return_probes else ())

    def continue_sessions(self, hist_offs, hist_items, item_idx=None, k=1, steps=1, no_repeat=True, excl_offs=None, excl_items=None,
                          excl_mask=None, hidden=None, return_hidden=False, oversample=None):
        """`steps` selections per session, the best item of each fed back on the device as the session's next input
        (g4r_continue_sessions).  Arguments as in recommend_sessions; no_repeat adds every fed-back item to its session's exclusion
        list.  Returns (cols int32[n, steps, k], scores float32[n, steps, k]), + the hidden states that produced the last step's
        scores with return_hidden=True."""
        offs, hi, n = _hist(hist_offs, hist_items)
        steps = int(steps)
        if steps < 1:
            raise ValueError('steps must be at least 1')
        it, n_sel = _cand(item_idx, self.cfg.n_items)
        xo, xi, mask = _excl(n, excl_offs, excl_items, excl_mask, self.cfg.n_items, 'n')
        h0, h0p = _hidden_in(hidden, n, self.layers)
        hout, houtp = _hidden_out(n, self.layers, return_hidden)
        cols, scores = _topk_out((n, steps, k))
        _chk(lib().g4r_continue_sessions(self.h, _i64(offs), _i32(hi), n, h0p, _i32(it), n_sel, k, 0 if oversample is None else int(oversample),
                                         steps, 1 if no_repeat else 0, _i64(xo), _i32(xi), _u32(mask), _i32(cols), _f32(scores), houtp))
        return (cols, scores, hout) if return_hidden else (cols, scores)

    def beam_sessions(self, hist_offs, hist_items, item_idx=None, beams=4, steps=1, no_repeat=True, combine='sum', excl_offs=None,
                      excl_items=None, excl_mask=None, hidden=None, oversample=None):
        """Beam search over the continuations of whole sessions (g4r_beam_sessions).  Arguments as in continue_sessions, with
        k = beams, and combine ('sum' / 'product').  Returns the raw back-pointer records (parent int32[n, steps, beams], cols
        int32[n, steps, beams], step_scores float32[n, steps, beams]) and (path_scores float32[n, beams], scale_exp int32[n]) after
        the last step; beam_backtrack turns the records into paths."""
        offs, hi, n = _hist(hist_offs, hist_items)
        steps, beams = int(steps), int(beams)
        if steps < 1:
            raise ValueError('steps must be at least 1')
        if not 1 <= beams <= G4R_BEAM_MAX:
            raise ValueError('beams must be in [1, %d]' % G4R_BEAM_MAX)
        it, n_sel = _cand(item_idx, self.cfg.n_items)
        xo, xi, mask = _excl(n, excl_offs, excl_items, excl_mask, self.cfg.n_items, 'n')
        h0, h0p = _hidden_in(hidden, n, self.layers)
        parent = np.empty((n, steps, beams), dtype=np.int32)
        cols, step_scores = _topk_out((n, steps, beams))
        path_scores = np.empty((n, beams), dtype=np.float32)
        scale_exp = np.empty(n, dtype=np.int32)
        _chk(lib().g4r_beam_sessions(self.h, _i64(offs), _i32(hi), n, h0p, _i32(it), n_sel, beams, 0 if oversample is None else int(oversample),
                                     steps, 1 if no_repeat else 0, BEAM_COMBINE[combine], _i64(xo), _i32(xi), _u32(mask), _i32(parent),
                                     _i32(cols), _f32(step_scores), _f32(path_scores), _i32(scale_exp)))
        return parent, cols, step_scores, path_scores, scale_exp

    def sample_sessions(self, hist_offs, hist_items, item_idx=None, steps=1, samples=1, top_k=None, temperature=1.0, seed=0, first_step=0,
                        no_repeat=True, excl_offs=None, excl_items=None, excl_mask=None, hidden=None, return_hidden=False, top_p=None,
                        return_logprobs=False):
        """`samples` independent draws per session of `steps` items each from softmax(logit / temperature) over the eligible
        candidates (top_k: cut to the top_k best first), every drawn item fed back on the device (g4r_sample_sessions).  Arguments as
        in continue_sessions; draw (i, j) uses the noise of row id i * samples + j at steps first_step, first_step + 1, ...  Returns
        (cols int32[n, samples, steps], scores float32[n, samples, steps] -- the chosen positions' logits), + the hidden states that
        produced the last step's scores (float32[n * samples, layers[l]] each) with return_hidden=True.  top_p (a float in (0, 1],
        with top_k) and return_logprobs (+ logprobs float32[n, samples, steps], the last element) go through g4r_sample_sessions_lp;
        without either the call is g4r_sample_sessions'."""
        offs, hi, n = _hist(hist_offs, hist_items)
        steps, samples = int(steps), int(samples)
        if steps < 1:
            raise ValueError('steps must be at least 1')
        if not 1 <= samples <= G4R_SAMPLE_MAX:
            raise ValueError('samples must be in [1, %d]' % G4R_SAMPLE_MAX)
        it, n_sel = _cand(item_idx, self.cfg.n_items)
        xo, xi, mask = _excl(n, excl_offs, excl_items, excl_mask, self.cfg.n_items, 'n')
        h0, h0p = _hidden_in(hidden, n, self.layers)
        hout, houtp = _hidden_out(n * samples, self.layers, return_hidden)
        cols, scores = _topk_out((n, samples, steps))
        args = (self.h, _i64(offs), _i32(hi), n, h0p, _i32(it), n_sel, steps, 1 if no_repeat else 0, _i64(xo), _i32(xi), _u32(mask), samples,
                0 if top_k is None else int(top_k), float(temperature), int(seed), int(first_step), _i32(cols), _f32(scores), houtp)
        logprobs = np.empty((n, samples, steps), dtype=np.float32) if return_logprobs else None
        if top_p is None and not return_logprobs:
            _chk(lib().g4r_sample_sessions(*args))
        else:
            _chk(lib().g4r_sample_sessions_lp(*args, 0.0 if top_p is None else float(top_p), _f32(logprobs)))
        out = (cols, scores) + ((hout,) if return_hidden else ()) + ((logprobs,) if return_logprobs else ())
        return out

    def session_log_partition(self, hist_offs, hist_items, item_idx=None, temperature=1.0, excl_offs=None, excl_items=None, excl_mask=None,
                              hidden=None):
        """The row normaliser after replaying whole session histories (g4r_session_log_partition; arguments as in recommend_sessions):
        (zeta float32[n], Q uint64[n]) -- every session's largest eligible logit and the exact integer sum of
        rn(2^39 * expf(fl32(fl32(z - zeta) / temperature))) over its eligible candidate positions."""
        offs, hi, n = _hist(hist_offs, hist_items)
        it, n_sel = _cand(item_idx, self.cfg.n_items)
        xo, xi, mask = _excl(n, excl_offs, excl_items, excl_mask, self.cfg.n_items, 'n')
        h0, h0p = _hidden_in(hidden, n, self.layers)
        zeta = np.empty(n, dtype=np.float32)
        Q = np.empty(n, dtype=np.uint64)
        _chk(lib().g4r_session_log_partition(self.h, _i64(offs), _i32(hi), n, h0p, _i32(it), n_sel, _i64(xo), _i32(xi), _u32(mask),
                                             float(temperature), _f32(zeta), _u64(Q)))
        return zeta, Q

    def audience_sessions(self, hist_offs, hist_items, items, k, by='logprob', temperature=1.0, exclude_history=False, hidden=None):
        """For each of the M item indices `items` the k sessions with the largest value, after replaying whole session histories
        (g4r_audience_sessions; histories and hidden as in recommend_sessions): (sessions int32[M, k] -- indices into the histories,
        -1 behind a row's count --, values float32[M, k] -- NaN there --, counts int32[M]).  by: 'score' / 'logprob'."""
        offs, hi, n = _hist(hist_offs, hist_items)
        it = np.ascontiguousarray(items, dtype=np.int32).ravel()
        M, k = len(it), int(k)
        if not 1 <= M <= G4R_AUDIENCE_ITEMS_MAX:
            raise ValueError('the number of items must be in [1, %d]' % G4R_AUDIENCE_ITEMS_MAX)
        if not 1 <= k <= G4R_AUDIENCE_MAX or M * k > G4R_AUDIENCE_ENTRIES_MAX:
            raise ValueError('k must be in [1, %d] and items x k at most %d' % (G4R_AUDIENCE_MAX, G4R_AUDIENCE_ENTRIES_MAX))
        h0, h0p = _hidden_in(hidden, n, self.layers)
        sessions, values = _topk_out((M, k))
        counts = np.empty(M, dtype=np.int32)
        _chk(lib().g4r_audience_sessions(self.h, _i64(offs), _i32(hi), n, h0p, _i32(it), M, k, AUDIENCE_BY[by], float(temperature),
                                         1 if exclude_history else 0, _i32(sessions), _f32(values), _i32(counts)))
        return sessions, values, counts

    def debug_lse_terms(self, z, zeta, inv_t):
        """The terms of the row normaliser for the logits z relative to zeta (an array like z, or one value) at the float32 reciprocal
        temperature inv_t, from the device function the scan calls (g4r_debug_lse_terms): uint64[len(z)]."""
        z = np.ascontiguousarray(z, dtype=np.float32).ravel()
        zeta = np.ascontiguousarray(np.broadcast_to(np.asarray(zeta, dtype=np.float32), z.shape))
        out = np.empty(len(z), dtype=np.uint64)
        _chk(lib().g4r_debug_lse_terms(self.h, _f32(z), _f32(zeta), len(z), float(np.float32(inv_t)), _u64(out)))
        return out

    def debug_gumbel(self, seed, row_id, step, items):
        """The noise of sample_sessions for (seed, row id, step) and every item index of `items`, from the device function the
        selection calls (g4r_debug_gumbel): float32[len(items)]."""
        it = np.ascontiguousarray(items, dtype=np.int32)
        out = np.empty(len(it), dtype=np.float32)
        _chk(lib().g4r_debug_gumbel(self.h, int(seed), int(row_id), int(step), _i32(it), len(it), _f32(out)))
        return out

    def similar_items(self, q_idx, item_idx=None, k=20, metric='cosine', space='output', exclude_self=True, excl_mask=None):
        """The k candidates most similar to every query item in the model's own embedding space (g4r_similar_items; stateless):
        (cols int32[n, k], scores float32[n, k]); cols are positions in item_idx (item indices without it).  excl_mask as in
        recommend_step_filtered."""
        qi = np.ascontiguousarray(q_idx, dtype=np.int32)
        it, n_sel = _cand(item_idx, self.cfg.n_items)
        mask = _mask(excl_mask, self.cfg.n_items)
        cols, scores = _topk_out((len(qi), k))
        _chk(lib().g4r_similar_items(self.h, SIM_SPACES[space], SIM_METRICS[metric], _i32(qi), len(qi), _i32(it), n_sel, k,
                                     1 if exclude_self else 0, _u32(mask), _i32(cols), _f32(scores)))
        return cols, scores

    def diversify_lists(self, items, rel, k, lam=0.7, metric='cosine', space='output', normalize=True):
        """k of every row's P candidates picked by maximal marginal relevance (g4r_diversify_lists; stateless): items int32[n, P]
        (item indices), rel float32[n, P] -> (pos int32[n, k] positions in the row's list, values float32[n, k]), pick by pick."""
        it = np.ascontiguousarray(items, dtype=np.int32)
        rl = np.ascontiguousarray(rel, dtype=np.float32)
        if it.ndim != 2 or it.shape != rl.shape:
            raise ValueError('items and rel must be two arrays of one shape [n, P]')
        n, P = it.shape
        pos, values = _topk_out((n, k))
        _chk(lib().g4r_diversify_lists(self.h, SIM_SPACES[space], SIM_METRICS[metric], _i32(it), _f32(rl), n, P, k, float(lam),
                                       1 if normalize else 0, _i32(pos), _f32(values)))
        return pos, values

    def diversify_sessions(self, hist_offs, hist_items, item_idx=None, k=20, pool=100, lam=0.7, metric='cosine', space='output',
                           normalize=True, excl_offs=None, excl_items=None, excl_mask=None, hidden=None, return_hidden=False,
                           oversample=None):
        """recommend_sessions with k = pool followed on the device by diversify_lists over every session's pool
        (g4r_diversify_sessions): (cols int32[n, k], scores float32[n, k], pos int32[n, k], values float32[n, k]) in pick order, + the
        hidden states with return_hidden=True.  The other arguments as in recommend_sessions."""
        offs, hi, n = _hist(hist_offs, hist_items)
        it, n_sel = _cand(item_idx, self.cfg.n_items)
        xo, xi, mask = _excl(n, excl_offs, excl_items, excl_mask, self.cfg.n_items, 'n')
        h0, h0p = _hidden_in(hidden, n, self.layers)
        hout, houtp = _hidden_out(n, self.layers, return_hidden)
        cols, scores = _topk_out((n, k))
        pos, values = _topk_out((n, k))
        _chk(lib().g4r_diversify_sessions(self.h, _i64(offs), _i32(hi), n, h0p, _i32(it), n_sel, k, pool, 0 if oversample is None else int(oversample),
                                          _i64(xo), _i32(xi), _u32(mask), SIM_SPACES[space], SIM_METRICS[metric], float(lam),
                                          1 if normalize else 0, _i32(cols), _f32(scores), _i32(pos), _f32(values), houtp))
        return (cols, scores, pos, values, hout) if return_hidden else (cols, scores, pos, values)

    # -- item groups and per-group caps
    def set_item_groups(self, groups):
        """The model's group table (g4r_set_item_groups): int32[n_items], -1 = ungrouped; None clears it."""
        if groups is None:
            _chk(lib().g4r_set_item_groups(self.h, None, 0))
            return
        g = np.ascontiguousarray(groups, dtype=np.int32)
        _chk(lib().g4r_set_item_groups(self.h, _i32(g), g.size))

    def get_item_groups(self):
        out = np.empty(self.cfg.n_items, dtype=np.int32)
        _chk(lib().g4r_get_item_groups(self.h, _i32(out), out.size))
        return out

    @staticmethod
    def _priors(n, prior_offs, prior_groups):
        """The prior lists of n rows: (offsets int64[n + 1] or None, group indices int32 -- empty without lists, never None)."""
        offs = _arr(prior_offs, np.int64)
        groups = np.ascontiguousarray(np.zeros(0) if prior_groups is None else prior_groups, dtype=np.int32)
        if offs is not None and (len(offs) != n + 1 or offs[-1] > len(groups) or offs[0] < 0):
            raise ValueError('prior_offs must hold n + 1 offsets into prior_groups')
        return offs, groups

    def recommend_sessions_capped(self, hist_offs, hist_items, item_idx=None, k=20, pool=100, cap=1, excl_offs=None, excl_items=None,
                                  excl_mask=None, hidden=None, return_hidden=False, oversample=None):
        """recommend_sessions with k = pool followed on the device by the cap rule over every session's pool
        (g4r_recommend_sessions_capped): (cols int32[n, k], scores float32[n, k], pos int32[n, k], kept int32[n]), + the hidden states
        with return_hidden=True.  Entries at and after kept[i] are pads (-1, NaN, -1).  The other arguments as in recommend_sessions."""
        offs, hi, n = _hist(hist_offs, hist_items)
        it, n_sel = _cand(item_idx, self.cfg.n_items)
        xo, xi, mask = _excl(n, excl_offs, excl_items, excl_mask, self.cfg.n_items, 'n')
        h0, h0p = _hidden_in(hidden, n, self.layers)
        hout, houtp = _hidden_out(n, self.layers, return_hidden)
        cols, scores = _topk_out((n, k))
        pos, kept = np.empty((n, k), dtype=np.int32), np.empty(n, dtype=np.int32)
        _chk(lib().g4r_recommend_sessions_capped(self.h, _i64(offs), _i32(hi), n, h0p, _i32(it), n_sel, k, pool,
                                                 0 if oversample is None else int(oversample), _i64(xo), _i32(xi), _u32(mask), int(cap),
                                                 _i32(cols), _f32(scores), _i32(pos), _i32(kept), houtp))
        return (cols, scores, pos, kept, hout) if return_hidden else (cols, scores, pos, kept)

    def continue_sessions_capped(self, hist_offs, hist_items, item_idx=None, k=1, pool=100, cap=1, steps=1, no_repeat=True, excl_offs=None,
                                 excl_items=None, excl_mask=None, prior_offs=None, prior_groups=None, hidden=None, return_hidden=False,
                                 oversample=None):
        """continue_sessions with the cap rule between every step's selection of `pool` and its feedback
        (g4r_continue_sessions_capped): (cols int32[n, steps, k], scores float32[n, steps, k], kept int32[n, steps]), + the hidden
        states with return_hidden=True.  prior_offs / prior_groups: every session's prior group indices (CSR)."""
        offs, hi, n = _hist(hist_offs, hist_items)
        steps = int(steps)
        if steps < 1:
            raise ValueError('steps must be at least 1')
        it, n_sel = _cand(item_idx, self.cfg.n_items)
        xo, xi, mask = _excl(n, excl_offs, excl_items, excl_mask, self.cfg.n_items, 'n')
        po, pg = self._priors(n, prior_offs, prior_groups)
        h0, h0p = _hidden_in(hidden, n, self.layers)
        hout, houtp = _hidden_out(n, self.layers, return_hidden)
        cols, scores = _topk_out((n, steps, k))
        kept = np.empty((n, steps), dtype=np.int32)
        _chk(lib().g4r_continue_sessions_capped(self.h, _i64(offs), _i32(hi), n, h0p, _i32(it), n_sel, k, pool,
                                                0 if oversample is None else int(oversample), steps, 1 if no_repeat else 0, _i64(xo), _i32(xi),
                                                _u32(mask), int(cap), _i64(po), _i32(pg), _i32(cols), _f32(scores), _i32(kept), houtp))
        return (cols, scores, kept, hout) if return_hidden else (cols, scores, kept)

    def cap_lists(self, items, k, cap, prior_offs=None, prior_groups=None):
        """The cap rule over supplied lists (g4r_cap_lists; stateless): items int32[n, P] (item indices) -> (pos int32[n, k] kept
        positions in list order, then -1; kept int32[n])."""
        it = np.ascontiguousarray(items, dtype=np.int32)
        if it.ndim != 2:
            raise ValueError('items must be an array of shape [n, P]')
        n, P = it.shape
        po, pg = self._priors(n, prior_offs, prior_groups)
        pos, kept = np.empty((n, k), dtype=np.int32), np.empty(n, dtype=np.int32)
        _chk(lib().g4r_cap_lists(self.h, _i32(it), n, P, k, int(cap), _i64(po), _i32(pg), _i32(pos), _i32(kept)))
        return pos, kept

    def sim_norms(self):
        """State of the inverse-norm cache of similar_items: (bytes held, valid, builds so far)."""
        a = self.get_debug('sim_norms', 3)
        return int(a[0]), bool(a[1]), int(a[2])

    @staticmethod
    def _cand_csr(cand_offs, cand_items, rows):
        offs = np.ascontiguousarray(cand_offs, dtype=np.int64)
        items = np.ascontiguousarray(cand_items, dtype=np.int32)
        if len(offs) != rows + 1 or offs[0] < 0 or offs[-1] > len(items):
            raise ValueError('cand_offs must hold rows + 1 = %d offsets into cand_items' % (rows + 1))
        return offs, items

    @staticmethod
    def _cand_out(offs, k):
        n = len(offs) - 1
        if k == 0:
            return np.empty(int(offs[-1] - offs[0]), dtype=np.float32), None
        return np.empty((n, k), dtype=np.float32), np.empty((n, k), dtype=np.int32)

    def score_candidates(self, in_idx, cand_offs, cand_items, k=0):
        """Scores of per-row candidate lists (g4r_score_candidates; the hidden state advances as in predict_step): row r's list is
        cand_items[cand_offs[r]:cand_offs[r + 1]] (item indices).  k = 0: float32 scores in CSR order; k > 0: (pos int32[rows, k],
        scores float32[rows, k]), pos the positions in the row's list."""
        ii = np.ascontiguousarray(in_idx, dtype=np.int32)
        offs, items = self._cand_csr(cand_offs, cand_items, len(ii))
        scores, pos = self._cand_out(offs, k)
        _chk(lib().g4r_score_candidates(self.h, _i32(ii), len(ii), _i64(offs), _i32(items), k, _f32(scores), _i32(pos)))
        return scores if k == 0 else (pos, scores)

    def score_candidates_sessions(self, hist_offs, hist_items, cand_offs, cand_items, k=0, hidden=None, return_hidden=False):
        """score_candidates after replaying whole session histories, without the prediction state (g4r_score_candidates_sessions):
        histories and hidden as in recommend_sessions, one candidate list per session.  Returns what score_candidates returns,
        + the list of hidden states after the last items with return_hidden=True."""
        ho, hi, n = _hist(hist_offs, hist_items)
        offs, items = self._cand_csr(cand_offs, cand_items, n)
        h0, h0p = _hidden_in(hidden, n, self.layers)
        hout, houtp = _hidden_out(n, self.layers, return_hidden)
        scores, pos = self._cand_out(offs, k)
        _chk(lib().g4r_score_candidates_sessions(self.h, _i64(ho), _i32(hi), n, h0p, _i64(offs), _i32(items), k, _f32(scores), _i32(pos),
                                                 houtp))
        out = scores if k == 0 else (pos, scores)
        return (out, hout) if return_hidden else out

    def rank_targets(self, target_col, col_begin=0, mode='standard'):
        t = np.ascontiguousarray(target_col, dtype=np.int32)
        r = np.empty(len(t), dtype=np.float32)
        _chk(lib().g4r_rank_targets(self.h, _i32(t), len(t), col_begin, RANK_MODES[mode], _f32(r)))
        return r

    # -- multi-GPU
    def evaluate(self, plan, batch, items, cutoffs, mode):
        """Whole evaluation in one call (g4r_evaluate).  Returns (recall_sum[n_cut], mrr_sum[n_cut], n_events)."""
        cuts = np.ascontiguousarray(cutoffs, dtype=np.int32)
        rec = np.zeros(len(cuts), dtype=np.float64)
        mrr = np.zeros(len(cuts), dtype=np.float64)
        n = C.c_int64(0)
        it = _arr(items, np.int32)
        in_idx, out_idx, reset, M, cs, cm, nc = _plan(plan, batch)
        _chk(lib().g4r_evaluate(self.h, _i32(in_idx), _i32(out_idx), _u8(reset), _i32(M), int(plan['T']), batch, _i64(cs), _i32(cm), nc,
                                _i32(it), 0 if it is None else len(it), _i32(cuts), len(cuts), RANK_MODES[mode], _f64(rec), _f64(mrr),
                                C.byref(n)))
        return rec, mrr, int(n.value)

    def recommend_events(self, plan, batch, items, mode, slot, n_slots, k, excl_mask=None, seen=None, want_lists=True):
        """Top-k list, target rank and target score of every event of an evaluation plan in one call (g4r_recommend_events).
        slot: int64[T, batch], the output row of the event at (step, row), -1 for padding.  seen: None or the dict of
        evaluation.seen_tables plus 'sess' / 'pos' int32[T, batch].  Returns (items int32[n_slots, k], scores float32[n_slots, k],
        rank float32[n_slots], target_score float32[n_slots]); items / scores are None with want_lists=False."""
        T = int(plan['T'])
        it = _arr(items, np.int32)
        in_idx, out_idx, reset, M, cs, cm, nc = _plan(plan, batch)
        sl = np.ascontiguousarray(slot, dtype=np.int64)
        if sl.size != T * batch:
            raise ValueError('slot must hold T * batch = %d entries' % (T * batch))
        mask = _mask(excl_mask, self.cfg.n_items)
        st, _keep = self._seen_args(seen, T, batch)
        oi, os_ = _topk_out((n_slots, k)) if want_lists else (None, None)
        rk = np.empty(n_slots, dtype=np.float32)
        ts = np.empty(n_slots, dtype=np.float32)
        _chk(lib().g4r_recommend_events(self.h, _i32(in_idx), _i32(out_idx), _u8(reset), _i32(M), T, batch, _i64(cs), _i32(cm), nc,
                                        _i32(it), 0 if it is None else len(it), RANK_MODES[mode], _i64(sl), n_slots, k, _u32(mask), *st,
                                        _i32(oi), _f32(os_), _f32(rk), _f32(ts)))
        return oi, os_, rk, ts

    @staticmethod
    def _seen_args(seen, T, batch):
        """The six seen-table arguments of g4r_recommend_events / g4r_loglik_events (and the arrays they point into)."""
        if seen is None:
            return (None, None, None, 0, None, None), ()
        so, si, sf, ss, sp = (np.ascontiguousarray(seen[key], dtype=t) for key, t in (
            ('offs', np.int64), ('items', np.int32), ('first', np.int32), ('sess', np.int32), ('pos', np.int32)))
        if ss.size != T * batch or sp.size != T * batch or len(si) != len(sf) or so[-1] > len(si):
            raise ValueError('seen tables: sess / pos must hold T * batch entries, items / first one entry per offset')
        return (_i64(so), _i32(si), _i32(sf), len(so) - 1, _i32(ss), _i32(sp)), (so, si, sf, ss, sp)

    def loglik_events(self, plan, batch, items, slot, n_slots, temperature=1.0, excl_mask=None, seen=None):
        """Target logit, zeta, the integer normaliser Q and the target's eligibility of every event of an evaluation plan in one call
        (g4r_loglik_events; plan, items, slot, excl_mask and seen as in recommend_events).  Returns (z float32[n_slots], zeta
        float32[n_slots], Q uint64[n_slots], eligible bool[n_slots])."""
        T = int(plan['T'])
        it = _arr(items, np.int32)
        in_idx, out_idx, reset, M, cs, cm, nc = _plan(plan, batch)
        sl = np.ascontiguousarray(slot, dtype=np.int64)
        if sl.size != T * batch:
            raise ValueError('slot must hold T * batch = %d entries' % (T * batch))
        mask = _mask(excl_mask, self.cfg.n_items)
        st, _keep = self._seen_args(seen, T, batch)
        z = np.zeros(n_slots, dtype=np.float32)
        zeta = np.zeros(n_slots, dtype=np.float32)
        Q = np.zeros(n_slots, dtype=np.uint64)
        el = np.zeros(n_slots, dtype=np.uint8)
        _chk(lib().g4r_loglik_events(self.h, _i32(in_idx), _i32(out_idx), _u8(reset), _i32(M), T, batch, _i64(cs), _i32(cm), nc,
                                     _i32(it), 0 if it is None else len(it), _i64(sl), n_slots, _u32(mask), *st,
                                     float(np.float32(temperature)), _f32(z), _f32(zeta), _u64(Q), _u8(el)))
        return z, zeta, Q, el.astype(bool)

    def events_launches(self):
        """(steps, launches that scan the candidate columns, all launches, pieces) of the last recommend_events / loglik_events call."""
        return tuple(int(x) for x in self.get_debug('events_launches', 4))

    def comm_init(self, unique_id, nranks, rank):
        _chk(lib().g4r_comm_init(self.h, unique_id, nranks, rank))

    def comm_sync_sparse(self):
        _chk(lib().g4r_comm_sync_sparse(self.h))

    def p2p_enable(self):
        """The step's dense-gradient all-reduce through peer memory instead of RCCL (g4r_p2p_enable; collective)."""
        _chk(lib().g4r_p2p_enable(self.h))

    def p2p_export(self):
        """This rank's 64-byte IPC handle of its exchange region (g4r_p2p_export)."""
        buf = C.create_string_buffer(64)
        _chk(lib().g4r_p2p_export(self.h, buf))
        return buf.raw

    def p2p_attach(self, handles, nranks, rank):
        """handles: the ranks' 64-byte handles in rank order (g4r_p2p_attach)."""
        blob = b''.join(handles)
        if len(blob) != 64 * nranks:
            raise ValueError('p2p_attach: %d handles of 64 bytes expected' % nranks)
        _chk(lib().g4r_p2p_attach(self.h, blob, nranks, rank))

    def p2p_active(self):
        return bool(lib().g4r_p2p_active(self.h))

    def sync_enable(self):
        _chk(lib().g4r_sync_enable(self.h))

    def set_sync_every(self, k):
        """True when g4r_train_steps reconciles the item tables itself every k steps (small tables, g4r_set_sync_every); False when
        the caller has to call comm_sync_sparse."""
        rc = lib().g4r_set_sync_every(self.h, int(k))
        if rc < 0:
            raise NativeError(lib().g4r_last_error().decode())
        return rc == 1

    def sync_set_rule(self, param_rule, stat_rule):
        """'sum' / 'mean' for the parameter planes and for the optimizer-statistic planes of the reconciliation (g4r_sync_set_rule)."""
        r = {'sum': 0, 'mean': 1}
        _chk(lib().g4r_sync_set_rule(self.h, r[param_rule], r[stat_rule]))

    def sync_export(self, group=0):
        """(sorted ids int32[n], delta rows float32[n * row_floats] plane after plane) of the rows touched since the last sync."""
        n = int(lib().g4r_sync_export(self.h, group, None, None, 0))
        if n < 0:
            raise NativeError(lib().g4r_last_error().decode())
        w = int(lib().g4r_sync_row_floats(self.h, group))
        ids = np.empty(n, dtype=np.int32)
        rows = np.empty(n * w, dtype=np.float32)
        if lib().g4r_sync_export(self.h, group, _i32(ids), _f32(rows), n) != n:
            raise NativeError(lib().g4r_last_error().decode())
        return ids, rows

    def sync_import(self, parts, group=0):
        """parts: [(ids, rows)] of ALL ranks in rank order."""
        n = len(parts)
        counts = np.array([len(p[0]) for p in parts], dtype=np.int64)
        ids = [np.ascontiguousarray(p[0], dtype=np.int32) for p in parts]
        rows = [np.ascontiguousarray(p[1], dtype=np.float32) for p in parts]
        pi = (i32p * n)(*[_i32(a) for a in ids])
        pr = (f32p * n)(*[_f32(a) for a in rows])
        _chk(lib().g4r_sync_import(self.h, group, n, _i64(counts), pi, pr))

    def comm_min(self, value):
        v = C.c_int64(int(value))
        _chk(lib().g4r_comm_min_i64(self.h, C.byref(v)))
        return int(v.value)

    def comm_max(self, value):
        v = C.c_int64(int(value))
        _chk(lib().g4r_comm_max_i64(self.h, C.byref(v)))
        return int(v.value)

    def comm_nranks(self):
        n = int(lib().g4r_comm_nranks(self.h))
        if n < 0:
            raise NativeError(lib().g4r_last_error().decode())
        return n


def virtual_train_steps(models, t0, n):
    """Plan steps [t0, t0 + n) of `models` (handle q = rank q of len(models) ranks on one device) in lock-step, the dense gradients
    summed in process where the real run all-reduces them (g4r_virtual_train_steps)."""
    hs = (C.c_void_p * len(models))(*[m.h for m in models])
    _chk(lib().g4r_virtual_train_steps(hs, len(models), int(t0), int(n)))


def virtual_sync_dense(models):
    """Dense reconciliation of the item tables of `models` (handle q = rank q), the all-reduce taken in process (g4r_virtual_sync_dense)."""
    hs = (C.c_void_p * len(models))(*[m.h for m in models])
    _chk(lib().g4r_virtual_sync_dense(hs, len(models)))


def comm_unique_id():
    buf = C.create_string_buffer(128)
    _chk(lib().g4r_comm_unique_id(buf))
    return buf.raw


def bench_rows(n_items, width, rows_per_launch, launches=200, mode=1, device=0, seed=1):
    """(mean kernel us, wall us per launch) of the row gather / scatter micro-benchmark (g4r_bench_rows)."""
    k, w = C.c_double(), C.c_double()
    _chk(lib().g4r_bench_rows(device, int(n_items), int(width), int(rows_per_launch), int(launches), int(mode), int(seed), C.byref(k), C.byref(w)))
    return k.value, w.value


def selftest_mfma():
    e = C.c_float()
    _chk(lib().g4r_selftest_mfma(C.byref(e)))
    return e.value


class MemoryStress:
    """HBM / Infinity-Cache load on a stream of its own while the `with` body runs (g4r_stress_start / g4r_stress_stop)."""

    def __init__(self, mbytes=4096, launches=400, device=0):
        self.args = (int(device), int(mbytes), int(launches))
        self.h = None

    def __enter__(self):
        h = C.c_void_p()
        _chk(lib().g4r_stress_start(self.args[0], self.args[1], self.args[2], C.byref(h)))
        self.h = h
        return self

    def __exit__(self, *exc):
        if self.h is not None:
            _chk(lib().g4r_stress_stop(self.h))
            self.h = None
        return False

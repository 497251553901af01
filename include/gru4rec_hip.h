/*
 * gru4rec_hip.h -- C ABI of libgru4rec_hip.so: the MI355X (gfx950) implementation of GRU4Rec's
 * session-parallel mini-batch training / prediction hot path.
 *
 * This is the drop-in boundary.  The reference (hidasib/GRU4Rec) has no FFI of its own: its
 * device code is reached through compiled Theano functions.  Each entry point below replaces one
 * such Theano-function boundary (cited per function as reference file:line).  The Python host
 * (`gru4rec_amd/gru4rec.py`, mirroring the reference's `GRU4Rec` class) binds these with ctypes;
 * INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions
 *   - every call returns 0 on success, <0 on error; g4r_last_error() returns the message
 *   - plain pointers + sizes only; the caller owns every host buffer, the library owns device memory
 *   - a model handle is not thread-safe; one HIP stream per handle; calls are synchronous at return
 *     unless stated otherwise
 *   - all matrices are row-major fp32; layer sizes / embedding size must be multiples of 4
 */
#ifndef GRU4REC_HIP_H
#define GRU4REC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define G4R_MAX_LAYERS 8

/* gru4rec.py:136-143 (set_loss_function) */
enum { G4R_LOSS_XE = 0, G4R_LOSS_BPR_MAX = 1, G4R_LOSS_TOP1_MAX = 2, G4R_LOSS_BPR = 3, G4R_LOSS_TOP1 = 4,
       G4R_LOSS_XE_LOGIT = 5 };
/* gru4rec.py:144-161 (set_final_activation / set_hidden_activation) */
enum { G4R_ACT_LINEAR = 0, G4R_ACT_RELU = 1, G4R_ACT_TANH = 2, G4R_ACT_LEAKY = 3, G4R_ACT_ELU = 4,
       G4R_ACT_SELU = 5, G4R_ACT_SOFTMAX = 6, G4R_ACT_SOFTMAX_LOGIT = 7 /* final activation only; plain softmax when
       predicting, gru4rec.py:490-491,499-500 */ };
/* gru4rec.py:438-470: where the GRU input comes from */
enum { G4R_EMBED_CONSTRAINED = 0 /* Wy shared, :438-448 */, G4R_EMBED_SEPARATE = 1 /* E, :449-456 */,
       G4R_EMBED_ONEHOT = 2 /* no embedding, layer 0 reads rows of Wx[0] (I x 3D), :457-470; the constructor default */ };
/* gru4rec.py:392-399,411-418: learning-rate adaptation (`adapt`); NONE = plain SGD */
enum { G4R_ADAPT_ADAGRAD = 0, G4R_ADAPT_RMSPROP = 1, G4R_ADAPT_ADADELTA = 2, G4R_ADAPT_ADAM = 3, G4R_ADAPT_NONE = 4 };
/* evaluation.py:62-65 */
enum { G4R_RANK_STANDARD = 0, G4R_RANK_CONSERVATIVE = 1, G4R_RANK_MEDIAN = 2,
       G4R_RANK_TIEBREAKING = 3 /* :55: scores + uniform * 1e-10 in fp32 (Philox stream keyed by the model seed, the evaluation step,
       row and candidate column instead of the reference's MRG stream), then ranked as STANDARD */ };

/* Constructor arguments of the reference's GRU4Rec (gru4rec.py:97-135) that the hot path needs. */
typedef struct g4r_config {
    int32_t n_items;
    int32_t n_layers;
    int32_t layers[G4R_MAX_LAYERS];
    int32_t batch_size;
    int32_t n_sample;            /* additional negatives per step (0 = in-batch only) */
    int32_t loss;                /* G4R_LOSS_* */
    int32_t final_act;           /* G4R_ACT_* */
    float   final_act_p0, final_act_p1;
    int32_t hidden_act;          /* G4R_ACT_* (not softmax) */
    float   hidden_act_p0, hidden_act_p1;
    int32_t embed_mode;          /* G4R_EMBED_* */
    int32_t embedding;           /* width of E when embed_mode == SEPARATE */
    float   learning_rate, momentum, lmbd, bpreg, logq, sample_alpha;
    float   dropout_p_hidden, dropout_p_embed;
    int64_t sample_store;        /* ints in the negative-sample store (gru4rec.py:515,547) */
    uint64_t seed;               /* Philox key for sampler + dropout */
    int32_t device;              /* HIP device ordinal */
    int32_t rank, nranks;        /* data-parallel rank layout (1 process per GPU) */
    int32_t use_graph;           /* capture steady-state steps into a hipGraph */
    float   smoothing;           /* label smoothing of cross-entropy / xe_logit, gru4rec.py:226-235 */
    int32_t adapt;               /* G4R_ADAPT_* */
    float   adapt_p0, adapt_p1;  /* adapt_params (rmsprop / adadelta: decay; adam: beta1, beta2), gru4rec.py:301-304,342,368 */
    float   grad_cap;            /* global gradient-norm clip, 0 = off, gru4rec.py:386-389 */
    int32_t sparse_exact;        /* N > 1 only.  0: item rows stay GPU-local between reconciliations (north_star; g4r_comm_sync_sparse /
                                    g4r_set_sync_every).  1: EXACT replicas -- every step each rank's per-occurrence gradient rows of the
                                    gathered item rows are all-gathered and every rank applies all of them in rank order, with the
                                    reference's duplicate semantics over the concatenated occurrence list (gru4rec.py:335-340,407-431):
                                    replicas never diverge, no base copies, no sync_every (SURVEY 8e option 3).  Measured with virtual
                                    ranks: applying ALL ranks' per-occurrence Adagrad steps diverges from four
                                    ranks on, like summed deltas did in round 3 -- the popular items receive N full-size steps.
                                    2: the same exchange, MEAN form: an item's parameter increment is the mean over the ranks that
                                    touch it of each rank's own increment, its Adagrad accumulator the sum of those ranks'
                                    last-occurrence increments -- the GPU-local mode's reconciliation rule taken every step.
                                    3 (what GRU4Rec.sparse_exact = True selects): REDUCE form.  All ranks draw the same negatives; the
                                    gradient rows of those shared columns are summed over the ranks, the ranks' input / target
                                    occurrences are listed one rank behind the other, all scaled by 1 / nranks: the occurrence list of
                                    ONE batch of nranks x batch_size rows sharing one row of negatives (gru4rec.py:436-437), updated
                                    with the reference's rule.  Modes 1-3 want the same `seed` on every rank (one sample stream; dropout
                                    masks are keyed by seed + 7919 * rank inside the library); the ranks' raw dense gradients travel in
                                    the same all-gathered block and every rank sums them in rank order: ONE collective per step.
                                    Mode 3 checks every step that the ranks' negatives are the same ids (a rank in the padded tail of
                                    its plan holds none: the ids then come from the first rank that has them); a mismatch turns the
                                    step's cost into NaN on every rank -- the run stops at the caller's NaN check */
    int32_t defer_updates;       /* 1 (or G4R_DEFER=1 in the environment): single GPU, Adagrad without momentum / lmbd, graph replay -- the update of a
                                    gathered row (gru4rec.py:420-431) whose item is not gathered again inside the current window of 16 steps (known
                                    ahead from the plan and the sample store) is applied by ONE flush launch at the end of the window instead of by
                                    its step's update launch: the same operands and arithmetic, bit-identical results, a launch long enough for the
                                    HBM (~60 % of 8 TB/s at BASELINE configs[2]); costs 2-5 % of the step rate */
} g4r_config;

typedef struct g4r_model g4r_model;

/* ---- lifetime ------------------------------------------------------------------------------- */
int  g4r_device_count(void);
const char* g4r_last_error(void);
const char* g4r_version(void);
int  g4r_sizeof_config(void);   /* sizeof(g4r_config), for binding self-checks */
/* replaces GRU4Rec.init()'s theano.shared allocations, gru4rec.py:267-294 */
int  g4r_create(const g4r_config* cfg, g4r_model** out);
void g4r_destroy(g4r_model* m);

/* ---- parameters (gru4rec.py:742-781 savemodel/loadmodel get_value/set_value) ------------------ */
/* name: "Wy" [I,D], "By" [I], "E" [I,emb], "Wx" [in,3D], "Wh" [D,D], "Wrz" [D,2D], "Bh" [3D], "H" [B,D];
 * optimizer state with prefix "acc_" / "vel_" (gru4rec.py:331,401,425).  `layer` ignored for Wy/By/E. */
int g4r_set_param(g4r_model* m, const char* name, int32_t layer, const float* host, int64_t count);
int g4r_get_param(g4r_model* m, const char* name, int32_t layer, float* host, int64_t count);

/* ---- negative sampling (gru4rec.py:539-571; kernel semantics custom_theano_ops.py:318-349) ---- */
/* cum_p: float32 cumulative supp**alpha (P, :543-545,556); lq_tgt/lq_smp: logQ tables (:495), may be NULL */
int g4r_set_popularity(g4r_model* m, const float* cum_p, const float* lq_tgt, const float* lq_smp, int64_t n);
/* test hook: overwrite the device sample store (rows x n_sample) and freeze refills */
int g4r_set_sample_store(g4r_model* m, const int32_t* store, int64_t rows);
int g4r_get_sample_store(g4r_model* m, int32_t* store, int64_t rows);
int64_t g4r_sample_store_rows(g4r_model* m);

/* ---- epoch plan: the (X, Y, M, R) argument stream of train_function, gru4rec.py:599-651 ------- */
/* Host-side scheduler (no GPU needed): restates the while/for loop of fit() for a whole epoch.
 * Pass NULL outputs to only count.  Returns the number of steps T (or <0); *n_compact receives the
 * number of batch-shrink events (gru4rec.py:647-651).  compact_maps is [n_compact][batch_size]:
 * new row j takes old row map[j] (-1 = none). */
int64_t g4r_build_plan(const int32_t* offset_sessions, int64_t n_sessions, const int64_t* session_order,
                       const int32_t* data_items, int32_t batch_size, int32_t n_sample,
                       int32_t* in_idx, int32_t* out_idx, uint8_t* reset, int32_t* M,
                       int64_t* compact_steps, int32_t* compact_maps, int64_t max_steps, int64_t max_compact,
                       int64_t* n_compact);
/* upload a plan: in_idx/out_idx [T,B] int32, reset [T,B] uint8, M [T].  Also captures and instantiates the step graph
 * (nothing executes), so that the first g4r_train_steps call does not pay for it. */
int g4r_set_plan(g4r_model* m, const int32_t* in_idx, const int32_t* out_idx, const uint8_t* reset,
                 const int32_t* M, int64_t T, const int64_t* compact_steps, const int32_t* compact_maps,
                 int64_t n_compact);

/* ---- the hot path: replaces `train_function(in_idx, y, len(iters), reset)`, gru4rec.py:584,623 - */
/* runs plan steps [t0, t0+n): gather -> GRU -> sampled scoring -> loss -> backward -> Adagrad, with no
 * host round trip in between; per-step costs stay on the device until g4r_get_losses. */
int g4r_train_steps(g4r_model* m, int64_t t0, int64_t n_steps);
int g4r_get_losses(g4r_model* m, int64_t t0, int64_t n, float* out);     /* cost of :623 per step */
int g4r_synchronize(g4r_model* m);
int64_t g4r_global_step(g4r_model* m);
/* checkpoint resume ("optimizer-state save"): the number of sample-store refills so far, and the setter that
 * puts a fresh handle where a saved run stopped (global step: dropout counters, store row pointer; refills: store contents) */
int64_t g4r_refills(g4r_model* m);
int g4r_set_step_counters(g4r_model* m, int64_t global_step, int64_t refills);
/* average HIP-event time (ms) per launch of each step kernel since the last reset; names via index.
 * g4r_profile: 0 = off, 1 = on (steps are launched eagerly with start / stop events attached to every dispatch), 2 = on, with the
 * two roles of the single-GPU update launch as launches of their own (k_dense_grad, k_sparse_update): the embedding
 * gather / scatter north_star prices against the HBM roofline, timed ALONE (results are identical either way). */
int g4r_kernel_time(g4r_model* m, int32_t which, const char** name, double* total_ms, int64_t* launches);
int g4r_profile(g4r_model* m, int32_t enable);

/* hidden state (gru4rec.py:589-590 zeroing, :647-651 compaction; evaluation.py:134-139) */
int g4r_reset_hidden(g4r_model* m);

/* ---- prediction: replaces the compiled `self.predict` / evaluate functions --------------------- */
/* gru4rec.py:691-711 (+ symbolic_predict :729-741): allocate prediction state for `batch` rows */
int g4r_predict_begin(g4r_model* m, int32_t batch);
/* zero rows where zero_mask[0..n_mask) != 0 (n_mask <= batch of g4r_predict_begin; later rows keep their state), then keep
 * rows in `keep_rows` order (NULL = identity), evaluation.py:134-139, gru4rec.py:712-717 */
int g4r_predict_hidden(g4r_model* m, const uint8_t* zero_mask, int32_t n_mask, const int32_t* keep_rows, int32_t n_keep);
/* forward only; scores[m, n_sel] = final_act(h Wy[item_idx]^T + By) (all items if item_idx NULL); out may be NULL.
 * mrows may be smaller than the batch of g4r_predict_begin: rows from mrows on are not stepped and keep their state */
int g4r_predict_step(g4r_model* m, const int32_t* in_idx, int32_t mrows, const int32_t* item_idx, int64_t n_sel,
                     float* out_scores);
/* rank of column target_col[i] of row i among columns [col_begin, n_sel) of the last g4r_predict_step's
 * scores (evaluation.py:56-65; col_begin = 0 for the all-items case, = M when `items` were given) */
int g4r_rank_targets(g4r_model* m, const int32_t* target_col, int32_t mrows, int64_t col_begin, int32_t mode,
                     float* ranks);
/* not in the reference: the k best of the scores g4r_predict_step would return for the same call (same hidden-state update),
 * per row: score descending, equal scores by lower column, NaN last; scores bit-identical to g4r_predict_step's.
 * out_cols[mrows * k] are positions in item_idx (item indices when item_idx is NULL), out_scores[mrows * k].
 * 1 <= k <= min(n_sel, G4R_TOPK_MAX). */
#define G4R_TOPK_MAX 256
int g4r_recommend_step(g4r_model* m, const int32_t* in_idx, int32_t mrows, const int32_t* item_idx, int64_t n_sel,
                       int32_t k, int32_t* out_cols, float* out_scores);

/* not in the reference: g4r_recommend_step with excluded items.  Candidate positions whose item is excluded for a row are never
 * returned for it; the order and the scores of the rest are g4r_recommend_step's (softmax is NOT renormalised over them).
 * excl_offs[mrows + 1]: row r excludes the item indices excl_items[excl_offs[r] .. excl_offs[r + 1]) (any order, duplicates
 * allowed, at most G4R_EXCLUDE_MAX distinct per row); NULL = no per-row lists.  excl_mask[ceil(n_items / 32)]: bit (i & 31) of
 * word i >> 5 excludes item index i in every row; NULL = no mask.  Everything is checked before any launch (the hidden state is
 * not advanced by a refused call): offsets monotone, items in range, and at least k eligible candidate positions in every row
 * (duplicate positions count).  With both NULL this is g4r_recommend_step. */
#define G4R_EXCLUDE_MAX 1024
int g4r_recommend_step_filtered(g4r_model* m, const int32_t* in_idx, int32_t mrows, const int32_t* item_idx, int64_t n_sel,
                                int32_t k, const int64_t* excl_offs, const int32_t* excl_items, const uint32_t* excl_mask,
                                int32_t* out_cols, float* out_scores);

/* not in the reference: stateless top-k from whole session histories.  Session i (0 <= i < n) is the item indices
 * hist_items[hist_offs[i] .. hist_offs[i + 1]) (at least one; hist_offs rises strictly); its hidden state starts from h0 (one
 * pointer per layer to float[n][layers[l]], row i = session i; h0 NULL = zeros) and steps through the history on buffers of the
 * call's own.  out_cols / out_scores[n * k] are what g4r_recommend_step_filtered returns for the last item of the history after
 * g4r_predict_step has been fed the others, bit for bit (same item_idx / n_sel / k / exclusions, with excl_offs[n + 1] per
 * session).  out_hidden (one pointer per layer to float[n][layers[l]]; NULL = not wanted) receives the state after the last item.
 * The prediction state (g4r_predict_begin / _hidden / _step, g4r_recommend_step*) is neither read nor changed.  Everything is
 * checked before any launch, as in g4r_recommend_step_filtered; any n >= 1 works (processed in chunks of rows). */
int g4r_recommend_sessions(g4r_model* m, const int64_t* hist_offs, const int32_t* hist_items, int32_t n, const float* const* h0,
                           const int32_t* item_idx, int64_t n_sel, int32_t k, const int64_t* excl_offs, const int32_t* excl_items,
                           const uint32_t* excl_mask, int32_t* out_cols, float* out_scores, float* const* out_hidden);

/* not in the reference: two-stage top-k for large catalogues, the twins of g4r_recommend_step_filtered / g4r_recommend_sessions
 * (same arguments, same checks, same effect on the prediction state; excl_offs and excl_mask may both be NULL) with one more
 * argument, oversample >= 1.  Stage 1 scans the candidates in bf16 and keeps c = min(number of candidates, k * oversample) of them
 * per row, k * oversample <= G4R_SCAN_CAND_MAX; stage 2 scores those in fp32 and returns the k best.
 *   approximate score of (row, column): h and the item's Wy row rounded to bf16 (round to nearest even), the products summed in
 *     fp32 in any order, + By[item] in fp32, then the element-wise final activation in fp32;
 *   candidates of a row: the c best approximate scores among the row's eligible columns, in the order of g4r_recommend_step (score
 *     descending, equal scores by the lower column, NaN last).  Exclusions apply here, so an excluded item never reaches stage 2; a
 *     row with fewer than c eligible columns keeps all it has;
 *   result: every candidate is scored as g4r_predict_step scores it (bit-identical), and the k best by (exact score descending,
 *     lower column first, NaN last) are returned.
 * So every returned score is g4r_predict_step's bit pattern for that item and the order is g4r_recommend_step's; the only
 * approximation is which items reach stage 2, and with c >= the row's eligible columns the result IS the exact call's, bit for bit.
 * softmax / softmax_logit final activations are refused (their values need the whole row: the fp32 scan again); so are top layers
 * wider than 512.  The bf16 copy of Wy (a "shadow table", n_items x the top layer padded to 128 / 256 / 512, 2 bytes each) is built
 * on the first call and rebuilt on the first call after anything that may have changed Wy (g4r_train_steps,
 * g4r_virtual_train_steps, g4r_set_param, g4r_comm_sync_sparse, g4r_sync_import, g4r_virtual_sync_dense).  g4r_scan_table_release
 * frees it (the next scan rebuilds it); g4r_get_debug "scan_table" -> (bytes held, 1 if valid, builds so far); g4r_destroy frees it. */
#define G4R_SCAN_CAND_MAX 1024
int g4r_recommend_step_scan(g4r_model* m, const int32_t* in_idx, int32_t mrows, const int32_t* item_idx, int64_t n_sel, int32_t k,
                            int32_t oversample, const int64_t* excl_offs, const int32_t* excl_items, const uint32_t* excl_mask,
                            int32_t* out_cols, float* out_scores);
int g4r_recommend_sessions_scan(g4r_model* m, const int64_t* hist_offs, const int32_t* hist_items, int32_t n, const float* const* h0,
                                const int32_t* item_idx, int64_t n_sel, int32_t k, int32_t oversample, const int64_t* excl_offs,
                                const int32_t* excl_items, const uint32_t* excl_mask, int32_t* out_cols, float* out_scores,
                                float* const* out_hidden);
int g4r_scan_table_release(g4r_model* m);

/* not in the reference: approximate top-k over an item index (IVF).  The items are partitioned into n_lists lists, each with a
 * centroid of dimension Dtop + 1; item i is indexed by v_i = [Wy[i], By[i]], whose inner product with [h, 1] is the item's logit.
 *   g4r_ivf_assign   out_list[i] = the list of item i for the given centroids [n_lists][Dtop + 1] (finite): the list that maximises
 *                    v_i . c - |c|^2 / 2 in fp32, equal objectives to the lower list.  Computed on the device from the current Wy / By.
 *   g4r_ivf_set      installs an index: the centroids, list_offs[n_lists + 1] (from 0 to n_items, monotone) and list_items[n_items], a
 *                    permutation of all items that holds every list in ascending item index.  Everything is checked; the device
 *                    tables are built before it returns: a bf16 copy of Wy in list order (every list padded to whole blocks of 32
 *                    positions; n_items x the padded top layer x 2 bytes, plus the pads) -- the shadow table of the bf16 scan is not
 *                    needed and not built by this path.  They are rebuilt from the current weights on the first call after anything
 *                    that may have changed Wy (the entries listed above); the centroids and the partition stay as set, which costs
 *                    recall, never correctness.
 *   g4r_ivf_release  frees the host and device copies; g4r_destroy does too.  g4r_get_debug "ivf_index" -> (lists, blocks of 32
 *                    positions, bytes the device tables hold, 1 if they are valid, builds so far).
 * g4r_recommend_sessions_ivf takes the histories, h0, k, the exclusions and out_hidden of g4r_recommend_sessions_scan (all items
 * are the candidates), oversample >= 1 and nprobe in [1, min(n_lists, G4R_IVF_NPROBE_MAX)].  A row's result:
 *   probes      the nprobe lists with the largest fl32(h . c_w + c_b), equal values to the lower list; a function of the row's final
 *               hidden state only.  out_probes[n * nprobe] (NULL: not wanted) receives them, best first.
 *   candidates  over the eligible items of the probed lists, the c = min(k * oversample, G4R_SCAN_CAND_MAX) best approximate scores
 *               (the bf16 scan's, bit for bit) in the order (score descending, lower ITEM INDEX first, NaN last); exclusions apply here.
 *   result      the candidates scored as g4r_predict_step scores them and the k best by (exact score, lower item index first)
 *               returned as item indices.  out_found[i] = min(k, the candidates of row i): a row is short only when its probed
 *               lists hold fewer than k eligible items; the entries at and after out_found[i] hold item 0 and score NaN.
 * So a row's result does not depend on the rows it is called with or on the chunking, with nprobe = n_lists it is
 * g4r_recommend_sessions_scan's with the same oversample, and when c covers the eligible items of the probed lists it is the exact
 * top-k over their union.  The stage-1 lists take rows * nprobe * c * 8 bytes per chunk: nprobe * c <= G4R_IVF_WS_MAX.  Refused
 * before any launch: no index, softmax / softmax_logit, a top layer wider than 512, k, oversample, nprobe or nprobe * c out of range,
 * and what g4r_recommend_sessions refuses.  The prediction state is neither read nor changed. */
#define G4R_IVF_LISTS_MAX 65536
#define G4R_IVF_NPROBE_MAX 256
#define G4R_IVF_WS_MAX 65536
int g4r_ivf_assign(g4r_model* m, const float* centroids, int32_t n_lists, int32_t* out_list);
int g4r_ivf_set(g4r_model* m, const float* centroids, int32_t n_lists, const int64_t* list_offs, const int32_t* list_items);
int g4r_ivf_release(g4r_model* m);
int g4r_recommend_sessions_ivf(g4r_model* m, const int64_t* hist_offs, const int32_t* hist_items, int32_t n, const float* const* h0,
                               int32_t k, int32_t oversample, int32_t nprobe, const int64_t* excl_offs, const int32_t* excl_items,
                               const uint32_t* excl_mask, int32_t* out_cols, float* out_scores, int32_t* out_found,
                               float* const* out_hidden, int32_t* out_probes);

/* not in the reference: multi-step continuation of n whole sessions, stateless.  The arguments of g4r_recommend_sessions_scan
 * (oversample = 0: the exact selection of g4r_recommend_sessions) plus steps >= 1 and no_repeat; out_cols / out_scores hold
 * n * steps * k entries, [session][step][rank].  Step 0 is g4r_recommend_sessions(_scan) of the histories.  For s >= 1 the item of
 * step s - 1's best column (item_idx[column], or the column) is fed to the GRU as the session's next input and the k best are selected
 * again -- bit for bit what g4r_recommend_sessions(_scan) returns for the one-item history {that item}, started from the state the
 * previous step left, with the same candidates, mask and lists.  no_repeat != 0: every item fed back is also added to its session's
 * exclusion list, so it is never returned to that session again (the history itself is excluded only where the caller lists it in
 * excl_offs / excl_items); it needs a duplicate-free item_idx, at most G4R_EXCLUDE_MAX - (steps - 1) distinct listed items per
 * session and at least k + steps - 1 eligible candidate positions per session (no list ever holds a pad).  out_hidden receives the
 * state that produced the LAST step's scores: after the history and the steps - 1 fed-back items; the last winner is not consumed.
 * Everything is checked before any launch; the prediction state is neither read nor changed.  The feedback runs on the device: one
 * stream synchronisation and one download per chunk of rows, whatever steps is. */
int g4r_continue_sessions(g4r_model* m, const int64_t* hist_offs, const int32_t* hist_items, int32_t n, const float* const* h0,
                          const int32_t* item_idx, int64_t n_sel, int32_t k, int32_t oversample, int32_t steps, int32_t no_repeat,
                          const int64_t* excl_offs, const int32_t* excl_items, const uint32_t* excl_mask, int32_t* out_cols,
                          float* out_scores, float* const* out_hidden);

/* not in the reference: a device-resident session store, so that a serving process neither replays a session's history nor carries its
 * state and seen items between calls.  One store per model.  It holds `capacity` slots; slot s holds one session's hidden state (every
 * layer; per layer float[capacity][layers[l] padded to 4]), its seen list (at most seen_cap item indices, sorted, duplicate-free), the
 * list's length and an overflow flag.  The entries are slot-level: which session owns which slot, and which slot is given up when none
 * is free, is the caller's map (GRU4Rec.open_session_store keeps one in Python).  The store does not watch the weights: a caller that
 * changes them (g4r_train_steps, g4r_set_param, ...) closes the store, or serves states of the old weights.
 *   g4r_store_open   1 <= capacity < 2^31, 0 <= seen_cap <= G4R_EXCLUDE_MAX (0: no lists are kept).  Refused while a store is open.  Every
 *     slot starts at the zero state with an empty list.  A failed allocation frees what it got: the model stays usable, the store closed.
 *   g4r_store_close  frees the slots (no store open: nothing happens).  g4r_destroy closes it too.
 *   g4r_get_debug "session_store" -> (capacity, seen_cap, bytes the slots hold); all 0 without an open store.
 *   g4r_store_push   n rows; row r is the events ev_items[ev_offs[r] .. ev_offs[r + 1]) (item indices, at least one; ev_offs rises
 *     strictly: the history arguments of g4r_recommend_sessions) of the session in slot slots[r].  slots: distinct, in [0, capacity).
 *     fresh[r] != 0: the row starts from the zero state, an empty list and a clear flag, whatever the slot held; otherwise from what
 *     the slot holds.  The events step the row's state exactly as g4r_recommend_sessions steps a history from h0, and the state after
 *     the last one is written back to the slot.  seen_cap > 0: the row's items are merged into the slot's list in event order -- an
 *     item already listed is skipped; a full list records nothing further, and a new item then sets the slot's flag.  RULE: the list is
 *     the first seen_cap distinct items of the session in event order, held sorted; the flag says that the session has shown more.
 *     k == 0: nothing is selected, out_cols / out_scores are not touched.  1 <= k <= G4R_TOPK_MAX: out_cols / out_scores[n * k] are what
 *     g4r_recommend_sessions(_scan) returns for the session's whole history from zero, bit for bit (oversample 0: the exact selection,
 *     >= 1: the two-stage one, as g4r_continue_sessions takes it), with excl_mask and -- exclude_seen != 0 -- the slot's list AFTER this
 *     call's merge as the row's exclusion list.  exclude_seen needs seen_cap > 0, a duplicate-free item_idx and
 *     k + seen_cap + (candidate positions the mask takes) <= candidates: the lists live on the device, so every list counts as full
 *     (a conservative bound).  out_overflow[n] (NULL: not wanted) receives the rows' flags after the merge (0 with seen_cap = 0).
 *     Everything is checked before any launch and before any slot changes; a refused call changes nothing.  One stream synchronisation
 *     per chunk of rows.  The prediction state is neither read nor changed.
 *   g4r_store_peek   the selection of g4r_store_push (k >= 1) from what the slots hold: no events, nothing stepped, nothing written.
 *   g4r_store_read   rows of the store by slot -> out_hidden (one pointer per layer to float[n][layers[l] padded to 4]), out_seen
 *     int32[n][seen_cap] (entries from the row's length on are unspecified), out_len[n], out_flag[n]; any of them NULL: not wanted.
 *   g4r_store_write  the reverse (NULL: that part of the slots stays as it is; seen and len go together).  Refused: a length outside
 *     [0, seen_cap], a list that is not strictly ascending or holds an item index out of range.
 * Both take distinct slots in range, any 1 <= n <= capacity. */
int g4r_store_open(g4r_model* m, int64_t capacity, int32_t seen_cap);
int g4r_store_close(g4r_model* m);
int g4r_store_push(g4r_model* m, const int64_t* ev_offs, const int32_t* ev_items, const int32_t* slots, const int32_t* fresh, int32_t n,
                   const int32_t* item_idx, int64_t n_sel, int32_t k, int32_t oversample, int32_t exclude_seen, const uint32_t* excl_mask,
                   int32_t* out_cols, float* out_scores, int32_t* out_overflow);
int g4r_store_peek(g4r_model* m, const int32_t* slots, int32_t n, const int32_t* item_idx, int64_t n_sel, int32_t k, int32_t oversample,
                   int32_t exclude_seen, const uint32_t* excl_mask, int32_t* out_cols, float* out_scores, int32_t* out_overflow);
int g4r_store_read(g4r_model* m, const int32_t* slots, int32_t n, float* const* out_hidden, int32_t* out_seen, int32_t* out_len,
                   int32_t* out_flag);
int g4r_store_write(g4r_model* m, const int32_t* slots, int32_t n, const float* const* hidden, const int32_t* seen, const int32_t* len,
                    const int32_t* flag);

/* not in the reference: beam search over the continuations of n whole sessions, stateless.  The arguments of g4r_continue_sessions with
 * k = beams (1 <= beams <= min(candidates, G4R_BEAM_MAX)) plus `combine`.  Step 0 is g4r_recommend_sessions(_scan) of the histories with
 * k = beams: beam i of a session is column i, its path score that column's score.  For s >= 1 every beam's last item is fed to the GRU
 * from the beam's own state and its `beams` best next items are selected -- bit for bit g4r_recommend_sessions(_scan) of the one-item
 * history {that item} from that state, with the same candidates, mask and lists (no_repeat != 0: plus the items of the beam's own
 * path).  Of the session's beams x beams extensions (beam b, column j, step score x) the `beams` best by path score become the new
 * beams, each with the state its parent's step left:
 *   G4R_BEAM_SUM      path score = fl32(parent's path score + x);
 *   G4R_BEAM_PRODUCT  path score = fl32(parent's path score * x), a result of magnitude below 2^-126 (NaN is not) replaced by 0.0;
 *                     only for softmax / softmax_logit final activations (probabilities);
 *   order             path score descending, equal scores by the lower b * beams + j, NaN last.
 * G4R_BEAM_PRODUCT rescales after every step's selection, step 0 included: with m the new beam 0's path score, finite and > 0,
 * m = g * 2^e, 1 <= g < 2, every path score of the session is multiplied by 2^-e (exact) and e is added to the session's scale_exp:
 * path probability = path score * 2^scale_exp for any number of steps.  (G4R_BEAM_SUM leaves scale_exp 0.)
 * Outputs: the back-pointer records out_parent / out_cols / out_step_scores[n * steps * beams], [session][step][beam]: beam i of step s
 * extends beam out_parent of step s - 1 (step 0: i itself) by the candidate position out_cols (item index when item_idx is NULL)
 * whose step score is out_step_scores; out_path_scores[n * beams] and out_scale_exp[n] after the last step, best beam first.  The path
 * of a final beam is read backwards through out_parent.  The refusals of g4r_continue_sessions apply with k = beams; everything is
 * checked before any launch; the prediction state is neither read nor changed.  Selection, re-parenting and the list upkeep run on
 * the device: one stream synchronisation and one download per chunk of sessions, whatever steps and beams are. */
#define G4R_BEAM_MAX 32
#define G4R_BEAM_SUM 0
#define G4R_BEAM_PRODUCT 1
int g4r_beam_sessions(g4r_model* m, const int64_t* hist_offs, const int32_t* hist_items, int32_t n, const float* const* h0,
                      const int32_t* item_idx, int64_t n_sel, int32_t beams, int32_t oversample, int32_t steps, int32_t no_repeat,
                      int32_t combine, const int64_t* excl_offs, const int32_t* excl_items, const uint32_t* excl_mask,
                      int32_t* out_parent, int32_t* out_cols, float* out_step_scores, float* out_path_scores, int32_t* out_scale_exp);

/* not in the reference: stochastic decoding of the continuations of n whole sessions, stateless -- `samples` independent draws per
 * session from the model's own next-item distribution, with a temperature and an optional top-k truncation.  The arguments of
 * g4r_continue_sessions without k and oversample, plus samples (1 .. G4R_SAMPLE_MAX), top_k (0: none, else 1 .. min(candidates,
 * G4R_TOPK_MAX)), temperature (finite, > 0, finite reciprocal), seed and first_step (>= 0, first_step + steps <= 2^31 - 1).  Draw
 * (i, j) -- session i, sample j -- has the row id q = i * samples + j (n * samples <= 2^31 - 1).  Every draw starts from the state
 * after the history (from zero, or from h0 row i); at step s it draws one item, which is fed to the GRU as its next input and, with
 * no_repeat, joins its own exclusion list: g4r_continue_sessions' feedback on n * samples rows.
 *   logit z   of a candidate position: g4r_predict_step's score, bit for bit, for the element-wise final activations; for softmax /
 *             softmax_logit the pre-activation value h . Wy_i + By_i (no stored softmax matrix is read);
 *   noise g   lane (item & 3) of the Philox4x32-10 call (item >> 2, q, first_step + s, G4R_STREAM_GUMBEL) keyed by seed (low, high
 *             word), item the absolute item index: x -> u = (float)(x >> 9) * 2^-23 + 2^-24 -> g = -logf(-logf(u)) (precise logf);
 *   key       fl32(fl32(z * invT) + g), invT = 1.0f / temperature, never contracted into an FMA;
 *   choice    the eligible position with the largest key (equal keys: the lower position; NaN last): a draw from softmax(z / T) over
 *             the eligible positions.  top_k = t: the eligible positions are first cut to the t best by z (g4r_recommend_sessions'
 *             exact order with k = t, the same exclusions) and the argmax runs over those; top_k = 1 is g4r_continue_sessions' path (k = 1).
 * out_cols / out_scores[n * samples * steps], [session][sample][step]: the chosen position (item index when item_idx is NULL) and its
 * z, not its key.  out_hidden (NULL: not wanted): per layer n * samples rows, the state that produced the LAST step's scores.  The
 * refusals of g4r_continue_sessions apply with k = top_k, or 1 without it; everything is checked before any launch; the prediction
 * state is neither read nor changed.  One stream synchronisation and one download per chunk of sessions (a chunk holds at most
 * 512 draw rows).  Log-probabilities of the draws and nucleus (top-p) sampling: g4r_sample_sessions_lp. */
#define G4R_SAMPLE_MAX 64
#define G4R_STREAM_GUMBEL 0x47554D42u
int g4r_sample_sessions(g4r_model* m, const int64_t* hist_offs, const int32_t* hist_items, int32_t n, const float* const* h0,
                        const int32_t* item_idx, int64_t n_sel, int32_t steps, int32_t no_repeat, const int64_t* excl_offs,
                        const int32_t* excl_items, const uint32_t* excl_mask, int32_t samples, int32_t top_k, float temperature,
                        uint64_t seed, int32_t first_step, int32_t* out_cols, float* out_scores, float* const* out_hidden);

/* not in the reference: g4r_sample_sessions plus the log-probability of every drawn item (out_logprobs[n * samples * steps], NULL: not
 * wanted) and nucleus sampling (top_p in (0, 1], 0: off; it needs top_k).  With both off it makes g4r_sample_sessions' launches and
 * returns its bits.  Arithmetic of one draw row at one step, E its eligible candidate positions (exactly those the selection may return):
 *   zeta   the largest z over E in the selection's order (the exact selection's top-1);
 *   d_n    fl32(fl32(z_n - zeta) * invT), two roundings, no FMA;
 *   q_n    rn_u64(2^39 * expf(d_n)) (precise expf), 0 where d_n is NaN: the argmax has 2^39 exactly, a term more than about 27 below
 *          zeta * invT has 0;
 *   Q      the sum of q_n over E as an exact 64-bit integer: the same bits whatever the row count, the chip, the chunking (more than
 *          2^24 candidate positions are refused with these options, so Q < 2^63);
 *   logprob of the chosen position c: fl32((double)d_c - log((double)Den * 2^-39)), Den the integer mass of the set drawn from: Q when
 *          untruncated; C_t, the sum of q over the row's t = top_k best (zeta their first z), with top_k alone; C_m with top_p;
 *   top_p  the t best in the selection's order, C_j the integer prefix sums of their q: m is the smallest j with (double)C_j >=
 *          (double)top_p * (double)Q (none: m = t), and the draw is the argmax of the key over the first m entries.  So top_p = 1 gives
 *          top_p = 0's results, and a top_p below the first entry's share top_k = 1's with logprob 0.
 * Scores that are not finite (zeta NaN or infinite) give undefined log-probabilities. */
int g4r_sample_sessions_lp(g4r_model* m, const int64_t* hist_offs, const int32_t* hist_items, int32_t n, const float* const* h0,
                           const int32_t* item_idx, int64_t n_sel, int32_t steps, int32_t no_repeat, const int64_t* excl_offs,
                           const int32_t* excl_items, const uint32_t* excl_mask, int32_t samples, int32_t top_k, float temperature,
                           uint64_t seed, int32_t first_step, int32_t* out_cols, float* out_scores, float* const* out_hidden, float top_p,
                           float* out_logprobs);

/* not in the reference: the log-partition of n whole sessions, stateless: the replay of g4r_recommend_sessions (its arguments and
 * refusals with k = 1, at most 2^24 candidate positions), then out_zeta[i] = zeta and out_Q[i] = Q of session i as defined above, over
 * its eligible candidate positions at the given temperature.  lse = zeta * invT + log(Q * 2^-39) (in double) is the logarithm of the sum
 * of exp(z * invT) over them: z * invT - lse is the log-probability of any eligible position under softmax(z / temperature). */
int g4r_session_log_partition(g4r_model* m, const int64_t* hist_offs, const int32_t* hist_items, int32_t n, const float* const* h0,
                              const int32_t* item_idx, int64_t n_sel, const int64_t* excl_offs, const int32_t* excl_items,
                              const uint32_t* excl_mask, float temperature, float* out_zeta, uint64_t* out_Q);

/* not in the reference: audience selection, the transposed question -- for each of n_items items (item indices, duplicates allowed,
 * every position gets its own list) the k sessions with the largest value, stateless: the replay of g4r_recommend_sessions (hist_*, n,
 * h0 and their refusals), any n.  The value of (session i, item):
 *   by = G4R_AUDIENCE_SCORE     the item's score for the session, g4r_predict_step's bit pattern (what g4r_score_candidates_sessions
 *                               stores for an element-wise final activation); refused for softmax / softmax_logit
 *   by = G4R_AUDIENCE_LOGPROB   fl32((double)d - log((double)Q * 2^-39)), d = fl32(fl32(z - zeta) * invT): the log-probability
 *                               softmax(z / temperature) over the session's eligible items gives the item, zeta and Q of the session as
 *                               g4r_session_log_partition returns them over the whole catalogue (at most 2^24 items), z the item's
 *                               score (the pre-activation value for softmax / softmax_logit); temperature is read in this mode only
 * exclude_history != 0: a session whose history holds the item is not eligible for it and is never listed, and with
 * G4R_AUDIENCE_LOGPROB the session's history items leave its normaliser (g4r_session_log_partition with the history as the exclusion
 * list: at most G4R_EXCLUDE_MAX distinct items per history).
 * Output, [n_items][k] row-major and out_counts[n_items]: row j holds the out_counts[j] <= k eligible sessions with the largest value
 * for items[j], as indices into the histories, in g4r_recommend_step's order with the session in the column's place -- value
 * descending, equal values (float ==) to the lower index, NaN below every number; entries at and after out_counts[j] hold session -1
 * and value NaN.  The result depends on nothing else: not on the chunking (G4R_SESSIONS_CHUNK) nor on the other sessions of the call.
 * Limits: 1 <= k <= G4R_AUDIENCE_MAX = 65536 (not bounded by G4R_TOPK_MAX, it may exceed n), 1 <= n_items <= G4R_AUDIENCE_ITEMS_MAX =
 * 4096, n_items * k <= G4R_AUDIENCE_ENTRIES_MAX = 2^23 (the running lists, 16 bytes an entry and two sides, then take 256 MiB of
 * device memory and the unpacked result 64 MiB).  The lists stay on the device while the sessions stream past, 512 a chunk: one
 * stream synchronisation per chunk, no download before the last one.  Every check happens before any launch. */
#define G4R_AUDIENCE_MAX 65536
#define G4R_AUDIENCE_ITEMS_MAX 4096
#define G4R_AUDIENCE_ENTRIES_MAX (1LL << 23)
#define G4R_AUDIENCE_SCORE 0
#define G4R_AUDIENCE_LOGPROB 1
int g4r_audience_sessions(g4r_model* m, const int64_t* hist_offs, const int32_t* hist_items, int32_t n, const float* const* h0,
                          const int32_t* items, int32_t n_items, int32_t k, int32_t by, float temperature, int32_t exclude_history,
                          int32_t* out_sessions, float* out_values, int32_t* out_counts);

/* not in the reference: item-to-item neighbours in the model's own embedding space -- the k candidates most similar to each of n
 * query items.  Stateless: the prediction state and the training state are neither read nor changed.
 *   table T     space = G4R_SPACE_OUTPUT: Wy, rows of layers[n_layers - 1] floats.  G4R_SPACE_INPUT: E when embed_mode is
 *               G4R_EMBED_SEPARATE (rows of `embedding` floats), Wy when it is G4R_EMBED_CONSTRAINED; a one-hot input model has no
 *               input embedding and the call is refused with that reason.
 *   score       of (query item q, candidate item j).  G4R_SIM_DOT: sum_d T[q, d] * T[j, d], fp32 products, fp32 accumulation, one
 *               chain from zero in ascending d.  G4R_SIM_COSINE: (dot(q, j) * inv[q]) * inv[j], inv[i] = 1 / sqrt(sum_d T[i, d]^2)
 *               in fp32 (IEEE division and square root), inv[i] = 0 when the sum is 0: a zero row scores 0 against everything,
 *               itself included.  The score of a pair depends on the values of the two rows only -- not on the candidate's
 *               position, the other queries of the call, the chunks the call is cut into, or whether item_idx was given -- so it
 *               is bit-identical wherever the pair appears.
 *   selection   g4r_recommend_step's order: score descending, equal scores by the lower candidate position, NaN last;
 *               1 <= k <= min(candidates, G4R_TOPK_MAX).
 *   candidates  item_idx[n_sel] (duplicates allowed, every position is a candidate), NULL: all items.  out_cols holds positions in
 *               item_idx, item indices when it is NULL.
 *   exclusions  exclude_self != 0 skips every candidate position that holds the query's own item; excl_mask is the mask of
 *               g4r_recommend_step_filtered (NULL = none).  A query with fewer than k eligible positions is refused before any
 *               launch; the refusal names the query.
 *   q_idx[n]    query item indices, any n >= 1, duplicates allowed; processed in chunks of rows sized by the library
 *               (G4R_SIM_CHUNK in the environment forces a smaller chunk, for tests: the results do not depend on it).  Results are
 *               copied to the host once per chunk; there is no host round trip inside a chunk.
 * Everything is checked before the first launch.  The inverse norms are cached per table, built on the first cosine call and rebuilt
 * on the first one after anything that may have changed the tables (g4r_train_steps, g4r_virtual_train_steps, g4r_set_param,
 * g4r_comm_sync_sparse, g4r_sync_import, g4r_virtual_sync_dense); g4r_get_debug "sim_norms" -> (bytes held, 1 if valid, builds so
 * far); g4r_destroy frees them. */
#define G4R_SIM_DOT 0
#define G4R_SIM_COSINE 1
#define G4R_SPACE_OUTPUT 0
#define G4R_SPACE_INPUT 1
int g4r_similar_items(g4r_model* m, int32_t space, int32_t metric, const int32_t* q_idx, int64_t n, const int32_t* item_idx,
                      int64_t n_sel, int32_t k, int32_t exclude_self, const uint32_t* excl_mask, int32_t* out_cols, float* out_scores);

/* not in the reference: diversified top-k by maximal marginal relevance (MMR) -- k of a row's pool of P candidates picked greedily,
 * each pick trading the candidate's relevance against its largest similarity to the picks before it.  A row's pool is the positions
 * 0 .. P - 1 with item indices c_j and relevance s_j; position order is the tie order.  Every operation below is IEEE fp32, in this
 * order, never contracted into an FMA; lam is a float in [0, 1] and mu = 1.0f - lam.
 *   relevance   normalize == 0: r_j = s_j.  Otherwise, with lo / hi the minimum / maximum of the row's s (NaN entries skipped):
 *               r_j = (s_j - lo) / (hi - lo) when hi > lo, else every r_j = 0.0f.
 *   similarity  sim(i -> j) is g4r_similar_items' score of the pair (query item c_i, candidate item c_j) in the same space and
 *               metric, bit for bit: one ascending chain of dot products from zero, for G4R_SIM_COSINE (dot * inv[c_i]) * inv[c_j]
 *               with the cached inverse norms; a zero row gives 0.
 *   pick 0      v_j = lam * r_j over all positions.
 *   pick t >= 1 with i the position picked last, for every position j not picked yet: m_j = sim(i -> j) when t == 1, otherwise
 *               m_j = sim(i -> j) > m_j ? sim(i -> j) : m_j; v_j = (lam * r_j) - (mu * m_j): two rounded products, one rounded
 *               subtraction.
 *   selection   the largest v_j in g4r_recommend_step's order: value descending, the lower position first, NaN last.
 * out_pos / out_value[n * k] receive, pick by pick, the position in the pool and v.  1 <= k <= P <= G4R_DIVERSIFY_POOL_MAX.
 *
 * g4r_diversify_lists re-ranks n supplied lists: items[n * P] (item indices, duplicates allowed) and rel[n * P] (finite).  Stateless.
 * Everything is checked before any launch: k and P, the item indices, lam in [0, 1] (NaN refused), finite rel, space and metric as
 * in g4r_similar_items (a one-hot input model has no G4R_SPACE_INPUT).  Rows are processed in chunks, one synchronisation each.
 *
 * g4r_diversify_sessions takes the arguments of g4r_recommend_sessions_scan with k = pool (oversample = 0: the exact selection of
 * g4r_recommend_sessions; otherwise the bf16 scan with pool * oversample <= G4R_SCAN_CAND_MAX): the pool of session i is what that
 * call returns for it, positions in its order, s = its scores, the columns mapped to items through item_idx.  The selection stays
 * on the device; out_cols / out_scores[n * k] receive the picked candidates' columns (positions in item_idx, item indices when it
 * is NULL) and their model scores -- g4r_recommend_sessions' bit patterns -- in pick order, out_pos / out_value as above, out_hidden
 * as there.  Only n * k entries of each come back, once per chunk of rows.  The checks are those of g4r_recommend_sessions(_scan)
 * with k = pool (so every session needs `pool` eligible candidate positions) plus the ones above; a pool score that is not finite
 * follows the arithmetic and the order above, with no special case.  The prediction state is neither read nor changed. */
#define G4R_DIVERSIFY_POOL_MAX 128
int g4r_diversify_lists(g4r_model* m, int32_t space, int32_t metric, const int32_t* items, const float* rel, int64_t n, int32_t P,
                        int32_t k, float lam, int32_t normalize, int32_t* out_pos, float* out_value);
int g4r_diversify_sessions(g4r_model* m, const int64_t* hist_offs, const int32_t* hist_items, int32_t n, const float* const* h0,
                           const int32_t* item_idx, int64_t n_sel, int32_t k, int32_t pool, int32_t oversample,
                           const int64_t* excl_offs, const int32_t* excl_items, const uint32_t* excl_mask, int32_t space,
                           int32_t metric, float lam, int32_t normalize, int32_t* out_cols, float* out_scores, int32_t* out_pos,
                           float* out_value, float* const* out_hidden);

/* not in the reference: item groups (a brand, an artist, a category, a parent product) and per-group caps: "at most c per group" in a
 * top-k list or along a generated path.
 *
 * g4r_set_item_groups gives the model its group table: groups[n], n == n_items, entry i the dense group index of item i or -1 for an
 * ungrouped item (never capped); an entry below -1 is refused.  groups NULL with n 0 clears the table.  The number of groups is the
 * largest entry + 1.  The table is a device array of the model that only grows; it does not depend on the weights (no entry that
 * changes them touches it) and g4r_destroy frees it.  g4r_get_item_groups copies it back (out[n], n == n_items; refused without one).
 *
 * The cap rule.  A row has a list of P positions in selection order, position j with the column c_j and the score s_j; its item is
 * i_j = item_idx[c_j] (c_j itself without item_idx) and its group g_j = groups[i_j].  With a cap c >= 1 and a prior multiset of
 * groups (possibly empty; n0(g) the number of times g occurs in it), position j is KEPT iff
 *     g_j < 0   or   n0(g_j) + #{i < j : g_i == g_j} < c
 * -- the greedy walk down the list with one counter per group.  The result is the first min(k, kept) kept positions in list order:
 * n_kept is that count, entries at and after n_kept are pads (column -1, score NaN, position -1).  Scores are copied, never
 * recomputed: a returned score is g4r_recommend_sessions' bit pattern.  1 <= k <= P <= G4R_TOPK_MAX; a prior list holds at most
 * G4R_GROUP_PRIOR_MAX entries, each in [0, number of groups).
 *
 * g4r_recommend_sessions_capped takes the arguments of g4r_recommend_sessions_scan with k = pool (oversample = 0: the exact selection;
 * otherwise the bf16 scan with pool * oversample <= G4R_SCAN_CAND_MAX): the list of session i is what that call returns for it, the
 * prior is empty, and the rule runs on the device behind the selection.  out_cols / out_scores / out_pos[n * k] receive the kept
 * positions' columns, scores and positions in the pool, out_kept[n] the counts, out_hidden as there.  A row with out_kept == k is
 * exact over the whole catalogue (the walk ended inside the pool); so is one whose pool held all its eligible positions.
 *
 * g4r_continue_sessions_capped takes the arguments of g4r_continue_sessions the same way: every step selects `pool` positions, the
 * rule keeps up to k of them -- out_cols / out_scores[n * steps * k], out_kept[n * steps] -- and the first kept one is the winner:
 * it is fed back as the row's next input, joins the exclusion list with no_repeat as there, and its group, if it has one, joins
 * the row's prior.  The prior of session i at step 0 is prior_groups[prior_offs[i] .. prior_offs[i + 1]) (prior_offs NULL: empty).
 * A step at which the rule keeps nothing (out_kept == 0) falls back to the unconstrained best: list position 0 leaves in slot 0,
 * is fed back, and its group joins the prior like any winner's.  Every row needs pool + steps - 1 eligible candidate positions with
 * no_repeat, and a prior list plus steps - 1 must not exceed G4R_GROUP_PRIOR_MAX.
 *
 * g4r_cap_lists applies the rule to n supplied lists items[n * P] (item indices, duplicates allowed), each with its own prior
 * (prior_offs NULL: none): out_pos[n * k] and out_kept[n].  Stateless; rows go in chunks, one synchronisation each.
 *
 * Everything is checked before any device work, each refusal naming the limit or the row: no group table, cap < 1, pool outside
 * [1, G4R_TOPK_MAX], k outside [1, pool], a prior list too long, a prior group out of range, and the refusals of the uncapped entry
 * with k = pool.  The prediction state is neither read nor changed. */
#define G4R_GROUP_PRIOR_MAX 1024
int g4r_set_item_groups(g4r_model* m, const int32_t* groups, int64_t n);
int g4r_get_item_groups(g4r_model* m, int32_t* out, int64_t n);
int g4r_recommend_sessions_capped(g4r_model* m, const int64_t* hist_offs, const int32_t* hist_items, int32_t n, const float* const* h0,
                                  const int32_t* item_idx, int64_t n_sel, int32_t k, int32_t pool, int32_t oversample,
                                  const int64_t* excl_offs, const int32_t* excl_items, const uint32_t* excl_mask, int32_t cap,
                                  int32_t* out_cols, float* out_scores, int32_t* out_pos, int32_t* out_kept, float* const* out_hidden);
int g4r_continue_sessions_capped(g4r_model* m, const int64_t* hist_offs, const int32_t* hist_items, int32_t n, const float* const* h0,
                                 const int32_t* item_idx, int64_t n_sel, int32_t k, int32_t pool, int32_t oversample, int32_t steps,
                                 int32_t no_repeat, const int64_t* excl_offs, const int32_t* excl_items, const uint32_t* excl_mask,
                                 int32_t cap, const int64_t* prior_offs, const int32_t* prior_groups, int32_t* out_cols,
                                 float* out_scores, int32_t* out_kept, float* const* out_hidden);
int g4r_cap_lists(g4r_model* m, const int32_t* items, int64_t n, int32_t P, int32_t k, int32_t cap, const int64_t* prior_offs,
                  const int32_t* prior_groups, int32_t* out_pos, int32_t* out_kept);

/* not in the reference: scores of per-row candidate lists (the re-ranking stage behind a retrieval stage).  Row r's list is the
 * item indices cand_items[cand_offs[r] .. cand_offs[r + 1]) (at least one; cand_offs rises strictly; duplicates allowed, every
 * position is scored), at most G4R_CAND_MAX positions in all.  g4r_score_candidates advances the prediction state exactly as
 * g4r_predict_step does (in_idx / mrows as there).  k == 0: out_scores[cand_offs[mrows] - cand_offs[0]] receives the scores in CSR
 * order, row r's bit for bit those g4r_predict_step returns with item_idx = row r's list (softmax / softmax_logit normalise over the
 * row's own list); out_pos may be NULL.  1 <= k <= G4R_TOPK_MAX (every list at least k long): out_pos / out_scores[mrows * k]
 * receive row r's k best (position in its list, score), what g4r_recommend_step returns for that list, bit for bit.  Everything is
 * checked before the state advances. */
#define G4R_CAND_MAX 2147483392LL      /* 2^31 - 256 */
int g4r_score_candidates(g4r_model* m, const int32_t* in_idx, int32_t mrows, const int64_t* cand_offs, const int32_t* cand_items,
                         int32_t k, float* out_scores, int32_t* out_pos);
/* The same for n whole session histories, stateless: hist_offs / hist_items / h0 / h_out as in g4r_recommend_sessions (same chunks,
 * same replay), cand_offs[n + 1] / cand_items / k / out_scores / out_pos as in g4r_score_candidates with one list per session. */
int g4r_score_candidates_sessions(g4r_model* m, const int64_t* hist_offs, const int32_t* hist_items, int32_t n, const float* const* h0,
                                  const int64_t* cand_offs, const int32_t* cand_items, int32_t k, float* out_scores, int32_t* out_pos,
                                  float* const* h_out);

/* The whole of evaluation.evaluate_gpu (evaluation.py:86-147) as ONE call with no host round trip per step: the
 * session-parallel test loop comes as a plan (g4r_build_plan on the test sessions in id order with n_sample = 1: the loop of
 * evaluation.py:96-139 is the loop of fit), every step runs the GRU forward, scores all items (items == NULL) or
 * [targets | items], ranks the targets (mode = G4R_RANK_*), and adds #(rank <= cut) and sum 1/rank for each cut-off into
 * device accumulators; hidden rows of finished sessions are zeroed / dropped on the device (evaluation.py:134-139).
 * Outputs: recall_sum[n_cut], mrr_sum[n_cut] (divide by *n_events). */
int g4r_evaluate(g4r_model* m, const int32_t* in_idx, const int32_t* out_idx, const uint8_t* reset, const int32_t* M, int64_t T,
                 int32_t batch, const int64_t* compact_steps, const int32_t* compact_maps, int64_t n_compact,
                 const int32_t* items, int64_t n_items_sel, const int32_t* cutoffs, int32_t n_cut, int32_t mode,
                 double* recall_sum, double* mrr_sum, int64_t* n_events);

/* not in the reference: g4r_evaluate's test loop returning, for EVERY event, its top-k list, the rank of its target and the
 * target's score, instead of two sums.  Plan arguments (in_idx ... mode) as in g4r_evaluate; the rank of an event is the value
 * g4r_evaluate feeds to its sums (same counts, same tie rule, same 'tiebreaking' noise), so sum(rank <= cut) is its recall_sum.
 * With an element-wise final activation every step makes ONE pass over the candidates' Wy rows, which yields both the rows' k best
 * and the (greater, equal) counts against the rows' target scores; softmax / softmax_logit materialise the scores first, as
 * g4r_evaluate and g4r_recommend_step do (two passes and more).
 *   slot[T * batch]   where the event at (step, row) goes in the outputs; rows >= M[step] are padding (-1, not read).  Every slot
 *                     is in [0, n_slots) and used at most once; slots no event uses read zero.
 *   k                 1 <= k <= min(candidates, G4R_TOPK_MAX); the candidates are all items, or `items` (the list is chosen
 *                     among `items` only, never among the other rows' targets that g4r_evaluate ranks in front of them).
 *   excl_mask         as in g4r_recommend_step_filtered, NULL = none.
 *   seen_*            exclusion of the items an event's session has shown up to and including the input event, in linear space:
 *                     session s (0 <= s < n_seen) has the sorted, duplicate-free item indices seen_items[seen_offs[s] ..
 *                     seen_offs[s + 1]) (at most G4R_EXCLUDE_MAX) and, beside each, seen_first: the position in the session of
 *                     the item's first occurrence.  The event at (step, row) belongs to session seen_sess[step * batch + row] and
 *                     its input is that session's event number seen_pos[..]: an item is excluded iff it is in the session's list
 *                     with seen_first <= seen_pos.  seen_offs NULL = none.  Exclusions remove items from the list, never from
 *                     the rank.
 *   outputs           by slot, any may be NULL: out_items[n_slots * k] item indices (also with `items`), out_scores[n_slots * k]
 *                     in g4r_recommend_step's order (score descending, equal scores by the lower candidate position, NaN last)
 *                     and with g4r_predict_step's bit patterns (softmax with `items`: normalised over `items`, as
 *                     g4r_recommend_step returns them), out_rank[n_slots], out_target_score[n_slots] (the score the rank compared
 *                     with; softmax with `items`: normalised over [targets | items], as g4r_evaluate ranks it).
 * Everything is checked before the first launch (the prediction state is untouched by a refused call): sizes, indices, slots, the
 * tables, and that every session keeps at least k eligible candidate positions at its last event -- the refusal names the session.
 * Results are written on the device at the event's slot and copied to the host once, at the end; when n_slots * k * 8 bytes exceed
 * G4R_EVENTS_PIECE_BYTES (G4R_EVENTS_PIECE in the environment overrides it, for tests), in pieces of that many bytes of whole
 * steps, one synchronisation each.  No host round trip per step.  Uses the prediction state like g4r_evaluate (fresh state, `batch`
 * rows). */
#define G4R_EVENTS_PIECE_BYTES (1LL << 30)
int g4r_recommend_events(g4r_model* m, const int32_t* in_idx, const int32_t* out_idx, const uint8_t* reset, const int32_t* M, int64_t T,
                         int32_t batch, const int64_t* compact_steps, const int32_t* compact_maps, int64_t n_compact,
                         const int32_t* items, int64_t n_items_sel, int32_t mode, const int64_t* slot, int64_t n_slots, int32_t k,
                         const uint32_t* excl_mask, const int64_t* seen_offs, const int32_t* seen_items, const int32_t* seen_first,
                         int64_t n_seen, const int32_t* seen_sess, const int32_t* seen_pos, int32_t* out_items, float* out_scores,
                         float* out_rank, float* out_target_score);

/* not in the reference: the log-likelihood of the logged next item at EVERY event of a test set -- g4r_recommend_events' plan loop
 * giving every event what g4r_session_log_partition gives its replayed prefix, plus the z of its target.  Plan arguments, slot,
 * excl_mask and the seen_* tables as in g4r_recommend_events; temperature as in g4r_session_log_partition.
 * Contract (g4r_sample_sessions_lp's, so that the two agree).  For the event whose input is position p of its session and whose
 * target t is the session's next item, E = the eligible candidate positions: all items, or the positions of `items` (a duplicate
 * counts once per position), minus excl_mask, minus -- with the seen tables -- the items the session has shown up to and including
 * position p.  E is the set of positions g4r_recommend_events' list may hold for the event.
 *   z_n      g4r_predict_step's score of candidate n, bit for bit; the pre-activation value for softmax / softmax_logit
 *   zeta     the largest z over E in the selection's order (NaN below every number, -0.0 == +0.0)
 *   d_n      fl32(fl32(z_n - zeta) * fl32(1 / temperature)),  q_n = rn(2^39 * expf(d_n)) (0 for NaN),  Q = the exact sum of q_n over E
 * Outputs by slot: out_z[n_slots] = z_t (also for an ineligible target), out_zeta[n_slots], out_Q[n_slots], out_eligible[n_slots]
 * = 1 iff t holds a position in E.  From them, in float64 on the host:
 *   lse      fl32(zeta * invT + log(Q * 2^-39)): g4r_session_log_partition's bits for the prefix
 *   logprob  fl32(d_t - log(Q * 2^-39)) for an eligible target, -inf otherwise
 * Q is an integer sum, so every output is independent of batch, of how the columns are cut into ranges and of the pieces.
 * Everything is checked before the first launch: g4r_recommend_events' checks with k = 1 (every session keeps at least one eligible
 * position at its last event; the refusal names the session), the temperature, at most 2^24 candidate positions.  Per step and
 * whatever the final activation: two scans of the candidates' Wy rows (zeta, then Q relative to it), no score matrix.  Pieces of
 * G4R_EVENTS_PIECE_BYTES (16 bytes an event), one synchronisation and one download each.  Uses the prediction state like
 * g4r_evaluate. */
int g4r_loglik_events(g4r_model* m, const int32_t* in_idx, const int32_t* out_idx, const uint8_t* reset, const int32_t* M, int64_t T,
                      int32_t batch, const int64_t* compact_steps, const int32_t* compact_maps, int64_t n_compact, const int32_t* items,
                      int64_t n_items_sel, const int64_t* slot, int64_t n_slots, const uint32_t* excl_mask, const int64_t* seen_offs,
                      const int32_t* seen_items, const int32_t* seen_first, int64_t n_seen, const int32_t* seen_sess,
                      const int32_t* seen_pos, float temperature, float* out_z, float* out_zeta, uint64_t* out_Q, uint8_t* out_eligible);

/* ---- input pipeline: the pandas work in front of fit() for TAB separated files -------------
 * run.py:45-78 `pd.read_csv(sep='\t', usecols, dtype={session: int32, item: str})` + gru4rec.py:534-538
 * `itemids = data[item_key].unique(); itemidmap = Series(arange, index=itemids); data['ItemIdx'] = itemidmap[...]`.
 * Multi-threaded mmap parse; item indices are assigned in order of first appearance (= pandas unique()).  Host only.
 * Returns 0, G4R_IO_UNSUPPORTED when the file needs a general CSV parser (quoted fields, missing values, session ids
 * that are not int32: the caller falls back to pandas), or <0 with g4r_last_error().  time_col may be NULL.
 * n_threads: 0 = all cores (at most 64, at most one per MiB), > 0 = at most that many, < 0 = exactly -n_threads (tests). */
#define G4R_IO_UNSUPPORTED 1
typedef struct g4r_events g4r_events;
int g4r_events_load(const char* path, const char* session_col, const char* item_col, const char* time_col, int32_t n_threads,
                    g4r_events** out);
int64_t g4r_events_rows(const g4r_events* ev);
int64_t g4r_events_items(const g4r_events* ev);
int64_t g4r_events_item_bytes(const g4r_events* ev);     /* total length of the distinct item-id strings */
int32_t g4r_events_time_kind(const g4r_events* ev);      /* 0 = no time column, 1 = int64, 2 = float64 */
/* session[n_rows] int32, item_idx[n_rows] int32, time[n_rows] (int64 or double by time_kind), item_off[n_items + 1] offsets
 * into item_bytes (item ids in index order, not terminated).  Any output may be NULL. */
int g4r_events_copy(const g4r_events* ev, int32_t* session, int32_t* item_idx, void* time, int64_t* item_off, char* item_bytes);
void g4r_events_free(g4r_events* ev);

/* ---- multi-GPU (new: the reference is single-GPU).  RCCL all-reduce of dense GRU gradients ---- */
int g4r_comm_unique_id(char* out128);                         /* rank 0: ncclGetUniqueId */
int g4r_comm_init(g4r_model* m, const char* id128, int32_t nranks, int32_t rank);
/* Reconciliation of the GPU-local item tables (Wy / By / E and their optimizer state; north_star: "sparse embedding rows stay
 * GPU-local").  For every row some rank rewrote since the last call, every replica ends at
 *     base + sum over ranks q, in rank order, of (value on rank q - base),      base = the common value at the last call,
 * so each rank's updates are kept in full (a row one rank alone trained ends at that rank's value up to fp32 rounding) and the
 * replicas are bit-identical afterwards.  Packed (id list, delta rows) parts are
 * all-gathered in item-id ranges: the traffic follows the number of touched rows.  Called by fit() at the end of an epoch. */
int g4r_comm_sync_sparse(g4r_model* m);
/* combine rule of the reconciliation, per kind of plane: parameters (Wy / By / E and their velocities) and optimizer statistics
 * (Adagrad / RMSprop accumulators, Adam moments and counters).  G4R_SYNC_SUM: base + sum of the deltas of the ranks that touched
 * the row; G4R_SYNC_MEAN: base + their mean.  Default: parameters MEAN (N full-size steps from one starting point must not add up:
 * measured); statistics SUM with adapt = adagrad (squared gradients of all ranks' events add up as they would
 * on one GPU) and MEAN with rmsprop / adadelta / adam, whose statistics are moving averages: summed deltas of a decayed
 * average go negative once several ranks touch a row (NaN in the next sqrt) -- tests/test_gpu_virtual_ranks.py. */
#define G4R_SYNC_SUM 0
#define G4R_SYNC_MEAN 1
int g4r_sync_set_rule(g4r_model* m, int32_t param_rule, int32_t stat_rule);
/* allocates the touched-row bitmap and the base copies, base = the tables as they are now (g4r_comm_init calls it;
 * g4r_set_param of an item table afterwards also sets its base) */
int g4r_sync_enable(g4r_model* m);
/* The two halves of g4r_comm_sync_sparse without RCCL, for tests that emulate ranks with several handles on one GPU.
 * group 0: Wy / By rows, 1: E rows.  export: sorted ids of the touched rows and, plane after plane (Wy, acc_Wy, [vel ...], By,
 * acc_By, ...), their delta rows [n][W]; returns n (pass NULL pointers to size the buffers; g4r_sync_row_floats = sum of the plane
 * widths).  import: the parts of ALL ranks in rank order (this handle's own included) -> reset, add, new base, bitmap cleared. */
int64_t g4r_sync_row_floats(g4r_model* m, int32_t group);
int64_t g4r_sync_export(g4r_model* m, int32_t group, int32_t* ids, float* rows, int64_t cap_rows);
int g4r_sync_import(g4r_model* m, int32_t group, int32_t nparts, const int64_t* counts, const int32_t* const* ids,
                    const float* const* rows);
/* Virtual ranks: `n` handles on ONE device stand in for the n ranks of a data-parallel run (handle q created with rank = q,
 * nranks = n, no communicator; each with its own plan of the same length).  Runs plan steps [t0, t0 + n_steps) in lock-step:
 * per step every handle's kernels up to the dense gradients, the n gradient buffers summed in rank order (what the RCCL
 * all-reduce of the real run delivers), every handle's dense apply (divides by nranks) and GPU-local sparse update.  Item tables
 * are reconciled by the caller (g4r_sync_export / g4r_sync_import).  For validating the N > 1 training semantics -- e.g.
 * Recall@20 of 2 / 8 ranks against 1 (evaluation.py:62-75) -- on a one-GPU box; not a fast path. */
int g4r_virtual_train_steps(g4r_model* const* ms, int32_t n, int64_t t0, int64_t n_steps);
/* the dense form of g4r_comm_sync_sparse (item tables of up to G4R_SYNC_DENSE_MB = 64 MB per group: [n_items][plane widths + 1]
 * delta buffers packed, summed and applied on the device) with the sum taken in process over n handles of one device */
int g4r_virtual_sync_dense(g4r_model* const* ms, int32_t n);
/* k > 0: g4r_train_steps reconciles the item tables itself every k steps (counted across calls), between two steps and without
 * leaving the stream -- where every table takes the dense form and a communicator exists: returns 1; returns 0 when the caller has to
 * call g4r_comm_sync_sparse itself (tables too large for the dense form); k = 0 switches it off. */
int g4r_set_sync_every(g4r_model* m, int32_t k);
int g4r_comm_min_i64(g4r_model* m, int64_t* value);            /* in-place min over ranks */
int g4r_comm_max_i64(g4r_model* m, int64_t* value);            /* in-place max over ranks: the common plan length (shorter plans are
                                                                  padded with M = 0 steps so that every rank issues the same all-reduces) */
int g4r_comm_nranks(g4r_model* m);                             /* ranks RCCL reports for the communicator (1 without one) */
/* One-shot all-reduce of the dense GRU gradients through peer memory -- the switch next to the RCCL all-reduce (new: the reference
 * is single-GPU; north_star asks for the gradients of gru4rec.py:383-384's dense parameters to be all-reduced every step).  The
 * gradients are a few hundred KB, so instead of a ring every rank reads the other ranks' buffers over its point-to-point xGMI
 * links and adds them in rank order itself (k_p2p_allreduce: per-workgroup stamped hand-offs, two alternating buffers, no
 * host work per step, captured in the step graph).  One node, at most 8 ranks.
 *   g4r_p2p_enable   on a handle with a communicator: allocates this rank's exchange region, all-gathers the 64-byte IPC handles
 *                    through RCCL, maps the peers.  Collective.  GRU4Rec does this when G4R_P2P=1.
 *   g4r_p2p_export / g4r_p2p_attach   the same with the handles carried by the caller (handles: nranks x 64 bytes in rank order);
 *                    needs no RCCL, so two PROCESSES on one device can be each other's ranks (tests/test_gpu_p2p.py).
 * A peer that does not publish within G4R_P2P_TIMEOUT_MS (default 20000) makes g4r_train_steps fail instead of hang. */
int g4r_p2p_enable(g4r_model* m);
int g4r_p2p_export(g4r_model* m, char* out_handle64);
int g4r_p2p_attach(g4r_model* m, const char* handles, int32_t nranks, int32_t rank);
int g4r_p2p_active(g4r_model* m);                              /* 1 when the step's all-reduce is the peer-memory one */

/* ---- debugging / tests ---------------------------------------------------------------------- */
/* copy a named intermediate of the most recent step (e.g. "scores", "dS", "dV0", "hd0") */
int g4r_get_debug(g4r_model* m, const char* name, float* host, int64_t count);
/* Test support (tests/test_gpu_loss_rows.py): the loss launch of a training step on score rows the caller supplies.  scores: B x ldSc
 * floats (g4r_get_debug "ldSc"), in: the scores, out: d cost / d s as the step leaves it in "scores"; M: the active rows of the step
 * (1 .. batch_size); lossrow: batch_size floats out, rows < M written.  Runs the k_loss_rows instantiation the model's steps run, on
 * batch_size workgroups, and waits for it.  The step state on the device is the same before and after; the "scores" and "lossrow"
 * buffers are overwritten (every step rewrites them before it reads them).  count must be batch_size * ldSc. */
int g4r_debug_loss_rows(g4r_model* m, float* scores, int64_t count, int32_t M, float* lossrow);
/* Test support (tests/test_gpu_sample_sessions.py), not in the reference: out[p] = the noise g of g4r_sample_sessions for row id
 * row_id, step `step` and item index items[p] >= 0, p < n, computed by the device function its selection calls. */
int g4r_debug_gumbel(g4r_model* m, uint64_t seed, uint32_t row_id, uint32_t step, const int32_t* items, int64_t n, float* out);
/* Test support (tests/test_gpu_sample_logprobs.py), not in the reference: out[p] = the term q of g4r_sample_sessions_lp's row normaliser
 * for the logit z[p] relative to zeta[p] at the reciprocal temperature inv_t, p < n, computed by the device function its scan calls. */
int g4r_debug_lse_terms(g4r_model* m, const float* z, const float* zeta, int64_t n, float inv_t, uint64_t* out);
int g4r_selftest_mfma(float* max_abs_err);
/* Row gather / scatter micro-benchmark on a table of n_items x W floats (fresh allocation, random rows, every launch its own
 * rows): mode 0 gather to a compact buffer, 1 gather consumed in registers (what the step's fused gathers do), 2 Adagrad scatter
 * (gradient row read + parameter r/w + accumulator r/w).  Replaces, as an object of measurement, the reference's gather kernel
 * custom_theano_ops.py:505-519 and its sparse Adagrad scatter gru4rec.py:335-340,428-431.  kernel_us: mean dispatch-to-completion
 * time of a launch (HIP events attached to the dispatch); wall_us: back-to-back launches on one stream, per launch. */
int g4r_bench_rows(int32_t device, int64_t n_items, int32_t W, int64_t rows_per_launch, int32_t launches, int32_t mode, uint64_t seed,
                   double* kernel_us, double* wall_us);                    /* 16x16x4 f32 MFMA layout check */
/* Test support (tests/test_gpu_stress.py): `launches` passes of a streaming read-modify-write over `mbytes` MiB of device memory
 * on a stream of their own, queued asynchronously -- HBM / Infinity-Cache load next to the caller's training steps, the condition
 * under which round 3's stale-register pipeline (mutation build 4) went wrong and an idle GPU never shows.  g4r_stress_stop waits
 * for the passes and frees the buffer.  Nothing of the reference corresponds to it. */
int g4r_stress_start(int32_t device, int64_t mbytes, int32_t launches, void** handle);
int g4r_stress_stop(void* handle);

#ifdef __cplusplus
}
#endif
#endif

// g4r_host_model.hpp -- part of libgru4rec_hip.so's host code; included once, by g4r_api.hip (one translation unit: the kernels are templates
// instantiated there).  Holds: error string, kernel time slots, the model handle (g4r_model), allocation helpers, launch geometries and the shape policies that pick a kernel.
static thread_local std::string g_err;
static int fail(const std::string& s) { g_err = s; return -1; }
// printf-style setter for the host-only translation units of the library (g4r_io.cpp)
void g4r_set_error(const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
}
#define HIPCHK(x)                                                                                        \
    do {                                                                                                 \
        hipError_t e_ = (x);                                                                             \
        if (e_ != hipSuccess)                                                                            \
            return fail(std::string(#x) + ": " + hipGetErrorString(e_) + " @" + std::to_string(__LINE__)); \
    } while (0)
#define NCCLCHK(x)                                                                                         \
    do {                                                                                                   \
        ncclResult_t e_ = (x);                                                                             \
        if (e_ != ncclSuccess)                                                                             \
            return fail(std::string(#x) + ": " + ncclGetErrorString(e_) + " @" + std::to_string(__LINE__)); \
    } while (0)

enum { KN_GRU_P1 = 0, KN_GRU_P2, KN_SCORE_FWD, KN_LOSS, KN_SCORE_BWD, KN_BWD_PRE, KN_BWD_A, KN_BWD_B, KN_DENSE, KN_ALLREDUCE,
       KN_DENSE_APPLY, KN_SPARSE, KN_UPDATE, KN_BWD_FUSED, KN_FWD_FUSED, KN_GATE, KN_FLUSH, KN_SCAN, KN_FINISH, KN_GRU_V, KN_GRU_H, KN_GRU_DA, KN_GRU_DY, KN_OWNER_WINDOW, KN_AUD_KEYS, KN_AUD_MERGE, KN_COUNT };
static const char* KN_NAMES[KN_COUNT] = {"k_gru_p1", "k_gru_p2", "k_score_fwd", "k_loss_rows", "k_score_bwd", "k_gru_bwd_pre",
                                         "k_gru_bwd_a", "k_gru_bwd_b", "k_dense_grad", "rccl_allreduce", "k_dense_apply",
                                         "k_sparse_update", "k_update", "k_gru_bwd", "k_gru_fwd", "k_gru_gate", "k_sparse_flush", "k_defer_scan", "k_finish_rows", "k_gru_v", "k_gru_h", "k_gru_da", "k_gru_dy", "k_owner_window", "k_audience_keys", "k_audience_merge"};

struct EvRec { int kn; hipEvent_t a, b; };

// ---- the kernels of a training step: chosen once per model (choose_kernels, at g4r_create), dispatched on by step_head / step_tail
// The environment switches that steer the choice, read at g4r_create (tests and A/B runs toggle them between models)
struct KernelSwitches {
    bool no_lean = false;                 // G4R_NO_LEAN: the fused / LDS-staged kernels the lean launches replaced (tests/test_gpu_lean.py)
    bool no_mt = false, no_bmt = false;   // G4R_NO_MT / G4R_NO_BMT: the 64 x 64 scoring tiles instead of k_score_mt / k_score_bmt
    bool no_merge = false;                // G4R_NO_MERGE: dense gradients and sparse rows as two launches, never the merged k_update
    bool allow_lean_update = true;        // G4R_LEAN_UPDATE=0: the merged k_update where k_update_l would run, as the deferred mode runs it
    bool score_b_split = true;            // G4R_SCORE_B_SPLIT=0: k_score_b keeps its role A (the item-gradient tiles), no hosting in k_gru_dy
    bool owner_scan_in_update = false;    // G4R_OWNER_SCAN=1: k_update_l's owners of repeated items scan occ_idx themselves (no pre-scan in k_loss_rows)
    int owner_window = -1;                // G4R_OWNER_WINDOW=0: the owner tables come from the pre-scan in k_loss_rows, every step, not from k_owner_window once per window; 1: from k_owner_window wherever its LDS holds the list; unset: where that pays (g4r_host_create.hpp)
    bool pos_entries = true;              // G4R_POS_ENTRIES=0: the (last, first, count) entries are built inside every step (atomics in k_gru_v / k_score_s, occ_fl), also where k_owner_window could write them per position
    bool defer = false;                   // G4R_DEFER (default: g4r_config::defer_updates)
    int p2_geo = -1, ba_geo = -1;         // G4R_P2_GEO / G4R_BA_GEO = 0 / 1: the 4-wave / 8-wave geometry of k_gru_p2 / k_gru_bwd_a (-1: the policy)
    int wide2 = -1, p1_ks = 128, bb_ks = 0;      // G4R_WIDE2 (wide-layer kernel mask, -1: the policy), G4R_P1_KS / G4R_BB_KS (their K slices)
    unsigned long long skip_kn = 0;       // G4R_SKIP_KN: measurement aid, bit k = leave the launches of slot k (KN_*) out of the step
    bool trace = false;                   // G4R_TRACE: every launch of an (eager) step named on stderr and waited for; no step graphs
};
// What choose_kernels decided; the debug key `kernels` reports these values.  Tile forms: k_gru_p1* then k_gru_p2; k_gru_bwd_pre,
// k_gru_bwd_a, then k_onehot_step (layer 0 of a one-hot input) / k_gru_bwd_bw (dy as K-slice partial sums) / k_gru_bwd_b.
enum GruFwdKind { FWD_LEAN = 0 /* k_gru_v + k_gru_h */, FWD_FUSED = 1 /* k_gru_fwd_fused */, FWD_P1S = 2 /* k_gru_p1s + k_gru_gate */,
                  FWD_P1_N64 = 3, FWD_P1_N32 = 4 };
enum GruBwdKind { BWD_LEAN = 0 /* k_gru_da + k_gru_dy */, BWD_FUSED = 1 /* k_gru_bwd_fused */, BWD_ONEHOT = 2, BWD_BW = 3, BWD_B = 4 };
enum ScoreFwdKind { SF_LEAN = 0 /* k_score_s */, SF_MT = 1 /* k_score_mt_4s */, SF_T3 = 2, SF_T2 = 3, SF_K64 = 4, SF_K128 = 5 /* k_score_fwd_* */ };
enum ScoreBwdKind { SB_LEAN = 0 /* k_score_b */, SB_BMT = 1 /* k_score_bmt */, SB_BWD2 = 2 /* k_score_bwd2 */, SB_W = 3, SB_N = 4 /* k_score_bwd_w / _n */ };
// UP_MERGED: dense-gradient tiles and sparse rows in one launch; UP_SPLIT: k_dense_grad[2], (staged: all-reduce, k_dense_apply), k_sparse_update*
enum UpdateKind { UP_LEAN = 0 /* k_update_l */, UP_MERGED = 1 /* k_update */, UP_SPLIT = 2 };
// wide layers (g4r_wide_kernels.cuh): which kernels run (bit 1 k_gru_p1s + k_gru_gate, 8 k_gru_bwd_bw) and their K-slice geometry
struct WideGeo { int use = 0, ny = 1, nh = 1, kys = 0, khs = 0, bbn = 1, bbk = 0; };
struct StepKernels {
    int fwd[G4R_MAX_LAYERS], bwd[G4R_MAX_LAYERS];
    int p2_deep[G4R_MAX_LAYERS], ba_deep[G4R_MAX_LAYERS];      // k_gru_p2 / k_gru_bwd_a on 8 waves x 256-deep chunks
    WideGeo wg[G4R_MAX_LAYERS];
    int score_fwd;
    int loss_spec, loss_long, loss_quads;      // k_loss_rows<loss_long, loss_spec, loss_long || loss_quads ? 4 : 1>
    int score_bwd;
    int score_a_host;                     // k_score_b's role A: 0 in k_score_b itself, 1 as extra workgroups of the top layer's k_gru_dy (k_gru_dy_a); debug key `score_b_split`
    int kch, ksplit;                      // slabs of the scoring backward: kch score columns each, ksplit of them (-> DevModel)
    int bmt_slabs;                        // k_score_bmt's role-B slabs (0: not chosen)
    int nblkA, nblkB, ndtA, ndtB, nrtB;   // k_score_bwd_w / _n: role A tiles (n x d, one spare d column for dSBy), role B tiles (b x d x slab)
    int update;
    int chunks;                           // float4 chunks per lane of a gathered row in the sparse update (rows of <= 256 / 512 / 1024 floats)
    int wide_dense;                       // k_dense_grad2 (64 x 64 dense-gradient tiles) as a launch of its own
    int finish_rows;                      // k_finish_rows: layer 0's dy from K-slice partial sums, ahead of k_update / k_dense_grad
};

// A device array that only grows: what the inference entries keep between calls (g4r_model's p_*, r_*, ro_*, c_*, s_*, sim_*), sized by
// need, never by a batch.  reserve() is defined below, next to dalloc / dfree.  (The reconciliation keeps a separate kind, with
// headroom and a pinned-host form: g4r_model::Scratch / scratch_ensure, g4r_host_sync.hpp.)
template <class T>
struct DevBuf {
    T* p = nullptr;
    int64_t cap = 0;      // elements
    int reserve(g4r_model* m, int64_t n);
};

// The item index of g4r_recommend_sessions_ivf (g4r_host_ivf.hpp).  Host: what g4r_ivf_set was given -- centroids [nl][Dtop + 1], the
// lists' offsets and their items (ascending within a list).  Device, owned by the index, grow only, rebuilt from the host copy and the
// current Wy / By after weights_changed: the bf16 table in list order (every list padded to whole blocks of 32 positions), By and the
// item of every position, the lists' block ranges and lengths, the centroids (weights transposed [Dtop][nl], biases).  Per chunk: a
// row's centroid entries, its probes and their scores, the (list, row) bitmap, the lists' first triples, the work items, the sorted
// triples and the number of work items.
struct IvfIndex {
    bool set = false, valid = false;
    int nl = 0;
    int64_t nblk = 0, builds = 0;
    std::vector<float> cen;
    std::vector<int64_t> offs;
    std::vector<int32_t> items;
    DevBuf<uint4> tab;
    DevBuf<float> pos_by, cwt, cb, pscores;
    DevBuf<int> pos_item, blk, doffs, probes, toff, trip, n_work;
    DevBuf<uint2> ent;
    DevBuf<unsigned> member;
    DevBuf<int4> work;
};

struct g4r_model {
    g4r_config cfg;
    DevModel dm;                 // host master copy of the device-resident model descriptor
    DevModel* d_dm = nullptr;    // what the kernels read (passed by pointer: 8-byte kernarg)
    int n_cu = 256;              // compute units of the device (tile-count heuristics)
    KernelSwitches sw;           // the environment switches of the kernel choice, as g4r_create read them
    StepKernels kern;            // the kernels a training step runs (choose_kernels)
    hipStream_t stream = nullptr;
    std::vector<void*> allocs;
    // plan
    int *d_in = nullptr, *d_out = nullptr, *d_M = nullptr, *d_cmaps = nullptr;
    unsigned char* d_reset = nullptr;
    float* d_loss = nullptr;
    int64_t T = 0, loss_cap = 0;
    std::vector<int64_t> compact_steps;
    // samples
    int* d_ST = nullptr;
    float *d_P = nullptr, *d_lqt = nullptr, *d_lqs = nullptr;
    int64_t gl = 0;
    bool store_frozen = false, have_pop = false;
    unsigned refills = 0;
    int64_t gstep = 0;
    // launch geometry
    DenseTile* d_tiles = nullptr;
    int ntiles = 0, nblk_occ = 0, nblk_occ_g = 0;
    size_t smem_score = 0, smem_loss = 0, smem_sparse = 0;
    bool defer_on = false;       // deferred row updates (k_defer_scan / k_sparse_flush around every replay of the step graph)
    bool defer_broken = false;   // a call failed between a window's scan and its flush: pending row updates were lost, the handle refuses to go on
    hipEvent_t ev_df[4] = {nullptr, nullptr, nullptr, nullptr};      // profiling: scan / flush launches of a window
    DenseTile* d_tiles64 = nullptr;
    int ntiles64 = 0;
    float* d_tmpH = nullptr;
    // graph
    LeanS h_leanS;
    std::vector<LeanV> h_leanV; std::vector<LeanH> h_leanH; std::vector<LeanDa> h_leanDa; std::vector<LeanDy> h_leanDy;
    LeanS* d_leanS = nullptr;      // argument block of k_score_s
    LeanB* d_leanB = nullptr; LeanB h_leanB;      // argument block of k_score_b
    LeanU* d_leanU = nullptr; LeanU h_leanU;      // argument block of k_update_l, its 16 x 64 dense tiles
    DenseTile* d_tiles16 = nullptr; int ntiles16 = 0;
    bool own_window = false;     // k_owner_window writes the owner tables of a window of steps ahead of them (debug key `owner_window`)
    int own_last = 0;            // ring slot of the last step run (debug key `own_pos`)
    bool pos_entries = false;    // k_owner_window also writes the steps' per-position entries (DevModel::pos_ent; debug key `pos_entries`)
    int pos_hs = 0;              // hash slots of that form in k_owner_window's LDS
    hipEvent_t ev_ow[2] = {nullptr, nullptr};      // profiling: the window launch
    LeanV* d_leanV = nullptr; LeanH* d_leanH = nullptr; LeanDa* d_leanDa = nullptr; LeanDy* d_leanDy = nullptr;      // [layers] argument blocks (g4r_lean_kernels.cuh)
    hipGraphExec_t gexec = nullptr;
    hipGraphExec_t gexec_small = nullptr;        // single GPU: G4R_GRAPH_STEPS_SMALL steps, for what a run leaves after the big replays
    hipGraphExec_t gexec_head = nullptr;         // N > 1 fallback: one step's kernels up to the dense gradients, RCCL eager behind it
    int graph_steps = 0;
    bool dist_graph_failed = false;              // capturing the step with its RCCL all-reduce did not work: head graph + eager tail
    // profiling
    bool profiling = false;
    bool profile_split = false;
    bool exact = false;                          // g4r_config::sparse_exact with nranks > 1
    size_t smem_exact = 0;
    double kn_ms[KN_COUNT] = {0};
    int64_t kn_n[KN_COUNT] = {0};
    std::vector<hipEvent_t> evs;
    // prediction
    int pbatch = 0, ppar = 0;
    float* pH[G4R_MAX_LAYERS][2] = {{nullptr}};
    float* phout[G4R_MAX_LAYERS] = {nullptr};
    float *pVc[G4R_MAX_LAYERS] = {nullptr}, *pz[G4R_MAX_LAYERS] = {nullptr}, *pHr[G4R_MAX_LAYERS] = {nullptr};
    int *p_in = nullptr, *p_tgt = nullptr, *p_keep = nullptr;
    DevBuf<int> p_items;                         // the candidate items of one call (cand_upload)
    unsigned char* p_zero = nullptr;
    float* p_ranks = nullptr;
    DevBuf<float> p_scores;
    int* p_cnt = nullptr;                        // [pbatch][2] streamed (greater, equal) counts of the evaluation
    int64_t p_nsel = 0, p_ldo = 0;
    DevBuf<uint2> p_topk;                        // [rows][ranges][k] per-range lists of g4r_recommend_step (k_topk_range)
    DevBuf<int> p_tcols;                         // [rows][k] its result (the two are reserved together)
    DevBuf<float> p_tscores;
    DevBuf<long long> p_xoffs;                   // exclusions of g4r_recommend_step_filtered: [rows + 1] offsets into p_xitems,
    DevBuf<int> p_xitems;                        // the rows' sorted item lists,
    DevBuf<unsigned> p_xmask;                    // the global item bit mask
    // stateless replay of g4r_recommend_sessions, apart from the prediction state above: per layer a hidden ping-pong, the output,
    // the GRU scratch and the staging of the supplied initial / the final rows (chunk order), all for r_cap rows; the step-major
    // input items, the sort map and lengths of a chunk; its own score matrix (softmax / softmax_logit)
    int r_cap = 0;
    float* rH[G4R_MAX_LAYERS][2] = {{nullptr}};
    float* rhout[G4R_MAX_LAYERS] = {nullptr};
    float *rVc[G4R_MAX_LAYERS] = {nullptr}, *rz[G4R_MAX_LAYERS] = {nullptr}, *rHr[G4R_MAX_LAYERS] = {nullptr};
    float* rio[G4R_MAX_LAYERS] = {nullptr};
    int *r_perm = nullptr, *r_len = nullptr;
    DevBuf<int> r_in;
    DevBuf<float> r_scores;
    // multi-step continuation (g4r_continue_sessions): a chunk's [rows][steps][k] output, the rows' fed-back input items and the current
    // lengths of their growing exclusion lists (the lists themselves: p_xoffs = every row's begin, p_xitems with slack behind each)
    DevBuf<int> ro_cols, ro_in, ro_xlen;
    DevBuf<float> ro_scores;
    int64_t ro_calls = 0, ro_steps = 0;          // g4r_get_debug "continue_steps": calls that passed their checks, (chunk, step) chains enqueued
    // beam search (g4r_beam_sessions; rows = a chunk's beam rows): the beams' GRU input items; (parent, item) of the step's new beams; the
    // begin of every beam row's exclusion list, the two list buffers the lists alternate between and the lengths in each; what a chunk
    // downloads, as 4-byte words: [steps][rows] parent | column | step score, [rows] path score, [sessions] scale_exp
    DevBuf<int> bm_in, bm_sel, bm_xlen, bm_xitems, bm_out;
    DevBuf<long long> bm_beg;
    // sampling (g4r_sample_sessions; rows = a chunk's draw rows): the rows' ids, their chosen (column | item) of the step and its score;
    // outputs, feedback and lists live in the continuation's arrays (ro_*, p_xoffs / p_xitems / p_xmask)
    DevBuf<unsigned> sm_rowid;
    DevBuf<int> sm_pick;
    DevBuf<float> sm_z;
    // its log-probabilities and nucleus (g4r_sample_sessions_lp, g4r_session_log_partition): every row's zeta (the exact selection's top-1,
    // with the column the merge writes beside it), its integer normaliser Q and the chunk's [rows][steps] log-probabilities
    DevBuf<float> sm_zeta, sm_lp;
    DevBuf<int> sm_zcol;
    DevBuf<unsigned long long> sm_Q;
    // per-row candidate scoring (g4r_score_candidates*): one call's (or chunk's) CSR -- row offsets, candidate item indices, scores
    // in CSR order -- the work items of k_score_cand, the top-k lists of k_cand_pack and the selected (position, score) pairs
    DevBuf<long long> c_offs;
    DevBuf<int> c_items;
    DevBuf<float> c_scores;
    DevBuf<int4> c_work;
    DevBuf<uint2> c_topk;
    DevBuf<int> c_tpos;
    DevBuf<float> c_tscores;
    // two-stage top-k (g4r_recommend_step_scan / g4r_recommend_sessions_scan): the bf16 shadow table of Wy in MFMA fragment order
    // (g4r_scan_kernels.cuh), built on first use and again after anything that may have changed Wy (weights_changed); the
    // candidates' columns and counts of one call or chunk; the host copy of k_score_cand's work items
    DevBuf<uint4> s_tab;                         // (cap: 16-byte units)
    int64_t s_tab_builds = 0;
    bool s_tab_valid = false;
    DevBuf<int> s_cols;
    DevBuf<int> s_cnt;
    std::vector<int4> s_work;
    IvfIndex iv;                                 // the item index (g4r_ivf_set / g4r_recommend_sessions_ivf)
    // item neighbours (g4r_similar_items): the inverse row norms of the item tables (0: Wy, 1: E), built on the first cosine call and
    // again after anything that may have changed the tables (weights_changed); the query items of one chunk and their rows
    float* sim_inv[2] = {nullptr, nullptr};
    bool sim_valid[2] = {false, false};
    int64_t sim_builds = 0;
    DevBuf<int> sim_q;
    DevBuf<float> sim_rows;                      // [chunk rows][W] the chunk's query rows (k_sim_gather)
    // diversified top-k (g4r_diversify_lists / _sessions; k_mmr_rerank): a chunk's supplied lists [rows][P] and its picks [rows][k] --
    // position, value and, after a session selection, the picked candidates' columns and model scores
    DevBuf<int> dv_items, dv_pos, dv_cols;
    DevBuf<float> dv_rel, dv_val, dv_scores;
    // item groups and per-group caps (g4r_set_item_groups, g4r_*_capped, g4r_cap_lists; k_group_cap): the group table [n_items] (-1 =
    // ungrouped; it does not depend on the weights, so weights_changed leaves it alone) and the number of groups; a chunk's supplied
    // lists [rows][P]; what the rule keeps [rows][k] -- column, score, position -- and the counts [rows][steps]; the rows' prior lists
    // (begin, current length, the lists with their slack)
    DevBuf<int> gc_groups;
    bool gc_set = false;
    int32_t gc_ngroups = 0;
    DevBuf<int> gc_items, gc_cols, gc_pos, gc_kept, gc_plen, gc_prior;
    DevBuf<float> gc_scores;
    DevBuf<long long> gc_pbeg;
    // audience selection (g4r_audience_sessions; k_audience_keys / k_audience_merge): the M items repeated for every row of a chunk, their
    // work items and scores live in c_items / c_work / c_scores; a chunk's entries [M][rows]; the running lists' two sides [M][k] each;
    // (side, len)[M] twice, read and written alternately; what the call downloads, [M][k] each
    DevBuf<ulonglong2> au_ent, au_list[2];
    DevBuf<int> au_state, au_sess;
    DevBuf<float> au_val;
    // session store (g4r_store_*; g4r_host_store.hpp, g4r_store_kernels.cuh): per layer the slots' hidden rows [capacity][D[l]], the seen
    // lists [capacity][seen_cap] with their lengths and overflow flags [capacity]; per chunk the rows' slots and fresh marks (chunk
    // order), the (begin, length) of their lists for TkGrow, their flags, and the staging of g4r_store_read / _write
    struct SessionStore {
        bool open = false;
        int64_t capacity = 0;
        int seen_cap = 0;
        size_t bytes = 0;
        float* H[G4R_MAX_LAYERS] = {nullptr};
        int *items = nullptr, *len = nullptr, *flag = nullptr;
        DevBuf<int> slot, fresh, xlen, oflag, io;
        DevBuf<long long> xbeg;
    } st;
    unsigned tie_ctr = 0;                      // evaluation step counter of the 'tiebreaking' noise stream
    // the last g4r_recommend_events / g4r_loglik_events call (g4r_get_debug "events_launches"): its steps, the launches whose grid spans the candidate
    // columns, all its launches, the pieces its lists came back in
    int64_t ev_steps = 0, ev_scans = 0, ev_launches = 0, ev_pieces = 0;
    // rccl
    ncclComm_t comm = nullptr;
    bool comm_ready = false;
    // one-shot all-reduce of the dense gradients through peer memory (g4r_p2p_*): this rank's exchange region, the peers' regions
    // as mapped here (IPC), the kernel's argument block
    bool p2p_ready = false;
    void* p2p_region = nullptr;
    void* p2p_peer[G4R_P2P_MAX] = {nullptr};
    unsigned* p2p_round = nullptr;
    int p2p_nblk = 0, p2p_cap = 0;
    P2PArgs p2p_args;
    bool virtual_ranks = false;                  // member of a g4r_virtual_train_steps group: the dense gradients are summed in process
    float* d_vsum = nullptr;                     // scratch of that sum (first member of the group)
    // reconciliation of the GPU-local item tables (g4r_sync_kernels.cuh): per table group (0: Wy / By rows, 1: E rows) the
    // planes (current values, common base, row width) and scratch
    struct SyncPlane { float* cur; float* base; int W; int kind; };      // kind: 0 parameter / velocity, 1 optimizer statistic
    std::vector<SyncPlane> planes[2];
    int sync_rule[2] = {G4R_SYNC_MEAN, G4R_SYNC_SUM};      // combine rule of the parameter planes / of the statistic planes
    bool sync_rule_user = false;                           // set through g4r_sync_set_rule: g4r_sync_enable keeps it
    unsigned char* d_touched = nullptr;
    unsigned char* d_rowcnt = nullptr;           // [n_items] scratch: number of parts that hold a row (MEAN rule)
    int sync_every_dev = 0;                      // > 0: g4r_train_steps reconciles the (dense-form) item tables itself every that many steps
    int64_t since_sync = 0, n_dev_syncs = 0;
    // scratch of the packed-parts reconciliation, kept between calls (a call used to pay five hipMalloc / hipFree pairs)
    // (the inference entries' grow-only arrays are another kind: DevBuf, above)
    struct Scratch { void* p = nullptr; size_t cap = 0; bool host = false; };
    Scratch sc_ids, sc_blk, sc_cnt, sc_all, sc_send, sc_pack, sc_recv, sc_hall;      // sc_hall: pinned host copy of the gathered id lists
    float* d_dense[2] = {nullptr, nullptr};      // dense reconciliation buffers [n_items][sum of plane widths + 1] per table group (small catalogues)
    bool sync_on = false;
};

// The optional stage behind sessions_run's selection (g4r_diversify_sessions; g4r_host_diversify.hpp): k_mmr_rerank picks k of the
// `pool` the selection left in p_tcols / p_tscores, and the chunk downloads the picks instead of the pool
struct MmrStage {
    int tab; const float* T; int W;      // the item table (sim_table)
    bool cosine;
    float lam; int normalize;
    int k;                               // picks per row
    int32_t* out_pos; float* out_value;  // host, [n][k] next to sessions_run's out_cols / out_scores
};

// The other optional stage in that place (g4r_recommend_sessions_capped / g4r_continue_sessions_capped; g4r_host_groups.hpp): the
// selection runs with k = the pool, k_group_cap keeps up to `k` of every list by the cap rule -- with steps >= 1 on every step, between
// the merge and k_rollout_feed, which is pointed at what it kept -- and the chunk downloads that instead of the pools
struct CapStage {
    int cap, k;                                                  // positions of a group a row may keep; entries a row returns per step
    const int64_t* prior_offs; const int32_t* prior_groups;      // host: every session's prior groups (CSR; NULL: none)
    int32_t* out_pos; int32_t* out_kept;                         // host: [n][k] (NULL: not wanted), [n][max(steps, 1)]
};

// every entry that may rewrite Wy / E calls this: the bf16 shadow table of the two-stage top-k, the inverse norms of
// g4r_similar_items and the device tables of the item index are rebuilt on their next use
static inline void weights_changed(g4r_model* m) { m->s_tab_valid = false; m->sim_valid[0] = m->sim_valid[1] = false; m->iv.valid = false; }
// the captured step graphs, stale with what they captured (the kernel choice, the collective); the next step that wants one captures
// it again.  also_head: the head graph (one step's kernels up to the dense gradients) too
static inline void drop_step_graphs(g4r_model* m, bool also_head) {
    for (hipGraphExec_t* g : {&m->gexec, &m->gexec_small, also_head ? &m->gexec_head : nullptr})
        if (g && *g) { (void)hipGraphExecDestroy(*g); *g = nullptr; }
}

// ---- how the steps of a model run (g4r_host_step.hpp).  STEP_GRAPH: whole steps replayed from a captured graph, G4R_GRAPH_STEPS at a
// time.  STEP_HEAD_GRAPH: one step's kernels up to the dense gradients replayed, the tail (all-reduce, dense apply, sparse update)
// launched eagerly behind them.  STEP_EAGER: every launch from the host (use_graph = 0, per-kernel profiling, G4R_TRACE).
enum StepMode { STEP_GRAPH, STEP_HEAD_GRAPH, STEP_EAGER };
// one GPU, staged dense path without a communicator (the generic optimizers: rmsprop / adadelta / adam / plain SGD / grad_cap): no
// collective in the step, so the whole step is captured like the fused single-GPU step (it used to replay a head graph and launch
// its tail eagerly)
static inline bool local_staged(const g4r_model* m) {
    return !m->dm.apply_dense_inplace && m->cfg.nranks <= 1 && !m->comm_ready && !m->p2p_ready && !m->virtual_ranks;
}
// N > 1 (or the one-rank staged mode): the all-reduce is captured with the step, so that a replay covers 16 whole steps
// (kernels, RCCL all-reduce, dense apply) with no host work in between -- unless an earlier capture with the collective failed
static inline bool dist_graph_wanted(const g4r_model* m) {
    return !m->dm.apply_dense_inplace && !m->dist_graph_failed && (m->p2p_ready || m->comm_ready || local_staged(m));
}
// The one place that says which: g4r_train_steps asks it for a call's steps (again after a capture that failed: dist_graph_failed),
// g4r_set_plan for the graphs to capture ahead of the first step.
static inline StepMode step_mode(const g4r_model* m) {
    if (!m->cfg.use_graph || m->profiling || m->sw.trace) return STEP_EAGER;
    return (m->dm.apply_dense_inplace || dist_graph_wanted(m)) ? STEP_GRAPH : STEP_HEAD_GRAPH;
}
// The one place that says whether a step's owner tables came from a window launch (k_owner_window in front of the step's window:
// StepWindow::open) -- and whether its per-position entries did: StepWindow and every launch of the step ask here.  False (per-kernel
// profiling with the split update, G4R_OWNER_WINDOW=0 / G4R_POS_ENTRIES=0, lists past the caps): every kernel gets the null slot and
// the entries are built and taken back inside the step, through occ_fl.
static inline bool window_tables(const g4r_model* m) { return m->own_window && m->kern.update == UP_LEAN && !(m->profiling && m->profile_split); }
static inline bool window_entries(const g4r_model* m) { return m->pos_entries && window_tables(m); }
// slot `slot` of the entry ring (the step's index in its window), or null
static inline const int4* step_entries(const g4r_model* m, int slot) {
    return window_entries(m) ? (const int4*)m->dm.pos_ent + (size_t)slot * (size_t)((m->dm.R + 3) & ~3) : nullptr;
}
// the steps a run leaves behind its replays (fewer than the shortest graph holds): on the staged dense path the head graph + eager
// tail, else eager launches
static inline StepMode single_step_mode(const g4r_model* m, StepMode mode) {
    if (mode != STEP_GRAPH) return mode;
    return m->dm.apply_dense_inplace ? STEP_EAGER : STEP_HEAD_GRAPH;
}

template <class T>
static int dalloc(g4r_model* m, T** p, size_t n, bool zero = true) {
    void* q = nullptr;
    if (n == 0) n = 1;
    HIPCHK(hipMalloc(&q, n * sizeof(T)));
    if (zero) HIPCHK(hipMemsetAsync(q, 0, n * sizeof(T), m->stream));
    m->allocs.push_back(q);
    *p = (T*)q;
    return 0;
}
static void dfree(g4r_model* m, void* p) {
    if (!p) return;
    auto it = std::find(m->allocs.begin(), m->allocs.end(), p);
    if (it != m->allocs.end()) m->allocs.erase(it);
    (void)hipFree(p);
}
// Room for n elements; the contents are not kept.  The stream is drained before the old array goes (kernels enqueued on it may still
// read it), and the handle forgets the array before the new one is asked for: a failed hipMalloc leaves p = NULL, cap = 0, which the
// next call's reserve() sees, never a freed pointer that passes the capacity test.
template <class T>
int DevBuf<T>::reserve(g4r_model* m, int64_t n) {
    if (n <= cap) return 0;
    HIPCHK(hipStreamSynchronize(m->stream));
    dfree(m, p);
    p = nullptr; cap = 0;
    if (dalloc(m, &p, (size_t)n, false)) return -1;
    cap = n;
    return 0;
}
// The device temporaries of one call (g4r_evaluate, g4r_recommend_events): get() is dalloc; all of them are freed when the owner goes
// out of scope, whichever return ends the call
struct CallTemps {
    g4r_model* m;
    std::vector<void*> held;
    explicit CallTemps(g4r_model* m_) : m(m_) {}
    CallTemps(const CallTemps&) = delete;
    CallTemps& operator=(const CallTemps&) = delete;
    ~CallTemps() { for (void* q : held) dfree(m, q); }
    template <class T>
    int get(T** p, size_t n, bool zero = true) {
        if (dalloc(m, p, n, zero)) return -1;
        held.push_back(*p);
        return 0;
    }
};
// softmax / softmax_logit: a score needs its whole row (maximum, sum); the other final activations are element-wise (gru4rec.py:499-500)
static inline bool is_softmax(const DevModel& d) { return d.final_act == G4R_ACT_SOFTMAX || d.final_act == G4R_ACT_SOFTMAX_LOGIT; }
static inline int cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }
static constexpr auto k_score_store = k_score_all<32, false>;     // scores -> memory
static constexpr auto k_score_count = k_score_all<32, true>;      // scores compared with the row's target on the fly
// the forms of k_topk_range by name: k_topk_fused, k_topk_stored, ... (TK_FORMS, g4r_topk_kernels.cuh, says which is which)
#define TK_NAME(name, STORED, EXCL, ...) static constexpr auto name = k_topk_range<STORED, EXCL, ##__VA_ARGS__>;
TK_FORMS(TK_NAME)
#undef TK_NAME

static inline int env_int(const char* name, int dflt) { const char* v = getenv(name); return v ? atoi(v) : dflt; }
// dynamic LDS of the tile-GEMM kernels (g4r_gemm.cuh)
template <int BM, int BN, int BK, bool AKM, bool BNK>
static constexpr size_t tile_smem() { return (size_t)TileCfg<BM, BN, BK, AKM, BNK>::SMEM_FLOATS * sizeof(float); }
static const size_t SMEM_NN = tile_smem<GT_BM, GT_BN, GT_BK, false, false>() + GT_BM * sizeof(int);   // A [m][k], B [k][n] (+ row items)
static const size_t SMEM_NT = tile_smem<GT_BM, GT_BN, GT_BK, false, true>() + GT_BM * sizeof(int);    // A [m][k], B [n][k] (+ row items)
static const size_t SMEM_TN = tile_smem<GT_BM, GT_BN, GT_BK, true, false>();    // A [k][m], B [k][n]
// wide layers: 64-column tiles halve the number of GRU phase-1 workgroups (all resident at once) and read the weights in
// 256-byte runs; the 32-column tiles spread the tiny GEMMs of D ~ 100 over more CUs
static constexpr auto k_gru_p1_n32 = k_gru_p1<GT_BN, P1_BK>;
static constexpr auto k_gru_p1_n64 = k_gru_p1<64, 256>;
static const size_t SMEM_P1_N64 = tile_smem<GT_BM, 64, 256, false, false>() + GT_BM * sizeof(int);
static inline size_t smem_bwd_fused(int D) { return (size_t)((((BF_ROWS + 32) * (3 * D + 2) + D * (D + 2) + 32 + 3) & ~3) + 4 * 6 * 64) * sizeof(float); }
static inline bool wide_layer(int D) { return D >= 256; }
static const size_t SMEM_P1 = tile_smem<GT_BM, GT_BN, P1_BK, false, false>() + GT_BM * sizeof(int);
// k_gru_p2 / k_gru_bwd_a (32 x 32 tiles over K = D): 4 waves and 128-deep chunks; where the launch leaves CUs idle and K is longer than
// two such chunks, 8 waves (two wave groups that split every chunk's k range) and 256-deep chunks -- one workgroup per CU either way, half
// the memory round trips and half the MFMA chain per tile.  Measured (round 5, us): B = 240, D = 512: k_gru_p2 9.7 -> 8.2, k_gru_bwd_a
// 7.3 -> 6.2; B = 512, D = 256: 6.7 -> 6.4 / 4.5 -> 4.35 (left on the 4-wave form); 8 waves x 128 (9.2) and, for k_gru_bwd_a, 8 waves x
// 512 = the whole K in one chunk (6.4) were no better.  G4R_P2_GEO / G4R_BA_GEO = 0 / 1 override (tests).
static constexpr auto k_gru_p2_w4 = k_gru_p2<GT_NTH, GT_BK>;
static constexpr auto k_gru_p2_w8d = k_gru_p2<512, 256>;
static const size_t SMEM_P2_256 = tile_smem<GT_BM, GT_BN, 256, false, false>() + GT_BM * sizeof(int);
static constexpr auto k_gru_bwd_a_w4 = k_gru_bwd_a<GT_NTH, GT_BK>;
static constexpr auto k_gru_bwd_a_w8d = k_gru_bwd_a<512, 256>;
static const size_t SMEM_BA_256 = tile_smem<GT_BM, GT_BN, 256, false, true>();
static const size_t SMEM_BB = tile_smem<GT_BM, GT_BN, BB_BK, false, true>() + GT_BM * sizeof(int);
static constexpr auto k_score_fwd_k128 = k_score_fwd<GT_BN, GT_BK>;
// long score rows: 64-deep K chunks (more resident workgroups).  Measured at B = 512, N = 8704, D = 256 (us): 64 x 32 tiles
// with K chunks of 64: 39.2, 64 x 64 / 64: 41.4, 64 x 64 / 128: 42.4, 64 x 64 / 32: 45.9 -- the tile shape is not what bounds it
#define SFW_BN 32
#define SFW_BK 64
static constexpr auto k_score_fwd_k64 = k_score_fwd<SFW_BN, SFW_BK>;
static constexpr auto k_score_fwd_t2 = k_score_fwd<64, 32, T2_BK>;      // gemm_tile2: 64 x 64 tiles, double-buffered T2_BK-deep chunks
static const size_t SMEM_SF2 = (size_t)Tile2Cfg<T2_BK>::SMEM_FLOATS * sizeof(float);
static constexpr auto k_score_fwd_t3 = k_score_fwd<64, 32, 3>;          // gemm_tile3: the same tile fed by LDS-DMA through a ring of stages
static const size_t SMEM_SF3 = (size_t)Tile3Cfg<T3_NST, T3_BKS>::SMEM_FLOATS * sizeof(float);
static const size_t SMEM_BMT = std::max((size_t)BMT_NST_A * BMT_STAGE_A * sizeof(float), (size_t)BMT_NST_B * BMT_STAGE_B * sizeof(float) + 2048 * sizeof(int));
static const size_t SMEM_SF64 = tile_smem<SF_BM, SFW_BN, SFW_BK, false, true>() + SFW_BN * sizeof(int);
static constexpr auto k_score_bwd_n = k_score_bwd<32, GT_BK>;
static constexpr auto k_score_bwd_w = k_score_bwd<64, 64>;
static const size_t SMEM_SBW = std::max(tile_smem<64, 64, 64, true, false>(), tile_smem<64, 64, 64, false, false>());
#define ZROW_FLOATS 8192      // DevModel::zrow: an LDS-DMA tile walks K floats along it
#define G4R_DEFER_SLOTS 16    // ring slots of the step planes = steps of a deferral window (= G4R_GRAPH_STEPS; a power of two)
static_assert(G4R_OWN_SLOTS == G4R_DEFER_SLOTS, "the windows of g4r_train_steps serve the deferral ring and the owner ring alike");
static const size_t SMEM_SF = tile_smem<SF_BM, GT_BN, GT_BK, false, true>() + GT_BN * sizeof(int);
static constexpr auto k_score_mt_4s = k_score_mt<4, true>;       // W = 272: B = 512, N = 8704 on 256 CUs
static const size_t SMEM_MT_4S = (size_t)MtCfg<4, true>::SMEM_FLOATS * sizeof(float);
static const size_t SMEM_T2K = (size_t)(4 * 64 * 16) * sizeof(float);                               // gemm_tile2k: two 16-deep buffers per operand
static const size_t SMEM_T3 = (size_t)Tile3Cfg<3, 32>::SMEM_FLOATS * sizeof(float);                 // gemm_tile3: ring of three 32-deep stages

// ---- the instantiations of the step's templated kernels, as tables: the launch picks its entry from m->kern, g4r_create walks them for
// the LDS opt-in.  (hipcc emits device code only for the explicit instantiations of the .cuh files: an entry needs one there.)
// k_loss_rows<long row, spec, columns per thread>: [0] short rows, one column per thread; [1] short rows, four; [2] long rows (always four)
static constexpr decltype(&k_loss_rows<false, 0, 1>) K_LOSS_ROWS[3][4] = {
    {k_loss_rows<false, 0, 1>, k_loss_rows<false, 1, 1>, k_loss_rows<false, 2, 1>, k_loss_rows<false, 3, 1>},
    {k_loss_rows<false, 0, 4>, k_loss_rows<false, 1, 4>, k_loss_rows<false, 2, 4>, k_loss_rows<false, 3, 4>},
    {k_loss_rows<true, 0, 4>, k_loss_rows<true, 1, 4>, k_loss_rows<true, 2, 4>, k_loss_rows<true, 3, 4>}};
static inline auto loss_rows_kernel(const StepKernels& k) { return K_LOSS_ROWS[k.loss_long ? 2 : (k.loss_quads ? 1 : 0)][k.loss_spec]; }
// [chunks 1 / 2 / 4][momentum]; k_update holds at most two chunks per lane
static inline int chunk_index(int chunks) { return chunks == 1 ? 0 : (chunks == 2 ? 1 : 2); }
static constexpr decltype(&k_sparse_update<1, false>) K_SPARSE_UPDATE[3][2] = {
    {k_sparse_update<1, false>, k_sparse_update<1, true>}, {k_sparse_update<2, false>, k_sparse_update<2, true>}, {k_sparse_update<4, false>, k_sparse_update<4, true>}};
static constexpr decltype(&k_sparse_update_generic<1>) K_SPARSE_UPDATE_GENERIC[3] = {k_sparse_update_generic<1>, k_sparse_update_generic<2>, k_sparse_update_generic<4>};
static constexpr decltype(&k_update<1, 32, false>) K_UPDATE[2][2] = {{k_update<1, 32, false>, k_update<1, 32, true>}, {k_update<2, 32, false>, k_update<2, 32, true>}};

// the dense-gradient tiles of the model's GRU weights, TR x TC each (k_dense_grad: 32 x 32, k_dense_grad2: 64 x 64, k_update_l: 16 x 64)
static std::vector<DenseTile> dense_tiles(const DevModel& d, int TR, int TC) {
    std::vector<DenseTile> tiles;
    for (int l = 0; l < d.n_layers; ++l) {
        const int D = d.D[l], IN = d.IN[l];
        auto add = [&](const float* x0, const float* x1, int ldx, int nrows, int ncols, int coff, int ldo, long long base) {
            for (int r = 0; r < nrows; r += TR)
                for (int c = 0; c < ncols; c += TC) {
                    DenseTile t;
                    t.X0 = x0; t.X1 = x1; t.dV = d.dV[l]; t.base = base; t.ldx = ldx; t.ldv = 3 * D; t.nrows = nrows;
                    t.ncols = ncols; t.coff = coff; t.ldo = ldo; t.r0 = r; t.c0 = c; t.gather = (x0 == nullptr && nrows > 1) ? 1 : 0; t.pad = 0;
                    tiles.push_back(t);
                }
        };
        const float* yin = (l == 0) ? nullptr : d.hd[l - 1];     // layer 0: gathered in the kernel (a one-hot input has IN = 0: no tiles)
        add(yin, yin, IN, IN, 3 * D, 0, 3 * D, d.offWx[l]);                   // dWx  = yin^T dV
        add(d.Hr[l], d.Hr[l], D, D, D, 0, D, d.offWh[l]);                     // dWh  = (H r)^T dV[:, :D]
        add(d.H[l][0], d.H[l][1], D, D, 2 * D, D, 2 * D, d.offWrz[l]);        // dWrz = H^T dV[:, D:]
        add(nullptr, nullptr, 0, 1, 3 * D, 0, 3 * D, d.offBh[l]);             // dBh  = colsum(dV) (nrows == 1: the column-sum role)
    }
    return tiles;
}

// Which kernel runs each stage of the training step, from the shapes in `d` (d.touched included), the CU count and the switches: every
// precedence rule written once, for step_head / step_tail, the memory plan of g4r_create, the prediction GRU and the debug keys.
static StepKernels choose_kernels(const DevModel& d, int n_cu, const KernelSwitches& sw, bool defer_on) {
    StepKernels k = {};
    const int L = d.n_layers, B = d.B, top = L - 1;
    const bool onehot = d.embed_mode == G4R_EMBED_ONEHOT;
    auto deep = [&](int forced, int D) { return forced >= 0 ? forced != 0 : (D >= 384 && cdiv(D, GT_BN) * cdiv(B, GT_BM) <= n_cu); };
    // Wide layers: the K-sliced kernels of g4r_wide_kernels.cuh.  G4R_WIDE2 is a bit mask -- 1 k_gru_p1s + k_gru_gate, 8 k_gru_bwd_bw,
    // 16 k_dense_grad2; 0 = the round-1 kernels -- default: the policy below, from the A/B runs of round 5 (profiles/r05_experiments.md):
    //   16  the 64 x 64 dense-gradient tiles as a launch of their own where the dense gradients outweigh the sparse rows
    //       (6 D >= 2 B + n_sample: BASELINE configs[2] yes -- k_update 24.4 us as one launch, 17.7 + 7.5 as two; configs[3] shape no --
    //       20.6 merged, 20.3 + 13.4 apart: there the merged launch runs its two roles side by side)
    //    8  dy as K-slice partial sums wherever a consumer adds them up: the lower layer's k_gru_bwd_pre (any layer above an unfused
    //       one); for layer 0 the row-finishing workgroups of k_dense_grad2 (17.5 -> 7.0 us at configs[2]) or, with the merged k_update,
    //       k_finish_rows as a small launch in front of it (configs[3] shape: 10.8 -> 5.0 + 4.2 us, step 170.3 -> 167.7)
    //    1  phase 1 as partial sums + k_gru_gate from D = 512 on (25.0 -> 18.3 + 4.5 us at configs[2]; D = 256: 13.9 -> 12.9 + 4.3, off)
    // K-slice lengths for A/B runs: G4R_P1_KS (<= 128), G4R_BB_KS.
    int dmax = 0;
    for (int l = 0; l < L; ++l) dmax = std::max(dmax, d.D[l]);
    const bool automask = sw.wide2 < 0;
    const int mask = automask ? (1 | 8 | (6 * dmax >= d.R ? 16 : 0)) : sw.wide2;
    k.wide_dense = (mask & 16) && wide_layer(dmax) && !onehot;
    for (int l = 0; l < L; ++l) {
        const int D = d.D[l], IN = d.IN[l];
        const bool onehot0 = l == 0 && onehot;      // (no input rows: layer 0 reads rows of Wx[0])
        // narrow layers: the lean launches, in and D up to LN_MAXD.  Else (G4R_NO_LEAN=1) the fused kernels of round 2 where their LDS
        // plans hold the operands (k_gru_fwd_fused: load maps of 112 rows / columns; k_gru_bwd_fused: D up to BF_MAXD)
        const bool lean = !sw.no_lean && D <= LN_MAXD && IN <= LN_MAXD && D % 4 == 0 && IN % 4 == 0 && IN >= 4 && !onehot0;
        const bool ffwd = D <= FF_LDR && IN <= FF_LDR && D % 4 == 0 && IN % 4 == 0 && IN >= 4 && !onehot0 &&
                          (size_t)fwd_fused_lds(IN, D).total * sizeof(float) <= 156 * 1024;
        const bool fbwd = D <= BF_MAXD && D % 4 == 0 && IN % 4 == 0 && !onehot0;
        WideGeo& G = k.wg[l];
        G = WideGeo();
        if (wide_layer(D) && D % 64 == 0 && IN % 16 == 0 && IN >= 64 && !onehot0) {
            // phase 1: slices of <= 128 units (all in flight at once: gemm_tile2k_full); k_gru_gate adds <= 8 input / <= 16 slices in all
            if ((mask & 1) && (!automask || D >= 512)) {
                const int ks = std::min(128, std::max(16, sw.p1_ks / 16 * 16));
                G.ny = cdiv(IN, ks); G.kys = ((cdiv(IN, G.ny) + 15) / 16) * 16; G.ny = cdiv(IN, G.kys);
                G.nh = cdiv(D, ks); G.khs = ((cdiv(D, G.nh) + 15) / 16) * 16; G.nh = cdiv(D, G.khs);
                if (G.ny <= 8 && G.ny + G.nh <= 16) G.use |= 1;
            }
            // dy: enough slices of >= 128 (multiples of 32) for a workgroup per CU, <= 16 (what a consumer adds up in one round trip)
            const bool consumer = l == 0 || k.bwd[l - 1] != BWD_FUSED;
            if ((mask & 8) && consumer) {
                const int K = 3 * D, tiles = cdiv(IN, 64) * cdiv(B, 64);
                const int n = std::min(std::max(1, cdiv(n_cu, std::max(tiles, 1))), std::max(1, K / 128));
                int ks = ((cdiv(K, n) + 31) / 32) * 32;
                if (sw.bb_ks > 0) ks = std::max(32, sw.bb_ks / 32 * 32);
                if (cdiv(K, ks) <= 16) { G.use |= 8; G.bbk = ks; G.bbn = cdiv(K, ks); }
            }
        }
        k.fwd[l] = lean ? FWD_LEAN : ffwd ? FWD_FUSED : (G.use & 1) ? FWD_P1S : wide_layer(D) ? FWD_P1_N64 : FWD_P1_N32;
        k.bwd[l] = lean ? BWD_LEAN : fbwd ? BWD_FUSED : onehot0 ? BWD_ONEHOT : (G.use & 8) ? BWD_BW : BWD_B;
        k.p2_deep[l] = deep(sw.p2_geo, D);
        k.ba_deep[l] = deep(sw.ba_geo, D);
    }
    // `wide`: long score rows / big batches; D a multiple of 64 from B = 192, N = 2048 on (B = 240, N = 2288, D = 512: 22.2 vs 25.1 us)
    const int Dt = d.Dtop;
    const bool wide = (B >= 256 && d.ldSc >= 4096) || (Dt % 64 == 0 && B >= 192 && d.ldSc >= 2048);
    // LDS-DMA tiles (k_score_fwd_t3), D a multiple of 32: `wide`, and a wide top layer whenever the batch fills 64-row tiles -- fewer tiles than
    // the chip holds, only the ring's depth hides a stage's round trip (B = 240, N = 2288, D = 512: 18.7 -> 15.0 us)
    const bool dma = Dt % 32 == 0 && (wide || (Dt >= 256 && B >= 64 && d.ldSc >= 1024));
    // k_score_mt: <= n_cu tiles of 64 rows x W = 272 columns filling >= 7/8 of the CUs.  Its two-stage pipeline needs an even number of
    // 16-deep chunks: D a multiple of 32, at least 32.  G4R_NO_MT=1: off.
    bool mt = false;
    if (!sw.no_mt && dma && Dt % 32 == 0 && Dt >= 32 && n_cu / cdiv(B, 64) >= 1) {
        const int nrb = cdiv(B, 64), W = 16 * cdiv(d.ldSc, 16 * (n_cu / nrb));
        mt = W == 272 && nrb * cdiv(d.ldSc, W) * 8 >= n_cu * 7;
    }
    // k_score_s / k_score_b (register-fed 32 x 32 tiles): narrow top layers where k_score_fwd's LDS-staged tiles ran; k_score_b to B = 128
    const bool lean_s = !sw.no_lean && Dt <= LN_MAXD && Dt % 4 == 0 && !wide && !dma && B < 65536 && d.ldSc < 65536;
    k.score_fwd = lean_s ? SF_LEAN : mt ? SF_MT : dma ? SF_T3 : (wide && Dt % T2_BK == 0) ? SF_T2 : wide ? SF_K64 : SF_K128;
    // the (final activation, loss) pairs of BASELINE's configurations run compile-time specialised builds of the row-loss kernel
    k.loss_spec = (d.final_act == G4R_ACT_ELU && d.loss == G4R_LOSS_BPR_MAX) ? 1 : (d.final_act == G4R_ACT_SOFTMAX && d.loss == G4R_LOSS_XE) ? 2
                : (d.final_act == G4R_ACT_ELU && d.loss == G4R_LOSS_TOP1_MAX) ? 3 : 0;
    k.loss_long = (size_t)(2 * d.ldSc + 18 * LOSS_NW) * sizeof(float) > (size_t)(156 * 1024);      // one row copy in LDS, the other in the score row itself
    // four columns per thread and trip from 4 columns per thread on (B = 512, 8192 negatives: 15.2 -> 13.0 us; 2176 columns: no difference)
    k.loss_quads = d.ldSc >= 4 * LOSS_T;
    // Scoring backward: k_score_b, else k_score_bmt, else k_score_bwd2 (`wide`, D a multiple of 64), else k_score_bwd_w / _n.  k_score_bmt:
    // role A 272 x 32 tiles, role B 64 x 128 tiles x `ks` slabs, as many of each, two per CU.  It needs D a multiple of 128 up to 512, 272 /
    // (D / 32) bias columns per tile (four threads each), slabs of a multiple of 32 columns up to 2048, and the top layer's k_gru_bwd_a
    // (it carries the item rows' Adagrad rule).  G4R_NO_BMT=1: off.
    const bool bwd2 = wide && Dt % 64 == 0;
    const bool top_tiles = k.bwd[top] != BWD_LEAN && k.bwd[top] != BWD_FUSED;
    if (!sw.no_bmt && bwd2 && top_tiles && Dt % 128 == 0 && Dt <= 512 && d.ldSc % BMT_WA == 0 && d.ldSc <= 0xFFFF && B <= 0xFFFF) {
        const int ntA = d.ldSc / BMT_WA * (Dt / 32), den = cdiv(B, 64) * (Dt / 128), ks = ntA / den;
        if (ntA % den == 0 && ntA % 8 == 0 && ntA <= n_cu && ntA * 8 >= n_cu * 7 && BMT_WA % (Dt / 32) == 0 && 4 * (BMT_WA / (Dt / 32)) <= 256 &&
            ks >= 2 && ks <= 24 && d.ldSc % ks == 0 && (d.ldSc / ks) % 32 == 0 && d.ldSc / ks <= 2048)
            k.bmt_slabs = ks;
    }
    k.score_bwd = (lean_s && B <= 128) ? SB_LEAN : k.bmt_slabs ? SB_BMT : bwd2 ? SB_BWD2 : wide ? SB_W : SB_N;
    // k_score_b's role A (dSy, dSBy, the item rows' Adagrad pieces: nothing before the update reads them) rides in the top layer's k_gru_dy
    // launch, which leaves most CUs idle, instead of doubling the grid of the step's longest launch (profiles/r08_experiments.md)
    k.score_a_host = (sw.score_b_split && k.score_bwd == SB_LEAN && k.bwd[top] == BWD_LEAN) ? 1 : 0;
    // its slabs: ~17; half as many, twice as deep where k_gru_bwd_fused / k_gru_da sum them next to everything else they load
    const int slabs_target = top_tiles ? 17 : 9;
    k.kch = GT_BK * std::max(1, (cdiv(d.ldSc, GT_BK) + slabs_target / 2) / slabs_target);
    if (k.score_bwd == SB_LEAN) k.kch = 128;      // k_score_b: slabs of 128 score columns (eight waves x 16)
    else if (k.score_bwd == SB_BMT) k.kch = d.ldSc / k.bmt_slabs;      // as many role-B as role-A tiles
    else if (k.score_bwd == SB_BWD2) {
        // k_score_bwd2's tiles are all resident at once: take the slab count (12..24) whose role A + B tiles fill whole rounds of CUs best
        // (B = 512, N = 8704, D = 256: 17 slabs = 1088 tiles 64.2 us, 15 slabs = 1024 tiles 60.6 us); depth: 16-byte aligned rows
        const int ndt = Dt / 64, nrt = cdiv(B, 64), nA = cdiv(d.ldSc, 64) * ndt;
        double best = 2.0;
        for (int ks = 12; ks <= 24; ++ks) {
            const int kch = (cdiv(d.ldSc, ks) + 7) & ~7;
            if (cdiv(d.ldSc, kch) != ks) continue;
            const double rounds = (double)(nA + ks * nrt * ndt) / n_cu;
            const double waste = (std::ceil(rounds) - rounds) / std::ceil(rounds) + 1e-3 * std::abs(ks - 17);
            if (waste < best) { best = waste; k.kch = kch; }
        }
    }
    k.ksplit = cdiv(d.ldSc, k.kch);
    const int TB = wide ? 64 : 32;      // tile edge of k_score_bwd
    k.ndtA = cdiv(Dt + 1, TB); k.nblkA = cdiv(d.ldSc, TB) * k.ndtA;
    k.ndtB = cdiv(Dt, TB); k.nrtB = cdiv(B, TB); k.nblkB = k.ksplit * k.nrtB * k.ndtB;
    // Update: dense-gradient tiles and sparse rows in ONE launch (k_update) on the Adagrad path, item rows of <= 512 floats (its registers
    // hold two chunks per lane), no k_dense_grad2.  k_update_l: one GPU, B <= 128, rows of <= 256 floats, no deferral, no exact replicas,
    // no touched-row bitmap, layer 0's dy not in partial sums.
    const int w = std::max(Dt, d.Ein);
    k.chunks = w <= 256 ? 1 : (w <= 512 ? 2 : 4);
    const bool dy0_parts = (k.wg[0].use & 8) != 0;
    const bool merged = !d.generic && !sw.no_merge && k.chunks <= 2 && !k.wide_dense;
    const bool lean_u = !sw.no_lean && sw.allow_lean_update && merged && d.apply_dense_inplace && B <= 128 && k.chunks == 1 && !defer_on && d.xmode == 0 &&
                        !d.touched && !dy0_parts && d.R < 65536 && cdiv(d.R, 8) < 65536 && dense_tiles(d, 16, 64).size() < 65536;
    k.update = lean_u ? UP_LEAN : merged ? UP_MERGED : UP_SPLIT;
    k.finish_rows = dy0_parts && !k.wide_dense;      // (k_dense_grad2 finishes the rows in workgroups of its own)
    return k;
}
// publish the host descriptor to the device copy (stream-ordered; pageable source is staged before return)
static int sync_dm(g4r_model* m) {
    HIPCHK(hipMemcpyAsync(m->d_dm, &m->dm, sizeof(DevModel), hipMemcpyHostToDevice, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    return 0;
}

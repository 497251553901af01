// g4r_host_predict.hpp -- part of libgru4rec_hip.so's host code; included once, by g4r_api.hip (one translation unit: the kernels are templates
// instantiated there).  Holds: the prediction state and what steps it: g4r_predict_*, g4r_rank_targets, g4r_recommend_step(_filtered, _scan),
// g4r_evaluate; the forward GRU step and the scoring every inference entry shares.
// ------------------------------------------------------------------------------------------------ prediction
int g4r_predict_begin(g4r_model* m, int32_t batch) {
    if (!m || batch < 1) return fail("bad batch");
    HIPCHK(hipSetDevice(m->cfg.device));
    HIPCHK(hipStreamSynchronize(m->stream));
    DevModel& d = m->dm;
    if (batch != m->pbatch) {
        for (int l = 0; l < d.n_layers; ++l) {
            dfree(m, m->pH[l][0]); dfree(m, m->pH[l][1]); dfree(m, m->phout[l]);
            dfree(m, m->pVc[l]); dfree(m, m->pz[l]); dfree(m, m->pHr[l]);
            if (dalloc(m, &m->pVc[l], (size_t)batch * d.D[l]) || dalloc(m, &m->pz[l], (size_t)batch * d.D[l]) ||
                dalloc(m, &m->pHr[l], (size_t)batch * d.D[l]))
                return -1;
            if (dalloc(m, &m->pH[l][0], (size_t)batch * d.D[l]) || dalloc(m, &m->pH[l][1], (size_t)batch * d.D[l]) ||
                dalloc(m, &m->phout[l], (size_t)batch * d.D[l]))
                return -1;
        }
        dfree(m, m->p_in); dfree(m, m->p_tgt); dfree(m, m->p_keep); dfree(m, m->p_zero); dfree(m, m->p_ranks); dfree(m, m->p_cnt);
        if (dalloc(m, &m->p_in, batch) || dalloc(m, &m->p_tgt, batch) || dalloc(m, &m->p_keep, batch) ||
            dalloc(m, &m->p_zero, batch) || dalloc(m, &m->p_ranks, batch) || dalloc(m, &m->p_cnt, 2 * (size_t)batch))
            return -1;
        m->pbatch = batch;
    } else {
        for (int l = 0; l < d.n_layers; ++l)
            for (int q = 0; q < 2; ++q) HIPCHK(hipMemsetAsync(m->pH[l][q], 0, (size_t)batch * d.D[l] * sizeof(float), m->stream));
    }
    m->ppar = 0;
    m->tie_ctr = 0;
    HIPCHK(hipStreamSynchronize(m->stream));
    return 0;
}

// the hidden rows [0, rows) of the prediction state whose byte in d_mask is set start from zero
static void state_zero_rows(g4r_model* m, const unsigned char* d_mask, int rows) {
    const DevModel& d = m->dm;
    for (int l = 0; l < d.n_layers; ++l)
        hipLaunchKernelGGL(k_zero_rows, dim3(cdiv((long long)rows * d.D[l], 256)), dim3(256), 0, m->stream, m->pH[l][m->ppar], d_mask, rows, d.D[l]);
}

// the hidden rows of the prediction state gathered through d_map (row j <- row d_map[j], -1: zero) into the other ping-pong half
static void state_gather_rows(g4r_model* m, const int* d_map, int rows) {
    const DevModel& d = m->dm;
    for (int l = 0; l < d.n_layers; ++l)
        hipLaunchKernelGGL(k_gather_rows, dim3(cdiv((long long)rows * d.D[l], 256)), dim3(256), 0, m->stream, m->pH[l][m->ppar ^ 1],
                           (const float*)m->pH[l][m->ppar], d_map, rows, d.D[l]);
    m->ppar ^= 1;
}

int g4r_predict_hidden(g4r_model* m, const uint8_t* zero_mask, int32_t n_mask, const int32_t* keep_rows, int32_t n_keep) {
    if (!m || !m->pbatch) return fail("g4r_predict_begin first");
    HIPCHK(hipSetDevice(m->cfg.device));
    const int PB = m->pbatch;
    if (zero_mask) {
        if (n_mask < 0 || n_mask > PB) return fail("zero_mask is longer than the prediction batch (g4r_predict_begin)");
        std::vector<unsigned char> zm(PB, 0);      // rows past the mask keep their state
        memcpy(zm.data(), zero_mask, (size_t)n_mask);
        HIPCHK(hipMemcpyAsync(m->p_zero, zm.data(), PB, hipMemcpyHostToDevice, m->stream));
        HIPCHK(hipStreamSynchronize(m->stream));
        state_zero_rows(m, m->p_zero, PB);
    }
    if (keep_rows) {
        if (n_keep < 0 || n_keep > PB) return fail("n_keep out of range");
        std::vector<int> mp(PB, -1);
        for (int j = 0; j < n_keep; ++j) mp[j] = keep_rows[j];
        HIPCHK(hipMemcpyAsync(m->p_keep, mp.data(), PB * sizeof(int), hipMemcpyHostToDevice, m->stream));
        HIPCHK(hipStreamSynchronize(m->stream));
        state_gather_rows(m, m->p_keep, PB);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(m->stream));
    return 0;
}

struct StreamRank;
static int predict_forward(g4r_model* m, const int* d_in_idx, int mrows, const int* d_items, int64_t n_sel, const StreamRank* stream);

// validation and upload shared by g4r_predict_step / g4r_recommend_step: input items -> p_in, candidates -> p_items; *n_sel is
// set to n_items when item_idx is NULL
static int predict_inputs(g4r_model* m, const int32_t* in_idx, int32_t mrows, const int32_t* item_idx, int64_t* n_sel) {
    if (!m || !in_idx) return fail("null argument");
    if (!m->pbatch) return fail("g4r_predict_begin first");
    if (mrows < 1 || mrows > m->pbatch) return fail("mrows out of range");
    HIPCHK(hipSetDevice(m->cfg.device));
    const DevModel& d = m->dm;
    if (item_idx && *n_sel < 1) return fail("n_sel must be positive");
    for (int i = 0; i < mrows; ++i)
        if (in_idx[i] < 0 || in_idx[i] >= d.n_items) return fail("input item index out of range");
    HIPCHK(hipMemcpyAsync(m->p_in, in_idx, mrows * sizeof(int), hipMemcpyHostToDevice, m->stream));
    const int* d_items;
    return cand_upload(m, item_idx, n_sel, &d_items);
}

int g4r_predict_step(g4r_model* m, const int32_t* in_idx, int32_t mrows, const int32_t* item_idx, int64_t n_sel,
                     float* out_scores) {
    if (predict_inputs(m, in_idx, mrows, item_idx, &n_sel)) return -1;
    if (predict_forward(m, m->p_in, mrows, item_idx ? (const int*)m->p_items.p : (const int*)nullptr, n_sel, nullptr)) return -1;
    const int64_t ldo = m->p_ldo;
    if (out_scores) {
        HIPCHK(hipMemcpy2DAsync(out_scores, n_sel * sizeof(float), m->p_scores.p, ldo * sizeof(float), n_sel * sizeof(float), mrows,
                                hipMemcpyDeviceToHost, m->stream));
    }
    HIPCHK(hipStreamSynchronize(m->stream));
    return 0;
}

int g4r_rank_targets(g4r_model* m, const int32_t* target_col, int32_t mrows, int64_t col_begin, int32_t mode, float* ranks) {
    if (!m || !target_col || !ranks) return fail("null argument");
    if (!m->p_scores.p || mrows < 1 || mrows > m->pbatch) return fail("no scores / mrows out of range");
    if (mode < 0 || mode > G4R_RANK_TIEBREAKING) return fail("unknown rank mode");
    for (int i = 0; i < mrows; ++i)
        if (target_col[i] < 0 || target_col[i] >= m->p_nsel) return fail("target column out of range");
    HIPCHK(hipSetDevice(m->cfg.device));
    HIPCHK(hipMemcpyAsync(m->p_tgt, target_col, mrows * sizeof(int), hipMemcpyHostToDevice, m->stream));
    hipLaunchKernelGGL(k_rank_rows, dim3(mrows), dim3(256), 0, m->stream, (const float*)m->p_scores.p, (long long)m->p_nsel,
                       (long long)m->p_ldo, (const int*)m->p_tgt, (long long)col_begin, (int)mode, m->p_ranks,
                       (unsigned long long)m->cfg.seed, m->tie_ctr++);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(ranks, m->p_ranks, mrows * sizeof(float), hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    return 0;
}

// the buffers one forward GRU step works on: per layer the hidden ping-pong, the output and the scratch (the prediction state's,
// or the replay's of g4r_recommend_sessions)
struct GruBufs { float* (*H)[2]; float** hout; float** Vc; float** z; float** Hr; };
static GruBufs predict_bufs(g4r_model* m) { return GruBufs{m->pH, m->phout, m->pVc, m->pz, m->pHr}; }
static GruBufs replay_bufs(g4r_model* m) { return GruBufs{m->rH, m->rhout, m->rVc, m->rz, m->rHr}; }

// forward GRU of rows [0, mrows) (input items on the device): every layer reads H[l][par], writes H[l][par ^ 1] and hout[l].  Rows
// from mrows on are neither read nor written: every load of k_gru_p1 / k_gru_p2 is clamped to or masked by row < M, and both
// epilogues return for row >= M (the replay relies on it: a finished row keeps its last state and output)
static void gru_step(g4r_model* m, const GruBufs& b, int par, const int* d_in_idx, int mrows) {
    DevModel& d = m->dm;
    for (int l = 0; l < d.n_layers; ++l) {
        GruFwdPredict pa;
        pa.in_idx = (GP(const int))d_in_idx;
        pa.ysrc = (GP(const float))(l > 0 ? b.hout[l - 1] : nullptr);
        pa.Hcur = (GP(const float))b.H[l][par];
        pa.Hnext = (GP(float))b.H[l][par ^ 1];
        pa.hout = (GP(float))b.hout[l];
        pa.Vc = (GP(float))b.Vc[l]; pa.z = (GP(float))b.z[l]; pa.Hr = (GP(float))b.Hr[l];
        pa.M = mrows;
        if (wide_layer(d.D[l]))
            hipLaunchKernelGGL(k_gru_p1_n64, dim3(cdiv(3 * d.D[l], 64), cdiv(mrows, GT_BM)), dim3(GT_NTH_FEW), SMEM_P1_N64, m->stream,
                               (const DevModel*)m->d_dm, (StepState*)nullptr, l, 0, 0, pa);
        else
            hipLaunchKernelGGL(k_gru_p1_n32, dim3(cdiv(3 * d.D[l], GT_BN), cdiv(mrows, GT_BM)), dim3(GT_NTH_FEW), SMEM_P1, m->stream,
                               (const DevModel*)m->d_dm, (StepState*)nullptr, l, 0, 0, pa);
        {
            const dim3 g2(cdiv(d.D[l], GT_BN), cdiv(mrows, GT_BM));
            // (geometry from the TRAINING batch, not from this call's rows: the fp32 summation order of the hidden state must not depend
            // on the evaluation batch size, nor differ between training and prediction)
            if (m->kern.p2_deep[l])
                hipLaunchKernelGGL(k_gru_p2_w8d, g2, dim3(512), SMEM_P2_256, m->stream, (const DevModel*)m->d_dm, (StepState*)nullptr, l, 0, pa);
            else hipLaunchKernelGGL(k_gru_p2_w4, g2, dim3(GT_NTH), SMEM_NN, m->stream, (const DevModel*)m->d_dm, (StepState*)nullptr, l, 0, pa);
        }
    }
}

// one step of the prediction state: the top layer's output is left in phout[n_layers - 1] (shared by predict_forward /
// g4r_recommend_step)
// Rows from mrows on are not stepped and keep their state: gru_step leaves them untouched in the half it writes, where they are as
// they were two steps ago, so they are carried over from the half it read (a later call with more rows goes on from there)
static int predict_gru(g4r_model* m, const int* d_in_idx, int mrows) {
    const DevModel& d = m->dm;
    gru_step(m, predict_bufs(m), m->ppar, d_in_idx, mrows);
    if (mrows < m->pbatch)
        for (int l = 0; l < d.n_layers; ++l) {
            const size_t o = (size_t)mrows * d.D[l];
            HIPCHK(hipMemcpyAsync(m->pH[l][m->ppar ^ 1] + o, m->pH[l][m->ppar] + o, (size_t)(m->pbatch - mrows) * d.D[l] * sizeof(float),
                                  hipMemcpyDeviceToDevice, m->stream));
        }
    m->ppar ^= 1;
    return 0;
}

// scores of rows [0, mrows) of hsrc against the candidates -> out (row stride ldo), final activation applied (softmax per row)
static void score_rows(g4r_model* m, const float* hsrc, int mrows, const int* d_items, int64_t n_sel, float* out, int64_t ldo) {
    const bool sm = is_softmax(m->dm);
    hipLaunchKernelGGL(k_score_store, dim3(cdiv(n_sel, 32), cdiv(mrows, SC_BM)), dim3(256), m->smem_score, m->stream, (const DevModel*)m->d_dm,
                       hsrc, (int)mrows, d_items, (long long)n_sel, out, (long long)ldo, sm ? 0 : 1, (int*)nullptr, 0LL, (const int*)nullptr, 0u);
    if (sm) hipLaunchKernelGGL(k_softmax_rows, dim3(mrows), dim3(256), 0, m->stream, out, (long long)n_sel, (long long)ldo);
}

// forward GRU + scores of `mrows` rows whose input items sit on the device (shared by g4r_predict_step / g4r_evaluate)
// stream = nullptr: scores of all candidates go to p_scores (final activation applied).  Otherwise (evaluation with an
// element-wise final activation) nothing is materialised: stream->tgt lists the target item of every row; their scores are
// computed first (mrows x mrows tile, diagonal used), then every candidate tile is compared with them on the fly and
// p_ranks receives the ranks (stream->mode, candidates from column stream->col_begin on).
struct StreamRank { const int* tgt; long long col_begin; int mode; const int* tie_col; unsigned tie_ctr; };
static int predict_forward(g4r_model* m, const int* d_in_idx, int mrows, const int* d_items, int64_t n_sel, const StreamRank* stream) {
    DevModel& d = m->dm;
    const int64_t ldo = stream ? ((mrows + 3) & ~3) : ((n_sel + 3) & ~3LL);
    const int64_t need = stream ? (int64_t)m->pbatch * ((m->pbatch + 3) & ~3) : (int64_t)m->pbatch * ldo;
    if (m->p_scores.reserve(m, need)) return -1;
    if (predict_gru(m, d_in_idx, mrows)) return -1;
    const bool sm = is_softmax(d);
    const float* hsrc = (const float*)m->phout[d.n_layers - 1];
    if (stream) {
        if (sm) return fail("internal: streaming ranks need an element-wise final activation");
        hipLaunchKernelGGL(k_score_store, dim3(cdiv(mrows, 32), cdiv(mrows, SC_BM)), dim3(256), m->smem_score, m->stream, (const DevModel*)m->d_dm,
                           hsrc, (int)mrows, stream->tgt, (long long)mrows, m->p_scores.p, (long long)ldo, 1, (int*)nullptr, 0LL, (const int*)nullptr, 0u);
        hipLaunchKernelGGL(k_score_count, dim3(cdiv(n_sel, 32), cdiv(mrows, SC_BM)), dim3(256), m->smem_score, m->stream, (const DevModel*)m->d_dm,
                           hsrc, (int)mrows, d_items, (long long)n_sel, m->p_scores.p, (long long)ldo, 1, m->p_cnt, stream->col_begin,
                           stream->mode == G4R_RANK_TIEBREAKING ? stream->tie_col : (const int*)nullptr, stream->tie_ctr);
        hipLaunchKernelGGL(k_rank_counts, dim3(cdiv(mrows, 256)), dim3(256), 0, m->stream, m->p_cnt, (int)mrows, stream->mode, m->p_ranks);
        HIPCHK(hipGetLastError());
        m->p_nsel = 0; m->p_ldo = ldo;        // no score matrix to read back
        return 0;
    }
    score_rows(m, hsrc, mrows, d_items, n_sel, m->p_scores.p, ldo);
    HIPCHK(hipGetLastError());
    m->p_nsel = n_sel; m->p_ldo = ldo;
    return 0;
}

// GRU step + selection of a checked call whose inputs predict_inputs has uploaded; ex (device exclusions) NULL: the unfiltered kernels
// scan_c > 0: the two-stage selection with scan_c candidates per row (scan_check has refused softmax)
static int recommend_run(g4r_model* m, int32_t mrows, const int32_t* item_idx, int64_t n_sel, int32_t k, const TkExcl* ex,
                         int32_t* out_cols, float* out_scores, int32_t scan_c = 0) {
    DevModel& d = m->dm;
    const int* d_items = item_idx ? (const int*)m->p_items.p : (const int*)nullptr;
    const bool sm = is_softmax(d);
    // softmax needs the whole row first: the scores are materialised exactly as g4r_predict_step materialises them, then selected;
    // an element-wise final activation is selected as the tiles are scored (nothing stored)
    if (sm) {
        if (predict_forward(m, m->p_in, mrows, d_items, n_sel, nullptr)) return -1;
    } else {
        if (predict_gru(m, m->p_in, mrows)) return -1;
    }
    if (scan_c > 0) {
        if (topk_select_scan(m, (const float*)m->phout[d.n_layers - 1], mrows, d_items, n_sel, k, scan_c, ex)) return -1;
    } else if (topk_select(m, (const float*)m->phout[d.n_layers - 1], mrows, d_items, n_sel, k, ex, (const float*)m->p_scores.p, m->p_ldo)) return -1;
    const int64_t nout = (int64_t)mrows * k;
    HIPCHK(hipMemcpyAsync(out_cols, m->p_tcols.p, nout * sizeof(int), hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipMemcpyAsync(out_scores, m->p_tscores.p, nout * sizeof(float), hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    return 0;
}

// The three stateful entries.  oversample 0: the exact selection; otherwise the two-stage one, scan_check's refusals after
// recommend_check's.  predict_inputs only uploads: the state advances in recommend_run, after every check.  The exclusion lists
// are checked, sorted and de-duplicated (excl_pack) and uploaded where there are any
static int recommend_step_run(g4r_model* m, const int32_t* in_idx, int32_t mrows, const int32_t* item_idx, int64_t n_sel, int32_t k,
                              int32_t oversample, const int64_t* excl_offs, const int32_t* excl_items, const uint32_t* excl_mask,
                              int32_t* out_cols, float* out_scores) {
    int32_t c = 0;
    if (recommend_check(m, item_idx, n_sel, k, out_cols, out_scores)) return -1;
    if (oversample && scan_check(m, item_idx, n_sel, k, oversample, &c)) return -1;
    if (predict_inputs(m, in_idx, mrows, item_idx, &n_sel)) return -1;
    if (!excl_offs && !excl_mask) return recommend_run(m, mrows, item_idx, n_sel, k, nullptr, out_cols, out_scores, c);
    std::vector<long long> offs;
    std::vector<int32_t> items;
    if (excl_pack(m, mrows, item_idx, n_sel, k, excl_offs, excl_items, excl_mask, offs, items)) return -1;
    TkExcl ex;
    if (excl_upload(m, excl_offs != nullptr, offs, items, excl_mask, &ex)) return -1;
    return recommend_run(m, mrows, item_idx, n_sel, k, &ex, out_cols, out_scores, c);
}

int g4r_recommend_step(g4r_model* m, const int32_t* in_idx, int32_t mrows, const int32_t* item_idx, int64_t n_sel,
                       int32_t k, int32_t* out_cols, float* out_scores) {
    return recommend_step_run(m, in_idx, mrows, item_idx, n_sel, k, 0, nullptr, nullptr, nullptr, out_cols, out_scores);
}

int g4r_recommend_step_filtered(g4r_model* m, const int32_t* in_idx, int32_t mrows, const int32_t* item_idx, int64_t n_sel,
                                int32_t k, const int64_t* excl_offs, const int32_t* excl_items, const uint32_t* excl_mask,
                                int32_t* out_cols, float* out_scores) {
    return recommend_step_run(m, in_idx, mrows, item_idx, n_sel, k, 0, excl_offs, excl_items, excl_mask, out_cols, out_scores);
}

// (an oversample below 1 goes on as -1: scan_check refuses it in its turn; it is not taken for the exact selection)
int g4r_recommend_step_scan(g4r_model* m, const int32_t* in_idx, int32_t mrows, const int32_t* item_idx, int64_t n_sel, int32_t k,
                            int32_t oversample, const int64_t* excl_offs, const int32_t* excl_items, const uint32_t* excl_mask,
                            int32_t* out_cols, float* out_scores) {
    return recommend_step_run(m, in_idx, mrows, item_idx, n_sel, k, oversample < 1 ? -1 : oversample, excl_offs, excl_items, excl_mask,
                              out_cols, out_scores);
}

// ------------------------------------------------------------------------------------------------ evaluation over a plan
// the checks of a plan that g4r_evaluate and g4r_recommend_events share, in three parts because the two entries refuse in different
// orders (g4r_recommend_events checks k between the first and the other two, and every step's row count before the indices;
// g4r_evaluate the indices first): the rank mode and the compaction arrays,
static int plan_mode_check(int32_t mode, const int64_t* compact_steps, const int32_t* compact_maps, int64_t n_compact) {
    if (mode < 0 || mode > G4R_RANK_TIEBREAKING) return fail("unknown rank mode");
    if (n_compact > 0 && (!compact_steps || !compact_maps)) return fail("compaction arrays missing");
    return 0;
}

// every step's row count,
static int plan_rows_check(const int32_t* M, int64_t T, int B) {
    for (int64_t t = 0; t < T; ++t)
        if (M[t] < 1 || M[t] > B) return fail("plan M out of range");
    return 0;
}

// the item indices of the plan and of the candidates
static int plan_index_check(const DevModel& d, const int32_t* in_idx, const int32_t* out_idx, int64_t T, int B, const int32_t* items,
                            int64_t n_items_sel) {
    for (int64_t i = 0; i < T * B; ++i)
        if (in_idx[i] < 0 || in_idx[i] >= d.n_items || out_idx[i] < 0 || out_idx[i] >= d.n_items) return fail("plan item index out of range");
    for (int64_t i = 0; items && i < n_items_sel; ++i)
        if (items[i] < 0 || items[i] >= d.n_items) return fail("item index out of range");
    return 0;
}

// rows of exhausted slots are dropped before step t (evaluation.py:138; gru4rec.py:647-651 for the same plan format): every
// compaction map due at t (d_maps: [n_compact][B] on the device, *ci the next one) gathers the hidden rows.  Returns the maps applied
static int plan_compact(g4r_model* m, int64_t t, const int64_t* compact_steps, int64_t n_compact, const int* d_maps, int B, int64_t* ci) {
    int n = 0;
    for (; *ci < n_compact && compact_steps[*ci] == t; ++*ci, ++n) state_gather_rows(m, d_maps + *ci * B, B);
    return n;
}

int g4r_evaluate(g4r_model* m, const int32_t* in_idx, const int32_t* out_idx, const uint8_t* reset, const int32_t* M, int64_t T,
                 int32_t batch, const int64_t* compact_steps, const int32_t* compact_maps, int64_t n_compact,
                 const int32_t* items, int64_t n_items_sel, const int32_t* cutoffs, int32_t n_cut, int32_t mode,
                 double* recall_sum, double* mrr_sum, int64_t* n_events) {
    if (!m || !in_idx || !out_idx || !reset || !M || !cutoffs || !recall_sum || !mrr_sum || !n_events) return fail("null argument");
    if (T < 0 || batch < 1 || n_cut < 1 || n_cut > 64) return fail("bad evaluation sizes");
    if (plan_mode_check(mode, compact_steps, compact_maps, n_compact)) return -1;
    DevModel& d = m->dm;
    const int B = batch;
    if (plan_index_check(d, in_idx, out_idx, T, B, items, n_items_sel) || plan_rows_check(M, T, B)) return -1;
    if (g4r_predict_begin(m, batch)) return -1;            // fresh (zero) hidden state, scratch for `batch` rows
    int *e_in = nullptr, *e_out = nullptr, *e_maps = nullptr, *e_items = nullptr, *e_cand = nullptr, *e_cut = nullptr, *e_iota = nullptr;
    unsigned char* e_reset = nullptr;
    double* e_acc = nullptr;            // [rec(n_cut) | mrr(n_cut)]
    long long* e_n = nullptr;
    const size_t TB = (size_t)std::max<int64_t>(T, 1) * B;
    CallTemps tmp(m);
    if (tmp.get(&e_in, TB, false) || tmp.get(&e_out, TB, false) || tmp.get(&e_reset, TB, false) ||
        tmp.get(&e_maps, (size_t)std::max<int64_t>(n_compact, 1) * B, false) || tmp.get(&e_cut, n_cut, false) ||
        tmp.get(&e_acc, 2 * (size_t)n_cut) || tmp.get(&e_n, 1) || tmp.get(&e_iota, B, false) ||
        (items && (tmp.get(&e_items, (size_t)n_items_sel, false) || tmp.get(&e_cand, (size_t)B + n_items_sel, false))))
        return -1;
    hipStream_t s = m->stream;
    if (T > 0) {
        HIPCHK(hipMemcpyAsync(e_in, in_idx, TB * sizeof(int), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(e_out, out_idx, TB * sizeof(int), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(e_reset, reset, TB, hipMemcpyHostToDevice, s));
    }
    if (n_compact > 0) HIPCHK(hipMemcpyAsync(e_maps, compact_maps, (size_t)n_compact * B * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(e_cut, cutoffs, n_cut * sizeof(int), hipMemcpyHostToDevice, s));
    if (items) HIPCHK(hipMemcpyAsync(e_items, items, (size_t)n_items_sel * sizeof(int), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_iota, dim3(cdiv(B, 256)), dim3(256), 0, s, e_iota, B);
    const bool streaming = !is_softmax(d) && !getenv("G4R_EVAL_MATERIALIZE");
    int64_t ci = 0;
    for (int64_t t = 0; t < T; ++t) {
        const int Mt = M[t];
        plan_compact(m, t, compact_steps, n_compact, e_maps, B, &ci);
        const int* tgt = e_out + t * B;
        const int* cand = nullptr;
        int64_t n_sel = d.n_items;
        if (items) {
            hipLaunchKernelGGL(k_eval_candidates, dim3(cdiv((long long)Mt + n_items_sel, 256)), dim3(256), 0, s, e_cand, tgt, Mt,
                               (const int*)e_items, (long long)n_items_sel);
            cand = e_cand;
            n_sel = Mt + n_items_sel;
        }
        if (streaming) {
            // element-wise final activation: candidate tiles are ranked against the target score as they are produced
            // column of row i's target in the candidate list: i when [targets | items] are scored, the target item otherwise
            const StreamRank sr = {tgt, items ? (long long)Mt : 0LL, (int)mode, items ? (const int*)e_iota : tgt, (unsigned)t};
            if (predict_forward(m, e_in + t * B, Mt, cand, n_sel, &sr)) return -1;
        } else {
            // softmax needs the whole row first (max, sum): scores are materialised, then ranked
            if (predict_forward(m, e_in + t * B, Mt, cand, n_sel, nullptr)) return -1;
            hipLaunchKernelGGL(k_rank_rows, dim3(Mt), dim3(256), 0, s, (const float*)m->p_scores.p, (long long)m->p_nsel, (long long)m->p_ldo,
                               items ? (const int*)e_iota : tgt, items ? (long long)Mt : 0LL, (int)mode, m->p_ranks,
                               (unsigned long long)m->cfg.seed, (unsigned)t);
        }
        hipLaunchKernelGGL(k_eval_accum, dim3(1), dim3(256), 0, s, (const float*)m->p_ranks, Mt, (const int*)e_cut, (int)n_cut, e_acc,
                           e_acc + n_cut, e_n);
        // hidden rows of sessions that ended with this step start from zero (evaluation.py:137)
        state_zero_rows(m, e_reset + t * B, Mt);
    }
    HIPCHK(hipGetLastError());
    std::vector<double> acc(2 * (size_t)n_cut);
    long long n = 0;
    HIPCHK(hipMemcpyAsync(acc.data(), e_acc, acc.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&n, e_n, sizeof(n), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    for (int c = 0; c < n_cut; ++c) { recall_sum[c] = acc[c]; mrr_sum[c] = acc[n_cut + c]; }
    *n_events = n;
    return 0;
}

// g4r_host_predict.hpp -- part of libgru4rec_hip.so's host code; included once, by g4r_api.hip (one translation unit: the kernels are templates
// instantiated there).  Holds: prediction and evaluation: g4r_predict_*, g4r_rank_targets, g4r_recommend_step(_filtered),
// g4r_recommend_sessions, g4r_continue_sessions, g4r_evaluate, g4r_recommend_events.
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

int g4r_predict_hidden(g4r_model* m, const uint8_t* zero_mask, int32_t n_mask, const int32_t* keep_rows, int32_t n_keep) {
    if (!m || !m->pbatch) return fail("g4r_predict_begin first");
    HIPCHK(hipSetDevice(m->cfg.device));
    DevModel& d = m->dm;
    const int PB = m->pbatch;
    if (zero_mask) {
        if (n_mask < 0 || n_mask > PB) return fail("zero_mask is longer than the prediction batch (g4r_predict_begin)");
        std::vector<unsigned char> zm(PB, 0);      // rows past the mask keep their state
        memcpy(zm.data(), zero_mask, (size_t)n_mask);
        HIPCHK(hipMemcpyAsync(m->p_zero, zm.data(), PB, hipMemcpyHostToDevice, m->stream));
        HIPCHK(hipStreamSynchronize(m->stream));
        for (int l = 0; l < d.n_layers; ++l)
            hipLaunchKernelGGL(k_zero_rows, dim3(cdiv((long long)PB * d.D[l], 256)), dim3(256), 0, m->stream, m->pH[l][m->ppar],
                               (const unsigned char*)m->p_zero, PB, d.D[l]);
    }
    if (keep_rows) {
        if (n_keep < 0 || n_keep > PB) return fail("n_keep out of range");
        std::vector<int> mp(PB, -1);
        for (int j = 0; j < n_keep; ++j) mp[j] = keep_rows[j];
        HIPCHK(hipMemcpyAsync(m->p_keep, mp.data(), PB * sizeof(int), hipMemcpyHostToDevice, m->stream));
        HIPCHK(hipStreamSynchronize(m->stream));
        for (int l = 0; l < d.n_layers; ++l)
            hipLaunchKernelGGL(k_gather_rows, dim3(cdiv((long long)PB * d.D[l], 256)), dim3(256), 0, m->stream, m->pH[l][m->ppar ^ 1],
                               (const float*)m->pH[l][m->ppar], (const int*)m->p_keep, PB, d.D[l]);
        m->ppar ^= 1;
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
    DevModel& d = m->dm;
    if (!item_idx) *n_sel = d.n_items;
    if (*n_sel < 1) return fail("n_sel must be positive");
    for (int i = 0; i < mrows; ++i)
        if (in_idx[i] < 0 || in_idx[i] >= d.n_items) return fail("input item index out of range");
    HIPCHK(hipMemcpyAsync(m->p_in, in_idx, mrows * sizeof(int), hipMemcpyHostToDevice, m->stream));
    if (item_idx) {
        if (*n_sel > m->p_items_cap) {
            dfree(m, m->p_items);
            if (dalloc(m, &m->p_items, (size_t)*n_sel, false)) return -1;
            m->p_items_cap = *n_sel;
        }
        for (int64_t i = 0; i < *n_sel; ++i)
            if (item_idx[i] < 0 || item_idx[i] >= d.n_items) return fail("item index out of range");
        HIPCHK(hipMemcpyAsync(m->p_items, item_idx, *n_sel * sizeof(int), hipMemcpyHostToDevice, m->stream));
    }
    return 0;
}

int g4r_predict_step(g4r_model* m, const int32_t* in_idx, int32_t mrows, const int32_t* item_idx, int64_t n_sel,
                     float* out_scores) {
    if (predict_inputs(m, in_idx, mrows, item_idx, &n_sel)) return -1;
    if (predict_forward(m, m->p_in, mrows, item_idx ? (const int*)m->p_items : (const int*)nullptr, n_sel, nullptr)) return -1;
    const int64_t ldo = m->p_ldo;
    if (out_scores) {
        HIPCHK(hipMemcpy2DAsync(out_scores, n_sel * sizeof(float), m->p_scores, ldo * sizeof(float), n_sel * sizeof(float), mrows,
                                hipMemcpyDeviceToHost, m->stream));
    }
    HIPCHK(hipStreamSynchronize(m->stream));
    return 0;
}

int g4r_rank_targets(g4r_model* m, const int32_t* target_col, int32_t mrows, int64_t col_begin, int32_t mode, float* ranks) {
    if (!m || !target_col || !ranks) return fail("null argument");
    if (!m->p_scores || mrows < 1 || mrows > m->pbatch) return fail("no scores / mrows out of range");
    if (mode < 0 || mode > G4R_RANK_TIEBREAKING) return fail("unknown rank mode");
    for (int i = 0; i < mrows; ++i)
        if (target_col[i] < 0 || target_col[i] >= m->p_nsel) return fail("target column out of range");
    HIPCHK(hipSetDevice(m->cfg.device));
    HIPCHK(hipMemcpyAsync(m->p_tgt, target_col, mrows * sizeof(int), hipMemcpyHostToDevice, m->stream));
    hipLaunchKernelGGL(k_rank_rows, dim3(mrows), dim3(256), 0, m->stream, (const float*)m->p_scores, (long long)m->p_nsel,
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
static void predict_gru(g4r_model* m, const int* d_in_idx, int mrows) {
    gru_step(m, predict_bufs(m), m->ppar, d_in_idx, mrows);
    m->ppar ^= 1;
}

// scores of rows [0, mrows) of hsrc against the candidates -> out (row stride ldo), final activation applied (softmax per row)
static void score_rows(g4r_model* m, const float* hsrc, int mrows, const int* d_items, int64_t n_sel, float* out, int64_t ldo) {
    const DevModel& d = m->dm;
    const bool sm = (d.final_act == G4R_ACT_SOFTMAX || d.final_act == G4R_ACT_SOFTMAX_LOGIT);   // gru4rec.py:499-500
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
    if (need > m->p_scores_cap) {
        HIPCHK(hipStreamSynchronize(m->stream));
        dfree(m, m->p_scores);
        if (dalloc(m, &m->p_scores, (size_t)need, false)) return -1;
        m->p_scores_cap = need;
    }
    predict_gru(m, d_in_idx, mrows);
    const bool sm = (d.final_act == G4R_ACT_SOFTMAX || d.final_act == G4R_ACT_SOFTMAX_LOGIT);   // gru4rec.py:499-500
    const float* hsrc = (const float*)m->phout[d.n_layers - 1];
    if (stream) {
        if (sm) return fail("internal: streaming ranks need an element-wise final activation");
        hipLaunchKernelGGL(k_score_store, dim3(cdiv(mrows, 32), cdiv(mrows, SC_BM)), dim3(256), m->smem_score, m->stream, (const DevModel*)m->d_dm,
                           hsrc, (int)mrows, stream->tgt, (long long)mrows, m->p_scores, (long long)ldo, 1, (int*)nullptr, 0LL, (const int*)nullptr, 0u);
        hipLaunchKernelGGL(k_score_count, dim3(cdiv(n_sel, 32), cdiv(mrows, SC_BM)), dim3(256), m->smem_score, m->stream, (const DevModel*)m->d_dm,
                           hsrc, (int)mrows, d_items, (long long)n_sel, m->p_scores, (long long)ldo, 1, m->p_cnt, stream->col_begin,
                           stream->mode == G4R_RANK_TIEBREAKING ? stream->tie_col : (const int*)nullptr, stream->tie_ctr);
        hipLaunchKernelGGL(k_rank_counts, dim3(cdiv(mrows, 256)), dim3(256), 0, m->stream, m->p_cnt, (int)mrows, stream->mode, m->p_ranks);
        HIPCHK(hipGetLastError());
        m->p_nsel = 0; m->p_ldo = ldo;        // no score matrix to read back
        return 0;
    }
    score_rows(m, hsrc, mrows, d_items, n_sel, m->p_scores, ldo);
    HIPCHK(hipGetLastError());
    m->p_nsel = n_sel; m->p_ldo = ldo;
    return 0;
}

// the k checks shared by g4r_recommend_step / g4r_recommend_step_filtered
static int recommend_check(g4r_model* m, const int32_t* item_idx, int64_t n_sel, int32_t k, int32_t* out_cols, float* out_scores) {
    if (!m || !out_cols || !out_scores) return fail("null argument");
    const int64_t n_cand = item_idx ? n_sel : (int64_t)m->dm.n_items;
    if (k < 1 || k > G4R_TOPK_MAX) return fail("k must be in [1, " + std::to_string(G4R_TOPK_MAX) + "]");
    if (k > n_cand) return fail("k exceeds the number of candidates (n_sel = " + std::to_string(n_cand) + ")");
    if (n_cand > INT32_MAX) return fail("more than 2^31 - 1 candidates");
    return 0;
}

// selection of rows [0, mrows) of hsrc (the top layer's output) into p_tcols / p_tscores, enqueued only.  scores / ldo: the same
// rows' materialised scores (softmax / softmax_logit), unused otherwise.  ex (device exclusions) NULL: the unfiltered kernels;
// gx (g4r_continue_sessions, instead of ex): exclusions whose per-row lists grow on the device
static int topk_select(g4r_model* m, const float* hsrc, int32_t mrows, const int* d_items, int64_t n_sel, int32_t k, const TkExcl* ex,
                       const float* scores, int64_t ldo, const TkGrow* gx = nullptr) {
    const DevModel& d = m->dm;
    const bool sm = (d.final_act == G4R_ACT_SOFTMAX || d.final_act == G4R_ACT_SOFTMAX_LOGIT);
    // column ranges: (row blocks) x (ranges) workgroups, one per compute unit (the LDS of k_topk_range admits one per CU)
    const int row_blocks = cdiv(mrows, SC_BM);
    const int64_t tiles = (n_sel + TK_TN - 1) / TK_TN;
    const int64_t R0 = std::min<int64_t>(std::max(1, m->n_cu / row_blocks), tiles);
    const int tpr = (int)((tiles + R0 - 1) / R0);
    const int R = (int)((tiles + tpr - 1) / tpr);
    const int64_t need = (int64_t)mrows * R * k, nout = (int64_t)mrows * k;
    if (need > m->p_topk_cap || nout > m->p_tout_cap) {
        HIPCHK(hipStreamSynchronize(m->stream));
        if (need > m->p_topk_cap) {
            dfree(m, m->p_topk);
            if (dalloc(m, &m->p_topk, (size_t)need, false)) return -1;
            m->p_topk_cap = need;
        }
        if (nout > m->p_tout_cap) {
            dfree(m, m->p_tcols); dfree(m, m->p_tscores);
            if (dalloc(m, &m->p_tcols, (size_t)nout, false) || dalloc(m, &m->p_tscores, (size_t)nout, false)) return -1;
            m->p_tout_cap = nout;
        }
    }
    const dim3 grid(R, row_blocks);
    if (gx && sm)
        hipLaunchKernelGGL(k_topk_stored_g, grid, dim3(256), TK_SMEM_STORED_X, m->stream, (const DevModel*)m->d_dm, hsrc,
                           (int)mrows, d_items, (long long)n_sel, scores, (long long)ldo, (int)k, tpr, m->p_topk, *gx);
    else if (gx)
        hipLaunchKernelGGL(k_topk_fused_g, grid, dim3(256), TK_SMEM_FUSED_X, m->stream, (const DevModel*)m->d_dm, hsrc,
                           (int)mrows, d_items, (long long)n_sel, (const float*)nullptr, 0LL, (int)k, tpr, m->p_topk, *gx);
    else if (sm && !ex)
        hipLaunchKernelGGL(k_topk_stored, grid, dim3(256), TK_SMEM_STORED, m->stream, (const DevModel*)m->d_dm, hsrc,
                           (int)mrows, d_items, (long long)n_sel, scores, (long long)ldo, (int)k, tpr, m->p_topk);
    else if (sm)
        hipLaunchKernelGGL(k_topk_stored_x, grid, dim3(256), TK_SMEM_STORED_X, m->stream, (const DevModel*)m->d_dm, hsrc,
                           (int)mrows, d_items, (long long)n_sel, scores, (long long)ldo, (int)k, tpr, m->p_topk, *ex);
    else if (!ex)
        hipLaunchKernelGGL(k_topk_fused, grid, dim3(256), TK_SMEM_FUSED, m->stream, (const DevModel*)m->d_dm, hsrc,
                           (int)mrows, d_items, (long long)n_sel, (const float*)nullptr, 0LL, (int)k, tpr, m->p_topk);
    else
        hipLaunchKernelGGL(k_topk_fused_x, grid, dim3(256), TK_SMEM_FUSED_X, m->stream, (const DevModel*)m->d_dm, hsrc,
                           (int)mrows, d_items, (long long)n_sel, (const float*)nullptr, 0LL, (int)k, tpr, m->p_topk, *ex);
    hipLaunchKernelGGL(k_topk_merge, dim3(mrows), dim3(256), 0, m->stream, (const uint2*)m->p_topk, R, (int)k, m->p_tcols, m->p_tscores);
    HIPCHK(hipGetLastError());
    return 0;
}

// grow-only device buffer of one candidate call (stream-ordered: the stream is drained before the old one is freed)
extern "C++" {
template <class T>
static int cand_reserve(g4r_model* m, T** p, int64_t* cap, int64_t need) {
    if (need <= *cap) return 0;
    HIPCHK(hipStreamSynchronize(m->stream));
    dfree(m, *p);
    *p = nullptr;
    *cap = 0;
    if (dalloc(m, p, (size_t)need, false)) return -1;
    *cap = need;
    return 0;
}
}  // extern "C++"

// ------------------------------------------------------------------------------------------------ two-stage top-k (bf16 scan)
// the checks of scan = bf16 next to recommend_check's: *c = the candidates kept per row, min(number of candidates, k * oversample)
static int scan_check(g4r_model* m, const int32_t* item_idx, int64_t n_sel, int32_t k, int32_t oversample, int32_t* c) {
    const DevModel& d = m->dm;
    if (d.final_act == G4R_ACT_SOFTMAX || d.final_act == G4R_ACT_SOFTMAX_LOGIT)
        return fail("the bf16 scan is not implemented for softmax / softmax_logit final activations (their exact values need the whole row)");
    if (oversample < 1 || (int64_t)k * oversample > G4R_SCAN_CAND_MAX)
        return fail("oversample must be at least 1 and k * oversample at most G4R_SCAN_CAND_MAX = " + std::to_string(G4R_SCAN_CAND_MAX));
    if (d.Dtop > 512) return fail("the bf16 scan supports top layers of at most 512 units");
    *c = (int32_t)std::min<int64_t>(item_idx ? n_sel : (int64_t)d.n_items, (int64_t)k * oversample);
    return 0;
}

// k-chunks of 64 columns of the padded top layer (the instantiations of k_scan_bf16: 2, 4, 8)
static int scan_nch(const DevModel& d) { return d.Dtop <= 128 ? 2 : d.Dtop <= 256 ? 4 : 8; }

// the bf16 shadow table of Wy, (re)built on the stream when anything may have changed Wy since the last build
static int scan_table_ensure(g4r_model* m) {
    if (m->s_tab_valid) return 0;
    const DevModel& d = m->dm;
    const int KS = 4 * scan_nch(d);
    const int64_t nblk = ((int64_t)d.n_items + 31) / 32, units = nblk * KS * 64;
    if (units > m->s_tab_units) {
        HIPCHK(hipStreamSynchronize(m->stream));
        dfree(m, m->s_tab);
        m->s_tab = nullptr;
        m->s_tab_units = 0;
        if (dalloc(m, &m->s_tab, (size_t)units, false)) return -1;
        m->s_tab_units = units;
    }
    hipLaunchKernelGGL(k_wy_bf16, dim3((unsigned)((units + 255) / 256)), dim3(256), 0, m->stream, (const DevModel*)m->d_dm, m->s_tab,
                       (long long)nblk, KS);
    HIPCHK(hipGetLastError());
    m->s_tab_valid = true;
    ++m->s_tab_builds;
    return 0;
}

int g4r_scan_table_release(g4r_model* m) {
    if (!m) return fail("null model");
    HIPCHK(hipSetDevice(m->cfg.device));
    HIPCHK(hipStreamSynchronize(m->stream));
    dfree(m, m->s_tab);
    m->s_tab = nullptr;
    m->s_tab_units = 0;
    m->s_tab_valid = false;
    return 0;
}

// topk_select's two-stage twin (element-wise final activations only): rows [0, mrows) of hsrc -> p_tcols / p_tscores, enqueued only,
// no host synchronisation between the stages.  Stage 1: k_scan_bf16 keeps c candidates per row and range, k_scan_merge the row's c.
// Stage 2: k_score_cand scores them (fp32, bit-identical to g4r_predict_step), k_scan_pack + k_topk_merge return the k best.
// gx (g4r_continue_sessions, instead of ex): exclusions whose per-row lists grow on the device; work_ready: k_score_cand's work items
// of an earlier call with the same mrows and c are still in c_work (nothing is uploaded)
static int topk_select_scan(g4r_model* m, const float* hsrc, int32_t mrows, const int* d_items, int64_t n_sel, int32_t k, int32_t c,
                            const TkExcl* ex, const TkGrow* gx = nullptr, bool work_ready = false) {
    if (scan_table_ensure(m)) return -1;
    const int row_blocks = cdiv(mrows, SC_BM);
    const int64_t tiles = (n_sel + SCN_TN - 1) / SCN_TN;
    const int64_t R0 = std::min<int64_t>(std::max(1, m->n_cu / row_blocks), tiles);
    const int tpr = (int)((tiles + R0 - 1) / R0);
    const int R = (int)((tiles + tpr - 1) / tpr);
    const int nl = (c + k - 1) / k, L = nl * k;
    const int64_t need = (int64_t)mrows * R * c, nout = (int64_t)mrows * k, P = (int64_t)mrows * c;
    if (mrows > 65535) return fail("the bf16 scan takes at most 65535 rows per call");
    if (need > m->p_topk_cap || nout > m->p_tout_cap) {
        HIPCHK(hipStreamSynchronize(m->stream));
        if (need > m->p_topk_cap) {
            dfree(m, m->p_topk);
            m->p_topk = nullptr;
            m->p_topk_cap = 0;
            if (dalloc(m, &m->p_topk, (size_t)need, false)) return -1;
            m->p_topk_cap = need;
        }
        if (nout > m->p_tout_cap) {
            dfree(m, m->p_tcols); dfree(m, m->p_tscores);
            m->p_tcols = nullptr; m->p_tscores = nullptr;
            m->p_tout_cap = 0;
            if (dalloc(m, &m->p_tcols, (size_t)nout, false) || dalloc(m, &m->p_tscores, (size_t)nout, false)) return -1;
            m->p_tout_cap = nout;
        }
    }
    // k_score_cand's work items depend on c and the row count only: row r's list is positions [r c, (r + 1) c)
    if (!work_ready) {
        m->s_work.clear();
        for (int r = 0; r < mrows; ++r)
            for (int p = 0; p < c; p += CS_SLICE) m->s_work.push_back(make_int4(r, r * c + p, r * c + std::min(p + CS_SLICE, (int)c), r * c));
    }
    if (cand_reserve(m, &m->c_items, &m->c_items_cap, P) || cand_reserve(m, &m->c_scores, &m->c_scores_cap, P) ||
        cand_reserve(m, &m->c_work, &m->c_work_cap, (int64_t)m->s_work.size()) || cand_reserve(m, &m->c_topk, &m->c_topk_cap, (int64_t)mrows * L) ||
        cand_reserve(m, &m->s_cols, &m->s_cols_cap, P) || cand_reserve(m, &m->s_cnt, &m->s_cnt_cap, (int64_t)mrows))
        return -1;
    if (!work_ready) HIPCHK(hipMemcpyAsync(m->c_work, m->s_work.data(), m->s_work.size() * sizeof(int4), hipMemcpyHostToDevice, m->stream));
    const dim3 grid(R, row_blocks);
    const TkExcl x = ex ? *ex : TkExcl{nullptr, nullptr, nullptr};
#define SCAN_LAUNCH(N) hipLaunchKernelGGL(k_scan_bf16<N>, grid, dim3(256), SCN_SMEM, m->stream, (const DevModel*)m->d_dm, hsrc, (int)mrows, d_items, \
                                          (long long)n_sel, (const uint4*)m->s_tab, (int)c, tpr, m->p_topk, x)
#define SCAN_LAUNCH_G(N) hipLaunchKernelGGL((k_scan_bf16<N, TkGrow>), grid, dim3(256), SCN_SMEM, m->stream, (const DevModel*)m->d_dm, hsrc, (int)mrows, \
                                            d_items, (long long)n_sel, (const uint4*)m->s_tab, (int)c, tpr, m->p_topk, *gx)
    if (gx)
        switch (scan_nch(m->dm)) {
            case 2: SCAN_LAUNCH_G(2); break;
            case 4: SCAN_LAUNCH_G(4); break;
            default: SCAN_LAUNCH_G(8); break;
        }
    else
        switch (scan_nch(m->dm)) {
            case 2: SCAN_LAUNCH(2); break;
            case 4: SCAN_LAUNCH(4); break;
            default: SCAN_LAUNCH(8); break;
        }
#undef SCAN_LAUNCH
#undef SCAN_LAUNCH_G
    hipLaunchKernelGGL(k_scan_merge, dim3(mrows), dim3(256), 0, m->stream, (const uint2*)m->p_topk, R, (int)c, d_items, m->s_cols, m->c_items,
                       m->c_scores, m->s_cnt);
#if !(defined(G4R_MUTATE) && G4R_MUTATE == 12)      // test build 12: stage 2 ranks by the approximate scores k_scan_merge left there
    hipLaunchKernelGGL(k_score_cand, dim3((unsigned)m->s_work.size()), dim3(256), 0, m->stream, (const DevModel*)m->d_dm, hsrc,
                       (const int*)m->c_items, (const int4*)m->c_work, m->c_scores, 1);
#endif
    hipLaunchKernelGGL(k_scan_pack, dim3(cdiv(L, 256), mrows), dim3(256), 0, m->stream, (const float*)m->c_scores, (const int*)m->s_cols,
                       (const int*)m->s_cnt, (int)c, L, m->c_topk);
    hipLaunchKernelGGL(k_topk_merge, dim3(mrows), dim3(256), 0, m->stream, (const uint2*)m->c_topk, nl, (int)k, m->p_tcols, m->p_tscores);
    HIPCHK(hipGetLastError());
    return 0;
}

// GRU step + selection of a checked call whose inputs predict_inputs has uploaded; ex (device exclusions) NULL: the unfiltered kernels
// scan_c > 0: the two-stage selection with scan_c candidates per row (scan_check has refused softmax)
static int recommend_run(g4r_model* m, int32_t mrows, const int32_t* item_idx, int64_t n_sel, int32_t k, const TkExcl* ex,
                         int32_t* out_cols, float* out_scores, int32_t scan_c = 0) {
    DevModel& d = m->dm;
    const int* d_items = item_idx ? (const int*)m->p_items : (const int*)nullptr;
    const bool sm = (d.final_act == G4R_ACT_SOFTMAX || d.final_act == G4R_ACT_SOFTMAX_LOGIT);
    // softmax needs the whole row first: the scores are materialised exactly as g4r_predict_step materialises them, then selected;
    // an element-wise final activation is selected as the tiles are scored (nothing stored)
    if (sm) {
        if (predict_forward(m, m->p_in, mrows, d_items, n_sel, nullptr)) return -1;
    } else {
        predict_gru(m, m->p_in, mrows);
    }
    if (scan_c > 0) {
        if (topk_select_scan(m, (const float*)m->phout[d.n_layers - 1], mrows, d_items, n_sel, k, scan_c, ex)) return -1;
    } else if (topk_select(m, (const float*)m->phout[d.n_layers - 1], mrows, d_items, n_sel, k, ex, (const float*)m->p_scores, m->p_ldo)) return -1;
    const int64_t nout = (int64_t)mrows * k;
    HIPCHK(hipMemcpyAsync(out_cols, m->p_tcols, nout * sizeof(int), hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipMemcpyAsync(out_scores, m->p_tscores, nout * sizeof(float), hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    return 0;
}

int g4r_recommend_step(g4r_model* m, const int32_t* in_idx, int32_t mrows, const int32_t* item_idx, int64_t n_sel,
                       int32_t k, int32_t* out_cols, float* out_scores) {
    if (recommend_check(m, item_idx, n_sel, k, out_cols, out_scores)) return -1;
    if (predict_inputs(m, in_idx, mrows, item_idx, &n_sel)) return -1;
    return recommend_run(m, mrows, item_idx, n_sel, k, nullptr, out_cols, out_scores);
}

// the exclusion checks shared by g4r_recommend_step_filtered / g4r_recommend_sessions: every row's list is checked, sorted and
// de-duplicated into offs / items (left empty without excl_offs); a row with fewer than k eligible candidate positions is refused.
// grow (g4r_continue_sessions with no_repeat): the items every row's list will gain on the device, each taking one eligible position
static int excl_pack(g4r_model* m, int32_t mrows, const int32_t* item_idx, int64_t n_sel, int32_t k, const int64_t* excl_offs,
                     const int32_t* excl_items, const uint32_t* excl_mask, std::vector<long long>& offs, std::vector<int32_t>& items,
                     int32_t grow = 0) {
    const int64_t I = m->dm.n_items, nw = (I + 31) / 32;
    offs.clear();
    items.clear();
    // (without lists every row starts empty: row 0 stands for all of them)
    if (!excl_offs && grow > G4R_EXCLUDE_MAX)
        return fail("row 0 excludes 0 distinct items and generates " + std::to_string(grow) + " more (steps - 1), more than G4R_EXCLUDE_MAX = " +
                    std::to_string(G4R_EXCLUDE_MAX));
    if (excl_offs) {
        if (excl_offs[0] < 0) return fail("excl_offs[0] is negative");
        for (int r = 0; r < mrows; ++r)
            if (excl_offs[r + 1] < excl_offs[r]) return fail("excl_offs is not monotone at row " + std::to_string(r));
        if (excl_offs[mrows] > excl_offs[0] && !excl_items) return fail("null argument (excl_items)");
        offs.resize((size_t)mrows + 1, 0);
        items.reserve((size_t)std::min<int64_t>(excl_offs[mrows] - excl_offs[0], (int64_t)mrows * G4R_EXCLUDE_MAX));
        for (int r = 0; r < mrows; ++r) {
            const size_t b = items.size();
            for (int64_t j = excl_offs[r]; j < excl_offs[r + 1]; ++j) {
                if (excl_items[j] < 0 || excl_items[j] >= I) return fail("excluded item index out of range in row " + std::to_string(r));
                items.push_back(excl_items[j]);
            }
            std::sort(items.begin() + b, items.end());
            items.erase(std::unique(items.begin() + b, items.end()), items.end());
            if (items.size() - b > G4R_EXCLUDE_MAX)
                return fail("row " + std::to_string(r) + " excludes " + std::to_string(items.size() - b) + " distinct items, more than G4R_EXCLUDE_MAX = " +
                            std::to_string(G4R_EXCLUDE_MAX));
            if (items.size() - b + grow > G4R_EXCLUDE_MAX)
                return fail("row " + std::to_string(r) + " excludes " + std::to_string(items.size() - b) + " distinct items and generates " +
                            std::to_string(grow) + " more (steps - 1), more than G4R_EXCLUDE_MAX = " + std::to_string(G4R_EXCLUDE_MAX));
            offs[r + 1] = (long long)items.size();
        }
    }
    auto masked = [&](int32_t i) { return excl_mask && ((excl_mask[i >> 5] >> (i & 31)) & 1u); };
    // eligible candidate positions per row: n_cand - (positions of masked items) - (positions of the row's unmasked items)
    const int64_t n_cand = item_idx ? n_sel : I;
    int64_t n_masked = 0;
    std::vector<int32_t> uni;                 // with item_idx: the items of all rows' lists, sorted, and their position counts
    std::vector<int64_t> cnt;
    if (excl_offs && item_idx) {
        uni = items;
        std::sort(uni.begin(), uni.end());
        uni.erase(std::unique(uni.begin(), uni.end()), uni.end());
        cnt.assign(uni.size(), 0);
    }
    if (item_idx) {
        std::vector<uint32_t> in_uni((size_t)nw, 0u);
        for (int32_t i : uni) in_uni[i >> 5] |= 1u << (i & 31);
        for (int64_t p = 0; p < n_sel; ++p) {
            const int32_t i = item_idx[p];
            if (masked(i)) ++n_masked;
            else if ((in_uni[i >> 5] >> (i & 31)) & 1u) ++cnt[std::lower_bound(uni.begin(), uni.end(), i) - uni.begin()];
        }
    } else if (excl_mask) {
        for (int64_t w = 0; w < nw; ++w) {
            const uint32_t valid = (w == nw - 1 && (I & 31)) ? ((1u << (I & 31)) - 1u) : 0xFFFFFFFFu;
            n_masked += __builtin_popcount(excl_mask[w] & valid);
        }
    }
    for (int r = 0; r < mrows; ++r) {
        int64_t gone = n_masked;
        if (excl_offs)
            for (long long j = offs[r]; j < offs[r + 1]; ++j)
                if (!masked(items[j])) gone += item_idx ? cnt[std::lower_bound(uni.begin(), uni.end(), items[j]) - uni.begin()] : 1;
        if (n_cand - gone < k)
            return fail("row " + std::to_string(r) + " has " + std::to_string(n_cand - gone) + " eligible candidate positions, fewer than k = " +
                        std::to_string(k));
        if (n_cand - gone - grow < k)
            return fail("row " + std::to_string(r) + " has " + std::to_string(n_cand - gone) + " eligible candidate positions, fewer than k + steps - 1 = " +
                        std::to_string(k + grow) + " (every generated item takes one)");
    }
    return 0;
}

// upload of packed exclusions (into buffers that only grow, stream-ordered) -> *ex, the device view; has_lists: offs / items hold
// per-row lists
static int excl_upload(g4r_model* m, bool has_lists, const std::vector<long long>& offs, const std::vector<int32_t>& items,
                       const uint32_t* excl_mask, TkExcl* ex) {
    const int64_t nw = ((int64_t)m->dm.n_items + 31) / 32;
    if (has_lists) {
        if ((int64_t)offs.size() > m->p_xoffs_cap || (int64_t)items.size() > m->p_xitems_cap) {
            HIPCHK(hipStreamSynchronize(m->stream));
            if ((int64_t)offs.size() > m->p_xoffs_cap) {
                dfree(m, m->p_xoffs);
                if (dalloc(m, &m->p_xoffs, offs.size(), false)) return -1;
                m->p_xoffs_cap = (int64_t)offs.size();
            }
            if ((int64_t)items.size() > m->p_xitems_cap) {
                dfree(m, m->p_xitems);
                if (dalloc(m, &m->p_xitems, items.size(), false)) return -1;
                m->p_xitems_cap = (int64_t)items.size();
            }
        }
        HIPCHK(hipMemcpyAsync(m->p_xoffs, offs.data(), offs.size() * sizeof(long long), hipMemcpyHostToDevice, m->stream));
        if (!items.empty()) HIPCHK(hipMemcpyAsync(m->p_xitems, items.data(), items.size() * sizeof(int32_t), hipMemcpyHostToDevice, m->stream));
    }
    if (excl_mask) {
        if (nw > m->p_xmask_cap) {
            HIPCHK(hipStreamSynchronize(m->stream));
            dfree(m, m->p_xmask);
            if (dalloc(m, &m->p_xmask, (size_t)nw, false)) return -1;
            m->p_xmask_cap = nw;
        }
        HIPCHK(hipMemcpyAsync(m->p_xmask, excl_mask, (size_t)nw * sizeof(uint32_t), hipMemcpyHostToDevice, m->stream));
    }
    *ex = TkExcl{has_lists ? (const long long*)m->p_xoffs : nullptr, has_lists ? (const int*)m->p_xitems : nullptr,
                 excl_mask ? (const unsigned*)m->p_xmask : nullptr};
    return 0;
}

int g4r_recommend_step_filtered(g4r_model* m, const int32_t* in_idx, int32_t mrows, const int32_t* item_idx, int64_t n_sel,
                                int32_t k, const int64_t* excl_offs, const int32_t* excl_items, const uint32_t* excl_mask,
                                int32_t* out_cols, float* out_scores) {
    if (!excl_offs && !excl_mask) return g4r_recommend_step(m, in_idx, mrows, item_idx, n_sel, k, out_cols, out_scores);
    if (recommend_check(m, item_idx, n_sel, k, out_cols, out_scores)) return -1;
    if (predict_inputs(m, in_idx, mrows, item_idx, &n_sel)) return -1;      // (uploads only: the state advances in recommend_run)
    std::vector<long long> offs;
    std::vector<int32_t> items;
    if (excl_pack(m, mrows, item_idx, n_sel, k, excl_offs, excl_items, excl_mask, offs, items)) return -1;
    TkExcl ex;
    if (excl_upload(m, excl_offs != nullptr, offs, items, excl_mask, &ex)) return -1;
    return recommend_run(m, mrows, item_idx, n_sel, k, &ex, out_cols, out_scores);
}

int g4r_recommend_step_scan(g4r_model* m, const int32_t* in_idx, int32_t mrows, const int32_t* item_idx, int64_t n_sel, int32_t k,
                            int32_t oversample, const int64_t* excl_offs, const int32_t* excl_items, const uint32_t* excl_mask,
                            int32_t* out_cols, float* out_scores) {
    int32_t c = 0;
    if (recommend_check(m, item_idx, n_sel, k, out_cols, out_scores) || scan_check(m, item_idx, n_sel, k, oversample, &c)) return -1;
    if (predict_inputs(m, in_idx, mrows, item_idx, &n_sel)) return -1;      // (uploads only: the state advances in recommend_run)
    if (!excl_offs && !excl_mask) return recommend_run(m, mrows, item_idx, n_sel, k, nullptr, out_cols, out_scores, c);
    std::vector<long long> offs;
    std::vector<int32_t> items;
    if (excl_pack(m, mrows, item_idx, n_sel, k, excl_offs, excl_items, excl_mask, offs, items)) return -1;
    TkExcl ex;
    if (excl_upload(m, excl_offs != nullptr, offs, items, excl_mask, &ex)) return -1;
    return recommend_run(m, mrows, item_idx, n_sel, k, &ex, out_cols, out_scores, c);
}

// ------------------------------------------------------------------------------------------------ stateless session replay
// Rows per chunk of g4r_recommend_sessions: its score matrix (softmax / softmax_logit) is then never larger than g4r_recommend_step's
// at 512 rows.  G4R_SESSIONS_CHUNK > 0 (read per call) forces a smaller chunk: tests show the results do not depend on it.
#define G4R_REPLAY_CHUNK 512

// the replay buffers for chunks of `rows` rows and n_in step-major input items (grow only)
static int replay_reserve(g4r_model* m, int rows, int64_t n_in) {
    const DevModel& d = m->dm;
    if (rows > m->r_cap) {
        HIPCHK(hipStreamSynchronize(m->stream));
        m->r_cap = 0;
        for (int l = 0; l < d.n_layers; ++l) {
            float** bufs[] = {&m->rH[l][0], &m->rH[l][1], &m->rhout[l], &m->rVc[l], &m->rz[l], &m->rHr[l], &m->rio[l]};
            for (float** b : bufs) {
                dfree(m, *b);
                *b = nullptr;
                if (dalloc(m, b, (size_t)rows * d.D[l])) return -1;
            }
        }
        dfree(m, m->r_perm); dfree(m, m->r_len);
        m->r_perm = m->r_len = nullptr;
        if (dalloc(m, &m->r_perm, (size_t)rows, false) || dalloc(m, &m->r_len, (size_t)rows, false)) return -1;
        m->r_cap = rows;
    }
    if (n_in > m->r_in_cap) {
        HIPCHK(hipStreamSynchronize(m->stream));
        dfree(m, m->r_in);
        m->r_in = nullptr;
        m->r_in_cap = 0;
        if (dalloc(m, &m->r_in, (size_t)n_in, false)) return -1;
        m->r_in_cap = n_in;
    }
    return 0;
}

// the history / hidden-state checks of g4r_recommend_sessions / g4r_score_candidates_sessions
static int replay_check(g4r_model* m, const int64_t* hist_offs, const int32_t* hist_items, int32_t n, const float* const* h0,
                        float* const* out_hidden) {
    if (!hist_offs || !hist_items) return fail("null argument");
    if (n < 1) return fail("n must be positive");
    const DevModel& d = m->dm;
    if (hist_offs[0] < 0) return fail("hist_offs[0] is negative");
    for (int i = 0; i < n; ++i)
        if (hist_offs[i + 1] <= hist_offs[i]) return fail("history " + std::to_string(i) + " is empty (hist_offs must rise strictly)");
    for (int64_t j = hist_offs[0]; j < hist_offs[n]; ++j)
        if (hist_items[j] < 0 || hist_items[j] >= d.n_items) return fail("history item index out of range");
    for (int l = 0; l < d.n_layers; ++l) {
        if (h0 && !h0[l]) return fail("null argument (h0[" + std::to_string(l) + "])");
        if (out_hidden && !out_hidden[l]) return fail("null argument (out_hidden[" + std::to_string(l) + "])");
    }
    return 0;
}

// rows per chunk of a replay of n sessions
static int replay_chunk_rows(int32_t n) {
    const int env_c = env_int("G4R_SESSIONS_CHUNK", 0);
    return std::min<int>(n, env_c > 0 ? std::min(env_c, G4R_REPLAY_CHUNK) : G4R_REPLAY_CHUNK);
}

// The checked histories replayed chunk by chunk (C rows per chunk, replay_chunk_rows).  Per chunk: the rows are sorted by history
// length and stepped on the replay buffers; score(c0, Cc, perm, hsrc) enqueues what the caller computes from the top layer's output
// hsrc (sorted row r is session c0 + perm[r]); the final states go to out_hidden (NULL: not wanted); the stream is synchronised once
// and done(c0, Cc, perm) runs on the host.  Shared by g4r_recommend_sessions, g4r_score_candidates_sessions and g4r_continue_sessions.
// final_half (g4r_continue_sessions): score() leaves there the ping-pong half that holds EVERY row's final state after its rollout
// (-1: the replay's own rule, each row's in H[len & 1]).
extern "C++" {      // (this file is included inside extern "C")
template <class S, class F>
static int replay_chunks(g4r_model* m, const int64_t* hist_offs, const int32_t* hist_items, int32_t n, int C, const float* const* h0,
                         float* const* out_hidden, S score, F done, const int* final_half = nullptr) {
    const DevModel& d = m->dm;
    const int L = d.n_layers;
    const GruBufs rb = replay_bufs(m);
    std::vector<int> perm, len;
    std::vector<int32_t> steps;
    for (int c0 = 0; c0 < n; c0 += C) {
        const int Cc = std::min(C, n - c0);
        // rows sorted by history length, descending (stable): step t runs on the prefix of rows still active
        perm.resize(Cc);
        for (int r = 0; r < Cc; ++r) perm[r] = r;
        auto hlen = [&](int r) { return hist_offs[c0 + r + 1] - hist_offs[c0 + r]; };
        std::stable_sort(perm.begin(), perm.end(), [&](int a, int b) { return hlen(a) > hlen(b); });
        len.resize(Cc);
        for (int r = 0; r < Cc; ++r) len[r] = (int)hlen(perm[r]);
        const int T = len[0];
        // input items of every step, step-major [T][Cc] (rows that have finished by step t: 0, never read)
        steps.assign((size_t)T * Cc, 0);
        for (int r = 0; r < Cc; ++r) {
            const int32_t* h = hist_items + hist_offs[c0 + perm[r]];
            for (int t = 0; t < len[r]; ++t) steps[(size_t)t * Cc + r] = h[t];
        }
        if (replay_reserve(m, Cc, (int64_t)T * Cc)) return -1;
        HIPCHK(hipMemcpyAsync(m->r_in, steps.data(), steps.size() * sizeof(int), hipMemcpyHostToDevice, m->stream));
        HIPCHK(hipMemcpyAsync(m->r_perm, perm.data(), Cc * sizeof(int), hipMemcpyHostToDevice, m->stream));
        HIPCHK(hipMemcpyAsync(m->r_len, len.data(), Cc * sizeof(int), hipMemcpyHostToDevice, m->stream));
        for (int l = 0; l < L; ++l) {
            if (h0) HIPCHK(hipMemcpyAsync(m->rio[l], h0[l] + (size_t)c0 * d.D[l], (size_t)Cc * d.D[l] * sizeof(float), hipMemcpyHostToDevice, m->stream));
            hipLaunchKernelGGL(k_replay_begin, dim3(cdiv((long long)Cc * d.D[l], 256)), dim3(256), 0, m->stream, m->rH[l][0],
                               h0 ? (const float*)m->rio[l] : (const float*)nullptr, (const int*)m->r_perm, Cc, d.D[l]);
        }
        // step t: sorted rows [0, M_t) (M_t = rows with len > t), H[t & 1] -> H[(t + 1) & 1].  A row that has finished is never
        // written again (gru_step), so the top layer's rhout row keeps its last output and its state stays in H[len & 1]
        int Mt = Cc;
        for (int t = 0; t < T; ++t) {
            while (Mt > 0 && len[Mt - 1] <= t) --Mt;
            gru_step(m, rb, t & 1, (const int*)m->r_in + (size_t)t * Cc, Mt);
        }
        if (score(c0, Cc, (const std::vector<int>&)perm, (const float*)m->rhout[L - 1])) return -1;
        if (out_hidden)
            for (int l = 0; l < L; ++l) {
                const int fh = final_half ? *final_half : -1;
                hipLaunchKernelGGL(k_replay_final, dim3(cdiv((long long)Cc * d.D[l], 256)), dim3(256), 0, m->stream, m->rio[l],
                                   (const float*)m->rH[l][fh < 0 ? 0 : fh], (const float*)m->rH[l][fh < 0 ? 1 : fh], (const int*)m->r_perm,
                                   (const int*)m->r_len, Cc, d.D[l], T);
                HIPCHK(hipMemcpyAsync(out_hidden[l] + (size_t)c0 * d.D[l], m->rio[l], (size_t)Cc * d.D[l] * sizeof(float),
                                      hipMemcpyDeviceToHost, m->stream));
            }
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(m->stream));
        done(c0, Cc, (const std::vector<int>&)perm);
    }
    return 0;
}
}  // extern "C++"

// g4r_recommend_sessions (oversample = 0: the exact selection) and g4r_recommend_sessions_scan (oversample >= 1)
static int recommend_sessions_run(g4r_model* m, const int64_t* hist_offs, const int32_t* hist_items, int32_t n, const float* const* h0,
                                  const int32_t* item_idx, int64_t n_sel, int32_t k, int32_t oversample, const int64_t* excl_offs,
                                  const int32_t* excl_items, const uint32_t* excl_mask, int32_t* out_cols, float* out_scores,
                                  float* const* out_hidden) {
    // ---- every check before any device work (nothing here has state to advance, but a refused call launches nothing)
    if (recommend_check(m, item_idx, n_sel, k, out_cols, out_scores)) return -1;
    int32_t scan_c = 0;
    if (oversample && scan_check(m, item_idx, n_sel, k, oversample, &scan_c)) return -1;
    HIPCHK(hipSetDevice(m->cfg.device));
    if (replay_check(m, hist_offs, hist_items, n, h0, out_hidden)) return -1;
    const DevModel& d = m->dm;
    if (!item_idx) n_sel = d.n_items;
    for (int64_t p = 0; item_idx && p < n_sel; ++p)
        if (item_idx[p] < 0 || item_idx[p] >= d.n_items) return fail("item index out of range");
    std::vector<long long> xoffs;
    std::vector<int32_t> xitems;
    if ((excl_offs || excl_mask) && excl_pack(m, n, item_idx, n_sel, k, excl_offs, excl_items, excl_mask, xoffs, xitems)) return -1;
    const bool excl = excl_offs || excl_mask;
    // ---- buffers and the call-wide uploads
    const int C = replay_chunk_rows(n);
    const bool sm = (d.final_act == G4R_ACT_SOFTMAX || d.final_act == G4R_ACT_SOFTMAX_LOGIT);
    const int64_t ldo = (n_sel + 3) & ~3LL;
    if (sm && (int64_t)C * ldo > m->r_scores_cap) {
        HIPCHK(hipStreamSynchronize(m->stream));
        dfree(m, m->r_scores);
        m->r_scores = nullptr;
        m->r_scores_cap = 0;
        if (dalloc(m, &m->r_scores, (size_t)C * ldo, false)) return -1;
        m->r_scores_cap = (int64_t)C * ldo;
    }
    if (item_idx) {
        if (n_sel > m->p_items_cap) {
            HIPCHK(hipStreamSynchronize(m->stream));
            dfree(m, m->p_items);
            m->p_items = nullptr;
            m->p_items_cap = 0;
            if (dalloc(m, &m->p_items, (size_t)n_sel, false)) return -1;
            m->p_items_cap = n_sel;
        }
        HIPCHK(hipMemcpyAsync(m->p_items, item_idx, n_sel * sizeof(int), hipMemcpyHostToDevice, m->stream));
    }
    const int* d_items = item_idx ? (const int*)m->p_items : (const int*)nullptr;
    std::vector<int32_t> tcols((size_t)C * k);
    std::vector<float> tscores((size_t)C * k);
    std::vector<long long> coffs;
    std::vector<int32_t> citems;
    // ---- chunk by chunk: the replay, then the selection; one synchronisation per chunk
    auto score = [&](int c0, int Cc, const std::vector<int>& perm, const float* hsrc) -> int {
        if (sm) score_rows(m, hsrc, Cc, d_items, n_sel, m->r_scores, ldo);
        TkExcl ex;
        if (excl) {
            // the chunk's lists in sorted row order (each already sorted and de-duplicated by excl_pack)
            coffs.assign(1, 0);
            citems.clear();
            if (excl_offs)
                for (int r = 0; r < Cc; ++r) {
                    const int i = c0 + perm[r];
                    citems.insert(citems.end(), xitems.begin() + xoffs[i], xitems.begin() + xoffs[i + 1]);
                    coffs.push_back((long long)citems.size());
                }
            if (excl_upload(m, excl_offs != nullptr, coffs, citems, excl_mask, &ex)) return -1;
        }
        if (scan_c > 0) {
            if (topk_select_scan(m, hsrc, Cc, d_items, n_sel, k, scan_c, excl ? &ex : nullptr)) return -1;
        } else if (topk_select(m, hsrc, Cc, d_items, n_sel, k, excl ? &ex : nullptr, (const float*)m->r_scores, ldo)) return -1;
        HIPCHK(hipMemcpyAsync(tcols.data(), m->p_tcols, (size_t)Cc * k * sizeof(int), hipMemcpyDeviceToHost, m->stream));
        HIPCHK(hipMemcpyAsync(tscores.data(), m->p_tscores, (size_t)Cc * k * sizeof(float), hipMemcpyDeviceToHost, m->stream));
        return 0;
    };
    // sorted row r is session c0 + perm[r]
    auto done = [&](int c0, int Cc, const std::vector<int>& perm) {
        for (int r = 0; r < Cc; ++r) {
            memcpy(out_cols + (size_t)(c0 + perm[r]) * k, tcols.data() + (size_t)r * k, (size_t)k * sizeof(int32_t));
            memcpy(out_scores + (size_t)(c0 + perm[r]) * k, tscores.data() + (size_t)r * k, (size_t)k * sizeof(float));
        }
    };
    return replay_chunks(m, hist_offs, hist_items, n, C, h0, out_hidden, score, done);
}

int g4r_recommend_sessions(g4r_model* m, const int64_t* hist_offs, const int32_t* hist_items, int32_t n, const float* const* h0,
                           const int32_t* item_idx, int64_t n_sel, int32_t k, const int64_t* excl_offs, const int32_t* excl_items,
                           const uint32_t* excl_mask, int32_t* out_cols, float* out_scores, float* const* out_hidden) {
    return recommend_sessions_run(m, hist_offs, hist_items, n, h0, item_idx, n_sel, k, 0, excl_offs, excl_items, excl_mask, out_cols,
                                  out_scores, out_hidden);
}

int g4r_recommend_sessions_scan(g4r_model* m, const int64_t* hist_offs, const int32_t* hist_items, int32_t n, const float* const* h0,
                                const int32_t* item_idx, int64_t n_sel, int32_t k, int32_t oversample, const int64_t* excl_offs,
                                const int32_t* excl_items, const uint32_t* excl_mask, int32_t* out_cols, float* out_scores,
                                float* const* out_hidden) {
    if (oversample < 1) return fail("oversample must be at least 1 and k * oversample at most G4R_SCAN_CAND_MAX = " + std::to_string(G4R_SCAN_CAND_MAX));
    return recommend_sessions_run(m, hist_offs, hist_items, n, h0, item_idx, n_sel, k, oversample, excl_offs, excl_items, excl_mask,
                                  out_cols, out_scores, out_hidden);
}

// ------------------------------------------------------------------------------------------------ multi-step continuation
// g4r_continue_sessions: g4r_recommend_sessions(_scan) followed, per chunk and on the device, by steps - 1 rounds of
// (winner -> GRU input -> GRU step -> selection).  One synchronisation and one download per chunk whatever `steps` is.
int g4r_continue_sessions(g4r_model* m, const int64_t* hist_offs, const int32_t* hist_items, int32_t n, const float* const* h0,
                          const int32_t* item_idx, int64_t n_sel, int32_t k, int32_t oversample, int32_t steps, int32_t no_repeat,
                          const int64_t* excl_offs, const int32_t* excl_items, const uint32_t* excl_mask, int32_t* out_cols,
                          float* out_scores, float* const* out_hidden) {
    // ---- every check before any device work
    if (recommend_check(m, item_idx, n_sel, k, out_cols, out_scores)) return -1;
    if (steps < 1) return fail("steps must be at least 1");
    if (oversample < 0) return fail("oversample must be 0 (the exact selection) or at least 1");
    int32_t scan_c = 0;
    if (oversample && scan_check(m, item_idx, n_sel, k, oversample, &scan_c)) return -1;
    HIPCHK(hipSetDevice(m->cfg.device));
    if (replay_check(m, hist_offs, hist_items, n, h0, out_hidden)) return -1;
    const DevModel& d = m->dm;
    if (!item_idx) n_sel = d.n_items;
    for (int64_t p = 0; item_idx && p < n_sel; ++p)
        if (item_idx[p] < 0 || item_idx[p] >= d.n_items) return fail("item index out of range");
    const bool grow = no_repeat != 0 && steps > 1;      // the lists gain items on the device
    if (no_repeat && item_idx) {
        // only then does every generated item take exactly one eligible position
        std::vector<uint32_t> seen(((size_t)d.n_items + 31) / 32, 0u);
        for (int64_t p = 0; p < n_sel; ++p) {
            const int32_t i = item_idx[p];
            if ((seen[i >> 5] >> (i & 31)) & 1u) return fail("no_repeat needs duplicate-free candidates: item index " + std::to_string(i) + " is listed twice");
            seen[i >> 5] |= 1u << (i & 31);
        }
    }
    std::vector<long long> xoffs;
    std::vector<int32_t> xitems;
    const bool excl = excl_offs || excl_mask || grow;
    if (excl && excl_pack(m, n, item_idx, n_sel, k, excl_offs, excl_items, excl_mask, xoffs, xitems, grow ? steps - 1 : 0)) return -1;
    const bool lists = excl_offs || grow;
    ++m->ro_calls;
    // ---- buffers and the call-wide uploads
    const int C = replay_chunk_rows(n);
    const int L = d.n_layers;
    const bool sm = (d.final_act == G4R_ACT_SOFTMAX || d.final_act == G4R_ACT_SOFTMAX_LOGIT);
    const int64_t ldo = (n_sel + 3) & ~3LL;
    if (sm && (int64_t)C * ldo > m->r_scores_cap) {
        HIPCHK(hipStreamSynchronize(m->stream));
        dfree(m, m->r_scores);
        m->r_scores = nullptr;
        m->r_scores_cap = 0;
        if (dalloc(m, &m->r_scores, (size_t)C * ldo, false)) return -1;
        m->r_scores_cap = (int64_t)C * ldo;
    }
    if (item_idx) {
        if (cand_reserve(m, &m->p_items, &m->p_items_cap, n_sel)) return -1;
        HIPCHK(hipMemcpyAsync(m->p_items, item_idx, n_sel * sizeof(int), hipMemcpyHostToDevice, m->stream));
    }
    const int64_t per_row = (int64_t)steps * k;
    if (cand_reserve(m, &m->ro_cols, &m->ro_cols_cap, (int64_t)C * per_row) || cand_reserve(m, &m->ro_scores, &m->ro_scores_cap, (int64_t)C * per_row) ||
        cand_reserve(m, &m->ro_in, &m->ro_in_cap, (int64_t)C) || (grow && cand_reserve(m, &m->ro_xlen, &m->ro_xlen_cap, (int64_t)C)))
        return -1;
    const int* d_items = item_idx ? (const int*)m->p_items : (const int*)nullptr;
    std::vector<int32_t> tcols((size_t)C * per_row);
    std::vector<float> tscores((size_t)C * per_row);
    std::vector<long long> coffs;
    std::vector<int32_t> citems, clen;
    const GruBufs rb = replay_bufs(m);
    int final_half = -1;
    auto score = [&](int c0, int Cc, const std::vector<int>& perm, const float* hsrc) -> int {
        TkExcl ex{};
        TkGrow gx{};
        if (excl) {
            // the chunk's lists in sorted row order (each already sorted and de-duplicated by excl_pack); growing lists: the begin of
            // every row's list (steps - 1 slots of slack behind it) instead of the CSR offsets, the lengths apart
            const int slack = grow ? steps - 1 : 0;
            coffs.clear();
            citems.clear();
            clen.clear();
            if (!grow) coffs.push_back(0);
            if (lists)
                for (int r = 0; r < Cc; ++r) {
                    const int i = c0 + perm[r];
                    if (grow) coffs.push_back((long long)citems.size());
                    if (excl_offs) citems.insert(citems.end(), xitems.begin() + xoffs[i], xitems.begin() + xoffs[i + 1]);
                    if (grow) {
                        clen.push_back(excl_offs ? (int32_t)(xoffs[i + 1] - xoffs[i]) : 0);
                        citems.insert(citems.end(), (size_t)slack, 0);
                    } else coffs.push_back((long long)citems.size());
                }
            if (excl_upload(m, lists, coffs, citems, excl_mask, &ex)) return -1;
            if (grow) {
                HIPCHK(hipMemcpyAsync(m->ro_xlen, clen.data(), (size_t)Cc * sizeof(int), hipMemcpyHostToDevice, m->stream));
                gx = TkGrow{ex.offs, (const int*)m->ro_xlen, ex.items, ex.mask};
            }
        }
        const int T = (int)(hist_offs[c0 + perm[0] + 1] - hist_offs[c0 + perm[0]]);      // the chunk's longest history
        for (int s = 0; s < steps; ++s) {
            ++m->ro_steps;
            if (s == 1) {
                // every row's state into the half of the longest history: from here on all Cc rows step together
                for (int l = 0; l < L; ++l)
                    hipLaunchKernelGGL(k_rollout_align, dim3(cdiv((long long)Cc * d.D[l], 256)), dim3(256), 0, m->stream, m->rH[l][T & 1],
                                       (const float*)m->rH[l][(T & 1) ^ 1], (const int*)m->r_len, Cc, d.D[l], T);
            }
            if (s > 0) gru_step(m, rb, (T + s - 1) & 1, (const int*)m->ro_in, Cc);
            if (sm) score_rows(m, hsrc, Cc, d_items, n_sel, m->r_scores, ldo);
            if (scan_c > 0) {
                if (topk_select_scan(m, hsrc, Cc, d_items, n_sel, k, scan_c, (excl && !grow) ? &ex : nullptr, grow ? &gx : nullptr, s > 0)) return -1;
            } else if (topk_select(m, hsrc, Cc, d_items, n_sel, k, (excl && !grow) ? &ex : nullptr, (const float*)m->r_scores, ldo, grow ? &gx : nullptr))
                return -1;
            const bool last = s == steps - 1;
            hipLaunchKernelGGL(k_rollout_feed, dim3(Cc), dim3(64), 0, m->stream, (const int*)m->p_tcols, (const float*)m->p_tscores, (int)k, (int)steps,
                               s, d_items, m->ro_cols, m->ro_scores, last ? (int*)nullptr : m->ro_in, gx.beg,
                               last ? (int*)nullptr : const_cast<int*>(gx.len), const_cast<int*>(gx.items));      // (gx: all NULL unless the lists grow)
        }
        final_half = steps > 1 ? ((T + steps - 1) & 1) : -1;
        HIPCHK(hipMemcpyAsync(tcols.data(), m->ro_cols, (size_t)Cc * per_row * sizeof(int), hipMemcpyDeviceToHost, m->stream));
        HIPCHK(hipMemcpyAsync(tscores.data(), m->ro_scores, (size_t)Cc * per_row * sizeof(float), hipMemcpyDeviceToHost, m->stream));
        return 0;
    };
    auto done = [&](int c0, int Cc, const std::vector<int>& perm) {
        for (int r = 0; r < Cc; ++r) {
            memcpy(out_cols + (size_t)(c0 + perm[r]) * per_row, tcols.data() + (size_t)r * per_row, (size_t)per_row * sizeof(int32_t));
            memcpy(out_scores + (size_t)(c0 + perm[r]) * per_row, tscores.data() + (size_t)r * per_row, (size_t)per_row * sizeof(float));
        }
    };
    return replay_chunks(m, hist_offs, hist_items, n, C, h0, out_hidden, score, done, &final_half);
}

// ------------------------------------------------------------------------------------------------ per-row candidate lists
// the checks of the candidate lists of g4r_score_candidates*: rows >= 1 non-empty lists, items in range, at most G4R_CAND_MAX
// positions in all, 0 <= k <= G4R_TOPK_MAX and every list at least k long when k > 0
static int cand_check(g4r_model* m, int32_t rows, const int64_t* cand_offs, const int32_t* cand_items, int32_t k, float* out_scores,
                      int32_t* out_pos) {
    if (!m || !cand_offs || !cand_items || !out_scores) return fail("null argument");
    if (rows < 1) return fail("the number of rows must be positive");
    if (k < 0 || k > G4R_TOPK_MAX) return fail("k must be in [0, " + std::to_string(G4R_TOPK_MAX) + "]");
    if (k > 0 && !out_pos) return fail("null argument (out_pos)");
    if (cand_offs[0] < 0) return fail("cand_offs[0] is negative");
    for (int r = 0; r < rows; ++r) {
        const int64_t n = cand_offs[r + 1] - cand_offs[r];
        if (n < 1) return fail("candidate list " + std::to_string(r) + " is empty (cand_offs must rise strictly)");
        if (n < k) return fail("candidate list " + std::to_string(r) + " holds " + std::to_string(n) + " positions, fewer than k = " + std::to_string(k));
        if (cand_offs[r + 1] - cand_offs[0] > G4R_CAND_MAX)
            return fail("more than G4R_CAND_MAX = " + std::to_string((long long)G4R_CAND_MAX) + " candidate positions in one call");
    }
    const int64_t I = m->dm.n_items;
    for (int64_t p = cand_offs[0]; p < cand_offs[rows]; ++p)
        if (cand_items[p] < 0 || cand_items[p] >= I) return fail("candidate item index out of range");
    return 0;
}

// host staging of one candidate call (kept until the stream has been synchronised)
struct CandHost { std::vector<long long> offs; std::vector<int4> work; };

// Enqueues the scoring of `rows` checked candidate lists against rows of hsrc (the top layer's output): list r (the items
// items[offs[r] .. offs[r + 1]), absolute indices) is scored against hsrc row hrow[r] (hrow NULL: row r).  k == 0: the scores in CSR
// order -> out_scores[offs[rows] - offs[0]]; k > 0: row r's k best (position in its list, score) -> out_pos / out_scores[r * k ..].
// The copies to the host are enqueued; the caller synchronises.
static int cand_enqueue(g4r_model* m, const float* hsrc, int32_t rows, const int* hrow, const int64_t* offs, const int32_t* items,
                        int32_t k, float* out_scores, int32_t* out_pos, CandHost& hs) {
    const DevModel& d = m->dm;
    const bool sm = (d.final_act == G4R_ACT_SOFTMAX || d.final_act == G4R_ACT_SOFTMAX_LOGIT);
    const int64_t base = offs[0], P = offs[rows] - base;
    // work items (h row, first position, end position, the row's first position): slices of at most CS_SLICE positions
    hs.offs.resize((size_t)rows + 1);
    hs.work.clear();
    for (int r = 0; r <= rows; ++r) hs.offs[r] = offs[r] - base;
    for (int r = 0; r < rows; ++r)
        for (long long p = hs.offs[r]; p < hs.offs[r + 1]; p += CS_SLICE)
            hs.work.push_back(make_int4(hrow ? hrow[r] : r, (int)p, (int)std::min<long long>(p + CS_SLICE, hs.offs[r + 1]), (int)hs.offs[r]));
    // top-k: groups of consecutive rows whose lists (nl * k entries per row, nl = ceil(the group's longest / k)) fit in CS_TOPK_ENTRIES
    // together (a longer single row gets a buffer of its own size); one k_cand_pack + k_topk_merge pair per group
    std::vector<int4> groups;      // (first row, rows, nl, -)
    int64_t topk_need = 0;
    if (k > 0) {
        for (int r0 = 0; r0 < rows;) {
            int64_t mx = 0;
            int r1 = r0;
            while (r1 < rows && r1 - r0 < 65535) {
                const int64_t nm = std::max<int64_t>(mx, hs.offs[r1 + 1] - hs.offs[r1]);
                if (r1 > r0 && (int64_t)(r1 - r0 + 1) * ((nm + k - 1) / k) * k > CS_TOPK_ENTRIES) break;
                mx = nm;
                ++r1;
            }
            const int nl = (int)((mx + k - 1) / k);
            groups.push_back(make_int4(r0, r1 - r0, nl, 0));
            topk_need = std::max<int64_t>(topk_need, (int64_t)(r1 - r0) * nl * k);
            r0 = r1;
        }
    }
    if (cand_reserve(m, &m->c_offs, &m->c_offs_cap, (int64_t)rows + 1) || cand_reserve(m, &m->c_items, &m->c_items_cap, P) ||
        cand_reserve(m, &m->c_scores, &m->c_scores_cap, P) || cand_reserve(m, &m->c_work, &m->c_work_cap, (int64_t)hs.work.size()) ||
        (k > 0 && (cand_reserve(m, &m->c_topk, &m->c_topk_cap, topk_need) || cand_reserve(m, &m->c_tpos, &m->c_tpos_cap, (int64_t)rows * k) ||
                   cand_reserve(m, &m->c_tscores, &m->c_tscores_cap, (int64_t)rows * k))))
        return -1;
    HIPCHK(hipMemcpyAsync(m->c_offs, hs.offs.data(), hs.offs.size() * sizeof(long long), hipMemcpyHostToDevice, m->stream));
    HIPCHK(hipMemcpyAsync(m->c_items, items + base, (size_t)P * sizeof(int32_t), hipMemcpyHostToDevice, m->stream));
    HIPCHK(hipMemcpyAsync(m->c_work, hs.work.data(), hs.work.size() * sizeof(int4), hipMemcpyHostToDevice, m->stream));
    // softmax needs the row's raw scores first: stored without the activation, then normalised over the row's own list
    hipLaunchKernelGGL(k_score_cand, dim3((unsigned)hs.work.size()), dim3(256), 0, m->stream, (const DevModel*)m->d_dm, hsrc,
                       (const int*)m->c_items, (const int4*)m->c_work, m->c_scores, sm ? 0 : 1);
    if (sm) hipLaunchKernelGGL(k_softmax_csr, dim3(rows), dim3(256), 0, m->stream, m->c_scores, (const long long*)m->c_offs);
    if (k == 0) {
        HIPCHK(hipMemcpyAsync(out_scores, m->c_scores, (size_t)P * sizeof(float), hipMemcpyDeviceToHost, m->stream));
    } else {
        for (const int4& g : groups) {
            const int L = g.z * k;
            hipLaunchKernelGGL(k_cand_pack, dim3(cdiv(L, 256), g.y), dim3(256), 0, m->stream, (const float*)m->c_scores,
                               (const long long*)m->c_offs + g.x, L, m->c_topk);
            hipLaunchKernelGGL(k_topk_merge, dim3(g.y), dim3(256), 0, m->stream, (const uint2*)m->c_topk, g.z, (int)k,
                               m->c_tpos + (size_t)g.x * k, m->c_tscores + (size_t)g.x * k);
        }
        HIPCHK(hipMemcpyAsync(out_pos, m->c_tpos, (size_t)rows * k * sizeof(int32_t), hipMemcpyDeviceToHost, m->stream));
        HIPCHK(hipMemcpyAsync(out_scores, m->c_tscores, (size_t)rows * k * sizeof(float), hipMemcpyDeviceToHost, m->stream));
    }
    HIPCHK(hipGetLastError());
    return 0;
}

int g4r_score_candidates(g4r_model* m, const int32_t* in_idx, int32_t mrows, const int64_t* cand_offs, const int32_t* cand_items,
                         int32_t k, float* out_scores, int32_t* out_pos) {
    // every check before the state advances: the lists here, the input items and mrows in predict_inputs (which only uploads)
    if (cand_check(m, mrows, cand_offs, cand_items, k, out_scores, out_pos)) return -1;
    int64_t n_sel = 0;
    if (predict_inputs(m, in_idx, mrows, nullptr, &n_sel)) return -1;
    predict_gru(m, m->p_in, mrows);
    CandHost hs;
    if (cand_enqueue(m, (const float*)m->phout[m->dm.n_layers - 1], mrows, nullptr, cand_offs, cand_items, k, out_scores, out_pos, hs)) return -1;
    HIPCHK(hipStreamSynchronize(m->stream));
    return 0;
}

int g4r_score_candidates_sessions(g4r_model* m, const int64_t* hist_offs, const int32_t* hist_items, int32_t n, const float* const* h0,
                                  const int64_t* cand_offs, const int32_t* cand_items, int32_t k, float* out_scores, int32_t* out_pos,
                                  float* const* out_hidden) {
    if (cand_check(m, n, cand_offs, cand_items, k, out_scores, out_pos)) return -1;
    HIPCHK(hipSetDevice(m->cfg.device));
    if (replay_check(m, hist_offs, hist_items, n, h0, out_hidden)) return -1;
    CandHost hs;
    std::vector<int> hrow;
    // chunk rows are in session order (their lists are one contiguous stretch of the CSR, their results land in place); session
    // c0 + i's hidden row is the sorted row r with perm[r] = i
    auto score = [&](int c0, int Cc, const std::vector<int>& perm, const float* hsrc) -> int {
        hrow.resize(Cc);
        for (int r = 0; r < Cc; ++r) hrow[perm[r]] = r;
        float* dst = k ? out_scores + (size_t)c0 * k : out_scores + (cand_offs[c0] - cand_offs[0]);
        return cand_enqueue(m, hsrc, Cc, hrow.data(), cand_offs + c0, cand_items, k, dst, k ? out_pos + (size_t)c0 * k : nullptr, hs);
    };
    return replay_chunks(m, hist_offs, hist_items, n, replay_chunk_rows(n), h0, out_hidden, score, [](int, int, const std::vector<int>&) {});
}

int g4r_evaluate(g4r_model* m, const int32_t* in_idx, const int32_t* out_idx, const uint8_t* reset, const int32_t* M, int64_t T,
                 int32_t batch, const int64_t* compact_steps, const int32_t* compact_maps, int64_t n_compact,
                 const int32_t* items, int64_t n_items_sel, const int32_t* cutoffs, int32_t n_cut, int32_t mode,
                 double* recall_sum, double* mrr_sum, int64_t* n_events) {
    if (!m || !in_idx || !out_idx || !reset || !M || !cutoffs || !recall_sum || !mrr_sum || !n_events) return fail("null argument");
    if (T < 0 || batch < 1 || n_cut < 1 || n_cut > 64) return fail("bad evaluation sizes");
    if (mode < 0 || mode > G4R_RANK_TIEBREAKING) return fail("unknown rank mode");
    if (n_compact > 0 && (!compact_steps || !compact_maps)) return fail("compaction arrays missing");
    DevModel& d = m->dm;
    const int B = batch;
    for (int64_t i = 0; i < T * B; ++i)
        if (in_idx[i] < 0 || in_idx[i] >= d.n_items || out_idx[i] < 0 || out_idx[i] >= d.n_items) return fail("plan item index out of range");
    for (int64_t i = 0; i < n_items_sel; ++i)
        if (items[i] < 0 || items[i] >= d.n_items) return fail("item index out of range");
    if (g4r_predict_begin(m, batch)) return -1;            // fresh (zero) hidden state, scratch for `batch` rows
    int *e_in = nullptr, *e_out = nullptr, *e_M = nullptr, *e_maps = nullptr, *e_items = nullptr, *e_cand = nullptr, *e_cut = nullptr, *e_iota = nullptr;
    unsigned char* e_reset = nullptr;
    double* e_acc = nullptr;            // [rec(n_cut) | mrr(n_cut)]
    long long* e_n = nullptr;
    const size_t TB = (size_t)std::max<int64_t>(T, 1) * B;
    auto cleanup = [&]() {
        dfree(m, e_in); dfree(m, e_out); dfree(m, e_M); dfree(m, e_maps); dfree(m, e_items); dfree(m, e_cand); dfree(m, e_cut);
        dfree(m, e_iota); dfree(m, e_reset); dfree(m, e_acc); dfree(m, e_n);
    };
    if (dalloc(m, &e_in, TB, false) || dalloc(m, &e_out, TB, false) || dalloc(m, &e_reset, TB, false) ||
        dalloc(m, &e_maps, (size_t)std::max<int64_t>(n_compact, 1) * B, false) || dalloc(m, &e_cut, n_cut, false) ||
        dalloc(m, &e_acc, 2 * (size_t)n_cut) || dalloc(m, &e_n, 1) || dalloc(m, &e_iota, B, false) ||
        (items && (dalloc(m, &e_items, (size_t)n_items_sel, false) || dalloc(m, &e_cand, (size_t)B + n_items_sel, false)))) {
        cleanup();
        return -1;
    }
#define EVCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { cleanup(); return fail(std::string(#x ": ") + hipGetErrorString(e_)); } } while (0)
    hipStream_t s = m->stream;
    if (T > 0) {
        EVCHK(hipMemcpyAsync(e_in, in_idx, TB * sizeof(int), hipMemcpyHostToDevice, s));
        EVCHK(hipMemcpyAsync(e_out, out_idx, TB * sizeof(int), hipMemcpyHostToDevice, s));
        EVCHK(hipMemcpyAsync(e_reset, reset, TB, hipMemcpyHostToDevice, s));
    }
    if (n_compact > 0) EVCHK(hipMemcpyAsync(e_maps, compact_maps, (size_t)n_compact * B * sizeof(int), hipMemcpyHostToDevice, s));
    EVCHK(hipMemcpyAsync(e_cut, cutoffs, n_cut * sizeof(int), hipMemcpyHostToDevice, s));
    if (items) EVCHK(hipMemcpyAsync(e_items, items, (size_t)n_items_sel * sizeof(int), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_iota, dim3(cdiv(B, 256)), dim3(256), 0, s, e_iota, B);
    const bool sm_act = (d.final_act == G4R_ACT_SOFTMAX || d.final_act == G4R_ACT_SOFTMAX_LOGIT);
    const bool streaming = !sm_act && !getenv("G4R_EVAL_MATERIALIZE");
    int64_t ci = 0;
    for (int64_t t = 0; t < T; ++t) {
        const int Mt = M[t];
        if (Mt < 1 || Mt > B) { cleanup(); return fail("plan M out of range"); }
        // rows of exhausted slots are dropped before this step (evaluation.py:138; gru4rec.py:647-651 for the same plan format)
        while (ci < n_compact && compact_steps[ci] == t) {
            for (int l = 0; l < d.n_layers; ++l)
                hipLaunchKernelGGL(k_gather_rows, dim3(cdiv((long long)B * d.D[l], 256)), dim3(256), 0, s, m->pH[l][m->ppar ^ 1],
                                   (const float*)m->pH[l][m->ppar], (const int*)(e_maps + ci * B), B, d.D[l]);
            m->ppar ^= 1;
            ++ci;
        }
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
            if (predict_forward(m, e_in + t * B, Mt, cand, n_sel, &sr)) { cleanup(); return -1; }
        } else {
            // softmax needs the whole row first (max, sum): scores are materialised, then ranked
            if (predict_forward(m, e_in + t * B, Mt, cand, n_sel, nullptr)) { cleanup(); return -1; }
            hipLaunchKernelGGL(k_rank_rows, dim3(Mt), dim3(256), 0, s, (const float*)m->p_scores, (long long)m->p_nsel, (long long)m->p_ldo,
                               items ? (const int*)e_iota : tgt, items ? (long long)Mt : 0LL, (int)mode, m->p_ranks,
                               (unsigned long long)m->cfg.seed, (unsigned)t);
        }
        hipLaunchKernelGGL(k_eval_accum, dim3(1), dim3(256), 0, s, (const float*)m->p_ranks, Mt, (const int*)e_cut, (int)n_cut, e_acc,
                           e_acc + n_cut, e_n);
        // hidden rows of sessions that ended with this step start from zero (evaluation.py:137)
        for (int l = 0; l < d.n_layers; ++l)
            hipLaunchKernelGGL(k_zero_rows, dim3(cdiv((long long)Mt * d.D[l], 256)), dim3(256), 0, s, m->pH[l][m->ppar],
                               (const unsigned char*)(e_reset + t * B), Mt, d.D[l]);
    }
    EVCHK(hipGetLastError());
    std::vector<double> acc(2 * (size_t)n_cut);
    long long n = 0;
    EVCHK(hipMemcpyAsync(acc.data(), e_acc, acc.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    EVCHK(hipMemcpyAsync(&n, e_n, sizeof(n), hipMemcpyDeviceToHost, s));
    EVCHK(hipStreamSynchronize(s));
#undef EVCHK
    for (int c = 0; c < n_cut; ++c) { recall_sum[c] = acc[c]; mrr_sum[c] = acc[n_cut + c]; }
    *n_events = n;
    cleanup();
    return 0;
}

// ------------------------------------------------------------------------------------------------ per-event lists and ranks
// g4r_recommend_events: g4r_evaluate's plan loop, every step's rows ranked AND their k best selected in one pass over the candidates
// (k_topk_rank: k_topk_fused with the rank counters of k_score_count).  Per step, element-wise final activation: GRU, k_score_cand
// (the Mt target scores), k_topk_rank, k_rank_counts, k_events_merge (list, rank and target score straight to the event's place),
// k_zero_rows.  softmax / softmax_logit values need the whole row: the scores are materialised as g4r_evaluate materialises them
// (k_score_store, k_softmax_rows, k_rank_rows), then selected from memory (k_topk_stored) -- two passes and more (with `items` the
// row is normalised over [targets | items] for the rank, as g4r_evaluate does, and once more over `items` alone for the list, as
// g4r_recommend_step does).  Results stay on the device until the end of the call, or of a piece of it.
int g4r_recommend_events(g4r_model* m, const int32_t* in_idx, const int32_t* out_idx, const uint8_t* reset, const int32_t* M, int64_t T,
                         int32_t batch, const int64_t* compact_steps, const int32_t* compact_maps, int64_t n_compact,
                         const int32_t* items, int64_t n_items_sel, int32_t mode, const int64_t* slot, int64_t n_slots, int32_t k,
                         const uint32_t* excl_mask, const int64_t* seen_offs, const int32_t* seen_items, const int32_t* seen_first,
                         int64_t n_seen, const int32_t* seen_sess, const int32_t* seen_pos, int32_t* out_items, float* out_scores,
                         float* out_rank, float* out_target_score) {
    // ---- every check before any device work
    if (!m || !in_idx || !out_idx || !reset || !M || !slot) return fail("null argument");
    if (T < 0 || batch < 1 || n_slots < 0) return fail("bad evaluation sizes");
    if (mode < 0 || mode > G4R_RANK_TIEBREAKING) return fail("unknown rank mode");
    if (n_compact > 0 && (!compact_steps || !compact_maps)) return fail("compaction arrays missing");
    if (items && n_items_sel < 1) return fail("n_items_sel must be positive");
    DevModel& d = m->dm;
    const int B = batch;
    const int64_t I = d.n_items, n_cand = items ? n_items_sel : I;
    if (k < 1 || k > G4R_TOPK_MAX) return fail("k must be in [1, " + std::to_string(G4R_TOPK_MAX) + "]");
    if (k > n_cand) return fail("k exceeds the number of candidates (" + std::to_string(n_cand) + ")");
    if (n_cand > INT32_MAX) return fail("more than 2^31 - 1 candidates");
    for (int64_t t = 0; t < T; ++t)
        if (M[t] < 1 || M[t] > B) return fail("plan M out of range");
    for (int64_t i = 0; i < T * B; ++i)
        if (in_idx[i] < 0 || in_idx[i] >= I || out_idx[i] < 0 || out_idx[i] >= I) return fail("plan item index out of range");
    for (int64_t i = 0; items && i < n_items_sel; ++i)
        if (items[i] < 0 || items[i] >= I) return fail("item index out of range");
    {
        std::vector<bool> used((size_t)n_slots, false);
        for (int64_t t = 0; t < T; ++t)
            for (int r = 0; r < M[t]; ++r) {
                const int64_t s = slot[t * B + r];
                if (s < 0 || s >= n_slots) return fail("slot out of range at step " + std::to_string(t) + ", row " + std::to_string(r));
                if (used[(size_t)s]) return fail("slot " + std::to_string(s) + " is used twice");
                used[(size_t)s] = true;
            }
    }
    const bool seen = seen_offs != nullptr;
    if (seen) {
        if (!seen_items || !seen_first || !seen_sess || !seen_pos || n_seen < 1) return fail("null argument (seen-item tables)");
        if (seen_offs[0] < 0 || seen_offs[n_seen] > INT32_MAX) return fail("seen_offs out of range");
        for (int64_t s = 0; s < n_seen; ++s) {
            const int64_t b = seen_offs[s], e = seen_offs[s + 1];
            if (e < b) return fail("seen_offs is not monotone at session " + std::to_string(s));
            if (e - b > G4R_EXCLUDE_MAX)
                return fail("session " + std::to_string(s) + " holds " + std::to_string(e - b) + " distinct items, more than G4R_EXCLUDE_MAX = " +
                            std::to_string(G4R_EXCLUDE_MAX));
            for (int64_t j = b; j < e; ++j) {
                if (seen_items[j] < 0 || seen_items[j] >= I) return fail("seen item index out of range in session " + std::to_string(s));
                if (j > b && seen_items[j] <= seen_items[j - 1]) return fail("the item list of session " + std::to_string(s) + " is not sorted and duplicate-free");
                if (seen_first[j] < 0) return fail("negative first position in session " + std::to_string(s));
            }
        }
        for (int64_t t = 0; t < T; ++t)
            for (int r = 0; r < M[t]; ++r)
                if (seen_sess[t * B + r] < 0 || seen_sess[t * B + r] >= n_seen || seen_pos[t * B + r] < 0)
                    return fail("seen_sess / seen_pos out of range at step " + std::to_string(t) + ", row " + std::to_string(r));
    }
    if (seen || excl_mask) {
        // eligible candidate positions of every session at its last event (the seen set only grows): refused before the state is touched
        auto masked = [&](int32_t i) { return excl_mask && ((excl_mask[i >> 5] >> (i & 31)) & 1u); };
        int64_t n_masked = 0;
        std::vector<int32_t> mult;                // with `items`: candidate positions per item index
        if (items) {
            if (seen) mult.assign((size_t)I, 0);
            for (int64_t p = 0; p < n_items_sel; ++p) {
                if (masked(items[p])) ++n_masked;
                if (seen) ++mult[items[p]];
            }
        } else if (excl_mask) {
            for (int64_t i = 0; i < I; ++i) n_masked += masked((int32_t)i) ? 1 : 0;
        }
        if (n_cand - n_masked < k)
            return fail("the exclusions leave " + std::to_string(n_cand - n_masked) + " eligible candidate positions, fewer than k = " + std::to_string(k));
        if (seen) {
            std::vector<int32_t> last((size_t)n_seen, -1);
            for (int64_t t = 0; t < T; ++t)
                for (int r = 0; r < M[t]; ++r) last[seen_sess[t * B + r]] = std::max(last[seen_sess[t * B + r]], seen_pos[t * B + r]);
            for (int64_t s = 0; s < n_seen; ++s) {
                int64_t gone = n_masked;
                for (int64_t j = seen_offs[s]; j < seen_offs[s + 1]; ++j)
                    if (seen_first[j] <= last[s] && !masked(seen_items[j])) gone += items ? mult[seen_items[j]] : 1;
                if (n_cand - gone < k)
                    return fail("session " + std::to_string(s) + " has " + std::to_string(n_cand - gone) +
                                " eligible candidate positions at its last event, fewer than k = " + std::to_string(k));
            }
        }
    }
    const bool excl = seen || excl_mask;
    const bool sm = (d.final_act == G4R_ACT_SOFTMAX || d.final_act == G4R_ACT_SOFTMAX_LOGIT);
    // ---- pieces: the lists of at most `cap` events are held on the device at a time.  One piece: an event's place is its slot and
    // the buffers go to the caller's arrays as they are; several: its place is its number within the piece, rows are sorted into
    // the slots on the host after the piece's one synchronisation
    int64_t piece_bytes = G4R_EVENTS_PIECE_BYTES;
    if (const char* e = getenv("G4R_EVENTS_PIECE")) piece_bytes = std::max<int64_t>(1, atoll(e));      // tests: results do not depend on it
    const int64_t cap_ev = std::max<int64_t>(B, piece_bytes / ((int64_t)k * 8));
    const bool one_piece = n_slots <= cap_ev;
    const int64_t cap = std::max<int64_t>(1, one_piece ? n_slots : cap_ev);
    const size_t TB = (size_t)std::max<int64_t>(T, 1) * B;
    std::vector<long long> place(TB, 0);
    std::vector<int64_t> piece_end;               // step after the last of every piece
    {
        int64_t cnt = 0;
        for (int64_t t = 0; t < T; ++t) {
            if (!one_piece && cnt + M[t] > cap) { piece_end.push_back(t); cnt = 0; }
            for (int r = 0; r < M[t]; ++r) place[t * B + r] = one_piece ? slot[t * B + r] : cnt + r;
            cnt += M[t];
        }
        piece_end.push_back(T);
    }
    std::vector<int4> hseen;
    if (seen) {
        hseen.assign(TB, make_int4(0, 0, 0, 0));
        for (int64_t t = 0; t < T; ++t)
            for (int r = 0; r < M[t]; ++r) {
                const int s = seen_sess[t * B + r];
                hseen[t * B + r] = make_int4((int)seen_offs[s], (int)(seen_offs[s + 1] - seen_offs[s]), seen_pos[t * B + r], 0);
            }
    }
    // workspace of the range lists: the largest any step needs
    auto ranges = [&](int mrows, int* tpr) {
        const int row_blocks = cdiv(mrows, SC_BM);
        const int64_t tiles = (n_cand + TK_TN - 1) / TK_TN;
        const int64_t R0 = std::min<int64_t>(std::max(1, m->n_cu / row_blocks), tiles);
        *tpr = (int)((tiles + R0 - 1) / R0);
        return (int)((tiles + *tpr - 1) / *tpr);
    };
    int64_t need = 1;
    for (int64_t t = 0; t < T; ++t) { int tpr; need = std::max<int64_t>(need, (int64_t)M[t] * ranges(M[t], &tpr) * k); }
    if (g4r_predict_begin(m, batch)) return -1;            // fresh (zero) hidden state, scratch for `batch` rows
    if (need > m->p_topk_cap) {
        dfree(m, m->p_topk);
        m->p_topk = nullptr;
        m->p_topk_cap = 0;
        if (dalloc(m, &m->p_topk, (size_t)need, false)) return -1;
        m->p_topk_cap = need;
    }
    int *e_in = nullptr, *e_out = nullptr, *e_maps = nullptr, *e_items = nullptr, *e_cand = nullptr, *e_iota = nullptr, *e_sitems = nullptr,
        *e_sfirst = nullptr, *o_items = nullptr;
    unsigned char* e_reset = nullptr;
    unsigned* e_mask = nullptr;
    long long* e_place = nullptr;
    int4 *e_seen = nullptr, *e_work = nullptr;
    float *e_ts = nullptr, *o_scores = nullptr, *o_rank = nullptr, *o_ts = nullptr;
    auto cleanup = [&]() {
        dfree(m, e_in); dfree(m, e_out); dfree(m, e_maps); dfree(m, e_items); dfree(m, e_cand); dfree(m, e_iota); dfree(m, e_sitems);
        dfree(m, e_sfirst); dfree(m, o_items); dfree(m, e_reset); dfree(m, e_mask); dfree(m, e_place); dfree(m, e_seen); dfree(m, e_work);
        dfree(m, e_ts); dfree(m, o_scores); dfree(m, o_rank); dfree(m, o_ts);
    };
    const int64_t n_sl = seen ? seen_offs[n_seen] : 0, nw = (I + 31) / 32;
    if (dalloc(m, &e_in, TB, false) || dalloc(m, &e_out, TB, false) || dalloc(m, &e_reset, TB, false) || dalloc(m, &e_place, TB, false) ||
        dalloc(m, &e_maps, (size_t)std::max<int64_t>(n_compact, 1) * B, false) || dalloc(m, &e_iota, B, false) || dalloc(m, &e_work, B, false) ||
        dalloc(m, &e_ts, B) || dalloc(m, &o_items, (size_t)cap * k) || dalloc(m, &o_scores, (size_t)cap * k) || dalloc(m, &o_rank, (size_t)cap) ||
        dalloc(m, &o_ts, (size_t)cap) || (items && dalloc(m, &e_items, (size_t)n_items_sel, false)) ||
        (items && sm && dalloc(m, &e_cand, (size_t)B + n_items_sel, false)) ||
        (seen && (dalloc(m, &e_seen, TB, false) || dalloc(m, &e_sitems, (size_t)n_sl, false) || dalloc(m, &e_sfirst, (size_t)n_sl, false))) ||
        (excl_mask && dalloc(m, &e_mask, (size_t)nw, false))) {
        cleanup();
        return -1;
    }
#define EVCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { cleanup(); return fail(std::string(#x ": ") + hipGetErrorString(e_)); } } while (0)
    hipStream_t s = m->stream;
    std::vector<int4> work((size_t)B);            // k_score_cand: row r scores one position, r, of the step's target list
    for (int r = 0; r < B; ++r) work[r] = make_int4(r, r, r + 1, r);
    if (T > 0) {
        EVCHK(hipMemcpyAsync(e_in, in_idx, TB * sizeof(int), hipMemcpyHostToDevice, s));
        EVCHK(hipMemcpyAsync(e_out, out_idx, TB * sizeof(int), hipMemcpyHostToDevice, s));
        EVCHK(hipMemcpyAsync(e_reset, reset, TB, hipMemcpyHostToDevice, s));
        EVCHK(hipMemcpyAsync(e_place, place.data(), TB * sizeof(long long), hipMemcpyHostToDevice, s));
        if (seen) EVCHK(hipMemcpyAsync(e_seen, hseen.data(), TB * sizeof(int4), hipMemcpyHostToDevice, s));
    }
    EVCHK(hipMemcpyAsync(e_work, work.data(), (size_t)B * sizeof(int4), hipMemcpyHostToDevice, s));
    if (n_compact > 0) EVCHK(hipMemcpyAsync(e_maps, compact_maps, (size_t)n_compact * B * sizeof(int), hipMemcpyHostToDevice, s));
    if (items) EVCHK(hipMemcpyAsync(e_items, items, (size_t)n_items_sel * sizeof(int), hipMemcpyHostToDevice, s));
    if (seen && n_sl > 0) {
        EVCHK(hipMemcpyAsync(e_sitems, seen_items, (size_t)n_sl * sizeof(int), hipMemcpyHostToDevice, s));
        EVCHK(hipMemcpyAsync(e_sfirst, seen_first, (size_t)n_sl * sizeof(int), hipMemcpyHostToDevice, s));
    }
    if (excl_mask) EVCHK(hipMemcpyAsync(e_mask, excl_mask, (size_t)nw * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_iota, dim3(cdiv(B, 256)), dim3(256), 0, s, e_iota, B);
    // host staging of a piece (several pieces only); unused slots of the caller's arrays read zero either way
    std::vector<int32_t> st_items;
    std::vector<float> st_scores, st_rank, st_ts;
    if (!one_piece) {
        st_items.resize((size_t)cap * k); st_scores.resize((size_t)cap * k); st_rank.resize((size_t)cap); st_ts.resize((size_t)cap);
        if (out_items) memset(out_items, 0, (size_t)n_slots * k * sizeof(int32_t));
        if (out_scores) memset(out_scores, 0, (size_t)n_slots * k * sizeof(float));
        if (out_rank) memset(out_rank, 0, (size_t)n_slots * sizeof(float));
        if (out_target_score) memset(out_target_score, 0, (size_t)n_slots * sizeof(float));
    }
    m->ev_steps = T; m->ev_scans = 0; m->ev_launches = 0; m->ev_pieces = 0;
    const int top = d.n_layers - 1;
    int64_t ci = 0, t0 = 0;
    for (size_t pc = 0; pc < piece_end.size(); ++pc) {
        for (int64_t t = t0; t < piece_end[pc]; ++t) {
            const int Mt = M[t];
            // rows of exhausted slots are dropped before this step, as in g4r_evaluate
            while (ci < n_compact && compact_steps[ci] == t) {
                for (int l = 0; l < d.n_layers; ++l)
                    hipLaunchKernelGGL(k_gather_rows, dim3(cdiv((long long)B * d.D[l], 256)), dim3(256), 0, s, m->pH[l][m->ppar ^ 1],
                                       (const float*)m->pH[l][m->ppar], (const int*)(e_maps + ci * B), B, d.D[l]);
                m->ppar ^= 1;
                m->ev_launches += d.n_layers;
                ++ci;
            }
            const int* tgt = e_out + t * B;
            const int* d_items = items ? (const int*)e_items : (const int*)nullptr;
            // the noise key of a column and of the target are g4r_evaluate's, which scores [targets | items]: column Mt + j, target i
            const int* tie_col = items ? (const int*)e_iota : tgt;
            int tpr;
            const int R = ranges(Mt, &tpr);
            const dim3 grid(R, cdiv(Mt, SC_BM));
            const TkEvents ev = {e_ts, m->p_cnt, mode == G4R_RANK_TIEBREAKING ? tie_col : (const int*)nullptr, items ? (long long)Mt : 0LL, (unsigned)t,
                                 seen ? (const int4*)(e_seen + t * B) : (const int4*)nullptr, e_sitems, e_sfirst, e_mask};
            if (!sm) {
                predict_gru(m, e_in + t * B, Mt);
                const float* hsrc = (const float*)m->phout[top];
                hipLaunchKernelGGL(k_score_cand, dim3(Mt), dim3(256), 0, s, (const DevModel*)m->d_dm, hsrc, tgt, (const int4*)e_work, e_ts, 1);
                if (excl)
                    hipLaunchKernelGGL(k_topk_rank_x, grid, dim3(256), TK_SMEM_FUSED_X + TK_SEL_EV, s, (const DevModel*)m->d_dm, hsrc, Mt, d_items,
                                       (long long)n_cand, (const float*)nullptr, 0LL, (int)k, tpr, m->p_topk, ev);
                else
                    hipLaunchKernelGGL(k_topk_rank, grid, dim3(256), TK_SMEM_FUSED, s, (const DevModel*)m->d_dm, hsrc, Mt, d_items,
                                       (long long)n_cand, (const float*)nullptr, 0LL, (int)k, tpr, m->p_topk, ev);
                hipLaunchKernelGGL(k_rank_counts, dim3(cdiv(Mt, 256)), dim3(256), 0, s, m->p_cnt, Mt, (int)mode, m->p_ranks);
                m->ev_scans += 1;
                m->ev_launches += 2 * d.n_layers + 3;
            } else {
                const int* cand = nullptr;
                int64_t n_sel = I;
                if (items) {
                    hipLaunchKernelGGL(k_eval_candidates, dim3(cdiv((long long)Mt + n_items_sel, 256)), dim3(256), 0, s, e_cand, tgt, Mt,
                                       (const int*)e_items, (long long)n_items_sel);
                    cand = e_cand;
                    n_sel = Mt + n_items_sel;
                    ++m->ev_launches;
                }
                if (predict_forward(m, e_in + t * B, Mt, cand, n_sel, nullptr)) { cleanup(); return -1; }
                hipLaunchKernelGGL(k_rank_rows, dim3(Mt), dim3(256), 0, s, (const float*)m->p_scores, (long long)m->p_nsel, (long long)m->p_ldo,
                                   tie_col, items ? (long long)Mt : 0LL, (int)mode, m->p_ranks, (unsigned long long)m->cfg.seed, (unsigned)t);
                hipLaunchKernelGGL(k_events_tscore, dim3(cdiv(Mt, 256)), dim3(256), 0, s, (const float*)m->p_scores, (long long)m->p_ldo, tie_col, Mt, e_ts);
                m->ev_scans += 3;            // k_score_store, k_softmax_rows, k_rank_rows
                m->ev_launches += 2 * d.n_layers + 4;
                int64_t ldo = m->p_ldo;
                if (items) {                  // the list's scores are normalised over `items` alone (g4r_recommend_step's)
                    ldo = (n_items_sel + 3) & ~3LL;
                    score_rows(m, (const float*)m->phout[top], Mt, d_items, n_items_sel, m->p_scores, ldo);
                    m->ev_scans += 2;
                    m->ev_launches += 2;
                }
                if (excl)
                    hipLaunchKernelGGL(k_topk_stored_ev, grid, dim3(256), TK_SMEM_STORED_X + TK_SEL_EV, s, (const DevModel*)m->d_dm, (const float*)m->phout[top],
                                       Mt, d_items, (long long)n_cand, (const float*)m->p_scores, (long long)ldo, (int)k, tpr, m->p_topk, ev);
                else
                    hipLaunchKernelGGL(k_topk_stored, grid, dim3(256), TK_SMEM_STORED, s, (const DevModel*)m->d_dm, (const float*)m->phout[top],
                                       Mt, d_items, (long long)n_cand, (const float*)m->p_scores, (long long)ldo, (int)k, tpr, m->p_topk);
                m->ev_scans += 1;
                m->ev_launches += 1;
            }
            hipLaunchKernelGGL(k_events_merge, dim3(Mt), dim3(256), 0, s, (const uint2*)m->p_topk, R, (int)k, (const long long*)(e_place + t * B), d_items,
                               (const float*)m->p_ranks, (const float*)e_ts, o_items, o_scores, o_rank, o_ts);
            // hidden rows of sessions that ended with this step start from zero
            for (int l = 0; l < d.n_layers; ++l)
                hipLaunchKernelGGL(k_zero_rows, dim3(cdiv((long long)Mt * d.D[l], 256)), dim3(256), 0, s, m->pH[l][m->ppar],
                                   (const unsigned char*)(e_reset + t * B), Mt, d.D[l]);
            m->ev_launches += 1 + d.n_layers;
        }
        EVCHK(hipGetLastError());
        // ---- the piece's results: one download, one synchronisation
        int64_t n_ev = 0;
        for (int64_t t = t0; t < piece_end[pc]; ++t) n_ev += M[t];
        const int64_t rows = one_piece ? n_slots : n_ev;
        int32_t* h_items = one_piece ? out_items : st_items.data();
        float *h_scores = one_piece ? out_scores : st_scores.data(), *h_rank = one_piece ? out_rank : st_rank.data(),
              *h_ts = one_piece ? out_target_score : st_ts.data();
        if (rows > 0) {
            if (out_items) EVCHK(hipMemcpyAsync(h_items, o_items, (size_t)rows * k * sizeof(int32_t), hipMemcpyDeviceToHost, s));
            if (out_scores) EVCHK(hipMemcpyAsync(h_scores, o_scores, (size_t)rows * k * sizeof(float), hipMemcpyDeviceToHost, s));
            if (out_rank) EVCHK(hipMemcpyAsync(h_rank, o_rank, (size_t)rows * sizeof(float), hipMemcpyDeviceToHost, s));
            if (out_target_score) EVCHK(hipMemcpyAsync(h_ts, o_ts, (size_t)rows * sizeof(float), hipMemcpyDeviceToHost, s));
        }
        EVCHK(hipStreamSynchronize(s));
        ++m->ev_pieces;
        if (!one_piece)
            for (int64_t t = t0; t < piece_end[pc]; ++t)
                for (int r = 0; r < M[t]; ++r) {
                    const size_t from = (size_t)place[t * B + r], to = (size_t)slot[t * B + r];
                    if (out_items) memcpy(out_items + to * k, st_items.data() + from * k, (size_t)k * sizeof(int32_t));
                    if (out_scores) memcpy(out_scores + to * k, st_scores.data() + from * k, (size_t)k * sizeof(float));
                    if (out_rank) out_rank[to] = st_rank[from];
                    if (out_target_score) out_target_score[to] = st_ts[from];
                }
        t0 = piece_end[pc];
    }
#undef EVCHK
    cleanup();
    return 0;
}

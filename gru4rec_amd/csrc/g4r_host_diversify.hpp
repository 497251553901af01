// g4r_host_diversify.hpp -- part of libgru4rec_hip.so's host code; included once, by g4r_api.hip (one translation unit: the kernels are templates
// instantiated there).  Holds: diversified top-k by maximal marginal relevance: the checks, the launch of k_mmr_rerank, g4r_diversify_lists
// (supplied lists) and g4r_diversify_sessions (the stage behind sessions_run's selection).
// ------------------------------------------------------------------------------------------------ diversified top-k (MMR)
// Rows per chunk of g4r_diversify_lists: one workgroup per row, sixteen rounds of one workgroup per compute unit.
#define G4R_DIVERSIFY_CHUNK_ROWS 4096

// the checks both entries share (nothing is launched): k and the pool, lam, the metric and the space -> the stage's table
static int mmr_check(g4r_model* m, int32_t space, int32_t metric, int32_t P, int32_t k, float lam, int32_t normalize, MmrStage* st) {
    if (metric != G4R_SIM_DOT && metric != G4R_SIM_COSINE) return fail("metric must be G4R_SIM_DOT (0) or G4R_SIM_COSINE (1)");
    const float* T = nullptr;
    int W = 0;
    const int tab = sim_table(m, space, &T, &W);
    if (tab < 0) return -1;
    if (P < 1 || P > G4R_DIVERSIFY_POOL_MAX) return fail("the pool must hold between 1 and G4R_DIVERSIFY_POOL_MAX = " + std::to_string(G4R_DIVERSIFY_POOL_MAX) + " candidates");
    if (k < 1 || k > P) return fail("k must be in [1, pool = " + std::to_string(P) + "]");
    if (!(lam >= 0.f && lam <= 1.f)) return fail("lam must be in [0, 1]");
    *st = MmrStage{tab, T, W, metric == G4R_SIM_COSINE, lam, normalize ? 1 : 0, k, nullptr, nullptr};
    return 0;
}

// the inverse norms (cosine) and the buffers of the picks of chunks of `rows` rows
static int mmr_prepare(g4r_model* m, const MmrStage& st, int rows) {
    if (st.cosine && sim_norms_ensure(m, st.tab, st.T, st.W)) return -1;
    const int64_t n = (int64_t)rows * st.k;
    return (m->dv_pos.reserve(m, n) || m->dv_val.reserve(m, n) || m->dv_cols.reserve(m, n) || m->dv_scores.reserve(m, n)) ? -1 : 0;
}

// k_mmr_rerank over `rows` pools of P (columns, relevance), enqueued only; map / n_cols: the columns' items (NULL: the columns are items)
static int mmr_launch(g4r_model* m, const MmrStage& st, int rows, int P, const int* cols, const float* rel, const int* map, int64_t n_cols,
                      int* out_cols, float* out_rel) {
    const float* inv = st.cosine ? (const float*)m->sim_inv[st.tab] : (const float*)nullptr;
    auto kern = st.cosine ? k_mmr_rerank<true> : k_mmr_rerank<false>;
    hipLaunchKernelGGL(kern, dim3((unsigned)rows), dim3(256), MMR_SMEM(P), m->stream, st.T, st.W, (int)m->dm.n_items, cols, rel, map,
                       (long long)n_cols, inv, P, st.k, st.lam, st.normalize, m->dv_pos.p, m->dv_val.p, out_cols, out_rel);
    HIPCHK(hipGetLastError());
    return 0;
}

// sessions_run's stage: the pools are the selection's lists in p_tcols / p_tscores
static int mmr_enqueue(g4r_model* m, const MmrStage& st, int rows, int pool, const int* d_items, int64_t n_sel) {
    return mmr_launch(m, st, rows, pool, (const int*)m->p_tcols.p, (const float*)m->p_tscores.p, d_items, n_sel, m->dv_cols.p, m->dv_scores.p);
}

int g4r_diversify_lists(g4r_model* m, int32_t space, int32_t metric, const int32_t* items, const float* rel, int64_t n, int32_t P,
                        int32_t k, float lam, int32_t normalize, int32_t* out_pos, float* out_value) {
    // ---- every check before any device work
    if (!m || !items || !rel || !out_pos || !out_value) return fail("null argument");
    MmrStage st;
    if (mmr_check(m, space, metric, P, k, lam, normalize, &st)) return -1;
    if (n < 1) return fail("n must be positive");
    const int64_t I = m->dm.n_items;
    for (int64_t e = 0; e < n * P; ++e) {
        if (items[e] < 0 || items[e] >= I) return fail("item index out of range (list " + std::to_string(e / P) + ")");
        if (!std::isfinite(rel[e])) return fail("relevance that is not finite (list " + std::to_string(e / P) + ")");
    }
    HIPCHK(hipSetDevice(m->cfg.device));
    // ---- chunk by chunk: upload the lists, pick, copy the picks back (one synchronisation per chunk)
    const int C = (int)std::min<int64_t>(n, G4R_DIVERSIFY_CHUNK_ROWS);
    if (mmr_prepare(m, st, C) || m->dv_items.reserve(m, (int64_t)C * P) || m->dv_rel.reserve(m, (int64_t)C * P)) return -1;
    for (int64_t c0 = 0; c0 < n; c0 += C) {
        const int Cc = (int)std::min<int64_t>(C, n - c0);
        HIPCHK(hipMemcpyAsync(m->dv_items.p, items + c0 * P, (size_t)Cc * P * sizeof(int), hipMemcpyHostToDevice, m->stream));
        HIPCHK(hipMemcpyAsync(m->dv_rel.p, rel + c0 * P, (size_t)Cc * P * sizeof(float), hipMemcpyHostToDevice, m->stream));
        if (mmr_launch(m, st, Cc, P, (const int*)m->dv_items.p, (const float*)m->dv_rel.p, nullptr, I, nullptr, nullptr)) return -1;
        HIPCHK(hipMemcpyAsync(out_pos + c0 * k, m->dv_pos.p, (size_t)Cc * k * sizeof(int), hipMemcpyDeviceToHost, m->stream));
        HIPCHK(hipMemcpyAsync(out_value + c0 * k, m->dv_val.p, (size_t)Cc * k * sizeof(float), hipMemcpyDeviceToHost, m->stream));
        HIPCHK(hipStreamSynchronize(m->stream));
    }
    return 0;
}

int g4r_diversify_sessions(g4r_model* m, const int64_t* hist_offs, const int32_t* hist_items, int32_t n, const float* const* h0,
                           const int32_t* item_idx, int64_t n_sel, int32_t k, int32_t pool, int32_t oversample,
                           const int64_t* excl_offs, const int32_t* excl_items, const uint32_t* excl_mask, int32_t space,
                           int32_t metric, float lam, int32_t normalize, int32_t* out_cols, float* out_scores, int32_t* out_pos,
                           float* out_value, float* const* out_hidden) {
    if (!out_pos || !out_value) return fail("null argument");
    if (recommend_check(m, item_idx, n_sel, pool, out_cols, out_scores)) return -1;
    if (oversample < 0) return fail("oversample must be 0 (the exact selection) or at least 1");
    MmrStage st;
    if (mmr_check(m, space, metric, pool, k, lam, normalize, &st)) return -1;
    st.out_pos = out_pos;
    st.out_value = out_value;
    return sessions_run(m, hist_offs, hist_items, n, h0, item_idx, n_sel, pool, oversample, 0, 0, excl_offs, excl_items, excl_mask, out_cols,
                        out_scores, out_hidden, &st);
}

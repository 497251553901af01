// g4r_host_similar.hpp -- part of libgru4rec_hip.so's host code; included once, by g4r_api.hip (one translation unit: the kernels are templates
// instantiated there).  Holds: g4r_similar_items (item-to-item neighbours in the model's own embedding space).
// ------------------------------------------------------------------------------------------------ item neighbours
// Rows per chunk of g4r_similar_items: 32 row blocks of 128 query rows, which with one column range per XCD is one workgroup per
// compute unit, every range of the table read by the 32 workgroups of one XCD.  G4R_SIM_CHUNK > 0 (read per call) forces a smaller
// chunk: tests show the results do not depend on it.
#define G4R_SIM_CHUNK_ROWS 4096

// the item table of a space: 0 = Wy, 1 = E; -1 (with the reason set) where the model has none
static int sim_table(g4r_model* m, int32_t space, const float** T, int* W) {
    const DevModel& d = m->dm;
    if (space != G4R_SPACE_OUTPUT && space != G4R_SPACE_INPUT) { fail("space must be G4R_SPACE_OUTPUT (0) or G4R_SPACE_INPUT (1)"); return -1; }
    if (space == G4R_SPACE_OUTPUT || d.embed_mode == G4R_EMBED_CONSTRAINED) { *T = d.Wy; *W = d.Dtop; return 0; }
    if (d.embed_mode == G4R_EMBED_SEPARATE) { *T = d.E; *W = d.Ein; return 1; }
    fail("space = input: a one-hot input model has no input embedding (layer 0 reads a row of its weights per item, three gates wide, "
         "not an embedding of the item); use G4R_SPACE_OUTPUT");
    return -1;
}

// the inverse norms of table `tab`, (re)built on the stream when anything may have changed the table since the last build
static int sim_norms_ensure(g4r_model* m, int tab, const float* T, int W) {
    if (m->sim_valid[tab]) return 0;
    const int64_t I = m->dm.n_items;
    if (!m->sim_inv[tab] && dalloc(m, &m->sim_inv[tab], (size_t)I, false)) return -1;
    hipLaunchKernelGGL(k_item_norms, dim3((unsigned)((I + 16 * SIM_ROWS_PER_GROUP - 1) / (16 * SIM_ROWS_PER_GROUP))), dim3(256), 0, m->stream, T,
                       (long long)I, W, m->sim_inv[tab]);
    HIPCHK(hipGetLastError());
    m->sim_valid[tab] = true;
    ++m->sim_builds;
    return 0;
}

int g4r_similar_items(g4r_model* m, int32_t space, int32_t metric, const int32_t* q_idx, int64_t n, const int32_t* item_idx, int64_t n_sel,
                      int32_t k, int32_t exclude_self, const uint32_t* excl_mask, int32_t* out_cols, float* out_scores) {
    // ---- every check before any device work (cand_upload, among them, stages the candidate items: no state to advance)
    if (!m || !q_idx || !out_cols || !out_scores) return fail("null argument");
    if (metric != G4R_SIM_DOT && metric != G4R_SIM_COSINE) return fail("metric must be G4R_SIM_DOT (0) or G4R_SIM_COSINE (1)");
    const float* T = nullptr;
    int W = 0;
    const int tab = sim_table(m, space, &T, &W);
    if (tab < 0) return -1;
    if (n < 1) return fail("n must be positive");
    const DevModel& d = m->dm;
    const int64_t I = d.n_items, n_cand = item_idx ? n_sel : I;
    if (item_idx && n_sel < 1) return fail("n_sel must be positive");
    if (k < 1 || k > G4R_TOPK_MAX) return fail("k must be in [1, " + std::to_string(G4R_TOPK_MAX) + "]");
    if (k > n_cand) return fail("k exceeds the number of candidates (n_sel = " + std::to_string(n_cand) + ")");
    if (n_cand > INT32_MAX) return fail("more than 2^31 - 1 candidates");
    for (int64_t i = 0; i < n; ++i)
        if (q_idx[i] < 0 || q_idx[i] >= I) return fail("query item index out of range (query " + std::to_string(i) + ")");
    HIPCHK(hipSetDevice(m->cfg.device));
    const int* d_items = nullptr;
    if (cand_upload(m, item_idx, &n_sel, &d_items)) return -1;
    // eligible candidate positions of a query: all - the positions of masked items - (exclude_self) the positions of its own item
    auto masked = [&](int32_t i) { return excl_mask && ((excl_mask[i >> 5] >> (i & 31)) & 1u); };
    int64_t n_masked = 0;
    std::vector<int32_t> uq;       // with a candidate list and exclude_self: the distinct query items, sorted,
    std::vector<int64_t> own;      // and the number of unmasked candidate positions holding each
    auto query_slot = [&](int32_t i) { return (size_t)(std::lower_bound(uq.begin(), uq.end(), i) - uq.begin()); };
    if (item_idx) {
        if (exclude_self) {
            uq.assign(q_idx, q_idx + n);
            std::sort(uq.begin(), uq.end());
            uq.erase(std::unique(uq.begin(), uq.end()), uq.end());
            own.assign(uq.size(), 0);
        }
        for (int64_t p = 0; p < n_sel; ++p) {
            if (masked(item_idx[p])) ++n_masked;
            else if (exclude_self) {
                const size_t s = query_slot(item_idx[p]);
                if (s < uq.size() && uq[s] == item_idx[p]) ++own[s];
            }
        }
    } else if (excl_mask) {
        const int64_t nw = (I + 31) / 32;
        for (int64_t w = 0; w < nw; ++w) {
            const uint32_t valid = (w == nw - 1 && (I & 31)) ? ((1u << (I & 31)) - 1u) : 0xFFFFFFFFu;
            n_masked += __builtin_popcount(excl_mask[w] & valid);
        }
    }
    for (int64_t i = 0; i < n; ++i) {
        const int64_t gone = n_masked + ((exclude_self && !masked(q_idx[i])) ? (item_idx ? own[query_slot(q_idx[i])] : 1) : 0);
        if (n_cand - gone < k)
            return fail("query " + std::to_string(i) + " (item index " + std::to_string(q_idx[i]) + ") has " + std::to_string(n_cand - gone) +
                        " eligible candidate positions, fewer than k = " + std::to_string(k));
    }
    // ---- buffers and the call-wide uploads
    const int env_c = env_int("G4R_SIM_CHUNK", 0);
    const int C = (int)std::min<int64_t>(n, env_c > 0 ? std::min(env_c, G4R_SIM_CHUNK_ROWS) : G4R_SIM_CHUNK_ROWS);
    const bool cosine = metric == G4R_SIM_COSINE;
    if (cosine && sim_norms_ensure(m, tab, T, W)) return -1;
    TkExcl ex{};
    if (excl_mask && excl_upload(m, false, std::vector<long long>(), std::vector<int32_t>(), excl_mask, &ex)) return -1;
    if (m->sim_q.reserve(m, (int64_t)C) || m->sim_rows.reserve(m, (int64_t)C * W) || m->p_tcols.reserve(m, (int64_t)C * k) ||
        m->p_tscores.reserve(m, (int64_t)C * k))
        return -1;
    // ---- chunk by chunk: upload the query items, gather their rows, scan, merge, copy the chunk's rows back (one synchronisation per chunk)
    for (int64_t c0 = 0; c0 < n; c0 += C) {
        const int Cc = (int)std::min<int64_t>(C, n - c0);
        // row blocks x column ranges, about one workgroup per compute unit
        const TkRanges g = tk_ranges(m, Cc, n_cand, TK_TN);
        const int RB = g.row_blocks, tpr = g.tpr, R = g.R;
        if (m->p_topk.reserve(m, (int64_t)Cc * R * k)) return -1;      // (grows on the first chunk at most, and on a shorter last one)
        HIPCHK(hipMemcpyAsync(m->sim_q.p, q_idx + c0, Cc * sizeof(int), hipMemcpyHostToDevice, m->stream));
        hipLaunchKernelGGL(k_sim_gather, dim3(cdiv((long long)Cc * (W / 4), 256)), dim3(256), 0, m->stream, T, W, (const int*)m->sim_q.p, Cc, m->sim_rows.p);
        const dim3 grid((unsigned)(R * RB));
        if (cosine)
            hipLaunchKernelGGL(k_sim_range<true>, grid, dim3(256), SIM_SMEM, m->stream, T, W, (int)I, (const int*)m->sim_q.p, (const float*)m->sim_rows.p, Cc, d_items,
                               (long long)n_cand, (const float*)m->sim_inv[tab], ex.mask, exclude_self ? 1 : 0, (int)k, tpr, R, RB, m->p_topk.p);
        else
            hipLaunchKernelGGL(k_sim_range<false>, grid, dim3(256), SIM_SMEM, m->stream, T, W, (int)I, (const int*)m->sim_q.p, (const float*)m->sim_rows.p, Cc, d_items,
                               (long long)n_cand, (const float*)nullptr, ex.mask, exclude_self ? 1 : 0, (int)k, tpr, R, RB, m->p_topk.p);
        hipLaunchKernelGGL(k_topk_merge, dim3(Cc), dim3(256), 0, m->stream, (const uint2*)m->p_topk.p, R, (int)k, m->p_tcols.p, m->p_tscores.p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(out_cols + c0 * k, m->p_tcols.p, (size_t)Cc * k * sizeof(int), hipMemcpyDeviceToHost, m->stream));
        HIPCHK(hipMemcpyAsync(out_scores + c0 * k, m->p_tscores.p, (size_t)Cc * k * sizeof(float), hipMemcpyDeviceToHost, m->stream));
        HIPCHK(hipStreamSynchronize(m->stream));
    }
    return 0;
}

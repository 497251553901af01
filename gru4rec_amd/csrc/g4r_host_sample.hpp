// g4r_host_sample.hpp -- part of libgru4rec_hip.so's host code; included once, by g4r_api.hip (one translation unit: the kernels are templates
// instantiated there).  Holds: g4r_sample_sessions, stochastic decoding of session continuations (kernels: g4r_sample_kernels.cuh).
// ------------------------------------------------------------------------------------------------ sampling after a replay
// Per chunk of Cc sessions (replay_chunks): the replay on Cc rows, k_sample_expand, then every step -- step 0 included -- on
// rows = Cc x samples draw rows: (GRU step, from step 1 on) -> selection -> k_topk_merge -> k_sample_pick -> (k_score_cand, untruncated)
// -> k_rollout_feed with k = 1.  One synchronisation and one download per chunk whatever steps and samples are.
//   untruncated   k_topk_sample (k = 1) selects on the key; the merge returns (column, key), so the chosen column's z is recomputed
//                 by k_score_cand's chain: 5 launches per step beside the GRU's
//   top_k = t     k_topk_fused_g (k = t, the exact selection in its fused form, whatever the final activation) returns the t best
//                 (column, z); k_sample_pick takes the argmax of the key over them: 4 launches per step beside the GRU's
// Hidden states: as in g4r_beam_sessions the chain leaves the replay's two halves.  k_sample_expand gathers every session's final state
// (from the half its own history length picks) into `rio`; GRU step s reads half (s - 1) & 1 of (rio, rH[.][0]) and writes the other.
// The top layer's output of the draw rows at step 0 is the expanded copy in rz[top] (GRU scratch, idle until step 1).
// Exclusion lists: every draw row owns a copy of its session's list with steps - 1 slots of slack behind it (no_repeat), laid out per
// chunk on the host (the growing form of excl_chunk, one list per draw); without lists every row's is empty.
int g4r_sample_sessions(g4r_model* m, const int64_t* hist_offs, const int32_t* hist_items, int32_t n, const float* const* h0,
                        const int32_t* item_idx, int64_t n_sel, int32_t steps, int32_t no_repeat, const int64_t* excl_offs,
                        const int32_t* excl_items, const uint32_t* excl_mask, int32_t samples, int32_t top_k, float temperature,
                        uint64_t seed, int32_t first_step, int32_t* out_cols, float* out_scores, float* const* out_hidden) {
    // ---- every check before any kernel is launched (as sessions_run)
    if (!m) return fail("null argument");
    if (samples < 1 || samples > G4R_SAMPLE_MAX) return fail("samples must be in [1, G4R_SAMPLE_MAX = " + std::to_string(G4R_SAMPLE_MAX) + "]");
    if (top_k < 0 || top_k > G4R_TOPK_MAX) return fail("top_k must be 0 (no truncation) or in [1, " + std::to_string(G4R_TOPK_MAX) + "]");
    const int32_t k = top_k ? top_k : 1;
    if (recommend_check(m, item_idx, n_sel, k, out_cols, out_scores)) return -1;
    if (steps < 1) return fail("steps must be at least 1");
    const float invT = 1.0f / temperature;
    if (!(temperature > 0.f) || !std::isfinite(temperature) || !std::isfinite(invT))
        return fail("temperature must be a finite float > 0 with a finite reciprocal (the greedy limit is g4r_continue_sessions with k = 1)");
    if (first_step < 0 || (int64_t)first_step + steps > INT32_MAX) return fail("first_step must be >= 0 and first_step + steps at most 2^31 - 1");
    if (n >= 1 && (int64_t)n * samples > INT32_MAX) return fail("n * samples exceeds 2^31 - 1");
    HIPCHK(hipSetDevice(m->cfg.device));
    if (replay_check(m, hist_offs, hist_items, n, h0, out_hidden)) return -1;
    const DevModel& d = m->dm;
    const int* d_items;
    if (cand_upload(m, item_idx, &n_sel, &d_items)) return -1;
    const bool grow = no_repeat != 0 && steps > 1;      // the lists gain items on the device
    if (no_repeat && no_repeat_check(m, item_idx, n_sel)) return -1;
    std::vector<long long> xoffs;
    std::vector<int32_t> xitems;
    if ((excl_offs || excl_mask || grow) &&
        excl_pack(m, n, item_idx, n_sel, k, excl_offs, excl_items, excl_mask, xoffs, xitems, grow ? steps - 1 : 0))
        return -1;
    // ---- buffers: C sessions per chunk, so that C x samples draw rows fit the replay buffers
    const int S = samples, L = d.n_layers, slack = grow ? steps - 1 : 0;
    const int C = std::min(replay_chunk_rows(n), std::max(1, G4R_REPLAY_CHUNK / S));
    const int64_t rows_max = (int64_t)C * S;
    int64_t list_room = 1;      // the largest chunk's lists
    for (int c0 = 0; c0 < n; c0 += C) {
        const int c1 = std::min<int>(n, c0 + C);
        const int64_t held = excl_offs ? xoffs[c1] - xoffs[c0] : 0;
        list_room = std::max<int64_t>(list_room, (held + (int64_t)(c1 - c0) * slack) * S);
    }
    const int64_t nw = ((int64_t)d.n_items + 31) / 32;
    if (replay_reserve(m, (int)rows_max, 0)) return -1;
    if (m->ro_cols.reserve(m, rows_max * steps) || m->ro_scores.reserve(m, rows_max * steps) || m->ro_in.reserve(m, rows_max) ||
        m->ro_xlen.reserve(m, rows_max) || m->p_xoffs.reserve(m, rows_max) || m->p_xitems.reserve(m, list_room) ||
        (excl_mask && m->p_xmask.reserve(m, nw)) || m->sm_rowid.reserve(m, rows_max) || m->sm_pick.reserve(m, 2 * rows_max) ||
        m->sm_z.reserve(m, rows_max) || (!top_k && m->c_work.reserve(m, rows_max)))
        return -1;
    {      // the selection's own arrays at their largest chunk, so that no step of the chain has to grow (and drain the stream for) them
        const TkRanges g = tk_ranges(m, (int)rows_max, n_sel, TK_TN);
        if (m->p_topk.reserve(m, rows_max * g.R * k) || m->p_tcols.reserve(m, rows_max * k) || m->p_tscores.reserve(m, rows_max * k)) return -1;
    }
    if (excl_mask) HIPCHK(hipMemcpyAsync(m->p_xmask.p, excl_mask, (size_t)nw * sizeof(uint32_t), hipMemcpyHostToDevice, m->stream));
    const unsigned* d_mask = excl_mask ? (const unsigned*)m->p_xmask.p : nullptr;
    std::vector<int32_t> tcols((size_t)rows_max * steps);
    std::vector<float> tscores((size_t)rows_max * steps);
    std::vector<std::vector<float>> thid(out_hidden ? L : 0);
    for (int l = 0; l < (int)thid.size(); ++l) thid[l].resize((size_t)rows_max * d.D[l]);
    std::vector<unsigned> rowid;
    std::vector<long long> beg;
    std::vector<int32_t> litems, llen;
    std::vector<int4> work;
    float* bH[G4R_MAX_LAYERS][2];      // the chain's ping-pong
    BeamState from_replay{};
    from_replay.n_layers = L;
    for (int l = 0; l < L; ++l) {
        bH[l][0] = m->rio[l];
        bH[l][1] = m->rH[l][0];
        from_replay.src[l] = m->rH[l][0]; from_replay.src1[l] = m->rH[l][1];
        from_replay.dst[l] = m->rio[l];
        from_replay.W[l] = d.D[l];
    }
    const GruBufs bb{bH, m->rhout, m->rVc, m->rz, m->rHr};
    int* pick_col = m->sm_pick.p;
    // ---- chunk by chunk
    auto score = [&](int c0, int Cc, const std::vector<int>& perm, const float* hsess) -> int {
        const int rows = Cc * S;
        int* pick_item = pick_col + rows;
        // draw row r S + j: its row id (the caller's session index), its list
        rowid.resize(rows);
        beg.resize(rows);
        llen.resize(rows);
        litems.clear();
        for (int r = 0; r < Cc; ++r) {
            const int64_t i = (int64_t)c0 + perm[r];
            for (int j = 0; j < S; ++j) {
                rowid[(size_t)r * S + j] = (unsigned)(i * S + j);
                beg[(size_t)r * S + j] = (long long)litems.size();
                if (excl_offs) litems.insert(litems.end(), xitems.begin() + xoffs[i], xitems.begin() + xoffs[i + 1]);
                llen[(size_t)r * S + j] = excl_offs ? (int32_t)(xoffs[i + 1] - xoffs[i]) : 0;
                litems.insert(litems.end(), (size_t)slack, 0);
            }
        }
        HIPCHK(hipMemcpyAsync(m->sm_rowid.p, rowid.data(), (size_t)rows * sizeof(unsigned), hipMemcpyHostToDevice, m->stream));
        HIPCHK(hipMemcpyAsync(m->p_xoffs.p, beg.data(), (size_t)rows * sizeof(long long), hipMemcpyHostToDevice, m->stream));
        HIPCHK(hipMemcpyAsync(m->ro_xlen.p, llen.data(), (size_t)rows * sizeof(int), hipMemcpyHostToDevice, m->stream));
        if (!litems.empty()) HIPCHK(hipMemcpyAsync(m->p_xitems.p, litems.data(), litems.size() * sizeof(int32_t), hipMemcpyHostToDevice, m->stream));
        if (!top_k) {      // k_score_cand's work items: row r's list is the one position r
            work.resize(rows);
            for (int r = 0; r < rows; ++r) work[r] = make_int4(r, r, r + 1, r);
            HIPCHK(hipMemcpyAsync(m->c_work.p, work.data(), (size_t)rows * sizeof(int4), hipMemcpyHostToDevice, m->stream));
        }
        const TkGrow gx{(const long long*)m->p_xoffs.p, (const int*)m->ro_xlen.p, (const int*)m->p_xitems.p, d_mask};
        hipLaunchKernelGGL(k_sample_expand, dim3(rows), dim3(64), 0, m->stream, from_replay, (const int*)m->r_len, S, hsess, m->rz[L - 1], d.Dtop);
        const TkRanges g = tk_ranges(m, rows, n_sel, TK_TN);
        if (m->p_topk.reserve(m, (int64_t)rows * g.R * k)) return -1;
        const dim3 grid(g.R, g.row_blocks);
        for (int s = 0; s < steps; ++s) {
            if (s > 0) gru_step(m, bb, (s - 1) & 1, (const int*)m->ro_in.p, rows);
            const float* hsrc = s > 0 ? (const float*)m->rhout[L - 1] : (const float*)m->rz[L - 1];
            const unsigned step = (unsigned)(first_step + s);
            if (top_k)
                hipLaunchKernelGGL(k_topk_fused_g, grid, dim3(256), TK_SMEM_FUSED_X, m->stream, (const DevModel*)m->d_dm, hsrc, rows, d_items,
                                   (long long)n_sel, (const float*)nullptr, 0LL, (int)k, g.tpr, m->p_topk.p, gx);
            else
                hipLaunchKernelGGL(k_topk_sample, grid, dim3(256), TK_SMEM_SAMPLE, m->stream, (const DevModel*)m->d_dm, hsrc, rows, d_items,
                                   (long long)n_sel, (const float*)nullptr, 0LL, 1, g.tpr, m->p_topk.p,
                                   TkSample{gx.beg, gx.len, gx.items, gx.mask, (const unsigned*)m->sm_rowid.p, (unsigned long long)seed, step, invT});
            hipLaunchKernelGGL(k_topk_merge, dim3(rows), dim3(256), 0, m->stream, (const uint2*)m->p_topk.p, g.R, (int)k, m->p_tcols.p, m->p_tscores.p);
            hipLaunchKernelGGL(k_sample_pick, dim3(rows), dim3(64), 0, m->stream, (const int*)m->p_tcols.p, (const float*)m->p_tscores.p, (int)k,
                               top_k ? 1 : 0, d_items, (const unsigned*)m->sm_rowid.p, (unsigned long long)seed, step, invT, pick_col, pick_item,
                               m->sm_z.p);
            if (!top_k)
                hipLaunchKernelGGL(k_score_cand, dim3(rows), dim3(256), 0, m->stream, (const DevModel*)m->d_dm, hsrc, (const int*)pick_item,
                                   (const int4*)m->c_work.p, m->sm_z.p, 1);
            const bool last = s == steps - 1;
            hipLaunchKernelGGL(k_rollout_feed, dim3(rows), dim3(64), 0, m->stream, (const int*)pick_col, (const float*)m->sm_z.p, 1, (int)steps, s,
                               d_items, m->ro_cols.p, m->ro_scores.p, last ? (int*)nullptr : m->ro_in.p, gx.beg,
                               (last || !grow) ? (int*)nullptr : m->ro_xlen.p, m->p_xitems.p);
        }
        HIPCHK(hipGetLastError());
        for (int l = 0; l < (int)thid.size(); ++l)      // the state that produced the last step's scores
            HIPCHK(hipMemcpyAsync(thid[l].data(), bH[l][(steps - 1) & 1], (size_t)rows * d.D[l] * sizeof(float), hipMemcpyDeviceToHost, m->stream));
        HIPCHK(hipMemcpyAsync(tcols.data(), m->ro_cols.p, (size_t)rows * steps * sizeof(int), hipMemcpyDeviceToHost, m->stream));
        HIPCHK(hipMemcpyAsync(tscores.data(), m->ro_scores.p, (size_t)rows * steps * sizeof(float), hipMemcpyDeviceToHost, m->stream));
        return 0;
    };
    // draw row r S + j of the chunk is draw (c0 + perm[r], j)
    auto done = [&](int c0, int Cc, const std::vector<int>& perm) {
        for (int r = 0; r < Cc; ++r) {
            const size_t src = (size_t)r * S, dst = ((size_t)c0 + perm[r]) * S;
            memcpy(out_cols + dst * steps, tcols.data() + src * steps, (size_t)S * steps * sizeof(int32_t));
            memcpy(out_scores + dst * steps, tscores.data() + src * steps, (size_t)S * steps * sizeof(float));
            for (int l = 0; l < (int)thid.size(); ++l)
                memcpy(out_hidden[l] + dst * d.D[l], thid[l].data() + src * d.D[l], (size_t)S * d.D[l] * sizeof(float));
        }
    };
    return replay_chunks(m, hist_offs, hist_items, n, C, h0, nullptr, score, done);
}

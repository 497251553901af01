// g4r_host_sample.hpp -- part of libgru4rec_hip.so's host code; included once, by g4r_api.hip (one translation unit: the kernels are templates
// instantiated there).  Holds: g4r_sample_sessions(_lp), stochastic decoding of session continuations with its log-probabilities and
// nucleus, and g4r_session_log_partition (kernels: g4r_sample_kernels.cuh).
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
// Log-probabilities and the nucleus (g4r_sample_sessions_lp; the contract: include/gru4rec_hip.h).  Both rest on the row normaliser Q, the
// exact integer sum of lse_term over the row's eligible positions, formed by the scan itself relative to zeta, the row's largest eligible
// z -- which costs the untruncated path a second scan per step:
//   untruncated + out_logprobs   k_topk_fused_g (k = 1) -> k_topk_merge (zeta) -> zero Q -> k_topk_sample_q (the draw + Q) -> k_topk_merge
//                                -> k_sample_pick -> k_score_cand -> k_sample_logprob -> k_rollout_feed
//   top_k + top_p                k_topk_fused_g (k = t) -> k_topk_merge -> zero Q -> k_topk_fused_q (k = 1, its lists unused: Q) ->
//                                k_sample_pick_lp (nucleus, choice, log-probability) -> k_rollout_feed
//   top_k + out_logprobs only    no extra scan: k_sample_pick_lp takes its mass from the t best
// The log-probabilities go to [row][s] of sm_lp and come down with the paths.  top_p = 0 and out_logprobs = NULL (g4r_sample_sessions):
// the launches and the bits of before.
// more candidate positions than this and Q, at most 2^39 a term, could pass 2^63
#define G4R_LSE_CAND_MAX (1LL << 24)
static int sample_run(g4r_model* m, const int64_t* hist_offs, const int32_t* hist_items, int32_t n, const float* const* h0,
                      const int32_t* item_idx, int64_t n_sel, int32_t steps, int32_t no_repeat, const int64_t* excl_offs,
                      const int32_t* excl_items, const uint32_t* excl_mask, int32_t samples, int32_t top_k, float temperature,
                      uint64_t seed, int32_t first_step, int32_t* out_cols, float* out_scores, float* const* out_hidden, float top_p,
                      float* out_logprobs) {
    // ---- every check before any kernel is launched (as sessions_run)
    if (!m) return fail("null argument");
    if (!(top_p >= 0.f && top_p <= 1.f)) return fail("top_p must be 0 (no nucleus) or in (0, 1]");
    if (top_p > 0.f && !top_k) return fail("top_p needs top_k: the nucleus is sought among the top_k best");
    const bool lp = out_logprobs != nullptr, nucleus = top_p > 0.f;
    if ((lp || nucleus) && (item_idx ? n_sel : (int64_t)m->dm.n_items) > G4R_LSE_CAND_MAX)
        return fail("log-probabilities and top_p take at most 2^24 candidate positions (the exact row normaliser is a 64-bit integer)");
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
    if ((lp || nucleus) && (m->sm_zeta.reserve(m, rows_max) || m->sm_zcol.reserve(m, rows_max) || m->sm_Q.reserve(m, rows_max) ||
                            m->sm_lp.reserve(m, rows_max * steps)))
        return -1;
    {      // the selection's own arrays at their largest chunk, so that no step of the chain has to grow (and drain the stream for) them
        const TkRanges g = tk_ranges(m, (int)rows_max, n_sel, TK_TN);
        if (m->p_topk.reserve(m, rows_max * g.R * k) || m->p_tcols.reserve(m, rows_max * k) || m->p_tscores.reserve(m, rows_max * k)) return -1;
    }
    if (excl_mask) HIPCHK(hipMemcpyAsync(m->p_xmask.p, excl_mask, (size_t)nw * sizeof(uint32_t), hipMemcpyHostToDevice, m->stream));
    const unsigned* d_mask = excl_mask ? (const unsigned*)m->p_xmask.p : nullptr;
    std::vector<int32_t> tcols((size_t)rows_max * steps);
    std::vector<float> tscores((size_t)rows_max * steps);
    std::vector<float> tlp(lp ? (size_t)rows_max * steps : 0);
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
        TkRanges g;
        if (tk_reserve(m, rows, n_sel, TK_TN, k, &g)) return -1;
        auto range = [&](const float* hsrc, int kk, auto x) { tk_launch<false, true>(m, m->stream, g, hsrc, rows, d_items, n_sel, nullptr, 0, kk, x); };
        for (int s = 0; s < steps; ++s) {
            if (s > 0) gru_step(m, bb, (s - 1) & 1, (const int*)m->ro_in.p, rows);
            const float* hsrc = s > 0 ? (const float*)m->rhout[L - 1] : (const float*)m->rz[L - 1];
            const unsigned step = (unsigned)(first_step + s);
            const TkSample sx{gx.beg, gx.len, gx.items, gx.mask, (const unsigned*)m->sm_rowid.p, (unsigned long long)seed, step, invT};
            if (top_k)
                range(hsrc, k, gx);                                                                         // k_topk_fused_g
            else if (lp) {      // zeta first: the exact selection's top-1, then the draw's scan forms Q relative to it
                range(hsrc, 1, gx);
                hipLaunchKernelGGL(k_topk_merge, dim3(rows), dim3(256), 0, m->stream, (const uint2*)m->p_topk.p, g.R, 1, m->sm_zcol.p, m->sm_zeta.p);
                HIPCHK(hipMemsetAsync(m->sm_Q.p, 0, (size_t)rows * sizeof(unsigned long long), m->stream));
                range(hsrc, 1, TkSampleLse{sx, TkLse{(const float*)m->sm_zeta.p, 1, m->sm_Q.p, invT}});     // k_topk_sample_q
            } else
                range(hsrc, 1, sx);                                                                         // k_topk_sample
            hipLaunchKernelGGL(k_topk_merge, dim3(rows), dim3(256), 0, m->stream, (const uint2*)m->p_topk.p, g.R, (int)k, m->p_tcols.p, m->p_tscores.p);
            if (nucleus) {      // Q over the whole eligible set, relative to the list's first z; the k = 1 lists it leaves in p_topk are not read
                HIPCHK(hipMemsetAsync(m->sm_Q.p, 0, (size_t)rows * sizeof(unsigned long long), m->stream));
                range(hsrc, 1, TkGrowLse{gx, TkLse{(const float*)m->p_tscores.p, (int)k, m->sm_Q.p, invT}});     // k_topk_fused_q
            }
            if (top_k && (lp || nucleus))
                hipLaunchKernelGGL(k_sample_pick_lp, dim3(rows), dim3(64), 0, m->stream, (const int*)m->p_tcols.p, (const float*)m->p_tscores.p, (int)k,
                                   d_items, (const unsigned*)m->sm_rowid.p, (unsigned long long)seed, step, invT, top_p,
                                   (const unsigned long long*)m->sm_Q.p, pick_col, pick_item, m->sm_z.p, m->sm_lp.p, (int)steps, s);
            else
                hipLaunchKernelGGL(k_sample_pick, dim3(rows), dim3(64), 0, m->stream, (const int*)m->p_tcols.p, (const float*)m->p_tscores.p, (int)k,
                                   top_k ? 1 : 0, d_items, (const unsigned*)m->sm_rowid.p, (unsigned long long)seed, step, invT, pick_col, pick_item,
                                   m->sm_z.p);
            if (!top_k)
                hipLaunchKernelGGL(k_score_cand, dim3(rows), dim3(256), 0, m->stream, (const DevModel*)m->d_dm, hsrc, (const int*)pick_item,
                                   (const int4*)m->c_work.p, m->sm_z.p, 1);
            if (!top_k && lp)
                hipLaunchKernelGGL(k_sample_logprob, dim3(cdiv(rows, 256)), dim3(256), 0, m->stream, (const float*)m->sm_z.p, (const float*)m->sm_zeta.p,
                                   (const unsigned long long*)m->sm_Q.p, invT, rows, (int)steps, s, m->sm_lp.p);
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
        if (lp) HIPCHK(hipMemcpyAsync(tlp.data(), m->sm_lp.p, (size_t)rows * steps * sizeof(float), hipMemcpyDeviceToHost, m->stream));
        return 0;
    };
    // draw row r S + j of the chunk is draw (c0 + perm[r], j)
    auto done = [&](int c0, int Cc, const std::vector<int>& perm) {
        for (int r = 0; r < Cc; ++r) {
            const size_t src = (size_t)r * S, dst = ((size_t)c0 + perm[r]) * S;
            memcpy(out_cols + dst * steps, tcols.data() + src * steps, (size_t)S * steps * sizeof(int32_t));
            memcpy(out_scores + dst * steps, tscores.data() + src * steps, (size_t)S * steps * sizeof(float));
            if (lp) memcpy(out_logprobs + dst * steps, tlp.data() + src * steps, (size_t)S * steps * sizeof(float));
            for (int l = 0; l < (int)thid.size(); ++l)
                memcpy(out_hidden[l] + dst * d.D[l], thid[l].data() + src * d.D[l], (size_t)S * d.D[l] * sizeof(float));
        }
    };
    return replay_chunks(m, hist_offs, hist_items, n, C, h0, nullptr, score, done);
}

int g4r_sample_sessions(g4r_model* m, const int64_t* hist_offs, const int32_t* hist_items, int32_t n, const float* const* h0,
                        const int32_t* item_idx, int64_t n_sel, int32_t steps, int32_t no_repeat, const int64_t* excl_offs,
                        const int32_t* excl_items, const uint32_t* excl_mask, int32_t samples, int32_t top_k, float temperature,
                        uint64_t seed, int32_t first_step, int32_t* out_cols, float* out_scores, float* const* out_hidden) {
    return sample_run(m, hist_offs, hist_items, n, h0, item_idx, n_sel, steps, no_repeat, excl_offs, excl_items, excl_mask, samples, top_k,
                      temperature, seed, first_step, out_cols, out_scores, out_hidden, 0.f, nullptr);
}

int g4r_sample_sessions_lp(g4r_model* m, const int64_t* hist_offs, const int32_t* hist_items, int32_t n, const float* const* h0,
                           const int32_t* item_idx, int64_t n_sel, int32_t steps, int32_t no_repeat, const int64_t* excl_offs,
                           const int32_t* excl_items, const uint32_t* excl_mask, int32_t samples, int32_t top_k, float temperature,
                           uint64_t seed, int32_t first_step, int32_t* out_cols, float* out_scores, float* const* out_hidden, float top_p,
                           float* out_logprobs) {
    return sample_run(m, hist_offs, hist_items, n, h0, item_idx, n_sel, steps, no_repeat, excl_offs, excl_items, excl_mask, samples, top_k,
                      temperature, seed, first_step, out_cols, out_scores, out_hidden, top_p, out_logprobs);
}

// ------------------------------------------------------------------------------------------------ the log-partition after a replay
// Per chunk: the replay, the exact selection with k = 1 (k_topk_fused_g + k_topk_merge: zeta, the row's largest eligible z -- the
// pre-activation value for softmax / softmax_logit, as in g4r_sample_sessions), zero Q, k_topk_fused_q.  out_zeta[n], out_Q[n]:
// lse = zeta * invT + log(Q * 2^-39) is the log of the sum of exp(z * invT) over the session's eligible candidate positions.
int g4r_session_log_partition(g4r_model* m, const int64_t* hist_offs, const int32_t* hist_items, int32_t n, const float* const* h0,
                              const int32_t* item_idx, int64_t n_sel, const int64_t* excl_offs, const int32_t* excl_items,
                              const uint32_t* excl_mask, float temperature, float* out_zeta, uint64_t* out_Q) {
    if (!m || !out_zeta || !out_Q) return fail("null argument");
    int32_t dummy = 0;      // (recommend_check only looks at its output pointers for NULL)
    if (recommend_check(m, item_idx, n_sel, 1, &dummy, out_zeta)) return -1;
    const float invT = 1.0f / temperature;
    if (!(temperature > 0.f) || !std::isfinite(temperature) || !std::isfinite(invT))
        return fail("temperature must be a finite float > 0 with a finite reciprocal");
    if ((item_idx ? n_sel : (int64_t)m->dm.n_items) > G4R_LSE_CAND_MAX)
        return fail("the log-partition takes at most 2^24 candidate positions (the exact row normaliser is a 64-bit integer)");
    HIPCHK(hipSetDevice(m->cfg.device));
    if (replay_check(m, hist_offs, hist_items, n, h0, nullptr)) return -1;
    const int* d_items;
    if (cand_upload(m, item_idx, &n_sel, &d_items)) return -1;
    std::vector<long long> xoffs;
    std::vector<int32_t> xitems;
    if ((excl_offs || excl_mask) && excl_pack(m, n, item_idx, n_sel, 1, excl_offs, excl_items, excl_mask, xoffs, xitems)) return -1;
    const int C = replay_chunk_rows(n);
    const int64_t nw = ((int64_t)m->dm.n_items + 31) / 32;
    {
        const TkRanges g = tk_ranges(m, C, n_sel, TK_TN);
        if (m->p_topk.reserve(m, (int64_t)C * g.R)) return -1;
    }
    if (m->sm_zeta.reserve(m, C) || m->sm_zcol.reserve(m, C) || m->sm_Q.reserve(m, C) || m->p_xoffs.reserve(m, C) || m->ro_xlen.reserve(m, C) ||
        (excl_mask && m->p_xmask.reserve(m, nw)))
        return -1;
    if (excl_mask) HIPCHK(hipMemcpyAsync(m->p_xmask.p, excl_mask, (size_t)nw * sizeof(uint32_t), hipMemcpyHostToDevice, m->stream));
    std::vector<float> tz((size_t)C);
    std::vector<unsigned long long> tq((size_t)C);
    std::vector<long long> coffs;
    std::vector<int32_t> citems, clen;
    auto score = [&](int c0, int Cc, const std::vector<int>& perm, const float* hsrc) -> int {
        // the lists in their growing layout (every row's begin and length) with no slack: nothing is fed back here
        excl_chunk(xoffs, xitems, excl_offs != nullptr, c0, Cc, perm, 0, coffs, citems, clen);
        if (m->p_xitems.reserve(m, (int64_t)citems.size())) return -1;
        HIPCHK(hipMemcpyAsync(m->p_xoffs.p, coffs.data(), (size_t)Cc * sizeof(long long), hipMemcpyHostToDevice, m->stream));
        HIPCHK(hipMemcpyAsync(m->ro_xlen.p, clen.data(), (size_t)Cc * sizeof(int), hipMemcpyHostToDevice, m->stream));
        if (!citems.empty()) HIPCHK(hipMemcpyAsync(m->p_xitems.p, citems.data(), citems.size() * sizeof(int32_t), hipMemcpyHostToDevice, m->stream));
        const TkGrow gx{(const long long*)m->p_xoffs.p, (const int*)m->ro_xlen.p, (const int*)m->p_xitems.p,
                        excl_mask ? (const unsigned*)m->p_xmask.p : nullptr};
        TkRanges g;
        if (tk_reserve(m, Cc, n_sel, TK_TN, 1, &g)) return -1;
        tk_launch<false, true>(m, m->stream, g, hsrc, Cc, d_items, n_sel, nullptr, 0, 1, gx);      // k_topk_fused_g
        hipLaunchKernelGGL(k_topk_merge, dim3(Cc), dim3(256), 0, m->stream, (const uint2*)m->p_topk.p, g.R, 1, m->sm_zcol.p, m->sm_zeta.p);
        HIPCHK(hipMemsetAsync(m->sm_Q.p, 0, (size_t)Cc * sizeof(unsigned long long), m->stream));
        tk_launch<false, true>(m, m->stream, g, hsrc, Cc, d_items, n_sel, nullptr, 0, 1,
                               TkGrowLse{gx, TkLse{(const float*)m->sm_zeta.p, 1, m->sm_Q.p, invT}});      // k_topk_fused_q
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(tz.data(), m->sm_zeta.p, (size_t)Cc * sizeof(float), hipMemcpyDeviceToHost, m->stream));
        HIPCHK(hipMemcpyAsync(tq.data(), m->sm_Q.p, (size_t)Cc * sizeof(unsigned long long), hipMemcpyDeviceToHost, m->stream));
        return 0;
    };
    auto done = [&](int c0, int Cc, const std::vector<int>& perm) {
        for (int r = 0; r < Cc; ++r) {
            out_zeta[(size_t)c0 + perm[r]] = tz[r];
            out_Q[(size_t)c0 + perm[r]] = tq[r];
        }
    };
    return replay_chunks(m, hist_offs, hist_items, n, C, h0, nullptr, score, done);
}

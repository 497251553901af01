// g4r_host_audience.hpp -- part of libgru4rec_hip.so's host code; included once, by g4r_api.hip (one translation unit: the kernels are templates
// instantiated there).  Holds: g4r_audience_sessions, the k sessions with the largest value for each of M items (kernels:
// g4r_audience_kernels.cuh; the contract: include/gru4rec_hip.h).
// ------------------------------------------------------------------------------------------------ audience selection after a replay
// Per chunk of Cc sessions (replay_chunks): the replay, then
//   k_score_cand        z[Cc][M], the M items for every row (row r's list is the M items: g4r_predict_step's bit pattern)
//   by = LOGPROB only   g4r_session_log_partition's launches: k_topk_fused_g (k = 1) -> k_topk_merge (zeta) -> zero Q -> k_topk_fused_q
//   k_audience_keys     one entry per (item, row): eligibility, the value, the key with the session's index c0 + perm[r]
//   k_audience_merge    every item's Cc entries into its running list
// Nothing is downloaded per chunk; replay_chunks' one synchronisation per chunk stays.  After the last chunk k_audience_finish unpacks
// the lists and M x k (session, value) pairs and the M counts come down, once.  g4r_profile: the two audience kernels are timed with
// event pairs (slots k_audience_keys / k_audience_merge of g4r_kernel_time), read after each chunk's synchronisation.
extern "C++" {      // (this file is included inside extern "C")
template <class... P, class... A>
static void aud_launch(g4r_model* m, int kn, void (*kern)(P...), dim3 grid, A... a) {
    if (m->profiling) {
        const size_t e = kn == KN_AUD_KEYS ? 0 : 2;
        hipExtLaunchKernelGGL(kern, grid, dim3(256), 0, m->stream, m->evs[e], m->evs[e + 1], 0, static_cast<P>(a)...);
    } else
        hipLaunchKernelGGL(kern, grid, dim3(256), 0, m->stream, static_cast<P>(a)...);
}
}  // extern "C++"

int g4r_audience_sessions(g4r_model* m, const int64_t* hist_offs, const int32_t* hist_items, int32_t n, const float* const* h0,
                          const int32_t* items, int32_t n_items, int32_t k, int32_t by, float temperature, int32_t exclude_history,
                          int32_t* out_sessions, float* out_values, int32_t* out_counts) {
    // ---- every check before any kernel is launched (as sessions_run)
    if (!m || !items || !out_sessions || !out_values || !out_counts) return fail("null argument");
    const DevModel& d = m->dm;
    const int M = n_items;
    if (M < 1 || M > G4R_AUDIENCE_ITEMS_MAX) return fail("the number of items must be in [1, G4R_AUDIENCE_ITEMS_MAX = " + std::to_string(G4R_AUDIENCE_ITEMS_MAX) + "]");
    if (k < 1 || k > G4R_AUDIENCE_MAX) return fail("k must be in [1, G4R_AUDIENCE_MAX = " + std::to_string(G4R_AUDIENCE_MAX) + "]");
    if ((int64_t)M * k > G4R_AUDIENCE_ENTRIES_MAX)
        return fail("items x k = " + std::to_string((int64_t)M * k) + " exceeds G4R_AUDIENCE_ENTRIES_MAX = " + std::to_string((long long)G4R_AUDIENCE_ENTRIES_MAX));
    if (by != G4R_AUDIENCE_SCORE && by != G4R_AUDIENCE_LOGPROB) return fail("by must be G4R_AUDIENCE_SCORE or G4R_AUDIENCE_LOGPROB");
    const bool lp = by == G4R_AUDIENCE_LOGPROB, excl = exclude_history != 0;
    if (!lp && is_softmax(d))
        return fail("G4R_AUDIENCE_SCORE is not implemented for softmax / softmax_logit final activations (a score needs its whole row): use G4R_AUDIENCE_LOGPROB");
    float invT = 1.f;
    if (lp) {
        invT = 1.0f / temperature;
        if (!(temperature > 0.f) || !std::isfinite(temperature) || !std::isfinite(invT))
            return fail("temperature must be a finite float > 0 with a finite reciprocal");
        if ((int64_t)d.n_items > G4R_LSE_CAND_MAX)
            return fail("G4R_AUDIENCE_LOGPROB takes at most 2^24 items (the exact row normaliser is a 64-bit integer)");
    }
    for (int j = 0; j < M; ++j)
        if (items[j] < 0 || items[j] >= d.n_items) return fail("item index out of range");
    HIPCHK(hipSetDevice(m->cfg.device));
    if (replay_check(m, hist_offs, hist_items, n, h0, nullptr)) return -1;
    std::vector<long long> xoffs;
    std::vector<int32_t> xitems;
    // the sessions' sorted distinct history items; LOGPROB: every session keeps at least one item in its normaliser
    if (excl && excl_pack(m, n, nullptr, 0, lp ? 1 : 0, hist_offs, hist_items, nullptr, xoffs, xitems)) return -1;
    // ---- buffers
    const int C = replay_chunk_rows(n);
    const int slices = cdiv(M, CS_SLICE);
    const int64_t n_sel = d.n_items, MK = (int64_t)M * k;
    int64_t list_room = 1;      // the largest chunk's lists
    if (excl)
        for (int c0 = 0; c0 < n; c0 += C) list_room = std::max<int64_t>(list_room, xoffs[std::min<int>(n, c0 + C)] - xoffs[c0]);
    if (m->c_items.reserve(m, (int64_t)C * M) || m->c_scores.reserve(m, (int64_t)C * M) || m->c_work.reserve(m, (int64_t)C * slices) ||
        m->au_ent.reserve(m, (int64_t)C * M) || m->au_list[0].reserve(m, MK) || m->au_list[1].reserve(m, MK) || m->au_state.reserve(m, 4LL * M) ||
        m->au_sess.reserve(m, MK) || m->au_val.reserve(m, MK))
        return -1;
    if ((lp || excl) && (m->p_xoffs.reserve(m, C) || m->ro_xlen.reserve(m, C) || m->p_xitems.reserve(m, list_room))) return -1;
    if (lp) {
        const TkRanges g = tk_ranges(m, C, n_sel, TK_TN);
        if (m->p_topk.reserve(m, (int64_t)C * g.R) || m->sm_zeta.reserve(m, C) || m->sm_zcol.reserve(m, C) || m->sm_Q.reserve(m, C)) return -1;
    }
    if (m->profiling)
        while (m->evs.size() < 4) { hipEvent_t e; HIPCHK(hipEventCreate(&e)); m->evs.push_back(e); }
    // row r of a chunk scores the M items: positions [r M, (r + 1) M) of c_items / c_scores, whatever the chunk
    std::vector<int32_t> rep((size_t)C * M);
    std::vector<int4> work;
    for (int r = 0; r < C; ++r) {
        memcpy(rep.data() + (size_t)r * M, items, (size_t)M * sizeof(int32_t));
        for (int p = 0; p < M; p += CS_SLICE) work.push_back(make_int4(r, r * M + p, r * M + std::min(p + CS_SLICE, M), r * M));
    }
    HIPCHK(hipMemcpyAsync(m->c_items.p, rep.data(), rep.size() * sizeof(int32_t), hipMemcpyHostToDevice, m->stream));
    HIPCHK(hipMemcpyAsync(m->c_work.p, work.data(), work.size() * sizeof(int4), hipMemcpyHostToDevice, m->stream));
    HIPCHK(hipMemsetAsync(m->au_state.p, 0, 4 * (size_t)M * sizeof(int), m->stream));      // every list: side 0, empty
    std::vector<long long> coffs;
    std::vector<int32_t> citems, clen;
    int chunks = 0;
    // (side, len) of the lists before chunk number c: the half the merge reads, the other one it writes
    auto state = [&](int c) { return m->au_state.p + (size_t)(c & 1) * 2 * M; };
    auto score = [&](int c0, int Cc, const std::vector<int>& perm, const float* hsrc) -> int {
        if (lp || excl) {      // the lists in their growing layout (every row's begin and length) with no slack, as g4r_session_log_partition
            excl_chunk(xoffs, xitems, excl, c0, Cc, perm, 0, coffs, citems, clen);
            HIPCHK(hipMemcpyAsync(m->p_xoffs.p, coffs.data(), (size_t)Cc * sizeof(long long), hipMemcpyHostToDevice, m->stream));
            HIPCHK(hipMemcpyAsync(m->ro_xlen.p, clen.data(), (size_t)Cc * sizeof(int), hipMemcpyHostToDevice, m->stream));
            if (!citems.empty()) HIPCHK(hipMemcpyAsync(m->p_xitems.p, citems.data(), citems.size() * sizeof(int32_t), hipMemcpyHostToDevice, m->stream));
        }
        hipLaunchKernelGGL(k_score_cand, dim3((unsigned)(Cc * slices)), dim3(256), 0, m->stream, (const DevModel*)m->d_dm, hsrc, (const int*)m->c_items.p,
                           (const int4*)m->c_work.p, m->c_scores.p, 1);
        if (lp) {
            const TkGrow gx{(const long long*)m->p_xoffs.p, (const int*)m->ro_xlen.p, (const int*)m->p_xitems.p, (const unsigned*)nullptr};
            TkRanges g;
            if (tk_reserve(m, Cc, n_sel, TK_TN, 1, &g)) return -1;
            tk_launch<false, true>(m, m->stream, g, hsrc, Cc, nullptr, n_sel, nullptr, 0, 1, gx);      // k_topk_fused_g
            hipLaunchKernelGGL(k_topk_merge, dim3(Cc), dim3(256), 0, m->stream, (const uint2*)m->p_topk.p, g.R, 1, m->sm_zcol.p, m->sm_zeta.p);
            HIPCHK(hipMemsetAsync(m->sm_Q.p, 0, (size_t)Cc * sizeof(unsigned long long), m->stream));
            tk_launch<false, true>(m, m->stream, g, hsrc, Cc, nullptr, n_sel, nullptr, 0, 1,
                                   TkGrowLse{gx, TkLse{(const float*)m->sm_zeta.p, 1, m->sm_Q.p, invT}});      // k_topk_fused_q
        }
        aud_launch(m, KN_AUD_KEYS, k_audience_keys, dim3(cdiv((long long)Cc * M, 256)), m->c_scores.p, m->c_items.p, M, Cc, m->r_perm, c0,
                   excl ? m->p_xoffs.p : nullptr, excl ? m->ro_xlen.p : nullptr, excl ? m->p_xitems.p : nullptr, lp ? m->sm_zeta.p : nullptr,
                   lp ? m->sm_Q.p : nullptr, invT, m->au_ent.p);
        int P = 2;
        while (P < Cc) P <<= 1;
        aud_launch(m, KN_AUD_MERGE, k_audience_merge, dim3(cdiv(k, AUD_TILE), M), m->au_ent.p, Cc, P, (int)k, m->au_list[0].p, m->au_list[1].p,
                   state(chunks), state(chunks) + M, state(chunks + 1), state(chunks + 1) + M);
        ++chunks;
        return 0;
    };
    auto done = [&](int, int, const std::vector<int>&) {
        if (!m->profiling) return;
        for (int q = 0; q < 2; ++q) {
            float ms = 0.f;
            const int kn = q ? KN_AUD_MERGE : KN_AUD_KEYS;
            if (hipEventElapsedTime(&ms, m->evs[2 * q], m->evs[2 * q + 1]) == hipSuccess) { m->kn_ms[kn] += ms; m->kn_n[kn]++; }
        }
    };
    if (replay_chunks(m, hist_offs, hist_items, n, C, h0, nullptr, score, done)) return -1;
    // ---- the lists come down once
    hipLaunchKernelGGL(k_audience_finish, dim3(cdiv(k, 256), M), dim3(256), 0, m->stream, (const ulonglong2*)m->au_list[0].p,
                       (const ulonglong2*)m->au_list[1].p, (const int*)state(chunks), (const int*)state(chunks) + M, (int)k, m->au_sess.p, m->au_val.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out_sessions, m->au_sess.p, (size_t)MK * sizeof(int32_t), hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipMemcpyAsync(out_values, m->au_val.p, (size_t)MK * sizeof(float), hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipMemcpyAsync(out_counts, state(chunks) + M, (size_t)M * sizeof(int32_t), hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    return 0;
}

// g4r_host_beam.hpp -- part of libgru4rec_hip.so's host code; included once, by g4r_api.hip (one translation unit: the kernels are templates
// instantiated there).  Holds: g4r_beam_sessions, beam search over session continuations (kernels: g4r_beam_kernels.cuh).
// ------------------------------------------------------------------------------------------------ beam search after a replay
// Per chunk of Cc sessions (replay_chunks): the replay and step 0's selection (k = beams) on Cc rows, k_beam_expand, then steps - 1
// rounds on rows = Cc x beams beam rows of (GRU step -> selection with k = beams -> k_beam_select -> k_beam_advance).  One
// synchronisation and one download per chunk whatever steps and beams are.
// Hidden states: the chain does not alternate between the replay's two halves.  k_beam_expand gathers every session's final state
// (from the half its own history length picks) into `rio`, the replay's staging rows, idle once the replay has begun; every GRU step
// reads rio and writes rH[.][0]; k_beam_advance gathers the parents' rows from rH[.][0] back into rio.
// Exclusion lists: step 0 reads the sessions' CSR lists (TkExcl).  With no_repeat and steps > 1 every beam row owns a list with room
// for the steps - 1 items it gains, at the same place in each of two buffers: k_beam_expand fills buffer 0, every k_beam_advance reads
// the parents' lists in the current buffer and writes the other.  Without no_repeat the beam rows of a session alias the session's
// one list through TkGrow's beg / len.
int g4r_beam_sessions(g4r_model* m, const int64_t* hist_offs, const int32_t* hist_items, int32_t n, const float* const* h0,
                      const int32_t* item_idx, int64_t n_sel, int32_t beams, int32_t oversample, int32_t steps, int32_t no_repeat,
                      int32_t combine, const int64_t* excl_offs, const int32_t* excl_items, const uint32_t* excl_mask,
                      int32_t* out_parent, int32_t* out_cols, float* out_step_scores, float* out_path_scores, int32_t* out_scale_exp) {
    // ---- every check before any kernel is launched (as sessions_run)
    if (!m || !out_parent || !out_path_scores || !out_scale_exp) return fail("null argument");
    if (beams < 1 || beams > G4R_BEAM_MAX) return fail("beams must be in [1, " + std::to_string(G4R_BEAM_MAX) + "]");
    if (recommend_check(m, item_idx, n_sel, beams, out_cols, out_step_scores)) return -1;
    if (steps < 1) return fail("steps must be at least 1");
    if (oversample < 0) return fail("oversample must be 0 (the exact selection) or at least 1");
    if (combine != G4R_BEAM_SUM && combine != G4R_BEAM_PRODUCT) return fail("combine must be G4R_BEAM_SUM or G4R_BEAM_PRODUCT");
    const DevModel& d = m->dm;
    const bool sm = is_softmax(d);
    if (combine == G4R_BEAM_PRODUCT && !sm) return fail("G4R_BEAM_PRODUCT needs softmax scores (final activation softmax / softmax_logit)");
    int32_t scan_c = 0;
    if (oversample && scan_check(m, item_idx, n_sel, beams, oversample, &scan_c)) return -1;
    HIPCHK(hipSetDevice(m->cfg.device));
    if (replay_check(m, hist_offs, hist_items, n, h0, nullptr)) return -1;
    const int* d_items;
    if (cand_upload(m, item_idx, &n_sel, &d_items)) return -1;
    const bool grow = no_repeat != 0 && steps > 1;      // the lists gain items on the device
    if (no_repeat && no_repeat_check(m, item_idx, n_sel)) return -1;
    std::vector<long long> xoffs;
    std::vector<int32_t> xitems;
    const bool excl = excl_offs || excl_mask || grow;
    if (excl && excl_pack(m, n, item_idx, n_sel, beams, excl_offs, excl_items, excl_mask, xoffs, xitems, grow ? steps - 1 : 0)) return -1;
    const bool lists = excl_offs || grow;
    // ---- buffers: C sessions per chunk, so that C x beams beam rows fit the replay buffers
    const int W = beams, L = d.n_layers;
    const int C = std::min(replay_chunk_rows(n), std::max(1, G4R_REPLAY_CHUNK / W));
    const int64_t rows_max = (int64_t)C * W, ldo = (n_sel + 3) & ~3LL;
    if (replay_reserve(m, (int)rows_max, 0)) return -1;
    if (sm && m->r_scores.reserve(m, rows_max * ldo)) return -1;
    int64_t list_room = 0;      // the largest chunk's beam lists (a chunk's sessions do not depend on the order replay_chunks steps them in)
    if (grow)
        for (int c0 = 0; c0 < n; c0 += C) {
            const int c1 = std::min<int>(n, c0 + C);
            const int64_t held = excl_offs ? xoffs[c1] - xoffs[c0] : 0;
            list_room = std::max<int64_t>(list_room, (held + (int64_t)(c1 - c0) * (steps - 1)) * W);
        }
    const int64_t out_words = (3LL * steps + 1) * rows_max + C;
    if (m->bm_out.reserve(m, out_words) || m->bm_in.reserve(m, rows_max) || m->bm_sel.reserve(m, 2 * rows_max) ||
        (lists && steps > 1 && (m->bm_beg.reserve(m, rows_max) || m->bm_xlen.reserve(m, 2 * rows_max))) ||
        (grow && m->bm_xitems.reserve(m, 2 * list_room)))
        return -1;
    if (!scan_c) {      // the selection's own arrays at their largest, so that no step of the chain has to grow (and drain the stream for) them
        const TkRanges g = tk_ranges(m, (int)rows_max, n_sel, TK_TN);
        if (m->p_topk.reserve(m, rows_max * g.R * W) || m->p_tcols.reserve(m, rows_max * W) || m->p_tscores.reserve(m, rows_max * W)) return -1;
    }
    std::vector<int32_t> hout((size_t)out_words);
    std::vector<long long> coffs, beg;
    std::vector<int32_t> citems, clen, blen;
    float* bH[G4R_MAX_LAYERS][2];      // the chain's ping-pong: every GRU step reads half 0 (rio), writes half 1 (rH[.][0])
    BeamState from_replay{}, from_step{};
    from_replay.n_layers = from_step.n_layers = L;
    for (int l = 0; l < L; ++l) {
        bH[l][0] = m->rio[l];
        bH[l][1] = m->rH[l][0];
        from_replay.src[l] = m->rH[l][0]; from_replay.src1[l] = m->rH[l][1];
        from_step.src[l] = from_step.src1[l] = m->rH[l][0];
        from_replay.dst[l] = from_step.dst[l] = m->rio[l];
        from_replay.W[l] = from_step.W[l] = d.D[l];
    }
    const GruBufs bb{bH, m->rhout, m->rVc, m->rz, m->rHr};
    const int product = combine == G4R_BEAM_PRODUCT ? 1 : 0;
    auto select = [&](const float* hsrc, int mrows, const TkExcl* exp, const TkGrow* gxp, bool work_ready) -> int {
        if (sm) score_rows(m, hsrc, mrows, d_items, n_sel, m->r_scores.p, ldo);
        if (scan_c > 0) return topk_select_scan(m, hsrc, mrows, d_items, n_sel, W, scan_c, exp, gxp, work_ready);
        return topk_select(m, hsrc, mrows, d_items, n_sel, W, exp, (const float*)m->r_scores.p, ldo, gxp);
    };
    // ---- chunk by chunk
    auto score = [&](int c0, int Cc, const std::vector<int>& perm, const float* hsrc) -> int {
        const int rows = Cc * W;
        const size_t SR = (size_t)steps * rows;
        int* o_parent = m->bm_out.p;
        int* o_col = o_parent + SR;
        float* o_score = reinterpret_cast<float*>(o_col + SR);
        float* o_cum = o_score + SR;
        int* o_exp = reinterpret_cast<int*>(o_cum + rows);
        TkExcl ex{};
        if (excl) {
            if (lists) excl_chunk(xoffs, xitems, excl_offs != nullptr, c0, Cc, perm, -1, coffs, citems, clen);
            if (excl_upload(m, lists, coffs, citems, excl_mask, &ex)) return -1;
        }
        const bool blists = lists && steps > 1;      // the beam rows read per-row lists
        int64_t room = 0;                            // ints of one list buffer
        if (blists) {
            beg.resize(rows);
            blen.assign((size_t)2 * rows, 0);
            for (int r = 0; r < Cc; ++r) {
                const long long held = coffs[r + 1] - coffs[r];
                for (int i = 0; i < W; ++i) {
                    beg[(size_t)r * W + i] = grow ? room + i * (held + steps - 1) : coffs[r];
                    blen[(size_t)r * W + i] = (int32_t)held;      // (grow: k_beam_expand writes the lengths)
                }
                room += W * (held + steps - 1);
            }
            HIPCHK(hipMemcpyAsync(m->bm_beg.p, beg.data(), (size_t)rows * sizeof(long long), hipMemcpyHostToDevice, m->stream));
            if (!grow) HIPCHK(hipMemcpyAsync(m->bm_xlen.p, blen.data(), (size_t)rows * sizeof(int), hipMemcpyHostToDevice, m->stream));
        }
        // step 0 on the Cc session rows, then the sessions become their beam rows
        if (select(hsrc, Cc, excl ? &ex : nullptr, nullptr, false)) return -1;
        hipLaunchKernelGGL(k_beam_expand, dim3(rows), dim3(64), 0, m->stream, (const int*)m->p_tcols.p, (const float*)m->p_tscores.p, W, d_items,
                           from_replay, (const int*)m->r_len, product, steps > 1 ? 1 : 0, o_cum, o_exp, m->bm_in.p, o_parent, o_col, o_score,
                           ex.offs, ex.items, grow ? (const long long*)m->bm_beg.p : (const long long*)nullptr,
                           grow ? m->bm_xlen.p : (int*)nullptr, grow ? m->bm_xitems.p : (int*)nullptr);
        int cur = 0;      // the list buffer that holds the beam rows' lists (grow)
        for (int s = 1; s < steps; ++s) {
            gru_step(m, bb, 0, (const int*)m->bm_in.p, rows);
            TkGrow gx{};
            if (blists)
                gx = grow ? TkGrow{(const long long*)m->bm_beg.p, (const int*)m->bm_xlen.p + (size_t)cur * rows,
                                   (const int*)m->bm_xitems.p + (size_t)cur * room, ex.mask}
                          : TkGrow{(const long long*)m->bm_beg.p, (const int*)m->bm_xlen.p, ex.items, ex.mask};
            if (select(hsrc, rows, (excl && !blists) ? &ex : nullptr, blists ? &gx : nullptr, s > 1)) return -1;
            hipLaunchKernelGGL(k_beam_select, dim3(Cc), dim3(256), 0, m->stream, (const int*)m->p_tcols.p, (const float*)m->p_tscores.p, W, d_items,
                               product, o_cum, o_exp, m->bm_sel.p, m->bm_sel.p + rows, o_parent + (size_t)s * rows, o_col + (size_t)s * rows,
                               o_score + (size_t)s * rows);
            if (s == steps - 1) break;
            hipLaunchKernelGGL(k_beam_advance, dim3(rows), dim3(64), 0, m->stream, (const int*)m->bm_sel.p, (const int*)m->bm_sel.p + rows, W,
                               from_step, m->bm_in.p, gx.beg, grow ? gx.len : (const int*)nullptr, gx.items,
                               grow ? m->bm_xlen.p + (size_t)(cur ^ 1) * rows : (int*)nullptr,
                               grow ? m->bm_xitems.p + (size_t)(cur ^ 1) * room : (int*)nullptr);
            cur ^= 1;
        }
        HIPCHK(hipMemcpyAsync(hout.data(), m->bm_out.p, (3 * SR + rows + Cc) * sizeof(int32_t), hipMemcpyDeviceToHost, m->stream));
        return 0;
    };
    // sorted row r is session c0 + perm[r]: its records [step][beam] and its beams' path scores
    auto done = [&](int c0, int Cc, const std::vector<int>& perm) {
        const int rows = Cc * W;
        const size_t SR = (size_t)steps * rows;
        const int32_t* h_parent = hout.data();
        const int32_t* h_col = h_parent + SR;
        const float* h_score = reinterpret_cast<const float*>(h_col + SR);
        const float* h_cum = h_score + SR;
        const int32_t* h_exp = reinterpret_cast<const int32_t*>(h_cum + rows);
        for (int r = 0; r < Cc; ++r) {
            const size_t i = (size_t)c0 + perm[r];
            for (int s = 0; s < steps; ++s) {
                const size_t src = (size_t)s * rows + (size_t)r * W, dst = (i * steps + s) * W;
                memcpy(out_parent + dst, h_parent + src, (size_t)W * sizeof(int32_t));
                memcpy(out_cols + dst, h_col + src, (size_t)W * sizeof(int32_t));
                memcpy(out_step_scores + dst, h_score + src, (size_t)W * sizeof(float));
            }
            memcpy(out_path_scores + i * W, h_cum + (size_t)r * W, (size_t)W * sizeof(float));
            out_scale_exp[i] = h_exp[r];
        }
    };
    return replay_chunks(m, hist_offs, hist_items, n, C, h0, nullptr, score, done);
}

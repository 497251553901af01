// g4r_host_events.hpp -- part of libgru4rec_hip.so's host code; included once, by g4r_api.hip (one translation unit: the kernels are templates
// instantiated there).  Holds: g4r_recommend_events (per-event top-k lists and target ranks of a whole test set).
// ------------------------------------------------------------------------------------------------ per-event lists and ranks
// g4r_recommend_events: g4r_evaluate's plan loop, every step's rows ranked AND their k best selected in one pass over the candidates
// (k_topk_rank: k_topk_fused with the rank counters of k_score_count).  Per step, element-wise final activation: GRU, k_score_cand
// (the Mt target scores), k_topk_rank, k_rank_counts, k_events_merge (list, rank and target score straight to the event's place),
// k_zero_rows.  softmax / softmax_logit values need the whole row: the scores are materialised as g4r_evaluate materialises them
// (k_score_store, k_softmax_rows, k_rank_rows), then selected from memory (k_topk_stored) -- two passes and more (with `items` the
// row is normalised over [targets | items] for the rank, as g4r_evaluate does, and once more over `items` alone for the list, as
// g4r_recommend_step does).  Results stay on the device until the end of the call, or of a piece of it.
//
// events_check: every check of the call's plan, slots, seen tables and exclusions (each session keeps at least k eligible candidate
// positions at its last event), before any device work.  g4r_loglik_events (g4r_host_loglik.hpp) shares them, with k = 1.
static int events_check(g4r_model* m, const int32_t* in_idx, const int32_t* out_idx, const uint8_t* reset, const int32_t* M, int64_t T,
                        int32_t batch, const int64_t* compact_steps, const int32_t* compact_maps, int64_t n_compact, const int32_t* items,
                        int64_t n_items_sel, int32_t mode, const int64_t* slot, int64_t n_slots, int32_t k, const uint32_t* excl_mask,
                        const int64_t* seen_offs, const int32_t* seen_items, const int32_t* seen_first, int64_t n_seen,
                        const int32_t* seen_sess, const int32_t* seen_pos) {
    if (!m || !in_idx || !out_idx || !reset || !M || !slot) return fail("null argument");
    if (T < 0 || batch < 1 || n_slots < 0) return fail("bad evaluation sizes");
    if (plan_mode_check(mode, compact_steps, compact_maps, n_compact)) return -1;
    if (items && n_items_sel < 1) return fail("n_items_sel must be positive");
    DevModel& d = m->dm;
    const int B = batch;
    const int64_t I = d.n_items, n_cand = items ? n_items_sel : I;
    if (k < 1 || k > G4R_TOPK_MAX) return fail("k must be in [1, " + std::to_string(G4R_TOPK_MAX) + "]");
    if (k > n_cand) return fail("k exceeds the number of candidates (" + std::to_string(n_cand) + ")");
    if (n_cand > INT32_MAX) return fail("more than 2^31 - 1 candidates");
    if (plan_rows_check(M, T, B) || plan_index_check(d, in_idx, out_idx, T, B, items, n_items_sel)) return -1;
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
    return 0;
}

int g4r_recommend_events(g4r_model* m, const int32_t* in_idx, const int32_t* out_idx, const uint8_t* reset, const int32_t* M, int64_t T,
                         int32_t batch, const int64_t* compact_steps, const int32_t* compact_maps, int64_t n_compact,
                         const int32_t* items, int64_t n_items_sel, int32_t mode, const int64_t* slot, int64_t n_slots, int32_t k,
                         const uint32_t* excl_mask, const int64_t* seen_offs, const int32_t* seen_items, const int32_t* seen_first,
                         int64_t n_seen, const int32_t* seen_sess, const int32_t* seen_pos, int32_t* out_items, float* out_scores,
                         float* out_rank, float* out_target_score) {
    // ---- every check before any device work
    if (events_check(m, in_idx, out_idx, reset, M, T, batch, compact_steps, compact_maps, n_compact, items, n_items_sel, mode, slot, n_slots, k,
                     excl_mask, seen_offs, seen_items, seen_first, n_seen, seen_sess, seen_pos))
        return -1;
    DevModel& d = m->dm;
    const int B = batch;
    const int64_t I = d.n_items, n_cand = items ? n_items_sel : I;
    const bool seen = seen_offs != nullptr;
    const bool excl = seen || excl_mask;
    const bool sm = is_softmax(d);
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
    int64_t need = 1;
    for (int64_t t = 0; t < T; ++t) need = std::max<int64_t>(need, (int64_t)M[t] * tk_ranges(m, M[t], n_cand, TK_TN).R * k);
    if (g4r_predict_begin(m, batch)) return -1;            // fresh (zero) hidden state, scratch for `batch` rows
    if (m->p_topk.reserve(m, need)) return -1;
    int *e_in = nullptr, *e_out = nullptr, *e_maps = nullptr, *e_items = nullptr, *e_cand = nullptr, *e_iota = nullptr, *e_sitems = nullptr,
        *e_sfirst = nullptr, *o_items = nullptr;
    unsigned char* e_reset = nullptr;
    unsigned* e_mask = nullptr;
    long long* e_place = nullptr;
    int4 *e_seen = nullptr, *e_work = nullptr;
    float *e_ts = nullptr, *o_scores = nullptr, *o_rank = nullptr, *o_ts = nullptr;
    const int64_t n_sl = seen ? seen_offs[n_seen] : 0, nw = (I + 31) / 32;
    CallTemps tmp(m);
    if (tmp.get(&e_in, TB, false) || tmp.get(&e_out, TB, false) || tmp.get(&e_reset, TB, false) || tmp.get(&e_place, TB, false) ||
        tmp.get(&e_maps, (size_t)std::max<int64_t>(n_compact, 1) * B, false) || tmp.get(&e_iota, B, false) || tmp.get(&e_work, B, false) ||
        tmp.get(&e_ts, B) || tmp.get(&o_items, (size_t)cap * k) || tmp.get(&o_scores, (size_t)cap * k) || tmp.get(&o_rank, (size_t)cap) ||
        tmp.get(&o_ts, (size_t)cap) || (items && tmp.get(&e_items, (size_t)n_items_sel, false)) ||
        (items && sm && tmp.get(&e_cand, (size_t)B + n_items_sel, false)) ||
        (seen && (tmp.get(&e_seen, TB, false) || tmp.get(&e_sitems, (size_t)n_sl, false) || tmp.get(&e_sfirst, (size_t)n_sl, false))) ||
        (excl_mask && tmp.get(&e_mask, (size_t)nw, false)))
        return -1;
    hipStream_t s = m->stream;
    std::vector<int4> work((size_t)B);            // k_score_cand: row r scores one position, r, of the step's target list
    for (int r = 0; r < B; ++r) work[r] = make_int4(r, r, r + 1, r);
    if (T > 0) {
        HIPCHK(hipMemcpyAsync(e_in, in_idx, TB * sizeof(int), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(e_out, out_idx, TB * sizeof(int), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(e_reset, reset, TB, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(e_place, place.data(), TB * sizeof(long long), hipMemcpyHostToDevice, s));
        if (seen) HIPCHK(hipMemcpyAsync(e_seen, hseen.data(), TB * sizeof(int4), hipMemcpyHostToDevice, s));
    }
    HIPCHK(hipMemcpyAsync(e_work, work.data(), (size_t)B * sizeof(int4), hipMemcpyHostToDevice, s));
    if (n_compact > 0) HIPCHK(hipMemcpyAsync(e_maps, compact_maps, (size_t)n_compact * B * sizeof(int), hipMemcpyHostToDevice, s));
    if (items) HIPCHK(hipMemcpyAsync(e_items, items, (size_t)n_items_sel * sizeof(int), hipMemcpyHostToDevice, s));
    if (seen && n_sl > 0) {
        HIPCHK(hipMemcpyAsync(e_sitems, seen_items, (size_t)n_sl * sizeof(int), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(e_sfirst, seen_first, (size_t)n_sl * sizeof(int), hipMemcpyHostToDevice, s));
    }
    if (excl_mask) HIPCHK(hipMemcpyAsync(e_mask, excl_mask, (size_t)nw * sizeof(uint32_t), hipMemcpyHostToDevice, s));
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
            m->ev_launches += (int64_t)d.n_layers * plan_compact(m, t, compact_steps, n_compact, e_maps, B, &ci);
            const int* tgt = e_out + t * B;
            const int* d_items = items ? (const int*)e_items : (const int*)nullptr;
            // the noise key of a column and of the target are g4r_evaluate's, which scores [targets | items]: column Mt + j, target i
            const int* tie_col = items ? (const int*)e_iota : tgt;
            const TkRanges g = tk_ranges(m, Mt, n_cand, TK_TN);
            const TkEvents ev = {e_ts, m->p_cnt, mode == G4R_RANK_TIEBREAKING ? tie_col : (const int*)nullptr, items ? (long long)Mt : 0LL, (unsigned)t,
                                 seen ? (const int4*)(e_seen + t * B) : (const int4*)nullptr, e_sitems, e_sfirst, e_mask};
            if (!sm) {
                if (predict_gru(m, e_in + t * B, Mt)) return -1;
                const float* hsrc = (const float*)m->phout[top];
                hipLaunchKernelGGL(k_score_cand, dim3(Mt), dim3(256), 0, s, (const DevModel*)m->d_dm, hsrc, tgt, (const int4*)e_work, e_ts, 1);
                if (excl) tk_launch<false, true>(m, s, g, hsrc, Mt, d_items, n_cand, nullptr, 0, k, ev);      // k_topk_rank_x
                else tk_launch<false, false>(m, s, g, hsrc, Mt, d_items, n_cand, nullptr, 0, k, ev);          // k_topk_rank
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
                if (predict_forward(m, e_in + t * B, Mt, cand, n_sel, nullptr)) return -1;
                hipLaunchKernelGGL(k_rank_rows, dim3(Mt), dim3(256), 0, s, (const float*)m->p_scores.p, (long long)m->p_nsel, (long long)m->p_ldo,
                                   tie_col, items ? (long long)Mt : 0LL, (int)mode, m->p_ranks, (unsigned long long)m->cfg.seed, (unsigned)t);
                hipLaunchKernelGGL(k_events_tscore, dim3(cdiv(Mt, 256)), dim3(256), 0, s, (const float*)m->p_scores.p, (long long)m->p_ldo, tie_col, Mt, e_ts);
                m->ev_scans += 3;            // k_score_store, k_softmax_rows, k_rank_rows
                m->ev_launches += 2 * d.n_layers + 4;
                int64_t ldo = m->p_ldo;
                if (items) {                  // the list's scores are normalised over `items` alone (g4r_recommend_step's)
                    ldo = (n_items_sel + 3) & ~3LL;
                    score_rows(m, (const float*)m->phout[top], Mt, d_items, n_items_sel, m->p_scores.p, ldo);
                    m->ev_scans += 2;
                    m->ev_launches += 2;
                }
                const float* hsrc = (const float*)m->phout[top];
                if (excl) tk_launch<true, true>(m, s, g, hsrc, Mt, d_items, n_cand, (const float*)m->p_scores.p, ldo, k, ev);      // k_topk_stored_ev
                else tk_launch<true, false>(m, s, g, hsrc, Mt, d_items, n_cand, (const float*)m->p_scores.p, ldo, k);              // k_topk_stored
                m->ev_scans += 1;
                m->ev_launches += 1;
            }
            hipLaunchKernelGGL(k_events_merge, dim3(Mt), dim3(256), 0, s, (const uint2*)m->p_topk.p, g.R, (int)k, (const long long*)(e_place + t * B), d_items,
                               (const float*)m->p_ranks, (const float*)e_ts, o_items, o_scores, o_rank, o_ts);
            // hidden rows of sessions that ended with this step start from zero
            state_zero_rows(m, e_reset + t * B, Mt);
            m->ev_launches += 1 + d.n_layers;
        }
        HIPCHK(hipGetLastError());
        // ---- the piece's results: one download, one synchronisation
        int64_t n_ev = 0;
        for (int64_t t = t0; t < piece_end[pc]; ++t) n_ev += M[t];
        const int64_t rows = one_piece ? n_slots : n_ev;
        int32_t* h_items = one_piece ? out_items : st_items.data();
        float *h_scores = one_piece ? out_scores : st_scores.data(), *h_rank = one_piece ? out_rank : st_rank.data(),
              *h_ts = one_piece ? out_target_score : st_ts.data();
        if (rows > 0) {
            if (out_items) HIPCHK(hipMemcpyAsync(h_items, o_items, (size_t)rows * k * sizeof(int32_t), hipMemcpyDeviceToHost, s));
            if (out_scores) HIPCHK(hipMemcpyAsync(h_scores, o_scores, (size_t)rows * k * sizeof(float), hipMemcpyDeviceToHost, s));
            if (out_rank) HIPCHK(hipMemcpyAsync(h_rank, o_rank, (size_t)rows * sizeof(float), hipMemcpyDeviceToHost, s));
            if (out_target_score) HIPCHK(hipMemcpyAsync(h_ts, o_ts, (size_t)rows * sizeof(float), hipMemcpyDeviceToHost, s));
        }
        HIPCHK(hipStreamSynchronize(s));
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
    return 0;
}

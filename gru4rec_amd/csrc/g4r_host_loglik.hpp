// g4r_host_loglik.hpp -- part of libgru4rec_hip.so's host code; included once, by g4r_api.hip (one translation unit: the kernels are templates
// instantiated there).  Holds: g4r_loglik_events (the log-likelihood of the logged next item at every event of a whole test set).
// ------------------------------------------------------------------------------------------------ per-event log-likelihood
// g4r_loglik_events: g4r_recommend_events' plan loop, every step's rows given what g4r_session_log_partition gives a replayed prefix --
// zeta and the exact integer normaliser Q over the event's eligible candidate positions -- plus the z of the event's target (the
// contract: include/gru4rec_hip.h).  Per step, whatever the final activation (the scan works on z, the pre-activation value for
// softmax / softmax_logit, so no score matrix is materialised and the STORED selection is never taken):
//   GRU -> k_score_cand (the Mt targets' z) -> pass A: k_topk_rank_x with k = 1 (the exact selection under TkEvents' eligibility; its
//   rank counters are a by-product, cleared by k_loglik_finish) + k_topk_merge (zeta) -> zero Q -> pass B: k_topk_events_q (Q under the
//   same eligibility) -> k_loglik_finish ((z_t, zeta, Q) to the event's place) -> k_zero_rows.
// Two scans per step.  Whether the target itself holds an eligible position is decided here on the host, from the same tables the
// kernels read.  Results stay on the device until the end of the call, or of a piece of it (G4R_EVENTS_PIECE, 16 bytes an event).
int g4r_loglik_events(g4r_model* m, const int32_t* in_idx, const int32_t* out_idx, const uint8_t* reset, const int32_t* M, int64_t T,
                      int32_t batch, const int64_t* compact_steps, const int32_t* compact_maps, int64_t n_compact, const int32_t* items,
                      int64_t n_items_sel, const int64_t* slot, int64_t n_slots, const uint32_t* excl_mask, const int64_t* seen_offs,
                      const int32_t* seen_items, const int32_t* seen_first, int64_t n_seen, const int32_t* seen_sess,
                      const int32_t* seen_pos, float temperature, float* out_z, float* out_zeta, uint64_t* out_Q, uint8_t* out_eligible) {
    // ---- every check before any device work
    if (!out_z || !out_zeta || !out_Q || !out_eligible) return fail("null argument");
    if (events_check(m, in_idx, out_idx, reset, M, T, batch, compact_steps, compact_maps, n_compact, items, n_items_sel, G4R_RANK_STANDARD, slot,
                     n_slots, 1, excl_mask, seen_offs, seen_items, seen_first, n_seen, seen_sess, seen_pos))
        return -1;
    const float invT = 1.0f / temperature;
    if (!(temperature > 0.f) || !std::isfinite(temperature) || !std::isfinite(invT))
        return fail("temperature must be a finite float > 0 with a finite reciprocal");
    DevModel& d = m->dm;
    const int B = batch;
    const int64_t I = d.n_items, n_cand = items ? n_items_sel : I;
    if (n_cand > G4R_LSE_CAND_MAX)
        return fail("the log-likelihood takes at most 2^24 candidate positions (the exact row normaliser is a 64-bit integer)");
    const bool seen = seen_offs != nullptr;
    // ---- the targets' eligibility: a position in `items` (or any item), not masked, not shown by the session up to the input event
    // (unused slots of the caller's arrays read zero)
    if (n_slots > 0) memset(out_eligible, 0, (size_t)n_slots);
    {
        std::vector<bool> listed;
        if (items) {
            listed.assign((size_t)I, false);
            for (int64_t p = 0; p < n_items_sel; ++p) listed[items[p]] = true;
        }
        for (int64_t t = 0; t < T; ++t)
            for (int r = 0; r < M[t]; ++r) {
                const int32_t tg = out_idx[t * B + r];
                bool ok = (!items || listed[tg]) && !(excl_mask && ((excl_mask[tg >> 5] >> (tg & 31)) & 1u));
                if (ok && seen) {
                    const int s = seen_sess[t * B + r];
                    const int32_t *b = seen_items + seen_offs[s], *e = seen_items + seen_offs[s + 1];
                    const int32_t* f = std::lower_bound(b, e, tg);
                    if (f != e && *f == tg && seen_first[f - seen_items] <= seen_pos[t * B + r]) ok = false;
                }
                out_eligible[slot[t * B + r]] = ok ? 1 : 0;
            }
    }
    // ---- pieces, as g4r_recommend_events cuts them
    int64_t piece_bytes = G4R_EVENTS_PIECE_BYTES;
    if (const char* e = getenv("G4R_EVENTS_PIECE")) piece_bytes = std::max<int64_t>(1, atoll(e));      // tests: results do not depend on it
    const int64_t cap_ev = std::max<int64_t>(B, piece_bytes / 16);
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
    int64_t need = 1;      // workspace of the range lists (k = 1): the largest any step needs
    for (int64_t t = 0; t < T; ++t) need = std::max<int64_t>(need, (int64_t)M[t] * tk_ranges(m, M[t], n_cand, TK_TN).R);
    if (g4r_predict_begin(m, batch)) return -1;            // fresh (zero) hidden state, scratch for `batch` rows
    if (m->p_topk.reserve(m, need) || m->sm_zeta.reserve(m, B) || m->sm_zcol.reserve(m, B) || m->sm_Q.reserve(m, B)) return -1;
    int *e_in = nullptr, *e_out = nullptr, *e_maps = nullptr, *e_items = nullptr, *e_sitems = nullptr, *e_sfirst = nullptr;
    unsigned char* e_reset = nullptr;
    unsigned* e_mask = nullptr;
    long long* e_place = nullptr;
    int4 *e_seen = nullptr, *e_work = nullptr;
    float *e_ts = nullptr, *o_z = nullptr, *o_zeta = nullptr;
    unsigned long long* o_Q = nullptr;
    const int64_t n_sl = seen ? seen_offs[n_seen] : 0, nw = (I + 31) / 32;
    CallTemps tmp(m);
    if (tmp.get(&e_in, TB, false) || tmp.get(&e_out, TB, false) || tmp.get(&e_reset, TB, false) || tmp.get(&e_place, TB, false) ||
        tmp.get(&e_maps, (size_t)std::max<int64_t>(n_compact, 1) * B, false) || tmp.get(&e_work, B, false) || tmp.get(&e_ts, B) ||
        tmp.get(&o_z, (size_t)cap) || tmp.get(&o_zeta, (size_t)cap) || tmp.get(&o_Q, (size_t)cap) ||
        (items && tmp.get(&e_items, (size_t)n_items_sel, false)) ||
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
    // host staging of a piece (several pieces only)
    std::vector<float> st_z, st_zeta;
    std::vector<unsigned long long> st_Q;
    if (!one_piece) {
        st_z.resize((size_t)cap); st_zeta.resize((size_t)cap); st_Q.resize((size_t)cap);
        memset(out_z, 0, (size_t)n_slots * sizeof(float));
        memset(out_zeta, 0, (size_t)n_slots * sizeof(float));
        memset(out_Q, 0, (size_t)n_slots * sizeof(uint64_t));
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
            const TkRanges g = tk_ranges(m, Mt, n_cand, TK_TN);
            const TkEvents ev = {e_ts, m->p_cnt, (const int*)nullptr, 0LL, (unsigned)t, seen ? (const int4*)(e_seen + t * B) : (const int4*)nullptr,
                                 e_sitems, e_sfirst, e_mask};
            if (predict_gru(m, e_in + t * B, Mt)) return -1;
            const float* hsrc = (const float*)m->phout[top];
            hipLaunchKernelGGL(k_score_cand, dim3(Mt), dim3(256), 0, s, (const DevModel*)m->d_dm, hsrc, tgt, (const int4*)e_work, e_ts, 1);
            tk_launch<false, true>(m, s, g, hsrc, Mt, d_items, n_cand, nullptr, 0, 1, ev);      // pass A: k_topk_rank_x
            hipLaunchKernelGGL(k_topk_merge, dim3(Mt), dim3(256), 0, s, (const uint2*)m->p_topk.p, g.R, 1, m->sm_zcol.p, m->sm_zeta.p);
            HIPCHK(hipMemsetAsync(m->sm_Q.p, 0, (size_t)Mt * sizeof(unsigned long long), s));
            tk_launch<false, true>(m, s, g, hsrc, Mt, d_items, n_cand, nullptr, 0, 1,
                                   TkEventsLse{ev, TkLse{(const float*)m->sm_zeta.p, 1, m->sm_Q.p, invT}});      // pass B: k_topk_events_q
            hipLaunchKernelGGL(k_loglik_finish, dim3(cdiv(Mt, 256)), dim3(256), 0, s, (const long long*)(e_place + t * B), (const float*)e_ts,
                               (const float*)m->sm_zeta.p, (const unsigned long long*)m->sm_Q.p, m->p_cnt, Mt, o_z, o_zeta, o_Q);
            // hidden rows of sessions that ended with this step start from zero
            state_zero_rows(m, e_reset + t * B, Mt);
            m->ev_scans += 2;
            m->ev_launches += 2 * d.n_layers + 6 + d.n_layers;      // GRU, k_score_cand, A, merge, memset, B, finish, k_zero_rows
        }
        HIPCHK(hipGetLastError());
        // ---- the piece's results: one download, one synchronisation
        int64_t n_ev = 0;
        for (int64_t t = t0; t < piece_end[pc]; ++t) n_ev += M[t];
        const int64_t rows = one_piece ? n_slots : n_ev;
        float *h_z = one_piece ? out_z : st_z.data(), *h_zeta = one_piece ? out_zeta : st_zeta.data();
        unsigned long long* h_Q = one_piece ? (unsigned long long*)out_Q : st_Q.data();
        if (rows > 0) {
            HIPCHK(hipMemcpyAsync(h_z, o_z, (size_t)rows * sizeof(float), hipMemcpyDeviceToHost, s));
            HIPCHK(hipMemcpyAsync(h_zeta, o_zeta, (size_t)rows * sizeof(float), hipMemcpyDeviceToHost, s));
            HIPCHK(hipMemcpyAsync(h_Q, o_Q, (size_t)rows * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        }
        HIPCHK(hipStreamSynchronize(s));
        ++m->ev_pieces;
        if (!one_piece)
            for (int64_t t = t0; t < piece_end[pc]; ++t)
                for (int r = 0; r < M[t]; ++r) {
                    const size_t from = (size_t)place[t * B + r], to = (size_t)slot[t * B + r];
                    out_z[to] = st_z[from]; out_zeta[to] = st_zeta[from]; out_Q[to] = st_Q[from];
                }
        t0 = piece_end[pc];
    }
    return 0;
}

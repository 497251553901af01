// g4r_host_sessions.hpp -- part of libgru4rec_hip.so's host code; included once, by g4r_api.hip (one translation unit: the kernels are templates
// instantiated there).  Holds: the stateless entries that replay whole histories: the replay (replay_chunks), g4r_recommend_sessions(_scan),
// g4r_continue_sessions, the optional stages behind the selection (sessions_run), and the per-row candidate lists (g4r_score_candidates,
// g4r_score_candidates_sessions).
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
    return m->r_in.reserve(m, n_in);
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
// store (g4r_store_push, g4r_host_store.hpp; h0 and out_hidden NULL): the two edges go to the session store instead of the host.  Row i
// of the call starts from the store row of slot store->slots[i], or from zeros where store->fresh[i] is set (k_store_load), and its
// final state goes back to that row (k_store_save, k_replay_final's rule).  A chunk's slots and fresh marks lie in st.slot / st.fresh
// (chunk order) from its begin on, so score() may read them.
struct StoreEdge { const int32_t* slots; const int32_t* fresh; };
extern "C++" {      // (this file is included inside extern "C")
template <class S, class F>
static int replay_chunks(g4r_model* m, const int64_t* hist_offs, const int32_t* hist_items, int32_t n, int C, const float* const* h0,
                         float* const* out_hidden, S score, F done, const int* final_half = nullptr, const StoreEdge* store = nullptr) {
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
        HIPCHK(hipMemcpyAsync(m->r_in.p, steps.data(), steps.size() * sizeof(int), hipMemcpyHostToDevice, m->stream));
        HIPCHK(hipMemcpyAsync(m->r_perm, perm.data(), Cc * sizeof(int), hipMemcpyHostToDevice, m->stream));
        HIPCHK(hipMemcpyAsync(m->r_len, len.data(), Cc * sizeof(int), hipMemcpyHostToDevice, m->stream));
        if (store) {
            if (m->st.slot.reserve(m, Cc) || m->st.fresh.reserve(m, Cc)) return -1;
            HIPCHK(hipMemcpyAsync(m->st.slot.p, store->slots + c0, Cc * sizeof(int), hipMemcpyHostToDevice, m->stream));
            HIPCHK(hipMemcpyAsync(m->st.fresh.p, store->fresh + c0, Cc * sizeof(int), hipMemcpyHostToDevice, m->stream));
        }
        for (int l = 0; l < L; ++l) {
            if (store) {
                hipLaunchKernelGGL(k_store_load, dim3(cdiv((long long)Cc * d.D[l], 256)), dim3(256), 0, m->stream, m->rH[l][0],
                                   (const float*)m->st.H[l], (const int*)m->st.slot.p, (const int*)m->st.fresh.p, (const int*)m->r_perm, Cc, d.D[l]);
                continue;
            }
            if (h0) HIPCHK(hipMemcpyAsync(m->rio[l], h0[l] + (size_t)c0 * d.D[l], (size_t)Cc * d.D[l] * sizeof(float), hipMemcpyHostToDevice, m->stream));
            hipLaunchKernelGGL(k_replay_begin, dim3(cdiv((long long)Cc * d.D[l], 256)), dim3(256), 0, m->stream, m->rH[l][0],
                               h0 ? (const float*)m->rio[l] : (const float*)nullptr, (const int*)m->r_perm, Cc, d.D[l]);
        }
        // step t: sorted rows [0, M_t) (M_t = rows with len > t), H[t & 1] -> H[(t + 1) & 1].  A row that has finished is never
        // written again (gru_step), so the top layer's rhout row keeps its last output and its state stays in H[len & 1]
        int Mt = Cc;
        for (int t = 0; t < T; ++t) {
            while (Mt > 0 && len[Mt - 1] <= t) --Mt;
            gru_step(m, rb, t & 1, (const int*)m->r_in.p + (size_t)t * Cc, Mt);
        }
        if (score(c0, Cc, (const std::vector<int>&)perm, (const float*)m->rhout[L - 1])) return -1;
        if (store)
            for (int l = 0; l < L; ++l)
                hipLaunchKernelGGL(k_store_save, dim3(cdiv((long long)Cc * d.D[l], 256)), dim3(256), 0, m->stream, m->st.H[l],
                                   (const float*)m->rH[l][0], (const float*)m->rH[l][1], (const int*)m->st.slot.p, (const int*)m->r_perm,
                                   (const int*)m->r_len, Cc, d.D[l], T);
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

// The exclusion lists of a chunk's rows in sorted row order (sorted row r is session c0 + perm[r]; xoffs / xitems: every session's
// list, sorted and de-duplicated by excl_pack; has_lists false: all empty).  slack < 0: CSR, offs = [Cc + 1] offsets into items.
// Otherwise the lists grow on the device: offs = the begin of every row's list, `slack` free slots behind it, len = its length now
static void excl_chunk(const std::vector<long long>& xoffs, const std::vector<int32_t>& xitems, bool has_lists, int c0, int Cc,
                       const std::vector<int>& perm, int slack, std::vector<long long>& offs, std::vector<int32_t>& items,
                       std::vector<int32_t>& len) {
    const bool grow = slack >= 0;
    offs.clear();
    items.clear();
    len.clear();
    if (!grow) offs.push_back(0);
    for (int r = 0; r < Cc; ++r) {
        const int i = c0 + perm[r];
        if (grow) offs.push_back((long long)items.size());
        if (has_lists) items.insert(items.end(), xitems.begin() + xoffs[i], xitems.begin() + xoffs[i + 1]);
        if (grow) {
            len.push_back(has_lists ? (int32_t)(xoffs[i + 1] - xoffs[i]) : 0);
            items.insert(items.end(), (size_t)slack, 0);
        } else offs.push_back((long long)items.size());
    }
}

// no_repeat (g4r_continue_sessions, g4r_beam_sessions) needs duplicate-free candidates (item_idx, range-checked; NULL: all items):
// only then does every generated item take exactly one eligible position
static int no_repeat_check(g4r_model* m, const int32_t* item_idx, int64_t n_sel) {
    if (!item_idx) return 0;
    std::vector<uint32_t> seen(((size_t)m->dm.n_items + 31) / 32, 0u);
    for (int64_t p = 0; p < n_sel; ++p) {
        const int32_t i = item_idx[p];
        if ((seen[i >> 5] >> (i & 31)) & 1u) return fail("no_repeat needs duplicate-free candidates: item index " + std::to_string(i) + " is listed twice");
        seen[i >> 5] |= 1u << (i & 31);
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------ selection after a replay
// The body of g4r_recommend_sessions(_scan) and g4r_continue_sessions; the caller has run recommend_check and its own refusals.
// oversample 0: the exact selection, otherwise the two-stage one.
// steps = 0 (g4r_recommend_sessions*): per chunk the replay and one selection, downloaded from p_tcols / p_tscores.
// steps >= 1 (g4r_continue_sessions): that selection followed, per chunk and on the device, by steps - 1 rounds of (winner -> GRU
// input -> GRU step -> selection); k_rollout_feed files every step's lists in ro_cols / ro_scores and, with no_repeat, adds the winner
// to the row's exclusion list.  One synchronisation and one download per chunk whatever `steps` is.
// mmr (g4r_diversify_sessions; steps = 0, k = the pool): k_mmr_rerank picks mmr->k of every row's k selected candidates on the device
// and the chunk downloads those picks (columns, scores, pool positions, values) instead of the lists.  NULL: nothing is added.
// caps (g4r_recommend_sessions_capped, g4r_continue_sessions_capped; k = the pool, the caller has run cap_check): k_group_cap keeps up to
// caps->k of every row's k selected candidates by the cap rule.  steps = 0: the chunk downloads what it kept, with the pool positions
// and the counts.  steps >= 1: it runs on every step between the merge and k_rollout_feed, which is pointed at the kept lists with
// their k -- slot 0 is the capped winner --; the rows' prior lists grow on the device like the exclusion lists, and the counts
// come back as [rows][steps].  NULL: nothing is added.
static int mmr_prepare(g4r_model* m, const MmrStage& st, int rows);
static int mmr_enqueue(g4r_model* m, const MmrStage& st, int rows, int pool, const int* d_items, int64_t n_sel);
static int cap_prepare(g4r_model* m, const CapStage& st, int rows, int n_step);
static void cap_priors(const CapStage& st, int32_t n, std::vector<long long>& offs, std::vector<int32_t>& groups);
static int cap_priors_upload(g4r_model* m, int rows, const std::vector<long long>& offs, const std::vector<int32_t>& groups, const std::vector<int32_t>& len);
static int cap_enqueue(g4r_model* m, const CapStage& st, int rows, int pool, const int* d_items, int64_t n_sel, int steps, int s);
static int sessions_run(g4r_model* m, const int64_t* hist_offs, const int32_t* hist_items, int32_t n, const float* const* h0,
                        const int32_t* item_idx, int64_t n_sel, int32_t k, int32_t oversample, int32_t steps, int32_t no_repeat,
                        const int64_t* excl_offs, const int32_t* excl_items, const uint32_t* excl_mask, int32_t* out_cols,
                        float* out_scores, float* const* out_hidden, const MmrStage* mmr = nullptr, const CapStage* caps = nullptr) {
    // ---- every check before any kernel is launched.  cand_upload, among them, stages the candidate items (it may drain the stream, grow
    // p_items and enqueue the copy), and the no_repeat and excl_pack refusals come after it: nothing here has state to advance
    int32_t scan_c = 0;
    if (oversample && scan_check(m, item_idx, n_sel, k, oversample, &scan_c)) return -1;
    HIPCHK(hipSetDevice(m->cfg.device));
    if (replay_check(m, hist_offs, hist_items, n, h0, out_hidden)) return -1;
    const DevModel& d = m->dm;
    const int* d_items;
    if (cand_upload(m, item_idx, &n_sel, &d_items)) return -1;
    const bool rollout = steps > 0;
    const int n_step = std::max(steps, 1);
    const bool grow = no_repeat != 0 && steps > 1;      // the lists gain items on the device
    if (no_repeat && no_repeat_check(m, item_idx, n_sel)) return -1;
    std::vector<long long> xoffs;
    std::vector<int32_t> xitems;
    const bool excl = excl_offs || excl_mask || grow;
    if (excl && excl_pack(m, n, item_idx, n_sel, k, excl_offs, excl_items, excl_mask, xoffs, xitems, grow ? steps - 1 : 0)) return -1;
    const bool lists = excl_offs || grow;
    std::vector<long long> poffs;      // caps, steps >= 1: every session's prior groups
    std::vector<int32_t> pgroups;
    if (caps && rollout) cap_priors(*caps, n, poffs, pgroups);
    if (rollout) ++m->ro_calls;
    // ---- buffers
    const int C = replay_chunk_rows(n);
    const int L = d.n_layers;
    const bool sm = is_softmax(d);
    const int64_t ldo = (n_sel + 3) & ~3LL;
    if (sm && m->r_scores.reserve(m, (int64_t)C * ldo)) return -1;
    const int ko = caps ? caps->k : k;                               // entries of a row's list as it leaves
    const int64_t per_row = mmr ? mmr->k : (int64_t)n_step * ko;     // entries a row downloads
    if (mmr && mmr_prepare(m, *mmr, C)) return -1;
    if (caps && cap_prepare(m, *caps, C, n_step)) return -1;
    if (rollout && (m->ro_cols.reserve(m, (int64_t)C * per_row) || m->ro_scores.reserve(m, (int64_t)C * per_row) || m->ro_in.reserve(m, (int64_t)C) ||
                    (grow && m->ro_xlen.reserve(m, (int64_t)C))))
        return -1;
    std::vector<int32_t> tcols((size_t)C * per_row);
    std::vector<float> tscores((size_t)C * per_row);
    const bool cpos = caps && !rollout && caps->out_pos;
    std::vector<int32_t> tpos(mmr || cpos ? (size_t)C * per_row : 0);
    std::vector<int32_t> tkept(caps ? (size_t)C * n_step : 0);
    std::vector<float> tval(mmr ? (size_t)C * per_row : 0);
    std::vector<long long> coffs;
    std::vector<int32_t> citems, clen;
    std::vector<long long> pcoffs;
    std::vector<int32_t> pcgroups, pclen;
    const GruBufs rb = replay_bufs(m);
    int final_half = -1;
    // ---- chunk by chunk: the replay, then the selections; one synchronisation per chunk
    auto score = [&](int c0, int Cc, const std::vector<int>& perm, const float* hsrc) -> int {
        TkExcl ex{};
        TkGrow gx{};
        if (excl) {
            if (lists) excl_chunk(xoffs, xitems, excl_offs != nullptr, c0, Cc, perm, grow ? steps - 1 : -1, coffs, citems, clen);
            if (excl_upload(m, lists, coffs, citems, excl_mask, &ex)) return -1;
            if (grow) {
                HIPCHK(hipMemcpyAsync(m->ro_xlen.p, clen.data(), (size_t)Cc * sizeof(int), hipMemcpyHostToDevice, m->stream));
                gx = TkGrow{ex.offs, (const int*)m->ro_xlen.p, ex.items, ex.mask};
            }
        }
        if (caps && rollout) {      // the prior lists through the same packer and permutation, steps - 1 slots of slack behind each
            excl_chunk(poffs, pgroups, caps->prior_offs != nullptr, c0, Cc, perm, steps - 1, pcoffs, pcgroups, pclen);
            if (cap_priors_upload(m, Cc, pcoffs, pcgroups, pclen)) return -1;
        }
        const TkExcl* exp = (excl && !grow) ? &ex : nullptr;
        const TkGrow* gxp = grow ? &gx : nullptr;
        const int T = (int)(hist_offs[c0 + perm[0] + 1] - hist_offs[c0 + perm[0]]);      // the chunk's longest history
        for (int s = 0; s < n_step; ++s) {
            if (rollout) ++m->ro_steps;
            if (s == 1) {
                // every row's state into the half of the longest history: from here on all Cc rows step together
                for (int l = 0; l < L; ++l)
                    hipLaunchKernelGGL(k_rollout_align, dim3(cdiv((long long)Cc * d.D[l], 256)), dim3(256), 0, m->stream, m->rH[l][T & 1],
                                       (const float*)m->rH[l][(T & 1) ^ 1], (const int*)m->r_len, Cc, d.D[l], T);
            }
            if (s > 0) gru_step(m, rb, (T + s - 1) & 1, (const int*)m->ro_in.p, Cc);
            if (sm) score_rows(m, hsrc, Cc, d_items, n_sel, m->r_scores.p, ldo);
            if (scan_c > 0) {
                if (topk_select_scan(m, hsrc, Cc, d_items, n_sel, k, scan_c, exp, gxp, s > 0)) return -1;
            } else if (topk_select(m, hsrc, Cc, d_items, n_sel, k, exp, (const float*)m->r_scores.p, ldo, gxp)) return -1;
            if (caps && cap_enqueue(m, *caps, Cc, k, d_items, n_sel, steps, s)) return -1;
            if (rollout) {
                const bool last = s == steps - 1;
                hipLaunchKernelGGL(k_rollout_feed, dim3(Cc), dim3(64), 0, m->stream, caps ? (const int*)m->gc_cols.p : (const int*)m->p_tcols.p,
                                   caps ? (const float*)m->gc_scores.p : (const float*)m->p_tscores.p, ko,
                                   (int)steps, s, d_items, m->ro_cols.p, m->ro_scores.p, last ? (int*)nullptr : m->ro_in.p, gx.beg,
                                   last ? (int*)nullptr : const_cast<int*>(gx.len), const_cast<int*>(gx.items));      // (gx: all NULL unless the lists grow)
            }
        }
        final_half = steps > 1 ? ((T + steps - 1) & 1) : -1;
        if (mmr) {
            if (mmr_enqueue(m, *mmr, Cc, k, d_items, n_sel)) return -1;
            HIPCHK(hipMemcpyAsync(tpos.data(), m->dv_pos.p, (size_t)Cc * per_row * sizeof(int), hipMemcpyDeviceToHost, m->stream));
            HIPCHK(hipMemcpyAsync(tval.data(), m->dv_val.p, (size_t)Cc * per_row * sizeof(float), hipMemcpyDeviceToHost, m->stream));
        }
        if (caps) {
            if (cpos) HIPCHK(hipMemcpyAsync(tpos.data(), m->gc_pos.p, (size_t)Cc * per_row * sizeof(int), hipMemcpyDeviceToHost, m->stream));
            HIPCHK(hipMemcpyAsync(tkept.data(), m->gc_kept.p, (size_t)Cc * n_step * sizeof(int), hipMemcpyDeviceToHost, m->stream));
        }
        HIPCHK(hipMemcpyAsync(tcols.data(), mmr ? m->dv_cols.p : rollout ? m->ro_cols.p : caps ? m->gc_cols.p : m->p_tcols.p, (size_t)Cc * per_row * sizeof(int), hipMemcpyDeviceToHost, m->stream));
        HIPCHK(hipMemcpyAsync(tscores.data(), mmr ? m->dv_scores.p : rollout ? m->ro_scores.p : caps ? m->gc_scores.p : m->p_tscores.p, (size_t)Cc * per_row * sizeof(float), hipMemcpyDeviceToHost, m->stream));
        return 0;
    };
    // sorted row r is session c0 + perm[r]
    auto done = [&](int c0, int Cc, const std::vector<int>& perm) {
        for (int r = 0; r < Cc; ++r) {
            memcpy(out_cols + (size_t)(c0 + perm[r]) * per_row, tcols.data() + (size_t)r * per_row, (size_t)per_row * sizeof(int32_t));
            memcpy(out_scores + (size_t)(c0 + perm[r]) * per_row, tscores.data() + (size_t)r * per_row, (size_t)per_row * sizeof(float));
            if (mmr) {
                memcpy(mmr->out_pos + (size_t)(c0 + perm[r]) * per_row, tpos.data() + (size_t)r * per_row, (size_t)per_row * sizeof(int32_t));
                memcpy(mmr->out_value + (size_t)(c0 + perm[r]) * per_row, tval.data() + (size_t)r * per_row, (size_t)per_row * sizeof(float));
            }
            if (caps) {
                if (cpos) memcpy(caps->out_pos + (size_t)(c0 + perm[r]) * per_row, tpos.data() + (size_t)r * per_row, (size_t)per_row * sizeof(int32_t));
                memcpy(caps->out_kept + (size_t)(c0 + perm[r]) * n_step, tkept.data() + (size_t)r * n_step, (size_t)n_step * sizeof(int32_t));
            }
        }
    };
    return replay_chunks(m, hist_offs, hist_items, n, C, h0, out_hidden, score, done, &final_half);
}

int g4r_recommend_sessions(g4r_model* m, const int64_t* hist_offs, const int32_t* hist_items, int32_t n, const float* const* h0,
                           const int32_t* item_idx, int64_t n_sel, int32_t k, const int64_t* excl_offs, const int32_t* excl_items,
                           const uint32_t* excl_mask, int32_t* out_cols, float* out_scores, float* const* out_hidden) {
    if (recommend_check(m, item_idx, n_sel, k, out_cols, out_scores)) return -1;
    return sessions_run(m, hist_offs, hist_items, n, h0, item_idx, n_sel, k, 0, 0, 0, excl_offs, excl_items, excl_mask, out_cols, out_scores,
                        out_hidden);
}

int g4r_recommend_sessions_scan(g4r_model* m, const int64_t* hist_offs, const int32_t* hist_items, int32_t n, const float* const* h0,
                                const int32_t* item_idx, int64_t n_sel, int32_t k, int32_t oversample, const int64_t* excl_offs,
                                const int32_t* excl_items, const uint32_t* excl_mask, int32_t* out_cols, float* out_scores,
                                float* const* out_hidden) {
    if (oversample < 1) return fail("oversample must be at least 1 and k * oversample at most G4R_SCAN_CAND_MAX = " + std::to_string(G4R_SCAN_CAND_MAX));
    if (recommend_check(m, item_idx, n_sel, k, out_cols, out_scores)) return -1;
    return sessions_run(m, hist_offs, hist_items, n, h0, item_idx, n_sel, k, oversample, 0, 0, excl_offs, excl_items, excl_mask, out_cols,
                        out_scores, out_hidden);
}

int g4r_continue_sessions(g4r_model* m, const int64_t* hist_offs, const int32_t* hist_items, int32_t n, const float* const* h0,
                          const int32_t* item_idx, int64_t n_sel, int32_t k, int32_t oversample, int32_t steps, int32_t no_repeat,
                          const int64_t* excl_offs, const int32_t* excl_items, const uint32_t* excl_mask, int32_t* out_cols,
                          float* out_scores, float* const* out_hidden) {
    if (recommend_check(m, item_idx, n_sel, k, out_cols, out_scores)) return -1;
    if (steps < 1) return fail("steps must be at least 1");
    if (oversample < 0) return fail("oversample must be 0 (the exact selection) or at least 1");
    return sessions_run(m, hist_offs, hist_items, n, h0, item_idx, n_sel, k, oversample, steps, no_repeat, excl_offs, excl_items, excl_mask,
                        out_cols, out_scores, out_hidden);
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
    const bool sm = is_softmax(m->dm);
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
    if (m->c_offs.reserve(m, (int64_t)rows + 1) || m->c_items.reserve(m, P) || m->c_scores.reserve(m, P) ||
        m->c_work.reserve(m, (int64_t)hs.work.size()) ||
        (k > 0 && (m->c_topk.reserve(m, topk_need) || m->c_tpos.reserve(m, (int64_t)rows * k) || m->c_tscores.reserve(m, (int64_t)rows * k))))
        return -1;
    HIPCHK(hipMemcpyAsync(m->c_offs.p, hs.offs.data(), hs.offs.size() * sizeof(long long), hipMemcpyHostToDevice, m->stream));
    HIPCHK(hipMemcpyAsync(m->c_items.p, items + base, (size_t)P * sizeof(int32_t), hipMemcpyHostToDevice, m->stream));
    HIPCHK(hipMemcpyAsync(m->c_work.p, hs.work.data(), hs.work.size() * sizeof(int4), hipMemcpyHostToDevice, m->stream));
    // softmax needs the row's raw scores first: stored without the activation, then normalised over the row's own list
    hipLaunchKernelGGL(k_score_cand, dim3((unsigned)hs.work.size()), dim3(256), 0, m->stream, (const DevModel*)m->d_dm, hsrc,
                       (const int*)m->c_items.p, (const int4*)m->c_work.p, m->c_scores.p, sm ? 0 : 1);
    if (sm) hipLaunchKernelGGL(k_softmax_csr, dim3(rows), dim3(256), 0, m->stream, m->c_scores.p, (const long long*)m->c_offs.p);
    if (k == 0) {
        HIPCHK(hipMemcpyAsync(out_scores, m->c_scores.p, (size_t)P * sizeof(float), hipMemcpyDeviceToHost, m->stream));
    } else {
        for (const int4& g : groups) {
            const int L = g.z * k;
            hipLaunchKernelGGL(k_cand_pack, dim3(cdiv(L, 256), g.y), dim3(256), 0, m->stream, (const float*)m->c_scores.p,
                               (const long long*)m->c_offs.p + g.x, L, m->c_topk.p);
            hipLaunchKernelGGL(k_topk_merge, dim3(g.y), dim3(256), 0, m->stream, (const uint2*)m->c_topk.p, g.z, (int)k,
                               m->c_tpos.p + (size_t)g.x * k, m->c_tscores.p + (size_t)g.x * k);
        }
        HIPCHK(hipMemcpyAsync(out_pos, m->c_tpos.p, (size_t)rows * k * sizeof(int32_t), hipMemcpyDeviceToHost, m->stream));
        HIPCHK(hipMemcpyAsync(out_scores, m->c_tscores.p, (size_t)rows * k * sizeof(float), hipMemcpyDeviceToHost, m->stream));
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
    if (predict_gru(m, m->p_in, mrows)) return -1;
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

// g4r_host_groups.hpp -- part of libgru4rec_hip.so's host code; included once, by g4r_api.hip (one translation unit: the kernels are templates
// instantiated there).  Holds: item groups and per-group caps: the group table (g4r_set_item_groups / g4r_get_item_groups), the checks, the
// launch of k_group_cap, g4r_cap_lists (supplied lists) and g4r_recommend_sessions_capped / g4r_continue_sessions_capped (the stage behind
// sessions_run's selection).
// ------------------------------------------------------------------------------------------------ item groups, per-group caps
// Rows per chunk of g4r_cap_lists: one workgroup per row, sixteen rounds of one workgroup per compute unit.
#define G4R_CAP_CHUNK_ROWS 4096

int g4r_set_item_groups(g4r_model* m, const int32_t* groups, int64_t n) {
    if (!m) return fail("null argument");
    if (!groups && n == 0) { m->gc_set = false; m->gc_ngroups = 0; return 0; }
    if (!groups) return fail("null argument");
    if (n != m->dm.n_items) return fail("the group table must hold n_items = " + std::to_string(m->dm.n_items) + " entries, not " + std::to_string(n));
    int32_t hi = -1;
    for (int64_t i = 0; i < n; ++i) {
        if (groups[i] < -1) return fail("group of item index " + std::to_string(i) + " is below -1 (-1 = ungrouped)");
        hi = std::max(hi, groups[i]);
    }
    if (hi == INT32_MAX) return fail("group index out of range");
    HIPCHK(hipSetDevice(m->cfg.device));
    if (m->gc_groups.reserve(m, n)) return -1;
    m->gc_set = false;
    HIPCHK(hipMemcpyAsync(m->gc_groups.p, groups, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));      // (the caller's array may go)
    m->gc_set = true;
    m->gc_ngroups = hi + 1;
    return 0;
}

int g4r_get_item_groups(g4r_model* m, int32_t* out, int64_t n) {
    if (!m || !out) return fail("null argument");
    if (!m->gc_set) return fail("no item groups are set (g4r_set_item_groups)");
    if (n != m->dm.n_items) return fail("the group table holds n_items = " + std::to_string(m->dm.n_items) + " entries, not " + std::to_string(n));
    HIPCHK(hipSetDevice(m->cfg.device));
    HIPCHK(hipMemcpyAsync(out, m->gc_groups.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    return 0;
}

// the checks the three entries share (nothing is launched): the table, the cap, the list length P and k; n prior lists (prior_offs NULL:
// none), each with `grow` more entries to come on the device
static int cap_check(g4r_model* m, int32_t cap, int32_t P, int32_t k, int64_t n, const int64_t* prior_offs, const int32_t* prior_groups,
                     int32_t grow) {
    if (!m->gc_set) return fail("no item groups are set (g4r_set_item_groups)");
    if (cap < 1) return fail("cap must be at least 1");
    if (P < 1 || P > G4R_TOPK_MAX) return fail("the pool must hold between 1 and G4R_TOPK_MAX = " + std::to_string(G4R_TOPK_MAX) + " positions");
    if (k < 1 || k > P) return fail("k must be in [1, pool = " + std::to_string(P) + "]");
    if (n < 1) return fail("n must be positive");
    if (!prior_offs && grow > G4R_GROUP_PRIOR_MAX)
        return fail("row 0 has 0 prior groups and gains " + std::to_string(grow) + " more (steps - 1), more than G4R_GROUP_PRIOR_MAX = " +
                    std::to_string(G4R_GROUP_PRIOR_MAX));
    if (!prior_offs) return 0;
    if (prior_offs[0] < 0) return fail("prior_offs[0] is negative");
    for (int64_t r = 0; r < n; ++r) {
        const int64_t len = prior_offs[r + 1] - prior_offs[r];
        if (len < 0) return fail("prior_offs is not monotone at row " + std::to_string(r));
        if (len + grow > G4R_GROUP_PRIOR_MAX)
            return fail("row " + std::to_string(r) + " has " + std::to_string(len) + " prior groups" +
                        (grow ? " and gains " + std::to_string(grow) + " more (steps - 1)" : std::string()) + ", more than G4R_GROUP_PRIOR_MAX = " +
                        std::to_string(G4R_GROUP_PRIOR_MAX));
    }
    if (prior_offs[n] > prior_offs[0] && !prior_groups) return fail("null argument (prior_groups)");
    for (int64_t r = 0; r < n; ++r)
        for (int64_t j = prior_offs[r]; j < prior_offs[r + 1]; ++j)
            if (prior_groups[j] < 0 || prior_groups[j] >= m->gc_ngroups)
                return fail("prior group out of range in row " + std::to_string(r) + " (the model has " + std::to_string(m->gc_ngroups) + " groups)");
    return 0;
}

// the buffers of what chunks of `rows` rows keep over n_step steps
static int cap_prepare(g4r_model* m, const CapStage& st, int rows, int n_step) {
    const int64_t n = (int64_t)rows * st.k;
    return (m->gc_cols.reserve(m, n) || m->gc_scores.reserve(m, n) || m->gc_pos.reserve(m, n) || m->gc_kept.reserve(m, (int64_t)rows * n_step)) ? -1 : 0;
}

// every session's checked prior groups as excl_chunk takes lists (offsets from 0)
static void cap_priors(const CapStage& st, int32_t n, std::vector<long long>& offs, std::vector<int32_t>& groups) {
    offs.clear();
    groups.clear();
    if (!st.prior_offs) return;
    offs.resize((size_t)n + 1);
    for (int i = 0; i <= n; ++i) offs[i] = (long long)(st.prior_offs[i] - st.prior_offs[0]);
    if (offs[n] > 0) groups.assign(st.prior_groups + st.prior_offs[0], st.prior_groups + st.prior_offs[n]);
}

// a chunk's prior lists (begin of every row's list, the lists with their slack, the lengths now) onto the device
static int cap_priors_upload(g4r_model* m, int rows, const std::vector<long long>& offs, const std::vector<int32_t>& groups,
                             const std::vector<int32_t>& len) {
    if (m->gc_pbeg.reserve(m, rows) || m->gc_plen.reserve(m, rows) || m->gc_prior.reserve(m, std::max<int64_t>(1, (int64_t)groups.size()))) return -1;
    HIPCHK(hipMemcpyAsync(m->gc_pbeg.p, offs.data(), (size_t)rows * sizeof(long long), hipMemcpyHostToDevice, m->stream));
    HIPCHK(hipMemcpyAsync(m->gc_plen.p, len.data(), (size_t)rows * sizeof(int), hipMemcpyHostToDevice, m->stream));
    if (!groups.empty()) HIPCHK(hipMemcpyAsync(m->gc_prior.p, groups.data(), groups.size() * sizeof(int32_t), hipMemcpyHostToDevice, m->stream));
    return 0;
}

// k_group_cap over `rows` lists of P (columns, scores), enqueued only; map / n_cols: the columns' items (NULL: the columns are items);
// prior: the rows have prior lists in gc_pbeg / gc_plen / gc_prior
static int cap_launch(g4r_model* m, int cap, int k, int rows, int P, const int* cols, const float* scores, const int* map, int64_t n_cols,
                      bool prior, bool cont, bool append, int* out_cols, float* out_scores, int* out_pos, int* out_kept, int kept_stride) {
    hipLaunchKernelGGL(k_group_cap, dim3((unsigned)rows), dim3(GC_THREADS), 0, m->stream, cols, scores, P, map, (long long)n_cols,
                       (const int*)m->gc_groups.p, (int)m->dm.n_items, cap, k, prior ? (const long long*)m->gc_pbeg.p : (const long long*)nullptr,
                       prior ? m->gc_plen.p : (int*)nullptr, prior ? m->gc_prior.p : (int*)nullptr, cont ? 1 : 0, append ? 1 : 0, out_cols,
                       out_scores, out_pos, out_kept, kept_stride);
    HIPCHK(hipGetLastError());
    return 0;
}

// sessions_run's stage at step s of `steps` (0: a single selection, no continuation): the lists are the selection's, in p_tcols / p_tscores
static int cap_enqueue(g4r_model* m, const CapStage& st, int rows, int pool, const int* d_items, int64_t n_sel, int steps, int s) {
    const bool cont = steps > 0;
    return cap_launch(m, st.cap, st.k, rows, pool, (const int*)m->p_tcols.p, (const float*)m->p_tscores.p, d_items, n_sel, cont, cont,
                      cont && s < steps - 1, m->gc_cols.p, m->gc_scores.p, m->gc_pos.p, m->gc_kept.p + (cont ? s : 0), cont ? steps : 1);
}

int g4r_cap_lists(g4r_model* m, const int32_t* items, int64_t n, int32_t P, int32_t k, int32_t cap, const int64_t* prior_offs,
                  const int32_t* prior_groups, int32_t* out_pos, int32_t* out_kept) {
    // ---- every check before any device work
    if (!m || !items || !out_pos || !out_kept) return fail("null argument");
    if (cap_check(m, cap, P, k, n, prior_offs, prior_groups, 0)) return -1;
    const int64_t I = m->dm.n_items;
    for (int64_t e = 0; e < n * P; ++e)
        if (items[e] < 0 || items[e] >= I) return fail("item index out of range (list " + std::to_string(e / P) + ")");
    HIPCHK(hipSetDevice(m->cfg.device));
    // ---- chunk by chunk: upload the lists and their priors, walk, copy the kept positions back (one synchronisation per chunk)
    const int C = (int)std::min<int64_t>(n, G4R_CAP_CHUNK_ROWS);
    const CapStage st{cap, k, prior_offs, prior_groups, out_pos, out_kept};
    if (cap_prepare(m, st, C, 1) || m->gc_items.reserve(m, (int64_t)C * P)) return -1;
    std::vector<long long> beg;
    std::vector<int32_t> len, groups;
    for (int64_t c0 = 0; c0 < n; c0 += C) {
        const int Cc = (int)std::min<int64_t>(C, n - c0);
        if (prior_offs) {
            beg.resize(Cc);
            len.resize(Cc);
            for (int r = 0; r < Cc; ++r) {
                beg[r] = (long long)(prior_offs[c0 + r] - prior_offs[c0]);
                len[r] = (int32_t)(prior_offs[c0 + r + 1] - prior_offs[c0 + r]);
            }
            groups.assign(prior_groups ? prior_groups + prior_offs[c0] : nullptr, prior_groups ? prior_groups + prior_offs[c0 + Cc] : nullptr);
            if (cap_priors_upload(m, Cc, beg, groups, len)) return -1;
        }
        HIPCHK(hipMemcpyAsync(m->gc_items.p, items + c0 * P, (size_t)Cc * P * sizeof(int), hipMemcpyHostToDevice, m->stream));
        if (cap_launch(m, cap, k, Cc, P, (const int*)m->gc_items.p, nullptr, nullptr, I, prior_offs != nullptr, false, false, nullptr, nullptr,
                       m->gc_pos.p, m->gc_kept.p, 1))
            return -1;
        HIPCHK(hipMemcpyAsync(out_pos + c0 * k, m->gc_pos.p, (size_t)Cc * k * sizeof(int), hipMemcpyDeviceToHost, m->stream));
        HIPCHK(hipMemcpyAsync(out_kept + c0, m->gc_kept.p, (size_t)Cc * sizeof(int), hipMemcpyDeviceToHost, m->stream));
        HIPCHK(hipStreamSynchronize(m->stream));
    }
    return 0;
}

int g4r_recommend_sessions_capped(g4r_model* m, const int64_t* hist_offs, const int32_t* hist_items, int32_t n, const float* const* h0,
                                  const int32_t* item_idx, int64_t n_sel, int32_t k, int32_t pool, int32_t oversample,
                                  const int64_t* excl_offs, const int32_t* excl_items, const uint32_t* excl_mask, int32_t cap,
                                  int32_t* out_cols, float* out_scores, int32_t* out_pos, int32_t* out_kept, float* const* out_hidden) {
    if (!m || !out_pos || !out_kept) return fail("null argument");
    if (cap_check(m, cap, pool, k, n, nullptr, nullptr, 0)) return -1;
    if (recommend_check(m, item_idx, n_sel, pool, out_cols, out_scores)) return -1;
    if (oversample < 0) return fail("oversample must be 0 (the exact selection) or at least 1");
    const CapStage st{cap, k, nullptr, nullptr, out_pos, out_kept};
    return sessions_run(m, hist_offs, hist_items, n, h0, item_idx, n_sel, pool, oversample, 0, 0, excl_offs, excl_items, excl_mask, out_cols,
                        out_scores, out_hidden, nullptr, &st);
}

int g4r_continue_sessions_capped(g4r_model* m, const int64_t* hist_offs, const int32_t* hist_items, int32_t n, const float* const* h0,
                                 const int32_t* item_idx, int64_t n_sel, int32_t k, int32_t pool, int32_t oversample, int32_t steps,
                                 int32_t no_repeat, const int64_t* excl_offs, const int32_t* excl_items, const uint32_t* excl_mask,
                                 int32_t cap, const int64_t* prior_offs, const int32_t* prior_groups, int32_t* out_cols,
                                 float* out_scores, int32_t* out_kept, float* const* out_hidden) {
    if (!m || !out_kept) return fail("null argument");
    if (steps < 1) return fail("steps must be at least 1");
    if (cap_check(m, cap, pool, k, n, prior_offs, prior_groups, steps - 1)) return -1;
    if (recommend_check(m, item_idx, n_sel, pool, out_cols, out_scores)) return -1;
    if (oversample < 0) return fail("oversample must be 0 (the exact selection) or at least 1");
    const CapStage st{cap, k, prior_offs, prior_groups, nullptr, out_kept};
    return sessions_run(m, hist_offs, hist_items, n, h0, item_idx, n_sel, pool, oversample, steps, no_repeat, excl_offs, excl_items, excl_mask,
                        out_cols, out_scores, out_hidden, nullptr, &st);
}

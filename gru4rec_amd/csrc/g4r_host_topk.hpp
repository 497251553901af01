// g4r_host_topk.hpp -- part of libgru4rec_hip.so's host code; included once, by g4r_api.hip (one translation unit: the kernels are templates
// instantiated there).  Holds: top-k selection over rows of the top layer's output: the k checks, the range geometry, the candidate upload,
// the one launch of each range kernel (tk_launch, scan_launch), topk_select, the exclusion lists and masks, the two-stage bf16 scan (topk_select_scan, g4r_scan_table_release).
// ------------------------------------------------------------------------------------------------ exact top-k
// the k checks of every top-k entry over a model's scores: recommend_step_run and the three session wrappers (g4r_host_sessions.hpp)
static int recommend_check(g4r_model* m, const int32_t* item_idx, int64_t n_sel, int32_t k, int32_t* out_cols, float* out_scores) {
    if (!m || !out_cols || !out_scores) return fail("null argument");
    const int64_t n_cand = item_idx ? n_sel : (int64_t)m->dm.n_items;
    if (k < 1 || k > G4R_TOPK_MAX) return fail("k must be in [1, " + std::to_string(G4R_TOPK_MAX) + "]");
    if (k > n_cand) return fail("k exceeds the number of candidates (n_sel = " + std::to_string(n_cand) + ")");
    if (n_cand > INT32_MAX) return fail("more than 2^31 - 1 candidates");
    return 0;
}

// The candidate items of a call: range check, then the upload into p_items -> *d_items.  item_idx NULL (all items): *n_sel = n_items,
// *d_items = NULL.  Model state is not touched, so entries call it among their checks, ahead of those that read item_idx as indices
static int cand_upload(g4r_model* m, const int32_t* item_idx, int64_t* n_sel, const int** d_items) {
    const DevModel& d = m->dm;
    *d_items = nullptr;
    if (!item_idx) { *n_sel = d.n_items; return 0; }
    for (int64_t i = 0; i < *n_sel; ++i)
        if (item_idx[i] < 0 || item_idx[i] >= d.n_items) return fail("item index out of range");
    if (m->p_items.reserve(m, *n_sel)) return -1;
    HIPCHK(hipMemcpyAsync(m->p_items.p, item_idx, *n_sel * sizeof(int), hipMemcpyHostToDevice, m->stream));
    *d_items = m->p_items.p;
    return 0;
}

// Column ranges of a selection over n_cols candidate columns in tiles of tile_cols: (row blocks) x (ranges) workgroups, about one per
// compute unit (the LDS of k_topk_range admits one per CU); every range walks tpr tiles.  k_topk_merge is told R
struct TkRanges { int row_blocks, tpr, R; };
static TkRanges tk_ranges(const g4r_model* m, int mrows, int64_t n_cols, int tile_cols) {
    const int row_blocks = cdiv(mrows, SC_BM);
    const int64_t tiles = (n_cols + tile_cols - 1) / tile_cols;
    const int64_t R0 = std::min<int64_t>(std::max(1, m->n_cu / row_blocks), tiles);
    const int tpr = (int)((tiles + R0 - 1) / R0);
    return TkRanges{row_blocks, tpr, (int)((tiles + tpr - 1) / tpr)};
}
// *g = those ranges, with p_topk grown to the k entries per row and range they leave
static int tk_reserve(g4r_model* m, int mrows, int64_t n_cols, int tile_cols, int64_t k, TkRanges* g) {
    *g = tk_ranges(m, mrows, n_cols, tile_cols);
    return m->p_topk.reserve(m, (int64_t)mrows * g->R * k);
}

// THE launch of k_topk_range: the form is <STORED, EXCL> and the type of the trailing argument x (none: the unfiltered forms).  The
// grid is g's, the lists go to p_topk, the dynamic LDS is the form's (tk_smem).  scores / ldo: STORED only, NULL / 0 otherwise
extern "C++" {      // (this file is included inside extern "C")
template <bool STORED, bool EXCL, typename... X>
static void tk_launch(g4r_model* m, hipStream_t s, const TkRanges& g, const float* hsrc, int mrows, const int* d_items, int64_t n_sel,
                      const float* scores, int64_t ldo, int k, X... x) {
    hipLaunchKernelGGL((k_topk_range<STORED, EXCL, X...>), dim3(g.R, g.row_blocks), dim3(256), (tk_smem<STORED, EXCL, X...>()), s,
                       (const DevModel*)m->d_dm, hsrc, mrows, d_items, (long long)n_sel, scores, (long long)ldo, k, g.tpr, m->p_topk.p, x...);
}
}  // extern "C++"

// selection of rows [0, mrows) of hsrc (the top layer's output) into p_tcols / p_tscores, enqueued only.  scores / ldo: the same
// rows' materialised scores (softmax / softmax_logit), unused otherwise.  ex (device exclusions) NULL: the unfiltered kernels;
// gx (g4r_continue_sessions, instead of ex): exclusions whose per-row lists grow on the device
static int topk_select(g4r_model* m, const float* hsrc, int32_t mrows, const int* d_items, int64_t n_sel, int32_t k, const TkExcl* ex,
                       const float* scores, int64_t ldo, const TkGrow* gx = nullptr) {
    TkRanges g;
    const int64_t nout = (int64_t)mrows * k;
    if (tk_reserve(m, mrows, n_sel, TK_TN, k, &g) || m->p_tcols.reserve(m, nout) || m->p_tscores.reserve(m, nout)) return -1;
    auto launch = [&](auto... x) {      // stored (softmax / softmax_logit) or fused, with the exclusions x or none
        if (is_softmax(m->dm)) tk_launch<true, sizeof...(x) != 0>(m, m->stream, g, hsrc, mrows, d_items, n_sel, scores, ldo, k, x...);
        else tk_launch<false, sizeof...(x) != 0>(m, m->stream, g, hsrc, mrows, d_items, n_sel, nullptr, 0, k, x...);
    };
    if (gx) launch(*gx);
    else if (ex) launch(*ex);
    else launch();
    hipLaunchKernelGGL(k_topk_merge, dim3(mrows), dim3(256), 0, m->stream, (const uint2*)m->p_topk.p, g.R, (int)k, m->p_tcols.p, m->p_tscores.p);
    HIPCHK(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------------ two-stage top-k (bf16 scan)
// the checks of scan = bf16 next to recommend_check's: *c = the candidates kept per row, min(number of candidates, k * oversample)
static int scan_check(g4r_model* m, const int32_t* item_idx, int64_t n_sel, int32_t k, int32_t oversample, int32_t* c) {
    const DevModel& d = m->dm;
    if (is_softmax(d))
        return fail("the bf16 scan is not implemented for softmax / softmax_logit final activations (their exact values need the whole row)");
    if (oversample < 1 || (int64_t)k * oversample > G4R_SCAN_CAND_MAX)
        return fail("oversample must be at least 1 and k * oversample at most G4R_SCAN_CAND_MAX = " + std::to_string(G4R_SCAN_CAND_MAX));
    if (d.Dtop > 512) return fail("the bf16 scan supports top layers of at most 512 units");
    *c = (int32_t)std::min<int64_t>(item_idx ? n_sel : (int64_t)d.n_items, (int64_t)k * oversample);
    return 0;
}

// k-chunks of 64 columns of the padded top layer (the instantiations of k_scan_bf16: 2, 4, 8)
static int scan_nch(const DevModel& d) { return d.Dtop <= 128 ? 2 : d.Dtop <= 256 ? 4 : 8; }
// THE launch of k_scan_bf16 on the model's stream: the form is scan_nch's k-chunks and the type of the exclusions x (TkExcl or TkGrow)
extern "C++" {
template <typename E>
static void scan_launch(g4r_model* m, const TkRanges& g, const float* hsrc, int mrows, const int* d_items, int64_t n_sel, int c, E x) {
    const auto kern = scan_nch(m->dm) == 2 ? k_scan_bf16<2, E> : scan_nch(m->dm) == 4 ? k_scan_bf16<4, E> : k_scan_bf16<8, E>;
    hipLaunchKernelGGL(kern, dim3(g.R, g.row_blocks), dim3(256), SCN_SMEM, m->stream, (const DevModel*)m->d_dm, hsrc, mrows, d_items,
                       (long long)n_sel, (const uint4*)m->s_tab.p, c, g.tpr, m->p_topk.p, x);
}
}  // extern "C++"

// the bf16 shadow table of Wy, (re)built on the stream when anything may have changed Wy since the last build
static int scan_table_ensure(g4r_model* m) {
    if (m->s_tab_valid) return 0;
    const DevModel& d = m->dm;
    const int KS = 4 * scan_nch(d);
    const int64_t nblk = ((int64_t)d.n_items + 31) / 32, units = nblk * KS * 64;
    if (m->s_tab.reserve(m, units)) return -1;
    hipLaunchKernelGGL(k_wy_bf16, dim3((unsigned)((units + 255) / 256)), dim3(256), 0, m->stream, (const DevModel*)m->d_dm, m->s_tab.p,
                       (long long)nblk, KS);
    HIPCHK(hipGetLastError());
    m->s_tab_valid = true;
    ++m->s_tab_builds;
    return 0;
}

int g4r_scan_table_release(g4r_model* m) {
    if (!m) return fail("null model");
    HIPCHK(hipSetDevice(m->cfg.device));
    HIPCHK(hipStreamSynchronize(m->stream));
    dfree(m, m->s_tab.p);
    m->s_tab = DevBuf<uint4>();
    m->s_tab_valid = false;
    return 0;
}

// topk_select's two-stage twin (element-wise final activations only): rows [0, mrows) of hsrc -> p_tcols / p_tscores, enqueued only,
// no host synchronisation between the stages.  Stage 1: k_scan_bf16 keeps c candidates per row and range, k_scan_merge the row's c.
// Stage 2: k_score_cand scores them (fp32, bit-identical to g4r_predict_step), k_scan_pack + k_topk_merge return the k best.
// gx (g4r_continue_sessions, instead of ex): exclusions whose per-row lists grow on the device; work_ready: k_score_cand's work items
// of an earlier call with the same mrows and c are still in c_work (nothing is uploaded)
static int topk_select_scan(g4r_model* m, const float* hsrc, int32_t mrows, const int* d_items, int64_t n_sel, int32_t k, int32_t c,
                            const TkExcl* ex, const TkGrow* gx = nullptr, bool work_ready = false) {
    if (scan_table_ensure(m)) return -1;
    TkRanges g;
    const int nl = (c + k - 1) / k, L = nl * k;
    const int64_t nout = (int64_t)mrows * k, P = (int64_t)mrows * c;
    if (mrows > 65535) return fail("the bf16 scan takes at most 65535 rows per call");
    if (tk_reserve(m, mrows, n_sel, SCN_TN, c, &g) || m->p_tcols.reserve(m, nout) || m->p_tscores.reserve(m, nout)) return -1;
    // k_score_cand's work items depend on c and the row count only: row r's list is positions [r c, (r + 1) c)
    if (!work_ready) {
        m->s_work.clear();
        for (int r = 0; r < mrows; ++r)
            for (int p = 0; p < c; p += CS_SLICE) m->s_work.push_back(make_int4(r, r * c + p, r * c + std::min(p + CS_SLICE, (int)c), r * c));
    }
    if (m->c_items.reserve(m, P) || m->c_scores.reserve(m, P) || m->c_work.reserve(m, (int64_t)m->s_work.size()) ||
        m->c_topk.reserve(m, (int64_t)mrows * L) || m->s_cols.reserve(m, P) || m->s_cnt.reserve(m, (int64_t)mrows))
        return -1;
    if (!work_ready) HIPCHK(hipMemcpyAsync(m->c_work.p, m->s_work.data(), m->s_work.size() * sizeof(int4), hipMemcpyHostToDevice, m->stream));
    if (gx) scan_launch(m, g, hsrc, mrows, d_items, n_sel, c, *gx);
    else scan_launch(m, g, hsrc, mrows, d_items, n_sel, c, ex ? *ex : TkExcl{nullptr, nullptr, nullptr});
    hipLaunchKernelGGL(k_scan_merge, dim3(mrows), dim3(256), 0, m->stream, (const uint2*)m->p_topk.p, g.R, (int)c, d_items, m->s_cols.p, m->c_items.p,
                       m->c_scores.p, m->s_cnt.p);
#if !(defined(G4R_MUTATE) && G4R_MUTATE == 12)      // test build 12: stage 2 ranks by the approximate scores k_scan_merge left there
    hipLaunchKernelGGL(k_score_cand, dim3((unsigned)m->s_work.size()), dim3(256), 0, m->stream, (const DevModel*)m->d_dm, hsrc,
                       (const int*)m->c_items.p, (const int4*)m->c_work.p, m->c_scores.p, 1);
#endif
    hipLaunchKernelGGL(k_scan_pack, dim3(cdiv(L, 256), mrows), dim3(256), 0, m->stream, (const float*)m->c_scores.p, (const int*)m->s_cols.p,
                       (const int*)m->s_cnt.p, (int)c, L, m->c_topk.p);
    hipLaunchKernelGGL(k_topk_merge, dim3(mrows), dim3(256), 0, m->stream, (const uint2*)m->c_topk.p, nl, (int)k, m->p_tcols.p, m->p_tscores.p);
    HIPCHK(hipGetLastError());
    return 0;
}

// the exclusion checks shared by g4r_recommend_step_filtered / g4r_recommend_sessions: every row's list is checked, sorted and
// de-duplicated into offs / items (left empty without excl_offs); a row with fewer than k eligible candidate positions is refused.
// grow (g4r_continue_sessions with no_repeat): the items every row's list will gain on the device, each taking one eligible position
static int excl_pack(g4r_model* m, int32_t mrows, const int32_t* item_idx, int64_t n_sel, int32_t k, const int64_t* excl_offs,
                     const int32_t* excl_items, const uint32_t* excl_mask, std::vector<long long>& offs, std::vector<int32_t>& items,
                     int32_t grow = 0) {
    const int64_t I = m->dm.n_items, nw = (I + 31) / 32;
    offs.clear();
    items.clear();
    // (without lists every row starts empty: row 0 stands for all of them)
    if (!excl_offs && grow > G4R_EXCLUDE_MAX)
        return fail("row 0 excludes 0 distinct items and generates " + std::to_string(grow) + " more (steps - 1), more than G4R_EXCLUDE_MAX = " +
                    std::to_string(G4R_EXCLUDE_MAX));
    if (excl_offs) {
        if (excl_offs[0] < 0) return fail("excl_offs[0] is negative");
        for (int r = 0; r < mrows; ++r)
            if (excl_offs[r + 1] < excl_offs[r]) return fail("excl_offs is not monotone at row " + std::to_string(r));
        if (excl_offs[mrows] > excl_offs[0] && !excl_items) return fail("null argument (excl_items)");
        offs.resize((size_t)mrows + 1, 0);
        items.reserve((size_t)std::min<int64_t>(excl_offs[mrows] - excl_offs[0], (int64_t)mrows * G4R_EXCLUDE_MAX));
        for (int r = 0; r < mrows; ++r) {
            const size_t b = items.size();
            for (int64_t j = excl_offs[r]; j < excl_offs[r + 1]; ++j) {
                if (excl_items[j] < 0 || excl_items[j] >= I) return fail("excluded item index out of range in row " + std::to_string(r));
                items.push_back(excl_items[j]);
            }
            std::sort(items.begin() + b, items.end());
            items.erase(std::unique(items.begin() + b, items.end()), items.end());
            if (items.size() - b > G4R_EXCLUDE_MAX)
                return fail("row " + std::to_string(r) + " excludes " + std::to_string(items.size() - b) + " distinct items, more than G4R_EXCLUDE_MAX = " +
                            std::to_string(G4R_EXCLUDE_MAX));
            if (items.size() - b + grow > G4R_EXCLUDE_MAX)
                return fail("row " + std::to_string(r) + " excludes " + std::to_string(items.size() - b) + " distinct items and generates " +
                            std::to_string(grow) + " more (steps - 1), more than G4R_EXCLUDE_MAX = " + std::to_string(G4R_EXCLUDE_MAX));
            offs[r + 1] = (long long)items.size();
        }
    }
    auto masked = [&](int32_t i) { return excl_mask && ((excl_mask[i >> 5] >> (i & 31)) & 1u); };
    // eligible candidate positions per row: n_cand - (positions of masked items) - (positions of the row's unmasked items)
    const int64_t n_cand = item_idx ? n_sel : I;
    int64_t n_masked = 0;
    std::vector<int32_t> uni;                 // with item_idx: the items of all rows' lists, sorted, and their position counts
    std::vector<int64_t> cnt;
    if (excl_offs && item_idx) {
        uni = items;
        std::sort(uni.begin(), uni.end());
        uni.erase(std::unique(uni.begin(), uni.end()), uni.end());
        cnt.assign(uni.size(), 0);
    }
    if (item_idx) {
        std::vector<uint32_t> in_uni((size_t)nw, 0u);
        for (int32_t i : uni) in_uni[i >> 5] |= 1u << (i & 31);
        for (int64_t p = 0; p < n_sel; ++p) {
            const int32_t i = item_idx[p];
            if (masked(i)) ++n_masked;
            else if ((in_uni[i >> 5] >> (i & 31)) & 1u) ++cnt[std::lower_bound(uni.begin(), uni.end(), i) - uni.begin()];
        }
    } else if (excl_mask) {
        for (int64_t w = 0; w < nw; ++w) {
            const uint32_t valid = (w == nw - 1 && (I & 31)) ? ((1u << (I & 31)) - 1u) : 0xFFFFFFFFu;
            n_masked += __builtin_popcount(excl_mask[w] & valid);
        }
    }
    for (int r = 0; r < mrows; ++r) {
        int64_t gone = n_masked;
        if (excl_offs)
            for (long long j = offs[r]; j < offs[r + 1]; ++j)
                if (!masked(items[j])) gone += item_idx ? cnt[std::lower_bound(uni.begin(), uni.end(), items[j]) - uni.begin()] : 1;
        if (n_cand - gone < k)
            return fail("row " + std::to_string(r) + " has " + std::to_string(n_cand - gone) + " eligible candidate positions, fewer than k = " +
                        std::to_string(k));
        if (n_cand - gone - grow < k)
            return fail("row " + std::to_string(r) + " has " + std::to_string(n_cand - gone) + " eligible candidate positions, fewer than k + steps - 1 = " +
                        std::to_string(k + grow) + " (every generated item takes one)");
    }
    return 0;
}

// upload of packed exclusions (into buffers that only grow, stream-ordered) -> *ex, the device view; has_lists: offs / items hold
// per-row lists
static int excl_upload(g4r_model* m, bool has_lists, const std::vector<long long>& offs, const std::vector<int32_t>& items,
                       const uint32_t* excl_mask, TkExcl* ex) {
    const int64_t nw = ((int64_t)m->dm.n_items + 31) / 32;
    if (has_lists) {
        if (m->p_xoffs.reserve(m, (int64_t)offs.size()) || m->p_xitems.reserve(m, (int64_t)items.size())) return -1;
        HIPCHK(hipMemcpyAsync(m->p_xoffs.p, offs.data(), offs.size() * sizeof(long long), hipMemcpyHostToDevice, m->stream));
        if (!items.empty()) HIPCHK(hipMemcpyAsync(m->p_xitems.p, items.data(), items.size() * sizeof(int32_t), hipMemcpyHostToDevice, m->stream));
    }
    if (excl_mask) {
        if (m->p_xmask.reserve(m, nw)) return -1;
        HIPCHK(hipMemcpyAsync(m->p_xmask.p, excl_mask, (size_t)nw * sizeof(uint32_t), hipMemcpyHostToDevice, m->stream));
    }
    *ex = TkExcl{has_lists ? (const long long*)m->p_xoffs.p : nullptr, has_lists ? (const int*)m->p_xitems.p : nullptr,
                 excl_mask ? (const unsigned*)m->p_xmask.p : nullptr};
    return 0;
}

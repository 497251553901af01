// g4r_host_store.hpp -- part of libgru4rec_hip.so's host code; included once, by g4r_api.hip (one translation unit: the kernels are templates
// instantiated there).  Holds: the device-resident session store: g4r_store_open / _close, g4r_store_push / _peek (the replay of
// g4r_host_sessions.hpp with its two edges on the store, then the selection over lists that live in the store), g4r_store_read / _write.
// The entries are slot-level: which session owns which slot, and which slot is given up when none is free, is the caller's business.
// ------------------------------------------------------------------------------------------------ open / close
static void store_free(g4r_model* m) {
    g4r_model::SessionStore& st = m->st;
    for (int l = 0; l < G4R_MAX_LAYERS; ++l) { dfree(m, st.H[l]); st.H[l] = nullptr; }
    dfree(m, st.items); dfree(m, st.len); dfree(m, st.flag);
    st.items = st.len = st.flag = nullptr;
    st.open = false;
    st.capacity = 0; st.seen_cap = 0; st.bytes = 0;
}

int g4r_store_open(g4r_model* m, int64_t capacity, int32_t seen_cap) {
    if (!m) return fail("null model");
    if (m->st.open) return fail("a session store is open already (one per model): g4r_store_close first");
    if (capacity < 1 || capacity > INT32_MAX) return fail("capacity must be in [1, 2^31 - 1]");
    if (seen_cap < 0 || seen_cap > G4R_EXCLUDE_MAX) return fail("seen_cap must be in [0, G4R_EXCLUDE_MAX = " + std::to_string(G4R_EXCLUDE_MAX) + "]");
    HIPCHK(hipSetDevice(m->cfg.device));
    const DevModel& d = m->dm;
    g4r_model::SessionStore& st = m->st;
    // (dalloc zeroes on the stream: every slot starts as an empty session at the zero state)
    int rc = 0;
    size_t bytes = 0;
    for (int l = 0; l < d.n_layers && !rc; ++l) {
        rc = dalloc(m, &st.H[l], (size_t)capacity * d.D[l]);
        bytes += (size_t)capacity * d.D[l] * sizeof(float);
    }
    if (!rc) rc = dalloc(m, &st.items, (size_t)capacity * seen_cap);
    if (!rc) rc = dalloc(m, &st.len, (size_t)capacity);
    if (!rc) rc = dalloc(m, &st.flag, (size_t)capacity);
    if (!rc && hipStreamSynchronize(m->stream) != hipSuccess) rc = fail("hipStreamSynchronize failed while the session store was zeroed");
    if (rc) {      // the model stays usable, the store closed (g_err: the allocation's message)
        const std::string why = g_err;
        (void)hipGetLastError();
        store_free(m);
        return fail("g4r_store_open: " + why);
    }
    st.bytes = bytes + (size_t)capacity * ((size_t)seen_cap + 2) * sizeof(int);
    st.capacity = capacity;
    st.seen_cap = seen_cap;
    st.open = true;
    return 0;
}

int g4r_store_close(g4r_model* m) {
    if (!m) return fail("null model");
    if (!m->st.open) return 0;
    HIPCHK(hipSetDevice(m->cfg.device));
    HIPCHK(hipStreamSynchronize(m->stream));
    store_free(m);
    return 0;
}

// ------------------------------------------------------------------------------------------------ push / peek
// the slots of a call: in range and distinct
static int store_slots_check(g4r_model* m, const int32_t* slots, int32_t n) {
    if (!m) return fail("null model");
    if (!m->st.open) return fail("no session store is open (g4r_store_open)");
    if (!slots) return fail("null argument (slots)");
    if (n < 1) return fail("n must be positive");
    if (n > m->st.capacity) return fail("n = " + std::to_string(n) + " rows, more than the store's capacity " + std::to_string(m->st.capacity));
    std::vector<int32_t> s(slots, slots + n);
    std::sort(s.begin(), s.end());
    if (s[0] < 0 || s[n - 1] >= m->st.capacity) return fail("slot out of range");
    for (int i = 1; i < n; ++i)
        if (s[i] == s[i - 1]) return fail("slot " + std::to_string(s[i]) + " is listed twice: within a call a slot belongs to one row");
    return 0;
}

// The selection arguments of a store call, checked before anything is enqueued or any slot changes.  exclude_seen: every row's
// stored list is excluded, which needs lists (seen_cap > 0), duplicate-free candidates (every listed item takes exactly one candidate
// position, as no_repeat) and k + seen_cap + (candidate positions the mask takes) <= candidates -- the host does not see the lists on the
// device, so the bound counts every list as full.  *scan_c: the candidates per row of the two-stage selection (0: the exact one)
static int store_select_check(g4r_model* m, const int32_t* item_idx, int64_t n_sel, int32_t k, int32_t oversample, int32_t exclude_seen,
                              const uint32_t* excl_mask, int32_t* out_cols, float* out_scores, int32_t* scan_c) {
    *scan_c = 0;
    if (k == 0) return 0;
    if (recommend_check(m, item_idx, n_sel, k, out_cols, out_scores)) return -1;
    if (oversample < 0) return fail("oversample must be 0 (the exact selection) or at least 1");
    if (oversample && scan_check(m, item_idx, n_sel, k, oversample, scan_c)) return -1;
    const int64_t I = m->dm.n_items, nw = (I + 31) / 32, n_cand = item_idx ? n_sel : I;
    for (int64_t p = 0; item_idx && p < n_sel; ++p)
        if (item_idx[p] < 0 || item_idx[p] >= I) return fail("item index out of range");
    if (exclude_seen && m->st.seen_cap == 0) return fail("exclude_seen needs seen lists: the store was opened with seen_cap = 0");
    if (exclude_seen && no_repeat_check(m, item_idx, n_sel)) return -1;
    int64_t n_masked = 0;
    if (excl_mask) {
        if (item_idx) {
            for (int64_t p = 0; p < n_sel; ++p) n_masked += (excl_mask[item_idx[p] >> 5] >> (item_idx[p] & 31)) & 1u;
        } else {
            for (int64_t w = 0; w < nw; ++w) {
                const uint32_t valid = (w == nw - 1 && (I & 31)) ? ((1u << (I & 31)) - 1u) : 0xFFFFFFFFu;
                n_masked += __builtin_popcount(excl_mask[w] & valid);
            }
        }
    }
    const int64_t lists = exclude_seen ? m->st.seen_cap : 0;
    if (n_cand - n_masked - lists < k)
        return fail("k = " + std::to_string(k) + " needs k + seen_cap + masked candidate positions <= candidates: " + std::to_string(n_cand) +
                    " candidates, " + std::to_string(n_masked) + " masked, seen_cap = " + std::to_string(lists) +
                    " (conservative: the lists on the device are counted as full)");
    return 0;
}

// The selection of a chunk's Cc rows of hsrc behind k_store_seen, enqueued with its downloads into tcols / tscores (sorted row order)
static int store_select(g4r_model* m, const float* hsrc, int Cc, const int* d_items, int64_t n_sel, int32_t k, int32_t scan_c,
                        int32_t exclude_seen, const uint32_t* excl_mask, int32_t* tcols, float* tscores) {
    const bool sm = is_softmax(m->dm);
    const int64_t ldo = (n_sel + 3) & ~3LL;
    TkExcl ex{};
    if (excl_mask && excl_upload(m, false, std::vector<long long>(), std::vector<int32_t>(), excl_mask, &ex)) return -1;
    const TkGrow gx{(const long long*)m->st.xbeg.p, (const int*)m->st.xlen.p, (const int*)m->st.items, ex.mask};
    const TkExcl* exp = (!exclude_seen && excl_mask) ? &ex : nullptr;
    const TkGrow* gxp = exclude_seen ? &gx : nullptr;
    if (sm) {
        if (m->r_scores.reserve(m, (int64_t)Cc * ldo)) return -1;
        score_rows(m, hsrc, Cc, d_items, n_sel, m->r_scores.p, ldo);
    }
    if (scan_c > 0) {
        if (topk_select_scan(m, hsrc, Cc, d_items, n_sel, k, scan_c, exp, gxp)) return -1;
    } else if (topk_select(m, hsrc, Cc, d_items, n_sel, k, exp, (const float*)m->r_scores.p, ldo, gxp)) return -1;
    HIPCHK(hipMemcpyAsync(tcols, m->p_tcols.p, (size_t)Cc * k * sizeof(int), hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipMemcpyAsync(tscores, m->p_tscores.p, (size_t)Cc * k * sizeof(float), hipMemcpyDeviceToHost, m->stream));
    return 0;
}

// k_store_seen on a chunk's rows (st.slot / st.fresh hold their slots): steps / perm / len NULL = no events (g4r_store_peek); the flags are
// downloaded into tflag (sorted row order)
static int store_seen(g4r_model* m, const int* steps, int Cc, const int* perm, const int* len, const int* fresh, int32_t* tflag) {
    g4r_model::SessionStore& st = m->st;
    if (st.xbeg.reserve(m, Cc) || st.xlen.reserve(m, Cc) || st.oflag.reserve(m, Cc)) return -1;
    hipLaunchKernelGGL(k_store_seen, dim3(Cc), dim3(64), 0, m->stream, steps, Cc, perm, len, (const int*)st.slot.p, fresh, st.seen_cap, st.items,
                       st.len, st.flag, st.xbeg.p, st.xlen.p, st.oflag.p);
    HIPCHK(hipMemcpyAsync(tflag, st.oflag.p, (size_t)Cc * sizeof(int), hipMemcpyDeviceToHost, m->stream));
    return 0;
}

int g4r_store_push(g4r_model* m, const int64_t* ev_offs, const int32_t* ev_items, const int32_t* slots, const int32_t* fresh, int32_t n,
                   const int32_t* item_idx, int64_t n_sel, int32_t k, int32_t oversample, int32_t exclude_seen, const uint32_t* excl_mask,
                   int32_t* out_cols, float* out_scores, int32_t* out_overflow) {
    // ---- every check before any kernel is launched and before any slot changes
    if (store_slots_check(m, slots, n)) return -1;
    if (!fresh) return fail("null argument (fresh)");
    if (k < 0) return fail("k must be 0 (no selection) or in [1, " + std::to_string(G4R_TOPK_MAX) + "]");
    int32_t scan_c = 0;
    if (store_select_check(m, item_idx, n_sel, k, oversample, exclude_seen, excl_mask, out_cols, out_scores, &scan_c)) return -1;
    HIPCHK(hipSetDevice(m->cfg.device));
    if (replay_check(m, ev_offs, ev_items, n, nullptr, nullptr)) return -1;
    const int* d_items = nullptr;
    if (k > 0 && cand_upload(m, item_idx, &n_sel, &d_items)) return -1;
    std::vector<int32_t> fr(n);
    for (int i = 0; i < n; ++i) fr[i] = fresh[i] != 0;
    const StoreEdge edge{slots, fr.data()};
    const int C = replay_chunk_rows(n);
    const bool lists = m->st.seen_cap > 0;
    std::vector<int32_t> tcols((size_t)C * k), tflag((size_t)C, 0);
    std::vector<float> tscores((size_t)C * k);
    auto score = [&](int, int Cc, const std::vector<int>&, const float* hsrc) -> int {
        if (lists && store_seen(m, (const int*)m->r_in.p, Cc, (const int*)m->r_perm, (const int*)m->r_len, (const int*)m->st.fresh.p, tflag.data())) return -1;
        if (k > 0 && store_select(m, hsrc, Cc, d_items, n_sel, k, scan_c, exclude_seen, excl_mask, tcols.data(), tscores.data())) return -1;
        return 0;
    };
    auto done = [&](int c0, int Cc, const std::vector<int>& perm) {
        for (int r = 0; r < Cc; ++r) {
            if (k > 0) {
                memcpy(out_cols + (size_t)(c0 + perm[r]) * k, tcols.data() + (size_t)r * k, (size_t)k * sizeof(int32_t));
                memcpy(out_scores + (size_t)(c0 + perm[r]) * k, tscores.data() + (size_t)r * k, (size_t)k * sizeof(float));
            }
            if (out_overflow) out_overflow[c0 + perm[r]] = lists ? tflag[r] : 0;
        }
    };
    return replay_chunks(m, ev_offs, ev_items, n, C, nullptr, nullptr, score, done, nullptr, &edge);
}

int g4r_store_peek(g4r_model* m, const int32_t* slots, int32_t n, const int32_t* item_idx, int64_t n_sel, int32_t k, int32_t oversample,
                   int32_t exclude_seen, const uint32_t* excl_mask, int32_t* out_cols, float* out_scores, int32_t* out_overflow) {
    if (store_slots_check(m, slots, n)) return -1;
    if (k < 1) return fail("k must be in [1, " + std::to_string(G4R_TOPK_MAX) + "]");
    int32_t scan_c = 0;
    if (store_select_check(m, item_idx, n_sel, k, oversample, exclude_seen, excl_mask, out_cols, out_scores, &scan_c)) return -1;
    HIPCHK(hipSetDevice(m->cfg.device));
    const int* d_items = nullptr;
    if (cand_upload(m, item_idx, &n_sel, &d_items)) return -1;
    const DevModel& d = m->dm;
    const int C = replay_chunk_rows(n), top = d.n_layers - 1;
    const bool lists = m->st.seen_cap > 0;
    std::vector<int32_t> tflag((size_t)C, 0);
    // chunk by chunk, rows in the caller's order: the top layer's stored state IS its last output (the prediction GRU writes the same
    // value to both), so it is loaded into the replay's output rows and selected from there; nothing is stepped, nothing written back
    for (int c0 = 0; c0 < n; c0 += C) {
        const int Cc = std::min(C, n - c0);
        if (replay_reserve(m, Cc, 1) || m->st.slot.reserve(m, Cc)) return -1;
        HIPCHK(hipMemcpyAsync(m->st.slot.p, slots + c0, Cc * sizeof(int), hipMemcpyHostToDevice, m->stream));
        hipLaunchKernelGGL(k_store_load, dim3(cdiv((long long)Cc * d.D[top], 256)), dim3(256), 0, m->stream, m->rhout[top],
                           (const float*)m->st.H[top], (const int*)m->st.slot.p, (const int*)nullptr, (const int*)nullptr, Cc, d.D[top]);
        if (lists && store_seen(m, nullptr, Cc, nullptr, nullptr, nullptr, tflag.data())) return -1;
        if (store_select(m, (const float*)m->rhout[top], Cc, d_items, n_sel, k, scan_c, exclude_seen, excl_mask, out_cols + (size_t)c0 * k,
                         out_scores + (size_t)c0 * k))
            return -1;
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(m->stream));
        if (out_overflow)
            for (int r = 0; r < Cc; ++r) out_overflow[c0 + r] = lists ? tflag[r] : 0;
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------ read / write
// rows of the store by slot, G4R_REPLAY_CHUNK slots at a time through st.io (staging of 32-bit words) and the replay's rio rows
static int store_io(g4r_model* m, const int32_t* slots, int32_t n, float* const* hidden, int32_t* seen, int32_t* len, int32_t* flag, int to_store) {
    g4r_model::SessionStore& st = m->st;
    const DevModel& d = m->dm;
    const int C = std::min<int>(n, G4R_REPLAY_CHUNK), sc = st.seen_cap;
    const hipMemcpyKind kind = to_store ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost;
    auto move = [&](unsigned* store, unsigned* buf, void* host, int Cc, int W) -> int {
        if (W == 0) return 0;
        const size_t bytes = (size_t)Cc * W * 4;
        if (to_store) HIPCHK(hipMemcpyAsync(buf, host, bytes, kind, m->stream));
        hipLaunchKernelGGL(k_store_move, dim3(cdiv((long long)Cc * W, 256)), dim3(256), 0, m->stream, store, buf, (const int*)st.slot.p, Cc, W, to_store);
        if (!to_store) HIPCHK(hipMemcpyAsync(host, buf, bytes, kind, m->stream));
        return 0;
    };
    for (int c0 = 0; c0 < n; c0 += C) {
        const int Cc = std::min(C, n - c0);
        if (replay_reserve(m, Cc, 1) || st.slot.reserve(m, Cc) || st.io.reserve(m, (int64_t)Cc * (sc + 2))) return -1;
        HIPCHK(hipMemcpyAsync(st.slot.p, slots + c0, Cc * sizeof(int), hipMemcpyHostToDevice, m->stream));
        for (int l = 0; l < d.n_layers; ++l)
            if (hidden && move((unsigned*)st.H[l], (unsigned*)m->rio[l], hidden[l] + (size_t)c0 * d.D[l], Cc, d.D[l])) return -1;
        unsigned* io = (unsigned*)st.io.p;
        if (seen && move((unsigned*)st.items, io, seen + (size_t)c0 * sc, Cc, sc)) return -1;
        if (len && move((unsigned*)st.len, io + (size_t)Cc * sc, len + c0, Cc, 1)) return -1;
        if (flag && move((unsigned*)st.flag, io + (size_t)Cc * (sc + 1), flag + c0, Cc, 1)) return -1;
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(m->stream));
    }
    return 0;
}

int g4r_store_read(g4r_model* m, const int32_t* slots, int32_t n, float* const* out_hidden, int32_t* out_seen, int32_t* out_len,
                   int32_t* out_flag) {
    if (store_slots_check(m, slots, n)) return -1;
    for (int l = 0; out_hidden && l < m->dm.n_layers; ++l)
        if (!out_hidden[l]) return fail("null argument (out_hidden[" + std::to_string(l) + "])");
    HIPCHK(hipSetDevice(m->cfg.device));
    return store_io(m, slots, n, out_hidden, out_seen, out_len, out_flag, 0);
}

int g4r_store_write(g4r_model* m, const int32_t* slots, int32_t n, const float* const* hidden, const int32_t* seen, const int32_t* len,
                    const int32_t* flag) {
    if (store_slots_check(m, slots, n)) return -1;
    for (int l = 0; hidden && l < m->dm.n_layers; ++l)
        if (!hidden[l]) return fail("null argument (hidden[" + std::to_string(l) + "])");
    const int sc = m->st.seen_cap;
    if ((len != nullptr) != (seen != nullptr) && sc > 0) return fail("seen and len go together");
    for (int i = 0; len && i < n; ++i) {
        if (len[i] < 0 || len[i] > sc) return fail("len[" + std::to_string(i) + "] is not in [0, seen_cap = " + std::to_string(sc) + "]");
        const int32_t* s = seen + (size_t)i * sc;
        for (int j = 0; j < len[i]; ++j) {
            if (s[j] < 0 || s[j] >= m->dm.n_items) return fail("seen item index out of range in row " + std::to_string(i));
            if (j > 0 && s[j] <= s[j - 1]) return fail("the seen list of row " + std::to_string(i) + " is not strictly ascending");
        }
    }
    HIPCHK(hipSetDevice(m->cfg.device));
    return store_io(m, slots, n, const_cast<float* const*>((float* const*)hidden), const_cast<int32_t*>(seen), const_cast<int32_t*>(len),
                    const_cast<int32_t*>(flag), 1);
}

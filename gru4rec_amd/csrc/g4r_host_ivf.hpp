// g4r_host_ivf.hpp -- part of libgru4rec_hip.so's host code; included once, by g4r_api.hip (one translation unit: the kernels are templates
// instantiated there).  Holds: the item index (IVF) of the session entries: g4r_ivf_assign, g4r_ivf_set, g4r_ivf_release, the index's
// device tables (ivf_tables_ensure) and g4r_recommend_sessions_ivf.
// ------------------------------------------------------------------------------------------------ item index
// The host copy of the index (centroids, partition) is what g4r_ivf_set was given; the device tables are built from it and the CURRENT
// Wy / By, and again after weights_changed.  The centroids and the partition stay as they were set: a changed Wy costs recall, never
// correctness (every candidate is still scored exactly).
static int ivf_check_model(g4r_model* m) {
    if (!m) return fail("null model");
    if (m->dm.Dtop > 512) return fail("the item index supports top layers of at most 512 units");
    return 0;
}

int g4r_ivf_assign(g4r_model* m, const float* centroids, int32_t n_lists, int32_t* out_list) {
    if (ivf_check_model(m)) return -1;
    if (!centroids || !out_list) return fail("null argument");
    if (n_lists < 1 || n_lists > G4R_IVF_LISTS_MAX) return fail("n_lists must be in [1, G4R_IVF_LISTS_MAX = " + std::to_string(G4R_IVF_LISTS_MAX) + "]");
    const DevModel& d = m->dm;
    const int W = d.Dtop + 1;
    std::vector<float> hn((size_t)n_lists);
    for (int l = 0; l < n_lists; ++l) {
        double s = 0.0;
        for (int j = 0; j < W; ++j) {
            const float x = centroids[(size_t)l * W + j];
            if (!std::isfinite(x)) return fail("centroid " + std::to_string(l) + " is not finite");
            s += (double)x * x;
        }
        hn[l] = (float)(0.5 * s);
    }
    HIPCHK(hipSetDevice(m->cfg.device));
    CallTemps tmp(m);
    float *d_cen = nullptr, *d_hn = nullptr;
    int* d_out = nullptr;
    if (tmp.get(&d_cen, (size_t)n_lists * W, false) || tmp.get(&d_hn, (size_t)n_lists, false) || tmp.get(&d_out, (size_t)d.n_items, false)) return -1;
    HIPCHK(hipMemcpyAsync(d_cen, centroids, (size_t)n_lists * W * sizeof(float), hipMemcpyHostToDevice, m->stream));
    HIPCHK(hipMemcpyAsync(d_hn, hn.data(), (size_t)n_lists * sizeof(float), hipMemcpyHostToDevice, m->stream));
    hipLaunchKernelGGL(k_ivf_assign, dim3(cdiv(d.n_items, 256)), dim3(256), (size_t)(IVF_AC * W + IVF_AK) * sizeof(float), m->stream,
                       (const DevModel*)m->d_dm, (const float*)d_cen, (const float*)d_hn, (int)n_lists, d_out);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out_list, d_out, (size_t)d.n_items * sizeof(int), hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    return 0;
}

// the device tables of the index, (re)built on the stream from the host copy and the current Wy / By
static int ivf_tables_ensure(g4r_model* m) {
    IvfIndex& iv = m->iv;
    if (iv.valid) return 0;
    const DevModel& d = m->dm;
    const int nl = iv.nl, D = d.Dtop, W = D + 1, KS = 4 * scan_nch(d);
    std::vector<int> blk((size_t)nl + 1), offs((size_t)nl + 1);
    blk[0] = 0;
    for (int l = 0; l < nl; ++l) {
        offs[l] = (int)iv.offs[l];
        blk[l + 1] = blk[l] + (int)((iv.offs[l + 1] - iv.offs[l] + 31) / 32);
    }
    offs[nl] = (int)iv.offs[nl];
    const int64_t nblk = blk[nl], npos = nblk * 32, units = nblk * KS * 64;
    std::vector<int> pos_item((size_t)npos, -1);
    for (int l = 0; l < nl; ++l)
        std::copy(iv.items.begin() + iv.offs[l], iv.items.begin() + iv.offs[l + 1], pos_item.begin() + (size_t)blk[l] * 32);
    std::vector<float> cwt((size_t)D * nl), cb((size_t)nl);
    for (int l = 0; l < nl; ++l) {
        for (int j = 0; j < D; ++j) cwt[(size_t)j * nl + l] = iv.cen[(size_t)l * W + j];
        cb[l] = iv.cen[(size_t)l * W + D];
    }
    if (iv.tab.reserve(m, units) || iv.pos_by.reserve(m, npos) || iv.pos_item.reserve(m, npos) || iv.blk.reserve(m, (int64_t)nl + 1) ||
        iv.doffs.reserve(m, (int64_t)nl + 1) || iv.cwt.reserve(m, (int64_t)D * nl) || iv.cb.reserve(m, (int64_t)nl))
        return -1;
    HIPCHK(hipMemcpyAsync(iv.pos_item.p, pos_item.data(), (size_t)npos * sizeof(int), hipMemcpyHostToDevice, m->stream));
    HIPCHK(hipMemcpyAsync(iv.blk.p, blk.data(), blk.size() * sizeof(int), hipMemcpyHostToDevice, m->stream));
    HIPCHK(hipMemcpyAsync(iv.doffs.p, offs.data(), offs.size() * sizeof(int), hipMemcpyHostToDevice, m->stream));
    HIPCHK(hipMemcpyAsync(iv.cwt.p, cwt.data(), cwt.size() * sizeof(float), hipMemcpyHostToDevice, m->stream));
    HIPCHK(hipMemcpyAsync(iv.cb.p, cb.data(), cb.size() * sizeof(float), hipMemcpyHostToDevice, m->stream));
    if (units > 0)
        hipLaunchKernelGGL(k_ivf_tab, dim3((unsigned)((units + 255) / 256)), dim3(256), 0, m->stream, (const DevModel*)m->d_dm, (const int*)iv.pos_item.p,
                           iv.tab.p, iv.pos_by.p, (long long)nblk, KS);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(m->stream));      // (the staging vectors above go out of scope)
    iv.nblk = nblk;
    iv.valid = true;
    ++iv.builds;
    return 0;
}

int g4r_ivf_set(g4r_model* m, const float* centroids, int32_t n_lists, const int64_t* list_offs, const int32_t* list_items) {
    if (ivf_check_model(m)) return -1;
    if (!centroids || !list_offs || !list_items) return fail("null argument");
    if (n_lists < 1 || n_lists > G4R_IVF_LISTS_MAX) return fail("n_lists must be in [1, G4R_IVF_LISTS_MAX = " + std::to_string(G4R_IVF_LISTS_MAX) + "]");
    const DevModel& d = m->dm;
    const int64_t I = d.n_items;
    const int W = d.Dtop + 1;
    if (list_offs[0] != 0 || list_offs[n_lists] != I) return fail("list_offs must run from 0 to n_items = " + std::to_string(I));
    for (int l = 0; l < n_lists; ++l)
        if (list_offs[l + 1] < list_offs[l]) return fail("list_offs is not monotone at list " + std::to_string(l));
    std::vector<uint32_t> seen((size_t)(I + 31) / 32, 0u);
    for (int64_t p = 0; p < I; ++p) {
        const int32_t i = list_items[p];
        if (i < 0 || i >= I) return fail("list_items: item index out of range");
        if ((seen[i >> 5] >> (i & 31)) & 1u) return fail("list_items is not a permutation of the items: item index " + std::to_string(i) + " is listed twice");
        seen[i >> 5] |= 1u << (i & 31);
    }
    for (int l = 0; l < n_lists; ++l)
        for (int64_t p = list_offs[l] + 1; p < list_offs[l + 1]; ++p)
            if (list_items[p] <= list_items[p - 1]) return fail("list " + std::to_string(l) + " does not hold its items in ascending item index");
    for (size_t e = 0; e < (size_t)n_lists * W; ++e)
        if (!std::isfinite(centroids[e])) return fail("centroid " + std::to_string(e / W) + " is not finite");
    HIPCHK(hipSetDevice(m->cfg.device));
    HIPCHK(hipStreamSynchronize(m->stream));
    IvfIndex& iv = m->iv;
    iv.nl = n_lists;
    iv.cen.assign(centroids, centroids + (size_t)n_lists * W);
    iv.offs.assign(list_offs, list_offs + n_lists + 1);
    iv.items.assign(list_items, list_items + I);
    iv.set = true;
    iv.valid = false;
    return ivf_tables_ensure(m);
}

int g4r_ivf_release(g4r_model* m) {
    if (!m) return fail("null model");
    HIPCHK(hipSetDevice(m->cfg.device));
    HIPCHK(hipStreamSynchronize(m->stream));
    IvfIndex& iv = m->iv;
    for (void* p : {(void*)iv.tab.p, (void*)iv.pos_by.p, (void*)iv.pos_item.p, (void*)iv.blk.p, (void*)iv.doffs.p, (void*)iv.cwt.p, (void*)iv.cb.p,
                    (void*)iv.ent.p, (void*)iv.probes.p, (void*)iv.pscores.p, (void*)iv.member.p, (void*)iv.toff.p, (void*)iv.work.p,
                    (void*)iv.trip.p, (void*)iv.n_work.p})
        dfree(m, p);
    const int64_t builds = iv.builds;
    iv = IvfIndex();
    iv.builds = builds;
    return 0;
}

// THE launch of k_ivf_scan: the form is scan_nch's k-chunks
static void ivf_scan_launch(g4r_model* m, const float* hsrc, int rows, int np, int c, const TkExcl& ex) {
    const IvfIndex& iv = m->iv;
    const IvfTab ix{(const uint4*)iv.tab.p, (const float*)iv.pos_by.p, (const int*)iv.pos_item.p, (const int*)iv.blk.p, (const int*)iv.doffs.p};
    const auto kern = scan_nch(m->dm) == 2 ? k_ivf_scan<2> : scan_nch(m->dm) == 4 ? k_ivf_scan<4> : k_ivf_scan<8>;
    hipLaunchKernelGGL(kern, dim3(cdiv((long long)rows * np, 4)), dim3(256), IVF_SMEM, m->stream, (const DevModel*)m->d_dm, hsrc, ix,
                       (const int4*)iv.work.p, (const int*)iv.n_work.p, (const int*)iv.trip.p, np, c, m->p_topk.p, ex);
}

int g4r_recommend_sessions_ivf(g4r_model* m, const int64_t* hist_offs, const int32_t* hist_items, int32_t n, const float* const* h0, int32_t k,
                               int32_t oversample, int32_t nprobe, const int64_t* excl_offs, const int32_t* excl_items,
                               const uint32_t* excl_mask, int32_t* out_cols, float* out_scores, int32_t* out_found, float* const* out_hidden,
                               int32_t* out_probes) {
    // ---- every check before any kernel is launched
    if (!m || !out_cols || !out_scores || !out_found) return fail("null argument");
    IvfIndex& iv = m->iv;
    const DevModel& d = m->dm;
    if (!iv.set) return fail("no item index: g4r_ivf_set has not been called (GRU4Rec.build_item_index)");
    if (is_softmax(d))
        return fail("the item index is not implemented for softmax / softmax_logit final activations (their exact values need the whole row)");
    if (k < 1 || k > G4R_TOPK_MAX) return fail("k must be in [1, " + std::to_string(G4R_TOPK_MAX) + "]");
    if (k > d.n_items) return fail("k exceeds the number of candidates (n_sel = " + std::to_string(d.n_items) + ")");
    if (oversample < 1) return fail("oversample must be at least 1");
    if (nprobe < 1 || nprobe > iv.nl || nprobe > G4R_IVF_NPROBE_MAX)
        return fail("nprobe must be in [1, min(n_lists = " + std::to_string(iv.nl) + ", G4R_IVF_NPROBE_MAX = " + std::to_string(G4R_IVF_NPROBE_MAX) + ")]");
    const int c = (int)std::min<int64_t>((int64_t)k * oversample, G4R_SCAN_CAND_MAX), np = nprobe;
    if ((int64_t)np * c > G4R_IVF_WS_MAX)
        return fail("nprobe * min(k * oversample, G4R_SCAN_CAND_MAX) = " + std::to_string((int64_t)np * c) + " exceeds G4R_IVF_WS_MAX = " +
                    std::to_string(G4R_IVF_WS_MAX));
    HIPCHK(hipSetDevice(m->cfg.device));
    if (replay_check(m, hist_offs, hist_items, n, h0, out_hidden)) return -1;
    std::vector<long long> xoffs;
    std::vector<int32_t> xitems;
    const bool excl = excl_offs || excl_mask;
    if (excl && excl_pack(m, n, nullptr, d.n_items, k, excl_offs, excl_items, excl_mask, xoffs, xitems)) return -1;
    if (ivf_tables_ensure(m)) return -1;
    // ---- buffers
    const int C = replay_chunk_rows(n), nl = iv.nl;
    const int Lp = cdiv(nl, np) * np;               // a row's centroid entries: nl / np lists of np for k_topk_merge
    const int nlk = (c + k - 1) / k, L = nlk * k;    // a row's exact scores: nlk lists of k
    const int64_t P = (int64_t)C * c, T = (int64_t)C * np;
    if (iv.ent.reserve(m, (int64_t)C * Lp) || iv.probes.reserve(m, T) || iv.pscores.reserve(m, T) || iv.member.reserve(m, (int64_t)nl * cdiv(C, 32)) ||
        iv.toff.reserve(m, nl) || iv.work.reserve(m, T) || iv.trip.reserve(m, T) || iv.n_work.reserve(m, 1) || m->p_topk.reserve(m, T * c) ||
        m->p_tcols.reserve(m, (int64_t)C * k) || m->p_tscores.reserve(m, (int64_t)C * k) || m->c_items.reserve(m, P) || m->c_scores.reserve(m, P) ||
        m->c_topk.reserve(m, (int64_t)C * L) || m->s_cols.reserve(m, P) || m->s_cnt.reserve(m, (int64_t)C))
        return -1;
    std::vector<int32_t> tcols((size_t)C * k), tcnt((size_t)C), tprobes(out_probes ? (size_t)T : 0);
    std::vector<float> tscores((size_t)C * k);
    std::vector<long long> coffs;
    std::vector<int32_t> citems, clen;
    // ---- chunk by chunk: replay, probe, group, scan, then the bf16 scan's second stage; one synchronisation per chunk
    auto score = [&](int c0, int Cc, const std::vector<int>& perm, const float* hsrc) -> int {
        TkExcl ex{nullptr, nullptr, nullptr};
        if (excl) {
            if (excl_offs) excl_chunk(xoffs, xitems, true, c0, Cc, perm, -1, coffs, citems, clen);
            if (excl_upload(m, excl_offs != nullptr, coffs, citems, excl_mask, &ex)) return -1;
        }
        const int Tc = Cc * np, MW = cdiv(Cc, 32);
        // k_score_cand's work items: row r's list is positions [r c, (r + 1) c)
        m->s_work.clear();
        for (int r = 0; r < Cc; ++r)
            for (int p = 0; p < c; p += CS_SLICE) m->s_work.push_back(make_int4(r, r * c + p, r * c + std::min(p + CS_SLICE, c), r * c));
        if (m->c_work.reserve(m, (int64_t)m->s_work.size())) return -1;
        HIPCHK(hipMemcpyAsync(m->c_work.p, m->s_work.data(), m->s_work.size() * sizeof(int4), hipMemcpyHostToDevice, m->stream));
        hipLaunchKernelGGL(k_ivf_probe, dim3(cdiv(Lp, 256), cdiv(Cc, IVF_PR)), dim3(256), (size_t)IVF_PR * d.Dtop * sizeof(float), m->stream, hsrc, Cc, (int)d.Dtop,
                           (const float*)iv.cwt.p, (const float*)iv.cb.p, nl, Lp, iv.ent.p);
        hipLaunchKernelGGL(k_topk_merge, dim3(Cc), dim3(256), 0, m->stream, (const uint2*)iv.ent.p, Lp / np, np, iv.probes.p, iv.pscores.p);
        HIPCHK(hipMemsetAsync(iv.member.p, 0, (size_t)nl * MW * sizeof(unsigned), m->stream));
        hipLaunchKernelGGL(k_ivf_mark, dim3(cdiv(Tc, 256)), dim3(256), 0, m->stream, (const int*)iv.probes.p, Tc, np, MW, iv.member.p);
        hipLaunchKernelGGL(k_ivf_group, dim3(1), dim3(1024), 0, m->stream, (const unsigned*)iv.member.p, nl, MW, iv.toff.p, iv.work.p, iv.n_work.p);
        hipLaunchKernelGGL(k_ivf_place, dim3(cdiv(Tc, 256)), dim3(256), 0, m->stream, (const int*)iv.probes.p, Tc, np, MW, (const unsigned*)iv.member.p,
                           (const int*)iv.toff.p, iv.trip.p);
        ivf_scan_launch(m, hsrc, Cc, np, c, ex);
        hipLaunchKernelGGL(k_scan_merge, dim3(Cc), dim3(256), 0, m->stream, (const uint2*)m->p_topk.p, np, c, (const int*)nullptr, m->s_cols.p,
                           m->c_items.p, m->c_scores.p, m->s_cnt.p);
        hipLaunchKernelGGL(k_score_cand, dim3((unsigned)m->s_work.size()), dim3(256), 0, m->stream, (const DevModel*)m->d_dm, hsrc,
                           (const int*)m->c_items.p, (const int4*)m->c_work.p, m->c_scores.p, 1);
        hipLaunchKernelGGL(k_ivf_pack, dim3(cdiv(L, 256), Cc), dim3(256), 0, m->stream, (const float*)m->c_scores.p, (const int*)m->s_cols.p,
                           (const int*)m->s_cnt.p, c, L, m->c_topk.p);
        hipLaunchKernelGGL(k_topk_merge, dim3(Cc), dim3(256), 0, m->stream, (const uint2*)m->c_topk.p, nlk, (int)k, m->p_tcols.p, m->p_tscores.p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(tcols.data(), m->p_tcols.p, (size_t)Cc * k * sizeof(int), hipMemcpyDeviceToHost, m->stream));
        HIPCHK(hipMemcpyAsync(tscores.data(), m->p_tscores.p, (size_t)Cc * k * sizeof(float), hipMemcpyDeviceToHost, m->stream));
        HIPCHK(hipMemcpyAsync(tcnt.data(), m->s_cnt.p, (size_t)Cc * sizeof(int), hipMemcpyDeviceToHost, m->stream));
        if (out_probes) HIPCHK(hipMemcpyAsync(tprobes.data(), iv.probes.p, (size_t)Tc * sizeof(int), hipMemcpyDeviceToHost, m->stream));
        return 0;
    };
    // sorted row r is session c0 + perm[r]; the places at and after n_found hold (item 0, NaN)
    auto done = [&](int c0, int Cc, const std::vector<int>& perm) {
        for (int r = 0; r < Cc; ++r) {
            const size_t i = (size_t)(c0 + perm[r]);
            const int found = std::min(tcnt[r], (int)k);
            out_found[i] = found;
            for (int j = 0; j < k; ++j) {
                out_cols[i * k + j] = j < found ? tcols[(size_t)r * k + j] : 0;
                out_scores[i * k + j] = j < found ? tscores[(size_t)r * k + j] : NAN;
            }
            if (out_probes) memcpy(out_probes + i * np, tprobes.data() + (size_t)r * np, (size_t)np * sizeof(int32_t));
        }
    };
    return replay_chunks(m, hist_offs, hist_items, n, C, h0, out_hidden, score, done);
}

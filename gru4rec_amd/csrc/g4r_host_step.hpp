// g4r_host_step.hpp -- part of libgru4rec_hip.so's host code; included once, by g4r_api.hip (one translation unit: the kernels are templates
// instantiated there).  Holds: the training step: StepLauncher, step_head / step_tail (every launch of a step, in order), tail compaction, the captured step graphs, the windows of g4r_train_steps (+ virtual ranks), losses, counters, per-kernel profiling.
// ------------------------------------------------------------------------------------------------ the step
// What a step's launches go through.  open(kn) ... launch(...) ... close(): the launches of kernel slot kn (KN_*).  Profiling (recs):
// start / stop events attached to the dispatch itself (hipExtLaunchKernelGGL): kernel-only durations.  G4R_TRACE: every slot named on
// stderr and waited for.  G4R_SKIP_KN (tools/kn_cost.py): the slots set in m->sw.skip_kn are left out; the duration tells what they cost
// the captured step -- HIP events and rocprofv3 put a ~3 us floor under a dispatch that the graph does not pay, tools/probes/chain_probe.hip
extern "C++" {      // (a member template; g4r_api.hip includes the host files inside its extern "C" block)
struct StepLauncher {
    g4r_model* m;
    hipStream_t s;
    std::vector<EvRec>* recs;      // per-kernel profiling: the (slot, start, stop) records of this step; null otherwise
    size_t evi = 0;
    int kn = -1;
    hipEvent_t ev_a = nullptr, ev_b = nullptr;      // the open slot's event pair (null: untimed launches)
    StepLauncher(g4r_model* m_, std::vector<EvRec>* recs_) : m(m_), s(m_->stream), recs(recs_) {}
    // the slot of the launches that follow, timed by the pair (a, b) if there is one
    void use(int kn_, hipEvent_t a, hipEvent_t b) { kn = kn_; ev_a = a; ev_b = b; }
    void open(int kn_) {
        if (m->sw.trace) { fprintf(stderr, "[g4r] launch %s\n", KN_NAMES[kn_]); fflush(stderr); }
        use(kn_, nullptr, nullptr);
        if (!recs) return;
        while (m->evs.size() < evi + 2) { hipEvent_t e; (void)hipEventCreate(&e); m->evs.push_back(e); }
        use(kn_, m->evs[evi], m->evs[evi + 1]);
        evi += 2;
        recs->push_back(EvRec{kn_, ev_a, ev_b});
    }
    bool skipped() const { return m->sw.skip_kn && kn >= 0 && ((m->sw.skip_kn >> kn) & 1ull); }
    // (the arguments are converted to the kernel's parameter types here: hipExtLaunchKernelGGL marshals what it is handed)
    template <class... P, class... A>
    void launch(void (*kern)(P...), dim3 grid, dim3 block, size_t smem, A... a) {
        if (skipped()) return;
        if (ev_a) hipExtLaunchKernelGGL(kern, grid, block, (unsigned)smem, s, ev_a, ev_b, 0, static_cast<P>(a)...);
        else hipLaunchKernelGGL(kern, grid, block, smem, s, static_cast<P>(a)...);
    }
    void close() {
        if (!m->sw.trace) return;
        hipError_t e = hipStreamSynchronize(s);
        fprintf(stderr, "[g4r] done   %s: %s\n", KN_NAMES[kn], hipGetErrorString(e));
        fflush(stderr);
    }
};
}

// The k_loss_rows instantiation of this model (m->kern: loss_long, loss_spec, loss_quads) on `grid` workgroups -- the one place that
// launches it, for step_head and for g4r_debug_loss_rows (g4r_host_debug.hpp).
static void launch_loss_rows(StepLauncher& lk, dim3 grid) {
    g4r_model* m = lk.m;
    lk.launch(loss_rows_kernel(m->kern), grid, dim3(LOSS_T), m->smem_loss, (const DevModel*)m->d_dm, (StepState*)m->dm.st);
}

// g4r_profile(m, 2) times the two roles of a merged update as launches of their own
static inline bool update_merged(const g4r_model* m, const StepLauncher& lk) { return m->kern.update != UP_SPLIT && !(lk.recs && m->profile_split); }

// ---- the phases of the head, each a straight sequence over m->kern (choose_kernels)
// ent: the step's slot of the entry ring where its per-position entries came from the window launch, else null (step_entries)
static void gru_forward(g4r_model* m, StepLauncher& lk, int l, const int4* ent) {
    const DevModel& d = m->dm;
    const StepKernels& k = m->kern;
    const int B = d.B, first = l == 0 ? 1 : 0;
    const DevModel* dmp = (const DevModel*)m->d_dm;
    StepState* stp = (StepState*)d.st;
    const GruFwdPredict nopa = {};
    if (k.fwd[l] == FWD_LEAN) {
        const dim3 g(cdiv(d.D[l], 16), cdiv(B, 16));
        const LeanV& v = m->h_leanV[l];
        const LeanH& h = m->h_leanH[l];
        const auto kv = l > 0 ? k_gru_v<false, false> : (d.drop_e > 0.f ? k_gru_v<true, true> : k_gru_v<true, false>);
        lk.open(KN_GRU_V);
        lk.launch(kv, dim3(g.x, g.y, 3), dim3(512), 0, m->d_leanV + l, v.st, v.cur_in, v.Wx, v.Wrz, v.H0, v.H1, (unsigned)d.D[l] | ((unsigned)d.IN[l] << 16), B, l == 0 ? ent : nullptr);
        lk.close();
        lk.open(KN_GRU_H);
        lk.launch(k_gru_h, g, dim3(512), 0, m->d_leanH + l, h.Wh, h.Hr, h.Vc, h.z, h.cur_rst, h.H0, h.H1, d.D[l], B);
        lk.close();
        return;
    }
    if (k.fwd[l] == FWD_FUSED) {
        lk.open(KN_FWD_FUSED);
        lk.launch(k_gru_fwd_fused, dim3(cdiv(d.D[l], 32), cdiv(B, FF_ROWS)), dim3(512), (size_t)fwd_fused_lds(d.IN[l], d.D[l]).total * sizeof(float), dmp, stp, l, first);
        lk.close();
        return;
    }
    const WideGeo& G = k.wg[l];
    lk.open(KN_GRU_P1);
    if (k.fwd[l] == FWD_P1S) {
        lk.launch(k_gru_p1s, dim3(d.D[l] / 64 * cdiv(B, 64) * (3 * G.ny + 2 * G.nh)), dim3(256), SMEM_T2K, dmp, stp, l, first, G.ny, G.nh, G.kys, G.khs);
        lk.close();
        lk.open(KN_GATE);
        lk.launch(k_gru_gate, dim3(cdiv((long long)B * (d.D[l] / 4), 256)), dim3(256), 0, dmp, stp, l, G.ny, G.nh);
    } else if (k.fwd[l] == FWD_P1_N64) lk.launch(k_gru_p1_n64, dim3(cdiv(3 * d.D[l], 64), cdiv(B, GT_BM)), dim3(GT_NTH_FEW), SMEM_P1_N64, dmp, stp, l, 1, first, nopa);
    else lk.launch(k_gru_p1_n32, dim3(cdiv(3 * d.D[l], GT_BN), cdiv(B, GT_BM)), dim3(GT_NTH_FEW), SMEM_P1, dmp, stp, l, 1, first, nopa);
    lk.close();
    lk.open(KN_GRU_P2);
    const dim3 g2(cdiv(d.D[l], GT_BN), cdiv(B, GT_BM));
    if (k.p2_deep[l]) lk.launch(k_gru_p2_w8d, g2, dim3(512), SMEM_P2_256, dmp, stp, l, 1, nopa);
    else lk.launch(k_gru_p2_w4, g2, dim3(GT_NTH), SMEM_NN, dmp, stp, l, 1, nopa);
    lk.close();
}

static void score_forward_and_loss(g4r_model* m, StepLauncher& lk, const int4* ent) {
    const DevModel& d = m->dm;
    const StepKernels& k = m->kern;
    const int L = d.n_layers, B = d.B;
    const DevModel* dmp = (const DevModel*)m->d_dm;
    StepState* stp = (StepState*)d.st;
    const int* meta = d.cur_in + 2 * B;
    lk.open(KN_SCORE_FWD);
    switch (k.score_fwd) {
    case SF_LEAN:
        lk.launch(d.logq != 0.f ? k_score_s<true> : k_score_s<false>, dim3(cdiv(d.ldSc, 32), cdiv(B, 32)), dim3(256), 0, m->d_leanS, meta, d.cur_col, d.hd[L - 1], d.Wy,
                  d.By, d.Sc, (unsigned)d.Dtop | ((unsigned)B << 16), (unsigned)d.N | ((unsigned)d.ldSc << 16), ent);
        break;
    case SF_MT:
        lk.launch(k_score_mt_4s, dim3(cdiv(B, 64) * cdiv(d.ldSc, 272)), dim3(256), SMEM_MT_4S, d.cur_col, meta, d.hd[L - 1], d.Wy, d.zrow, dmp,
                  (unsigned)d.Dtop | ((unsigned)cdiv(B, 64) << 16), d.N, d.ldSc, B);
        break;
    case SF_T3: lk.launch(k_score_fwd_t3, dim3(cdiv(d.ldSc, 64), cdiv(B, 64)), dim3(GT_NTH), SMEM_SF3, dmp, stp); break;
    case SF_T2: lk.launch(k_score_fwd_t2, dim3(cdiv(d.ldSc, 64), cdiv(B, 64)), dim3(GT_NTH), SMEM_SF2, dmp, stp); break;
    case SF_K64: lk.launch(k_score_fwd_k64, dim3(cdiv(d.ldSc, SFW_BN), cdiv(B, SF_BM)), dim3(GT_NTH), SMEM_SF64, dmp, stp); break;
    default: lk.launch(k_score_fwd_k128, dim3(cdiv(d.ldSc, GT_BN), cdiv(B, SF_BM)), dim3(GT_NTH), SMEM_SF, dmp, stp); break;
    }
    lk.close();
    lk.open(KN_LOSS);
    // a step that ends in k_update_l and whose owner table no window launch has written: up to one more workgroup per idle CU, the
    // owner pre-scan of its repeated items (g4r_loss_kernel.cuh)
    const int nown = std::min(cdiv(d.R, LOSS_NW), std::max(2 * m->n_cu - B, 32));
    launch_loss_rows(lk, dim3(B + (k.update == UP_LEAN && d.own_pos && !window_tables(m) ? nown : 0)));
    lk.close();
}

// per-kernel profiling times k_score_b with both roles in it (what the per-kernel tables price as the scoring backward), as it times
// the update in two launches: the moved form (role A in the top layer's k_gru_dy launch) is what graph replay and plain eager steps run
static inline bool score_a_hosted(const g4r_model* m, const StepLauncher& lk) { return m->kern.score_a_host && !lk.recs; }

static void score_backward(g4r_model* m, StepLauncher& lk, const int4* ent) {
    const DevModel& d = m->dm;
    const StepKernels& k = m->kern;
    const int L = d.n_layers, B = d.B;
    const DevModel* dmp = (const DevModel*)m->d_dm;
    StepState* stp = (StepState*)d.st;
    const int* meta = d.cur_in + 2 * B;
    const unsigned dimsN = (unsigned)d.N | ((unsigned)d.ldSc << 16);
    lk.open(KN_SCORE_BWD);
    switch (k.score_bwd) {
    case SB_LEAN: {
        const LeanB& q = m->h_leanB;
        const bool hosted = score_a_hosted(m, lk);      // role B alone: role A rides in the top layer's k_gru_dy launch (gru_backward)
        lk.launch(hosted ? k_score_b<false> : k_score_b<true>, dim3((hosted ? 0 : q.nA) + d.ksplit * q.nrb * q.ndb), dim3(512), 0, m->d_leanB, meta, d.cur_col, d.Sc,
                  d.hd[L - 1], d.Wy, d.accWy, (unsigned)d.Dtop | ((unsigned)B << 16), dimsN, ent);
        break;
    }
    case SB_BMT:
        lk.launch(k_score_bmt, dim3(2 * (d.ldSc / BMT_WA * (d.Dtop / 32))), dim3(256), SMEM_BMT, d.Sc, d.hd[L - 1], d.Wy, d.col_item, meta, d.zrow, dmp,
                  (unsigned)d.Dtop | ((unsigned)(d.Dtop / 32) << 16), dimsN, (unsigned)B | ((unsigned)d.kch << 16), (unsigned)cdiv(B, 64) | ((unsigned)(d.Dtop / 128) << 16));
        break;
    case SB_BWD2: {
        const int ndt = d.Dtop / 64, nrt = cdiv(B, 64);
        const int nA = cdiv(d.ldSc, 64) * ndt, nB = d.ksplit * nrt * ndt, nC = cdiv(d.ldSc, 64);
        lk.launch(k_score_bwd2, dim3(nA + nB + nC), dim3(GT_NTH), (size_t)(4 * 64 * 16) * sizeof(float) + (size_t)std::max(d.kch, 64) * sizeof(int), dmp, stp, nA, nB, ndt, nrt);
        break;
    }
    case SB_W: lk.launch(k_score_bwd_w, dim3(k.nblkA + k.nblkB), dim3(GT_NTH), SMEM_SBW + (size_t)d.kch * sizeof(int), dmp, stp, k.nblkA, k.ndtA, k.ndtB, k.nrtB); break;
    default: lk.launch(k_score_bwd_n, dim3(k.nblkA + k.nblkB), dim3(GT_NTH), std::max(SMEM_TN, SMEM_NN) + (size_t)d.kch * sizeof(int), dmp, stp, k.nblkA, k.ndtA, k.ndtB, k.nrtB); break;
    }
    lk.close();
}

static void gru_backward(g4r_model* m, StepLauncher& lk, int l, const int4* ent) {
    const DevModel& d = m->dm;
    const StepKernels& k = m->kern;
    const int L = d.n_layers, B = d.B;
    const DevModel* dmp = (const DevModel*)m->d_dm;
    StepState* stp = (StepState*)d.st;
    if (k.bwd[l] == BWD_LEAN) {
        const int nrb = cdiv(B, 16), gx = cdiv(d.IN[l], 16);
        const int* meta = d.cur_in + 2 * B;
        const LeanDa& q = m->h_leanDa[l];
        const LeanDy& y = m->h_leanDy[l];
        const unsigned dims = (unsigned)d.D[l] | ((unsigned)d.IN[l] << 16);
        lk.open(KN_GRU_DA);
        lk.launch(k_gru_da, dim3(cdiv(d.D[l], 16), nrb), dim3(128), 0, m->d_leanDa + l, meta, q.dsrc, q.Wh, q.z, q.c, q.H0, q.H1, (unsigned)d.D[l] | ((unsigned)q.ks << 16), B);
        lk.close();
        lk.open(KN_GRU_DY);
        if (score_a_hosted(m, lk) && l == L - 1) {
            // + k_score_b's role A, two tiles per workgroup, in grid rows behind the launch's own (k_gru_dy_a: what keeps the two
            // independent -- single-occurrence accumulator rows, no buffer one writes and the other reads -- is written there)
            const LeanB& b = m->h_leanB;
            lk.launch(k_gru_dy_a, dim3(gx, nrb + cdiv(cdiv(b.nA, 2), gx)), dim3(1024), 0, m->d_leanDy + l, meta, y.occ_idx, y.dV, y.drp, y.Wx, y.r, dims, B, m->d_leanB, d.cur_col,
                      d.Sc, d.hd[L - 1], d.accWy, (unsigned)d.Dtop | ((unsigned)B << 16), (unsigned)d.N | ((unsigned)d.ldSc << 16), (unsigned)b.nA | ((unsigned)b.ndh << 16), ent, l == 0 ? ent : nullptr);
        } else lk.launch(k_gru_dy, dim3(gx, nrb), dim3(1024), 0, m->d_leanDy + l, meta, y.occ_idx, y.dV, y.drp, y.Wx, y.r, dims, B, l == 0 ? ent : nullptr);
        lk.close();
        return;
    }
    if (k.bwd[l] == BWD_FUSED) {
        lk.open(KN_BWD_FUSED);
        lk.launch(k_gru_bwd_fused, dim3(cdiv(d.IN[l], 32), cdiv(B, BF_ROWS)), dim3(512), smem_bwd_fused(d.D[l]), dmp, stp, l);
        lk.close();
        return;
    }
    lk.open(KN_BWD_PRE);
    lk.launch(k_gru_bwd_pre, dim3(cdiv((long long)B * d.D[l], 256)), dim3(256), 0, dmp, stp, l);
    lk.close();
    lk.open(KN_BWD_A);
    dim3 ga(cdiv(d.D[l], GT_BN), cdiv(B, GT_BM));
    // behind k_score_bmt (raw gradient rows in the step plane) the top layer's launch carries their Adagrad rule: one extra
    // workgroup per 16 item rows (score_fin_rows)
    int nfin = 0;
    if (l == L - 1 && k.score_bwd == SB_BMT) { nfin = cdiv(cdiv(d.N, 16), (int)ga.x); ga.y += nfin; }
    if (k.ba_deep[l]) lk.launch(k_gru_bwd_a_w8d, ga, dim3(512), SMEM_BA_256, dmp, stp, l, nfin);
    else lk.launch(k_gru_bwd_a_w4, ga, dim3(GT_NTH), SMEM_NT, dmp, stp, l, nfin);
    lk.close();
    lk.open(KN_BWD_B);
    const WideGeo& G = k.wg[l];
    if (k.bwd[l] == BWD_ONEHOT) lk.launch(k_onehot_step, dim3(cdiv((long long)B * d.Ein, 4 * 256)), dim3(256), 0, dmp, stp);
    else if (k.bwd[l] == BWD_BW) lk.launch(k_gru_bwd_bw, dim3(cdiv(d.IN[l], 64) * cdiv(B, 64) * G.bbn), dim3(256), SMEM_T3, dmp, stp, l, G.bbn, G.bbk);
    else lk.launch(k_gru_bwd_b, dim3(cdiv(d.IN[l], GT_BN), cdiv(B, GT_BM)), dim3(GT_NTH_FEW), SMEM_BB, dmp, stp, l);
    lk.close();
}

// The dense gradients.  Merged: their tiles (+ fused dense Adagrad on a single GPU; gradients to the RCCL buffer otherwise) and the
// sparse row update in ONE launch (k_update_l / k_update): the two are independent, the all-reduce / dense apply of N > 1 follow behind
// (step_tail).  Else a launch of their own.
// (the dense-gradient tiles on a BRANCH of the step graph next to the sparse rows -- they share nothing -- were measured: the
// fork / join costs more than running them side by side gives, 126.6 -> 139.8 us per step at configs[2]; profiles/r05_experiments.md #8)
// k_update_l.  roles 0: the whole launch (bookkeeping, dense tiles, row workgroups); under g4r_profile(m, 2) its two halves as launches of
// their own -- 1: the dense tiles, 2: bookkeeping + row workgroups -- the same workgroups running the same code on the same operands, so
// a profiled step leaves the bits of an unprofiled one (the grid's block ranges are arguments: a half passes 0 for the ranges it leaves out).
// The step's owner table: its slot of the ring where a window launch wrote it, else slot 0 (the pre-scan in k_loss_rows).
static void launch_update_l(g4r_model* m, StepLauncher& lk, int slot, int roles) {
    const DevModel& d = m->dm;
    const int nb8 = cdiv(d.R, 8);
    const unsigned nbk = roles == 1 ? 0u : 1u + (unsigned)cdiv(d.ldSc, 512);
    const unsigned ntiles = roles == 2 ? 0u : (unsigned)m->ntiles16, nrow = roles == 1 ? 0u : (unsigned)nb8;
    const int* opos = (const int*)(m->d_tiles16 + m->ntiles16) + (window_tables(m) ? (size_t)slot * d.R * 16 : (size_t)0);
    lk.launch(d.mom > 0.f ? k_update_l<true> : k_update_l<false>, dim3(nbk + ntiles + nrow), dim3(512), 0, m->d_leanU, m->d_tiles16, d.occ_idx, d.occ_fl, d.dSx, d.dSy, d.dSBy,
              opos, ntiles | ((unsigned)nb8 << 16), (unsigned)d.R | ((unsigned)d.B << 16), nbk, step_entries(m, slot));
}

static void dense_gradients(g4r_model* m, StepLauncher& lk, int slot) {
    const DevModel& d = m->dm;
    const StepKernels& k = m->kern;
    const int B = d.B;
    const DevModel* dmp = (const DevModel*)m->d_dm;
    StepState* stp = (StepState*)d.st;
    const dim3 gfin(cdiv((long long)B * (d.IN[0] / 4), 256));      // k_finish_rows: dy of layer 0 from K-slice partial sums
    const bool mo = d.mom > 0.f;
    if (!update_merged(m, lk)) {
        lk.open(KN_DENSE);
        if (k.update == UP_LEAN) launch_update_l(m, lk, slot, 1);      // (its other half: step_tail)
        else if (k.wide_dense) lk.launch(k_dense_grad2, dim3(m->ntiles64 + (d.bbn[0] > 0 ? gfin.x : 0)), dim3(256), SMEM_T2K, dmp, stp, m->d_tiles64, m->ntiles64);
        else {
            if (k.finish_rows) lk.launch(k_finish_rows, gfin, dim3(256), 0, dmp, stp);
            lk.launch(k_dense_grad<32>, dim3(m->ntiles), dim3(GT_NTH_FEW), SMEM_TN, dmp, stp, m->d_tiles);
        }
        lk.close();
        return;
    }
    if (k.finish_rows) {      // (with the merged update: only when asked for, G4R_WIDE2)
        lk.open(KN_FINISH);
        lk.launch(k_finish_rows, gfin, dim3(256), 0, dmp, stp);
        lk.close();
    }
    lk.open(KN_UPDATE);
    if (k.update == UP_LEAN) launch_update_l(m, lk, slot, 0);
    else
        lk.launch(K_UPDATE[k.chunks == 1 ? 0 : 1][mo], dim3(m->ntiles + m->nblk_occ + 1), dim3(SP_WAVES * 64), std::max(SMEM_TN, m->smem_sparse), dmp, stp, m->d_tiles,
                  m->ntiles, m->nblk_occ);
    lk.close();
}

// Every launch of a training step, in order, as m->kern chose them (choose_kernels): step_head, then step_tail.
// The head: everything up to the dense gradients or the merged update.
// slot: the step's index in its window (a graph's steps: their index in the graph; eager steps: g4r_train_steps' windows) -- the table
// of the owner ring k_owner_window wrote for it (g4r_update_kernels.cuh); 0 where the pre-scan in k_loss_rows writes the table
static int step_head(g4r_model* m, StepLauncher& lk, int slot) {
    const int L = m->dm.n_layers;
    const int4* ent = step_entries(m, slot);
    for (int l = 0; l < L; ++l) gru_forward(m, lk, l, ent);
    score_forward_and_loss(m, lk, ent);
    score_backward(m, lk, ent);
    for (int l = L - 1; l >= 0; --l) gru_backward(m, lk, l, ent);
    dense_gradients(m, lk, slot);
    HIPCHK(hipGetLastError());
    return 0;
}

// The tail: all-reduce, clip, dense apply, sparse update -- what the step has left behind its head (nothing on a single GPU with the
// merged update).
// multi-rank: dense-gradient all-reduce, dense Adagrad, then the sparse embedding update, in stream order.
// (running the first two on a stream of their own next to the sparse update -- which touches item rows only -- was measured on one
// MI355X with a one-rank communicator: the two cross-stream event dependencies cost ~20 us per step, more than the ~11 us of sparse
// update they can hide; that path was removed in round 6)
// k_p2p_allreduce, the RCCL calls, k_grad_sqsum / k_grad_clip and k_exact_occ are no slot's launches: neither G4R_SKIP_KN nor
// per-dispatch events apply to them.
static int step_tail(g4r_model* m, StepLauncher& lk) {
    const DevModel& d = m->dm;
    const StepKernels& k = m->kern;
    hipStream_t s = m->stream;
    const DevModel* dmp = (const DevModel*)m->d_dm;
    StepState* stp = (StepState*)d.st;
    if (!d.apply_dense_inplace) {
        // staged dense path: (RCCL all-reduce when there are ranks) -> (global gradient norm -> clip factor, generic path with
        // grad_cap) -> dense rule on the flat gradient buffer
        const bool dist = !m->virtual_ranks && (m->cfg.nranks > 1 || m->comm_ready || m->p2p_ready);
        if (m->cfg.nranks > 1 && !m->comm_ready && !m->p2p_ready && !m->virtual_ranks) return fail("nranks > 1 but g4r_comm_init was not called");
        if (dist && !m->exact) {      // (exact-replica mode: the dense gradients travel with the all-gather of the occurrence blocks below)
            lk.open(KN_ALLREDUCE);
            if (lk.ev_a) (void)hipEventRecord(lk.ev_a, s);
            if (m->p2p_ready) hipLaunchKernelGGL(k_p2p_allreduce, dim3(m->p2p_nblk), dim3(256), 0, s, m->p2p_args, (float*)d.dense_g);
            else NCCLCHK(ncclAllReduce(d.dense_g, d.dense_g, d.dense_count, ncclFloat, ncclSum, m->comm, s));
            if (lk.ev_b) (void)hipEventRecord(lk.ev_b, s);
            lk.close();
        }
        if (d.generic && d.grad_cap > 0.f) {
            hipLaunchKernelGGL(k_grad_sqsum, dim3(G4R_NORM_BLOCKS), dim3(256), 0, s, dmp, stp);
            hipLaunchKernelGGL(k_grad_clip, dim3(1), dim3(64), 0, s, dmp);
        }
        // (generic optimizer path: the dense rule runs as extra workgroups of the sparse update's launch below)
        if (!d.generic) {
            lk.open(KN_DENSE_APPLY);
            lk.launch(k_dense_apply, dim3(cdiv(d.dense_count, 256)), dim3(256), 0, dmp);
            lk.close();
        }
    }
    if (d.generic) {
        // generic optimizer path: the sparse rule on raw per-occurrence gradients
        int nblk_g = m->nblk_occ_g;
        size_t smem_g = m->smem_sparse;
        if (m->exact) {
            // exact-replica mode: every rank's block of (occurrence list, gradient rows) to every rank, then the (last, first, count)
            // table of the concatenated list; the update below then runs over nranks * R occurrences, identically on every rank
            if (!m->virtual_ranks) {      // (virtual ranks: g4r_virtual_train_steps has copied the blocks)
                if (!m->comm_ready) return fail("sparse_exact needs the RCCL communicator (g4r_comm_init)");
                NCCLCHK(ncclAllGather((const float*)d.xbase + (size_t)m->cfg.rank * (size_t)d.xstride, (float*)d.xbase, (size_t)d.xstride, ncclFloat, m->comm, s));
            }
            const long long rlist = d.xmode == 3 ? (long long)d.xn * 2 * d.B + d.ns : (long long)d.R * d.xn;      // xlist_len
            hipLaunchKernelGGL(k_exact_occ, dim3(cdiv(rlist, 256)), dim3(256), 0, s, dmp);
            nblk_g = cdiv(rlist, SP_WAVES);
            smem_g = m->smem_exact;
        }
        const int nda = d.apply_dense_inplace ? 0 : cdiv(d.dense_count, SP_WAVES * 64);      // workgroups of the dense rule behind the row blocks
        lk.open(KN_SPARSE);
        lk.launch(K_SPARSE_UPDATE_GENERIC[chunk_index(k.chunks)], dim3(nblk_g + 1 + nda), dim3(SP_WAVES * 64), smem_g, dmp, stp, nblk_g, nda);
        lk.close();
    } else if (!update_merged(m, lk)) {
        lk.open(KN_SPARSE);
        if (k.update == UP_LEAN) launch_update_l(m, lk, 0, 2);      // (no window launch in front of such a step: slot 0, the null entry slot)
        else lk.launch(K_SPARSE_UPDATE[chunk_index(k.chunks)][d.mom > 0.f], dim3(m->nblk_occ + 1), dim3(SP_WAVES * 64), m->smem_sparse, dmp, stp, m->nblk_occ);
        lk.close();
    }
    HIPCHK(hipGetLastError());
    return 0;
}

// one whole step, unprofiled (the capture of the step graphs, plain eager steps)
static int whole_step(g4r_model* m, int slot) {
    StepLauncher lk(m, nullptr);
    return step_head(m, lk, slot) || step_tail(m, lk) ? -1 : 0;
}

static int apply_compaction(g4r_model* m, int64_t ci) {
    // gru4rec.py:647-651: H[i] <- H[i][valid_mask]; the current hidden state lives in H[l][gstep & 1]
    DevModel& d = m->dm;
    const int B = d.B;
    for (int l = 0; l < d.n_layers; ++l) {
        float* Hc = d.H[l][m->gstep & 1];
        const int W = d.D[l];
        hipLaunchKernelGGL(k_gather_rows, dim3(cdiv((long long)B * W, 256)), dim3(256), 0, m->stream, m->d_tmpH, (const float*)Hc,
                           (const int*)(m->d_cmaps + ci * B), B, W);
        HIPCHK(hipMemcpyAsync(Hc, m->d_tmpH, (size_t)B * W * sizeof(float), hipMemcpyDeviceToDevice, m->stream));
    }
    return 0;
}
// the host-scheduled events that sit in front of plan step t: batch compaction (*ci: the next entry of compact_steps), sample-store refill
static int between_steps(g4r_model* m, int64_t t, size_t* ci) {
    while (*ci < m->compact_steps.size() && m->compact_steps[*ci] == t) { if (apply_compaction(m, (int64_t)*ci)) return -1; ++*ci; }
    if (m->dm.ns > 0 && !m->store_frozen && m->gstep > 0 && m->gstep % m->gl == 0) {
        if (refill_store(m)) return -1;      // gru4rec.py:618-620
        hipLaunchKernelGGL(k_restage_inputs, dim3(1), dim3(512), 0, m->stream, (const DevModel*)m->d_dm, (StepState*)m->dm.st);
    }
    return 0;
}

#define G4R_GRAPH_STEPS 16
#define G4R_GRAPH_STEPS_SMALL 4
// `n` whole steps captured from the model's stream into an executable graph
static int capture_steps(g4r_model* m, int n, hipStreamCaptureMode cmode, hipGraphExec_t* out) {
    hipGraph_t graph = nullptr;
    HIPCHK(hipStreamBeginCapture(m->stream, cmode));
    int rc = 0;
    for (int i = 0; i < n && !rc; ++i) rc = whole_step(m, i);
    hipError_t e = hipStreamEndCapture(m->stream, &graph);
    if (rc || e != hipSuccess || !graph) {
        if (graph) (void)hipGraphDestroy(graph);
        (void)hipGetLastError();
        if (!rc) fail(std::string("graph capture: ") + hipGetErrorString(e));
        return -1;
    }
    e = hipGraphInstantiate(out, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (e != hipSuccess) { *out = nullptr; (void)hipGetLastError(); return fail(std::string("graph instantiate: ") + hipGetErrorString(e)); }
    return 0;
}
static int ensure_graph(g4r_model* m) {
    if (m->gexec) return 0;
    const bool dist = !m->dm.apply_dense_inplace && !local_staged(m);
    const bool rccl_in_graph = dist && (!m->p2p_ready || (m->exact && m->comm_ready));      // (exact replicas: the step's collective is RCCL's all-gather even when the peer-memory all-reduce is attached)
    if (dist) {
        // RCCL sets its channels up on first use: that must not happen inside a capture (dense_g is scratch between steps)
        if (!m->p2p_ready) NCCLCHK(ncclAllReduce(m->dm.dense_g, m->dm.dense_g, m->dm.dense_count, ncclFloat, ncclSum, m->comm, m->stream));
        if (m->exact && m->comm_ready)      // the exact-replica step's collective is an all-gather: connect what THAT needs outside the capture, too
            NCCLCHK(ncclAllGather((const float*)m->dm.xbase + (size_t)m->cfg.rank * (size_t)m->dm.xstride, (float*)m->dm.xbase, (size_t)m->dm.xstride,
                                  ncclFloat, m->comm, m->stream));
        HIPCHK(hipStreamSynchronize(m->stream));
    }
    if (capture_steps(m, G4R_GRAPH_STEPS, rccl_in_graph ? hipStreamCaptureModeRelaxed : hipStreamCaptureModeThreadLocal, &m->gexec)) return -1;
    m->graph_steps = G4R_GRAPH_STEPS;
    if (!dist) {
        // a second, short graph: a run of 20 steps replays 16 + 4 instead of 16 + four eager steps (six launches each).  Best
        // effort: without it the remainder is launched eagerly as before.
        if (capture_steps(m, G4R_GRAPH_STEPS_SMALL, hipStreamCaptureModeThreadLocal, &m->gexec_small)) m->gexec_small = nullptr;
    }
    return 0;
}
static int ensure_head_graph(g4r_model* m) {
    if (m->gexec_head) return 0;
    hipGraph_t graph;
    StepLauncher lk(m, nullptr);
    HIPCHK(hipStreamBeginCapture(m->stream, hipStreamCaptureModeThreadLocal));
    if (step_head(m, lk, 0)) { hipGraph_t g2; (void)hipStreamEndCapture(m->stream, &g2); return -1; }
    HIPCHK(hipStreamEndCapture(m->stream, &graph));
    HIPCHK(hipGraphInstantiate(&m->gexec_head, graph, nullptr, nullptr, 0));
    (void)hipGraphDestroy(graph);
    return 0;
}
// the step graph for this model: the whole step (single GPU; N > 1 with RCCL captured), or -- if RCCL cannot be captured on this
// runtime -- the head graph with an eager tail.  Returns 0 / -1; step_mode(m) tells which one is ready.
static int ensure_step_graph(g4r_model* m) {
    if (m->dm.apply_dense_inplace) return ensure_graph(m);
    if (dist_graph_wanted(m)) {
        if (ensure_graph(m) == 0) return 0;
        m->dist_graph_failed = true;
        fprintf(stderr, "[g4r] RCCL all-reduce could not be captured into the step graph (%s); launching it eagerly\n", g_err.c_str());
    }
    return ensure_head_graph(m);
}

// A window of `nw` steps -- one graph replay, or up to G4R_DEFER_SLOTS eager steps: open() in front of them, close() behind.  Deferred row
// updates: which rows may wait (scan), ... steps ..., their flush.  Where the steps end in k_update_l with the owner tables on: the tables
// of the window's steps (k_owner_window: slot i of the ring = step i of the window).  A call that fails between a window's scan and its
// flush launch leaves the handle broken (defer_broken): the row updates pending then are lost.
struct StepWindow {
    g4r_model* m;
    const bool own_win;
    bool scanned = false;
    explicit StepWindow(g4r_model* m_) : m(m_), own_win(window_tables(m_)) {}
    ~StepWindow() { if (scanned) m->defer_broken = true; }
    bool on() const { return m->defer_on || own_win; }
    // t, g: plan step and global step of the window's first step
    int open(int64_t t, int64_t g, int64_t nw) {
        const DevModel& d = m->dm;
        const DevModel* dmp = (const DevModel*)m->d_dm;
        if (own_win) {
            StepLauncher lk(m, nullptr);      // (G4R_SKIP_KN, tools/kn_cost.py: what the window launch costs a step)
            if (m->profiling) for (auto& e : m->ev_ow) if (!e) (void)hipEventCreate(&e);
            lk.use(KN_OWNER_WINDOW, m->profiling ? m->ev_ow[0] : nullptr, m->profiling ? m->ev_ow[1] : nullptr);
            const int hs = window_entries(m) ? m->pos_hs : 0;      // the steps' per-position entries with their owner tables
            lk.launch(k_owner_window, dim3((unsigned)(nw * cdiv(2 * d.B, OW_NW))), dim3(OW_T), (size_t)(((d.R + 3) & ~3) + 16 * OW_NW + 4 * hs) * sizeof(int), dmp, t, g, nw, hs);
            HIPCHK(hipGetLastError());      // (a refused launch would leave the steps the tables of an older window)
        }
        if (!m->defer_on) return 0;
        scanned = true;
        const dim3 gs(cdiv(nw * d.R, 256));
        if (m->profiling) (void)hipEventRecord(m->ev_df[0], m->stream);
        hipLaunchKernelGGL(k_defer_scan, gs, dim3(256), 0, m->stream, dmp, (long long)t, (long long)g, (int)nw, 0);
        hipLaunchKernelGGL(k_defer_scan, gs, dim3(256), 0, m->stream, dmp, (long long)t, (long long)g, (int)nw, 1);
        if (m->profiling) (void)hipEventRecord(m->ev_df[1], m->stream);
        return 0;
    }
    int close(int64_t g, int64_t nw) {
        auto timed = [&](int kn, hipEvent_t a, hipEvent_t b) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, a, b) == hipSuccess) { m->kn_ms[kn] += ms; m->kn_n[kn]++; }
        };
        if (own_win) {
            m->own_last = (int)nw - 1;
            if (m->profiling) {
                HIPCHK(hipStreamSynchronize(m->stream));
                timed(KN_OWNER_WINDOW, m->ev_ow[0], m->ev_ow[1]);
            }
        }
        if (!m->defer_on) return 0;
        if (m->profiling) (void)hipEventRecord(m->ev_df[2], m->stream);
        hipLaunchKernelGGL(k_sparse_flush, dim3(cdiv(nw * m->dm.dRcap, SP_WAVES * FL_NR)), dim3(SP_WAVES * 64), 0, m->stream, (const DevModel*)m->d_dm, (long long)g, (int)nw);
        if (m->profiling) {
            (void)hipEventRecord(m->ev_df[3], m->stream);
            HIPCHK(hipStreamSynchronize(m->stream));
            timed(KN_SCAN, m->ev_df[0], m->ev_df[1]);
            timed(KN_FLUSH, m->ev_df[2], m->ev_df[3]);
        }
        scanned = false;
        return 0;
    }
};

// one step outside a graph replay, in mode `mode` (single_step_mode)
static int single_step(g4r_model* m, StepMode mode, int slot, std::vector<EvRec>& recs) {
    if (m->profiling) {
        // per-kernel durations: start/stop events attached to every dispatch (hipExtLaunchKernelGGL), i.e. the
        // kernel's own begin/end timestamps -- the quantity rocprofv3 --kernel-trace reports; eager launches
        recs.clear();
        StepLauncher lk(m, &recs);
        if (step_head(m, lk, slot) || step_tail(m, lk)) return -1;
        HIPCHK(hipStreamSynchronize(m->stream));
        for (auto& r : recs) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) { m->kn_ms[r.kn] += ms; m->kn_n[r.kn]++; }
        }
        return 0;
    }
    if (mode != STEP_HEAD_GRAPH) return whole_step(m, slot);
    // staged dense path: the step's compute kernels replay from a graph; the RCCL all-reduce, the dense apply and the sparse update
    // are launched eagerly behind it
    if (ensure_head_graph(m)) return -1;
    HIPCHK(hipGraphLaunch(m->gexec_head, m->stream));
    StepLauncher lk(m, nullptr);
    return step_tail(m, lk);
}

int g4r_train_steps(g4r_model* m, int64_t t0, int64_t n_steps) {
    if (!m) return fail("null model");
    if (!m->d_in) return fail("no plan uploaded");
    if (t0 < 0 || n_steps < 0 || t0 + n_steps > m->T) return fail("step range outside the plan");
    if (m->dm.ns > 0 && !m->have_pop && !m->store_frozen) return fail("negative sampling needs g4r_set_popularity first");
    weights_changed(m);      // (deferred row updates are flushed inside this call: they are covered too)
    if (m->defer_on) {
        // k_defer_scan keys its newest-use table by the low 32 bits of the global step (signed atomicMax): refuse before they wrap
        // (27 h of training at 22 K steps/s on one handle; g4r_set_step_counters rebases the step and clears the table)
        if (m->gstep + n_steps >= ((int64_t)1 << 31) - 64) return fail("deferred row updates: the global step would pass 2^31 -- rebase it with g4r_set_step_counters (epoch boundary) or create the model without defer_updates");
        if (m->defer_broken) return fail("deferred row updates: an earlier call failed between a window's scan and its flush launch; the row updates pending then are lost -- recreate the model");
    }
    StepWindow win(m);
    HIPCHK(hipSetDevice(m->cfg.device));
    hipLaunchKernelGGL(k_set_state, dim3(1), dim3(512), 0, m->stream, (const DevModel*)m->d_dm, (StepState*)m->dm.st, (long long)t0, (long long)m->gstep);
    StepMode mode = step_mode(m);
    if (mode == STEP_GRAPH && !m->dm.apply_dense_inplace) {      // (the fused single-GPU step captures at its first run long enough, below)
        if (ensure_step_graph(m)) return -1;
        mode = step_mode(m);
    }
    const StepMode single = single_step_mode(m, mode);
    size_t ci = std::lower_bound(m->compact_steps.begin(), m->compact_steps.end(), t0) - m->compact_steps.begin();
    int64_t t = t0;
    const int64_t tend = t0 + n_steps;
    std::vector<EvRec> recs;
    while (t < tend) {
        if (between_steps(m, t, &ci)) return -1;
        const bool devsync = m->sync_every_dev > 0 && m->comm_ready;
        if (devsync && m->since_sync >= m->sync_every_dev) {
            if (sync_dense_enqueue(m)) return -1;
            ++m->n_dev_syncs;
        }
        // steps until the next event
        int64_t run = tend - t;
        if (devsync) run = std::min<int64_t>(run, m->sync_every_dev - m->since_sync);
        if (ci < m->compact_steps.size()) run = std::min(run, m->compact_steps[ci] - t);
        if (m->dm.ns > 0 && !m->store_frozen) run = std::min<int64_t>(run, m->gl - (m->gstep % m->gl));
        if (run <= 0) return fail("internal: empty run");
        // the run, window by window: the big graph while it fits, then the small one (where there is one), then eager steps -- in windows
        // of up to G4R_DEFER_SLOTS where deferral or the owner tables want windows, else one by one
        const bool replay = mode == STEP_GRAPH && run >= G4R_GRAPH_STEPS_SMALL;
        if (replay && ensure_graph(m)) return -1;
        for (int64_t done = 0, nw; done < run; done += nw) {
            const int64_t left = run - done;
            hipGraphExec_t g = nullptr;
            if (replay && left >= m->graph_steps) { g = m->gexec; nw = m->graph_steps; }
            else if (replay && m->gexec_small && left >= G4R_GRAPH_STEPS_SMALL) { g = m->gexec_small; nw = G4R_GRAPH_STEPS_SMALL; }
            else nw = win.on() ? std::min<int64_t>(G4R_DEFER_SLOTS, left) : 1;
            const bool windowed = g || win.on();
            if (windowed && win.open(t + done, m->gstep + done, nw)) return -1;
            if (g) HIPCHK(hipGraphLaunch(g, m->stream));
            else for (int i = 0; i < nw; ++i) if (single_step(m, single, windowed ? i : 0, recs)) return -1;
            if (windowed && win.close(m->gstep + done, nw)) return -1;
        }
        t += run;
        m->gstep += run;
        m->since_sync += run;
    }
    HIPCHK(hipStreamSynchronize(m->stream));
    if (m->p2p_ready) {
        unsigned late = 0;
        HIPCHK(hipMemcpy(&late, m->p2p_round + m->p2p_nblk, sizeof(late), hipMemcpyDeviceToHost));
        if (late) return fail("p2p all-reduce: a peer did not publish its gradients within G4R_P2P_TIMEOUT_MS (dead rank?)");
    }
    return 0;
}

// ---- virtual ranks ------------------------------------------------------------------------------------------------------
// n handles on ONE device stand in for the n ranks of a data-parallel run (each created with nranks = n, its own rank, its own
// plan): every step runs each handle's kernels up to the dense gradients, sums the n gradient buffers in rank order -- what the
// RCCL all-reduce delivers -- and lets each handle apply the sum (k_dense_apply divides by nranks) next to its GPU-local sparse
// update.  Item tables are reconciled by the caller with g4r_sync_export / g4r_sync_import.  Validation only (three stream
// synchronisations per step): the numbers it produces are what an n-GPU run computes, not how fast.
int g4r_virtual_train_steps(g4r_model* const* ms, int32_t n, int64_t t0, int64_t n_steps) {
    if (!ms || n < 1 || n > 16) return fail("virtual ranks: 1..16 handles");
    for (int q = 0; q < n; ++q) {
        g4r_model* m = ms[q];
        if (!m || !m->d_in) return fail("virtual ranks: null model / no plan uploaded");
        if (m->cfg.nranks != n || m->cfg.rank != q) return fail("virtual ranks: handle q must be created with rank = q, nranks = n");
        if (m->cfg.device != ms[0]->cfg.device || m->dm.dense_count != ms[0]->dm.dense_count || m->exact != ms[0]->exact || m->dm.xstride != ms[0]->dm.xstride)
            return fail("virtual ranks: handles differ");
        if (m->comm_ready || m->p2p_ready) return fail("virtual ranks: the handle already has a communicator / peer mappings");
        if (t0 < 0 || n_steps < 0 || t0 + n_steps > m->T) return fail("step range outside the plan");
        if (m->dm.ns > 0 && !m->have_pop && !m->store_frozen) return fail("negative sampling needs g4r_set_popularity first");
        m->virtual_ranks = true;
    }
    for (int q = 0; q < n; ++q) weights_changed(ms[q]);
    HIPCHK(hipSetDevice(ms[0]->cfg.device));
    g4r_model* m0 = ms[0];
    const int cnt = m0->dm.dense_count;
    if (!m0->d_vsum && dalloc(m0, &m0->d_vsum, (size_t)cnt)) return -1;
    VSumArgs va;
    memset(&va, 0, sizeof(va));
    std::vector<size_t> ci(n);
    for (int q = 0; q < n; ++q) {
        g4r_model* m = ms[q];
        va.src[q] = m->dm.dense_g; va.dst[q] = m->dm.dense_g;
        hipLaunchKernelGGL(k_set_state, dim3(1), dim3(512), 0, m->stream, (const DevModel*)m->d_dm, (StepState*)m->dm.st, (long long)t0, (long long)m->gstep);
        ci[q] = std::lower_bound(m->compact_steps.begin(), m->compact_steps.end(), t0) - m->compact_steps.begin();
    }
    for (int64_t t = t0; t < t0 + n_steps; ++t) {
        for (int q = 0; q < n; ++q) {
            g4r_model* m = ms[q];
            StepLauncher lk(m, nullptr);
            if (between_steps(m, t, &ci[q]) || step_head(m, lk, 0)) return -1;
        }
        for (int q = 0; q < n; ++q) HIPCHK(hipStreamSynchronize(ms[q]->stream));
        if (m0->exact) {
            // what the all-gather of the exact-replica mode delivers: every handle's own block into every other handle's buffer
            for (int q = 0; q < n; ++q)
                for (int p = 0; p < n; ++p)
                    if (p != q) HIPCHK(hipMemcpyAsync((float*)ms[q]->dm.xbase + (size_t)p * (size_t)m0->dm.xstride,
                                                      (const float*)ms[p]->dm.xbase + (size_t)p * (size_t)m0->dm.xstride,
                                                      (size_t)m0->dm.xstride * sizeof(float), hipMemcpyDeviceToDevice, ms[q]->stream));
            // (the next step's kernels of handle p rewrite p's block: every copy out of it must have run before p's tail is queued)
            for (int q = 0; q < n; ++q) HIPCHK(hipStreamSynchronize(ms[q]->stream));
        }
        if (!m0->exact) {      // (exact-replica mode: the blocks carry the dense gradients, every handle sums them itself)
            hipLaunchKernelGGL(k_virtual_sum, dim3(cdiv(cnt, 256)), dim3(256), 0, m0->stream, va, n, cnt, m0->d_vsum);
            hipLaunchKernelGGL(k_virtual_bcast, dim3(cdiv(cnt, 256)), dim3(256), 0, m0->stream, va, n, cnt, (const float*)m0->d_vsum);
            HIPCHK(hipStreamSynchronize(m0->stream));
        }
        for (int q = 0; q < n; ++q) {
            StepLauncher lk(ms[q], nullptr);
            if (step_tail(ms[q], lk)) return -1;
            ms[q]->gstep += 1;
        }
    }
    for (int q = 0; q < n; ++q) HIPCHK(hipStreamSynchronize(ms[q]->stream));
    return 0;
}

int g4r_get_losses(g4r_model* m, int64_t t0, int64_t n, float* out) {
    if (!m || !out) return fail("null argument");
    if (t0 < 0 || n < 0 || t0 + n > m->T) return fail("range outside the plan");
    HIPCHK(hipSetDevice(m->cfg.device));
    HIPCHK(hipStreamSynchronize(m->stream));
    HIPCHK(hipMemcpy(out, m->d_loss + t0, n * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}
int g4r_synchronize(g4r_model* m) {
    if (!m) return fail("null model");
    HIPCHK(hipSetDevice(m->cfg.device));
    HIPCHK(hipStreamSynchronize(m->stream));
    return 0;
}
int64_t g4r_global_step(g4r_model* m) { return m ? m->gstep : -1; }
int64_t g4r_refills(g4r_model* m) { return m ? (int64_t)m->refills : -1; }
// resume: continue the counter-based random streams (dropout masks are keyed by the global step, the sample store by its refill
// number) where a checkpointed run stopped; the store is regenerated as that run's last refill left it
int g4r_set_step_counters(g4r_model* m, int64_t global_step, int64_t refills) {
    if (!m) return fail("null model");
    if (global_step < 0 || refills < 0) return fail("negative counter");
    HIPCHK(hipSetDevice(m->cfg.device));
    m->gstep = global_step;
    if (m->defer_on)      // (the scan's "newest step that gathers the item" table is keyed by the global step)
        HIPCHK(hipMemsetAsync(m->dm.last_use, 0, (size_t)(m->cfg.embed_mode != G4R_EMBED_CONSTRAINED ? 2 : 1) * m->dm.n_items * sizeof(int), m->stream));
    if (m->dm.ns > 0 && !m->store_frozen) {
        if (!m->have_pop) return fail("g4r_set_popularity first");
        if (refills < 1) return fail("a model with negative sampling has filled its store at least once");
        m->refills = (unsigned)(refills - 1);
        if (refill_store(m)) return -1;
        HIPCHK(hipStreamSynchronize(m->stream));
    } else {
        m->refills = (unsigned)refills;
    }
    return 0;
}
int g4r_profile(g4r_model* m, int32_t enable) {
    if (!m) return fail("null model");
    m->profiling = enable != 0;
    m->profile_split = enable == 2;      // the sparse row update timed ALONE (k_sparse_update next to k_dense_grad instead of the merged k_update)
    if (enable) for (int i = 0; i < KN_COUNT; ++i) { m->kn_ms[i] = 0; m->kn_n[i] = 0; }
    return 0;
}
int g4r_kernel_time(g4r_model* m, int32_t which, const char** name, double* total_ms, int64_t* launches) {
    if (!m || which < 0 || which >= KN_COUNT) return fail("bad kernel index");
    if (name) *name = KN_NAMES[which];
    if (total_ms) *total_ms = m->kn_ms[which];
    if (launches) *launches = m->kn_n[which];
    return 0;
}

int g4r_reset_hidden(g4r_model* m) {
    if (!m) return fail("null model");
    HIPCHK(hipSetDevice(m->cfg.device));
    for (int l = 0; l < m->dm.n_layers; ++l)
        for (int q = 0; q < 2; ++q)
            HIPCHK(hipMemsetAsync(m->dm.H[l][q], 0, (size_t)m->dm.B * m->dm.D[l] * sizeof(float), m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    return 0;
}

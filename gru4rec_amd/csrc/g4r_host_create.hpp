// g4r_host_create.hpp -- part of libgru4rec_hip.so's host code; included once, by g4r_api.hip (one translation unit: the kernels are templates
// instantiated there).  Holds: g4r_device_count / g4r_sizeof_config / g4r_create (the memory plan: every buffer of the step is allocated here) / g4r_destroy.

int g4r_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}
const char* g4r_last_error(void) { return g_err.c_str(); }
#ifndef G4R_HIPCC_VERSION
#define G4R_HIPCC_VERSION "unknown"
#endif
// library version, target, and the hipcc the device code was generated with (gru4rec_amd/build.py passes it; the same build
// audits the generated code for premature uses of hand-counted asm loads and refuses to install a library that has one)
const char* g4r_version(void) { return "gru4rec_hip 0.4 (gfx950; hipcc " G4R_HIPCC_VERSION "; isa-audited)"; }
int g4r_sizeof_config(void) { return (int)sizeof(g4r_config); }

// argument blocks of the lean kernels the step runs (g4r_lean_kernels.cuh): everything they read from the model, from pointers that are
// final here.  Those of k_score_s and k_update_l also carry the device descriptor's address: g4r_create uploads them once that exists.
static int build_lean_args(g4r_model* m) {
    DevModel& d = m->dm;
    const StepKernels& k = m->kern;
    const int L = d.n_layers;
    std::vector<LeanV> av(L); std::vector<LeanH> ah(L); std::vector<LeanDa> aa(L); std::vector<LeanDy> ay(L);
    const bool constrained = d.embed_mode == G4R_EMBED_CONSTRAINED;
    bool any_layer = false;
    for (int l = 0; l < L; ++l) {
        if (k.fwd[l] != FWD_LEAN) continue;
        any_layer = true;
        LeanV& v = av[l]; memset(&v, 0, sizeof(v));
        v.Wx = d.dense_p + d.offWx[l]; v.Wrz = d.dense_p + d.offWrz[l]; v.Bh = d.dense_p + d.offBh[l];
        v.H0 = d.H[l][0]; v.H1 = d.H[l][1];
        v.ysrc = (l == 0) ? (constrained ? d.Wy : d.E) : d.hd[l - 1];
        v.cur_in = d.cur_in; v.Vc = d.Vc[l]; v.r = d.r[l]; v.Hr = d.Hr[l]; v.z = d.z[l]; v.yin0 = d.yin0;
        v.occ_idx = d.occ_idx; v.occ_fl = d.occ_fl + 4 * (constrained ? (size_t)0 : (size_t)d.n_items);
        v.st = d.st; v.seed = d.seed; v.B = d.B; v.D = d.D[l]; v.IN = d.IN[l]; v.R = d.R; v.first = (l == 0) ? 1 : 0; v.pub_fl = d.xmode == 0 ? 1 : 0;
        v.drop_e = d.drop_e; v.dbg = d.dbgclk; v.dbgtile = d.dbgtile; v.n_items = d.n_items;
        LeanH& h = ah[l]; memset(&h, 0, sizeof(h));
        h.Wh = d.dense_p + d.offWh[l]; h.H0 = d.H[l][0]; h.H1 = d.H[l][1]; h.Hr = d.Hr[l]; h.Vc = d.Vc[l]; h.z = d.z[l];
        h.cur_rst = d.cur_in + d.B; h.c = d.c[l]; h.hd = d.hd[l]; h.st = d.st; h.seed = d.seed; h.B = d.B; h.D = d.D[l];
        h.hidden_act = d.hidden_act; h.stream = (int)(G4R_STREAM_DROP_HIDDEN + (unsigned)l); h.ha_p0 = d.ha_p0; h.ha_p1 = d.ha_p1; h.drop_h = d.drop_h; h.dbg = d.dbgclk; h.dbgtile = d.dbgtile;
        LeanDa& q = aa[l]; memset(&q, 0, sizeof(q));
        q.Wh = h.Wh; q.H0 = h.H0; q.H1 = h.H1; q.z = d.z[l]; q.c = d.c[l];
        if (l == L - 1) { q.dsrc = d.dhpart; q.ks = d.ksplit; }
        else if (d.bbn[l + 1] > 0) { q.dsrc = d.dyp; q.ks = d.bbn[l + 1]; }
        else { q.dsrc = d.dyl[l]; q.ks = 1; }
        q.dV = d.dV[l]; q.drp = d.drp; q.st = d.st; q.seed = d.seed; q.B = d.B; q.D = d.D[l]; q.hidden_act = d.hidden_act; q.stream = h.stream;
        q.ha_p0 = d.ha_p0; q.ha_p1 = d.ha_p1; q.drop_h = d.drop_h; q.dbg = d.dbgclk; q.dbgtile = d.dbgtile;
        LeanDy& y = ay[l]; memset(&y, 0, sizeof(y));
        y.Wx = v.Wx; y.H0 = h.H0; y.H1 = h.H1; y.r = d.r[l]; y.drp = d.drp; y.dV = d.dV[l]; y.occ_idx = d.occ_idx; y.occ_fl = v.occ_fl;
        y.accT = constrained ? d.accWy : d.accE; y.dSx = d.dSx; y.dAx = d.dAx; y.dylo = (l > 0) ? d.dyl[l - 1] : nullptr;
        y.st = d.st; y.seed = d.seed; y.dSx_stride = d.dSx_stride; y.B = d.B; y.D = d.D[l]; y.IN = d.IN[l]; y.layer0 = (l == 0) ? 1 : 0;
        y.generic = d.generic; y.defer_mask = d.defer_mask; y.lr = d.lr; y.drop_e = d.drop_e; y.dbg = d.dbgclk; y.dbgtile = d.dbgtile; y.n_items = d.n_items;
    }
    m->h_leanV = av; m->h_leanH = ah; m->h_leanDa = aa; m->h_leanDy = ay;      // (host copies: the step's launches pass their hot fields as kernel arguments)
    if (any_layer) {
        if (dalloc(m, &m->d_leanV, (size_t)L) || dalloc(m, &m->d_leanH, (size_t)L) || dalloc(m, &m->d_leanDa, (size_t)L) || dalloc(m, &m->d_leanDy, (size_t)L)) return -1;
        HIPCHK(hipMemcpyAsync(m->d_leanV, av.data(), L * sizeof(LeanV), hipMemcpyHostToDevice, m->stream));
        HIPCHK(hipMemcpyAsync(m->d_leanH, ah.data(), L * sizeof(LeanH), hipMemcpyHostToDevice, m->stream));
        HIPCHK(hipMemcpyAsync(m->d_leanDa, aa.data(), L * sizeof(LeanDa), hipMemcpyHostToDevice, m->stream));
        HIPCHK(hipMemcpyAsync(m->d_leanDy, ay.data(), L * sizeof(LeanDy), hipMemcpyHostToDevice, m->stream));
    }
    if (k.score_fwd == SF_LEAN) {
        LeanS q; memset(&q, 0, sizeof(q));
        q.col_item = d.col_item; q.occ_idx = d.occ_idx + d.B; q.occ_fl = d.occ_fl; q.mp = nullptr; q.dbg = d.dbgclk; q.dbgtile = d.dbgtile; q.R = d.R; q.pub_fl = d.xmode == 0 ? 1 : 0; q.logq = d.logq;
        m->h_leanS = q;
        if (dalloc(m, &m->d_leanS, (size_t)1)) return -1;
    }
    if (k.score_bwd == SB_LEAN) {
        LeanB q; memset(&q, 0, sizeof(q));
        q.accBy = d.accBy; q.occ_fl = d.occ_fl; q.dSy = d.dSy; q.dAy = d.dAy; q.dSBy = d.dSBy; q.dABy = d.dABy; q.dhpart = d.dhpart; q.dbg = d.dbgclk; q.dbgtile = d.dbgtile;
        q.dSy_stride = d.dSy_stride; q.dSBy_stride = d.dSBy_stride; q.defer_mask = d.defer_mask; q.generic = d.generic;
        q.ndh = cdiv(d.Dtop + 1, 64); q.nA = cdiv(d.ldSc, 16) * q.ndh; q.nrb = cdiv(d.B, 16); q.ndb = cdiv(d.Dtop, 64); q.lr = d.lr;
        m->h_leanB = q;
        if (dalloc(m, &m->d_leanB, (size_t)1)) return -1;
        HIPCHK(hipMemcpyAsync(m->d_leanB, &m->h_leanB, sizeof(LeanB), hipMemcpyHostToDevice, m->stream));
    }
    if (k.update == UP_LEAN) {
        // k_update_l: argument block + its table of 16 x 64 dense tiles
        LeanU u; memset(&u, 0, sizeof(u));
        u.mp = nullptr; u.st = d.st; u.Wy = d.Wy; u.E = d.E; u.accWy = d.accWy; u.accE = d.accE; u.velWy = d.velWy; u.velE = d.velE;
        u.By = d.By; u.accBy = d.accBy; u.velBy = d.velBy; u.dAx = d.dAx; u.dAy = d.dAy; u.dABy = d.dABy;
        u.dense_p = d.dense_p; u.dense_acc = d.dense_acc; u.dense_vel = d.dense_vel; u.yin0 = d.yin0; u.meta = d.cur_in + 2 * d.B;
        u.dbg = d.dbgclk; u.dbgtile = d.dbgtile; u.n_items = d.n_items; u.constrained = constrained ? 1 : 0; u.wE = d.Ein; u.wY = d.Dtop;
        u.lr = d.lr; u.mom = d.mom; u.lmbd = d.lmbd;
        m->h_leanU = u;
        const std::vector<DenseTile> tiles = dense_tiles(d, 16, 64);
        m->ntiles16 = (int)tiles.size();
        // behind the tiles, in the same allocation: the ring of owner tables (G4R_OWN_SLOTS x [R][16] ints), so that k_update_l finds
        // its step's table from its arguments at the first load.  k_owner_window fills a window's tables ahead of its steps; with
        // G4R_OWNER_WINDOW=0, or a list too long for that kernel's LDS or too short to pay for a launch of its own, k_loss_rows' pre-scan fills slot 0 inside every step; G4R_OWNER_SCAN=1: no table
        const size_t nslot = cdiv((long long)G4R_OWN_SLOTS * d.R * 16 * sizeof(int), (long long)sizeof(DenseTile));
        if (dalloc(m, &m->d_tiles16, tiles.size() + nslot) || dalloc(m, &m->d_leanU, (size_t)1)) return -1;
        d.own_pos = m->sw.owner_scan_in_update ? nullptr : (int*)(m->d_tiles16 + tiles.size());
        m->h_leanU.own_on = d.own_pos ? 1 : 0;
        // the window launch costs a step what one launch per 16 steps costs (measured as the step with and without it: 0.19 us at R = 64, bench
        // cfg #1; 0.82 us at cfg #2's R = 2304); the pre-scan costs the loss launch in proportion to the workgroups it adds -- nothing measurable
        // at 4 (cfg #1: the window form LOST those 0.19 us per step), 1.5 us at 144 (cfg #2; profiles/owner_window.md, with the lengths between).  So: the window form where the pre-scan would add more than G4R_OWN_WINDOW_MINWG
        // workgroups; G4R_OWNER_WINDOW=1 asks for it at any length the LDS holds
        const bool pays = cdiv(d.R, LOSS_NW) > G4R_OWN_WINDOW_MINWG;
        m->own_window = d.own_pos && d.R <= G4R_OWN_WINDOW_MAXR && (m->sw.owner_window > 0 || (m->sw.owner_window < 0 && pays));
        // The window launch also writes every step's (last + 1, R - first, count) entries by position (DevModel::pos_ent; the ring sits
        // next to the owner ring), where every kernel that publishes or reads them is a lean one and the hash of k_owner_window -- a power of
        // two of slots >= 1.5 R, 16 bytes each -- fits its LDS next to the ids (R <= 5461).  Else, and with G4R_POS_ENTRIES=0, the
        // entries are built inside every step as before (debug key `pos_entries`).
        int hs = 64;
        while (hs < d.R + d.R / 2) hs *= 2;
        const bool all_lean = k.fwd[0] == FWD_LEAN && k.bwd[0] == BWD_LEAN && k.score_fwd == SF_LEAN && k.score_bwd == SB_LEAN;
        m->pos_entries = m->own_window && m->sw.pos_entries && all_lean && d.xmode == 0 && hs <= G4R_POS_ENT_MAXHS;
        if (m->pos_entries) {
            m->pos_hs = hs;
            int4* ring = nullptr;
            if (dalloc(m, &ring, (size_t)G4R_OWN_SLOTS * (size_t)((d.R + 3) & ~3))) return -1;
            d.pos_ent = (int*)ring;
        }
        HIPCHK(hipMemcpyAsync(m->d_tiles16, tiles.data(), tiles.size() * sizeof(DenseTile), hipMemcpyHostToDevice, m->stream));
        HIPCHK(hipStreamSynchronize(m->stream));      // (before `tiles` goes out of scope)
    }
    HIPCHK(hipStreamSynchronize(m->stream));
    return 0;
}

// the environment switches of the kernel choice (KernelSwitches), read once per model
static KernelSwitches read_switches(const g4r_config& cfg) {
    KernelSwitches w;
    w.no_lean = getenv("G4R_NO_LEAN") != nullptr; w.no_mt = getenv("G4R_NO_MT") != nullptr; w.no_bmt = getenv("G4R_NO_BMT") != nullptr;
    w.no_merge = getenv("G4R_NO_MERGE") != nullptr; w.owner_scan_in_update = env_int("G4R_OWNER_SCAN", 0) != 0;
    w.owner_window = env_int("G4R_OWNER_WINDOW", -1); w.pos_entries = env_int("G4R_POS_ENTRIES", 1) != 0;
    w.score_b_split = env_int("G4R_SCORE_B_SPLIT", 1) != 0;
    w.allow_lean_update = env_int("G4R_LEAN_UPDATE", 1) != 0; w.defer = env_int("G4R_DEFER", cfg.defer_updates) != 0;
    w.p2_geo = env_int("G4R_P2_GEO", -1); w.ba_geo = env_int("G4R_BA_GEO", -1);
    w.wide2 = env_int("G4R_WIDE2", -1); w.p1_ks = env_int("G4R_P1_KS", 128); w.bb_ks = env_int("G4R_BB_KS", 0);
    const char* skip = getenv("G4R_SKIP_KN");
    w.skip_kn = skip ? strtoull(skip, nullptr, 0) : 0ull;
    w.trace = getenv("G4R_TRACE") != nullptr;
    return w;
}

int g4r_create(const g4r_config* cfg, g4r_model** out) {
    if (!cfg || !out) return fail("null argument");
    if (cfg->n_layers < 1 || cfg->n_layers > G4R_MAX_LAYERS) return fail("n_layers out of range");
    if (cfg->batch_size < 1 || cfg->n_items < 1) return fail("batch_size / n_items must be positive");
    for (int l = 0; l < cfg->n_layers; ++l)
        if (cfg->layers[l] % 4 != 0 || cfg->layers[l] < 4 || cfg->layers[l] > 1024)
            return fail("layer sizes must be multiples of 4 in [4, 1024]");
    if (cfg->embed_mode == G4R_EMBED_SEPARATE && (cfg->embedding % 4 != 0 || cfg->embedding < 4 || cfg->embedding > 1024))
        return fail("embedding must be a multiple of 4 in [4, 1024]");
    if (cfg->embed_mode != G4R_EMBED_CONSTRAINED && cfg->embed_mode != G4R_EMBED_SEPARATE && cfg->embed_mode != G4R_EMBED_ONEHOT)
        return fail("unsupported embedding mode");
    if (cfg->embed_mode == G4R_EMBED_ONEHOT && 3 * cfg->layers[0] > 1024)
        return fail("one-hot input: 3 * layers[0] must be <= 1024 (row width of the Wx[0] table)");
    if (cfg->loss < 0 || cfg->loss > G4R_LOSS_XE_LOGIT) return fail("unsupported loss");
    if (cfg->smoothing != 0.f && cfg->loss != G4R_LOSS_XE && cfg->loss != G4R_LOSS_XE_LOGIT) return fail("smoothing needs a cross-entropy loss");
    if (cfg->hidden_act == G4R_ACT_SOFTMAX_LOGIT) return fail("softmax_logit is not a hidden activation");
    if (cfg->adapt < 0 || cfg->adapt > G4R_ADAPT_NONE) return fail("unknown adapt");
    if (cfg->grad_cap < 0.f) return fail("grad_cap must be >= 0");
    if (cfg->hidden_act == G4R_ACT_SOFTMAX) return fail("softmax is not a hidden activation");
    int ndev = g4r_device_count();
    if (ndev <= 0) return fail("no HIP device visible: the gfx950 path has no CPU fallback");
    if (cfg->device < 0 || cfg->device >= ndev) return fail("device ordinal out of range");
    HIPCHK(hipSetDevice(cfg->device));
    int n_cu = 0;
    HIPCHK(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, cfg->device));
    g4r_model* m = new g4r_model();
    m->cfg = *cfg;
    m->n_cu = std::max(n_cu, 1);
    if (hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking) != hipSuccess) { delete m; return fail("stream create"); }
    // ---- 1. the shape scalars of the model
    DevModel& d = m->dm;
    memset(&d, 0, sizeof(d));
    const int L = cfg->n_layers, B = cfg->batch_size;
    d.n_items = cfg->n_items; d.n_layers = L; d.B = B;
    // negatives: generate_length = sample_store // n_sample ; a store of <= 1 rows means "no store" (gru4rec.py:546-550), i.e. a
    // fresh row of negatives for every step (:614-615): a one-row store that is refilled before every step
    const int ns = std::max(cfg->n_sample, 0);
    int64_t gl = (ns > 0 && cfg->sample_store > 0) ? cfg->sample_store / ns : 0;
    if (ns > 0 && gl <= 1) gl = 1;
    m->gl = gl;
    d.ns = ns; d.N = B + ns; d.R = 2 * B + ns; d.ldSc = (d.N + 15) & ~15;
    d.gl = (int)std::max<int64_t>(gl, 1);
    d.loss = cfg->loss; d.final_act = cfg->final_act; d.hidden_act = cfg->hidden_act; d.embed_mode = cfg->embed_mode;
    d.fa_p0 = cfg->final_act_p0; d.fa_p1 = cfg->final_act_p1; d.ha_p0 = cfg->hidden_act_p0; d.ha_p1 = cfg->hidden_act_p1;
    d.lr = cfg->learning_rate; d.mom = cfg->momentum; d.lmbd = cfg->lmbd; d.bpreg = cfg->bpreg; d.logq = cfg->logq;
    d.inv_B = 1.0f / (float)B;
    d.smoothing = cfg->smoothing;
    d.adapt = cfg->adapt; d.ap0 = cfg->adapt_p0; d.ap1 = cfg->adapt_p1; d.grad_cap = cfg->grad_cap;
    // exact-replica mode of N > 1: raw per-occurrence gradients (the generic path's producers), exchanged every step
    // (G4R_FORCE_STAGED=1: the N > 1 data path with a one-rank communicator -- what a 1-GPU box can run and time of it)
    const bool exact = cfg->sparse_exact != 0 && (cfg->nranks > 1 || getenv("G4R_FORCE_STAGED") != nullptr);
    if (cfg->sparse_exact != 0 && cfg->grad_cap > 0.f) { g4r_destroy(m); return fail("sparse_exact does not support grad_cap (the norm would be per rank)"); }
    m->exact = exact;
    d.generic = (cfg->adapt != G4R_ADAPT_ADAGRAD || cfg->grad_cap > 0.f || exact) ? 1 : 0;
    d.drop_h = cfg->dropout_p_hidden; d.drop_e = cfg->dropout_p_embed;
    // dropout masks are keyed by (seed, step, row, column) with LOCAL rows: in exact-replica mode the ranks share cfg->seed (ONE stream of
    // negatives: refill_store), so the masks take a rank-specific key -- the nranks x B rows of the joint batch must not repeat one pattern
    d.seed = cfg->seed + ((cfg->sparse_exact != 0 && cfg->nranks > 1) ? 7919ull * (unsigned long long)cfg->rank : 0ull);
    d.Dtop = cfg->layers[L - 1];
    // width of the layer-0 input rows: shared Wy rows, E rows, or (one-hot input) rows of Wx[0] = [cand|r|z] pre-activations
    d.Ein = (cfg->embed_mode == G4R_EMBED_CONSTRAINED) ? d.Dtop : (cfg->embed_mode == G4R_EMBED_ONEHOT ? 3 * cfg->layers[0] : cfg->embedding);
    int off = 0;
    for (int l = 0; l < L; ++l) {
        d.D[l] = cfg->layers[l];
        d.IN[l] = (l == 0) ? (cfg->embed_mode == G4R_EMBED_ONEHOT ? 0 : d.Ein) : cfg->layers[l - 1];
        d.offWx[l] = off; off += d.IN[l] * 3 * d.D[l];
        d.offWh[l] = off; off += d.D[l] * d.D[l];
        d.offWrz[l] = off; off += d.D[l] * 2 * d.D[l];
        d.offBh[l] = off; off += 3 * d.D[l];
    }
    d.dense_count = off;
    // G4R_FORCE_STAGED=1: exercise the multi-rank data path (gradient staging -> RCCL -> k_dense_apply) on one GPU
    d.apply_dense_inplace = (cfg->nranks <= 1 && !getenv("G4R_FORCE_STAGED") && !d.generic) ? 1 : 0;
    d.grad_scale = 1.0f / (float)std::max(cfg->nranks, 1);
    d.xn = exact ? cfg->nranks : 1;      // exact-replica mode: ranks in the exchanged block, and the form of its update list
    d.xmode = exact ? std::min(std::max(cfg->sparse_exact, 1), 3) : 0;
    // ---- 2. the kernels of the training step
    m->sw = read_switches(*cfg);
    if (m->sw.skip_kn)
        fprintf(stderr, "[g4r] G4R_SKIP_KN=0x%llx: launches are left out of every training step -- its results are invalid (a measurement aid)\n", m->sw.skip_kn);
    // Deferred row updates (g4r_step_kernels.cuh: k_defer_scan / k_sparse_flush): the single-GPU Adagrad step without momentum / L2 term, replayed
    // from the step graph.  The step planes become rings of G4R_GRAPH_STEPS slots (one window = one graph replay).  OPT-IN (G4R_DEFER=1;
    // GRU4Rec.defer_updates, bench.py --defer): bit-identical results and a flush launch at 59 % of the HBM peak on the bytes it
    // moves at BASELINE configs[2] -- but the step gets 2-5 % SLOWER, because the update launch it relieves is at its latency floor
    // (cfg3: k_sparse_update 7.5 -> 6.2 us with 90 % of the rows gone) or bound by its dense-gradient tiles (cfg4), and the flush
    // (2.9 / 7.4 us per step) and scan (0.7 / 1.1) come on top (profiles/r05_experiments.md #7).
    m->defer_on = d.apply_dense_inplace && !d.generic && cfg->momentum <= 0.f && cfg->lmbd == 0.f && m->sw.defer;
    m->kern = choose_kernels(d, m->n_cu, m->sw, m->defer_on);
    const StepKernels& k = m->kern;
    d.kch = k.kch; d.ksplit = k.ksplit;
    for (int l = 0; l < L; ++l) d.bbn[l] = (k.wg[l].use & 8) ? k.wg[l].bbn : 0;
    // ---- 3. the memory plan: every buffer of the step, sized for the kernels chosen
    const size_t I = cfg->n_items;
#define DA(p, n) if (dalloc(m, &(p), (n))) { g4r_destroy(m); return -1; }
    DA(d.dense_p, off); DA(d.dense_acc, off); DA(d.dense_vel, off); DA(d.dense_g, off);
    DA(d.Wy, I * d.Dtop); DA(d.accWy, I * d.Dtop); DA(d.By, I); DA(d.accBy, I);
    if (cfg->momentum > 0.f) { DA(d.velWy, I * d.Dtop); DA(d.velBy, I); }
    if (cfg->embed_mode != G4R_EMBED_CONSTRAINED) {     // E table, or Wx[0] as a row table (one-hot input)
        DA(d.E, I * d.Ein); DA(d.accE, I * d.Ein);
        if (cfg->momentum > 0.f) DA(d.velE, I * d.Ein);
    }
    if (d.generic) {
        const bool two = (cfg->adapt == G4R_ADAPT_ADADELTA || cfg->adapt == G4R_ADAPT_ADAM), cnt = (cfg->adapt == G4R_ADAPT_ADAM);
        if (two) { DA(d.acc2Wy, I * d.Dtop); DA(d.acc2By, I); DA(d.dense_acc2, off); if (d.E) DA(d.acc2E, I * d.Ein); }
        if (cnt) { DA(d.cntWy, I * d.Dtop); DA(d.cntBy, I); DA(d.dense_cnt, off); if (d.E) DA(d.cntE, I * d.Ein); }
        DA(d.gsq_part, G4R_NORM_BLOCKS); DA(d.gclip, 1);
        const float one = 1.f;
        if (hipMemcpyAsync(d.gclip, &one, sizeof(float), hipMemcpyHostToDevice, m->stream) != hipSuccess || hipStreamSynchronize(m->stream) != hipSuccess) {
            g4r_destroy(m); return fail("gclip init");
        }
    }
    int maxD = 0;
    for (int l = 0; l < L; ++l) {
        const size_t bd = (size_t)B * d.D[l];
        maxD = std::max(maxD, d.D[l]);
        DA(d.H[l][0], bd); DA(d.H[l][1], bd);
        DA(d.r[l], bd); DA(d.z[l], bd); DA(d.c[l], bd); DA(d.hd[l], bd); DA(d.Hr[l], bd);
        DA(d.dV[l], bd * 3); DA(d.dyl[l], bd); DA(d.Vc[l], bd);
    }
    DA(m->d_tmpH, (size_t)B * maxD);
    {      // narrow layers: the K-slice partial planes of dr' (k_gru_da -> k_gru_dy)
        size_t drp_floats = 0;
        for (int l = 0; l < L; ++l) if (k.fwd[l] == FWD_LEAN) drp_floats = std::max(drp_floats, (size_t)cdiv(d.D[l], 16) * B * d.D[l]);
        if (drp_floats) DA(d.drp, drp_floats);
    }
    DA(d.yin0, (size_t)B * std::max(d.IN[0], 4));
    DA(d.Sc, (size_t)B * d.ldSc);
    {
        // occ_idx | dSx | dSy | dSBy of this rank in ONE block (DevModel::xbase): what the exact-replica mode all-gathers every step.
        // Offsets are multiples of 64 floats (16-byte rows stay aligned); occ_idx is staged with 16-byte loads up to Rpad.
        auto up64 = [](size_t n) { return (n + 63) & ~(size_t)63; };
        const size_t nOcc = up64((size_t)((d.R + 255) & ~255) + 256 + 64);
        d.xoffSx = (int)nOcc;
        d.xoffSy = (int)(nOcc + up64((size_t)B * d.Ein));
        d.xoffSBy = (int)(d.xoffSy + up64((size_t)d.ldSc * d.Dtop));
        // exact-replica mode: the rank's raw dense gradients ride in the same block (ONE collective per step: the all-gather
        // replaces the all-reduce, every rank adds the ranks' gradients up itself, in rank order -- dense_apply_elem)
        d.xoffDg = (int)(d.xoffSBy + up64((size_t)d.ldSc));
        d.xstride = (long long)(d.xoffDg + (exact ? up64((size_t)d.dense_count) : 0));
        float* xb = nullptr;
        DA(xb, (size_t)d.xn * (size_t)d.xstride);
        d.xbase = xb;
        float* own = xb + (size_t)(exact ? cfg->rank : 0) * (size_t)d.xstride;
        d.occ_idx = (int*)own; d.dSx = own + d.xoffSx; d.dSy = own + d.xoffSy; d.dSBy = own + d.xoffSBy;
        if (exact) d.dense_g = own + d.xoffDg;      // (the buffer allocated above stays unused)
    }
    DA(d.dAx, (size_t)B * d.Ein); DA(d.dAy, (size_t)d.ldSc * d.Dtop); DA(d.dABy, d.ldSc);
    if (m->defer_on) {      // (the deferred mode's step planes: rings of G4R_DEFER_SLOTS slots)
        const size_t W = G4R_DEFER_SLOTS;
        d.defer_mask = (int)W - 1;
        d.dRcap = cdiv(d.R, SP_WAVES) * SP_WAVES;
        d.dSx_stride = (long long)(((size_t)B * d.Ein + 63) & ~(size_t)63);
        d.dSy_stride = (long long)(((size_t)d.ldSc * d.Dtop + 63) & ~(size_t)63);
        d.dSBy_stride = (long long)(((size_t)d.ldSc + 63) & ~(size_t)63);
        float *rx = nullptr, *ry = nullptr, *rb = nullptr;
        DA(rx, W * (size_t)d.dSx_stride); DA(ry, W * (size_t)d.dSy_stride); DA(rb, W * (size_t)d.dSBy_stride);
        d.dSx = rx; d.dSy = ry; d.dSBy = rb;
        DA(d.last_use, (size_t)(cfg->embed_mode != G4R_EMBED_CONSTRAINED ? 2 : 1) * I);
        DA(d.dcand, W * (size_t)d.dRcap); DA(d.dlist, W * (size_t)d.dRcap); DA(d.dstat, 2048);
        if (hipMemsetAsync(d.dlist, 0xFF, W * (size_t)d.dRcap * sizeof(int), m->stream) != hipSuccess) { g4r_destroy(m); return fail("dlist init"); }
        for (auto& e : m->ev_df) if (hipEventCreate(&e) != hipSuccess) { g4r_destroy(m); return fail("event create"); }
    }
    DA(d.lossrow, B);
    DA(d.col_item, d.ldSc); DA(d.cur_in, 2 * (size_t)B + 8); DA(d.cur_col, d.ldSc);
    DA(d.occ_fl, (size_t)(cfg->embed_mode != G4R_EMBED_CONSTRAINED ? 2 : 1) * I * 4);
    DA(d.st, 1);
    DA(d.dhpart, (size_t)d.ksplit * B * d.Dtop);      // dh of the scoring backward, one plane per slab
    m->nblk_occ = cdiv(d.R, SP_WAVES);
    m->nblk_occ_g = m->nblk_occ;      // generic optimizer path (one occurrence per wave; exact-replica mode: sized at launch)
    m->smem_sparse = (size_t)(((d.R + 255) & ~255) + 256) * sizeof(int) + (2 + 64) * SP_WAVES * sizeof(int) +
                     (size_t)SP_WAVES * (std::max(d.Dtop, d.Ein) + 4) * sizeof(float);
    if (ns > 0) DA(m->d_ST, (size_t)gl * ns);
    d.ST = m->d_ST;
    // dense-gradient tile tables: 32 x 32 (k_dense_grad, k_update), 64 x 64 (k_dense_grad2)
    auto tile_table = [&](int edge, DenseTile** dst, int* n) {
        const std::vector<DenseTile> tiles = dense_tiles(d, edge, edge);
        *n = (int)tiles.size();
        return dalloc(m, dst, tiles.size()) == 0 && hipMemcpyAsync(*dst, tiles.data(), tiles.size() * sizeof(DenseTile), hipMemcpyHostToDevice, m->stream) == hipSuccess &&
               hipStreamSynchronize(m->stream) == hipSuccess;
    };
    if (!tile_table(32, &m->d_tiles, &m->ntiles) || (k.wide_dense && !tile_table(64, &m->d_tiles64, &m->ntiles64))) { g4r_destroy(m); return fail("tile upload"); }
    {      // wide layers: the K-slice partial planes of phase 1 (k_gru_p1s -> k_gru_gate) and of dy (k_gru_bwd_bw -> its consumer)
        size_t dyp_floats = 0, vp_floats = 0;
        for (int l = 0; l < L; ++l) {
            const WideGeo& G = k.wg[l];
            if (G.use & 1) vp_floats = std::max(vp_floats, (size_t)(G.ny + G.nh) * B * 3 * d.D[l]);
            if (G.use & 8) dyp_floats = std::max(dyp_floats, (size_t)G.bbn * B * d.IN[l]);
        }
        if (dyp_floats) DA(d.dyp, dyp_floats);
        if (vp_floats) DA(d.vp, vp_floats);
    }
#undef DA
    // LDS opt-in
    m->smem_score = ((size_t)(SC_BM + 32) * (SC_KC + 2) + 32) * sizeof(float);
    m->smem_loss = (size_t)((k.loss_long ? 1 : 2) * d.ldSc + 18 * LOSS_NW) * sizeof(float);
    const int big = 156 * 1024;      // leaves room for the few bytes of static LDS some kernels use (__syncthreads_or)
    const void* const lds_kernels[] = {
        (const void*)k_gru_p1_n32, (const void*)k_gru_p1_n64, (const void*)k_gru_p2_w4, (const void*)k_gru_p2_w8d, (const void*)k_score_fwd_k128,
        (const void*)k_score_fwd_k64, (const void*)k_score_fwd_t2, (const void*)k_score_fwd_t3, (const void*)k_score_mt_4s, (const void*)k_score_bmt,
        (const void*)k_score_bwd_n, (const void*)k_gru_bwd_fused, (const void*)k_gru_fwd_fused, (const void*)k_score_bwd_w, (const void*)k_score_bwd2,
        (const void*)k_gru_bwd_a_w4, (const void*)k_gru_bwd_a_w8d, (const void*)k_gru_bwd_b, (const void*)k_dense_grad<32>,
        (const void*)k_score_store, (const void*)k_score_count, (const void*)k_sim_range<false>, (const void*)k_sim_range<true>,
        (const void*)k_mmr_rerank<false>, (const void*)k_mmr_rerank<true>, (const void*)k_ivf_assign, (const void*)k_owner_window,
#define TK_PTR(name, ...) (const void*)name,
#define SCAN_PTR(NCH, E) (const void*)k_scan_bf16<NCH, E>,
#define IVF_PTR(NCH) (const void*)k_ivf_scan<NCH>,
        TK_FORMS(TK_PTR) SCAN_FORMS(SCAN_PTR) IVF_FORMS(IVF_PTR)      // every form of the range kernels: the lists themselves
#undef TK_PTR
#undef SCAN_PTR
#undef IVF_PTR
    };
    auto opt_in = [&](const void* kern) { return hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, big); };
    for (const void* kern : lds_kernels) HIPCHK(opt_in(kern));
    for (auto& row : K_LOSS_ROWS) for (auto kern : row) HIPCHK(opt_in((const void*)kern));
    for (auto& row : K_SPARSE_UPDATE) for (auto kern : row) HIPCHK(opt_in((const void*)kern));
    for (auto kern : K_SPARSE_UPDATE_GENERIC) HIPCHK(opt_in((const void*)kern));
    for (auto& row : K_UPDATE) for (auto kern : row) HIPCHK(opt_in((const void*)kern));
    if (m->smem_loss > (size_t)big) { g4r_destroy(m); return fail("batch_size + n_sample too large for the row-loss kernel (one copy of a score row must fit the 160 KB of LDS)"); }
    if (m->smem_sparse > (size_t)big) { g4r_destroy(m); return fail("2 * batch_size + n_sample too large for the sparse update (the step's list of gathered rows must fit the 160 KB of LDS)"); }
    if (m->exact) {
        const size_t rlist = d.xmode == 3 ? (size_t)d.xn * 2 * B + d.ns : (size_t)d.R * d.xn;      // xlist_len: entries of the exchanged list
        m->smem_exact = (size_t)(((rlist + 255) & ~(size_t)255) + 256) * sizeof(int) + 64 * SP_WAVES * sizeof(int);
        if (m->smem_exact > (size_t)big) {
            g4r_destroy(m);
            return fail("sparse_exact: the exchanged occurrence list (REDUCE form: nranks * 2 * batch_size + n_sample entries; MEAN / SUM: nranks * (2 * batch_size + n_sample)) does not fit the 160 KB of LDS the update stages it in -- use the GPU-local mode (sync_every) at this shape");
        }
    }
    { float* z = nullptr; if (dalloc(m, &z, ZROW_FLOATS)) { g4r_destroy(m); return -1; } d.zrow = z; }
    if (getenv("G4R_CLK")) {
        if (dalloc(m, &d.dbgclk, 64 + 8 * (size_t)d.R) || dalloc(m, &d.dbgtile, 8 * (size_t)(4096 + 4096))) { g4r_destroy(m); return -1; }
    }
    if (build_lean_args(m)) { g4r_destroy(m); return -1; }
    if (dalloc(m, &m->d_dm, 1) || sync_dm(m)) { g4r_destroy(m); return -1; }
    if (m->d_leanU) {
        m->h_leanU.mp = m->d_dm;
        if (hipMemcpyAsync(m->d_leanU, &m->h_leanU, sizeof(LeanU), hipMemcpyHostToDevice, m->stream) != hipSuccess || hipStreamSynchronize(m->stream) != hipSuccess) { g4r_destroy(m); return fail("lean args upload"); }
    }
    if (m->d_leanS) {
        m->h_leanS.mp = m->d_dm;
        if (hipMemcpyAsync(m->d_leanS, &m->h_leanS, sizeof(LeanS), hipMemcpyHostToDevice, m->stream) != hipSuccess || hipStreamSynchronize(m->stream) != hipSuccess) { g4r_destroy(m); return fail("lean args upload"); }
    }
    *out = m;
    return 0;
}

void g4r_destroy(g4r_model* m) {
    if (!m) return;
    (void)hipSetDevice(m->cfg.device);
    if (m->stream) (void)hipStreamSynchronize(m->stream);
    drop_step_graphs(m, true);
    if (m->comm_ready) (void)ncclCommDestroy(m->comm);
    for (void* q : m->p2p_peer) if (q) (void)hipIpcCloseMemHandle(q);
    if (m->p2p_region) (void)hipFree(m->p2p_region);
    for (auto e : m->evs) (void)hipEventDestroy(e);
    for (auto e : m->ev_df) if (e) (void)hipEventDestroy(e);
    for (auto e : m->ev_ow) if (e) (void)hipEventDestroy(e);
    for (g4r_model::Scratch* sc : {&m->sc_ids, &m->sc_blk, &m->sc_cnt, &m->sc_all, &m->sc_send, &m->sc_pack, &m->sc_recv, &m->sc_hall}) {
        if (sc->p) { if (sc->host) (void)hipHostFree(sc->p); else (void)hipFree(sc->p); }
        sc->p = nullptr; sc->cap = 0;
    }
    for (void* p : m->allocs) (void)hipFree(p);
    if (m->stream) (void)hipStreamDestroy(m->stream);
    delete m;
}

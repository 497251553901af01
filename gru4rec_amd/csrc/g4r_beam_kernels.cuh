// Beam-search kernels (gfx950), behind g4r_beam_sessions (not in the reference): the device-side edge between one step's selection
// and the next step's GRU input when the rows of the chain are BEAMS.  Session row r of a chunk owns the beam rows r W + i, i < W.
//   k_beam_expand   after step 0 (in place of k_rollout_align): session row r becomes its W beam rows -- state, input item, path score
//                   and exclusion list
//   k_beam_select   one workgroup per session: the W best of the W x W extensions by path score, the power-of-two rescale, the
//                   back-pointer record of the step
//   k_beam_advance  one wave per new beam row: the parent's state and exclusion list become the row's own, the item its next input
// Path score of the extension (b, j) -- column j of beam b's selection, step score s: 'sum' fl32(cum_b + s); 'product' fl32(cum_b * s),
// a result of magnitude below 2^-126 (NaN is not) replaced by +0.0, so that nothing depends on the denormal mode.  Order: path score
// descending, equal scores by the lower b W + j, NaN last: topk_key over (path score, b W + j).  'product' rescale, after every
// selection: m = the new beam 0's path score; when m is finite and > 0, e = floor(log2 m) (frexp) and every path score of the session
// is multiplied by 2^-e (exact), e added to the session's scale_exp: path probability = path score x 2^scale_exp.
// A host loop reproduces every one of these operations bit for bit (tests/test_gpu_beam_sessions.py).
#pragma once
#include "g4r_rollout_kernels.cuh"

#define BM_MAX G4R_BEAM_MAX      // widest beam: BM_MAX^2 = 1024 extensions per session

// the hidden states a beam kernel moves: per layer, rows of W floats from src (k_beam_expand: src1 holds the rows of odd history
// length) to dst
struct BeamState { const float* src[G4R_MAX_LAYERS]; const float* src1[G4R_MAX_LAYERS]; float* dst[G4R_MAX_LAYERS]; int W[G4R_MAX_LAYERS]; int n_layers; };

// the exponent the rescale removes: floor(log2 m) for a finite m > 0, otherwise 0
__device__ __forceinline__ int beam_exp(float m) {
    if (!(m > 0.f) || m == __builtin_inff()) return 0;
    int x;
    (void)frexpf(m, &x);
    return x - 1;
}

// one wave: dst[0 .. n] <- the sorted list src[0 .. n) with `item` (not in it) inserted at its place; *dlen <- n + 1.  src and dst
// never overlap (the session's list and a beam's, or the two list buffers), so plain loads and stores need no ordering
__device__ __forceinline__ void beam_list_insert(const int* src, int n, int item, int* dst, int* dlen) {
    const int lane = threadIdx.x;
    int a = 0, b = n;
    while (a < b) { const int mid = (a + b) >> 1; if (src[mid] < item) a = mid + 1; else b = mid; }
    for (int j = lane; j < n; j += 64) dst[j + (j >= a ? 1 : 0)] = src[j];
    if (lane == 0) { dst[a] = item; *dlen = n + 1; }
}

// One wave per beam row q = r W + i (grid = rows W, 64 threads).  tcols / tscores: step 0's [rows][W] selection.  The row's path score
// is score i (rescaled by the exponent of score 0 with `product`; scale_exp[r] <- that exponent, or 0), its back-pointer record of
// step 0 (parent i, column, score).  more != 0 (steps > 1): every layer's state of session row r -- in st.src (even history length)
// or st.src1 (odd) -- is copied to row q of st.dst, next_in[q] <- the item of column i, and with xlen != NULL (no_repeat) the row's
// list xitems[beg[q] ..) <- the session's sorted list sitems[soffs[r] .. soffs[r + 1]) plus that item
__global__ __launch_bounds__(64) void k_beam_expand(const int* tcols, const float* tscores, int W, const int* item_idx, BeamState st,
                                                    const int* len, int product, int more, float* cum, int* scale_exp, int* next_in,
                                                    int* bp_parent, int* bp_col, float* bp_score, const long long* soffs,
                                                    const int* sitems, const long long* beg, int* xlen, int* xitems) {
    const int q = blockIdx.x, lane = threadIdx.x, r = q / W, i = q - r * W;
    const int col = tcols[q];
    const float sc = tscores[q];
    const int e = product ? beam_exp(tscores[(size_t)r * W]) : 0;
    if (lane == 0) {
        cum[q] = product ? ldexpf(sc, -e) : sc;
        bp_parent[q] = i; bp_col[q] = col; bp_score[q] = sc;
        if (i == 0) scale_exp[r] = e;
    }
    if (!more) return;
    const int item = item_idx ? item_idx[col] : col;
    if (lane == 0) next_in[q] = item;
    const int odd = len[r] & 1;
    for (int l = 0; l < st.n_layers; ++l) {
        const int D = st.W[l];
        const float* s = (odd ? st.src1[l] : st.src[l]) + (size_t)r * D;
        float* d = st.dst[l] + (size_t)q * D;
        for (int j = lane; j < D; j += 64) d[j] = s[j];
    }
    if (xlen) beam_list_insert(sitems + soffs[r], (int)(soffs[r + 1] - soffs[r]), item, xitems + beg[q], xlen + q);
}

// One workgroup per session r (grid = sessions, 256 threads).  tcols / tscores: this step's [rows W][W] selection of the session's W
// beam rows; cum[r W ..]: their path scores, replaced by the new beams'.  New beam i (rank i of the W^2 extensions): sel_parent /
// sel_item[r W + i] <- the parent beam b and the extension's item; bp_*[r W + i] <- (b, column, step score), this step's record
__global__ __launch_bounds__(256) void k_beam_select(const int* tcols, const float* tscores, int W, const int* item_idx, int product,
                                                     float* cum, int* scale_exp, int* sel_parent, int* sel_item, int* bp_parent,
                                                     int* bp_col, float* bp_score) {
    __shared__ unsigned long long sk[BM_MAX * BM_MAX];
    __shared__ float sp[BM_MAX * BM_MAX];
    __shared__ float s_cum[BM_MAX];
    __shared__ int s_win[BM_MAX];
    const int r = blockIdx.x, tid = threadIdx.x, n = W * W;
    const size_t base = (size_t)r * n;
    if (tid < W) s_cum[tid] = cum[(size_t)r * W + tid];
    __syncthreads();
    for (int c = tid; c < n; c += 256) {
        const float s = tscores[base + c], a = s_cum[c / W];
        float p = product ? __fmul_rn(a, s) : __fadd_rn(a, s);      // (never contracted with anything around it)
        if (product && fabsf(p) < 0x1p-126f) p = 0.f;
        sp[c] = p;
        sk[c] = topk_key(p, (unsigned)c);
    }
    __syncthreads();
    // the keys are distinct (c is), so the number of larger keys is the extension's rank
    for (int c = tid; c < n; c += 256) {
        const unsigned long long mine = sk[c];
        int rank = 0;
        for (int o = 0; o < n; ++o) rank += sk[o] > mine ? 1 : 0;
        if (rank < W) s_win[rank] = c;
    }
    __syncthreads();
    if (tid < W) {
        const int c = s_win[tid], b = c / W, col = tcols[base + c];
        const size_t q = (size_t)r * W + tid;
        const int e = product ? beam_exp(sp[s_win[0]]) : 0;
        cum[q] = product ? ldexpf(sp[c], -e) : sp[c];
        if (tid == 0 && e != 0) scale_exp[r] += e;
        sel_parent[q] = b;
        sel_item[q] = item_idx ? item_idx[col] : col;
        bp_parent[q] = b; bp_col[q] = col; bp_score[q] = tscores[base + c];
    }
}

// One wave per new beam row q = r W + i (grid = rows W, 64 threads): every layer's state of the parent row r W + sel_parent[q] in
// st.src -> row q of st.dst (the OTHER ping-pong half: the gather cannot be in place), next_in[q] <- sel_item[q], and with
// len_dst != NULL (no_repeat) the parent's sorted list in the current list buffer, plus the item -> the row's list in the other one
// (both buffers lay beam row q's list at beg[q], the beams of one session having equal room)
__global__ __launch_bounds__(64) void k_beam_advance(const int* sel_parent, const int* sel_item, int W, BeamState st, int* next_in,
                                                     const long long* beg, const int* len_src, const int* items_src, int* len_dst,
                                                     int* items_dst) {
    const int q = blockIdx.x, lane = threadIdx.x, r = q / W;
    const int p = r * W + sel_parent[q], item = sel_item[q];
#if defined(G4R_MUTATE) && G4R_MUTATE == 15      // test build: the state of row i itself instead of row parent[i]
    const int ps = q;
#else
    const int ps = p;
#endif
    for (int l = 0; l < st.n_layers; ++l) {
        const int D = st.W[l];
        const float* s = st.src[l] + (size_t)ps * D;
        float* d = st.dst[l] + (size_t)q * D;
        for (int j = lane; j < D; j += 64) d[j] = s[j];
    }
    if (lane == 0) next_in[q] = item;
    if (len_dst) beam_list_insert(items_src + beg[p], len_src[p], item, items_dst + beg[q], len_dst + q);
}

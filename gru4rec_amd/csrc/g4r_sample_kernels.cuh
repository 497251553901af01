// Sampling kernels (gfx950), behind g4r_sample_sessions (not in the reference): stochastic decoding of session continuations from the
// model's own next-item distribution by the Gumbel-max trick -- the argmax of key = fl32(fl32(z * invT) + g) over the eligible
// candidate positions is a draw from softmax(z / T) over them, so a draw is a SELECTION and nothing materialises a score row, a softmax
// or a prefix sum.  Session row r of a chunk owns the draw rows r S + j, j < S = samples.
//   k_topk_sample    k_topk_range<false, true, TkSample> (g4r_topk_kernels.cuh): the fused score-and-select kernel selecting on the key
//   k_sample_expand  after the replay: session row r's state (every layer) and top-layer output become those of its S draw rows
//   k_sample_pick    one wave per draw row, behind k_topk_merge.  top_k = t: the argmax of the key over the row's t best (column, z);
//                    untruncated: the merge's one (column, key) entry.  Leaves the row's chosen column and item
//   k_debug_gumbel   gumbel_noise for a list of items (tests compare it with a float64 twin)
// Log-probabilities and the nucleus (g4r_sample_sessions_lp, g4r_session_log_partition) rest on the row normaliser Q, an exact 64-bit
// integer formed inside the scan (TkLse, g4r_topk_kernels.cuh):
//   k_topk_sample_q  k_topk_range<false, true, TkSampleLse>: k_topk_sample + Q;  k_topk_fused_q  <false, true, TkGrowLse>: the exact
//                    selection with growing lists + Q
//   k_sample_pick_lp k_sample_pick for top_k = t with the nucleus cut m (wave scan of the t terms against top_p Q) and the draw's
//                    log-probability;  k_sample_logprob  the untruncated draw's, from Q, zeta and the chosen z
//   k_debug_lse_terms  lse_term for a list of (z, zeta) (tests compare it with a float64 twin)
// The per-step tail is k_rollout_feed with k = 1 (g4r_rollout_kernels.cuh) on (chosen column, its z): z is the merge's own in the top_k
// path and is recomputed for the one chosen column per row by k_score_cand in the untruncated one (g4r_predict_step's bit pattern).
#pragma once
#include "g4r_beam_kernels.cuh"
#include "g4r_cand_kernels.cuh"

// (The three forms of the range kernel are instantiated with the others, from TK_FORMS.  The sampling form's LDS is the EXCL fused
// kernel's: the row ids live in registers, 8 per lane.)

// One wave per draw row q = r S + j (grid = rows S, 64 threads): every layer's state of session row r -- in st.src (even history length)
// or st.src1 (odd) -- is copied to row q of st.dst, the row's top-layer output hsrc[r] to hdst[q] (Dtop floats each)
__global__ __launch_bounds__(64) void k_sample_expand(BeamState st, const int* len, int S, const float* hsrc, float* hdst, int Dtop) {
    const int q = blockIdx.x, lane = threadIdx.x, r = q / S;
    const int odd = len[r] & 1;
    for (int l = 0; l < st.n_layers; ++l) {
        const int D = st.W[l];
        const float* s = (odd ? st.src1[l] : st.src[l]) + (size_t)r * D;
        float* d = st.dst[l] + (size_t)q * D;
        for (int j = lane; j < D; j += 64) d[j] = s[j];
    }
    for (int j = lane; j < Dtop; j += 64) hdst[(size_t)q * Dtop + j] = hsrc[(size_t)r * Dtop + j];
}

// One wave per draw row (grid = rows, 64 threads).  tcols / tvals: the merge's [rows][t] result.  keyed != 0 (top_k = t): tvals are
// the scores z of the row's t best eligible columns; the row's choice is the entry with the largest topk_key(key, column) -- equal
// keys to the lower column, NaN last --, key = fl32(fl32(z * invT) + gumbel_noise(seed, row_id[row], step, item)); pick_z[row] <- its z.
// keyed == 0 (t = 1): the entry is the choice already (the range kernel selected on the key); pick_z is left to k_score_cand.
// pick_col / pick_item[row] <- the chosen column and its item index (item_idx[column], or the column)
__global__ __launch_bounds__(64) void k_sample_pick(const int* tcols, const float* tvals, int t, int keyed, const int* item_idx,
                                                    const unsigned* row_id, unsigned long long seed, unsigned step, float invT,
                                                    int* pick_col, int* pick_item, float* pick_z) {
    const int row = blockIdx.x, lane = threadIdx.x;
    const size_t o = (size_t)row * t;
    int bj = 0;
    if (keyed) {
        const unsigned q = row_id[row];
        unsigned long long best = 0ull;
        for (int j = lane; j < t; j += 64) {
            const int col = tcols[o + j];
            if (col < 0) continue;      // (a pad: never there, every row keeps t eligible positions)
            const int item = item_idx ? item_idx[col] : col;
            const float key = __fadd_rn(__fmul_rn(tvals[o + j], invT), gumbel_noise(seed, q, step, item));
            const unsigned long long kk = topk_key(key, (unsigned)col);
            if (kk > best) { best = kk; bj = j; }
        }
#pragma unroll
        for (int w = 32; w > 0; w >>= 1) {
            const unsigned lo = __shfl_xor((unsigned)best, w), hi = __shfl_xor((unsigned)(best >> 32), w);
            const int oj = __shfl_xor(bj, w);
            const unsigned long long ob = ((unsigned long long)hi << 32) | lo;
            if (ob > best) { best = ob; bj = oj; }      // (keys of distinct columns are distinct: every lane ends with the same pair)
        }
    }
    if (lane == 0) {
        const int col = tcols[o + bj];
        pick_col[row] = col;
        pick_item[row] = item_idx ? item_idx[col] : col;
        if (keyed) pick_z[row] = tvals[o + bj];
    }
}

// k_sample_pick's sibling for the top_k = t path of g4r_sample_sessions_lp (one wave per draw row): the same choice, made among the first m
// of the row's t best, and its log-probability.  With zeta = the list's first z, q_j = lse_term(z_j, zeta, invT) and C_j their integer
// prefix sums (a wave scan, 64 entries at a time), m is the smallest j with (double)C_j >= (double)top_p * (double)Q[row] (none: m = t;
// top_p == 0, no nucleus: m = t and Q is not read) and lp[row][s] = fl32((double)d_c - log((double)C_m * 2^-39)), d_c the chosen entry's
// fl32(fl32(z_c - zeta) * invT).  Q: the row's normaliser over its WHOLE eligible set (k_topk_range<.., TkGrowLse>).
__global__ __launch_bounds__(64) void k_sample_pick_lp(const int* tcols, const float* tvals, int t, const int* item_idx, const unsigned* row_id,
                                                       unsigned long long seed, unsigned step, float invT, float top_p,
                                                       const unsigned long long* Q, int* pick_col, int* pick_item, float* pick_z, float* lp,
                                                       int steps, int s) {
    const int row = blockIdx.x, lane = threadIdx.x;
    const size_t o = (size_t)row * t;
    const float zeta = tvals[o];
    const double need = top_p > 0.f ? __dmul_rn((double)top_p, (double)Q[row]) : 0.0;
    unsigned long long carry = 0ull, den = 0ull;
    int m = t;
    bool found = false;      // (the same in every lane)
    for (int j0 = 0; j0 < t && !found; j0 += 64) {
        const int j = j0 + lane;
        unsigned long long c = (j < t && tcols[o + j] >= 0) ? lse_term(tvals[o + j], zeta, invT) : 0ull;
#pragma unroll
        for (int w = 1; w < 64; w <<= 1) {
            const unsigned lo = __shfl_up((unsigned)c, w), hi = __shfl_up((unsigned)(c >> 32), w);
            if (lane >= w) c += ((unsigned long long)hi << 32) | lo;
        }
        c += carry;
        if (top_p > 0.f) {
            const unsigned long long hit = __ballot(j < t && (double)c >= need);
            if (hit) {
                const int f = __ffsll(hit) - 1;
                m = j0 + f + 1;
                den = ((unsigned long long)__shfl((unsigned)(c >> 32), f) << 32) | __shfl((unsigned)c, f);
                found = true;
            }
        }
        carry = ((unsigned long long)__shfl((unsigned)(c >> 32), 63) << 32) | __shfl((unsigned)c, 63);
    }
    if (!found) den = carry;      // C_t
    const unsigned q = row_id[row];
    unsigned long long best = 0ull;
    int bj = 0;
    for (int j = lane; j < m; j += 64) {
        const int col = tcols[o + j];
        if (col < 0) continue;      // (a pad: never there, every row keeps t eligible positions)
        const int item = item_idx ? item_idx[col] : col;
        const float key = __fadd_rn(__fmul_rn(tvals[o + j], invT), gumbel_noise(seed, q, step, item));
        const unsigned long long kk = topk_key(key, (unsigned)col);
        if (kk > best) { best = kk; bj = j; }
    }
#pragma unroll
    for (int w = 32; w > 0; w >>= 1) {
        const unsigned lo = __shfl_xor((unsigned)best, w), hi = __shfl_xor((unsigned)(best >> 32), w);
        const int oj = __shfl_xor(bj, w);
        const unsigned long long ob = ((unsigned long long)hi << 32) | lo;
        if (ob > best) { best = ob; bj = oj; }
    }
    if (lane == 0) {
        const int col = tcols[o + bj];
        const float zc = tvals[o + bj];
        pick_col[row] = col;
        pick_item[row] = item_idx ? item_idx[col] : col;
        pick_z[row] = zc;
        const float d = __fmul_rn(__fsub_rn(zc, zeta), invT);
        lp[(size_t)row * steps + s] = (float)((double)d - log((double)den * 0x1p-39));
    }
}

// The untruncated path's log-probability, behind k_score_cand (one thread per draw row): lp[row][s] = fl32((double)d_c - log((double)Q[row]
// * 2^-39)), d_c = fl32(fl32(z[row] - zeta[row]) * invT), z the chosen position's logit
__global__ __launch_bounds__(256) void k_sample_logprob(const float* z, const float* zeta, const unsigned long long* Q, float invT, int rows,
                                                        int steps, int s, float* lp) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= rows) return;
    lp[(size_t)row * steps + s] = lse_logprob(z[row], zeta[row], Q[row], invT);
}

// out[p] = lse_term(z[p], zeta[p], invT): the function the scan calls
__global__ __launch_bounds__(256) void k_debug_lse_terms(const float* z, const float* zeta, float invT, long long n, unsigned long long* out) {
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p < n) out[p] = lse_term(z[p], zeta[p], invT);
}

// out[p] = gumbel_noise(seed, q, step, items[p]): the function the selection calls
__global__ __launch_bounds__(256) void k_debug_gumbel(unsigned long long seed, unsigned q, unsigned step, const int* items, long long n,
                                                      float* out) {
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p < n) out[p] = gumbel_noise(seed, q, step, items[p]);
}

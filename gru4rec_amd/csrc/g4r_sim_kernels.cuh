// Item-to-item neighbours (gfx950), behind g4r_similar_items (not in the reference).
//   k_item_norms  inv[i] = 1 / sqrt(sum_d T[i, d]^2) of every row of an item table (0 for a zero row): one streaming pass
//   k_sim_gather  the chunk's query rows copied into one contiguous block
//   k_sim_range   k_topk_range's sibling whose BOTH operands are rows of the item table: tiles of Q x T[cols]^T (Q = the chunk's
//                 query rows, gathered), no bias, no activation; cosine multiplies by the two inverse norms in the epilogue.  The
//                 range's k best per row leave through the queues / thresholds / topk_merge_row of g4r_topk_kernels.cuh, and
//                 k_topk_merge finishes the rows as it does for g4r_recommend_step.
// Score of a pair (the contract of include/gru4rec_hip.h): one ascending-k fp32 MFMA chain from zero over the two rows, then
// (dot * inv[query]) * inv[candidate item] for cosine.  Nothing else enters it -- not the column, the row, the range or the chunk --
// so a pair's score bits are the same wherever the pair appears.
#pragma once
#include "g4r_topk_kernels.cuh"

#define SIM_ROWS_PER_GROUP 4      // k_item_norms: rows per 16-lane group (their loads go out together)

// grid: ceil(n / 64) workgroups of 256 threads; a 16-lane group sums the squares of SIM_ROWS_PER_GROUP consecutive rows (lane l adds
// the float4s l, l + 16, ... of the row in that order, then the 16 partial sums meet in a fixed xor tree: the order depends on W alone)
__global__ __launch_bounds__(256) void k_item_norms(const float* __restrict__ T, long long n, int W, float* __restrict__ inv) {
    const int li = threadIdx.x & 15, w4 = W >> 2;
    const long long r0 = ((long long)blockIdx.x * 16 + (threadIdx.x >> 4)) * SIM_ROWS_PER_GROUP;
    float s[SIM_ROWS_PER_GROUP];
#pragma unroll
    for (int j = 0; j < SIM_ROWS_PER_GROUP; ++j) {
        s[j] = 0.f;
        const long long r = min(r0 + j, n - 1);      // (rows past the table: the last row again, not stored)
        for (int c = li; c < w4; c += 16) {
            const float4 x = ld4(T + (size_t)r * W + 4 * c);
            s[j] = fmaf(x.x, x.x, s[j]); s[j] = fmaf(x.y, x.y, s[j]); s[j] = fmaf(x.z, x.z, s[j]); s[j] = fmaf(x.w, x.w, s[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < SIM_ROWS_PER_GROUP; ++j) {
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) s[j] += __shfl_xor(s[j], o);
        if (li == 0 && r0 + j < n) inv[r0 + j] = s[j] > 0.f ? 1.0f / sqrtf(s[j]) : 0.f;
    }
}

// Q[r] = T[q_idx[r]]: the chunk's query rows, gathered once into one contiguous block (bit copies).  The scan reloads its A tile for
// every tile of columns when a row is wider than SC_KC floats; rows scattered over a table of gigabytes are then as many pages to
// translate every time, one block is a few
__global__ __launch_bounds__(256) void k_sim_gather(const float* __restrict__ T, int W, const int* __restrict__ q_idx, int mrows, float* __restrict__ Q) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    const int w4 = W >> 2;
    if (e >= (long long)mrows * w4) return;
    const int r = (int)(e / w4), c = (int)(e - (long long)r * w4);
    st4(Q + (size_t)r * W + 4 * c, ld4(T + (size_t)q_idx[r] * W + 4 * c));
}

// LDS: k_topk_fused's [queues | counts | lengths | thresholds | A tile | B tile | column items] + the rows' query items.  The merge
// scratch aliases the B tile (rewritten for every tile of columns), so that a table of at most SC_KC floats per row keeps its A
// tile -- the workgroup's 128 query rows -- for the whole range.
#define SIM_SMEM (tk_smem<false, false>() + SC_BM * 4)
static_assert(4 * TK_SCRATCH_WAVE <= TK_TN * (SC_KC + 2) * 4, "the merge scratch must fit in the B tile");
static_assert(SIM_SMEM <= 156 * 1024, "k_sim_range LDS over the 156 KiB the kernels may ask for");

// One chunk of query rows.  The grid is one-dimensional: workgroup -> tile (G4R_XCD_TILE) -> (column range, 128-row block) with the
// row blocks of a range NEXT to each other, so that the workgroups that scan the same rows of T sit on one XCD and run together: a
// range of T comes from HBM about once per chunk, the other row blocks find it in that XCD's L2.
//   T / W        the item table and its row width (floats, a multiple of 4)
//   q_idx, Q     the chunk's query items [mrows] and their rows [mrows][W] (k_sim_gather)
//   item_idx     the candidates [n_sel], NULL: every item (n_sel = n_items)
//   inv          COS: the table's inverse norms, by ITEM index
//   xmask        item bit mask of excluded items, NULL: none; self: a column holding the row's own query item is skipped
// Excluded, self and out-of-range columns never reach a queue, so the lists hold eligible entries and pads only.
template <bool COS>
__global__ __launch_bounds__(256) void k_sim_range(const float* __restrict__ T, int W, int n_items, const int* __restrict__ q_idx,
                                                   const float* __restrict__ Q, int mrows,
                                                   const int* __restrict__ item_idx, long long n_sel, const float* __restrict__ inv,
                                                   const unsigned* __restrict__ xmask, int self, int k, int tpr, int R, int RB, uint2* ws) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, li = lane & 15, lg = lane >> 4;
    uint2* s_q = reinterpret_cast<uint2*>(smem);
    int* s_qn = reinterpret_cast<int*>(s_q + SC_BM * TK_Q);
    int* s_ln = s_qn + SC_BM;
    unsigned long long* s_thr = reinterpret_cast<unsigned long long*>(s_ln + SC_BM);
    float* sA = reinterpret_cast<float*>(s_thr + SC_BM);
    const int ldk = SC_KC + 2;
    float* sB = sA + SC_BM * ldk;
    int* sItem = reinterpret_cast<int*>(sB + TK_TN * ldk);
    int* sQi = sItem + TK_TN;
    char* scratch = reinterpret_cast<char*>(sB) + wid * TK_SCRATCH_WAVE;
    uint2* sl = reinterpret_cast<uint2*>(scratch);
    unsigned long long* skq = reinterpret_cast<unsigned long long*>(scratch + TK_MAX * 8);

    const int tile = G4R_XCD_TILE(blockIdx.x, gridDim.x);
    const int range = tile / RB, rbase = (tile - range * RB) * SC_BM;
    const long long c0 = (long long)range * tpr * TK_TN, c1 = min(n_sel, c0 + (long long)tpr * TK_TN);
    if (tid < SC_BM) {
        s_qn[tid] = 0; s_ln[tid] = 0; s_thr[tid] = 0ull;
        sQi[tid] = rbase + tid < mrows ? q_idx[rbase + tid] : -1;
    }
    __syncthreads();
    auto list = [&](int r) { return ws + ((size_t)(rbase + r) * R + range) * k; };
    auto merge_all = [&]() {
        for (int r = wid; r < SC_BM; r += 4)
            if (s_qn[r] > 0) topk_merge_row<false>(r, list(r), k, s_q + r * TK_Q, skq, sl, s_qn, s_ln, s_thr);
        __syncthreads();
    };
    // this lane's 8 rows (the MFMA accumulator layout): their query items and, for cosine, inverse norms
    int qi[2][4];
    float iq[2][4];
#pragma unroll
    for (int ri = 0; ri < 2; ++ri)
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) {
            qi[ri][rg] = sQi[32 * wid + 16 * ri + 4 * lg + rg];
            iq[ri][rg] = (COS && qi[ri][rg] >= 0) ? inv[qi[ri][rg]] : 0.f;
        }
    const bool a_once = W <= SC_KC;      // one k-chunk: the A tile is loaded for the first tile of columns and kept
    for (long long n0 = c0; n0 < c1; n0 += TK_TN) {
        if (tid < TK_TN) {
            const long long n = n0 + tid;
            const int item = n < c1 ? (item_idx ? item_idx[n] : (int)n) : -1;
            sItem[tid] = item;
        }
        // this lane's two columns: item, inverse norm and mask word go out now and are first used in the epilogue, behind the tile's
        // loads and MFMA chain (staged through LDS in front of the barrier they cost every tile one more memory round trip)
        int it[2];
        unsigned xw[2];
        float ic[2];
#pragma unroll
        for (int cj = 0; cj < 2; ++cj) {
            const long long n = n0 + 16 * cj + li;
            it[cj] = n < c1 ? (item_idx ? item_idx[n] : (int)n) : -1;
            const int ia = max(it[cj], 0);
            xw[cj] = xmask ? xmask[ia >> 5] : 0u;
#if defined(G4R_MUTATE) && G4R_MUTATE == 13      // test build: the candidate's inverse norm read at its POSITION, not at its item index
            ic[cj] = COS ? inv[min(n, (long long)n_items - 1)] : 0.f;
#else
            ic[cj] = COS ? inv[ia] : 0.f;
#endif
        }
        __syncthreads();
        f32x4 acc[2][2];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int kc0 = 0; kc0 < W; kc0 += SC_KC) {
            const int kc = min(SC_KC, W - kc0), kc4 = kc >> 2;
            if (!a_once || n0 == c0)
                for (int e = tid; e < SC_BM * kc4; e += 256) {
                    const int i = e / kc4, c4 = e - i * kc4, q = sQi[i];
                    float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (q >= 0) x = ld4(Q + (size_t)(rbase + i) * W + kc0 + 4 * c4);
                    float2* d = reinterpret_cast<float2*>(sA + i * ldk + 4 * c4);
                    d[0] = make_float2(x.x, x.y);
                    d[1] = make_float2(x.z, x.w);
                }
            for (int e = tid; e < TK_TN * kc4; e += 256) {
                const int j = e / kc4, c4 = e - j * kc4, item = sItem[j];
                float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
                if (item >= 0) x = ld4(T + (size_t)item * W + kc0 + 4 * c4);
                float2* d = reinterpret_cast<float2*>(sB + j * ldk + 4 * c4);
                d[0] = make_float2(x.x, x.y);
                d[1] = make_float2(x.z, x.w);
            }
            __syncthreads();
            for (int kk = 0; kk < kc; kk += 4) {
                const float a0 = sA[(32 * wid + li) * ldk + kk + lg];
                const float a1 = sA[(32 * wid + 16 + li) * ldk + kk + lg];
#pragma unroll
                for (int cj = 0; cj < 2; ++cj) {
                    const float b = sB[(16 * cj + li) * ldk + kk + lg];
                    acc[0][cj] = mfma16(a0, b, acc[0][cj]);
                    acc[1][cj] = mfma16(a1, b, acc[1][cj]);
                }
            }
            __syncthreads();
        }
        bool dr[2];
#pragma unroll
        for (int cj = 0; cj < 2; ++cj) dr[cj] = it[cj] >= 0 && ((xw[cj] >> (it[cj] & 31)) & 1u);
#pragma unroll
        for (int ri = 0; ri < 2; ++ri)
#pragma unroll
            for (int rg = 0; rg < 4; ++rg) {
                const int r = 32 * wid + 16 * ri + 4 * lg + rg;
                const unsigned long long t = s_thr[r];
#pragma unroll
                for (int cj = 0; cj < 2; ++cj) {
                    const long long n = n0 + 16 * cj + li;
                    float v = acc[ri][cj][rg];
                    if constexpr (COS) v = (v * iq[ri][rg]) * ic[cj];
                    const bool ok = qi[ri][rg] >= 0 && it[cj] >= 0 && !dr[cj] && !(self && it[cj] == qi[ri][rg]);
                    const unsigned long long key = topk_key(v, (unsigned)n);
                    if (ok && key > t) {
                        const int p = atomicAdd(s_qn + r, 1);
                        s_q[r * TK_Q + p] = make_uint2(__float_as_uint(v), (unsigned)n);
                    }
                }
            }
        __syncthreads();
        if (__syncthreads_or(tid < SC_BM && s_qn[tid] > TK_Q - TK_TN)) merge_all();
    }
    merge_all();
    for (int r = wid; r < SC_BM; r += 4)
        if (rbase + r < mrows) {
            uint2* L = list(r);
            for (int j = s_ln[r] + lane; j < k; j += 64) L[j] = make_uint2(0u, 0xFFFFFFFFu);
        }
}

template __global__ void k_sim_range<false>(const float*, int, int, const int*, const float*, int, const int*, long long, const float*, const unsigned*, int, int, int, int, int, uint2*);
template __global__ void k_sim_range<true>(const float*, int, int, const int*, const float*, int, const int*, long long, const float*, const unsigned*, int, int, int, int, int, uint2*);

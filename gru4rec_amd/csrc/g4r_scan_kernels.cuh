// Two-stage top-k kernels (gfx950), behind g4r_recommend_step_scan / g4r_recommend_sessions_scan (not in the reference).
//   k_wy_bf16     Wy (fp32) -> the bf16 shadow table, stored in MFMA fragment order
//   k_scan_bf16   bf16 scores of a column range -> the range's c best per row (the bf16 twin of k_topk_fused / k_topk_fused_x)
//   k_scan_merge  the ranges' lists of one row -> the row's c candidates: column, item index (the fixed-stride CSR k_score_cand
//                 reads: row r's list starts at r * c), approximate score, and the number of real candidates
//   k_scan_pack   exact scores of the candidates (k_score_cand) -> (score bits, COLUMN) lists for the unchanged k_topk_merge
// Contract.  The approximate score of (row, column) is: h and the item's Wy row rounded to bf16 (round to nearest even), the
// products summed in fp32 (MFMA order), + By[item] in fp32, then the element-wise final activation in fp32.  A row's candidates
// are the c best approximate scores among its eligible columns in topk_key order; exclusions apply here, exactly as the EXCL
// range kernels apply them, so an excluded item never reaches the second stage.  Every candidate is then scored by k_score_cand
// (bit-identical to g4r_predict_step) and k_topk_merge returns the k best by topk_key(exact score, column).  The lists handed to
// k_topk_merge carry the candidates' COLUMNS, not their list positions, so equal exact scores fall to the lower column whatever
// order stage 1 left the candidates in, and its output needs no map back.
//
// Shadow table: items in blocks of 32, the top layer padded to Dp = 64 * NCH columns (zeros), KS = Dp / 16 k-steps.  The 16-byte
// unit ((block * KS + ks) * 2 + half) * 32 + r holds Wy[32 * block + r][16 * ks + 8 * half .. + 8) as bf16: one wave load of
// consecutive units IS the A operand of v_mfma_f32_32x32x16_bf16 for 32 consecutive items (lane l: row l & 31, k = 8 (l >> 5) + j).
#pragma once
#include "g4r_cand_kernels.cuh"

#define SCN_CMAX G4R_SCAN_CAND_MAX      // longest candidate list per row
#define SCN_TN 64                       // columns per wave tile: two 32-item MFMA fragments
#define SCN_SCRATCH_WAVE (SCN_CMAX * 8 + TK_Q * 8 + G4R_EXCLUDE_MAX * 4)      // bytes: list copy, sorted queue keys, exclusion list
#define SCN_SMEM (SC_BM * TK_Q * 8 + SC_BM * (4 + 4 + 8 + 8 + 4) + 4 * 64 * 4 + 4 * SCN_SCRATCH_WAVE)
static_assert(SCN_SMEM <= 156 * 1024, "scan LDS over the 156 KiB a kernel may ask for");

typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ unsigned short bf16_rne(float x) {
    const unsigned u = __float_as_uint(x);
    if (x != x) return (unsigned short)((u >> 16) | 0x40u);
    return (unsigned short)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}

// one thread per 16-byte unit of the table; nblk blocks of 32 items, KS k-steps
__global__ __launch_bounds__(256) void k_wy_bf16(const DevModel* __restrict__ mp, uint4* tab, long long nblk, int KS) {
    const DevModel& m = *mp;
    const long long u = (long long)blockIdx.x * 256 + threadIdx.x;
    if (u >= nblk * KS * 64) return;
    const int r = (int)(u & 31), half = (int)((u >> 5) & 1);
    const long long bk = u >> 6, blk = bk / KS;
    const int ks = (int)(bk - blk * KS), D = m.Dtop, k0 = 16 * ks + 8 * half;
    const long long item = blk * 32 + r;
    unsigned short v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (item < m.n_items && k0 + j < D) ? bf16_rne(m.Wy[(size_t)item * D + k0 + j]) : (unsigned short)0;
    tab[u] = make_uint4(v[0] | ((unsigned)v[1] << 16), v[2] | ((unsigned)v[3] << 16), v[4] | ((unsigned)v[5] << 16), v[6] | ((unsigned)v[7] << 16));
}

// the float whose topk_key has the high word s (key 0 -> NaN: nothing is "below" an unset threshold)
__device__ __forceinline__ float scan_thr_float(unsigned long long key) {
    const unsigned s = (unsigned)(key >> 32);
    return __uint_as_float((s & 0x80000000u) ? (s ^ 0x80000000u) : ~s);
}

// Stage 1.  Workgroup (blockIdx.x, blockIdx.y) = column range x 128-row block, as k_topk_range; the range is `tpr` tiles of 64
// columns.  Wave w owns rows 32 w .. 32 w + 31 of the block for the whole range and never meets the other waves: its h rows sit
// in registers as the B operand (bf16, converted once), the Wy fragments stream from the shadow table into a two-deep register
// ring of 64-column k-chunks, and its rows' survivor queues, thresholds and merges (topk_merge_row, lists of length c) are its own.
// A score is looked at closely only when it is not below its row's threshold score (one float compare per score).
// Output: ws[(row * gridDim.x + range) * c + j], as k_topk_range with k = c.
// E: TkExcl, or TkGrow (g4r_continue_sessions: per-row lists that grow on the device between launches).
template <int NCH, typename E = TkExcl>
__global__ __launch_bounds__(256) void k_scan_bf16(const DevModel* __restrict__ mp, const float* h, int mrows, const int* item_idx,
                                                   long long n_sel, const uint4* tab, int c, int tpr, uint2* ws, E xarg) {
    using F = TkForm<E>;
    const TkExcl ex = F::excl(xarg);
    constexpr int KS = 4 * NCH;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const DevModel& m = *mp;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, r32 = lane & 31, half = lane >> 5;
    uint2* s_q = reinterpret_cast<uint2*>(smem);
    int* s_qn = reinterpret_cast<int*>(s_q + SC_BM * TK_Q);
    int* s_ln = s_qn + SC_BM;
    unsigned long long* s_thr = reinterpret_cast<unsigned long long*>(s_ln + SC_BM);
    long long* s_xb = reinterpret_cast<long long*>(s_thr + SC_BM);
    int* s_xn = reinterpret_cast<int*>(s_xb + SC_BM);
    float* s_by = reinterpret_cast<float*>(s_xn + SC_BM) + wid * 64;
    char* scratch = reinterpret_cast<char*>(reinterpret_cast<float*>(s_xn + SC_BM) + 4 * 64) + wid * SCN_SCRATCH_WAVE;
    uint2* sl = reinterpret_cast<uint2*>(scratch);
    unsigned long long* skq = reinterpret_cast<unsigned long long*>(scratch + SCN_CMAX * 8);
    int* sx = reinterpret_cast<int*>(scratch + SCN_CMAX * 8 + TK_Q * 8);

    const int rbase = blockIdx.y * SC_BM, range = blockIdx.x, R = gridDim.x;
    const long long c0 = (long long)range * tpr * SCN_TN, c1 = min(n_sel, c0 + (long long)tpr * SCN_TN);
    const int lrow = 32 * wid + r32, grow = rbase + lrow;      // this lane's row: local, global
    if (half == 0) {
        s_qn[lrow] = 0; s_ln[lrow] = 0; s_thr[lrow] = 0ull;
        if constexpr (F::GROW) {
            long long b;
            int n;
            F::row_list(F::grow(xarg), grow, mrows, b, n);
            s_xb[lrow] = b;
            s_xn[lrow] = n;
        } else {
            const bool on = ex.offs && grow < mrows;
            const long long b = on ? ex.offs[grow] : 0ll;
            s_xb[lrow] = b;
            s_xn[lrow] = on ? (int)(ex.offs[grow + 1] - b) : 0;
        }
    }
    // B operand: lane l holds h[row l & 31][16 ks + 8 (l >> 5) + j]
    const int D = m.Dtop;
    bf16x8 hb[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int kk = 16 * ks + 8 * half + j;
            hb[ks][j] = (short)((grow < mrows && kk < D) ? bf16_rne(h[(size_t)grow * D + kk]) : (unsigned short)0);
        }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();

    auto list = [&](int r) { return ws + ((size_t)(rbase + r) * R + range) * c; };
    auto merge_mine = [&]() {
        for (int r = 32 * wid; r < 32 * wid + 32; ++r)
            if (s_qn[r] > 0) topk_merge_row<true>(r, list(r), c, s_q + r * TK_Q, skq, sl, s_qn, s_ln, s_thr, s_xb[r], s_xn[r], item_idx, ex, sx);
    };
    // items of the tile at n0: element f = the item of column n0 + 32 f + (lane & 31), -1 past the range's end
    auto tile_items = [&](long long n0, int (&it)[2]) {
#pragma unroll
        for (int f = 0; f < 2; ++f) {
            const long long n = n0 + 32 * f + r32;
            it[f] = n < c1 ? (item_idx ? item_idx[n] : (int)n) : -1;
        }
    };
    // k-chunk ch (four k-steps) of both fragments of a tile
    auto load_chunk = [&](const int (&it)[2], int ch, bf16x8 (&w)[4][2]) {
#pragma unroll
        for (int f = 0; f < 2; ++f) {
            const int item = max(it[f], 0);
            const uint4* p = tab + ((size_t)(item >> 5) * KS + 4 * ch) * 64 + 32 * half + (item & 31);
#pragma unroll
            for (int s = 0; s < 4; ++s) w[s][f] = __builtin_bit_cast(bf16x8, p[64 * s]);
        }
    };

    bf16x8 w[2][4][2];
    int it[2], itn[2];
    tile_items(c0, it);
    if (c0 < c1) load_chunk(it, 0, w[0]);
    for (long long n0 = c0; n0 < c1; n0 += SCN_TN) {
        const int bi = half ? it[1] : it[0];            // the item of column n0 + lane
        const float by = bi >= 0 ? m.By[bi] : 0.f;
        tile_items(n0 + SCN_TN, itn);
        f32x16 acc[2];
#pragma unroll
        for (int f = 0; f < 2; ++f)
#pragma unroll
            for (int j = 0; j < 16; ++j) acc[f][j] = 0.f;
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
            if (ch + 1 < NCH) load_chunk(it, ch + 1, w[(ch + 1) & 1]);
            else if (n0 + SCN_TN < c1) load_chunk(itn, 0, w[0]);      // (NCH is even: the next tile starts in w[0] again)
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int f = 0; f < 2; ++f)
                    acc[f] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[ch & 1][s][f], hb[4 * ch + s], acc[f], 0, 0, 0);
        }
        s_by[lane] = by;
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
        // accumulator register j of fragment f: column n0 + 32 f + (j & 3) + 8 (j >> 2) + 4 half, row = this lane's
#pragma unroll
        for (int f = 0; f < 2; ++f) {
            const unsigned long long t = s_thr[lrow];
            const float tf = scan_thr_float(t);
            float v[16];
            bool any = false;
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int cc = 32 * f + (j & 3) + 8 * (j >> 2) + 4 * half;
                v[j] = final_act_fwd(m.final_act, m.fa_p0, m.fa_p1, acc[f][j] + s_by[cc]);
                any |= !(v[j] < tf);
            }
            if (__any(any)) {
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const long long n = n0 + 32 * f + (j & 3) + 8 * (j >> 2) + 4 * half;
                    if (grow < mrows && n < c1 && !(v[j] < tf) && topk_key(v[j], (unsigned)n) > t) {
                        const int p = atomicAdd(s_qn + lrow, 1);
                        s_q[lrow * TK_Q + p] = make_uint2(__float_as_uint(v[j]), (unsigned)n);
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                __builtin_amdgcn_wave_barrier();
                if (__any(s_qn[lrow] > TK_Q - 32)) merge_mine();
            }
        }
        it[0] = itn[0]; it[1] = itn[1];
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    merge_mine();
    for (int r = 32 * wid; r < 32 * wid + 32; ++r)
        if (rbase + r < mrows) {
            uint2* L = list(r);
            for (int j = s_ln[r] + lane; j < c; j += 64) L[j] = make_uint2(0u, 0xFFFFFFFFu);
        }
}

// One workgroup per row: the c-th largest key of the row's nl * c entries by k_topk_merge's radix select, then every real entry
// at or above it (exactly c; all the real ones, fewer than c, when the row has fewer than c eligible columns) goes to
// cols / items / approx[row * c + p] in no particular order and cnt[row] receives their number.  Positions past it hold column -1
// and item 0, which k_score_cand scores and k_scan_pack drops.
__global__ __launch_bounds__(256) void k_scan_merge(const uint2* ws, int nl, int c, const int* item_idx, int* cols, int* items,
                                                    float* approx, int* cnt) {
    __shared__ int hist[256];
    __shared__ int s_digit, s_need, s_cnt;
    const int tid = threadIdx.x;
    const uint2* L = ws + (size_t)blockIdx.x * nl * c;
    const int N = nl * c;
    unsigned long long prefix = 0ull, mask = 0ull;
    int need = c;
    for (int shift = 56; shift >= 0; shift -= 8) {
        hist[tid] = 0;
        if (tid == 0) { s_digit = 0; s_need = need; }
        __syncthreads();
        for (int i = tid; i < N; i += 256) {
            const unsigned long long key = topk_key(L[i]);
            if ((key & mask) == prefix) atomicAdd(hist + (int)((key >> shift) & 255u), 1);
        }
        __syncthreads();
        for (int o = 1; o < 256; o <<= 1) {
            const int x = tid + o < 256 ? hist[tid + o] : 0;
            __syncthreads();
            hist[tid] += x;
            __syncthreads();
        }
        const int ge = hist[tid], gt = tid < 255 ? hist[tid + 1] : 0;
        if (ge >= need && gt < need) { s_digit = tid; s_need = need - gt; }
        __syncthreads();
        prefix |= (unsigned long long)s_digit << shift;
        mask |= 255ull << shift;
        need = s_need;
        __syncthreads();
    }
    if (tid == 0) s_cnt = 0;
    __syncthreads();
    const size_t o = (size_t)blockIdx.x * c;
    for (int i = tid; i < N; i += 256) {
        const uint2 e = L[i];
        const unsigned long long key = topk_key(e);
        if (key != 0ull && key >= prefix) {
            const int p = atomicAdd(&s_cnt, 1);
            if (p < c) {
                cols[o + p] = (int)e.y;
                items[o + p] = item_idx ? item_idx[e.y] : (int)e.y;
                approx[o + p] = __uint_as_float(e.x);
            }
        }
    }
    __syncthreads();
    const int n = min(s_cnt, c);
    for (int p = n + tid; p < c; p += 256) { cols[o + p] = -1; items[o + p] = 0; approx[o + p] = 0.f; }
    if (tid == 0) cnt[blockIdx.x] = n;
}

// row r = blockIdx.y: ws[r][L] entry j = (bits of sc[r * c + j], column cols[r * c + j]) for j < cnt[r], the pad after it
__global__ __launch_bounds__(256) void k_scan_pack(const float* sc, const int* cols, const int* cnt, int c, int L, uint2* ws) {
    const int j = blockIdx.x * 256 + threadIdx.x, r = blockIdx.y;
    if (j >= L) return;
    ws[(size_t)r * L + j] = j < cnt[r] ? make_uint2(__float_as_uint(sc[(size_t)r * c + j]), (unsigned)cols[(size_t)r * c + j])
                                       : make_uint2(0u, 0xFFFFFFFFu);
}

// The six forms, once: F(k-chunks of 64 columns of the padded top layer, the type of the exclusions).  The instantiations here and
// the LDS opt-in at create (g4r_host_create.hpp) are this list; scan_launch (g4r_host_topk.hpp) picks NCH by scan_nch.
#define SCAN_FORMS(F) F(2, TkExcl) F(4, TkExcl) F(8, TkExcl) F(2, TkGrow) F(4, TkGrow) F(8, TkGrow)
#define SCAN_INSTANTIATE(NCH, E) \
    template __global__ void k_scan_bf16<NCH, E>(const DevModel*, const float*, int, const int*, long long, const uint4*, int, int, uint2*, E);
SCAN_FORMS(SCAN_INSTANTIATE)
#undef SCAN_INSTANTIATE

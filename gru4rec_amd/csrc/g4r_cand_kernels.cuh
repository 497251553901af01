// Per-row candidate scoring kernels (gfx950), behind g4r_score_candidates / g4r_score_candidates_sessions (not in the reference).
//   k_score_cand    row r's own candidate list (CSR) -> its scores in CSR order: gathered Wy rows, the k_score_all chain
//   k_softmax_csr   k_softmax_rows over each CSR row (softmax / softmax_logit final activations)
//   k_cand_pack     CSR scores -> per-row lists of (score bits, position) for the unchanged k_topk_merge
// Bit-exactness: a score is computed by the very instruction sequence of k_score_all -- 16x16x4 fp32 MFMAs over ascending k of the
// padded Dtop, from zero, then + By[item], then the element-wise final activation -- with the row's hidden state broadcast to all
// 16 A rows (15 of the 16 output rows are discarded: the gather, not the MFMA, bounds the kernel).  Element (0, j) of an MFMA depends
// only on A row 0, B column j and the accumulator (0, j), so every score equals g4r_predict_step's at the same item, bit for bit.
#pragma once
#include "g4r_topk_kernels.cuh"

#define CS_SLICE 256           // positions per work item: a long row is split, so it is not serialised behind short ones
#define CS_KC 128              // Wy columns staged per wave and chunk
#define CS_LD (CS_KC + 4)      // LDS row stride of the staged rows: the B reads (row li, column kk + lg) hit 64 distinct banks
#define CS_TOPK_ENTRIES (1 << 24)   // top-k list entries one k_cand_pack / k_topk_merge pair may fill (128 MiB)
#define CS_DMAX 1024           // widest top layer (g4r_create refuses wider ones): the hidden row is staged in LDS once per work item

// One workgroup per work item {h row, first position, end position, first position of the row's list}; positions index `items` and
// `out`.  Wave w scores the groups of 16 positions p0 + 16 w + 64 i: the group's Wy rows are gathered (one float4 per lane, half a
// wave per row and load) into the wave's LDS slab chunk by chunk, then fed to the MFMA chain as k_score_all's B operand.
__global__ __launch_bounds__(256) void k_score_cand(const DevModel* __restrict__ mp, const float* h, const int* items, const int4* work,
                                                    float* out, int apply_act) {
    __shared__ __attribute__((aligned(16))) float sH[CS_DMAX];
    __shared__ __attribute__((aligned(16))) float sB[4][16 * CS_LD];
    __shared__ int sIt[4][16];
    const DevModel& m = *mp;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, li = lane & 15, lg = lane >> 4;
    const int D = m.Dtop;
    const int4 w = work[blockIdx.x];
    const float* hr = h + (size_t)w.x * D;
    for (int j = 4 * tid; j < D; j += 1024) *reinterpret_cast<float4*>(sH + j) = ld4(hr + j);
    __syncthreads();
    float* sb = sB[wid];
    int* si = sIt[wid];
    for (int g0 = w.y + 16 * wid; g0 < w.z; g0 += 64) {
        // the group's 16 positions; past the slice's end the last one is scored again and not stored
        const int p = min(g0 + li, w.z - 1);
#if defined(G4R_MUTATE) && G4R_MUTATE == 11      // test build: a work item past a row's first slice reads the first slice's items
        const int item = items[w.y > w.w ? p - (w.y - w.w) : p];
#else
        const int item = items[p];
#endif
        if (lane < 16) si[lane] = item;
        f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int kc0 = 0; kc0 < D; kc0 += CS_KC) {
            const int kc = min(CS_KC, D - kc0), kc4 = kc >> 2;
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            __builtin_amdgcn_wave_barrier();      // sIt written / the previous chunk's B reads done before the slab is refilled
            for (int e = lane; e < 16 * kc4; e += 64) {
                const int r = e / kc4, c4 = e - r * kc4;
                *reinterpret_cast<float4*>(sb + r * CS_LD + 4 * c4) = ld4(m.Wy + (size_t)si[r] * D + kc0 + 4 * c4);
            }
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            __builtin_amdgcn_wave_barrier();
            for (int kk = 0; kk < kc; kk += 4) acc = mfma16(sH[kc0 + kk + lg], sb[li * CS_LD + kk + lg], acc);
        }
        if (lg == 0 && g0 + li < w.z) {
            float v = acc[0] + m.By[item];
            if (apply_act) v = final_act_fwd(m.final_act, m.fa_p0, m.fa_p1, v);
            out[g0 + li] = v;
        }
    }
}

// in-place softmax of each CSR row (one 256-thread workgroup per row): k_softmax_rows' code with n_sel = the row's length, so the
// bits equal k_softmax_rows' over that row's list
__global__ __launch_bounds__(256) void k_softmax_csr(float* sc, const long long* offs) {
    __shared__ float red[8];
    float* row = sc + offs[blockIdx.x];
    const long long n_sel = offs[blockIdx.x + 1] - offs[blockIdx.x];
    float mx = -INFINITY;
    for (long long j = threadIdx.x; j < n_sel; j += 256) mx = fmaxf(mx, row[j]);
    mx = block_max_256(mx, red);
    float sm = 0.f;
    for (long long j = threadIdx.x; j < n_sel; j += 256) sm += expf(row[j] - mx);
    sm = block_sum_256(sm, red);
    for (long long j = threadIdx.x; j < n_sel; j += 256) row[j] = expf(row[j] - mx) / sm;
}

// rows [0, gridDim.y) of a CSR (offs relative to sc) -> ws[row][L]: entry j = (score bits, position j) for j < the row's length,
// the pad (position 0xFFFFFFFF, key 0) after it.  L = nl * k: the row's nl lists of k_topk_merge.  Real keys are > 0 and distinct
// (positions are), so k_topk_merge returns the k best positions in the order of g4r_recommend_step.
__global__ __launch_bounds__(256) void k_cand_pack(const float* sc, const long long* offs, int L, uint2* ws) {
    const int j = blockIdx.x * 256 + threadIdx.x, r = blockIdx.y;
    if (j >= L) return;
    const long long b = offs[r], n = offs[r + 1] - b;
    ws[(size_t)r * L + j] = j < n ? make_uint2(__float_as_uint(sc[b + j]), (unsigned)j) : make_uint2(0u, 0xFFFFFFFFu);
}

// Per-group caps (gfx950), behind g4r_recommend_sessions_capped / g4r_continue_sessions_capped / g4r_cap_lists (not in the reference).
//   k_group_cap  the greedy walk down a row's list of P <= G4R_TOPK_MAX positions with one counter per item group: position j is kept
//                iff its item is ungrouped or fewer than `cap` positions of its group lie in the row's prior list and ahead of it in
//                the list (the cap rule of include/gru4rec_hip.h).  The first k kept positions leave, in list order.
// One 256-thread workgroup per row, thread j owns position j.  Nothing is scored: a returned score is the bit pattern that came in.
// The phases, one barrier each:
//   1  the row's groups (column -> item -> group table) and its prior list into LDS;
//   2  every thread counts its group in the prior list and among the positions ahead of it -- all lanes of a wave read the same
//      LDS address in the same trip, a broadcast -- and forms its keep flag; 64-bit ballot + popcount rank the kept positions
//      inside a wave, the wave totals go through LDS;
//   3  the kept positions of rank < k write (column, score, position), the slots behind them the pad, thread 0 the count.
#pragma once
#include "g4r_topk_kernels.cuh"

#define GC_THREADS 256
static_assert(G4R_TOPK_MAX <= GC_THREADS, "k_group_cap: one thread per list position");
static_assert(G4R_GROUP_PRIOR_MAX % 4 == 0, "k_group_cap reads the staged prior list in quads");

// grid: one workgroup of GC_THREADS threads per row.
//   cols, scores     [rows][P] the lists in selection order (scores NULL: g4r_cap_lists, nothing to copy)
//   map, n_cols      column -> item index (NULL: the column is the item); a column outside [0, n_cols) counts as ungrouped
//   groups, n_items  the model's group table, -1 = ungrouped
//   pbeg, plen, prior  the row's prior list prior[pbeg[row] .. pbeg[row] + plen[row]), unsorted group indices, at most
//                    G4R_GROUP_PRIOR_MAX of them (prior NULL: every row's is empty)
//   cont             continuation mode: a row that keeps nothing sends its list position 0 out in slot 0 (the fallback winner); its
//                    count stays 0 and reports it
//   append           (continuation, every step but the last) the group of the row's winner -- slot 0 --, if it has one, is
//                    appended to the prior list and plen[row] bumped; the host leaves the slack behind every list
//   out_cols, out_scores, out_pos  [rows][k] (each may be NULL): the first k kept positions, then pads (-1, NaN, -1)
//   out_kept         out_kept[row * kept_stride] = min(k, kept positions)
__global__ __launch_bounds__(GC_THREADS) void k_group_cap(const int* __restrict__ cols, const float* __restrict__ scores, int P,
                                                          const int* __restrict__ map, long long n_cols, const int* __restrict__ groups,
                                                          int n_items, int cap, int k, const long long* __restrict__ pbeg, int* plen,
                                                          int* prior, int cont, int append, int* __restrict__ out_cols,
                                                          float* __restrict__ out_scores, int* __restrict__ out_pos,
                                                          int* __restrict__ out_kept, int kept_stride) {
    __shared__ __attribute__((aligned(16))) int s_grp[GC_THREADS];
    __shared__ __attribute__((aligned(16))) int s_prior[G4R_GROUP_PRIOR_MAX];
    __shared__ int s_wtot[GC_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const size_t row = blockIdx.x;
    const float pad = __int_as_float(0x7FC00000);

    // ---- 1: the groups of the list, the prior list
    const bool mine = tid < P;
    int col = -1, g = -1;
    float s = pad;
    if (mine) {
        col = cols[row * P + tid];
        if (scores) s = scores[row * P + tid];
        int item = -1;
        if (col >= 0 && col < n_cols) item = map ? map[col] : col;
        if (item >= 0 && item < n_items) g = groups[item];
    }
    s_grp[tid] = g;
    const int n0 = prior ? min(plen[row], G4R_GROUP_PRIOR_MAX) : 0, n04 = (n0 + 3) & ~3;
    const long long beg = prior ? pbeg[row] : 0;
    for (int i = tid; i < n04; i += GC_THREADS) s_prior[i] = i < n0 ? prior[beg + i] : -2;      // (-2 matches no group)
    __syncthreads();

    // ---- 2: the counter of the position's group where the walk reaches it, the keep flag, its rank among the kept
    int cnt = 0;
    if (g >= 0) {
        for (int i = 0; i < n04; i += 4) {
            const int4 q = *reinterpret_cast<const int4*>(s_prior + i);
            cnt += (q.x == g) + (q.y == g) + (q.z == g) + (q.w == g);
        }
#if defined(G4R_MUTATE) && G4R_MUTATE == 26      // test build: the positions of earlier waves are forgotten
        const int first = wid * 64;
#else
        const int first = 0;
#endif
        for (int i = first; i < tid; i += 4) {      // (i + 3 <= 255: inside s_grp)
            const int4 q = *reinterpret_cast<const int4*>(s_grp + i);
            cnt += (q.x == g) + (i + 1 < tid && q.y == g) + (i + 2 < tid && q.z == g) + (i + 3 < tid && q.w == g);
        }
    }
    const bool keep = mine && (g < 0 || cnt < cap);
    const unsigned long long bal = __ballot(keep);
    if (lane == 0) s_wtot[wid] = __popcll(bal);
    __syncthreads();
    int rank = __popcll(bal & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
    for (int w = 0; w < GC_THREADS / 64; ++w) {
        const int t = s_wtot[w];
        total += t;
        if (w < wid) rank += t;
    }
    const int nk = min(k, total);

    // ---- 3: the first k kept positions, the pads, the count; the winner's group joins the prior list
    const size_t o = row * k;
    const bool fallback = cont && total == 0;      // thread 0 owns list position 0 and slot 0
    if (keep && rank < k) {
        if (out_cols) out_cols[o + rank] = col;
        if (out_scores) out_scores[o + rank] = s;
        if (out_pos) out_pos[o + rank] = tid;
    }
    if (tid >= nk && tid < k) {
        const bool fb = fallback && tid == 0;
        if (out_cols) out_cols[o + tid] = fb ? col : -1;
        if (out_scores) out_scores[o + tid] = fb ? s : pad;
        if (out_pos) out_pos[o + tid] = fb ? 0 : -1;
    }
    if (tid == 0) out_kept[row * kept_stride] = nk;
    if (append && g >= 0 && ((keep && rank == 0) || (fallback && tid == 0))) {      // exactly one thread: every read of the list is behind a barrier
        prior[beg + n0] = g;
        plen[row] = n0 + 1;
    }
}

// Multi-step continuation kernels (gfx950), behind g4r_continue_sessions (not in the reference): the device-side edge between one
// step's selection and the next step's GRU input.
//   k_rollout_align  after the replay a row's state lies in the ping-pong half its own history length picks (H[len & 1]); the rollout
//                    steps ALL rows of the chunk together, so rows of the other parity are first copied into the half of the chunk's
//                    longest history (H[tmax & 1])
//   k_rollout_feed   per row, after the merge of step s: the step's k (column, score) pairs go to [row][s][.] of the chunk's output,
//                    the winner's item index becomes the row's GRU input of step s + 1 and, with no_repeat, is inserted into the
//                    row's sorted exclusion list (TkGrow, g4r_topk_kernels.cuh)
#pragma once
#include "g4r_topk_kernels.cuh"

// sorted row r of one layer: H[tmax & 1] <- H[(tmax & 1) ^ 1] where len[r] and tmax differ in parity (dst / src: those two halves)
__global__ __launch_bounds__(256) void k_rollout_align(float* dst, const float* src, const int* len, int rows, int W, int tmax) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)rows * W) return;
    const int r = (int)(e / W);
    if ((len[r] ^ tmax) & 1) dst[e] = src[e];
}

// One wave per row (grid = rows, 64 threads).  tcols / tscores: the merge's [rows][k] result of step s.  out_cols / out_scores:
// [rows][steps][k].  next_in != NULL (every step but the last): next_in[row] <- the item index of the winning column (item_idx[col],
// or col).  grow.len != NULL (no_repeat, every step but the last): that item is inserted into the row's sorted list
// xitems[beg .. beg + len): the place by binary search, the tail moved up by one in runs of 64 from the top (each lane's store
// carries the value its own load returned, and a run's stores end below the addresses the next run loads), then the item and the
// new length.  The item is never in the list already: it was eligible in the selection that has just chosen it.  The host leaves
// steps - 1 slots of slack behind every list, and checks that no list outgrows G4R_EXCLUDE_MAX.
__global__ __launch_bounds__(64) void k_rollout_feed(const int* tcols, const float* tscores, int k, int steps, int s, const int* item_idx,
                                                     int* out_cols, float* out_scores, int* next_in, const long long* xbeg, int* xlen,
                                                     int* xitems) {
    const int row = blockIdx.x, lane = threadIdx.x;
    const size_t o = ((size_t)row * steps + s) * k;
    for (int j = lane; j < k; j += 64) {
        out_cols[o + j] = tcols[(size_t)row * k + j];
        out_scores[o + j] = tscores[(size_t)row * k + j];
    }
    if (!next_in) return;
    const int col = tcols[(size_t)row * k];
    const int item = item_idx ? item_idx[col] : col;
    if (lane == 0) next_in[row] = item;
    if (!xlen) return;
    int* L = xitems + xbeg[row];
    const int n = xlen[row];
    int a = 0, b = n;
    while (a < b) { const int mid = (a + b) >> 1; if (L[mid] < item) a = mid + 1; else b = mid; }
#if defined(G4R_MUTATE) && G4R_MUTATE == 14      // test build: an item that sorts above the whole list is dropped
    if (a == n) return;
#endif
    for (int top = n; top > a; top -= 64) {
        const int j = top - 1 - lane;      // this run: positions (top - 64, top - 1] that are >= a
        const bool on = j >= a;
        const int v = on ? L[j] : 0;
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (on) L[j + 1] = v;
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    if (lane == 0) { L[a] = item; xlen[row] = n + 1; }
}

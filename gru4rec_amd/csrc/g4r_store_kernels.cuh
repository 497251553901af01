// Session-store kernels (gfx950), behind g4r_store_push / g4r_store_peek / g4r_store_read / g4r_store_write (not in the reference): the
// edges between the replay of a call's events (replay_chunks, g4r_host_sessions.hpp) and the slots of the device-resident store.
// A store holds `capacity` slots: per layer the hidden rows [capacity][W_l] (W_l: the model's 4-padded width), the seen lists
// [capacity][seen_cap] (sorted, duplicate-free item indices), their lengths [capacity] and overflow flags [capacity].  Within a call a
// slot belongs to one row of one chunk (the host refuses a slot listed twice), so nothing here needs an atomic.
//   k_store_load   sorted row r of a layer's H[0] <- the store row of its slot, or zeros for a fresh row
//   k_store_save   the store row of sorted row r's slot <- its final state, from the ping-pong half its own event count selects
//   k_store_seen   per row: the call's items merged into the slot's sorted list (k_rollout_feed's insertion), the row's (begin, length)
//                  written for the TkGrow selection forms
//   k_store_move   rows of 32-bit words between a staging array and the store's rows of a list of slots (read / write)
// slot / fresh are in chunk order (the caller's rows), perm[r] is the chunk row of sorted row r (NULL: r itself).
#pragma once
#include "g4r_topk_kernels.cuh"

__global__ __launch_bounds__(256) void k_store_load(float* H0, const float* store, const int* slot, const int* fresh, const int* perm,
                                                    int rows, int W) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)rows * W) return;
    const int r = (int)(e / W), j = (int)(e - (long long)r * W);
    const int i = perm ? perm[r] : r;
    H0[e] = (fresh && fresh[i]) ? 0.f : store[(size_t)slot[i] * W + j];
}

// len[r]: sorted row r's event count (k_replay_final's rule: the state lies in H[len & 1]); tmax: the chunk's longest row (len[0])
__global__ __launch_bounds__(256) void k_store_save(float* store, const float* H0, const float* H1, const int* slot, const int* perm,
                                                    const int* len, int rows, int W, int tmax) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)rows * W) return;
    const int r = (int)(e / W), j = (int)(e - (long long)r * W);
#if defined(G4R_MUTATE) && G4R_MUTATE == 33      // test build: every row read from the half of the chunk's longest row
    const int par = tmax & 1;
#else
    const int par = len[r] & 1;
    (void)tmax;
#endif
    store[(size_t)slot[perm[r]] * W + j] = (par ? H1 : H0)[e];
}

// One wave per sorted row (grid = rows, 64 threads), run before the selection.  steps: the chunk's step-major input items [T][rows]
// (what the replay uploaded), row r's events are steps[t * rows + r], t < len[r], in event order; len NULL (g4r_store_peek): no events.
// Each item is merged into the slot's list s_items[slot * seen_cap ..): the place by binary search (every lane runs the same search),
// an item found there is skipped, otherwise the tail is moved up by one in runs of 64 from the top -- each lane's store carries the
// value its own load returned, and a run's stores end below the addresses the next run loads -- then lane 0 writes the item.  The
// fence + wave barrier behind every run and behind lane 0's store order them before the loads of the next run / the next item's
// search (k_rollout_feed's load-before-store rule, g4r_rollout_kernels.cuh).  A full list records nothing further: a new item sets
// the slot's flag.  So the list is the first seen_cap distinct items of the session in event order, held sorted.  A fresh row starts
// from length 0 and a clear flag.  xbeg / xlen[r]: the row's list for TkGrow; oflag[r]: its flag after the call.
__global__ __launch_bounds__(64) void k_store_seen(const int* steps, int rows, const int* perm, const int* len, const int* slot,
                                                   const int* fresh, int seen_cap, int* s_items, int* s_len, int* s_flag, long long* xbeg,
                                                   int* xlen, int* oflag) {
    const int row = blockIdx.x, lane = threadIdx.x;
    const int i = perm ? perm[row] : row;
    const int sl = slot[i];
    const bool fr = fresh && fresh[i];
    int* L = s_items + (size_t)sl * seen_cap;
    int n = fr ? 0 : s_len[sl];
    int flag = fr ? 0 : s_flag[sl];
    const int T = len ? len[row] : 0;
    for (int t = 0; t < T; ++t) {
        const int item = steps[(size_t)t * rows + row];
        int a = 0, b = n;
        while (a < b) { const int mid = (a + b) >> 1; if (L[mid] < item) a = mid + 1; else b = mid; }
        if (a < n && L[a] == item) continue;
        if (n >= seen_cap) { flag = 1; continue; }
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
        if (lane == 0) L[a] = item;
        ++n;
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    if (lane == 0) {
        if (len) { s_len[sl] = n; s_flag[sl] = flag; }
        xbeg[row] = (long long)sl * seen_cap;
        xlen[row] = n;
        oflag[row] = flag;
    }
}

// to_store 0: buf[r][.] <- store[slot[r]][.]; 1: the other way.  W words per row
__global__ __launch_bounds__(256) void k_store_move(unsigned* store, unsigned* buf, const int* slot, int rows, int W, int to_store) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)rows * W) return;
    const int r = (int)(e / W), j = (int)(e - (long long)r * W);
    const size_t s = (size_t)slot[r] * W + j;
    if (to_store) store[s] = buf[e];
    else buf[e] = store[s];
}

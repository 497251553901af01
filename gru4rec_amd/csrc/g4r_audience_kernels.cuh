// Audience kernels (gfx950), behind g4r_audience_sessions (not in the reference): the k sessions with the largest value for each of M
// items -- a selection DOWN the columns of the [sessions][items] value matrix, kept on the device while the sessions stream past in
// chunks of at most AUD_CHUNK rows (replay_chunks), so that only M x k entries ever reach the host.
//   k_audience_keys    a chunk's z[rows][M] (k_score_cand: g4r_predict_step's bit pattern) -> one entry per (item, row), item-major
//   k_audience_merge   one item's chunk entries + that item's running list (k sorted entries) -> its new running list
//   k_audience_finish  after the last chunk: the running lists -> (session, value) arrays, padded behind every item's count
// An entry is 16 bytes: x = topk_key(value, session) -- g4r_recommend_step's order with the session's index into the caller's histories
// in the place of the column: value descending, equal values (float ==, so -0.0 == +0.0) to the lower index, NaN below every number --,
// y = the value's own bits (the key folds -0.0 and every NaN).  Key 0 pads: an ineligible (item, row) pair.  Sessions are distinct, so
// the keys of one item are, and "the k best" is exactly the k largest keys whatever the chunking.
// The running lists live in two buffers A and B of [M][k] entries; side[j] says which one holds item j's list and len[j] its length.
// A merge reads (side_in, len_in) and the list on that side, writes the merged list to the OTHER side and (side_out, len_out) -- the
// host swaps the two small arrays between launches -- or, when no chunk entry can enter the list, writes nothing but
// side_out = side_in: every workgroup of an item reaches that decision from the same words of the previous launches, so no workgroup
// waits for, or reads anything from, another one of its own launch.
#pragma once
#include "g4r_topk_kernels.cuh"

#define AUD_CHUNK 512          // most rows of a chunk (G4R_REPLAY_CHUNK): the entries k_audience_merge sorts in LDS
#define AUD_TILE 1024          // list entries per workgroup of k_audience_merge (4 per thread)

// One thread per (sorted row r, item j) of a chunk (grid = ceil(rows M / 256)).  z[r][M]: the items' scores for the row; perm[r]: the
// row's place in the chunk, c0 the chunk's first session.  xbeg / xlen / xitems (NULL: no exclusion): row r's sorted distinct history
// items, xlen[r] of them from xitems[xbeg[r]]: a row whose history holds the item is not eligible for it.  zeta / Q (NULL: the value
// is z itself): the row's normaliser, the value is lse_logprob.  ent[j][rows] <- the entry, key 0 where the row is not eligible.
__global__ __launch_bounds__(256) void k_audience_keys(const float* z, const int* items, int M, int rows, const int* perm, int c0,
                                                       const long long* xbeg, const int* xlen, const int* xitems, const float* zeta,
                                                       const unsigned long long* Q, float invT, ulonglong2* ent) {
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= (long long)rows * M) return;
    const int r = (int)(p / M), j = (int)(p - (long long)r * M);
    bool ok = true;
    if (xbeg) {
        const int item = items[j];
        const int* l = xitems + xbeg[r];
        int lo = 0, hi = xlen[r];
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (l[mid] < item) lo = mid + 1; else hi = mid;
        }
        ok = !(lo < xlen[r] && l[lo] == item);
    }
    float v = z[p];
    if (zeta) v = lse_logprob(v, zeta[r], Q[r], invT);
#if defined(G4R_MUTATE) && G4R_MUTATE == 28      // test build: the session's index within its chunk
    const unsigned sess = (unsigned)perm[r];
#else
    const unsigned sess = (unsigned)(c0 + perm[r]);
#endif
    ent[(size_t)j * rows + r] = ok ? make_ulonglong2(topk_key(v, sess), (unsigned long long)__float_as_uint(v)) : make_ulonglong2(0ull, 0ull);
}

// the number of keys greater than x among a[0 .. n), a sorted descending
template <class A>
__device__ __forceinline__ int aud_rank(A a, int n, unsigned long long x) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a(mid) > x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// Grid (ceil(k / AUD_TILE), M), 256 threads: workgroup (t, j) merges item j's chunk entries ent[j][rows] into its running list.
// Every workgroup of the item sorts the chunk's entries in LDS (bitonic over P, the power of two >= max(rows, 2), pads last; nv of
// them are real).  Nothing can enter the list when nv == 0, or when the list is full and its last key beats the chunk's best: then
// only (side_out, len_out) = (side_in, len_in) is written.  Otherwise element i of either sorted run goes to (i + the number of
// greater keys in the other run) of the list on the other side -- the keys are distinct, so the places are --, places at and beyond
// k are dropped: the workgroup places list entries [t AUD_TILE, (t + 1) AUD_TILE) and the chunk entries t 256 + tid, + 256 gridDim.x, ...
__global__ __launch_bounds__(256) void k_audience_merge(const ulonglong2* ent, int rows, int P, int k, ulonglong2* A, ulonglong2* B,
                                                        const int* side_in, const int* len_in, int* side_out, int* len_out) {
    __shared__ unsigned long long sK[AUD_CHUNK];
    __shared__ unsigned sV[AUD_CHUNK];
    __shared__ int s_nv;
    const int tid = threadIdx.x, j = blockIdx.y, t = blockIdx.x;
    const ulonglong2* e = ent + (size_t)j * rows;
    if (tid == 0) s_nv = 0;
    __syncthreads();
    int mine = 0;
    for (int i = tid; i < P; i += 256) {
        const ulonglong2 x = i < rows ? e[i] : make_ulonglong2(0ull, 0ull);
        sK[i] = x.x;
        sV[i] = (unsigned)x.y;
        mine += x.x != 0ull ? 1 : 0;
    }
    if (mine) atomicAdd(&s_nv, mine);
    for (int size = 2; size <= P; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (int i = tid; i < (P >> 1); i += 256) {
                const int a = 2 * i - (i & (stride - 1)), b = a + stride;
                const unsigned long long ka = sK[a], kb = sK[b];
                if ((ka < kb) == ((a & size) == 0)) {
                    const unsigned va = sV[a];
                    sK[a] = kb; sK[b] = ka;
                    sV[a] = sV[b]; sV[b] = va;
                }
            }
        }
    __syncthreads();
    const int nv = s_nv, side = side_in[j], len = len_in[j];
    const ulonglong2* src = (side ? B : A) + (size_t)j * k;
    ulonglong2* dst = (side ? A : B) + (size_t)j * k;
    const bool keep = nv == 0 || (len == k && src[k - 1].x > sK[0]);
    if (t == 0 && tid == 0) {
        side_out[j] = keep ? side : side ^ 1;
        len_out[j] = keep ? len : min(k, len + nv);
    }
    if (keep) return;
    for (int i = t * AUD_TILE + tid; i < min(len, (t + 1) * AUD_TILE); i += 256) {
        const ulonglong2 x = src[i];
        const int to = i + aud_rank([&](int q) { return sK[q]; }, nv, x.x);
        if (to < k) dst[to] = x;
    }
    for (int c = t * 256 + tid; c < nv; c += 256 * gridDim.x) {
        const unsigned long long key = sK[c];
        const int to = c + aud_rank([&](int q) { return src[q].x; }, len, key);
        if (to < k) dst[to] = make_ulonglong2(key, (unsigned long long)sV[c]);
    }
}

// Grid (ceil(k / 256), M): item j's list (on side[j], len[j] entries) -> sess / val[j][k]: the session's index (the key's low word,
// complemented) and the value's bits; -1 and NaN at and after len[j]
__global__ __launch_bounds__(256) void k_audience_finish(const ulonglong2* A, const ulonglong2* B, const int* side, const int* len, int k,
                                                         int* sess, float* val) {
    const int i = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
    if (i >= k) return;
    const size_t o = (size_t)j * k + i;
    if (i < len[j]) {
        const ulonglong2 x = (side[j] ? B : A)[o];
        sess[o] = (int)~(unsigned)x.x;
        val[o] = __uint_as_float((unsigned)x.y);
    } else {
        sess[o] = -1;
        val[o] = __uint_as_float(0x7FC00000u);
    }
}

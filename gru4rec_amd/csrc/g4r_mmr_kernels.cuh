// Diversified top-k (gfx950), behind g4r_diversify_lists / g4r_diversify_sessions (not in the reference).
//   k_mmr_rerank  maximal marginal relevance over a row's pool of P <= G4R_DIVERSIFY_POOL_MAX candidates: one 256-thread workgroup per
//                 row gathers the pool's table rows in k-chunks, forms the pool's P x P matrix of raw dot products in 16 x 16 MFMA
//                 tiles and then picks k positions greedily, each pick by a workgroup arg-max on topk_key.
// The arithmetic is the contract of include/gru4rec_hip.h, every operation IEEE fp32 in the order given there:
//   relevance   r_j = s_j, or (s_j - lo) / (hi - lo) over the row's minimum and maximum (0 when hi == lo) with `normalize`
//   similarity  g4r_similar_items' pair score with the picked item as the query and the pool member as the candidate: one
//               ascending-k chain of mfma16 from zero over the two table rows (the accumulators of a row wider than one k-chunk
//               wait in the matrix between the chunks, so the chain is never split), cosine (dot * inv[picked]) * inv[member]
//   value       pick 0: lam * r_j.  Pick t >= 1: (lam * r_j) - (mu * m_j), m_j the largest similarity to the picks so far; two
//               rounded products and one rounded subtraction
//   pick        the largest value in topk_key's order (value descending, lower position first, NaN last)
// Entry [i][j] of the matrix has row i as the MFMA's A operand and row j as its B operand, as k_sim_range has the query and the
// candidate: nothing is taken from the matrix's symmetry.  The inverse norms scale an entry where it is used.
#pragma once
#include "g4r_sim_kernels.cuh"

#define MMR_KC SC_KC                       // floats of a table row staged per k-chunk
#define MMR_LDK (MMR_KC + 2)
#define MMR_PAD(P) (((P) + 15) & ~15)      // the pool padded to whole MFMA tiles (pad rows are zero rows nobody picks)
// LDS: [matrix Pp x Pp | staged chunk Pp x MMR_LDK]
#define MMR_SMEM(P) ((size_t)MMR_PAD(P) * (MMR_PAD(P) + MMR_LDK) * 4)
static_assert(G4R_DIVERSIFY_POOL_MAX % 16 == 0 && G4R_DIVERSIFY_POOL_MAX <= 128, "one thread of the first two waves per pool position");
static_assert(MMR_SMEM(G4R_DIVERSIFY_POOL_MAX) + 4096 <= 156 * 1024, "k_mmr_rerank LDS over the 156 KiB the kernels may ask for");

// a * b rounded on its own.  hipcc contracts a product into the subtraction that uses it, and __fmul_rn does not stop it (the headers
// define it as the plain product); the empty asm hides the product from that
__device__ __forceinline__ float mmr_mul(float a, float b) {
    float p = a * b;
    asm volatile("" : "+v"(p));
    return p;
}

// grid: one workgroup of 256 threads per row.
//   T / W / n_items  the item table, its row width (floats, a multiple of 4) and its rows
//   cols, rel        [rows][P] the pool: candidate columns and their relevance (g4r_diversify_lists: item indices, map NULL)
//   map, n_cols      column -> item index (NULL: the column is the item); a column outside [0, n_cols) counts as a zero row
//   inv              COS: the table's inverse norms, by item index
//   out_pos, out_val [rows][k] the picked positions and their values; out_cols / out_rel (NULL: not wanted) cols / rel of the picks
template <bool COS>
__global__ __launch_bounds__(256) void k_mmr_rerank(const float* __restrict__ T, int W, int n_items, const int* __restrict__ cols,
                                                    const float* __restrict__ rel, const int* __restrict__ map, long long n_cols,
                                                    const float* __restrict__ inv, int P, int k, float lam, int normalize,
                                                    int* __restrict__ out_pos, float* __restrict__ out_val, int* __restrict__ out_cols,
                                                    float* __restrict__ out_rel) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ int s_item[G4R_DIVERSIFY_POOL_MAX];
    __shared__ float s_inv[G4R_DIVERSIFY_POOL_MAX];
    __shared__ float s_red[8];
    __shared__ unsigned long long s_best[4];
    __shared__ int s_last;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, li = lane & 15, lg = lane >> 4;
    const int Pp = MMR_PAD(P), nt = Pp >> 4, nq = (nt + 3) >> 2;
    float* sG = smem;
    float* sR = smem + Pp * Pp;
    const size_t row = blockIdx.x;
    cols += row * P; rel += row * P;

    // ---- the pool: items, inverse norms, relevance (thread j owns position j)
    const bool mine = tid < P;
    int col = -1, item = -1;
    float s = 0.f, iv = 0.f;
    if (mine) {
        col = cols[tid];
        s = rel[tid];
        if (col >= 0 && col < n_cols) item = map ? map[col] : col;
        if (item < 0 || item >= n_items) item = -1;
        if (COS && item >= 0) iv = inv[item];
    }
    if (tid < G4R_DIVERSIFY_POOL_MAX) { s_item[tid] = item; s_inv[tid] = iv; }
    float r = s;
    if (normalize) {
        float lo = mine ? s : INFINITY, hi = mine ? s : -INFINITY;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { lo = fminf(lo, __shfl_xor(lo, o)); hi = fmaxf(hi, __shfl_xor(hi, o)); }
        if (lane == 0) { s_red[wid] = lo; s_red[4 + wid] = hi; }
        __syncthreads();
        lo = fminf(fminf(s_red[0], s_red[1]), fminf(s_red[2], s_red[3]));
        hi = fmaxf(fmaxf(s_red[4], s_red[5]), fmaxf(s_red[6], s_red[7]));
        r = hi > lo ? __fdiv_rn(s - lo, hi - lo) : 0.f;
    }
    __syncthreads();

    // ---- the matrix of raw dot products, k-chunk by k-chunk
    for (int kc0 = 0; kc0 < W; kc0 += MMR_KC) {
        const int kc = min(MMR_KC, W - kc0), kc4 = kc >> 2;
        for (int e = tid; e < Pp * kc4; e += 256) {
            const int i = e / kc4, c4 = e - i * kc4, it = s_item[i];
            float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
            if (it >= 0) x = ld4(T + (size_t)it * W + kc0 + 4 * c4);
            float2* d = reinterpret_cast<float2*>(sR + i * MMR_LDK + 4 * c4);
            d[0] = make_float2(x.x, x.y);
            d[1] = make_float2(x.z, x.w);
        }
        __syncthreads();
        // a wave takes four tiles of one tile row at a time: four independent chains keep the MFMA pipe busy
        for (int q = wid; q < nt * nq; q += 4) {
            const int ti = q / nq, tj0 = (q - ti * nq) * 4;
            f32x4 acc[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int tj = min(tj0 + u, nt - 1);
#pragma unroll
                for (int rg = 0; rg < 4; ++rg) acc[u][rg] = kc0 ? sG[(16 * ti + 4 * lg + rg) * Pp + 16 * tj + li] : 0.f;
            }
            for (int kk = 0; kk < kc; kk += 4) {
                const float a = sR[(16 * ti + li) * MMR_LDK + kk + lg];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int tj = min(tj0 + u, nt - 1);
                    acc[u] = mfma16(a, sR[(16 * tj + li) * MMR_LDK + kk + lg], acc[u]);
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (tj0 + u < nt) {
#pragma unroll
                    for (int rg = 0; rg < 4; ++rg) sG[(16 * ti + 4 * lg + rg) * Pp + 16 * (tj0 + u) + li] = acc[u][rg];
                }
        }
        __syncthreads();
    }

    // ---- k greedy picks
    const float mu = 1.0f - lam, lr = mmr_mul(lam, r);
    float mj = 0.f;
    bool free_ = mine;
    out_pos += row * k; out_val += row * k;
    for (int t = 0; t < k; ++t) {
        float v = lr;
        if (t > 0 && free_) {
            const int last = s_last;
            float sim = sG[last * Pp + tid];
            if constexpr (COS) sim = (sim * s_inv[last]) * iv;
#if defined(G4R_MUTATE) && G4R_MUTATE == 24      // test build: from the second update on, the similarity to the LAST pick alone
            mj = sim;
#else
            mj = (t == 1 || sim > mj) ? sim : mj;
#endif
            v = lr - mmr_mul(mu, mj);
        }
        const unsigned long long key = free_ ? topk_key(v, (unsigned)tid) : 0ull;
        unsigned long long best = key;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned lo = __shfl_xor((unsigned)best, o), hi = __shfl_xor((unsigned)(best >> 32), o);
            const unsigned long long x = ((unsigned long long)hi << 32) | lo;
            best = x > best ? x : best;
        }
        if (lane == 0) s_best[wid] = best;      // (the last round's were read in front of the barrier that ended it)
        __syncthreads();
        best = max(max(s_best[0], s_best[1]), max(s_best[2], s_best[3]));
        if (free_ && key == best) {      // the keys of a row are distinct and a free position's is never 0: exactly one thread
            free_ = false;
            s_last = tid;
            out_pos[t] = tid;
            out_val[t] = v;
            if (out_cols) out_cols[row * k + t] = col;
            if (out_rel) out_rel[row * k + t] = s;
        }
        __syncthreads();
    }
}

template __global__ void k_mmr_rerank<false>(const float*, int, int, const int*, const float*, const int*, long long, const float*, int, int, float, int, int*, float*, int*, float*);
template __global__ void k_mmr_rerank<true>(const float*, int, int, const int*, const float*, const int*, long long, const float*, int, int, float, int, int*, float*, int*, float*);

// Item-index (IVF) kernels (gfx950), behind g4r_ivf_assign / g4r_ivf_set / g4r_recommend_sessions_ivf (not in the reference).
//   k_ivf_assign   the best list of every item: argmax over the lists of v.c - |c|^2 / 2 in fp32, v = [Wy[i], By[i]]
//   k_ivf_tab      the index's bf16 table in LIST order (k_wy_bf16's fragment layout), By and the item of every position
//   k_ivf_probe    a row's centroid scores fl32(h.c_w + c_b) as (score bits, list) entries; the unchanged k_topk_merge then
//                  returns the row's nprobe best lists, best first, equal scores by the lower list
//   k_ivf_mark / k_ivf_group / k_ivf_place   a chunk's (list, row, slot) triples counting-sorted by list, then row, into work
//                  items of one list and at most 32 of the rows that probe it; no host synchronisation
//   k_ivf_scan     one wave per work item: k_scan_bf16's stage 1 over the list's blocks, for the rows of the work item
//   k_ivf_pack     k_scan_pack for rows that may hold fewer than k candidates
// Contract of a row.  Its probes are the nprobe lists with the largest centroid score.  The approximate score of an eligible item
// of a probed list is the one stated at the top of g4r_scan_kernels.cuh (the same MFMA, the same k order, + By, the final activation
// in fp32); the exclusions apply here.  The row's candidates are the c best approximate scores in topk_key(score, ITEM INDEX)
// order: the "column" of every list entry is the item index, never the position in a list, so k_scan_merge runs with item_idx = NULL
// and the tie rule of the exact call (the lower item first) holds.  Stage 2 is the bf16 scan's.  Nothing a row receives depends on
// the rows it shares a chunk or a work item with: an MFMA output column depends on its own B column only.
//
// Index table: list l is the blocks [blk[l], blk[l + 1]) of 32 positions; position 32 b + r holds item pos_item[32 b + r], -1 on the
// pads that fill a list's last block; the lists hold their items in ascending item index.  The 16-byte unit
// ((b * KS + ks) * 2 + half) * 32 + r holds Wy[pos_item[32 b + r]][16 ks + 8 half .. + 8) as bf16 (zeros on pads and past Dtop).
#pragma once
#include "g4r_scan_kernels.cuh"

#define IVF_SMEM (SCN_SMEM + 4 * 64 * 4 + SC_BM * 4)      // + the tile's items per wave, + every row's output list
static_assert(IVF_SMEM <= 156 * 1024, "index scan LDS over the 156 KiB a kernel may ask for");
#define IVF_AC 32        // centroids per LDS chunk of k_ivf_assign
#define IVF_AK 32        // item-vector elements held in registers at a time
#define IVF_PR 16        // rows per workgroup of k_ivf_probe

// One thread per item.  cen: [nl][W] centroids (W = Dtop + 1: the last element pairs with By), hn[l] = |c_l|^2 / 2.  Per chunk of
// IVF_AC centroids (staged in LDS, read as broadcasts) the dot products run over ascending k, one fp32 FMA chain each from zero;
// J = dot - hn, and a list replaces the best so far only when its J is greater: equal objectives go to the lower list.
__global__ __launch_bounds__(256) void k_ivf_assign(const DevModel* __restrict__ mp, const float* cen, const float* hn, int nl, int* out) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const DevModel& m = *mp;
    const int D = m.Dtop, W = D + 1, tid = threadIdx.x;
    const long long item = (long long)blockIdx.x * 256 + tid;
    const bool on = item < m.n_items;
    const float* wy = m.Wy + (size_t)(on ? item : 0) * D;
    const float by = m.By[on ? item : 0];
    float best = 0.f;
    int bl = -1;
    for (int c0 = 0; c0 < nl; c0 += IVF_AC) {
        const int nc = min(IVF_AC, nl - c0);
        __syncthreads();
        // (IVF_AK floats of slack behind the chunk, zero like the rows of the centroids past nl: the last k-group of a row reads on into
        // what follows it, against elements of v that are zero)
        for (int e = tid; e < IVF_AC * W + IVF_AK; e += 256) smem[e] = e < nc * W ? cen[(size_t)c0 * W + e] : 0.f;
        __syncthreads();
        float acc[IVF_AC];
#pragma unroll
        for (int c = 0; c < IVF_AC; ++c) acc[c] = 0.f;
        for (int k0 = 0; k0 < W; k0 += IVF_AK) {
            float v[IVF_AK];
#pragma unroll
            for (int j = 0; j < IVF_AK; ++j) v[j] = k0 + j < D ? wy[k0 + j] : (k0 + j == D ? by : 0.f);
#pragma unroll
            for (int c = 0; c < IVF_AC; ++c) {
                const float* cr = smem + c * W + k0;
                float a = acc[c];
#pragma unroll
                for (int j = 0; j < IVF_AK; ++j) a = fmaf(v[j], cr[j], a);      // (finite centroids: 0 * c adds nothing)
                acc[c] = a;
            }
        }
#pragma unroll
        for (int c = 0; c < IVF_AC; ++c) {
            const float J = acc[c] - hn[min(c0 + c, nl - 1)];
            if (c < nc && (bl < 0 || J > best)) { best = J; bl = c0 + c; }
        }
    }
    if (on) out[item] = bl;
}

// one thread per 16-byte unit of the index table (k_wy_bf16 with the item read from pos_item); the threads of half 0, k-step 0 also
// store By by position
__global__ __launch_bounds__(256) void k_ivf_tab(const DevModel* __restrict__ mp, const int* pos_item, uint4* tab, float* pos_by, long long nblk, int KS) {
    const DevModel& m = *mp;
    const long long u = (long long)blockIdx.x * 256 + threadIdx.x;
    if (u >= nblk * KS * 64) return;
    const int r = (int)(u & 31), half = (int)((u >> 5) & 1);
    const long long bk = u >> 6, blk = bk / KS;
    const int ks = (int)(bk - blk * KS), D = m.Dtop, k0 = 16 * ks + 8 * half;
    const int item = pos_item[blk * 32 + r];
    unsigned short v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (item >= 0 && k0 + j < D) ? bf16_rne(m.Wy[(size_t)item * D + k0 + j]) : (unsigned short)0;
    tab[u] = make_uint4(v[0] | ((unsigned)v[1] << 16), v[2] | ((unsigned)v[3] << 16), v[4] | ((unsigned)v[5] << 16), v[6] | ((unsigned)v[7] << 16));
    if (ks == 0 && half == 0) pos_by[blk * 32 + r] = item >= 0 ? m.By[item] : 0.f;
}

// Workgroup (blockIdx.x, blockIdx.y) = 256 lists x IVF_PR rows (staged in LDS); a thread owns one list: one fp32 FMA chain over
// ascending k from zero per (row, list), then + c_b -- a function of the row's own h only.  cwt: [D][nl] (transposed: consecutive threads
// read consecutive floats), cb: [nl].  ent[row * Lp + l] = (score bits, l); positions [nl, Lp) hold the pad k_topk_merge ignores.
__global__ __launch_bounds__(256) void k_ivf_probe(const float* h, int mrows, int D, const float* cwt, const float* cb, int nl, int Lp, uint2* ent) {
    extern __shared__ __attribute__((aligned(16))) float sh[];
    const int tid = threadIdx.x, r0 = blockIdx.y * IVF_PR, l = blockIdx.x * 256 + tid;
    for (int e = tid; e < IVF_PR * D; e += 256) {
        const int r = e / D;
        sh[e] = r0 + r < mrows ? h[(size_t)(r0 + r) * D + (e - r * D)] : 0.f;
    }
    __syncthreads();
    if (l >= Lp) return;
    if (l < nl) {
        float acc[IVF_PR];
#pragma unroll
        for (int r = 0; r < IVF_PR; ++r) acc[r] = 0.f;
        for (int k = 0; k < D; ++k) {
            const float c = cwt[(size_t)k * nl + l];
#pragma unroll
            for (int r = 0; r < IVF_PR; ++r) acc[r] = fmaf(sh[r * D + k], c, acc[r]);
        }
        const float b = cb[l];
#pragma unroll
        for (int r = 0; r < IVF_PR; ++r)
            if (r0 + r < mrows) ent[(size_t)(r0 + r) * Lp + l] = make_uint2(__float_as_uint(acc[r] + b), (unsigned)l);
    } else {
        for (int r = 0; r < IVF_PR; ++r)
            if (r0 + r < mrows) ent[(size_t)(r0 + r) * Lp + l] = make_uint2(0u, 0xFFFFFFFFu);
    }
}

// ---- grouping: a chunk's T = rows * np triples (list = probes[row * np + slot], row, slot) -> work items ----------------------
// member[l * MW + (row >> 5)] bit (row & 31): row probes list l (a row probes a list at most once).  Zeroed on the stream first.
__global__ __launch_bounds__(256) void k_ivf_mark(const int* probes, int T, int np, int MW, unsigned* member) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    const int row = t / np;
    atomicOr(member + (size_t)probes[t] * MW + (row >> 5), 1u << (row & 31));
}
// ONE workgroup of 1024 threads; thread t owns a contiguous stretch of lists.  cnt[l] = the rows that probe l (a popcount); exclusive
// sums over the lists of cnt -> toff[l], the list's first triple, and of ceil(cnt / 32) -> its first work item.  work[w] = (list,
// first triple, rows <= 32, -); *n_work = their number, at most T.
__global__ __launch_bounds__(1024) void k_ivf_group(const unsigned* member, int nl, int MW, int* toff, int4* work, int* n_work) {
    __shared__ int s_t[1024], s_w[1024];
    const int tid = threadIdx.x, per = (nl + 1023) / 1024, l0 = min(tid * per, nl), l1 = min(l0 + per, nl);
    int ct = 0, cw = 0;
    for (int l = l0; l < l1; ++l) {
        int c = 0;
        for (int w = 0; w < MW; ++w) c += __popc(member[(size_t)l * MW + w]);
        ct += c;
        cw += (c + 31) >> 5;
    }
    s_t[tid] = ct; s_w[tid] = cw;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const int a = tid >= o ? s_t[tid - o] : 0, b = tid >= o ? s_w[tid - o] : 0;
        __syncthreads();
        s_t[tid] += a; s_w[tid] += b;
        __syncthreads();
    }
    int t = s_t[tid] - ct, w = s_w[tid] - cw;
    for (int l = l0; l < l1; ++l) {
        int c = 0;
        for (int x = 0; x < MW; ++x) c += __popc(member[(size_t)l * MW + x]);
        toff[l] = t;
        for (int j = 0; j < c; j += 32) work[w++] = make_int4(l, t + j, min(32, c - j), 0);
        t += c;
    }
    if (tid == 1023) *n_work = s_w[1023];
}
// triple (row, slot) of list l goes to trip[toff[l] + (the rows below `row` that probe l)] as row * 256 + slot: sorted by list, then row
__global__ __launch_bounds__(256) void k_ivf_place(const int* probes, int T, int np, int MW, const unsigned* member, const int* toff, int* trip) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    const int row = t / np, slot = t - row * np, l = probes[t];
    const unsigned* mw = member + (size_t)l * MW;
    int rank = __popc(mw[row >> 5] & ((1u << (row & 31)) - 1u));
    for (int w = 0; w < (row >> 5); ++w) rank += __popc(mw[w]);
    trip[toff[l] + rank] = row * 256 + slot;
}

// The views of the index a scan reads (device pointers)
struct IvfTab {
    const uint4* tab;          // the bf16 table, list order
    const float* pos_by;       // By by position
    const int* pos_item;       // item by position, -1 on pads
    const int* blk;            // [nl + 1] list l = blocks [blk[l], blk[l + 1])
    const int* offs;           // [nl + 1] list l = entries [offs[l], offs[l + 1]) of the index's item order (its length)
};

// Stage 1 over an index.  One wave per work item (list, first triple, rows): lane l serves row slot l & 31 -- the row and probe slot
// of triple first + (l & 31) -- and the wave walks the list's blocks two at a time as k_scan_bf16 walks a column range: the rows'
// h as the bf16 B operand in registers, the blocks' fragments streamed as A, wave-private survivor queues, thresholds and merges
// (topk_merge_row with the exclusions of each lane's own row).  The waves of a workgroup never meet.  Entries are (score bits, ITEM).
// Output: ws[(row * np + slot) * c + j], unused entries (0, 0xFFFFFFFF).  Waves past *n_work leave.
template <int NCH>
__global__ __launch_bounds__(256) void k_ivf_scan(const DevModel* __restrict__ mp, const float* h, IvfTab ix, const int4* work, const int* n_work,
                                                  const int* trip, int np, int c, uint2* ws, TkExcl ex) {
    constexpr int KS = 4 * NCH;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const DevModel& m = *mp;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, r32 = lane & 31, half = lane >> 5;
    const int wi = blockIdx.x * 4 + wid;
    if (wi >= *n_work) return;      // (no workgroup barrier anywhere below)
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
    int* s_it = reinterpret_cast<int*>(reinterpret_cast<char*>(smem) + SCN_SMEM) + wid * 64;
    int* s_dst = reinterpret_cast<int*>(reinterpret_cast<char*>(smem) + SCN_SMEM + 4 * 64 * 4);

    const int4 wk = work[wi];
    const int list = wk.x, nrow = wk.z;
    const bool on = r32 < nrow;
    const int tr = trip[wk.y + (on ? r32 : 0)];
    const int grow = tr >> 8, slot = tr & 255;                  // this lane's row of the chunk and its probe slot
    const int lrow = 32 * wid + r32;
    if (half == 0) {
        s_qn[lrow] = 0; s_ln[lrow] = 0; s_thr[lrow] = 0ull;
        s_dst[lrow] = grow * np + slot;
        const bool xon = ex.offs && on;
        const long long b = xon ? ex.offs[grow] : 0ll;
        s_xb[lrow] = b;
        s_xn[lrow] = xon ? (int)(ex.offs[grow + 1] - b) : 0;
    }
    const int D = m.Dtop;
    bf16x8 hb[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int kk = 16 * ks + 8 * half + j;
            hb[ks][j] = (short)((on && kk < D) ? bf16_rne(h[(size_t)grow * D + kk]) : (unsigned short)0);
        }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();

    const int b0 = ix.blk[list];
#if defined(G4R_MUTATE) && G4R_MUTATE == 31      // test build: the last block of a list whose length is no multiple of 32 is not scanned
    const int b1 = ix.blk[list + 1] - (((ix.offs[list + 1] - ix.offs[list]) & 31) ? 1 : 0);
#else
    const int b1 = ix.blk[list + 1];
#endif
    auto out_list = [&](int r) { return ws + (size_t)s_dst[r] * c; };
    auto merge_mine = [&]() {
        for (int r = 32 * wid; r < 32 * wid + nrow; ++r)
            if (s_qn[r] > 0) topk_merge_row<true>(r, out_list(r), c, s_q + r * TK_Q, skq, sl, s_qn, s_ln, s_thr, s_xb[r], s_xn[r], nullptr, ex, sx);
    };
    // fragment f of the tile at block b is block b + f; past the list's end the last block is read again and its items are -1
    auto tile_items = [&](int b, int (&it)[2]) {
#pragma unroll
        for (int f = 0; f < 2; ++f) it[f] = b + f < b1 ? ix.pos_item[(size_t)(b + f) * 32 + r32] : -1;
    };
    auto load_chunk = [&](int b, int ch, bf16x8 (&w)[4][2]) {
#pragma unroll
        for (int f = 0; f < 2; ++f) {
            const int bb = min(b + f, b1 - 1);
            const uint4* p = ix.tab + ((size_t)bb * KS + 4 * ch) * 64 + 32 * half + r32;
#pragma unroll
            for (int s = 0; s < 4; ++s) w[s][f] = __builtin_bit_cast(bf16x8, p[64 * s]);
        }
    };

    bf16x8 w[2][4][2];
    int it[2], itn[2];
    tile_items(b0, it);
    if (b0 < b1) load_chunk(b0, 0, w[0]);
    for (int b = b0; b < b1; b += 2) {
        const int bi = half ? it[1] : it[0];            // the item of position 32 b + lane
        const float by = bi >= 0 ? ix.pos_by[(size_t)min(b + half, b1 - 1) * 32 + r32] : 0.f;
        tile_items(b + 2, itn);
        f32x16 acc[2];
#pragma unroll
        for (int f = 0; f < 2; ++f)
#pragma unroll
            for (int j = 0; j < 16; ++j) acc[f][j] = 0.f;
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
            if (ch + 1 < NCH) load_chunk(b, ch + 1, w[(ch + 1) & 1]);
            else if (b + 2 < b1) load_chunk(b + 2, 0, w[0]);      // (NCH is even: the next tile starts in w[0] again)
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int f = 0; f < 2; ++f)
                    acc[f] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[ch & 1][s][f], hb[4 * ch + s], acc[f], 0, 0, 0);
        }
        s_by[lane] = by;
        s_it[lane] = bi;
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
        // accumulator register j of fragment f: position 32 (b + f) + (j & 3) + 8 (j >> 2) + 4 half, row = this lane's
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
                    const int item = s_it[32 * f + (j & 3) + 8 * (j >> 2) + 4 * half];
                    if (on && item >= 0 && !(v[j] < tf) && topk_key(v[j], (unsigned)item) > t) {
                        const int p = atomicAdd(s_qn + lrow, 1);
                        s_q[lrow * TK_Q + p] = make_uint2(__float_as_uint(v[j]), (unsigned)item);
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                __builtin_amdgcn_wave_barrier();
                if (__any(s_qn[lrow] > TK_Q - 32)) merge_mine();
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();      // the tile's s_by / s_it reads done before the next tile writes them
        it[0] = itn[0]; it[1] = itn[1];
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    merge_mine();
    for (int r = 32 * wid; r < 32 * wid + nrow; ++r) {
        uint2* L = out_list(r);
        for (int j = s_ln[r] + lane; j < c; j += 64) L[j] = make_uint2(0u, 0xFFFFFFFFu);
    }
}

// k_scan_pack for rows that may hold fewer than k real candidates.  k_topk_merge returns exactly k entries and takes every key of
// the row as distinct, so the places past cnt[r] are not pads here: place j holds (NaN, column 0x80000000 + j) -- keys that are
// distinct, below every real entry's (NaN last, and a real NaN's lower column first) and never a real column (those are < 2^31).
// The entries a row returns at and after min(cnt[r], k) are then these: score NaN, a negative column.
__global__ __launch_bounds__(256) void k_ivf_pack(const float* sc, const int* cols, const int* cnt, int c, int L, uint2* ws) {
    const int j = blockIdx.x * 256 + threadIdx.x, r = blockIdx.y;
    if (j >= L) return;
    ws[(size_t)r * L + j] = j < cnt[r] ? make_uint2(__float_as_uint(sc[(size_t)r * c + j]), (unsigned)cols[(size_t)r * c + j])
                                       : make_uint2(0x7FC00000u, 0x80000000u + (unsigned)j);
}

#define IVF_FORMS(F) F(2) F(4) F(8)
#define IVF_INSTANTIATE(NCH) \
    template __global__ void k_ivf_scan<NCH>(const DevModel*, const float*, IvfTab, const int4*, const int*, const int*, int, int, uint2*, TkExcl);
IVF_FORMS(IVF_INSTANTIATE)
#undef IVF_INSTANTIATE

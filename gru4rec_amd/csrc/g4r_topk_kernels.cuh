// Top-K next-item recommendation kernels (gfx950), behind g4r_recommend_step (not in the reference).
//   k_topk_range   ONE kernel template, k_topk_range<STORED, EXCL, X...>: the k best of a column range per row.  Its thirteen
//                  instantiations ("forms") are listed once, by name, in TK_FORMS below
//   k_topk_merge   the ranges' lists of one row -> the row's k best (int32 column, float score)
//   k_events_merge k_topk_merge writing its row, the row's rank and target score at the event's place in the call's output
// A form is three things.  STORED: the scores are read from a matrix already in memory (softmax / softmax_logit final activations)
// instead of being computed tile by tile as k_score_all computes them (fused: nothing stored).  EXCL: excluded items are dropped where
// a survivor queue is merged into its row's list (topk_merge_row): a global bit mask over item indices and a sorted per-row list (at
// most G4R_EXCLUDE_MAX items); the EXCL = false forms without a trailing argument are the unfiltered kernels, instruction for
// instruction.  X: the type of the ONE trailing kernel argument (none for the two unfiltered forms), which says what else the scan
// does -- rank counters (TkEvents), lists that grow between launches (TkGrow), a draw (TkSample), the row normaliser (Tk...Lse).
// What a trailing-argument type carries is stated once, in its description TkForm<X> next to the structs; the kernel reads its
// constexpr flags and its views from there, and the dynamic LDS of a form (tk_smem) follows from the same flags.
// To add a form: (1) a struct for the trailing argument with its TkForm specialisation (only what the type HAS; a type that pairs an
// existing one with the row normaliser derives from TkFormLse), (2) one line in TK_FORMS -- the explicit instantiation, the host-side
// name and the LDS opt-in at create all come from that line, (3) one tk_launch call (g4r_host_topk.hpp).  A launch of a form that
// is not in TK_FORMS has no device code: the build refuses the library (build.py, kernels_without_device_code).
//
// Order (the contract of g4r_recommend_step): score descending, equal scores (float ==, so -0.0 == +0.0) by the lower column,
// NaN below every number.  topk_key() maps (score, column) to one 64-bit key whose unsigned order IS that order; the keys of one
// row are distinct (columns are), so "the k best" is exactly the k largest keys.  Key 0 is never a real entry's: it pads.
#pragma once
#include "g4r_eval_kernels.cuh"

#define TK_MAX G4R_TOPK_MAX      // largest k
#define TK_Q 64          // survivor queue per row (LDS); merged into the row's list once any row holds more than TK_Q - 32
#define TK_TN 32         // columns per tile (as k_score_all<32>): a tile adds at most 32 survivors per row

__device__ __forceinline__ unsigned long long topk_key(float v, unsigned col) {
    unsigned u = __float_as_uint(v);
    if ((u << 1) == 0u) u = 0u;                                       // -0.0 -> +0.0
    const unsigned s = (v != v) ? 1u : ((u & 0x80000000u) ? ~u : (u | 0x80000000u));   // NaN 1, -inf 0x007FFFFF, +inf 0xFF800000
#if defined(G4R_MUTATE) && G4R_MUTATE == 7      // test build: equal scores broken by the HIGHER column
    const unsigned c = col;
#else
    const unsigned c = ~col;
#endif
    return ((unsigned long long)s << 32) | c;
}
// (score bits, column) as stored in the lists; column 0xFFFFFFFF pads a list (columns are < 2^31) and keys 0
__device__ __forceinline__ unsigned long long topk_key(uint2 e) { return e.y == 0xFFFFFFFFu ? 0ull : topk_key(__uint_as_float(e.x), e.y); }

// ---- the parts a trailing argument can carry: five plain structs of device pointers and scalars -------------------------------
// Exclusions of one g4r_recommend_step_filtered call (device pointers, NULL = none): row r's sorted, duplicate-free item indices are
// items[offs[r] .. offs[r + 1]), at most G4R_EXCLUDE_MAX of them; bit (i & 31) of mask[i >> 5] excludes item index i in every row.
struct TkExcl { const long long* offs; const int* items; const unsigned* mask; };

// The trailing argument of the g4r_recommend_events forms (k_topk_range<.., .., TkEvents>), one evaluation step's rows.
// Rank counters (fused form only): tscore[r] is row r's target score (k_score_cand: g4r_predict_step's bit pattern); every column
// of the range whose score is greater / equal adds to cnt[2 r] / cnt[2 r + 1] -- excluded columns too: exclusions shape the list,
// never the rank.  tie_col != NULL ('tiebreaking'): score (r, n) is moved by tie_noise(r, n + col_off) and the target's by
// tie_noise(r, tie_col[r]) for the comparison only (k_score_all's keys: col_off = the number of target columns g4r_evaluate puts
// in front of `items`).  Exclusions (EXCL): seen[r] = (begin, length, position, -): the row's session list is the sorted distinct
// items s_items[begin .. begin + length), s_first[begin + j] the position in the session of item j's first occurrence; an item is
// excluded iff it is found there with s_first <= position (the input event's position).  One pair of arrays per call serves every
// event of a session.  mask: TkExcl's.  seen == NULL: no lists.
struct TkEvents {
    const float* tscore; int* cnt; const int* tie_col; long long col_off; unsigned tie_ctr;
    const int4* seen; const int* s_items; const int* s_first; const unsigned* mask;
};

// The trailing argument of the g4r_continue_sessions forms (k_topk_range<.., true, TkGrow>, k_scan_bf16<.., TkGrow>): TkExcl whose
// per-row lists GROW on the device between launches.  Row r's sorted, duplicate-free list is items[beg[r] .. beg[r] + len[r]); the
// host leaves slack behind every list, k_rollout_feed (g4r_rollout_kernels.cuh) inserts into it and bumps len[r].  A type of its
// own -- as every one below -- so that the forms that exist keep their kernel arguments and their code.
struct TkGrow { const long long* beg; const int* len; const int* items; const unsigned* mask; };

// The trailing argument of the g4r_sample_sessions form (k_topk_range<false, true, TkSample>): TkGrow's fields, plus what turns the
// selection into a draw.  Row r of the launch is the draw with row id row_id[r]; the value pushed to a row's queue, compared with
// its threshold and kept in the lists is key = fl32(fl32(z * invT) + gumbel_noise(seed, row id, step, item)) in place of the score z:
// the argmax of the keys over the eligible columns is a draw from softmax(z / T) over them (Gumbel-max), and the threshold, queue
// and merge logic are the selection's own.
// (Every score gets its noise.  Skipping the Philox call and the logarithms of a score whose key cannot beat its row's threshold
// whatever the noise -- g < 17 -- gives the same results and was measured: it does not pay, profiles/sample_sessions.md.)
struct TkSample {
    const long long* beg; const int* len; const int* items; const unsigned* mask;
    const unsigned* row_id; unsigned long long seed; unsigned step; float invT;
};

// The row normaliser of g4r_sample_sessions_lp / g4r_session_log_partition: Q[row] = the sum over the row's ELIGIBLE candidate positions
// of q = lse_term(z, zeta[row * zs], invT), an exact 64-bit integer -- every term is a function of the term alone and integer adds
// commute, so Q has the same bits however the columns are cut into ranges and whatever order the workgroups finish in.  zeta: the
// largest eligible z of the row (the exact selection's top-1), so that every term is at most 2^39; Q is zeroed on the stream first.
// Never a trailing argument itself: it rides with another one (TkSampleLse, TkGrowLse, TkEventsLse).
struct TkLse { const float* zeta; int zs; unsigned long long* Q; float invT; };
// q of one score: d = fl32(fl32(z - zeta) * invT) (two roundings, no FMA), q = rn(2^39 * expf(d)) (the library's expf; the product
// with a power of two is exact); NaN gives 0
__device__ __forceinline__ unsigned long long lse_term(float z, float zeta, float invT) {
    const float d = __fmul_rn(__fsub_rn(z, zeta), invT);
    if (d != d) return 0ull;
    return __float2ull_rn(0x1p39f * expf(d));
}
// The log-probability softmax(z * invT) over a row's eligible positions gives the position with logit z: fl32((double)d - log((double)Q
// * 2^-39)), d = fl32(fl32(z - zeta) * invT) (two roundings, no FMA); zeta and the integer Q: the row's normaliser (TkLse).  The one
// expression behind k_sample_logprob and k_audience_keys: the same (z, zeta, Q, invT) give the same bits in either.
__device__ __forceinline__ float lse_logprob(float z, float zeta, unsigned long long Q, float invT) {
    const float d = __fmul_rn(__fsub_rn(z, zeta), invT);
    return (float)((double)d - log((double)Q * 0x1p-39));
}

// ---- one description per trailing-argument pack: TkForm<X...> -----------------------------------------------------------------
// k_topk_range, and k_scan_bf16 for its one argument, ask a pack four yes/no questions (constexpr flags) and five views:
//   EV    TkEvents' rows: session-list exclusions with positions; rank counters in the fused form without LSE
//   GROW  the rows' lists are (begin, length) pairs that may grow between launches, staged by row_list
//   SMP   the value selected on is the draw's key
//   LSE   the scan also forms the row normaliser Q
//   excl(x) / events(x) / grow(x) / sample(x) / lse(x)   the part as its own struct
// TkFormNone answers "no such part" to everything: every flag false, every view the all-NULL struct.  It is the whole description of
// the empty pack (the unfiltered forms take no trailing argument) and the base of every other one, which states only what it has.
template <typename... X> struct TkFormNone {
    static constexpr bool EV = false, GROW = false, SMP = false, LSE = false;
    static __device__ __forceinline__ TkExcl excl(X...) { return TkExcl{}; }
    static __device__ __forceinline__ TkEvents events(X...) { return TkEvents{}; }
    static __device__ __forceinline__ TkGrow grow(X...) { return TkGrow{}; }
    static __device__ __forceinline__ TkSample sample(X...) { return TkSample{}; }
    static __device__ __forceinline__ TkLse lse(X...) { return TkLse{}; }
    // (GROW) row `row`'s list start and length, 0 and 0 for a row past the call's, as the range kernels stage them
    static __device__ __forceinline__ void row_list(const TkGrow& g, int row, int mrows, long long& b, int& n) {
        const bool on = row < mrows;
        b = on ? g.beg[row] : 0ll;
        n = on ? g.len[row] : 0;
    }
};
template <typename... X> struct TkForm : TkFormNone<X...> {};
template <> struct TkForm<TkExcl> : TkFormNone<TkExcl> {
    static __device__ __forceinline__ TkExcl excl(TkExcl e) { return e; }
};
template <> struct TkForm<TkEvents> : TkFormNone<TkEvents> {
    static constexpr bool EV = true;
    static __device__ __forceinline__ TkExcl excl(TkEvents e) { return TkExcl{nullptr, e.s_items, e.mask}; }
    static __device__ __forceinline__ TkEvents events(TkEvents e) { return e; }
};
template <> struct TkForm<TkGrow> : TkFormNone<TkGrow> {
    static constexpr bool GROW = true;
    static __device__ __forceinline__ TkExcl excl(TkGrow g) { return TkExcl{nullptr, g.items, g.mask}; }
    static __device__ __forceinline__ TkGrow grow(TkGrow g) { return g; }
};
template <> struct TkForm<TkSample> : TkFormNone<TkSample> {
    static constexpr bool GROW = true, SMP = true;
    static __device__ __forceinline__ TkExcl excl(TkSample s) { return TkExcl{nullptr, s.items, s.mask}; }
    static __device__ __forceinline__ TkGrow grow(TkSample s) { return TkGrow{s.beg, s.len, s.items, s.mask}; }
    static __device__ __forceinline__ TkSample sample(TkSample s) { return s; }
};
// The description of a type C = { A a; TkLse l; } that pairs another trailing argument with the row normaliser: A's own, through a,
// plus LSE.  (The fused EXCL forms only, as k_topk_range asserts.)
template <typename C, typename A> struct TkFormLse : TkForm<A> {
    static constexpr bool LSE = true;
    static __device__ __forceinline__ TkExcl excl(const C& x) { return TkForm<A>::excl(x.a); }
    static __device__ __forceinline__ TkEvents events(const C& x) { return TkForm<A>::events(x.a); }
    static __device__ __forceinline__ TkGrow grow(const C& x) { return TkForm<A>::grow(x.a); }
    static __device__ __forceinline__ TkSample sample(const C& x) { return TkForm<A>::sample(x.a); }
    static __device__ __forceinline__ TkLse lse(const C& x) { return x.l; }
};
// TkSampleLse = TkSample's draw plus the sum (g4r_sample_sessions_lp).  TkGrowLse = TkGrow's selection (launched with k = 1) plus the
// sum (top_p, g4r_session_log_partition).  Eligibility is decided per score: per tile every row's 32-bit word of the columns its own
// list takes and the word of the columns the global mask takes.
struct TkSampleLse { TkSample a; TkLse l; };
template <> struct TkForm<TkSampleLse> : TkFormLse<TkSampleLse, TkSample> {};
struct TkGrowLse { TkGrow a; TkLse l; };
template <> struct TkForm<TkGrowLse> : TkFormLse<TkGrowLse, TkGrow> {};
// TkEventsLse (g4r_loglik_events): the row normaliser under TkEvents' eligibility.  The rows' lists are the SESSION-level ones (seen /
// s_items / s_first), so the per-tile word of a row marks a column only when its item is found in the session list with s_first <=
// the row's position; the mask as before.  No rank counters (tscore / cnt / tie_col are not read); launched with k = 1, its lists unused.
struct TkEventsLse { TkEvents a; TkLse l; };
template <> struct TkForm<TkEventsLse> : TkFormLse<TkEventsLse, TkEvents> {};

// ---- the forms, once -----------------------------------------------------------------------------------------------------------
// F(host-side name, STORED, EXCL[, trailing-argument type]).  The explicit instantiations (TK_INSTANTIATE, after the kernel), the
// host's names (g4r_host_model.hpp) and the LDS opt-in at create (g4r_host_create.hpp) are this list and nothing else.
//   k_topk_fused / k_topk_stored       scores selected as they are produced (element-wise final activation) / out of p_scores (softmax)
//   k_topk_fused_x / k_topk_stored_x   the same two with exclusions (g4r_recommend_step_filtered)
//   k_topk_fused_g / k_topk_stored_g   the same two with lists that grow on the device (g4r_continue_sessions)
//   k_topk_rank / k_topk_rank_x        g4r_recommend_events: k_topk_fused + the rank counters of k_score_count / + its exclusions
//   k_topk_stored_ev                   softmax / softmax_logit with those exclusions (no counters)
//   k_topk_events_q                    g4r_loglik_events: the row normaliser Q under those exclusions (k = 1)
//   k_topk_sample                      selection on the Gumbel-perturbed key (g4r_sample_sessions)
//   k_topk_sample_q / k_topk_fused_q   the same draw + Q (g4r_sample_sessions_lp) / k_topk_fused_g + Q (launched with k = 1)
#define TK_FORMS(F)                                \
    F(k_topk_fused, false, false)                  \
    F(k_topk_stored, true, false)                  \
    F(k_topk_fused_x, false, true, TkExcl)         \
    F(k_topk_stored_x, true, true, TkExcl)         \
    F(k_topk_fused_g, false, true, TkGrow)         \
    F(k_topk_stored_g, true, true, TkGrow)         \
    F(k_topk_rank, false, false, TkEvents)         \
    F(k_topk_rank_x, false, true, TkEvents)        \
    F(k_topk_stored_ev, true, true, TkEvents)      \
    F(k_topk_events_q, false, true, TkEventsLse)   \
    F(k_topk_sample, false, true, TkSample)        \
    F(k_topk_sample_q, false, true, TkSampleLse)   \
    F(k_topk_fused_q, false, true, TkGrowLse)

// ---- LDS of a form, from the flags the kernel carves it by ---------------------------------------------------------------------
// [queues | queue counts | list lengths | thresholds | (EXCL) list starts, lengths | (EXCL, EV) positions | tail]; the tail is the
// four waves' merge scratch (STORED) or the score tile [A | B | the tile's items | (LSE) the rows' words, the mask's word] (fused),
// whose A tile the merge scratch aliases: a merge runs between the last read of one tile and the first write of the next.
#define TK_SCRATCH_WAVE (TK_MAX * 8 + TK_Q * 8)          // bytes: a copy of the row's list + the sorted queue keys
#define TK_SCRATCH_WAVE_X (TK_SCRATCH_WAVE + G4R_EXCLUDE_MAX * 4)   // EXCL: + the row's sorted exclusion list
#define TK_SMEM_SEL (SC_BM * TK_Q * 8 + SC_BM * 4 * 2 + SC_BM * 8)
#define TK_SEL_X (SC_BM * 12)           // EXCL: + every row's list start (8 B) and length (4 B), staged once per workgroup
#define TK_SEL_EV (SC_BM * 4)           // EXCL with EV: + every row's position in its session
#define TK_TILE (((SC_BM + TK_TN) * (SC_KC + 2) + TK_TN) * 4)
#define TK_TILE_LSE ((SC_BM + 4) * 4)   // LSE: + per tile every row's word of the columns its list takes, and the global mask's word
static_assert(4 * TK_SCRATCH_WAVE_X <= SC_BM * (SC_KC + 2) * 4, "the EXCL merge scratch must fit in the fused kernel's A tile");
// bytes in front of the tail (k_topk_range finds its tail here)
constexpr size_t tk_smem_head(bool EXCL, bool EV) { return TK_SMEM_SEL + (EXCL ? TK_SEL_X + (EV ? TK_SEL_EV : 0) : 0); }
// The dynamic LDS of k_topk_range<STORED, EXCL, X...>, of a 160 KiB CU: stored 77,824 B, 95,744 B with EXCL, 96,256 B with TkEvents'
// positions; fused 150,912 B, 152,448 B with EXCL (the sampling form too: its row ids live in registers), 152,960 B with TkEvents'
// positions; with the row normaliser 152,976 B, TkEventsLse 153,488 B
template <bool STORED, bool EXCL, typename... X> constexpr size_t tk_smem() {
    using F = TkForm<X...>;
    constexpr size_t n = tk_smem_head(EXCL, F::EV) + (STORED ? 4 * (EXCL ? TK_SCRATCH_WAVE_X : TK_SCRATCH_WAVE) : TK_TILE + (F::LSE ? TK_TILE_LSE : 0));
    static_assert(n <= 156 * 1024, "top-k LDS over the 156 KiB the kernels may ask for");
    return n;
}

// One wave merges the survivor queue of local row r into the row's sorted list L (global, length n <= k): the queue is sorted in
// registers (bitonic over the 64 lanes), then every element's place in the union is its own index plus the number of elements of
// the other sequence above it (binary search), and the first k places are written.  The row's threshold becomes its k-th key.
// EXCL: every queue entry whose item (item_idx[column], or the column) is excluded -- its bit in ex.mask, or found by binary search
// in the row's list (staged in sx, loaded together with the list copy) -- becomes the pad (key 0) before the sort and is not
// counted in c.  The list then only ever holds eligible entries, so the threshold is an eligible key; an excluded item can still
// beat it, but enters the range's queue at most once (a range visits each column once): the queue bound (<= 32 per tile) holds.
// (xb, nx: the row's list is ex.items[xb .. xb + nx), read from LDS so that its load goes out together with the list copy)
// SEEN (TkEvents): an item found in the row's list is dropped only when first[xb + its place] <= pos
template <bool EXCL, bool SEEN = false>
__device__ __forceinline__ void topk_merge_row(int r, uint2* L, int k, uint2* sq, unsigned long long* skq, uint2* sl, int* s_qn,
                                               int* s_ln, unsigned long long* s_thr, long long xb = 0, int nx = 0,
                                               const int* item_idx = nullptr, TkExcl ex = TkExcl{}, int* sx = nullptr, const int* first = nullptr,
                                               int pos = 0) {
    const int lane = threadIdx.x & 63;
    int c = s_qn[r];
    const int n = s_ln[r];
    uint2 e;
    unsigned long long q;
    if constexpr (!EXCL) {
        for (int j = lane; j < n; j += 64) sl[j] = L[j];
        e = lane < c ? sq[lane] : make_uint2(0u, 0xFFFFFFFFu);
        q = lane < c ? topk_key(e) : 0ull;
    } else {
        e = lane < c ? sq[lane] : make_uint2(0u, 0xFFFFFFFFu);
        const int item = lane < c ? (item_idx ? item_idx[e.y] : (int)e.y) : 0;
        bool drop = lane < c && ex.mask && ((ex.mask[item >> 5] >> (item & 31)) & 1u);
        for (int j = lane; j < n; j += 64) sl[j] = L[j];
        for (int j = lane; j < nx; j += 64) sx[j] = ex.items[xb + j];
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (lane < c && !drop && nx > 0) {
#if defined(G4R_MUTATE) && G4R_MUTATE == 9      // test build: the search never matches the LAST item of the row's list
            const int hi = nx - 1;
#else
            const int hi = nx;
#endif
            int a = 0, b = hi;
            while (a < b) { const int mid = (a + b) >> 1; if (sx[mid] < item) a = mid + 1; else b = mid; }
            drop = a < hi && sx[a] == item;
            if constexpr (SEEN) drop = drop && first[xb + a] <= pos;
        }
        const bool keep = lane < c && !drop;
        c = __popcll(__ballot(keep));
        if (!keep) e = make_uint2(0u, 0xFFFFFFFFu);
        q = keep ? topk_key(e) : 0ull;
    }
#pragma unroll
    for (int w = 2; w <= 64; w <<= 1)
#pragma unroll
        for (int j = w >> 1; j > 0; j >>= 1) {
            const unsigned lo = __shfl_xor((unsigned)q, j), hi = __shfl_xor((unsigned)(q >> 32), j);
            const unsigned ex = __shfl_xor(e.x, j), ey = __shfl_xor(e.y, j);
            const unsigned long long o = ((unsigned long long)hi << 32) | lo;
            const bool desc = (lane & w) == 0, lower = (lane & j) == 0;
            if ((lower == desc) ? (o > q) : (o < q)) { q = o; e = make_uint2(ex, ey); }
        }
    skq[lane] = q;
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (int j = lane; j < n; j += 64) {
        const uint2 x = sl[j];
        const unsigned long long kx = topk_key(x);
        int a = 0, b = c;
        while (a < b) { const int mid = (a + b) >> 1; if (skq[mid] > kx) a = mid + 1; else b = mid; }
        const int pos = j + a;
        if (pos < k) L[pos] = x;
        if (pos == k - 1) s_thr[r] = kx;
    }
    if (lane < c) {
        int a = 0, b = n;
        while (a < b) { const int mid = (a + b) >> 1; if (topk_key(sl[mid]) > q) a = mid + 1; else b = mid; }
        const int pos = lane + a;
        if (pos < k) L[pos] = e;
        if (pos == k - 1) s_thr[r] = q;
    }
    if (lane == 0) { s_ln[r] = min(k, n + c); s_qn[r] = 0; }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// Stage 1.  Workgroup (blockIdx.x, blockIdx.y) = column range x 128-row block; the range is `tpr` tiles of 32 columns.  Per tile
// a score is pushed to its row's queue only when its key beats the row's threshold (the k-th key of the range's list so far:
// later columns lose every tie, so an equal score never gets in).  Output: ws[(row * gridDim.x + range) * k + j], the range's
// k best of the row in key order, entries past the range's column count padded with column 0xFFFFFFFF (key 0).
// STORED = false: the tile is computed as k_score_all computes it (one ascending-k fp32 MFMA chain from zero, + By, then the final
// activation), so every score is bit-identical to g4r_predict_step's.  STORED = true: the tile is read from `sc` (ldo floats per row).
// EXCL: the exclusions (the trailing argument's excl view and the rows' lists) apply at every merge (topk_merge_row), the per-wave
// scratch grows by the row's list (TK_SCRATCH_WAVE_X).  The unfiltered forms take no trailing argument, so their kernel arguments --
// and with them their code -- are those of the unfiltered kernel.  What else a form does is read from F = TkForm<X...>:
// EV (with EXCL) the rows' lists are the session lists with positions, (fused, no LSE) the rank counters; GROW the lists are
// (begin, length) pairs; SMP (fused, EXCL) the value selected on is the draw's key, see TkSample; LSE (fused, EXCL) the scan also adds
// every ELIGIBLE score's lse_term to the row's Q, see TkLse -- under EV with the session lists' eligibility (g4r_loglik_events).
template <bool STORED, bool EXCL, typename... X>
__global__ __launch_bounds__(256) void k_topk_range(const DevModel* __restrict__ mp, const float* h, int mrows, const int* item_idx,
                                                    long long n_sel, const float* sc, long long ldo, int k, int tpr, uint2* ws,
                                                    X... xs) {
    using F = TkForm<X...>;
    constexpr bool EV = F::EV;        // g4r_recommend_events: rank counters, session-list exclusions
    static_assert(sizeof...(X) == ((EXCL || EV) ? 1 : 0), "EXCL takes one trailing argument (its lists), an EV form its TkEvents, the unfiltered forms none");
    constexpr bool SMP = F::SMP;      // g4r_sample_sessions: keys in place of scores
    static_assert(!SMP || (EXCL && !STORED), "an SMP form is fused and takes its (possibly empty) lists");
    constexpr bool LSE = F::LSE;      // the row normaliser Q formed in the scan (TkLse)
    static_assert(!LSE || (EXCL && !STORED), "an LSE form is fused and takes its (possibly empty) lists");
    const TkExcl ex = F::excl(xs...);
    const TkEvents ev = F::events(xs...);
    const TkSample smp = F::sample(xs...);
    const TkLse lse = F::lse(xs...);
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, li = lane & 15, lg = lane >> 4;
    uint2* s_q = reinterpret_cast<uint2*>(smem);
    int* s_qn = reinterpret_cast<int*>(s_q + SC_BM * TK_Q);
    int* s_ln = s_qn + SC_BM;
    unsigned long long* s_thr = reinterpret_cast<unsigned long long*>(s_ln + SC_BM);
    long long* s_xb = reinterpret_cast<long long*>(s_thr + SC_BM);      // (EXCL only)
    int* s_xn = reinterpret_cast<int*>(s_xb + SC_BM);
    int* s_xp = s_xn + SC_BM;                                           // (EXCL with TkEvents only)
    char* tail = reinterpret_cast<char*>(smem) + tk_smem_head(EXCL, EV);
    float* sA = reinterpret_cast<float*>(tail);
    const int ldk = SC_KC + 2;
    float* sB = sA + SC_BM * ldk;
    int* sItem = reinterpret_cast<int*>(sB + TK_TN * ldk);
    unsigned* s_rowx = reinterpret_cast<unsigned*>(sItem + TK_TN);      // (LSE only) [SC_BM] the tile's columns taken by the row's list,
    unsigned* s_dropw = s_rowx + SC_BM;                                 // by the global mask
    char* scratch = tail + wid * (EXCL ? TK_SCRATCH_WAVE_X : TK_SCRATCH_WAVE);
    uint2* sl = reinterpret_cast<uint2*>(scratch);
    unsigned long long* skq = reinterpret_cast<unsigned long long*>(scratch + TK_MAX * 8);
    int* sx = reinterpret_cast<int*>(scratch + TK_SCRATCH_WAVE);

    const int rbase = blockIdx.y * SC_BM, range = blockIdx.x, R = gridDim.x;
    const long long c0 = (long long)range * tpr * TK_TN, c1 = min(n_sel, c0 + (long long)tpr * TK_TN);
    if (tid < SC_BM) { s_qn[tid] = 0; s_ln[tid] = 0; s_thr[tid] = 0ull; }
    if constexpr (EXCL && EV) {
        if (tid < SC_BM) {
            const int4 w = (ev.seen && rbase + tid < mrows) ? ev.seen[rbase + tid] : make_int4(0, 0, 0, 0);
            s_xb[tid] = w.x; s_xn[tid] = w.y; s_xp[tid] = w.z;
        }
    } else if constexpr (EXCL && F::GROW) {
        if (tid < SC_BM) {
            long long b;
            int n;
            F::row_list(F::grow(xs...), rbase + tid, mrows, b, n);
            s_xb[tid] = b;
            s_xn[tid] = n;
        }
    } else if constexpr (EXCL)
        if (tid < SC_BM) {
            const bool on = ex.offs && rbase + tid < mrows;
            const long long b = on ? ex.offs[rbase + tid] : 0ll;
            s_xb[tid] = b;
            s_xn[tid] = on ? (int)(ex.offs[rbase + tid + 1] - b) : 0;
        }
    __syncthreads();
    auto list = [&](int r) { return ws + ((size_t)(rbase + r) * R + range) * k; };
    auto merge_all = [&]() {
        for (int r = wid; r < SC_BM; r += 4)
            if (s_qn[r] > 0) {
                if constexpr (EXCL && EV)
                    topk_merge_row<true, true>(r, list(r), k, s_q + r * TK_Q, skq, sl, s_qn, s_ln, s_thr, s_xb[r], s_xn[r], item_idx, ex, sx, ev.s_first, s_xp[r]);
                else if constexpr (EXCL) topk_merge_row<true>(r, list(r), k, s_q + r * TK_Q, skq, sl, s_qn, s_ln, s_thr, s_xb[r], s_xn[r], item_idx, ex, sx);
                else topk_merge_row<false>(r, list(r), k, s_q + r * TK_Q, skq, sl, s_qn, s_ln, s_thr);
            }
        __syncthreads();
    };
    // rank counters (events form, fused): every lane's own share of its 8 rows' (greater, equal) counts over the whole range
    constexpr bool RANK = EV && !STORED && !LSE;      // (TkEventsLse: the normaliser, no counters)
    float tt[2][4];
    int cg[2][4], ce[2][4];
    if constexpr (RANK) {
#pragma unroll
        for (int ri = 0; ri < 2; ++ri)
#pragma unroll
            for (int rg = 0; rg < 4; ++rg) {
                const int row = rbase + 32 * wid + 16 * ri + 4 * lg + rg, rc = min(row, mrows - 1);
                float t = ev.tscore[rc];
                if (ev.tie_col) t += tie_noise(mp->seed, ev.tie_ctr, row, ev.tie_col[rc]);
                tt[ri][rg] = t; cg[ri][rg] = 0; ce[ri][rg] = 0;
            }
    }
    unsigned rq[2][4];      // (sampling form) the row ids of the lane's 8 rows
    if constexpr (SMP) {
#pragma unroll
        for (int ri = 0; ri < 2; ++ri)
#pragma unroll
            for (int rg = 0; rg < 4; ++rg) rq[ri][rg] = smp.row_id[min(rbase + 32 * wid + 16 * ri + 4 * lg + rg, mrows - 1)];
    }
    // (LSE) zeta of the lane's 8 rows and the lane's own share of their Q over the whole range.  Eligibility is decided per score here
    // (the selection only applies exclusions where a queue is merged): thread r < SC_BM walks row r's sorted list with a cursor --
    // all-items calls, whose columns are item indices: one lower_bound at c0, then per tile a compare with the next list item held in
    // a register and a load only on a hit -- or, with a candidate list, searches the row's list for each of the tile's 32 items.
    // Rows with an empty list do neither.  The lists grow between launches, so nothing is kept across them.
    // TkEventsLse: row r's list is its SESSION's, and an item found there takes its column only when its first occurrence is at or
    // before the row's position (lx_seen: one more load, on a hit only) -- merge-time TkEvents eligibility, decided per score.
    float zt[2][4];
    unsigned long long qa[2][4];
    long long lx_b = 0;
    int lx_n = 0, lx_cur = 0, lx_next = 0, lx_pos = 0;
    auto lx_seen = [&](int j) -> bool {
        if constexpr (EV) {
#if defined(G4R_MUTATE) && G4R_MUTATE == 27      // test build: the input event's own item (first occurrence AT the position) stays in Q
            return ev.s_first[lx_b + j] < lx_pos;
#else
            return ev.s_first[lx_b + j] <= lx_pos;
#endif
        } else {
            (void)j;
            return true;
        }
    };
    if constexpr (LSE && EV)
        if (tid < SC_BM) lx_pos = s_xp[tid];
    if constexpr (LSE) {
#pragma unroll
        for (int ri = 0; ri < 2; ++ri)
#pragma unroll
            for (int rg = 0; rg < 4; ++rg) {
                zt[ri][rg] = lse.zeta[(size_t)min(rbase + 32 * wid + 16 * ri + 4 * lg + rg, mrows - 1) * lse.zs];
                qa[ri][rg] = 0ull;
            }
        if (tid < SC_BM) {
            lx_b = s_xb[tid];
            lx_n = s_xn[tid];
#if defined(G4R_MUTATE) && G4R_MUTATE == 25      // test build: the LAST item of the row's list is never marked, its term is counted
            if (lx_n > 0) --lx_n;
#endif
            if (!item_idx && lx_n > 0) {
                int a = 0, b = lx_n;
                while (a < b) { const int mid = (a + b) >> 1; if ((long long)ex.items[lx_b + mid] < c0) a = mid + 1; else b = mid; }
                lx_cur = a;
                if (a < lx_n) lx_next = ex.items[lx_b + a];
            }
        }
    }
    for (long long n0 = c0; n0 < c1; n0 += TK_TN) {
        float v[2][2][4];      // [ri][cj][rg]: row 32 wid + 16 ri + 4 lg + rg, column n0 + 16 cj + li (the MFMA accumulator layout)
        if constexpr (!STORED) {
            const DevModel& m = *mp;
            const int D = m.Dtop;
            if (tid < TK_TN) {
                const long long n = n0 + tid;
                sItem[tid] = n < c1 ? (item_idx ? item_idx[n] : (int)n) : -1;
                if constexpr (LSE) {      // the tile's columns the global mask takes: one word, from the 32 threads that load the items
                    const int item = sItem[tid];
                    const unsigned long long dr = __ballot(item >= 0 && ex.mask && ((ex.mask[item >> 5] >> (item & 31)) & 1u));
                    if (tid == 0) *s_dropw = (unsigned)dr;
                }
            }
            __syncthreads();
            if constexpr (LSE) {
                if (tid < SC_BM) {      // row tid's word: the tile's columns whose item is in the row's list
                    unsigned w = 0u;
                    if (lx_n > 0 && !item_idx) {
                        const long long n1 = n0 + TK_TN;
                        while (lx_cur < lx_n && lx_next < n1) {
                            if (lx_seen(lx_cur)) w |= 1u << (int)(lx_next - n0);
                            if (++lx_cur < lx_n) lx_next = ex.items[lx_b + lx_cur];
                        }
                    } else if (lx_n > 0) {
                        for (int j = 0; j < TK_TN; ++j) {
                            const int item = sItem[j];
                            if (item < 0) break;      // (the columns past c1 close the last tile)
                            int a = 0, b = lx_n;
                            while (a < b) { const int mid = (a + b) >> 1; if (ex.items[lx_b + mid] < item) a = mid + 1; else b = mid; }
                            if (a < lx_n && ex.items[lx_b + a] == item && lx_seen(a)) w |= 1u << j;
                        }
                    }
                    s_rowx[tid] = w;      // (read after the chain's barriers below, written again after the next tile's first one)
                }
            }
            f32x4 acc[2][2];
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};
            for (int kc0 = 0; kc0 < D; kc0 += SC_KC) {
                const int kc = min(SC_KC, D - kc0), kc4 = kc >> 2;
                for (int e = tid; e < SC_BM * kc4; e += 256) {
                    const int i = e / kc4, c4 = e - i * kc4, row = rbase + i;
                    float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (row < mrows) x = ld4(h + (size_t)row * D + kc0 + 4 * c4);
                    float2* d = reinterpret_cast<float2*>(sA + i * ldk + 4 * c4);
                    d[0] = make_float2(x.x, x.y);
                    d[1] = make_float2(x.z, x.w);
                }
                for (int e = tid; e < TK_TN * kc4; e += 256) {
                    const int j = e / kc4, c4 = e - j * kc4, item = sItem[j];
                    float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (item >= 0) x = ld4(m.Wy + (size_t)item * D + kc0 + 4 * c4);
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
#pragma unroll
            for (int cj = 0; cj < 2; ++cj) {
                const int item = sItem[16 * cj + li];
                const float add = item >= 0 ? m.By[item] : 0.f;
#pragma unroll
                for (int ri = 0; ri < 2; ++ri)
#pragma unroll
                    for (int rg = 0; rg < 4; ++rg) v[ri][cj][rg] = final_act_fwd(m.final_act, m.fa_p0, m.fa_p1, acc[ri][cj][rg] + add);
            }
        } else {
#pragma unroll
            for (int ri = 0; ri < 2; ++ri)
#pragma unroll
                for (int rg = 0; rg < 4; ++rg) {
                    const int row = min(rbase + 32 * wid + 16 * ri + 4 * lg + rg, mrows - 1);
#pragma unroll
                    for (int cj = 0; cj < 2; ++cj) v[ri][cj][rg] = sc[(size_t)row * ldo + min(n0 + 16 * cj + li, c1 - 1)];
                }
        }
#pragma unroll
        for (int ri = 0; ri < 2; ++ri)
#pragma unroll
            for (int rg = 0; rg < 4; ++rg) {
                const int r = 32 * wid + 16 * ri + 4 * lg + rg;
                const unsigned long long t = s_thr[r];
                unsigned gone = 0u;      // (LSE) the tile's columns that are not eligible in this row
                if constexpr (LSE) gone = s_rowx[r] | *s_dropw;
#pragma unroll
                for (int cj = 0; cj < 2; ++cj) {
                    const long long n = n0 + 16 * cj + li;
                    if constexpr (LSE)
                        if (rbase + r < mrows && n < c1 && !((gone >> (16 * cj + li)) & 1u)) qa[ri][rg] += lse_term(v[ri][cj][rg], zt[ri][rg], lse.invT);
                    if constexpr (RANK) {      // in front of every exclusion: those are applied where a queue is merged
                        float x = v[ri][cj][rg];
                        if (ev.tie_col) x += tie_noise(mp->seed, ev.tie_ctr, rbase + r, n + ev.col_off);
                        cg[ri][rg] += (n < c1 && x > tt[ri][rg]) ? 1 : 0;
                        ce[ri][rg] += (n < c1 && x == tt[ri][rg]) ? 1 : 0;
                    }
                    float val = v[ri][cj][rg];
                    if constexpr (SMP)      // the draw's key (never contracted into an FMA); the tile's items are still in sItem
                        val = __fadd_rn(__fmul_rn(val, smp.invT), gumbel_noise(smp.seed, rq[ri][rg], smp.step, max(sItem[16 * cj + li], 0)));
                    const unsigned long long key = topk_key(val, (unsigned)n);
                    if (rbase + r < mrows && n < c1 && key > t) {
                        const int p = atomicAdd(s_qn + r, 1);
                        s_q[r * TK_Q + p] = make_uint2(__float_as_uint(val), (unsigned)n);
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
    if constexpr (LSE) {
        // the 16 lanes that share a row are added up (integers: any order gives the same bits), then one atomic per row and workgroup
#pragma unroll
        for (int ri = 0; ri < 2; ++ri)
#pragma unroll
            for (int rg = 0; rg < 4; ++rg) {
                unsigned long long q = qa[ri][rg];
#pragma unroll
                for (int o = 1; o < 16; o <<= 1) {
                    const unsigned lo = __shfl_xor((unsigned)q, o), hi = __shfl_xor((unsigned)(q >> 32), o);
                    q += ((unsigned long long)hi << 32) | lo;
                }
                const int row = rbase + 32 * wid + 16 * ri + 4 * lg + rg;
                if (li == 0 && row < mrows && q) atomicAdd(lse.Q + row, q);
            }
    }
    if constexpr (RANK) {
        // the 16 lanes that share a row (same lg) are added up, then one atomic pair per row and workgroup
#pragma unroll
        for (int ri = 0; ri < 2; ++ri)
#pragma unroll
            for (int rg = 0; rg < 4; ++rg) {
                int g = cg[ri][rg], e = ce[ri][rg];
#pragma unroll
                for (int o = 1; o < 16; o <<= 1) { g += __shfl_xor(g, o); e += __shfl_xor(e, o); }
                const int row = rbase + 32 * wid + 16 * ri + 4 * lg + rg;
                if (li == 0 && row < mrows) {
                    if (g) atomicAdd(ev.cnt + 2 * row, g);
                    if (e) atomicAdd(ev.cnt + 2 * row + 1, e);
                }
            }
    }
}

// Stage 2.  One workgroup per row: the k-th largest key T of the row's nl * k entries by an MSB-first radix select (eight 8-bit
// digits of the 64-bit key), then the k entries with key >= T (exactly k: keys are distinct), sorted in LDS, written out.
// With exclusions (EXCL range kernels) the lists hold eligible entries and pads only; g4r_recommend_step_filtered refuses a row with
// fewer than k eligible candidate positions, so the union of the row's lists still holds at least k real keys (every eligible
// position is kept unless k better eligible ones of its range are) and "exactly k at or above T" still holds.
// (topk_merge_lists: the body, for the whole workgroup; L = the row's lists, oc / os = the row's outputs; item_idx != NULL: the
// item index of the column is written instead of the column -- k_events_merge)
__device__ __forceinline__ void topk_merge_lists(const uint2* L, int nl, int k, int* oc, float* os, const int* item_idx) {
    __shared__ int hist[256];
    __shared__ int s_digit, s_need, s_cnt;
    __shared__ unsigned long long sk[TK_MAX];
    __shared__ uint2 se[TK_MAX];
    const int tid = threadIdx.x;
    const int N = nl * k;
    unsigned long long prefix = 0ull, mask = 0ull;
    int need = k;
    for (int shift = 56; shift >= 0; shift -= 8) {
        hist[tid] = 0;
        __syncthreads();
        for (int i = tid; i < N; i += 256) {
            const unsigned long long key = topk_key(L[i]);
            if ((key & mask) == prefix) atomicAdd(hist + (int)((key >> shift) & 255u), 1);
        }
        __syncthreads();
        // suffix sums: hist[d] <- number of matching entries whose digit is >= d
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
    sk[tid] = 0ull;
    __syncthreads();
    for (int i = tid; i < N; i += 256) {
        const uint2 e = L[i];
        const unsigned long long key = topk_key(e);
        if (key >= prefix) {
            const int p = atomicAdd(&s_cnt, 1);
            if (p < TK_MAX) { sk[p] = key; se[p] = e; }      // (exactly k <= TK_MAX get here)
        }
    }
    __syncthreads();
    for (int w = 2; w <= TK_MAX; w <<= 1)
        for (int j = w >> 1; j > 0; j >>= 1) {
            const int p = tid ^ j;
            if (p > tid) {
                const unsigned long long a = sk[tid], b = sk[p];
                if (((tid & w) == 0) ? (a < b) : (a > b)) {
                    sk[tid] = b; sk[p] = a;
                    const uint2 t = se[tid]; se[tid] = se[p]; se[p] = t;
                }
            }
            __syncthreads();
        }
    if (tid < k) {
        oc[tid] = item_idx ? item_idx[se[tid].y] : (int)se[tid].y;
        os[tid] = __uint_as_float(se[tid].x);
    }
}
__global__ __launch_bounds__(256) void k_topk_merge(const uint2* ws, int nl, int k, int* out_cols, float* out_scores) {
    topk_merge_lists(ws + (size_t)blockIdx.x * nl * k, nl, k, out_cols + (size_t)blockIdx.x * k, out_scores + (size_t)blockIdx.x * k, nullptr);
}
// g4r_recommend_events: row r of one step is the event at place[r] of the call's outputs (its slot, or its number within the piece
// being filled); the row's list (item indices: item_idx maps the columns of a candidate list), its rank and its target score go there
__global__ __launch_bounds__(256) void k_events_merge(const uint2* ws, int nl, int k, const long long* place, const int* item_idx,
                                                      const float* ranks, const float* tscore, int* out_items, float* out_scores,
                                                      float* out_rank, float* out_tscore) {
    const size_t s = (size_t)place[blockIdx.x];
    topk_merge_lists(ws + (size_t)blockIdx.x * nl * k, nl, k, out_items + s * k, out_scores + s * k, item_idx);
    if (threadIdx.x == 0) { out_rank[s] = ranks[blockIdx.x]; out_tscore[s] = tscore[blockIdx.x]; }
}
// softmax / softmax_logit: the target score of every row out of the materialised scores (column tcol[r] of row r)
__global__ __launch_bounds__(256) void k_events_tscore(const float* sc, long long ldo, const int* tcol, int mrows, float* out) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r < mrows) out[r] = sc[(size_t)r * ldo + tcol[r]];
}

#define TK_INSTANTIATE(name, STORED, EXCL, ...)                                                                                       \
    template __global__ void k_topk_range<STORED, EXCL, ##__VA_ARGS__>(const DevModel*, const float*, int, const int*, long long, \
                                                                       const float*, long long, int, int, uint2*, ##__VA_ARGS__);
TK_FORMS(TK_INSTANTIATE)
#undef TK_INSTANTIATE
// g4r_loglik_events: row r of one step is the event at place[r] (as k_events_merge places it): its target's z, the row's zeta and Q
// go there.  Clears the rank counters the k = 1 selection (k_topk_range<false, true, TkEvents>) left behind, as k_rank_counts does.
__global__ __launch_bounds__(256) void k_loglik_finish(const long long* place, const float* tz, const float* zeta, const unsigned long long* Q,
                                                       int* cnt, int mrows, float* out_z, float* out_zeta, unsigned long long* out_Q) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= mrows) return;
    const size_t s = (size_t)place[r];
    out_z[s] = tz[r]; out_zeta[s] = zeta[r]; out_Q[s] = Q[r];
    cnt[2 * r] = 0; cnt[2 * r + 1] = 0;
}

// ---- stateless replay of session histories (g4r_recommend_sessions) ---------------------------------------------------------
// A chunk's rows are sorted by history length, descending; perm[r] is the chunk row (caller's order) of sorted row r, len[r] its
// length.  Step t runs the prediction GRU kernels on sorted rows [0, M_t), reading the ping-pong buffer H[t & 1] and writing
// H[(t + 1) & 1], so a row's state after its last step lies in H[len & 1].
// k_replay_begin: sorted row r of one layer's H[0] <- the supplied initial row perm[r] (src: [rows][W], chunk order), or zeros
__global__ __launch_bounds__(256) void k_replay_begin(float* H0, const float* src, const int* perm, int rows, int W) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)rows * W) return;
    const int r = (int)(e / W), j = (int)(e - (long long)r * W);
    H0[e] = src ? src[(size_t)perm[r] * W + j] : 0.f;
}
// k_replay_final: dst[perm[r]] (chunk order) <- sorted row r's final state, taken from the buffer its own length's parity picks.
// tmax: the chunk's longest history (len[0])
__global__ __launch_bounds__(256) void k_replay_final(float* dst, const float* H0, const float* H1, const int* perm, const int* len,
                                                      int rows, int W, int tmax) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)rows * W) return;
    const int r = (int)(e / W), j = (int)(e - (long long)r * W);
#if defined(G4R_MUTATE) && G4R_MUTATE == 10      // test build: every row read from the buffer of the chunk's longest history
    const int par = tmax & 1;
#else
    const int par = len[r] & 1;
    (void)tmax;
#endif
    dst[(size_t)perm[r] * W + j] = (par ? H1 : H0)[e];
}

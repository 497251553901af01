// Device-side helpers for the gfx950 (MI355X) GRU4Rec kernels: wave64 reductions, fp32 MFMA tile
// primitive, Philox4x32-10, activations.  CDNA4 only (wave = 64 lanes; v_mfma_f32_16x16x4_f32).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gru4rec_hip.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

#define G4R_EPS_LOSS 1e-24f    /* gru4rec.py:230,241 */
#define G4R_EPS_ADAGRAD 1e-6f  /* gru4rec.py:330 */
#define G4R_OWN_INLINE 15      /* earlier occurrences an owner-table row holds (DevModel::own_pos) */
#define G4R_OWN_SLOTS 16       /* owner tables in the ring: the steps of a window (= G4R_GRAPH_STEPS, k_owner_window) */
#define G4R_OWN_WINDOW_MAXR 12288      /* longest occurrence list k_owner_window stages in its LDS (48 KB of ids) */
#define G4R_POS_ENT_MAXHS 8192          /* most hash slots (16 bytes each) of k_owner_window's per-position entries: the ids, the waves' position rows and the hash share 156 KB of LDS */
#define G4R_OWN_WINDOW_MINWG 4        /* pre-scan workgroups of k_loss_rows (16 occurrences each) up to which the pre-scan stays: a window launch would cost more */

// Mutation builds for the parity suite's self-test (tests/test_gpu_mutation.py builds them as variant libraries next to the product
// one and expects the parity tests to turn red): G4R_MUTATE=1 inflates every per-occurrence sparse accumulator increment by
// 1 %, =2 every sparse Adagrad step by 1 %, =3 every dense accumulator increment by 1 %.  Never defined in the product build.
#if defined(G4R_MUTATE) && G4R_MUTATE == 1
#define G4R_MUT_ACC(x) ((x) * 1.01f)
#else
#define G4R_MUT_ACC(x) (x)
#endif
#if defined(G4R_MUTATE) && G4R_MUTATE == 2
#define G4R_MUT_STEP(x) ((x) * 1.01f)
#else
#define G4R_MUT_STEP(x) (x)
#endif
#if defined(G4R_MUTATE) && G4R_MUTATE == 3
#define G4R_MUT_DACC(x) ((x) * 1.01f)
#else
#define G4R_MUT_DACC(x) (x)
#endif

#if defined(G4R_MUTATE) && G4R_MUTATE == 6      // the Adagrad step of ONE item row per step (the item of score column 0: the first target) x 1.5
#define G4R_MUT_ROW(n, x) ((n) == 0 ? (x) * 1.5f : (x))
#else
#define G4R_MUT_ROW(n, x) (x)
#endif
#if defined(G4R_MUTATE) && G4R_MUTATE == 8      // test build: the owner scan of the lean update (k_loss_rows' pre-scan, or k_update_l's own
// scan under G4R_OWNER_SCAN=1) skips the last id of every 1024-slice after the first
#define G4R_MUT_SLICE_SKIP(j, base0, start) ((base0) > (start) && (j) == (base0) + 1023)
#else
#define G4R_MUT_SLICE_SKIP(j, base0, start) false
#endif
#if defined(G4R_MUTATE) && G4R_MUTATE == 5      // the 1 / nranks factor of the exact-replica joint update (REDUCE / MEAN forms) x 1.01
#define G4R_MUT_XSCALE(x) ((x) * 1.01f)
#else
#define G4R_MUT_XSCALE(x) (x)
#endif
#if defined(G4R_MUTATE) && G4R_MUTATE == 16      // test build: the owner walk of k_sparse_update_generic drops the first hit of every pass after
// the first (an item with more than 64 earlier occurrences in a step loses one of them per later pass)
#define G4R_MUT_PASS_SKIP(pass, ri) ((pass) > 0 && (ri) == 0)
#else
#define G4R_MUT_PASS_SKIP(pass, ri) false
#endif
#if defined(G4R_MUTATE) && G4R_MUTATE == 17      // test build: opt_rule's new second statistic (adadelta's update average, Adam's mean) x 1.01
#define G4R_MUT_STAT2(x) ((x) * 1.01f)
#else
#define G4R_MUT_STAT2(x) (x)
#endif
#if defined(G4R_MUTATE) && G4R_MUTATE == 18      // test build: k_loss_rows' grp_fast takes a group of V columns whose LAST column is the first
// inactive in-batch one (column M) as wholly active
#define G4R_MUT_FAST_M(M) ((M) + 1)
#else
#define G4R_MUT_FAST_M(M) (M)
#endif
#if defined(G4R_MUTATE) && G4R_MUTATE == 19      // test build: k_loss_rows' first pass starts its loop past the prefetched groups one STEP late
#define G4R_MUT_FIRST_LATE(step) (step)
#else
#define G4R_MUT_FIRST_LATE(step) 0
#endif

#if defined(G4R_MUTATE) && G4R_MUTATE == 21      // test build: k_owner_window takes the sample-store row of EVERY step of its window from the
// window's first global step
#define G4R_MUT_WIN_G(g0, s) (g0)
#else
#define G4R_MUT_WIN_G(g0, s) ((g0) + (s))
#endif
#if defined(G4R_MUTATE) && G4R_MUTATE == 32      // test build: k_owner_window's per-position entries count a repeated item whose occurrences
// are all sampled negatives one too low
#define G4R_MUT_ENT_CNT(cnt, allsmp) (((allsmp) && (cnt) > 1) ? (cnt) - 1 : (cnt))
#else
#define G4R_MUT_ENT_CNT(cnt, allsmp) (cnt)
#endif
#if defined(G4R_MUTATE) && G4R_MUTATE == 29      // test build: finish_rows leaves out the sixteenth K-slice plane of dy
#define G4R_MUT_PLANES(nsl) min((nsl), 15)
#else
#define G4R_MUT_PLANES(nsl) (nsl)
#endif
#if defined(G4R_MUTATE) && G4R_MUTATE == 30      // test build: k_gru_p1s keys its embedding-dropout mask by the k offset INSIDE the slice
#define G4R_MUT_DROP_K(ks) 0
#else
#define G4R_MUT_DROP_K(ks) (ks)
#endif

// Philox stream ids (counter word 3); twin of oracle/philox.py
#define G4R_STREAM_SAMPLE 0x53414D50u
#define G4R_STREAM_DROP_EMBED 0x44454D42u
#define G4R_STREAM_DROP_HIDDEN 0x44484944u
#define G4R_STREAM_TIEBREAK 0x54494542u
// (G4R_STREAM_GUMBEL, the stream of g4r_sample_sessions' noise, is part of the ABI: include/gru4rec_hip.h)

// ---------------------------------------------------------------------------------------------
// Pointers that the kernels read out of device-resident descriptors (DevModel, DenseTile) would be generic
// ("flat") to the compiler: flat_load/flat_store also count against lgkmcnt and therefore serialise with every
// LDS access.  On the device pass the descriptor fields are typed as global-address-space pointers, so every
// access through them is a global_load/global_store; the host pass sees plain pointers of identical layout.
#if defined(__HIP_DEVICE_COMPILE__)
#define GAS __attribute__((address_space(1)))
#else
#define GAS
#endif
#define GP(T) GAS T*

__device__ __forceinline__ float4 ld4(const GAS float* p) { return *(const GAS float4*)p; }
__device__ __forceinline__ void st4(GAS float* p, float4 v) { *(GAS float4*)p = v; }
__device__ __forceinline__ int4 ldi4(const GAS int* p) { return *(const GAS int4*)p; }
#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ float4 ld4(const float* p) { return *(const float4*)p; }
__device__ __forceinline__ void st4(float* p, float4 v) { *(float4*)p = v; }
#endif
// Guarded loads WITHOUT a branch around the load: the address is clamped to the (always valid) base and the value
// is masked when it is consumed.  `cond ? load : 0` would make the zero a write-after-write hazard on the load's
// destination registers, and hipcc then puts an s_waitcnt vmcnt(0) behind every load of a batch (one full memory
// round trip per load instead of one per batch).
__device__ __forceinline__ float4 ld4_if(const GAS float* base, size_t off, bool ok) {
    const float4 v = ld4(base + (ok ? off : (size_t)0));
    return make_float4(ok ? v.x : 0.f, ok ? v.y : 0.f, ok ? v.z : 0.f, ok ? v.w : 0.f);
}
// raw variants: the element at `off` if ok, otherwise SOME valid element (no select after the load, so a group of them
// stays in flight together); for values that are only consumed under the same condition
__device__ __forceinline__ float4 ld4_at(const GAS float* base, size_t off, bool ok) { return ld4(base + (ok ? off : (size_t)0)); }
__device__ __forceinline__ float ldf_at(const GAS float* base, size_t off, bool ok) { return base[ok ? off : (size_t)0]; }
__device__ __forceinline__ float ldf_if(const GAS float* base, size_t off, bool ok) {
    const float v = base[ok ? off : (size_t)0];
    return ok ? v : 0.f;
}

// ---------------------------------------------------------------------------------------------
// Device-resident step state.  The step index lives on the device so that a captured hipGraph of
// step kernels is step-agnostic: the first kernel of a step reads *_a and republishes it as *_b,
// the middle kernels read *_b, the last kernel writes *_a = *_b + 1.  No kernel both reads and
// writes the same word, so stream order alone makes it race-free.
#define G4R_NORM_BLOCKS 256

struct StepState {
    long long t_a, t_b;   // plan step within the epoch
    long long g_a, g_b;   // global step (drives sample-store row, dropout counters, H ping-pong parity)
    int M_a, M_b;         // active batch rows of the step (plan M[t]), carried here so that a kernel needs ONE
                          // memory round trip (this struct, passed as a kernel argument) to know its context
    int nan_flag;
    int pad;
};

struct DevModel {
    // ---- configuration
    int n_items, n_layers, B, ns, N, R, ldSc;
    int loss, final_act, hidden_act, embed_mode;
    float fa_p0, fa_p1, ha_p0, ha_p1;
    float lr, mom, lmbd, bpreg, logq, inv_B, smoothing, pad_f;
    // generic optimizer path (adapt != adagrad, or grad_cap > 0): gradient producers leave RAW gradients in dS* / dense_g,
    // the update kernels apply the rule (gru4rec.py:300-381) and the global-norm clip (:386-389)
    int generic, adapt;
    float ap0, ap1, grad_cap, pad_g;
    GP(float) acc2Wy; GP(float) acc2By; GP(float) acc2E; GP(float) cntWy; GP(float) cntBy; GP(float) cntE;
    GP(float) dense_acc2; GP(float) dense_cnt;
    GP(float) gsq_part;      // [G4R_NORM_BLOCKS] partial sums of squares
    GP(float) gclip;         // [1] clip factor of this step (1 when the norm is below grad_cap)
    float drop_h, drop_e;
    unsigned long long seed;
    int D[G4R_MAX_LAYERS], IN[G4R_MAX_LAYERS];
    int Dtop, Ein;
    // ---- dense GRU parameters: one flat buffer [Wx0|Wh0|Wrz0|Bh0|Wx1|...]
    int offWx[G4R_MAX_LAYERS], offWh[G4R_MAX_LAYERS], offWrz[G4R_MAX_LAYERS], offBh[G4R_MAX_LAYERS];
    int dense_count;
    GP(float) dense_p; GP(float) dense_acc; GP(float) dense_vel; GP(float) dense_g;
    int apply_dense_inplace;   // 1: Adagrad fused into the gradient kernel (single GPU)
    float grad_scale;          // 1/nranks when gradients are all-reduced
    // ---- sparse tables (row-major, row = item)
    GP(float) Wy; GP(float) accWy; GP(float) velWy; GP(float) By; GP(float) accBy; GP(float) velBy;
    GP(float) E; GP(float) accE; GP(float) velE;
    // ---- per-layer state and saved activations
    GP(float) H[G4R_MAX_LAYERS][2];
    GP(float) r[G4R_MAX_LAYERS]; GP(float) z[G4R_MAX_LAYERS]; GP(float) c[G4R_MAX_LAYERS];
    GP(float) hd[G4R_MAX_LAYERS]; GP(float) Hr[G4R_MAX_LAYERS];
    GP(float) dV[G4R_MAX_LAYERS]; GP(float) dyl[G4R_MAX_LAYERS]; GP(float) Vc[G4R_MAX_LAYERS];
    // ---- scoring / loss
    GP(float) Sc; GP(float) dSx; GP(float) dSy; GP(float) dSBy; GP(float) dhpart; GP(float) lossrow; GP(float) loss_steps;
    // per-occurrence Adagrad pieces written by the gradient producers: dS* hold lr * g / sqrt(acc_pre + g^2 + eps)
    // (the scaled step), dA* hold acc_pre + g^2 (the accumulator value the LAST occurrence leaves behind)
    GP(float) dAx; GP(float) dAy; GP(float) dABy;
    int ksplit, kch;
    GP(float) yin0;    // [B][IN0] layer-0 input rows as the GRU saw them (gathered, embedding dropout applied)
    GP(int) occ_idx;   // [R] item of each gathered-row occurrence (X | Y | samples), -1 = inactive
    GP(int) col_item;  // [ldSc] item of each score column, -1 = inactive
    // inputs of the NEXT step, staged at fixed addresses by the bookkeeping block of the update kernel (and by k_set_state /
    // after a sample-store refill), so that the first kernels of a step load them next to the step state instead of behind it
    GP(int) cur_in;    // [2 B + 8]  in_idx row of the step about to run | its reset flags (one int per row) | (g lo, g hi, M, t lo, t hi)
    GP(int) cur_col;   // [ldSc] item of every score column of the step about to run (targets | -1 | samples | -1)
    // [tables][n_items][4]: (last occurrence + 1, R - first occurrence, count, 0) of every item touched this step, written
    // with atomics by the kernels that publish occ_idx and zeroed again by the row's owner in k_sparse_update
    // (table 0: Wy / By rows, table 1: separate input embedding E)
    GP(int) occ_fl;
    // multi-rank runs: [tables][n_items] bytes, set to 1 by the wave that rewrites a row of the item tables (the rows to
    // reconcile at the next g4r_comm_sync_sparse); null on a single GPU
    GP(unsigned char) touched;
    // ---- plan + samples
    GP(const int) in_idx; GP(const int) out_idx; GP(const int) Mplan;
    GP(const unsigned char) reset;
    GP(const int) ST;
    int gl;
    GP(const float) lq_tgt; GP(const float) lq_smp;
    GP(StepState) st;
    GP(long long) dbgclk;   // optional [kernel][16] phase timestamps (100 MHz wall clock), block 0 only
    GP(const float) zrow;   // 8192 zero floats: what the LDS-DMA tiles read for rows outside the matrix / inactive gathered rows
    GP(long long) dbgtile;  // optional [dense tile][8] phase timestamps of the dense-gradient tiles (G4R_CLK)
    // Per-occurrence exchange blocks.  occ_idx | dSx | dSy | dSBy of this rank are carved out of ONE block of xstride floats; in the
    // exact-replica mode of N > 1 (g4r_config::sparse_exact) xbase holds xn = nranks such blocks, this rank's own at index `rank`
    // (where the pointers above point) and the peers' filled in by an all-gather every step, and the generic sparse update walks the
    // concatenated occurrence list K = q * R + k (block q, occurrence k) in rank order.  xn = 1: the own block alone.
    GP(float) xbase;
    long long xstride;
    int xn, xoffSx, xoffSy, xoffSBy;      // float offsets of dSx / dSy / dSBy inside a block (occ_idx sits at offset 0, as ints)
    int xmode, xoffDg;                      // g4r_config::sparse_exact when xn > 1 (1 SUM, 2 MEAN, 3 REDUCE form of the exact-replica mode), else 0
    // wide layers (g4r_wide_kernels.cuh): dy = dV Wx^T of layer l leaves k_gru_bwd_bw as bbn[l] K-slice partial sums dyp[s][B][IN_l]
    // (0: the layer's dy is complete where the consumer expects it); they are added up, in slice order, by the kernel that consumes
    // dy anyway -- the lower layer's k_gru_bwd_pre, or (layer 0) the row-finishing workgroups of k_dense_grad2
    GP(float) dyp;
    int bbn[G4R_MAX_LAYERS];
    GP(float) vp;        // K-slice partial sums of GRU phase 1, vp[slice][B][3D] (k_gru_p1s -> k_gru_gate)
    // Deferred row updates (single GPU, Adagrad without momentum; g4r_step_kernels.cuh: k_defer_scan / k_sparse_flush).  The step
    // planes dSx / dSy / dSBy are rings of defer_mask + 1 slots (slot = global step & defer_mask; 0: one plane, nothing is deferred):
    // a row whose item is not gathered again before the end of the current window of steps keeps its step row in the ring and
    // is applied by ONE flush launch per window -- the same arithmetic on the same operands, in a launch long enough for the HBM.
    int defer_mask, dRcap;
    long long dSx_stride, dSy_stride, dSBy_stride;      // floats between two slots
    GP(int) last_use;    // [tables][n_items] newest scanned global step (low 32 bits) in which the item's row is gathered
    GP(int) dcand;       // [slots][dRcap] 1: occurrence k of that step is its item's last use inside the window (k_defer_scan)
    GP(int) dlist;       // [slots][dRcap] item of an occurrence whose row update is pending (written by its owner wave), else -1
    GP(unsigned) dstat;  // [1024][2] rows / bias entries applied by flush launches, per workgroup id mod 1024 (statistics)
    // narrow layers (g4r_lean_kernels.cuh): dr' = da Wh^T leaves k_gru_da as ceil(D / 16) K-slice partial planes drp[slice][B][D]; k_gru_dy adds them
    GP(float) drp;
    // owner table of the lean update (k_update_l): a ring of G4R_OWN_SLOTS tables of [R][16] ints, row k of the owner of a repeated
    // item = (number of earlier occurrences, their positions in ascending order), -1 when there are more than G4R_OWN_INLINE of them
    // (k_update_l scans for those).  k_owner_window (g4r_update_kernels.cuh) writes the tables of a whole window of steps, slot = the
    // step's index in its window; G4R_OWNER_WINDOW=0 and lists longer than its LDS: the pre-scan in k_loss_rows writes slot 0 every
    // step (g4r_loss_kernel.cuh).  The ring sits behind k_update_l's dense-tile table.  Null: no owner table (G4R_OWNER_SCAN=1, or no
    // k_update_l): every owner scans occ_idx itself.
    GP(int) own_pos;
    // per-position entries of the window form: a second ring of G4R_OWN_SLOTS tables of [(R + 3) & ~3] int4 next to own_pos, slot s,
    // position k = (last + 1, R - first, count, 0) of the item at position k over its table -- the value occ_fl[table][item] has once
    // the forward kernels of that step have published it; zeros where the position holds no item.  k_owner_window writes it; the
    // step's kernels then take the entry by position and nobody touches occ_fl.  Null: the entries are built inside every step.
    GP(int) pos_ent;
};
// step plane of global step g
#define G4R_SLOT(m, g) ((size_t)((g) & (long long)(m).defer_mask))
#define G4R_DSX(m, g) ((m).dSx + G4R_SLOT(m, g) * (size_t)(m).dSx_stride)
#define G4R_DSY(m, g) ((m).dSy + G4R_SLOT(m, g) * (size_t)(m).dSy_stride)
#define G4R_DSBY(m, g) ((m).dSBy + G4R_SLOT(m, g) * (size_t)(m).dSBy_stride)

// In-kernel phase traces (tools/clk*.py) exist only in builds made with G4R_BUILD_CLK=1 (-DG4R_CLK_TRACE): a test of a
// descriptor field at the top of a kernel makes its first instructions wait for the descriptor's scalar loads, which the vector
// loads of the step state otherwise overlap -- measured 0.5 us per launch on k_score_fwd.
#if defined(G4R_CLK_TRACE)
#define G4R_DBGCLK(m) ((m).dbgclk)
#define G4R_DBGTILE(m) ((m).dbgtile)
#else
#define G4R_DBGCLK(m) ((GAS long long*)nullptr)
#define G4R_DBGTILE(m) ((GAS long long*)nullptr)
#endif
// phase timestamp (debug): one lane of block 0 records the constant-rate wall clock
#define G4R_TICK(m, kern, phase)                                                                     \
    do {                                                                                             \
        if (G4R_DBGCLK(m) && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0)                  \
            G4R_DBGCLK(m)[(kern) * 16 + (phase)] = wall_clock64();                                       \
    } while (0)

// ---------------------------------------------------------------------------------------------
// Wave-wide reductions with DPP row operations (no LDS round trips): xor-1 / xor-2 within quads, then the mirrored
// half row and the mirrored row leave every lane with the sum of its 16-lane row; the four row sums are combined
// through scalar registers.  All 64 lanes must be active.  The result is wave-uniform.
template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
__device__ __forceinline__ float readlane_f(float v, int l) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
}
__device__ __forceinline__ float wave_sum(float v) {
    v += dpp_mov<0xB1>(v);       // quad_perm [1,0,3,2]
    v += dpp_mov<0x4E>(v);       // quad_perm [2,3,0,1]
    v += dpp_mov<0x141>(v);      // row_half_mirror
    v += dpp_mov<0x140>(v);      // row_mirror
    return (readlane_f(v, 0) + readlane_f(v, 16)) + (readlane_f(v, 32) + readlane_f(v, 48));
}
__device__ __forceinline__ float wave_max(float v) {
    v = fmaxf(v, dpp_mov<0xB1>(v));
    v = fmaxf(v, dpp_mov<0x4E>(v));
    v = fmaxf(v, dpp_mov<0x141>(v));
    v = fmaxf(v, dpp_mov<0x140>(v));
    return fmaxf(fmaxf(readlane_f(v, 0), readlane_f(v, 16)), fmaxf(readlane_f(v, 32), readlane_f(v, 48)));
}

// block-wide reductions for a 256-thread (4-wave) block; `red` is 8 floats of LDS scratch
__device__ __forceinline__ float block_sum_256(float v, float* red) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[w] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}
__device__ __forceinline__ float block_max_256(float v, float* red) {
    v = wave_max(v);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[w] = v;
    __syncthreads();
    return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// D(16x16) += A(16x4) * B(4x16), fp32 in / fp32 accumulate (exact fmaf chain).
// lane l supplies A[i = l&15][k = l>>4] and B[k = l>>4][j = l&15]; holds D[row = 4*(l>>4)+reg][col = l&15].
__device__ __forceinline__ f32x4 mfma16(float a, float b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
// D(32x32) += A(32x2) * B(2x32), fp32.  lane l supplies A[i = l&31][k = l>>5] and B[k = l>>5][j = l&31]; holds
// D[row = 8*(reg>>2) + 4*(l>>5) + (reg&3)][col = l&31] in its 16 registers.  Measured on MI355X with register-resident operands
// (tools/probes/mfma_probe.hip): this shape sustains 155 TFLOP/s (65 cycles per 4096 flop per SIMD) from ONE dependent chain per
// wave, the 16x16x4 shape 99-126 TFLOP/s (40-51 cycles per 2048 flop) whatever the number of chains / waves: the mid-size GEMMs
// (gemm_tile2) use this one.
// Workgroups are dealt to the 8 XCDs round robin (workgroup id mod 8), and every XCD has its own L2.  xcd_tile turns the
// id of a workgroup into a tile index such that the workgroups of ONE XCD walk a contiguous range of tiles: neighbouring tiles
// (same score columns / same slab of gathered rows) then share an L2 instead of pulling the same bytes into eight of them.
// A bijection on [0, n) for any n (XCD x owns ceil((n - x) / 8) ids).
__device__ __forceinline__ int xcd_tile(int id, int n) {
    const int per = n >> 3, rem = n & 7, x = id & 7, s = id >> 3;
    return x * per + min(x, rem) + s;
}
#ifndef G4R_XCD_SWIZZLE
#define G4R_XCD_SWIZZLE 1
#endif
#if G4R_XCD_SWIZZLE
#define G4R_XCD_TILE(id, n) xcd_tile((int)(id), (int)(n))
#else
#define G4R_XCD_TILE(id, n) ((int)(id))
#endif
typedef float f32x16 __attribute__((ext_vector_type(16)));
__device__ __forceinline__ f32x16 mfma32(float a, float b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}


// ---------------------------------------------------------------------------------------------
struct Philox4 { unsigned x, y, z, w; };
__device__ __forceinline__ Philox4 philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3,
                                                 unsigned k0, unsigned k1) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        const unsigned n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    Philox4 r = {c0, c1, c2, c3};
    return r;
}
__device__ __forceinline__ float u32_to_unit(unsigned x) { return (float)(x >> 8) * (1.0f / 16777216.0f); }

// dropout multiplier (0 or 1/retain) for element (row, col) at global step g; twin of oracle.philox.dropout_mask
__device__ __forceinline__ float drop_mult(unsigned long long seed, unsigned g, unsigned stream, int row, int col,
                                           float retain) {
    const Philox4 p = philox4x32_10((unsigned)(col >> 2), (unsigned)row, g, stream, (unsigned)seed,
                                    (unsigned)(seed >> 32));
    const int e = col & 3;
    const unsigned x = e == 0 ? p.x : (e == 1 ? p.y : (e == 2 ? p.z : p.w));
    return u32_to_unit(x) < retain ? 1.0f / retain : 0.0f;
}
// evaluation mode 'tiebreaking' (evaluation.py:55): uniform * 1e-10 for score (row, col) of evaluation step `ctr`;
// twin of oracle.philox.uniform_rows(..., STREAM_TIEBREAK)
__device__ __forceinline__ float tie_noise(unsigned long long seed, unsigned ctr, int row, long long col) {
    const Philox4 p = philox4x32_10((unsigned)(col >> 2), (unsigned)row, ctr, G4R_STREAM_TIEBREAK, (unsigned)seed, (unsigned)(seed >> 32));
    const int e = (int)(col & 3);
    const unsigned x = e == 0 ? p.x : (e == 1 ? p.y : (e == 2 ? p.z : p.w));
    return u32_to_unit(x) * 1e-10f;
}
// Gumbel noise of g4r_sample_sessions for (row id q, decoding step, item index): lane item & 3 of the Philox call (item >> 2, q, step,
// G4R_STREAM_GUMBEL) keyed by the caller's seed; u = (x >> 9) 2^-23 + 2^-24 (exact in fp32, in [2^-24, 1 - 2^-24]); g = -log(-log u) with
// the precise logf, finite, in about [-2.82, 16.64].  The one definition behind the selection (k_topk_range<.., TkSample>, k_sample_pick)
// and k_debug_gumbel; tests/sampling_ref.py holds its float64 twin
__device__ __forceinline__ float gumbel_noise(unsigned long long seed, unsigned q, unsigned step, int item) {
#if defined(G4R_MUTATE) && G4R_MUTATE == 20      // test build: the noise ignores the step
    step = 0u;
#endif
    const Philox4 p = philox4x32_10((unsigned)item >> 2, q, step, G4R_STREAM_GUMBEL, (unsigned)seed, (unsigned)(seed >> 32));
    const int e = item & 3;
    const unsigned x = e == 0 ? p.x : (e == 1 ? p.y : (e == 2 ? p.z : p.w));
    const float u = __fadd_rn(__fmul_rn((float)(x >> 9), 0x1p-23f), 0x1p-24f);
    return -logf(-logf(u));
}
__device__ __forceinline__ float4 drop_mult4(unsigned long long seed, unsigned g, unsigned stream, int row, int col4,
                                             float retain) {
    const Philox4 p = philox4x32_10((unsigned)col4, (unsigned)row, g, stream, (unsigned)seed, (unsigned)(seed >> 32));
    const float inv = 1.0f / retain;
    float4 m;
    m.x = u32_to_unit(p.x) < retain ? inv : 0.0f;
    m.y = u32_to_unit(p.y) < retain ? inv : 0.0f;
    m.z = u32_to_unit(p.z) < retain ? inv : 0.0f;
    m.w = u32_to_unit(p.w) < retain ? inv : 0.0f;
    return m;
}

// ---------------------------------------------------------------------------------------------
// Hardware transcendentals (v_exp_f32 / v_rcp_f32 / v_rsq_f32, ~1 ulp each): the element-wise chains of the
// loss / GRU / Adagrad kernels run at one or two waves per SIMD, where the IEEE-exact expf / division / sqrtf
// expansions (20-40 dependent instructions each) were the critical path.  Relative error <= ~1e-6, far inside
// the parity tolerance (the fp32 summation-order differences against the oracle are of the same size).
__device__ __forceinline__ float fexp(float x) { return __expf(x); }
__device__ __forceinline__ float frcp(float x) { return __builtin_amdgcn_rcpf(x); }
__device__ __forceinline__ float frsq(float x) { return __builtin_amdgcn_rsqf(x); }
__device__ __forceinline__ float sigmoidf_(float x) { return frcp(1.0f + fexp(-x)); }
__device__ __forceinline__ float ftanh(float x) { return 1.0f - 2.0f * frcp(fexp(2.0f * x) + 1.0f); }

// element-wise activations, gru4rec.py:189-223.  The piecewise ones (leaky / elu / selu) have a derivative that jumps at 0, and the
// reference's T.grad decides on the INPUT (switch on X >= 0).  The backward kernels only have the output, so the forward encodes
// the branch in the sign bit of a zero result: x < 0 always yields a value with the sign bit set (exp(x) - 1 rounds to +0 for
// |x| < 6e-8: returned as -0.0), x >= 0 never does.  -0.0 behaves as 0 in every later use; act_bwd_from_out reads the sign bit.
// (One score in ~2e5 lands in that window at the first step of an RSC15-sized run; deciding on the output there put a factor
// 1/alpha on one element of d cost / d s, which the training dynamics amplified to 1e-2 relative cost differences 300 steps later.)
__device__ __forceinline__ float neg_branch(float v) { return v == 0.0f ? -0.0f : v; }
__device__ __forceinline__ float act_fwd(int kind, float p0, float p1, float x) {
    switch (kind) {
        case G4R_ACT_RELU: return fmaxf(x, 0.0f);
        case G4R_ACT_TANH: return ftanh(x);
        case G4R_ACT_LEAKY: return x >= 0.0f ? fabsf(x) : neg_branch(p0 * x);
        case G4R_ACT_ELU: return x >= 0.0f ? fabsf(x) : neg_branch(p0 * (fexp(x) - 1.0f));
        case G4R_ACT_SELU: return x >= 0.0f ? p0 * fabsf(x) : neg_branch(p0 * (p1 * (fexp(x) - 1.0f)));
        default: return x;
    }
}
// The FINAL activation of the inference kernels (k_score_all, k_score_cand, the top-k / scan / index tiles: one function, so that their
// scores stay equal to the bit).  ftanh is good to an ulp of 1.0 (2^-23) whatever its argument: right for a hidden unit, but a score of 0.1
// is then off by 1e-6 of itself, and a candidate list whose scores are all small has no larger score to measure that against
// (tests/test_gpu_predict_edges.py, the one-candidate list: 1.24 x its bound).  Below |x| = 0.25 tanh is its odd series up to x^9 (the
// next term, 8.9e-3 x^11, is under 1e-8 of the result); from there on ftanh's ulp is under 5e-7 of the result.
__device__ __forceinline__ float final_act_fwd(int kind, float p0, float p1, float x) {
    if (kind != G4R_ACT_TANH) return act_fwd(kind, p0, p1, x);
    const float x2 = x * x;
    const float s = x * (1.0f + x2 * (-0.33333334f + x2 * (0.13333334f + x2 * (-0.053968254f + x2 * 0.021869488f))));
    return fabsf(x) < 0.25f ? s : ftanh(x);
}
// act_fwd's values without a branch around the exponential of elu / selu (element loops of the loss kernel: both sides of that
// branch run in nearly every wave, the branch only adds its bookkeeping); a NaN input still comes out as NaN
__device__ __forceinline__ float act_fwd_sel(int kind, float p0, float p1, float x) {
    if (kind == G4R_ACT_ELU || kind == G4R_ACT_SELU) {
        const float xm = x > 0.0f ? 0.0f : x;
        float t = (kind == G4R_ACT_ELU) ? p0 * (fexp(xm) - 1.0f) : p0 * (p1 * (fexp(xm) - 1.0f));
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("" : "+v"(t));      // hipcc otherwise turns the select below back into a branch around the exponential
#endif
        return x >= 0.0f ? (kind == G4R_ACT_ELU ? fabsf(x) : p0 * fabsf(x)) : neg_branch(t);
    }
    return act_fwd(kind, p0, p1, x);
}
// derivative expressed through the OUTPUT y (for the piecewise activations the sign BIT of y tells the branch, see above)
__device__ __forceinline__ float act_bwd_from_out(int kind, float p0, float p1, float y) {
    const bool pos = !(__builtin_bit_cast(unsigned, y) >> 31);
    switch (kind) {
        case G4R_ACT_RELU: return y > 0.0f ? 1.0f : 0.0f;
        case G4R_ACT_TANH: return 1.0f - y * y;
        case G4R_ACT_LEAKY: return pos ? 1.0f : p0;
        case G4R_ACT_ELU: return pos ? 1.0f : y + p0;
        case G4R_ACT_SELU: return pos ? p0 : y + p0 * p1;
        default: return 1.0f;
    }
}
// The hidden layers' derivative da / dc, from the candidate c[l] the forward stored: the one place k_gru_da, k_gru_bwd_fused and
// k_gru_bwd_pre take it from (their tanh fast paths stay in the kernels).  The product build is act_bwd_from_out under another name.
// Test builds (tests/test_gpu_mutation.py, tests/test_gpu_hidden_act.py): G4R_MUTATE=22 decides the branch of leaky / elu / selu on the
// VALUE of c (c >= 0) instead of its sign bit -- wrong exactly where the forward returned -0.0; =23 puts a factor 1.01 on their
// negative-branch slope.
__device__ __forceinline__ float hidden_act_bwd(int kind, float p0, float p1, float c) {
#if defined(G4R_MUTATE) && G4R_MUTATE == 22
    if (kind == G4R_ACT_LEAKY || kind == G4R_ACT_ELU || kind == G4R_ACT_SELU) {
        const bool pos = c >= 0.0f;
        return kind == G4R_ACT_LEAKY ? (pos ? 1.0f : p0) : kind == G4R_ACT_ELU ? (pos ? 1.0f : c + p0) : (pos ? p0 : c + p0 * p1);
    }
#endif
#if defined(G4R_MUTATE) && G4R_MUTATE == 23
    if ((kind == G4R_ACT_LEAKY || kind == G4R_ACT_ELU || kind == G4R_ACT_SELU) && (__builtin_bit_cast(unsigned, c) >> 31))
        return act_bwd_from_out(kind, p0, p1, c) * 1.01f;
#endif
    return act_bwd_from_out(kind, p0, p1, c);
}

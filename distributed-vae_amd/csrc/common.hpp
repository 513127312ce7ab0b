// Internal header of libmmvae_hip.so: shapes, workspace layout, and the gfx950 device helpers
// (fp32 MFMA tile products out of LDS, wave reductions, Philox) shared by every kernel file.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>
#include "../../include/mmvae.h"
#include "tune.h"

namespace mmvae {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int WAVE = 64;
constexpr int ROWS32 = 32;   // row block of the small-layer / row-wise kernels
constexpr int NP = 128;      // padded width of every narrow (<=128) dimension in MFMA tiles
constexpr int MAP_PAD = 256;  // valid entries behind the row map's last one (scalar requests run up to two K tiles of 64 ahead)
constexpr int DW11_LD = 132;  // row stride of the dW11 slab: H weights + 1 bias column, H <= 128
constexpr int SMALL_LD = 256; // row stride of a small-layer dW slab: [N<=128][K+1<=256]

__host__ __device__ inline int cdiv(int a, int b) { return (a + b - 1) / b; }
__host__ __device__ inline int64_t cdiv64(int64_t a, int64_t b) { return (a + b - 1) / b; }
__host__ __device__ inline int rup(int a, int b) { return cdiv(a, b) * b; }
__host__ __device__ inline int64_t imin64(int64_t a, int64_t b) { return a < b ? a : b; }
__host__ __device__ inline int64_t clamp64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }
// the row of a matrix of n_total rows that position pos of a selection reads: rows[pos] (rows null: pos itself), clamped, so
// that a row map that is none reads a wrong row, never outside the matrix
__host__ __device__ inline int64_t src_row(const int64_t* rows, int64_t pos, int64_t n_total) {
    return clamp64(rows ? rows[pos] : pos, 0, n_total - 1);
}
// the rows [c0, c1) of segment seg of a segment table (launch_segments, below): inside [0, n] and at most seg_len of them,
// whatever the table holds
__host__ __device__ inline void seg_range(const int64_t* seg_begin, int seg, int64_t n, int64_t seg_len, int64_t& c0, int64_t& c1) {
    c0 = clamp64(seg_begin[seg], 0, n);
    c1 = imin64(clamp64(seg_begin[seg + 1], c0, n), c0 + seg_len);
}

// ------------------------------------------------------------------------------------------
// Workspace layout (offsets in floats).  Authoritative copy; Python asks through
// mmvae_ws_offset().
// ------------------------------------------------------------------------------------------
struct Splits {
    int ks_fc1;   // split-K of fc1 forward
    int ns_fc11;  // column splits of the fused fc11 kernel
    int ks_dw;    // batch splits of the dW1 GEMM (and of both big dW GEMMs on the general path)
    int ks_dw11;  // batch splits of the dW11 GEMM on the fast path
    int ks_small; // batch splits of the batched small-layer dW GEMM
    int ks_gd10;  // gene splits of the d(d10) = dZ11 W11 GEMM (fast path; the fused general kernel uses ns_fc11)
};

constexpr int N_SMALL = 12;  // fc2 fc3 fc4 fc5 fcc musig fc6 fc7 fc8 fc9 fc10 + fc1.bias

struct Layout {
    int nblk32;   // ceil(B/32)
    int nblk64;   // ceil(B/64)
    Splits sp;
    // forward, saved for backward
    int64_t R[5];                  // R1..R4 [A,B,H], R5 [A,B,L]
    int nblkc;                       // ceil(B / CHAIN_ROWS)
    // cells per workgroup of the FORWARD chain launches (CHAIN_ROWS unless MMVAE_TUNE_CHAIN_ROWS_FWD asks for a smaller block:
    // measured, no gain) and their count
    int chain_rows_fwd, nblkf;
    int nblkl;                       // ceil(B / LAT_ROWS)
    int64_t bn_mean[5], bn_rstd[5];  // [A,W]
    int64_t bn_part[5];            // [A][nblk32][2][W]   (block mean, block M2)
    int64_t XLOW, CPROB, CC, YSOFT, CSMP, Y, MS, MU, LV, SS, ZIN;
    int64_t Dk[5];                 // D6 [A,B,L], D7..D10 [A,B,H]
    int64_t c_part, c_mean, c_iv;  // [A][nblk32][2][C], [A,C], [A,C]
    int64_t lat_part;              // [A][nblk32][2]  (kl sum, entropy sum)
    int64_t fc1_slab;              // [KS][A][B][NP]
    int n11;                       // loss partial slots per arm (zero-filled, a subset is written)
    int64_t fc11_part;             // [A][n11][2] (squared error sum, mismatch count)
    int64_t GD10_slab;             // [max(ns_fc11, ks_gd10)][A][B][H]
    int64_t DZ11;                  // [A][B][D]
    int64_t couple_part;           // [nblk32][2]  (pair distance sum, pair l2 sum)
    int64_t T_part, T;             // [nblk32][A][C], [A][C]
    // backward
    int64_t DZ[11];                // DZ[1..4] [A,B,H], DZ[5] [A,B,L], DZ[6] [A,B,L], DZ[7..10] [A,B,H]
    int64_t GZIN, GMS, GZC, G[6];  // G[5] [A,B,L] (grad wrt x_low); G[1..4] [A,B,H] grad wrt BN_i output
    int64_t bnb_part[6], bnb_sum[6];  // [A][nblk32][2][W], [A][2][W]   (index 1..5)
    int64_t dw1_slab;              // [KS][A][H][D]
    int64_t dw11_slab;             // [KS][A][D][DW11_LD]
    int64_t small_slab;            // [KS][A][N_SMALL][NP*SMALL_LD]
    int64_t xbits;                 // uint32 [A][B][ceil(D/32)] dropout keep-mask, bit-packed (fast path)
    // bf16 slice planes of the SMALL operands of the large GEMMs (fp32x3 engine, gemm_bf16.hip): [A][3][rows][cols] bf16,
    // zero-padded to whole tiles so that the GEMMs copy them into LDS without bounds checks or arithmetic
    int64_t pl_w1;                 // W1   [H -> 128][D -> rup 32]
    int64_t pl_w11;                // [W11 | b11]  [D -> rup 128][H + 1 -> 128]
    int64_t pl_dz1;                // dZ1  [B -> rup 256][H -> 128]
    int64_t pl_d10;                // [d10 | 1]  [B -> rup 256][H + 1 -> 128]
    // weights of the small layers for the fp32x3 form of the chain kernels (chain.hip): [A][PL_SMALL_SLOTS][3][128][128] bf16,
    // slot 0..3 fc2..fc5, 4..8 fc6..fc10 ([N][K] as in the parameters), 9..17 the same layers transposed ([K][N])
    int64_t pl_small;
    // exact batch sums (fixed-point accumulators, see acc_add below): [ACC_NSETS][A] sets of ACC_SET_FLOATS floats;
    // set k < 5: (sum, sum of squares) of BatchNorm k's input, set 5 + (l - 1): (sum G, sum G * xhat) of layer l's
    // BatchNorm backward, l = 1..5.  Sets 0..4 are zeroed by the first kernel of a forward pass, 5..9 by the first
    // kernel of a backward pass.
    int64_t acc;
    int64_t acc_end;               // end of the accumulator sets (the backward pass zeroes [ACC_BWD sets, acc_end))
    int64_t rowmap;                // uint32 [B + MAP_PAD]: element offsets of the batch's rows in the resident matrix (mmvae_train_step_rows)
    int64_t total;
};
// accumulator set geometry (device side below)
constexpr int PL_SMALL_LAYERS = 9, PL_SMALL_DEC0 = 4, PL_SMALL_SLOTS = 2 * PL_SMALL_LAYERS;   // (slot of fc6: the decoder's first)
constexpr int ACC_W = 128;                             // columns per set
constexpr int ACC_SET_I64 = 6 * ACC_W + 8;             // [6][ACC_W] slots + tail block, [0]: addends outside the window (-> NaN)
constexpr int ACC_SET_FLOATS = 2 * ACC_SET_I64;
constexpr int ACC_NSETS = 12;
// set indices: 0..4 BatchNorm 1..5 forward (sum, sum of squares), ACC_C the statistics of c for the coupling terms (both
// zeroed by the first kernel of a training forward pass), ACC_T the coupling's T sums (sum 1 only; zeroed by the coupling
// launcher, which may run more than once per forward pass), ACC_BWD + l - 1 the BatchNorm backward sums of layer l = 1..5
// (zeroed by the first kernel of a backward pass)
constexpr int ACC_C = 5, ACC_T = 6, ACC_BWD = 7;
inline int64_t acc_set_off(const Layout& L, int A, int set) { return L.acc + (int64_t)set * A * ACC_SET_FLOATS; }

Layout make_layout(const mmvae_dims& d, const mmvae_exec* ex);
Splits default_splits(const mmvae_dims& d, const mmvae_exec* ex);

// Per-arm parameter offsets (floats) -- mirrors mmvae_param_layout_t
struct POff {
    int64_t per_arm;
    int64_t o[MMVAE_N_PARAM_TENSORS];
    int64_t bn_per_arm;
    int64_t bn_mean[MMVAE_N_BN], bn_var[MMVAE_N_BN];
};
POff make_poff(const mmvae_dims& d);

void set_error(const char* fmt, ...);
// the launch just made failed: record why and return MMVAE_E_LAUNCH from the calling launcher
#define HIP_LAUNCH_CHECK(what)                                                        \
    do {                                                                              \
        hipError_t e_ = hipGetLastError();                                            \
        if (e_ != hipSuccess) {                                                       \
            set_error("%s: %s", what, hipGetErrorString(e_));                         \
            return MMVAE_E_LAUNCH;                                                    \
        }                                                                             \
    } while (0)
// mmvae_hyper.gemm_bf16 and mmvae_augment's gemm_bf16 name one of three engines (include/mmvae.h)
inline int check_gemm_engine(int gemm_bf16) {
    if (gemm_bf16 >= 0 && gemm_bf16 <= 2) return 0;
    set_error("gemm_bf16 must be 0, 1 or 2 (got %d)", gemm_bf16);
    return MMVAE_E_BADARG;
}

#ifdef __HIPCC__
// ------------------------------------------------------------------------------------------
// Device helpers
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ int lane_id() { return threadIdx.x & 63; }
__device__ __forceinline__ int wave_id() { return threadIdx.x >> 6; }

// Row of accumulator register r for this lane in a 32x32 MFMA result (col = lane & 31).
__device__ __forceinline__ int acc_row(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

__device__ __forceinline__ f32x16 mfma32(float a, float b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ f32x16 zero16() {
    f32x16 z;
#pragma unroll
    for (int i = 0; i < 16; ++i) z[i] = 0.f;
    return z;
}

// acc[32x32] += A[32 x K] * Bt[32 x K]^T.  Both tiles are LDS images with K contiguous
// (rows a_row0.. of At, rows b_row0.. of Bt).  `kgroups` groups of 8 k's.  Each lane fetches
// 4 consecutive k's with one ds_read_b128 and feeds 4 MFMAs: the k order inside a group is
// permuted identically for A and B, which leaves the dot product unchanged.
__device__ __forceinline__ void mma_nt(f32x16& acc, const float* At, int lda, int a_row0,
                                       const float* Bt, int ldb, int b_row0, int kgroups) {
    const int lane = lane_id();
    const float* pa = At + (a_row0 + (lane & 31)) * lda + 4 * (lane >> 5);
    const float* pb = Bt + (b_row0 + (lane & 31)) * ldb + 4 * (lane >> 5);
    // fragments of group g+1 are requested before the MFMAs of group g: LDS latency hides under them
    float4 a = *reinterpret_cast<const float4*>(pa);
    float4 b = *reinterpret_cast<const float4*>(pb);
    for (int g = 0; g < kgroups; ++g) {
        const int gn = (g + 1 < kgroups) ? g + 1 : g;
        const float4 an = *reinterpret_cast<const float4*>(pa + 8 * gn);
        const float4 bn = *reinterpret_cast<const float4*>(pb + 8 * gn);
        acc = mfma32(a.x, b.x, acc);
        acc = mfma32(a.y, b.y, acc);
        acc = mfma32(a.z, b.z, acc);
        acc = mfma32(a.w, b.w, acc);
        a = an;
        b = bn;
    }
}

// acc[32x32] += A[32 x K] * Bk[K x 32]; A as above (K contiguous), Bk an LDS image [k][n] with n
// contiguous (columns n0..n0+31).
__device__ __forceinline__ void mma_nn(f32x16& acc, const float* At, int lda, int a_row0,
                                       const float* Bk, int ldb, int n0, int kgroups) {
    const int lane = lane_id();
    const float* pa = At + (a_row0 + (lane & 31)) * lda + 4 * (lane >> 5);
    const float* pb = Bk + (4 * (lane >> 5)) * ldb + n0 + (lane & 31);
    float4 a = *reinterpret_cast<const float4*>(pa);
    float b0 = pb[0], b1 = pb[ldb], b2 = pb[2 * ldb], b3 = pb[3 * ldb];
    for (int g = 0; g < kgroups; ++g) {
        const int gn = (g + 1 < kgroups) ? g + 1 : g;
        const float4 an = *reinterpret_cast<const float4*>(pa + 8 * gn);
        const float* q = pb + (8 * gn) * ldb;
        const float n0_ = q[0], n1_ = q[ldb], n2_ = q[2 * ldb], n3_ = q[3 * ldb];
        acc = mfma32(a.x, b0, acc);
        acc = mfma32(a.y, b1, acc);
        acc = mfma32(a.z, b2, acc);
        acc = mfma32(a.w, b3, acc);
        a = an;
        b0 = n0_; b1 = n1_; b2 = n2_; b3 = n3_;
    }
}

// two adjacent 32-column tiles sharing the A fragments (n0 and n0 + 32); second tile optional
__device__ __forceinline__ void mma_nn2(f32x16& acc0, f32x16& acc1, bool second, const float* At, int lda,
                                        int a_row0, const float* Bk, int ldb, int n0, int kgroups) {
    const int lane = lane_id();
    const float* pa = At + (a_row0 + (lane & 31)) * lda + 4 * (lane >> 5);
    const float* pb = Bk + (4 * (lane >> 5)) * ldb + n0 + (lane & 31);
    const int o1 = second ? 32 : 0;
    float4 a = *reinterpret_cast<const float4*>(pa);
    float b0 = pb[0], b1 = pb[ldb], b2 = pb[2 * ldb], b3 = pb[3 * ldb];
    float c0 = pb[o1], c1 = pb[ldb + o1], c2 = pb[2 * ldb + o1], c3 = pb[3 * ldb + o1];
    for (int g = 0; g < kgroups; ++g) {
        const int gn = (g + 1 < kgroups) ? g + 1 : g;
        const float4 an = *reinterpret_cast<const float4*>(pa + 8 * gn);
        const float* q = pb + (8 * gn) * ldb;
        const float n0_ = q[0], n1_ = q[ldb], n2_ = q[2 * ldb], n3_ = q[3 * ldb];
        const float m0_ = q[o1], m1_ = q[ldb + o1], m2_ = q[2 * ldb + o1], m3_ = q[3 * ldb + o1];
        acc0 = mfma32(a.x, b0, acc0);
        if (second) acc1 = mfma32(a.x, c0, acc1);
        acc0 = mfma32(a.y, b1, acc0);
        if (second) acc1 = mfma32(a.y, c1, acc1);
        acc0 = mfma32(a.z, b2, acc0);
        if (second) acc1 = mfma32(a.z, c2, acc1);
        acc0 = mfma32(a.w, b3, acc0);
        if (second) acc1 = mfma32(a.w, c3, acc1);
        a = an;
        b0 = n0_; b1 = n1_; b2 = n2_; b3 = n3_;
        c0 = m0_; c1 = m1_; c2 = m2_; c3 = m3_;
    }
}

// acc[32x32] += Pk[K x 32]^T * Qk[K x 32]; both LDS images [k][.] with the non-k index contiguous.
// ksteps = K/2.
__device__ __forceinline__ void mma_tn(f32x16& acc, const float* Pk, int ldp, int m0,
                                       const float* Qk, int ldq, int n0, int ksteps) {
    const int lane = lane_id();
    const float* pa = Pk + (lane >> 5) * ldp + m0 + (lane & 31);
    const float* pb = Qk + (lane >> 5) * ldq + n0 + (lane & 31);
#pragma unroll 4
    for (int s = 0; s < ksteps; ++s) {
        acc = mfma32(pa[2 * s * ldp], pb[2 * s * ldq], acc);
    }
}

// Branch-free [1 x 4] load of a row-major matrix, zero outside [R, Cn].  Addresses are clamped and the
// result selected, so a tile's loads issue back to back (a per-element `if`, or even a uniform
// vec/scalar `if` around each load, makes hipcc wait vmcnt(0) per load).  VEC: ld % 4 == 0,
// Cn % 4 == 0, col % 4 == 0, base 16-byte aligned -- decide it once per tile, outside the loads.
template <bool VEC>
__device__ __forceinline__ float4 ldg4_t(const float* __restrict__ m, int64_t ld, int row, int col, int R, int Cn) {
    const bool rok = row < R;
    const float* p = m + (int64_t)(rok ? row : 0) * ld;
    float4 v;
    if (VEC) {
        const bool ok = rok && (col < Cn);
        v = *reinterpret_cast<const float4*>(p + (ok ? col : 0));
        v.x = ok ? v.x : 0.f; v.y = ok ? v.y : 0.f; v.z = ok ? v.z : 0.f; v.w = ok ? v.w : 0.f;
        return v;
    }
    const bool o0 = rok && (col < Cn), o1 = rok && (col + 1 < Cn), o2 = rok && (col + 2 < Cn), o3 = rok && (col + 3 < Cn);
    v.x = p[o0 ? col : 0]; v.y = p[o1 ? col + 1 : 0]; v.z = p[o2 ? col + 2 : 0]; v.w = p[o3 ? col + 3 : 0];
    v.x = o0 ? v.x : 0.f; v.y = o1 ? v.y : 0.f; v.z = o2 ? v.z : 0.f; v.w = o3 ? v.w : 0.f;
    return v;
}
struct VecTag { static constexpr bool value = true; };
struct ScalarTag { static constexpr bool value = false; };

// Workgroup barrier that orders LDS traffic only.  __syncthreads() also waits vmcnt(0), i.e. for every
// global store the wave has in flight; after an epilogue that is several microseconds per barrier.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// All-reduce over groups of W = 64 (the wave) or 32 (each half of it) lanes without LDS traffic: four DPP steps
// inside each row of 16 lanes (quad_perm xor 1, quad_perm xor 2, row_half_mirror, row_mirror) and the gfx950
// half-exchange instructions v_permlane16_swap / v_permlane32_swap across rows; the 32-lane group stops before
// the last.  (__shfl_xor lowers to ds_bpermute_b32, ~100 cycles of dependent latency per step; the row-wise
// kernels chain ~15 reductions per cell.)
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
template <int W, typename Op>
__device__ __forceinline__ float group_allreduce(float v, Op op) {
    static_assert(W == 64 || W == 32, "a group is the wave or half of it");
    v = op(v, dpp_f<0xB1>(v));    // quad_perm [1,0,3,2]
    v = op(v, dpp_f<0x4E>(v));    // quad_perm [2,3,0,1]
    v = op(v, dpp_f<0x141>(v));   // row_half_mirror
    v = op(v, dpp_f<0x140>(v));   // row_mirror: every lane holds its 16-lane row's result
    {
        const unsigned u = __builtin_bit_cast(unsigned, v);
        const auto r = __builtin_amdgcn_permlane16_swap(u, u, false, false);
        v = op(__builtin_bit_cast(float, (unsigned)r[0]), __builtin_bit_cast(float, (unsigned)r[1]));
    }
    if constexpr (W == 64) {
        const unsigned u = __builtin_bit_cast(unsigned, v);
        const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
        v = op(__builtin_bit_cast(float, (unsigned)r[0]), __builtin_bit_cast(float, (unsigned)r[1]));
    }
    return v;
}
template <int W>
__device__ __forceinline__ float group_sum(float v) {
    return group_allreduce<W>(v, [](float a, float b) { return a + b; });
}
template <int W>
__device__ __forceinline__ float group_max(float v) {
    return group_allreduce<W>(v, [](float a, float b) { return fmaxf(a, b); });
}
template <int W>
__device__ __forceinline__ int group_min_i(int v) {
    const float f = group_allreduce<W>(__builtin_bit_cast(float, v), [](float a, float b) {
        const int x = __builtin_bit_cast(int, a), y = __builtin_bit_cast(int, b);
        return __builtin_bit_cast(float, x < y ? x : y);
    });
    return __builtin_bit_cast(int, f);
}
__device__ __forceinline__ float wave_sum(float v) { return group_sum<64>(v); }
__device__ __forceinline__ float wave_max(float v) { return group_max<64>(v); }
__device__ __forceinline__ int wave_min_i(int v) { return group_min_i<64>(v); }

// ---- consumer-side recombination of per-row-block partials ---------------------------------
// Batch statistics cross every row block, so each BatchNorm used to cost a tiny finalize launch
// between two layers.  Instead every workgroup of the CONSUMING kernel recombines the producers'
// partials itself (125 KB out of L2 at B = 5000, W = 100; all workgroups compute bit-identical
// results because the order is fixed by (NT, nblk) alone).
//
// part: [nblk][2][W] = (block mean, block M2) over min(PR, B - PR blk) rows.  All NT threads call;
// thread t < W returns column t's (mean, M2) over the whole batch.  scratch: 3 * PART_MAXG * W floats
// of LDS the caller does not need until the next barrier it executes itself.
constexpr int PART_MAXG = 16;
constexpr int PART_BATCH = 16;
// rows per workgroup of the small-layer chain kernels (chain.hip) = rows per statistics partial they emit
#ifndef MMVAE_CHAIN_ROWS
#define MMVAE_CHAIN_ROWS 64
#endif
constexpr int CHAIN_ROWS = MMVAE_CHAIN_ROWS;
// cells per workgroup of the latent-block kernels (rowwise.hip, LatCell: their waves per workgroup, cells per wave and the
// two cell geometries).  These kernels are VALU-bound, so what counts is cells per CU: 48 gives 105 workgroups per arm at
// B = 5000 -- one per CU, three cells per wave slot (a wave, or half of one) -- where 32 gave 314 workgroups on 256 CUs,
// i.e. 58 CUs with two (four cells per wave slot).
constexpr int LAT_ROWS = 48;
// half-wave form of the latent kernels (rowwise.hip): a cell owns 32 lanes x LH_CPL registers (C <= 32 LH_CPL)
constexpr int LH_CPL = 3;
// The backward kernel runs beside the dW11 GEMM of the side stream, where smaller workgroups spread over all CUs
// measured faster in the step (61 against 70 us) although slower alone (32 against 24 us); with dW11 on 160 CUs
// (round 2, chain kernels on the split engine) 8 cells per workgroup again beat 16 (step 718 against 725 us; 32: 729).
#ifndef MMVAE_LAT_ROWS_BWD
#define MMVAE_LAT_ROWS_BWD 8
#endif
constexpr int LAT_ROWS_BWD = MMVAE_LAT_ROWS_BWD;
// The exact batch-sum accumulators (acc_add below) hold ACC_MAX_ADDENDS addends of the largest magnitude per column without a
// carry between their slots; a training batch may therefore have at most ACC_MAX_ADDENDS x (the fewest cells any producing
// workgroup adds at once) cells per rank.  Producers: the fc1 epilogue and the coupling (32-cell blocks), the chain kernels
// (CHAIN_ROWS, or the forward launches' smaller blocks, >= 8), the latent kernels (LAT_ROWS / LAT_ROWS_BWD).
constexpr int ACC_MAX_ADDENDS = 4096;
constexpr int ACC_MIN_PRODUCER_ROWS = LAT_ROWS_BWD < 8 ? LAT_ROWS_BWD : 8;
static_assert(ACC_MIN_PRODUCER_ROWS <= LAT_ROWS_BWD && ACC_MIN_PRODUCER_ROWS <= LAT_ROWS && ACC_MIN_PRODUCER_ROWS <= CHAIN_ROWS &&
              ACC_MIN_PRODUCER_ROWS <= 32 && ACC_MIN_PRODUCER_ROWS <= 8,
              "a producer of batch sums with fewer cells per workgroup lowers the batch-size cap of make_ctx: name it here");

template <bool VEC, int NT>
__device__ __forceinline__ void stats_from_partials_t(const float* __restrict__ part, int nblk, int B, int PR, int W,
                                                      float* scratch, float& mean_out, float& m2_out) {
    constexpr int E = VEC ? 4 : 1;
    const int units = 2 * W / E;   // load units per partial: the first W/E hold means, the rest M2s
    const int G = max(1, min(min(NT / units, PART_MAXG), nblk));
    const int t = threadIdx.x, u = t % units, g = t / units;
    if (g < G) {
        const bool is_mean = u * E < W;
        const int col = is_mean ? u * E : u * E - W;
        const float* p = part + u * E;
        float sh[E], s1[E], s2[E];
        float n = 0.f;
        // the group's first block mean is the shift: s2 - s1^2/n then loses nothing to cancellation.  It is the first
        // value of the first batch (a separate load for it would cost one more memory latency in front of the batch)
#pragma unroll
        for (int e = 0; e < E; ++e) { sh[e] = 0.f; s1[e] = 0.f; s2[e] = 0.f; }
        // PART_BATCH loads in flight per pass, clamped and weighted instead of branched (a branch around
        // a load makes hipcc wait for every load separately: one memory latency per partial)
        for (int i0 = g; i0 < nblk; i0 += PART_BATCH * G) {
            float v[PART_BATCH][E];
#pragma unroll
            for (int j = 0; j < PART_BATCH; ++j) {
                const int i = min(i0 + j * G, nblk - 1);
                if constexpr (VEC) {
                    const float4 q = *reinterpret_cast<const float4*>(p + (int64_t)i * 2 * W);
                    v[j][0] = q.x; v[j][1] = q.y; v[j][2] = q.z; v[j][3] = q.w;
                } else {
                    v[j][0] = p[(int64_t)i * 2 * W];
                }
            }
            if (i0 == g) {
#pragma unroll
                for (int e = 0; e < E; ++e) sh[e] = is_mean ? v[0][e] : 0.f;
            }
#pragma unroll
            for (int j = 0; j < PART_BATCH; ++j) {
                const int i = i0 + j * G;
                const float nb = i < nblk ? (float)min(PR, B - PR * i) : 0.f;
                const float w = is_mean ? nb : (i < nblk ? 1.f : 0.f);
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const float d = v[j][e] - sh[e];
                    s1[e] += w * d;
                    s2[e] += nb * d * d;
                }
                n += nb;
            }
        }
#pragma unroll
        for (int e = 0; e < E; ++e) {
            if (is_mean) {
                scratch[(g * 3 + 0) * W + col + e] = sh[e] + s1[e] / n;
                scratch[(g * 3 + 1) * W + col + e] = s2[e] - s1[e] * s1[e] / n;
            } else {
                scratch[(g * 3 + 2) * W + col + e] = s1[e];
            }
        }
    }
    lds_barrier();
    float n = 0.f, mean = 0.f, m2 = 0.f;
    if (t < W) {
        for (int k = 0; k < G; ++k) {   // Chan's pairwise update over the groups, fixed order
            const int cnt = (nblk - k + G - 1) / G;
            const float nb = (float)(PR * cnt - (((nblk - 1) % G == k) ? PR * nblk - B : 0));
            const float mg = scratch[(k * 3 + 0) * W + t];
            const float m2g = scratch[(k * 3 + 1) * W + t] + scratch[(k * 3 + 2) * W + t];
            const float nn = n + nb, dl = mg - mean;
            mean += dl * (nb / nn);
            m2 += m2g + dl * dl * (n * nb / nn);
            n = nn;
        }
    }
    mean_out = mean;
    m2_out = m2;
}
template <int NT>
__device__ __forceinline__ void stats_from_partials(const float* __restrict__ part, int nblk, int B, int PR, int W,
                                                    float* scratch, float& mean_out, float& m2_out) {
    if ((W & 3) == 0) stats_from_partials_t<true, NT>(part, nblk, B, PR, W, scratch, mean_out, m2_out);
    else stats_from_partials_t<false, NT>(part, nblk, B, PR, W, scratch, mean_out, m2_out);
}

// part: [nblk][n] plain partial sums -> thread t < n returns sum over blocks of part[.][t].
// scratch: NT * 4 doubles at most (G * n with G = NT / units).
template <bool VEC, int NT>
__device__ __forceinline__ float sums_from_partials_t(const float* __restrict__ part, int nblk, int n, double* scratch) {
    constexpr int E = VEC ? 4 : 1;
    const int units = n / E;
    const int G = max(1, min(min(NT / units, PART_MAXG), nblk));
    const int t = threadIdx.x, u = t % units, g = t / units;
    if (g < G) {
        double s[E];
#pragma unroll
        for (int e = 0; e < E; ++e) s[e] = 0.0;
        const float* p = part + u * E;
        for (int i0 = g; i0 < nblk; i0 += PART_BATCH * G) {
            float v[PART_BATCH][E];
#pragma unroll
            for (int j = 0; j < PART_BATCH; ++j) {
                const int i = min(i0 + j * G, nblk - 1);
                if constexpr (VEC) {
                    const float4 q = *reinterpret_cast<const float4*>(p + (int64_t)i * n);
                    v[j][0] = q.x; v[j][1] = q.y; v[j][2] = q.z; v[j][3] = q.w;
                } else {
                    v[j][0] = p[(int64_t)i * n];
                }
            }
#pragma unroll
            for (int j = 0; j < PART_BATCH; ++j) {
                const bool ok = i0 + j * G < nblk;
#pragma unroll
                for (int e = 0; e < E; ++e) s[e] += ok ? (double)v[j][e] : 0.0;
            }
        }
#pragma unroll
        for (int e = 0; e < E; ++e) scratch[g * n + u * E + e] = s[e];
    }
    lds_barrier();
    double r = 0.0;
    if (t < n)
        for (int k = 0; k < G; ++k) r += scratch[k * n + t];
    return (float)r;
}
template <int NT>
__device__ __forceinline__ float sums_from_partials(const float* __restrict__ part, int nblk, int n, double* scratch) {
    if ((n & 3) == 0) return sums_from_partials_t<true, NT>(part, nblk, n, scratch);
    return sums_from_partials_t<false, NT>(part, nblk, n, scratch);
}

// ReLU that keeps NaN (torch.relu does; fmaxf(NaN, 0) = 0 would turn a diverged hidden layer into zeros and the loss
// back into a finite number)
__device__ __forceinline__ float relu_keep_nan(float v) { return v < 0.f ? 0.f : v; }

// ---- fp32x3 engine (gemm_bf16.hip): the three bf16 slices of two fp32 values (low half: a, high half: b) ------------
__device__ __forceinline__ unsigned cvt_pk_bf16(float a, float b) {   // one v_cvt_pk_bf16_f32 (low half: a), round to nearest even
    unsigned r;
    asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ void split3(float a, float b, unsigned (&w)[3]) {
    // eleven VALU instructions per pair: 3 conversions, 4 half -> float, 4 exact subtractions
    w[0] = cvt_pk_bf16(a, b);
    a -= __uint_as_float(w[0] << 16);
    b -= __uint_as_float(w[0] & 0xFFFF0000u);
    w[1] = cvt_pk_bf16(a, b);
    a -= __uint_as_float(w[1] << 16);
    b -= __uint_as_float(w[1] & 0xFFFF0000u);
    w[2] = cvt_pk_bf16(a, b);
}

// ---- exact batch sums through fixed-point atomic accumulators ----------------------------------
// The alternative to the partial arrays above (production; MMVAE_TUNE_BN_PARTIALS switches back): a producing
// workgroup ADDS its block sums to one accumulator per column instead of storing them, so a consumer reads W numbers
// instead of W x (number of producing workgroups).  Floating-point atomics would make the result depend on the arrival
// order; these are integer adds, which commute: a block sum v (a double, |v| < 2^58) is written as the fixed-point number
// round-toward-zero(|v| * 2^84) = h * 2^92 + m * 2^46 + l (0 <= m, l < 2^46, h < 2^50), the three pieces get the sign of v
// and are added to three 64-bit slots with device-scope no-return atomics; 2^12 addends of the largest magnitude and
// either sign fit in the high slot and 2^17 in the others without a carry between the slots (more workgroups than that
// add to one column only for batches beyond 65 000 cells).  Window: block sums below 2^58 = 2.9e17 -- squares of
// activations of 6e7 in every cell of a 64-cell block --, resolution 2^-84 = 5e-26: the variance of a nearly dead unit
// (BatchNorm eps 1e-8 and below) and gradient sums of 1e-20 are still resolved.  A value outside the window (or NaN / Inf)
// counts in the set's flag word and every consumer then returns NaN (the reference's fp32 arithmetic overflows later, at
// squares of 3e38: a documented limit of this build).  The result is the exact sum of the block sums -- bit-identical
// from run to run and for every consumer -- and the consumers form mean and variance from it in fp64.
// Layout of a set: [6][ACC_W] slots (sum 1 high / middle / low, sum 2 high / middle / low; column-minor, so that the lanes
// of one atomic instruction -- one column each -- fall into as few cache lines as possible: the L2 retires an atomic
// request per line, and with one slot per line the same adds took 6 us per launch instead of 1), then the flag word.
__device__ __forceinline__ void acc_add(long long* __restrict__ set, int sum, int col, double v) {
    const double a = fabs(v);
    if (!(a < 0x1p58)) {
        __hip_atomic_fetch_add(set + 6 * ACC_W, 1ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    const double t = a * 0x1p84;
    const double h = floor(t * 0x1p-92);
    const double r = t - h * 0x1p92;             // exact: the low bits of t
    const double m = floor(r * 0x1p-46);
    const double l = floor(r - m * 0x1p46);
    long long ih = (long long)h, im = (long long)m, il = (long long)l;
    if (v < 0.0) { ih = -ih; im = -im; il = -il; }
    long long* p = set + (3 * sum) * ACC_W + col;
    if (ih) __hip_atomic_fetch_add(p, ih, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (im) __hip_atomic_fetch_add(p + ACC_W, im, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (il) __hip_atomic_fetch_add(p + 2 * ACC_W, il, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// column `col` of a set: both sums (NaN when the set's flag word is non-zero)
__device__ __forceinline__ void acc_get(const long long* __restrict__ set, int col, double& s1, double& s2) {
    long long q[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) q[k] = set[k * ACC_W + col];
    const long long bad = set[6 * ACC_W];
    s1 = ((double)q[0] * 0x1p92 + (double)q[1] * 0x1p46 + (double)q[2]) * 0x1p-84;
    s2 = ((double)q[3] * 0x1p92 + (double)q[4] * 0x1p46 + (double)q[5]) * 0x1p-84;
    if (bad) { s1 = __builtin_nan(""); s2 = s1; }
}
// (sum, sum of squares) over B rows -> (mean, M2) as stats_from_partials returns them
__device__ __forceinline__ void acc_mean_m2(const long long* __restrict__ set, int col, int B, float& mean, float& m2) {
    double s1, s2;
    acc_get(set, col, s1, s2);
    const double mu = s1 / (double)B;
    mean = (float)mu;
    m2 = (float)fmax(s2 - s1 * mu, 0.0);
    if (s1 != s1) m2 = mean;
}
// a block's (mean, M2) over nb rows -> its contribution to (sum, sum of squares)
__device__ __forceinline__ void acc_add_stats(long long* __restrict__ set, int col, float nb, float mean, float m2) {
    const double n = (double)nb, mu = (double)mean;
    acc_add(set, 0, col, n * mu);
    acc_add(set, 1, col, (double)m2 + n * mu * mu);
}
__device__ __forceinline__ void acc_add_sums(long long* __restrict__ set, int col, float s1, float s2) {
    acc_add(set, 0, col, (double)s1);
    acc_add(set, 1, col, (double)s2);
}
// zero n4 float4 of p, spread over the whole grid (first kernel of a pass: the accumulator sets it is going to fill)
__device__ __forceinline__ void grid_zero(float* __restrict__ p, int n4) {
    const int nt = blockDim.x * blockDim.y * blockDim.z;
    const int64_t nblk = (int64_t)gridDim.x * gridDim.y * gridDim.z;
    const int64_t blk = blockIdx.x + (int64_t)gridDim.x * (blockIdx.y + (int64_t)gridDim.y * blockIdx.z);
    for (int64_t i = blk * nt + threadIdx.x + blockDim.x * (threadIdx.y + blockDim.y * threadIdx.z); i < n4; i += nblk * nt)
        reinterpret_cast<float4*>(p)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
}

// ---- Philox4x32-10 -----------------------------------------------------------------------
struct u32x4 { uint32_t x, y, z, w; };

__host__ __device__ inline u32x4 philox4x32(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                            uint32_t k0, uint32_t k1) {
    const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)M0 * c0;
        const uint64_t p1 = (uint64_t)M1 * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
        const uint32_t n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        const uint32_t n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += W0; k1 += W1;
    }
    return u32x4{c0, c1, c2, c3};
}

// Noise streams of the Philox mode.  Counter = (element group, stream id, step); key = seed.  (The contract is stated in
// DESIGN.md section 20 and restated on the host in tests/noise_restatement.py, to which tests/test_gpu_noise.py holds the kernels.)
enum { STREAM_XMASK = 0, STREAM_GUMBEL = 1, STREAM_STATE = 2, STREAM_SMASK = 3 };

struct NoiseDev {
    int mode;
    const uint8_t* x_mask;
    const float* u_gumbel;
    const float* u_state;
    const uint8_t* s_mask;
    uint32_t k0, k1;       // seed
    uint32_t step_lo, step_hi;
    uint32_t x_mlog2;      // input dropout: m = 1 << x_mlog2 random bits per element (see xmask_keep)
    uint32_t x_thr;        //   keep iff the element's m-bit field < x_thr, x_thr = round((1-p) 2^16) >> (16 - m) in [0, 2^m]
    uint32_t s_keep_thr;   // state dropout: keep iff u32 < thr (thr = (1-p) * 2^32, saturated)
};

__host__ __device__ inline uint32_t keep_threshold(float p_drop) {
    double k = (1.0 - (double)p_drop) * 4294967296.0;
    if (k >= 4294967295.0) return 0xFFFFFFFFu;
    if (k <= 0.0) return 0u;
    return (uint32_t)k;
}

__host__ __device__ inline uint32_t keep_threshold16(float p_drop) {
    double k = (1.0 - (double)p_drop) * 65536.0 + 0.5;
    if (k >= 65536.0) return 65536u;
    if (k <= 0.0) return 0u;
    return (uint32_t)k;
}

// 4 random words for elements [4*g, 4*g+3] of stream (arm, kind).
__device__ __forceinline__ u32x4 noise_words(const NoiseDev& nz, int arm, int kind, uint64_t group) {
    return philox4x32((uint32_t)group, (uint32_t)(group >> 32), (uint32_t)(arm * 4 + kind) ^ (nz.step_hi << 8),
                      nz.step_lo, nz.k0, nz.k1);
}
__device__ __forceinline__ float u01(uint32_t w) { return (float)(w >> 8) * (1.0f / 16777216.0f); }
__device__ __forceinline__ uint32_t pick(const u32x4& w, int i) {
    return i == 0 ? w.x : (i == 1 ? w.y : (i == 2 ? w.z : w.w));
}
// scalar access helpers (used by the row-wise kernels; the GEMM loaders use the vector form)
__device__ __forceinline__ float noise_uniform(const NoiseDev& nz, int arm, int kind, uint64_t idx) {
    const u32x4 w = noise_words(nz, arm, kind, idx >> 2);
    return u01(pick(w, (int)(idx & 3)));
}
__device__ __forceinline__ bool noise_keep(const NoiseDev& nz, int arm, int kind, uint64_t idx, uint32_t thr) {
    const u32x4 w = noise_words(nz, arm, kind, idx >> 2);
    const uint32_t v = pick(w, (int)(idx & 3));
    return thr == 0xFFFFFFFFu ? true : (v < thr);
}
// Input-dropout keep decision for gene `col` of cell `row`.  The B x D mask is the only noise large enough for the
// generator to cost time (25 M elements per arm per step: 21 us of Philox at 16 bits per element), so an element takes
// only as many random bits as the keep probability needs: m = 1, 2, 4, 8 or 16, the smallest with round((1-p) 2^16)
// a multiple of 2^(16-m) (p = 0.5: one bit per element; resolution of p: 2^-16).  One Philox call serves the 128/m
// consecutive genes [cg * 128/m, ...) of one row: counter (cg, row, stream ^ (step_hi << 8), step_lo); element i of the
// group owns bits [i m, (i+1) m) of the 128-bit output (word i m / 32), and is kept iff that field < x_thr.
__device__ __forceinline__ u32x4 xmask_words(const NoiseDev& nz, int arm, uint32_t row, uint32_t cg) {
    return philox4x32(cg, row, (uint32_t)(arm * 4 + STREAM_XMASK) ^ (nz.step_hi << 8), nz.step_lo, nz.k0, nz.k1);
}
__device__ __forceinline__ bool xmask_field_keep(const NoiseDev& nz, const u32x4& w, uint32_t i) {
    const uint32_t bit = i << nz.x_mlog2;
    const uint32_t f = (pick(w, (int)(bit >> 5)) >> (bit & 31u)) & (0xFFFFFFFFu >> (32 - (1 << nz.x_mlog2)));
    return f < nz.x_thr;
}
__device__ __forceinline__ bool xmask_keep(const NoiseDev& nz, int arm, int row, int col) {
    const int epg_log2 = 7 - nz.x_mlog2;
    const u32x4 w = xmask_words(nz, arm, (uint32_t)row, (uint32_t)col >> epg_log2);
    return xmask_field_keep(nz, w, (uint32_t)col & ((1u << epg_log2) - 1u));
}
// Keep-mask words one work item of make_xbits_range writes: with m <= 4 bits per element one Philox call (128 bits) fills
// 4 / m words; otherwise, and for an explicit mask, one word.  The launchers size their grids by it.
__host__ __device__ __forceinline__ int xbits_words_per_thread(const NoiseDev& nz) {
    const uint32_t mlog2 = nz.x_mlog2, m = 1u << mlog2;
    return nz.mode != 0 && m <= 4 ? (int)(4u >> mlog2) : 1;
}
// The bit-packed dropout keep-mask of x (k_make_xbits, gemm_fast.hip; also a role of the step's prologue launch,
// gemm_bf16.hip): threads first, first + stride, ... of the A * B * ceil(wpr / words-per-thread) work items.
__device__ __forceinline__ void make_xbits_range(const NoiseDev& nz, int A, int B, int D, int wpr, uint32_t* __restrict__ bits,
                                                 int64_t first, int64_t stride) {
    const uint32_t mlog2 = nz.x_mlog2, m = 1u << mlog2;
    const int wpt = xbits_words_per_thread(nz);
    const int tpr = (wpr + wpt - 1) / wpt;                // threads per row
    const int64_t n = (int64_t)A * B * tpr;
    for (int64_t i = first; i < n; i += stride) {
        const int tq = (int)(i % tpr);
        const int64_t ar = i / tpr;
        const int row = (int)(ar % B), arm = (int)(ar / B);
        uint32_t* out = bits + ar * wpr;
        if (nz.mode == 0) {
            const uint8_t* mk = nz.x_mask + ((int64_t)arm * B + row) * D;
            for (int k = 0; k < wpt; ++k) {
                const int w = tq * wpt + k;
                if (w >= wpr) break;
                uint32_t word = 0;
                for (int j = 0; j < 32; ++j) {
                    const int col = 32 * w + j;
                    if (col < D && mk[col]) word |= (1u << j);
                }
                out[w] = word;
            }
            continue;
        }
        if (m <= 4) {
            // one call = genes [tq * 128/m, ...) = words tq * wpt .. + wpt - 1
            const u32x4 r = xmask_words(nz, arm, (uint32_t)row, (uint32_t)tq);
            for (int k = 0; k < wpt; ++k) {
                const int w = tq * wpt + k;
                if (w >= wpr) break;
                uint32_t word = 0;
                if (m == 1) {
                    const uint32_t f = pick(r, k);   // gene j of the word <-> bit j
                    word = nz.x_thr >= 2 ? 0xFFFFFFFFu : (nz.x_thr == 1 ? ~f : 0u);
                } else {
                    for (int j = 0; j < 32; ++j) word |= xmask_field_keep(nz, r, (uint32_t)(32 * k + j)) ? (1u << j) : 0u;
                }
                const int left = D - 32 * w;
                if (left < 32) word &= (1u << left) - 1u;
                out[w] = word;
            }
        } else {
            // 32 genes = m / 4 calls of 128 / m genes
            const int w = tq, ncall = (int)(m >> 2), epc = 32 / ncall;
            uint32_t word = 0;
            for (int j = 0; j < ncall; ++j) {
                const u32x4 r = xmask_words(nz, arm, (uint32_t)row, (uint32_t)(w * ncall + j));
                for (int e = 0; e < epc; ++e) word |= xmask_field_keep(nz, r, (uint32_t)e) ? (1u << (j * epc + e)) : 0u;
            }
            const int left = D - 32 * w;
            if (left < 32) word &= (1u << left) - 1u;
            out[w] = word;
        }
    }
}
#endif  // __HIPCC__

// shape rules shared by default_splits (which sees only the dims and the exec) and make_plan (api.hip)
inline bool fast_dims(const mmvae_dims& d) { return (d.D & 3) == 0 && (d.H & 3) == 0; }
inline bool bf16_tiles_fit(const mmvae_dims& d) { return d.H <= 124; }         // the bf16 engines' D x H tiles
inline bool x3_fc11_fits(const mmvae_dims& d) { return d.H + 1 <= 112; }       // k_x3_fc11g: [d10 | 1] within 112 columns
inline bool chain_planes_fit(const mmvae_dims& d) { return d.C + d.S <= 128 && d.L <= 128; }   // one 128 x 128 plane per layer
// the fused fc11 kernels of the bf16 engines: the loss partials of their 128-cell blocks fit the slots
inline bool fc11_slots_fit(const Layout& L, int B) { return (int64_t)cdiv(B, 128) * L.sp.ks_gd10 <= L.n11; }

// Per-call plan: which kernels a call runs, on which stream, and which launch writes what for whom.  make_plan (api.hip)
// builds it once per entry point; the launchers and drivers read it and decide nothing themselves.
enum CallKind { CALL_STEP, CALL_STEP_ROWS, CALL_FORWARD, CALL_BACKWARD, CALL_LOSS, CALL_CLASSIFY, CALL_REPLAY /*debug stage*/,
                CALL_DECODE /*mmvae_decode, and the decoder half of mmvae_state_changes*/, CALL_TRAVERSE /*its encoder half*/,
                CALL_ENCODE = 10 /*9 stays unknown to mmvae_debug_plan; mmvae_encode: the encoder and the latent block, or its head alone*/,
                CALL_ZINB_STEP = 11 /*mmvae_zinb_train_step: the step's forward and backward around the ZINB gradient kernels; no side stream*/ };
// fc1, dW1, dW11: gemm_big.hip, fp32 matrix instruction (gemm_fast.hip), k_bf16_* / k_x3_* (gemm_bf16.hip)
enum GemmFamily { GEMM_GENERAL, GEMM_FP32, GEMM_BF16, GEMM_X3 };
// fc11 + d(d10): k_fc11_fused, k_fc11_zg (d(d10) folded in), k_fc11_zt + k_gd10_*, k_bf16_fc11* (+ k_bf16_gemm), k_x3_fc11g;
// decode (x_rec only: no x, no loss, no dZ11): k_fc11_fused_out (GENERAL), k_fc11_zt_out (ZT), k_fc11_out<1> / <3>
enum Fc11Family { FC11_GENERAL, FC11_ZG, FC11_ZT, FC11_BF16, FC11_X3, FC11_OUT_BF16, FC11_OUT_X3 };
// the launch that zeroes the loss partial slots and the forward accumulator sets at the start of a forward pass (none:
// eval mode or a replayed stage -- the fc11 launchers then zero their slots themselves)
enum FwdZero { ZERO_NONE, ZERO_MEMSET, ZERO_XBITS /*k_make_xbits*/, ZERO_PRESPLIT /*the head k_presplit launch*/ };
// a fused step's coupling terms: main stream behind fc11 (do_loss), side stream, or a role of the decoder chain's launch
enum CouplePlace { COUPLE_INLINE, COUPLE_SIDE, COUPLE_IN_DEC };
struct Plan {
    CallKind kind;
    bool fast;              // 16-byte aligned params and x, shape within 32-bit offsets
    GemmFamily big;         // (GEMM_GENERAL exactly off the fast path)
    bool small_x3;          // the batched small-layer dW products on k_x3_small (when every product fits its tiles)
    Fc11Family fc11;
    int gd10_slabs;         // d(d10) slabs the decoder backward sums
    int dw11_slabs;         // dW11 slabs the gradient reduction sums
    bool chain_planes;      // the chain kernels' fp32x3 form (small-layer weight planes, Layout::pl_small)
    bool lat_half;          // the latent kernels' half-wave form
    bool narrow;            // bf16 storage: W1, [W11 | b11] and dZ1 are read as bf16, slice 0 of their planes
    bool presplit;          // slice planes: k_presplit at the head of the forward pass (W1 and [W11 | b11], small layers),
    bool bwd_small_planes;  //   k_presplit at the head of a backward call of its own (small layers),
    bool d10_planes;        //   the decoder chain ([d10 | 1]),
    bool dz1_in_apply;      //   k_bn_bwd_apply (dZ1)
    bool dec_planes;        //   decode: k_presplit with the decoder's weights only (fc6..fc10 slots, [W11 | b11])
    FwdZero zero;
    bool rowmap;            // the batch is read through the row map (mmvae_train_step_rows; the head launch builds it)
    bool dz11_bf16;         // the fused fc11 kernel writes dZ11 as bf16 and dW11 reads it so (bf16 storage)
    bool dw11_side;         // dW11 and the fc11 tensors' reduction on the side stream beside the backward chain
    bool loss_on_side;      // the fused step's loss scalars follow dW11 on the side stream
    CouplePlace couple;
    bool lat_fork_rides;    // EV_LAT rides on the latent forward kernel
    bool fc11_fork_rides;   // EV_FORK rides on the fused fc11 kernel: do_backward's dW11 fork only waits
};

// ------------------------------------------------------------------------------------------
// Launch context handed to the stage launchers (host)
// ------------------------------------------------------------------------------------------
struct Ctx {
    mmvae_dims d;
    mmvae_hyper h;
    Layout lay;
    POff po;
    float* ws;
    hipStream_t stream;
    mmvae_exec ex;          // copy of the caller's execution context (zeros when the caller passed none)
    mmvae_exec* ex_out;     // the caller's own, for `early_recorded` (may be null)
    hipStream_t side() const { return reinterpret_cast<hipStream_t>(ex.side_stream); }
    hipEvent_t ev(int i) const { return reinterpret_cast<hipEvent_t>(ex.ev[i]); }
    int tune(int i) const { return ex.tune[i]; }
    // training-mode batch sums through the fixed-point accumulators (production) or the per-workgroup partial arrays
    bool use_acc() const { return !ex.tune[MMVAE_TUNE_BN_PARTIALS]; }
    bool dropout() const { return h.training && h.x_drop > 0.f; }   // input dropout is on: the keep-mask exists and is applied
    float fc11_coef() const { return (float)(d.A > 1 ? d.A - 1 : 1) / (float)d.B; }   // weight of fc11's loss term in dZ11
    // the range Plan::zero names a launch for: [fc11_part, end of the forward accumulator sets)
    // (through the coupling's T set: the fused step's coupling runs inside the decoder chain's launch and finds it zeroed; the
    // coupling's own launcher zeroes it again, it may run more than once per forward pass)
    int64_t fwd_zero_floats() const { return acc_set_off(lay, d.A, ACC_BWD) - lay.fc11_part; }
    int64_t bwd_zero_floats() const { return lay.acc_end - acc_set_off(lay, d.A, ACC_BWD); }
    // mmvae_train_step_rows: the batch is rows x_rows[0 .. B) (device, int64) of the resident matrix [x_nrows][x_ld] that the
    // call's `x` points at; the head launch of the step turns them into the row map (Layout::rowmap)
    const int64_t* x_rows = nullptr;
    // ... and, optionally, its bf16 copy (same shape and leading dimension, in elements): the bf16 engine's large GEMMs and its
    // fused fc11 kernel read x from it and dZ11 travels as bf16 (Plan::dz11_bf16)
    const unsigned short* x16 = nullptr;
    int64_t x_ld = 0, x_nrows = 0;
    Plan plan{};            // make_plan (api.hip), once per entry point
};
// ahead of an fc11 kernel that adds to the loss partial slots: no launch of this call has zeroed them (Plan::zero: eval mode,
// a replayed stage), so fill them here
inline int zero_fc11_part(const Ctx& c) {
    if (c.plan.zero != ZERO_NONE) return 0;
    hipError_t e = hipMemsetAsync(c.ws + c.lay.fc11_part, 0, sizeof(float) * 2 * (size_t)c.d.A * c.lay.n11, c.stream);
    if (e != hipSuccess) { set_error("memset: %s", hipGetErrorString(e)); return MMVAE_E_LAUNCH; }
    return 0;
}
#ifdef __HIPCC__
// Launch on the context's stream.  stop_ev != nullptr: a fork event rides on the kernel (hipExtLaunchKernel's stop event: the
// dispatch packet's own completion signal) instead of a hipEventRecord behind it -- a recorded event is a barrier packet of
// its own, 6 - 7 us of idle main stream at every fork; the fork then only makes the side stream wait.  The plan names the
// launches that carry one (Plan::lat_fork_rides, fc11_fork_rides) and their launchers pass it.
template <class K, class... Args>
inline void launch_k(const Ctx& c, hipEvent_t stop_ev, K kernel, dim3 grid, dim3 block, unsigned shm, Args... args) {
    if (stop_ev) hipExtLaunchKernelGGL(kernel, grid, block, shm, c.stream, nullptr, stop_ev, 0, args...);
    else hipLaunchKernelGGL(kernel, grid, block, shm, c.stream, args...);
}
#endif
// events of mmvae_exec.ev by role
enum { EV_LAT = 0, EV_COUPLE, EV_FC11, EV_FORK, EV_JOIN, EV_DEC, EV_ENC, EV_SPARE /* unused */ };

#ifdef __HIPCC__
NoiseDev make_noise_dev(const mmvae_noise* nz, const mmvae_hyper& h);
#endif

// stage launchers (one per kernel family); each returns 0 or MMVAE_E_LAUNCH
int launch_fc1_fwd(const Ctx& c, const mmvae_noise* nz, const float* params, const float* x, int64_t xs);
int launch_bn_eval_stats(const Ctx& c, const float* bn_running);   // eval mode: all five layers, one launch
int launch_chain_fwd_enc(const Ctx& c, int layer /*2..5*/, const float* params, float* bn_running, int64_t* nbt);
int launch_chain_fwd_enc_eval(const Ctx& c, const float* params);   // eval mode: fc2..fc5 in one launch
int launch_lat_fwd(const Ctx& c, const mmvae_noise* nz, const float* params, float* bn_running, int64_t* nbt,
                   int32_t* labels = nullptr /*eval: argmax of c per cell and arm*/);
// mmvae_encode: where the latent kernel stores the caller's outputs -- cell b of arm a is row a * rows + row0 + b of each
// array that is not null.  head: only x_low / c_prob are wanted, the kernel returns behind the first softmax.
struct EncOut {
    float *x_low, *c_prob, *c, *c_smp, *s_mean, *s_logvar;
    int32_t* labels;
    int64_t row0, rows;
    bool head;
};
// the latent forward of a CALL_ENCODE plan (k_lat_fwd_g<W, NW, ENC>: the forward's kernel body with EncOut's stores); labels_ab: compact
// [A, B] labels for the confusion counts, or null
int launch_lat_enc(const Ctx& c, const mmvae_noise* nz, const float* params, float* bn_running, int64_t* nbt,
                   const EncOut& eo, int32_t* labels_ab);
// mmvae_intermed: mu = fc_mu(y), var = sigmoid(fc_sigma(y)) for N rows of every arm (k_intermed)
int launch_intermed(const mmvae_dims& d, const POff& po, const float* params, const float* y, int64_t y_arm_stride, float* mu,
                    float* var, hipStream_t s);
// mmvae_prune_apply: +0.0f at the positions of the categories cat_mask does not keep, in each non-null buffer (k_prune_apply, prune.hip)
int launch_prune_apply(const mmvae_dims& d, const POff& po, const uint32_t cat_mask[4], float* params, float* grads,
                       float* exp_avg, float* exp_avg_sq, hipStream_t s);
int launch_chain_fwd_dec(const Ctx& c, const float* params);   // (with the coupling terms as a role: Plan::couple)
int launch_fc11_fused(const Ctx& c, const float* params, const float* x, int64_t xs, float* x_rec, int need_grad);
int launch_couple(const Ctx& c);
// zrec != null (double [A], device): rec[a] is zrec[a], the ZINB loss of arm a, in place of the MSE expression
int launch_loss_finalize(const Ctx& c, float* loss_out, int mode = 0 /*1: the T sums only, 2: the scalars only*/,
                         const double* zrec = nullptr);
int launch_chain_bwd_dec(const Ctx& c, const float* params);
int launch_lat_bwd(const Ctx& c, const mmvae_noise* nz, const float* params);
int launch_chain_bwd_enc(const Ctx& c, int layer /*5..2*/, const float* params);
int launch_bn_bwd_apply1(const Ctx& c);
int launch_dw_big(const Ctx& c, const mmvae_noise* nz, const float* x, int64_t xs);
int launch_dw_small(const Ctx& c, int which = 3 /*bit0 decoder layers, bit1 encoder side*/);
// one product of the batched small-layer gradient GEMM: out[m][n] = sum_b P[b][m] * Q'[b][n]  (gemm_big.hip, gemm_bf16.hip)
struct TnDesc {
    const float* P; int64_t p_arm_stride; int ldp; int Mv;   // rows of out
    const float* Q; int64_t q_arm_stride; int ldq; int Nv;   // cols of out (before the ones column)
    int q_ones;            // 1: column Nv of Q is the constant 1 (bias gradient)
    int q_xmask;           // 1: Q is x, apply dropout keep-mask (scale applied by the reducer)
    const float* q_mean;   // != null: Q <- (Q - mean[n]) * rstd[n]   (BatchNorm-normalised input)
    const float* q_rstd;   //          arrays are [A][Nv]
    float* out; int64_t out_arm_stride; int64_t out_ks_stride; int ldo;   // out[ks][arm][m][n]
};

struct TnDescs { TnDesc d[N_SMALL]; };
int launch_dw_small_x3(const Ctx& c, const TnDescs& ts, int nsel);
struct AdamHost { float* p; float* m; float* v; int64_t step; float lr, b1, b2, eps, wd; int decoupled; };
// slabs -> grads; with `adam` (p != null) the Adam update is fused into the same pass
int launch_reduce_grads(const Ctx& c, float* grads, float grad_scale, const AdamHost* adam,
                        int which = 3 /*bit0 fc11 tensors, bit1 the rest*/);
int launch_adam(int64_t n, float* p, const float* g, float* m, float* v, int64_t step, float lr, float b1,
                float b2, float eps, float wd, int decoupled, hipStream_t s);
int launch_make_xbits(const Ctx& c, const mmvae_noise* nz);
// first thing of a forward pass whose Plan::zero is ZERO_MEMSET or ZERO_XBITS: zero the loss partial slots and the
// forward accumulator sets (folded into k_make_xbits when that runs, a fill otherwise)
int launch_forward_zero(const Ctx& c, const mmvae_noise* nz);
int launch_fc1_epi(const Ctx& c, const float* params);
// fp32 matrix-instruction family (gemm_fast.hip): GEMM_FP32, FC11_ZG (d(d10) folded in), FC11_ZT (+ launch_gd10_fp32)
int launch_fc1_fwd_fp32(const Ctx& c, const float* params, const float* x, int64_t xs);
int launch_fc11_zg(const Ctx& c, const float* params, const float* x, int64_t xs, float* x_rec, int need_grad);
int launch_fc11_zt(const Ctx& c, const float* params, const float* x, int64_t xs, float* x_rec, int need_grad);
int launch_gd10_fp32(const Ctx& c, const float* params);
int launch_dw1_fp32(const Ctx& c, const float* x, int64_t xs);
int launch_dw11_fp32(const Ctx& c);
// bf16-operand variants of the five D x H GEMMs (gemm_bf16.hip; mmvae_hyper.gemm_bf16), same outputs / layouts
// gemm_bf16 == 2: fp32 operands split exactly into three bf16 slices each (six slice products per product: fp32-grade
// results on the bf16 matrix pipe); the same tile engine with three LDS planes per operand
// the k_presplit launch of Plan::presplit (head = true) or Plan::bwd_small_planes
int launch_x3_planes(const Ctx& c, const float* params, bool head, const mmvae_noise* nz = nullptr);
int launch_fc1_fwd_bf16(const Ctx& c, const float* params, const float* x, int64_t xs);           // GEMM_BF16 and GEMM_X3
int launch_dw1_bf16(const Ctx& c, const float* x, int64_t xs);
int launch_dw11_bf16(const Ctx& c);
int launch_fc11_x3(const Ctx& c, const float* params, const float* x, int64_t xs);                // FC11_X3: loss, dZ11 and d(d10)
// FC11_BF16: need_grad without x_rec the same in one fused kernel, else k_bf16_fc11 (and launch_gd10_bf16 for d(d10))
int launch_fc11_bf16(const Ctx& c, const float* params, const float* x, int64_t xs, float* x_rec, int need_grad);
int launch_gd10_bf16(const Ctx& c, const float* params);
// decode (Plan::fc11 of a CALL_DECODE plan): x_rec = relu([d10 | 1] [W11 | b11]^T) and nothing else -- no x, no loss, no dZ11
int launch_fc11_zt_out(const Ctx& c, const float* params, float* x_rec);         // gemm_fast.hip
int launch_fc11_fused_out(const Ctx& c, const float* params, float* x_rec);      // gemm_big.hip
int launch_fc11_out_bf16(const Ctx& c, float* x_rec);                            // gemm_bf16.hip, from the slice planes
int launch_dec_planes(const Ctx& c, const float* params);                        // Plan::dec_planes
// the decoder input rows [c | s] (ZIN of the decoder's workspace): decode packs the caller's c and s; the traversal
// (mmvae_state_changes) builds n_samp rows per cell from the encoder's workspace
struct ZinBuild {
    int A, R, C, S, L;            // arms, rows of the decoder, widths
    // decode (enc_ws == nullptr): c + a * c_arm + r * C, s + a * s_arm + r * S
    const float* c; int64_t c_arm; const float* s; int64_t s_arm;
    // traversal: row r = samp * B + b; enc_ws holds the encoder's CSMP / Y / MU ([A][B][.])
    const float* enc_ws; int64_t csmp, y, mu; int B, d_s;
    const float* params; int64_t per_arm, o_wsig, o_bsig;   // fc_sigma.weight / .bias
    const float* u;               // explicit U(0,1) [A][n_samp][B], or nullptr: Philox (seed, offset) of `nz`
    float* zin;                   // [A][R][C + S]
};
int launch_zin_build(const ZinBuild& z, const mmvae_noise* nz, const mmvae_hyper& h, hipStream_t s);
// planes x planes GEMM (gemm_pp.hip): tiled slice planes of a matrix X [R][K] -- NP planes (3 exact slices / 1 rounded), each
// [KT = ceil(K / 16)][Rp = R rounded up to 256][16] bf16, zero for k >= K
struct TPlanes { unsigned short* p; int64_t plane; int Rp, KT; };
inline int tp_rp(int R) { return rup(R, 256); }
inline int tp_kt(int K) { return cdiv(K, 16); }
inline int64_t tp_plane_elems(int R, int K) { return (int64_t)tp_kt(K) * tp_rp(R) * 16; }
inline TPlanes tp_make(unsigned short* p, int R, int K) { return TPlanes{p, tp_plane_elems(R, K), tp_rp(R), tp_kt(K)}; }
int launch_tp_from_f32(hipStream_t s, const float* src, int64_t ld, int R, int K, int NP, TPlanes dst, float* zero_flags_of_scratch = nullptr);
int launch_rp_from_f32(hipStream_t s, const float* src, int64_t ld, int R, int K, int NP, TPlanes dst);   // row-major planes [NP][Rp][KT][16]
constexpr int PP_MAX_WG = 256;                           // workgroups of a K-split k_pp_gemm launch at most (partial slots)
constexpr int PP_MAX_KS = 8;
constexpr int PP_FLAG_SLOTS = 16;                        // launches between two launch_pp_zero_flags
constexpr int PP_FLAG_WORDS = PP_FLAG_SLOTS * PP_MAX_WG;
int64_t pp_scratch_floats();
int launch_pp_zero_flags(hipStream_t s, float* scratch);
int launch_pp_gemm(hipStream_t s, int NP, TPlanes a, TPlanes b, int M, int N, const float* scale, const float* shift, bool affine, bool relu,
                   float* out32, int64_t ld32, int ncols32, const TPlanes* outp, float* scratch, int64_t scratch_floats, int flag_slot, int force = 0,
                   const unsigned* a_map = nullptr, int a_map_rows = 0);
int launch_pp_rowmap(hipStream_t s, const int64_t* rows, int n, int64_t n_rows, unsigned* out, int n_pad, float* zero_flags_of_scratch = nullptr);
// evaluation labels / consensus (consensus.hip)
int launch_classify(const float* cc, int64_t n_cells, int C, int32_t* labels, hipStream_t s);
int launch_confmat(const int32_t* labels, int A, int64_t n, int C, int64_t* counts, hipStream_t s);
int launch_consensus(const int64_t* counts, int npairs, int C, double* cm_norm, double* consensus, hipStream_t s);
constexpr int PS_LDS_MAX_C = 116;   // largest C whose pair-statistics histogram fits a workgroup's LDS (consensus.hip)
int launch_pair_stats(const int32_t* labels, const float* probs, int64_t n, int C, const int32_t* pairs, int n_pairs,
                      int64_t* counts, int64_t* dist_acc, int path, hipStream_t s);
int launch_pair_finish(const int64_t* counts, const int64_t* dist_acc, int n_pairs, int C, double* cm_norm, double* emp,
                       double* dist_norm, double* diag_mean, double* diag_min, hipStream_t s);
// mutual-information evaluation (mutinfo.hip)
constexpr int MI_LDS_MAX_WORDS = 16384;   // F * C + C + F 32-bit counts at most for the LDS histograms of k_mi_counts (64 KiB)
int launch_mi_counts(const int32_t* labels, int A, int64_t n, int C, const void* targets, int tsize, int64_t ldt, int F,
                     int64_t* counts, int64_t* t_sum, int64_t* p_sum, int path, hipStream_t s);
int launch_ami_binary(const int64_t* n11, const int64_t* t_sum, const int64_t* p_sum, int A, int F, int C, int64_t N, double* ws,
                      double* ami, hipStream_t s);
// ---- what the analysis routines below share ----
// 16-byte loads of a row's elements: the base is 16-byte aligned and the row pitch a whole number of 16 bytes
inline bool wide16(const void* p, int64_t ld, int elem_bytes) { return reinterpret_cast<uintptr_t>(p) % 16 == 0 && (ld * elem_bytes) % 16 == 0; }
// a byte count as a size_t; 0 where it is beyond SIZE_MAX / 2 (a workspace nobody can have)
inline size_t bytes_or_0(unsigned __int128 bytes) { return bytes > (unsigned __int128)(SIZE_MAX / 2) ? 0 : (size_t)bytes; }
// The segment scheme of silhouette, state_corr and group_moments (segments.hip).  n rows arrive ordered by group, offsets
// [G + 1] cutting them; group g with f_g > 0 rows is cut into ceil(f_g / seg_len) consecutive segments that never cross a group
// boundary, at most nseg_max(n, G, seg_len) in all.  One launch writes the table: gseg[g] the group's first segment,
// gseg[G] their number, seg_begin[s] the first row of segment s, seg_begin[gseg[G]] = offsets[G] (launch_segments; offsets
// null: one group, 0 and n).  A partial kernel then owns one segment (seg_range) and a finish kernel adds each group's
// segments in order.  The workspace: part double [nseg_max][doubles_per_segment], seg_begin int64 [nseg_max + 1], gseg int32
// [G + 1] rounded up to whole 8 bytes.
inline int64_t nseg_max(int64_t n, int G, int seg_len) { return (int64_t)G + n / seg_len; }
inline size_t seg_ws_bytes(int64_t nseg, int64_t doubles_per_segment, int G) {
    const unsigned __int128 s = (unsigned __int128)nseg;
    return bytes_or_0(8 * (s * (unsigned __int128)doubles_per_segment + s + 1) + 4 * (((unsigned __int128)G + 2) / 2 * 2));
}
struct SegWs { double* part; int64_t* seg_begin; int* gseg; };
inline SegWs seg_ws_carve(void* ws, int64_t nseg, int64_t doubles_per_segment) {
    double* part = static_cast<double*>(ws);
    int64_t* seg_begin = reinterpret_cast<int64_t*>(part + nseg * doubles_per_segment);
    return SegWs{part, seg_begin, reinterpret_cast<int*>(seg_begin + nseg + 1)};
}
int launch_segments(const int64_t* offsets, int G, int64_t n, int seg_len, int64_t nseg_max, int* gseg, int64_t* seg_begin,
                    hipStream_t st);
// silhouette samples (silhouette.hip)
constexpr int SIL_SEG_COLS = 512;      // columns per segment at most: a longer cluster is cut into pieces of this many
constexpr int SIL_ROW_TILE = 256;      // rows per workgroup of k_sil_partial, one thread each
constexpr int SIL_LDS_FLOATS = 4096;   // floats of staged columns per pass (16 KiB)
constexpr int SIL_MAX_D = 128;
constexpr int SIL_N_DV = 10;
constexpr int SIL_DV[SIL_N_DV] = {1, 2, 3, 4, 6, 8, 12, 16, 24, 32};   // float4 pieces per point k_sil_partial is built for
constexpr int64_t SIL_MAX_SEGMENTS = (int64_t)1 << 23;                 // a grid's x extent times 256 threads stays below 2^32
int sil_dv(int d);
int launch_silhouette(const float* x, int64_t ld, int64_t n, int d, const int64_t* offsets, int K, const int64_t* perm, void* ws,
                      double* s, hipStream_t st);
// state-gene correlation (statecorr.hip)
constexpr int SC_SEG_ROWS = 256;       // rows per segment at most: a longer group is cut into pieces of this many
constexpr int SC_TILE = 256;           // genes per workgroup of k_sc_partial: one wave, four consecutive genes a lane
constexpr int SC_MAX_S = 32;           // the model's limit on state_dim; more passes of 4, 2 or 1 states, not more registers
constexpr int64_t SC_MAX_BLOCKS = ((int64_t)1 << 31) - 1;              // segments x gene tiles, and groups x gene tiles, one grid each
int launch_state_corr(const float* data, int64_t ld, int64_t n_total, int D, const int64_t* rows, const float* state, int64_t lds,
                      int64_t n, int S, const int64_t* offsets, int G, void* ws, double* r, int64_t* count, bool wide, hipStream_t st);
// rank sums of every gene, each group against the rest (ranksum.hip)
constexpr int RS_MAX_N = MMVAE_RANKSUM_MAX_N;   // cells of one call: their 4-byte keys, padded to a power of two, are 128 KiB of LDS
constexpr int RS_MAX_G = 4096;         // groups of one call: their offsets lie in LDS beside the keys (16 KiB)
constexpr int RS_THREADS = 1024;       // threads of k_rs_rank at most (half the padded keys where those are fewer)
constexpr int RS_BIG = 1024;           // a group of more cells is reduced by the whole workgroup, a smaller one by one wave
constexpr int RS_CHUNK = 512;          // genes staged gene-major at a time: two workgroups for each of the 256 CUs
// the order-preserving key of a float: a < b exactly where key(a) < key(b); -0.0 and +0.0 share a key; -inf lowest, +inf highest
__host__ __device__ inline uint32_t rs_key(float v) {
    uint32_t b = __builtin_bit_cast(uint32_t, v);
    if ((b << 1) == 0) b = 0;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
int rs_pow2(int64_t n);                // the padded number of keys: the power of two from 128 up that holds n
inline size_t rs_lds_bytes(int64_t n, int G) { return 4 * ((size_t)rs_pow2(n) + (size_t)G + 1); }
int launch_rank_sum(const float* x, int64_t ld, int64_t n_total, int D, const int64_t* rows, int n, const int64_t* offsets, int G,
                    float eps, void* ws, int64_t* rank_sum2, int64_t* tie_term, int64_t* n_pos, double* sum, hipStream_t st);
// The blocked path.  Its cap of 2^20 cells is what the outputs' formats hold, not a buffer's size: a gene with every value tied
// has the tie term n^3 - n < 2^60, which an int64 holds; lo + hi + 1 <= 2 n + 1 < 2^22 fits the uint32 kept per cell; and a
// group's sum of them stays below 2^42, so that U minus its mean is exact in fp64 on the host, as z_and_p assumes.
constexpr int RSB_MAX_N = MMVAE_RANKSUM_BLOCKED_MAX_N;
constexpr int RSB_MIN_BLOCK = 128;     // the smallest block of cells: the smallest number of padded keys of the sort
constexpr int RSB_THREADS = 1024;      // threads of k_rsb_rank
constexpr int RSB_CELLS = 4;           // cells a thread of k_rsb_rank carries: key, lo and hi in registers
constexpr int RSB_TILE = RSB_THREADS * RSB_CELLS;   // cells per workgroup of k_rsb_rank; one partial of the tie term each
constexpr size_t RSB_WS_BYTES = (size_t)4 << 30;    // the workspace at most: the gene chunk shrinks with n to stay below it
enum { RSB_FORM_AUTO = -1, RSB_FORM_STAGED = 0, RSB_FORM_IN_PLACE = 1 };
// a gene's share of the workspace: the staged values, the sorted keys and lo + hi + 1 (4 bytes a cell each), the tile partials
inline size_t rsb_gene_bytes(int64_t n) { return 12 * (size_t)n + 8 * (size_t)((n + RSB_TILE - 1) / RSB_TILE); }
inline int rsb_chunk(int64_t n, int D) {
    size_t c = RSB_WS_BYTES / rsb_gene_bytes(n);                        // (at least 341: n <= RSB_MAX_N)
    if (c > (size_t)RS_CHUNK) c = RS_CHUNK;
    return (size_t)D < c ? D : (int)c;
}
int launch_rank_sum_blocked(const float* x, int64_t ld, int64_t n_total, int D, const int64_t* rows, int n, const int64_t* offsets,
                            int G, float eps, int L, void* ws, int64_t* rank_sum2, int64_t* tie_term, int64_t* n_pos, double* sum,
                            int form, int phases, hipStream_t st);
// k nearest neighbours, their votes and purity (knn.hip)
constexpr int KNN_MAX_K = MMVAE_KNN_MAX_K;
constexpr int KNN_MAX_D = SIL_MAX_D;   // k_knn_partial is built for the float4 pieces of SIL_DV
constexpr int KNN_MAX_N = MMVAE_KNN_MAX_N;      // queries, and references: an index and a list's slot stay far inside 32 bits
constexpr int KNN_MAX_CLASSES = 4096;
constexpr int KNN_LDS_FLOATS = 2048;   // floats of staged reference columns per pass (8 KiB: with the lists of k = 15, nine workgroups a CU)
constexpr int KNN_TILE = 64;           // queries per workgroup of k_knn_partial and k_knn_merge: one wave, one thread a query
constexpr int KNN_VOTE_TILE = 64;      // queries per workgroup of k_knn_votes, one thread each
constexpr int KNN_MIN_SEG = 256;       // reference columns per segment at least, where the entry chooses
constexpr int KNN_TARGET_WGS = 1024;   // workgroups of k_knn_partial aimed at: four one-wave workgroups for each of the 256 CUs
constexpr size_t KNN_WS_BYTES = (size_t)2 << 30;    // the workspace at most
enum { KNN_PHASE_ALL = 0, KNN_PHASE_PARTIAL = 1, KNN_PHASE_MERGE = 2 };
// the segment length the entry chooses: as FEW segments as fill the chip -- every segment starts its lists empty, and while a
// list fills nearly every candidate enters it -- so KNN_TARGET_WGS workgroups over the query tiles
// (the count does not depend on k, so that the workspace grows with k), no more than the workspace's cap allows, none
// shorter than KNN_MIN_SEG
inline int64_t knn_seg_cols(int64_t nq, int64_t nr, int k) {
    int64_t nseg = KNN_TARGET_WGS / cdiv64(nq, KNN_TILE);
    const int64_t cap = (int64_t)(KNN_WS_BYTES / (8 * (size_t)nq * (size_t)k));     // (at least 4: nq <= 2^20, k <= 64)
    nseg = nseg > cap ? cap : nseg;
    nseg = nseg < 1 ? 1 : nseg;
    const int64_t len = cdiv64(nr, nseg);
    return len < KNN_MIN_SEG ? KNN_MIN_SEG : len;
}
// part uint64 [nseg][k][nq] for nseg = ceil(nr / seg_cols) > 1 segments; 8 bytes (unused) for one
inline size_t knn_ws_bytes(int64_t nq, int64_t nr, int k, int64_t seg_cols) {
    const int64_t nseg = cdiv64(nr, seg_cols);
    return nseg <= 1 ? 8 : bytes_or_0((unsigned __int128)8 * (unsigned __int128)nseg * (unsigned __int128)nq * (unsigned __int128)k);
}
int launch_knn(const float* q, int64_t ldq, int64_t nq, const float* r, int64_t ldr, int64_t nr, int d, int k, const int* qgroup,
               const int* rgroup, int64_t seg_cols, void* ws, int* idx, float* dist2, int phases, hipStream_t st);
int launch_knn_votes(const int* idx, int64_t nq, int k, const int* rlabel, int64_t nr, int n_classes, const int* qlabel, int* pred,
                     double* purity, int* top2, hipStream_t st);
// Gaussian classifiers: group moments and class scores (gaussclf.hip)
constexpr int GC_SEG_ROWS = 256;       // rows per segment at most: a longer group is cut into pieces of this many
constexpr int GC_ROW_CHUNK = 32;       // rows of a segment staged in LDS at a time by k_gc_partial
constexpr int GC_N_DC = 4;
constexpr int GC_DC[GC_N_DC] = {16, 32, 64, 128};   // the largest d of each instance of k_gc_partial (1, 3, 9, 33 sums a thread)
constexpr int GC_ROW_TILE = 64;        // cells per workgroup of k_gc_scores: one cell a lane of every wave
constexpr int GC_SCORE_WAVES = 16;     // waves per workgroup of k_gc_scores at most: they share the cells and split the classes
constexpr int GC_COL_BLOCK = 8;        // columns of W whose inner products k_gc_scores carries at once
constexpr int GC_MAX_D = 128;
constexpr int GC_MAX_K = 4096;
constexpr int GC_MAX_F = 64;
constexpr int GC_MAX_G = 1 << 20;      // groups of one mmvae_group_moments call (GC_MAX_K x GC_MAX_F fits four times)
int gc_dclass(int d);
int launch_group_moments(const float* x, int64_t ld, int64_t n, int d, const int64_t* offsets, int G, const float* pivot, void* ws,
                         double* s, double* M, int dclass, hipStream_t st);
int launch_gauss_scores(const float* x, int64_t ld, int64_t n, int d, const int* model, int F, int K, const double* mu,
                        const double* W, const double* c0, const int64_t* perm, int* label, double* best, double* second,
                        double* scores, hipStream_t st);
// leaf posteriors merged up a tree (leafmerge.hip)
constexpr int LM_WAVES = 4;            // waves per workgroup of k_lm_normalise and k_lm_merge: one cell a wave
constexpr int LM_MAX_L = GC_MAX_K;     // leaves: the classes one mmvae_gauss_scores call can score
constexpr int LM_MAX_K = 4096;         // labels of one merge level
constexpr int LM_MAX_T = 4096;         // merge levels of one call
constexpr int LM_MAX_GRID = 1 << 20;   // workgroups along the cells at most: a workgroup strides over the rest
int launch_leaf_merge(double* p, int64_t ldp, int64_t n, int L, const int* level_start, int T, const int* start, int K_total,
                      int K_max, const int* leaf, int nnz, int* label, double* prob, double* second, double* merged, int K0,
                      hipStream_t st);
// zero-inflated negative binomial heads, terms and sums (zinb.hip)
constexpr int ZB_MAX_H = 128;          // the K extent one LDS tile holds
template <int NH>
struct ZbHeads {
    const float* W[NH];      // [D, H] each, nn.Linear's layout
    const float* b[NH];      // [D]
};
// what the entries on d10 and X share: d10 [N, H] at pitch ldh, the heads fc11, fc11_p, fc11_r, X [N, D] at pitch ldx; the
// gradient entries read scale, mask (the selected heads, bits 1, 2, 4) and segments (0 = the launcher's rule) as well
struct ZinbIn {
    const float* d10;
    int64_t ldh, N;
    int H, D;
    ZbHeads<3> hd;
    const float* X;
    int64_t ldx;
    double eps, scale;
    int mask, segments;
};
// the outputs of the gradient entries: dW_j [D, H], db_j [D] of the selected heads and the term's sums (mmvae_zinb_head_grads),
// gd10 [N, H] at pitch ldg (mmvae_zinb_d10_grad); mmvae_zinb_step_grads has both
struct ZinbGradOut {
    float* dW[3];
    float* db[3];
    double *cell_sum, *gene_sum;
    float* gd10;
    int64_t ldg;
};
size_t zb_ws_bytes(int64_t N, int D);  // the partial sums of the 32 x 32 sub-tiles; 0 for a size no size_t holds
int64_t zb_tiles(int64_t N, int D);    // the workgroups of one grid; 0 where a grid cannot hold them
int launch_zinb_heads(const float* d10, int64_t ldh, int64_t N, int H, int D, const float* Wp, const float* bp, const float* Wr,
                      const float* br, float* x_p, float* x_r, int64_t ldo, hipStream_t st);
int launch_zinb_nll(const ZinbIn& in, void* ws, double* cell_sum, double* gene_sum, hipStream_t st);
int launch_zinb_terms(const float* x_rec, int64_t ld_rec, const float* x_p, int64_t ld_p, const float* x_r, int64_t ld_r, const float* X,
                      int64_t ldx, int64_t N, int D, double eps, void* ws, double* cell_sum, double* gene_sum, float* terms,
                      int64_t ld_t, hipStream_t st);
// the sub-tiles' partials of zb_reduce (zb_tile.hpp) added in tile order: cell_sum [N], gene_sum [D]
int zb_finish(void* ws, int64_t N, int D, double* cell_sum, double* gene_sum, hipStream_t st);
// gradients of the ZINB term with respect to the heads (zinb_grad.hip); segments: 0 = the launcher's rule
int zg_segments(int64_t N, int D, int asked, int* tiles_per_seg);   // the cell segments of a call (and the cell tiles of one)
size_t zg_ws_bytes(int64_t N, int D, int H, int asked);             // zb_ws_bytes, then the segments' partials; 0 as zb_ws_bytes
int64_t zg_tiles(int64_t N, int D, int asked);                      // the workgroups of one grid; 0 where a grid cannot hold them
// with out.gd10 the same pass leaves gd10 too (k_zg_step), at a segment a gene tile: ws is zs_ws_bytes then, zg_ws_bytes without
int launch_zinb_head_grads(const ZinbIn& in, void* ws, const ZinbGradOut& out, hipStream_t st);
int launch_zinb_terms_grad(const float* x_rec, int64_t ld_rec, const float* x_p, int64_t ld_p, const float* x_r, int64_t ld_r,
                           const float* X, int64_t ldx, int64_t N, int D, double eps, double scale, float* g_rec, float* g_p, float* g_r,
                           int64_t ld_g, hipStream_t st);
// the gradient with respect to d10 (zinb_grad.hip): the segments are of the gene tiles here
int zd_segments(int64_t N, int D, int asked, int* tiles_per_seg);
size_t zd_ws_bytes(int64_t N, int D, int H, int asked);             // the segments' partials; 0 for a size no size_t holds
int64_t zd_tiles(int64_t N, int D, int asked);                      // the workgroups of one grid; 0 where a grid cannot hold them
int launch_zinb_d10_grad(const ZinbIn& in, void* ws, float* gd10, int64_t ldg, hipStream_t st);
size_t zs_ws_bytes(int64_t N, int D, int H, int asked);             // zg_ws_bytes, then the gene tiles' partials of gd10
// the decoder trunk's backward from gd10 (zinb_trunk.hip); act / ld: zin, d6 .. d10; W: fc6 .. fc10; grads: dW6, db6, .. db10
constexpr int TR_MAX_W = 128;          // H and L at most: a row of dZ in LDS
constexpr int TR_MAX_SEG = 1024;       // cell segments one call may ask for
int tr_segments(int64_t N, int asked, int64_t* cells_per_seg);
size_t tr_ws_bytes(int64_t N, int Z, int L, int H, int asked);
int launch_decoder_trunk_grads(int64_t N, int Z, int L, int H, const float* const* act, const int64_t* ld, const float* const* W,
                               const float* gd10, int64_t ldg, int segments, void* ws, float* const* grads, float* gzin, int64_t ldgz,
                               hipStream_t st);
// zrec[a] = (the sum of cell_sum[a][0 .. N) in a fixed order) / (N D): zinb_loss of every arm (zinb_grad.hip)
int launch_zinb_rec(const double* cell_sum, int A, int64_t N, int D, double* zrec, hipStream_t st);
void host_zinb_grad(int64_t n, const float* X, const float* a_rec, const float* a_p, const float* a_r, double eps, double* g, double* term);
void host_digamma(int64_t n, const double* x, double* out);
// count distributions (countdist.hip); the host_ pair runs the element code on the host
int launch_count_logp(const mmvae_count_logp_t& a, void* ws, hipStream_t st);
int launch_count_sample(const mmvae_count_sample_t& s, hipStream_t st);
int launch_zinb_sample(const float* d10, int64_t ldh, int H, const float* W, const float* b, const float* Wp, const float* bp,
                       const float* Wr, const float* br, const mmvae_count_sample_t& s, hipStream_t st);
void host_count_logp(const mmvae_count_logp_t& a);
void host_count_sample(const mmvae_count_sample_t& s);
// random forest on 256-bin features (forest.hip)
constexpr int RF_THREADS = 256;        // threads of every workgroup: k_rf_fit one tree, k_rf_predict four rows (one a wave)
constexpr int RF_BINS = 256;           // bins of a feature: one a thread of the candidate search, four a lane of the scan
constexpr int RF_MAX_D = 128;
constexpr int RF_MAX_K = 128;          // the class x bin histogram of uint32 in LDS: 128 KiB at most, 21.5 KiB of partial sums
constexpr int RF_MAX_F = 64;
constexpr int RF_MAX_T = 4096;         // trees a fold
constexpr int64_t RF_MAX_N = (int64_t)1 << 24;   // rows: n^2 exact in a double, 2 n nodes and F n rows in an int
constexpr int64_t RF_TREE_BYTES_PER_ROW = 56;    // a tree's tables per row of the call: 2 nodes and 1 stack entry of 16, 2 list entries of 4
constexpr int64_t RF_CHUNK_BYTES = (int64_t)1 << 30;   // per-tree tables of one chunk of launches at most (at least one tree)
int rf_chunk(int64_t n, int F, int T);
size_t rf_ws_bytes(int64_t n, int F, int K, int T);
int launch_forest(const uint8_t* bins, int64_t ld, int64_t n, int d, const int* codes, const int* fold, int K, int F, int T,
                  int mtry, uint64_t seed, void* ws, int* label, int* best, int* second, int* votes, int* tree_count,
                  int* tree_nodes, hipStream_t st);
// principal components: Gram matrix on the fp64 MFMA, block product, projection (pca.hip)
constexpr int GRAM_TILE = 64;          // rows and columns of G per workgroup of k_gram_partial: four waves of 32 x 32
constexpr int GRAM_KC = 32;            // rows of the data staged in LDS at a time: eight MFMA steps of four
constexpr int GRAM_PITCH = 80;         // doubles per staged row: the four rows an MFMA operand reads fall on disjoint banks
constexpr int GRAM_SEG_ROWS = 256;     // rows per segment, where the rows are cut at all and until GRAM_MAX_SEGS are in use
constexpr int GRAM_MAX_SEGS = 3;       // segments at most: the first lands in G, the others in the workspace (2 G at most)
constexpr int GRAM_FILL_TILES = 256;   // upper-triangle tiles from which the rows are not cut: one workgroup a compute unit
constexpr int GRAM_MAX_D = 32768;
constexpr int RM_ROWS = 16;            // rows per workgroup of k_rows_mul: four a wave
constexpr int RM_CHUNK = 64;           // coordinates staged at a time, and the most columns of the block (b, k <= 64)
int gram_segments(int64_t n, int D, int64_t* seg_rows);
int launch_gram(const float* data, int64_t ld, int64_t n_total, const int64_t* rows, int64_t n, int D, const float* pivot, void* ws,
                double* s, double* G, int cov, bool wide, hipStream_t st);
int launch_symm_mul(const double* C, int64_t ldc, int D, const double* Q, int b, double* Y, hipStream_t st);
int launch_pca_project(const float* data, int64_t ld, int64_t n_total, const int64_t* rows, int64_t n, int D, const double* mean,
                       const double* V, int k, double* Z, hipStream_t st);
// data preparation: normalise / log-CPM from dense or CSR counts, per-gene statistics (dataprep.hip)
constexpr int CPM_THREADS = 256;       // threads of a workgroup of k_cpm_dense / k_cpm_csr: one workgroup a selected row
constexpr int CPM_WINDOW = 4096;       // columns of the dense row that k_cpm_csr rebuilds in LDS at a time (32 KiB)
constexpr int CPM_MAX_G = 1 << 20;     // genes at most: an int32 row sums to below 2^51, exact in a double
constexpr int GS_SEG_ROWS = 256;       // rows per segment of k_gs_partial
constexpr int GS_TILE = 256;           // genes per workgroup of k_gs_partial: one wave, four consecutive genes a lane
constexpr int64_t GS_MAX_BLOCKS = ((int64_t)1 << 31) - 1;              // segments x gene tiles of one grid
int launch_cpm_dense(const void* x, int vtype, int64_t ld, int64_t n_total, int G, const int64_t* rows, int64_t n, const int* genes,
                     int ng, double scaler, int log_mode, void* out, int otype, double* norms, bool wide, hipStream_t st);
int launch_cpm_csr(const int64_t* indptr, const int* indices, const void* data, int vtype, int64_t nnz, int64_t n_total, int G,
                   const int64_t* rows, int64_t n, const int* inv, int ng, double scaler, int log_mode, void* out, int otype,
                   double* norms, hipStream_t st);
int64_t gs_nseg(int64_t n);
int launch_gene_stats(const void* data, int vtype, int64_t ld, int64_t n_total, int D, const int64_t* rows, int64_t n, double eps,
                      void* ws, int64_t* n_above, double* mean, double* sd, bool wide, hipStream_t st);
int launch_dump_noise(const mmvae_dims& d, const mmvae_hyper& h, const mmvae_noise* nz, uint8_t* x_mask,
                      float* u_gumbel, float* u_state, uint8_t* s_mask, hipStream_t s);

}  // namespace mmvae

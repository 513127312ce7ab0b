// The latent block's forward kernel (k_lat_fwd_g) with what it shares with the backward kernel (LatArgs, LatCell, the noise
// readers) and its host-side arguments.  A header, because two translation units instantiate the kernel: rowwise.hip the
// forward pass's forms, encode.hip mmvae_encode's -- instantiated side by side in one unit, the forward pass's forms
// compiled to other code than without their siblings.
#ifndef MMVAE_LAT_FWD_HPP
#define MMVAE_LAT_FWD_HPP
#include "common.hpp"
#include "couple.hpp"   // CPL
#include <type_traits>
#include <math.h>

namespace mmvae {

// ---------------------------------------------------------------------------------------------
struct LatArgs {
    int A, B, L, C, S;
    float tau, temp, eps, s_drop;
    int hard, training, eval_flag;
    int64_t per_arm, o_wc, o_bc, o_wms, o_bms;
    // workspace offsets
    int64_t R5, mean5, rstd5, XLOW, CPROB, CC, YSOFT, CSMP, Y, MS, MU, LV, SS, ZIN, c_part, lat_part;
    // backward only
    int64_t GZIN, GMS, GZC, G5, bnb_part5, T, c_mean, c_iv;
    float am1, beta, lam;
    int32_t* labels;   // non-null (eval): labels[arm * B + b] = argmax_k c, the `classify` of the consensus path
    // forward, training: BN5's partials [A][nblk][2][L] are recombined by every row block
    int64_t bn_part5, run_mean_off, run_var_off, run_arm_stride;
    int bn5_n;             // partials fc5's launch emitted (one per CHAIN_ROWS cells)
    int64_t acc_bn5, acc_bnb5;   // accumulator sets ([A] each) instead of bn_part5 (read) / bnb_part5 (added to); -1 = partials
    int64_t acc_c, acc_T;        // ... instead of c_part (added to by the forward kernels) / T (read by the backward kernels)
    float bn_momentum;
    // category subset of the pruning-time forward (nn_model.py:332-335: c = softmax(c_prob[:, mask] / tau) on the kept
    // categories, 0 elsewhere): bit k of cmask = category k is kept; use_mask == 0: all of them
    uint32_t cmask[4];
    int use_mask;
};
__device__ __forceinline__ bool cat_kept(const LatArgs& a, int col) {
    return !a.use_mask || ((a.cmask[(col >> 5) & 3] >> (col & 31)) & 1u) != 0u;
}

__device__ __forceinline__ float gumbel_u(const NoiseDev& nz, int arm, int B, int C, int b, int col) {
    if (nz.mode == 0) return nz.u_gumbel[((int64_t)arm * B + b) * C + col];
    return noise_uniform(nz, arm, STREAM_GUMBEL, (uint64_t)b * C + col);
}
__device__ __forceinline__ float state_u(const NoiseDev& nz, int arm, int B, int S, int b, int s) {
    if (nz.mode == 0) return nz.u_state[((int64_t)arm * B + b) * S + s];
    return noise_uniform(nz, arm, STREAM_STATE, (uint64_t)b * S + s);
}
__device__ __forceinline__ bool state_keep(const NoiseDev& nz, int arm, int B, int S, int b, int s) {
    if (nz.mode == 0) return nz.s_mask[((int64_t)arm * B + b) * S + s] != 0;
    return noise_keep(nz, arm, STREAM_SMASK, (uint64_t)b * S + s, nz.s_keep_thr);
}

// ---------------------------------------------------------------------------------------------
// The latent block, forward (lat_fwd) and backward (lat_bwd): one body each, compiled for two cell geometries.  A cell
// (one row of the batch) lives on W lanes of a wave, CP column registers in each; a wave instruction serves CPW = 64 / W
// cells; a wave carries NR such cell groups side by side; NW waves per workgroup.  NW x CPW x NR = LAT_ROWS (forward) /
// LAT_ROWS_BWD (backward, common.hpp) cells per workgroup in either geometry, so the partial layouts, the grids and the
// workspace do not depend on it.
//                                                  W    NW x CPW x NR
constexpr int LAT_NW = 16, LAT_NR = LAT_ROWS / LAT_NW;             // k_lat_fwd     64   16 x 1 x 3
constexpr int LH_NW = 8, LH_NR = LAT_ROWS / (LH_NW * 2);           // k_lat_fwd_h   32    8 x 2 x 3
constexpr int LATB_NW = 8, LATB_NR = LAT_ROWS_BWD / LATB_NW;       // k_lat_bwd     64    8 x 1 x 1
constexpr int LBH_NW = 4, LBH_NR = LAT_ROWS_BWD / (LBH_NW * 2);    // k_lat_bwd_h   32    4 x 2 x 1
static_assert(LAT_NR * LAT_NW == LAT_ROWS && LH_NR * LH_NW * 2 == LAT_ROWS, "LAT_ROWS must be a multiple of 16");
static_assert(LATB_NR * LATB_NW == LAT_ROWS_BWD && LBH_NR * LBH_NW * 2 == LAT_ROWS_BWD, "LAT_ROWS_BWD must be a multiple of 8");

// Cell geometry.  W = 64, the wave form: the wave is one cell, 64 lanes x CPL = 128 column slots (C <= 128, L <= 64,
// 2 S <= 64).  W = 32, the half-wave form (make_plan picks it for C <= 96, L <= 32, 2 S <= 32 -- the reference's 92 / 10 /
// 2): 32 lanes x LH_CPL = 96 column slots for 92 categories.  These kernels are VALU-bound (a wave instruction occupies
// its SIMD for four cycles): three registers for two cells instead of two for one is a quarter less element-wise work,
// and a reduction is one step shorter (group_allreduce, common.hpp) and counts for two cells.
template <int W>
struct LatCell {
    static_assert(W == 64 || W == 32, "a cell is the wave or half of it");
    static constexpr int CPW = 64 / W;                    // cells served by one wave instruction
    static constexpr int CP = W == 64 ? CPL : LH_CPL;     // column registers per lane: column sub + W t in register t
    static __device__ __forceinline__ int sub(int lane) { return lane & (W - 1); }     // lane within the cell
    static __device__ __forceinline__ int base(int lane) { return lane & (64 - W); }   // the cell's first lane (shuffle sources)
    static __device__ __forceinline__ int cell(int lane) { return lane / W; }          // cell within the wave
    static __device__ __forceinline__ float sum(float v) { return group_sum<W>(v); }   // over the cell's lanes
    static __device__ __forceinline__ float max(float v) { return group_max<W>(v); }
    static __device__ __forceinline__ int min_i(int v) { return group_min_i<W>(v); }
};

// Addressing of the latent kernels' per-cell arrays ([A, B, width] floats in the workspace): one wave-uniform base per
// array AT THE WORKGROUP'S FIRST CELL (a buffer descriptor for loads, a pointer for stores; both from kernel arguments and
// blockIdx alone, so they are computed on the scalar unit and live in SGPRs) and a 32-bit byte offset per lane -- no 64-bit
// multiply-add per access.  A workgroup owns at most LAT_ROWS cells of at most 256 floats (check_dims: C + S, L + C <= 255,
// 2 S <= 64), so a byte offset stays below LAT_BLOCK_BYTES whatever B is and never reaches LAT_OOB, the offset a lane
// without an element asks for: beyond the descriptor's range, where a buffer load returns 0 and touches no memory.
// Loads only; stores stay guarded by their predicate.
constexpr uint32_t LAT_BLOCK_BYTES = (uint32_t)LAT_ROWS * 256u * 4u, LAT_OOB = 0x80000000u;
static_assert(LAT_ROWS_BWD <= LAT_ROWS && LAT_BLOCK_BYTES < LAT_OOB && (uint64_t)LAT_BLOCK_BYTES + LAT_OOB <= 0xFFFFFFFFull,
              "32-bit byte offsets within a workgroup's cells");
// rows x width floats at p
__device__ __forceinline__ __amdgpu_buffer_rsrc_t lat_rsrc(const float* p, int rows, int width) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p), 0, rows * width * 4, 0x00020000);
}
__device__ __forceinline__ float lat_ld(__amdgpu_buffer_rsrc_t rs, uint32_t byte_off) {
    return __builtin_bit_cast(float, (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rs, (int)byte_off, 0, 0));
}
__device__ __forceinline__ void lat_st(float* base, uint32_t byte_off, float v) {
    *reinterpret_cast<float*>(reinterpret_cast<char*>(base) + byte_off) = v;
}

// Stages fcc (transposed to [L][C]) and the state-head weights in LDS once per workgroup.
__device__ __forceinline__ void lat_stage_weights(float* WcT, float* Wm, const float* __restrict__ Wc,
                                                  const float* __restrict__ Wms, int L, int C, int S) {
    for (int i = threadIdx.x; i < C * L; i += blockDim.x) {
        const int col = i / L, k = i % L;
        WcT[k * C + col] = Wc[i];
    }
    for (int i = threadIdx.x; i < 2 * S * (L + C); i += blockDim.x) Wm[i] = Wms[i];
    __syncthreads();
}

// Forward.  grid (ceil(B/LAT_ROWS), A), 64 NW threads; cell slot r (NW CPW) + wv CPW + cell of the workgroup is cell group
// r of wave wv -- all NR of them side by side: the per-cell work is one long dependency chain (three softmaxes = six
// reductions, the Gumbel transform, four state-head dot products), and a wave that walks its cells one after the other
// spends most of its time waiting on that chain (measured: 15 k cycles per cell with 4 waves per SIMD).
//
//
//
// ENC (mmvae_encode, launch_lat_enc): 0 the forward pass's kernel, with the forward pass's arguments and nothing else; 1 takes
// an EncOut (common.hpp) behind them and additionally stores the outputs the caller asked for at the caller's rows; 2 the
// encoder's head: x_low and c_prob into the EncOut, then it returns -- no second softmax, no sample, no state head.  The
// arithmetic is this one body's in every form, so what an encode returns is a forward's bit for bit.
struct NoEnc {};
__device__ __forceinline__ NoEnc enc_out() { return {}; }
__device__ __forceinline__ const EncOut& enc_out(const EncOut& e) { return e; }
template <int W, int NW, int ENC = 0, class... Enc>
__global__ __launch_bounds__(64 * NW) void k_lat_fwd_g(const LatArgs a_in, const NoiseDev nz_in, const float* __restrict__ params,
                                                      float* __restrict__ ws, float* __restrict__ bn_running, int64_t* __restrict__ nbt,
                                                      const Enc... enc) {
    static_assert(sizeof...(Enc) == (ENC != 0 ? 1 : 0), "the encode forms take one EncOut, the forward pass's none");
    [[maybe_unused]] const auto& eo = enc_out(enc...);
    using Cell = LatCell<W>;
    constexpr int CPW = Cell::CPW, CP = Cell::CP, NR = LAT_ROWS / (NW * CPW), NT = 64 * NW;
    static_assert(NR * NW * CPW == LAT_ROWS && NT % 128 == 0 && LAT_ROWS % (NT / 128) == 0, "cells per workgroup");
    const LatArgs a = a_in;
    const NoiseDev nz = nz_in;
    extern __shared__ __attribute__((aligned(16))) float lat_smem[];
    __shared__ __attribute__((aligned(16))) float sh_buf[LAT_ROWS * 128];   // prologue scratch, then the c tile
    __shared__ float sh_ps[NT / 128][128];
    __shared__ float sh_red[NW][2], sh_bn5[2][64];
    const int arm = blockIdx.y, blk = blockIdx.x, b0 = blk * LAT_ROWS;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int sub = Cell::sub(lane), base = Cell::base(lane), cell = Cell::cell(lane);
    const int B = a.B, L = a.L, C = a.C, S = a.S;
    const float* P = params + (int64_t)arm * a.per_arm;
    float* WcT = lat_smem;            // [L][C]
    float* Wms = lat_smem + C * L;    // [2S][L+C]
    const int64_t ab = (int64_t)arm * B;
    const int64_t ab0 = ab + b0;                 // the workgroup's first cell (lat_ld / lat_st above)
    const int nrows = min(LAT_ROWS, B - b0);     // its cells within the batch
    const float eps = a.eps;

    int slot[NR], bb[NR];
    bool okr[NR];
    float r5[NR];
    {
        const auto rR5 = lat_rsrc(ws + a.R5 + ab0 * L, nrows, L);
        const uint32_t lob = sub < L ? (uint32_t)sub * 4u : LAT_OOB;
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            slot[r] = r * (NW * CPW) + wv * CPW + cell;
            bb[r] = b0 + slot[r];
            okr[r] = bb[r] < B;                   // per cell
            r5[r] = lat_ld(rR5, (uint32_t)min(slot[r], nrows - 1) * (uint32_t)L * 4u + lob);   // beyond the batch: the last cell's
        }
    }
    bool vcol[CP];
    float bcv[CP];
    {
        const auto rBC = lat_rsrc(P + a.o_bc, 1, C);
#pragma unroll
        for (int t = 0; t < CP; ++t) {
            vcol[t] = sub + W * t < C;
            bcv[t] = lat_ld(rBC, vcol[t] ? (uint32_t)(sub + W * t) * 4u : LAT_OOB);
        }
    }
    // stores: the workgroup's first row of every array + a 32-bit byte offset
    float* const pXLOW = ws + a.XLOW + ab0 * L;
    float* const pY = ws + a.Y + ab0 * (L + C);
    float* const pZIN = ws + a.ZIN + ab0 * (C + S);
    lat_stage_weights(WcT, Wms, P + a.o_wc, P + a.o_wms, L, C, S);
    const float* bms = P + a.o_bms;

    if (a.bn_part5 >= 0) {
        float mean, m2;
        if (a.acc_bn5 >= 0) {
            mean = m2 = 0.f;
            if ((int)threadIdx.x < L)
                acc_mean_m2(reinterpret_cast<const long long*>(ws + a.acc_bn5) + (int64_t)arm * ACC_SET_I64, threadIdx.x, B, mean, m2);
        } else {
            stats_from_partials<NT>(ws + a.bn_part5 + (int64_t)arm * a.bn5_n * 2 * L, a.bn5_n, B, CHAIN_ROWS, L, sh_buf, mean, m2);
        }
        if (threadIdx.x < L) {
            const int t = threadIdx.x;
            const float rstd = 1.0f / sqrtf(m2 / (float)B + eps);
            sh_bn5[0][t] = mean;
            sh_bn5[1][t] = rstd;
            if (blk == 0) {
                ws[a.mean5 + arm * L + t] = mean;
                ws[a.rstd5 + arm * L + t] = rstd;
                if (bn_running) {
                    float* rm = bn_running + a.run_mean_off + arm * a.run_arm_stride;
                    float* rv = bn_running + a.run_var_off + arm * a.run_arm_stride;
                    rm[t] = (1.f - a.bn_momentum) * rm[t] + a.bn_momentum * mean;
                    rv[t] = (1.f - a.bn_momentum) * rv[t] + a.bn_momentum * (m2 / (float)max(B - 1, 1));
                }
                if (nbt && t == 0) nbt[arm * MMVAE_N_BN + 4] += 1;
            }
        }
        lds_barrier();
    }
    const float mu5 = sub < L ? (a.bn_part5 >= 0 ? sh_bn5[0][sub] : ws[a.mean5 + arm * L + sub]) : 0.f;
    const float rs5 = sub < L ? (a.bn_part5 >= 0 ? sh_bn5[1][sub] : ws[a.rstd5 + arm * L + sub]) : 0.f;

    // ---- x_low = BN5(R5)
    float xl[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        xl[r] = sub < L ? (r5[r] - mu5) * rs5 : 0.f;
        if (okr[r] && sub < L) {
            lat_st(pXLOW, ((uint32_t)slot[r] * (uint32_t)L + (uint32_t)sub) * 4u, xl[r]);
            lat_st(pY, ((uint32_t)slot[r] * (uint32_t)(L + C) + (uint32_t)sub) * 4u, xl[r]);
            if constexpr (ENC != 0)
                if (eo.x_low) eo.x_low[((int64_t)arm * eo.rows + eo.row0 + bb[r]) * L + sub] = xl[r];
        }
    }
    // ---- zc = fcc(x_low); c_prob = softmax(zc)
    float z[NR][CP];
#pragma unroll
    for (int r = 0; r < NR; ++r)
#pragma unroll
        for (int t = 0; t < CP; ++t) z[r][t] = bcv[t];
    for (int k = 0; k < L; ++k) {
        float w[CP];
#pragma unroll
        for (int t = 0; t < CP; ++t) w[t] = vcol[t] ? WcT[k * C + sub + W * t] : 0.f;
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const float xk = __shfl(xl[r], base + k, 64);   // this lane's own cell
#pragma unroll
            for (int t = 0; t < CP; ++t) z[r][t] += xk * w[t];
        }
    }
    float m[NR], ssum[NR], e[NR][CP];
    float cp[NR][CP], cc[NR][CP], lc[NR][CP], ys[NR][CP], cs[NR][CP];
    auto softmax_rows = [&](float (&v)[NR][CP], float (&out)[NR][CP]) {
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            m[r] = -INFINITY;
#pragma unroll
            for (int t = 0; t < CP; ++t) if (vcol[t]) m[r] = fmaxf(m[r], v[r][t]);
        }
#pragma unroll
        for (int r = 0; r < NR; ++r) m[r] = Cell::max(m[r]);
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            ssum[r] = 0.f;
#pragma unroll
            for (int t = 0; t < CP; ++t) { e[r][t] = vcol[t] ? expf(v[r][t] - m[r]) : 0.f; ssum[r] += e[r][t]; }
        }
#pragma unroll
        for (int r = 0; r < NR; ++r) ssum[r] = Cell::sum(ssum[r]);
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const float inv = 1.f / ssum[r];
#pragma unroll
            for (int t = 0; t < CP; ++t) out[r][t] = e[r][t] * inv;
        }
    };
    softmax_rows(z, cp);
    if constexpr (ENC == 2) {
        if (eo.c_prob) {
#pragma unroll
            for (int r = 0; r < NR; ++r)
#pragma unroll
                for (int t = 0; t < CP; ++t)
                    if (okr[r] && vcol[t]) eo.c_prob[((int64_t)arm * eo.rows + eo.row0 + bb[r]) * C + sub + W * t] = cp[r][t];
        }
        return;
    }
    // ---- c = softmax(c_prob / tau)
    const float inv_tau = 1.f / a.tau, inv_temp = 1.f / a.temp;
    float tmp[NR][CP];
#pragma unroll
    for (int r = 0; r < NR; ++r)
#pragma unroll
        for (int t = 0; t < CP; ++t) tmp[r][t] = cat_kept(a, sub + W * t) ? cp[r][t] * inv_tau : -INFINITY;   // masked-out: exp(-inf) = 0
    softmax_rows(tmp, cc);
#pragma unroll
    for (int r = 0; r < NR; ++r)
#pragma unroll
        for (int t = 0; t < CP; ++t) lc[r][t] = logf(cc[r][t] + eps);
    // ---- Gumbel-softmax sample
    bool hard = a.hard != 0;
    if (a.eval_flag) {
        hard = true;
#pragma unroll
        for (int r = 0; r < NR; ++r)
#pragma unroll
            for (int t = 0; t < CP; ++t) ys[r][t] = cc[r][t];
    } else {
#pragma unroll
        for (int r = 0; r < NR; ++r)
#pragma unroll
            for (int t = 0; t < CP; ++t) {
                tmp[r][t] = 0.f;
                if (vcol[t]) {
                    const float U = gumbel_u(nz, arm, B, C, min(bb[r], B - 1), sub + W * t);
                    const float g = -logf(-logf(U + eps) + eps);
                    tmp[r][t] = (lc[r][t] + g) * inv_temp;
                }
            }
        softmax_rows(tmp, ys);
    }
    if (hard) {
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            float mv = -INFINITY;
#pragma unroll
            for (int t = 0; t < CP; ++t) if (vcol[t]) mv = fmaxf(mv, ys[r][t]);
            mv = Cell::max(mv);
            int cand = 1 << 30;
#pragma unroll
            for (int t = 0; t < CP; ++t) if (vcol[t] && ys[r][t] == mv) cand = min(cand, sub + W * t);
            cand = Cell::min_i(cand);
            if (a.labels && a.eval_flag && okr[r] && sub == 0) a.labels[ab + bb[r]] = cand;    // eval: ys == c
            if constexpr (ENC == 1)
                if (eo.labels && okr[r] && sub == 0) eo.labels[(int64_t)arm * eo.rows + eo.row0 + bb[r]] = cand;
#pragma unroll
            for (int t = 0; t < CP; ++t) {
                const float hv = (sub + W * t == cand) ? 1.f : 0.f;
                cs[r][t] = (hv - ys[r][t]) + ys[r][t];   // (y_hard - y).detach() + y, nn_model.py:492
            }
        }
    } else {
#pragma unroll
        for (int r = 0; r < NR; ++r)
#pragma unroll
            for (int t = 0; t < CP; ++t) cs[r][t] = ys[r][t];
    }
    // ---- store; c goes to the workgroup tile for the block statistics (zero rows beyond the batch)
    float kl_acc = 0.f, ent_acc = 0.f;
    float* const pCPROB = ws + a.CPROB + ab0 * C;
    float* const pCC = ws + a.CC + ab0 * C;
    float* const pYSOFT = ws + a.YSOFT + ab0 * C;
    float* const pCSMP = ws + a.CSMP + ab0 * C;
#pragma unroll
    for (int r = 0; r < NR; ++r) {
#pragma unroll
        for (int t = 0; t < CP; ++t) {
            const int col = sub + W * t;
            sh_buf[slot[r] * 128 + col] = (okr[r] && vcol[t]) ? cc[r][t] : 0.f;
            if (okr[r] && vcol[t]) {
                const uint32_t o = ((uint32_t)slot[r] * (uint32_t)C + (uint32_t)col) * 4u;
                lat_st(pCPROB, o, cp[r][t]);
                lat_st(pCC, o, cc[r][t]);
                lat_st(pYSOFT, o, ys[r][t]);
                lat_st(pCSMP, o, cs[r][t]);
                lat_st(pY, ((uint32_t)slot[r] * (uint32_t)(L + C) + (uint32_t)(L + col)) * 4u, cs[r][t]);
                lat_st(pZIN, ((uint32_t)slot[r] * (uint32_t)(C + S) + (uint32_t)col) * 4u, cs[r][t]);
                if constexpr (ENC == 1) {
                    const int64_t eo_o = ((int64_t)arm * eo.rows + eo.row0 + bb[r]) * C + col;
                    if (eo.c_prob) eo.c_prob[eo_o] = cp[r][t];
                    if (eo.c) eo.c[eo_o] = cc[r][t];
                    if (eo.c_smp) eo.c_smp[eo_o] = cs[r][t];
                }
                ent_acc += cc[r][t] * lc[r][t];
            }
        }
    }
    // ---- state head: [mu | sigma_pre] = y [Wmu; Wsigma]^T + b
    float mso[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) mso[r] = 0.f;
    for (int o = 0; o < 2 * S; ++o) {
        const float* w = Wms + (int64_t)o * (L + C);
        const float wl = sub < L ? w[sub] : 0.f;
        float wc[CP], pr[NR];
#pragma unroll
        for (int t = 0; t < CP; ++t) wc[t] = vcol[t] ? w[L + sub + W * t] : 0.f;
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            pr[r] = xl[r] * wl;
#pragma unroll
            for (int t = 0; t < CP; ++t) pr[r] += cs[r][t] * wc[t];
        }
        const float bo = bms[o];
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const float pv = Cell::sum(pr[r]) + bo;
            if (sub == o) mso[r] = pv;
        }
    }
    float* const pMS = ws + a.MS + ab0 * 2 * S;
    float* const pMU = ws + a.MU + ab0 * S;
    float* const pLV = ws + a.LV + ab0 * S;
    float* const pSS = ws + a.SS + ab0 * S;
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        if (okr[r] && sub < 2 * S) lat_st(pMS, ((uint32_t)slot[r] * (uint32_t)(2 * S) + (uint32_t)sub) * 4u, mso[r]);
        const float sg = __shfl(mso[r], base + ((sub + S) & (W - 1)), 64);
        if (okr[r] && sub < S) {
            const int b = bb[r];
            const float mu = mso[r];
            const float var = 1.f / (1.f + expf(-sg));
            const float lv = logf(var + eps);
            const float sd = sqrtf(expf(lv));
            const float U = state_u(nz, arm, B, S, b, sub);
            const float sv = U * sd + mu;
            float sin_ = sv;
            if (a.training && a.s_drop > 0.f) sin_ = state_keep(nz, arm, B, S, b, sub) ? sv / (1.f - a.s_drop) : 0.f;
            const uint32_t so = ((uint32_t)slot[r] * (uint32_t)S + (uint32_t)sub) * 4u;
            lat_st(pMU, so, mu);
            lat_st(pLV, so, lv);
            lat_st(pSS, so, sv);
            lat_st(pZIN, ((uint32_t)slot[r] * (uint32_t)(C + S) + (uint32_t)(C + sub)) * 4u, sin_);
            if constexpr (ENC == 1) {
                const int64_t eo_o = ((int64_t)arm * eo.rows + eo.row0 + b) * S + sub;
                if (eo.s_mean) eo.s_mean[eo_o] = mu;
                if (eo.s_logvar) eo.s_logvar[eo_o] = lv;
            }
            kl_acc += 1.f + lv - mu * mu - expf(lv);
        }
    }
    // ---- block partials (as k_lat_fwd): two passes over the LDS tile, NT / 128 row groups
    kl_acc = wave_sum(kl_acc);
    ent_acc = wave_sum(ent_acc);
    if (lane == 0) { sh_red[wv][0] = kl_acc; sh_red[wv][1] = ent_acc; }
    lds_barrier();
    {
        constexpr int G = NT / 128, RPG = LAT_ROWS / G;
        const int col = threadIdx.x & 127, g = threadIdx.x >> 7;
        const int nv = min(LAT_ROWS, B - b0);
        const bool live = col < W * CP;              // columns the cells wrote
        float v[RPG];
        float s1 = 0.f;
#pragma unroll
        for (int i = 0; i < RPG; ++i) { v[i] = live ? sh_buf[(g + G * i) * 128 + col] : 0.f; s1 += v[i]; }
        sh_ps[g][col] = s1;
        lds_barrier();
        float tot = 0.f;
#pragma unroll
        for (int k = 0; k < G; ++k) tot += sh_ps[k][col];
        const float mean = tot / (float)nv;
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < RPG; ++i) { const float d = v[i] - mean; q += (g + G * i < nv) ? d * d : 0.f; }
        lds_barrier();
        sh_ps[g][col] = q;
        lds_barrier();
        if (g == 0 && col < C) {
            float m2 = 0.f;
#pragma unroll
            for (int k = 0; k < G; ++k) m2 += sh_ps[k][col];
            if (a.acc_c >= 0) {
                acc_add_stats(reinterpret_cast<long long*>(ws + a.acc_c) + (int64_t)arm * ACC_SET_I64, col, (float)nv, mean, m2);
            } else {
                float* p = ws + a.c_part + (((int64_t)arm * gridDim.x + blk) * 2) * C;
                p[col] = mean;
                p[C + col] = m2;
            }
        }
    }
    if (threadIdx.x == 0) {
        float* p = ws + a.lat_part + ((int64_t)arm * gridDim.x + blk) * 2;
        float k0 = 0.f, k1 = 0.f;
#pragma unroll
        for (int w = 0; w < NW; ++w) { k0 += sh_red[w][0]; k1 += sh_red[w][1]; }
        p[0] = k0;
        p[1] = k1;
    }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
inline LatArgs make_lat_args(const Ctx& c) {
    const mmvae_dims& d = c.d;
    const Layout& L = c.lay;
    LatArgs a{};
    a.A = d.A; a.B = d.B; a.L = d.L; a.C = d.C; a.S = d.S;
    a.tau = c.h.tau; a.temp = c.h.temp; a.eps = c.h.eps; a.s_drop = c.h.s_drop;
    a.use_mask = (c.h.cat_mask[0] | c.h.cat_mask[1] | c.h.cat_mask[2] | c.h.cat_mask[3]) != 0u;
    for (int i = 0; i < 4; ++i) a.cmask[i] = c.h.cat_mask[i];
    a.hard = c.h.hard; a.training = c.h.training; a.eval_flag = c.h.eval_flag;
    a.per_arm = c.po.per_arm; a.o_wc = c.po.o[10]; a.o_bc = c.po.o[11]; a.o_wms = c.po.o[12]; a.o_bms = c.po.o[14];
    a.R5 = L.R[4]; a.mean5 = L.bn_mean[4]; a.rstd5 = L.bn_rstd[4];
    a.XLOW = L.XLOW; a.CPROB = L.CPROB; a.CC = L.CC; a.YSOFT = L.YSOFT; a.CSMP = L.CSMP; a.Y = L.Y; a.MS = L.MS;
    a.MU = L.MU; a.LV = L.LV; a.SS = L.SS; a.ZIN = L.ZIN; a.c_part = L.c_part; a.lat_part = L.lat_part;
    a.GZIN = L.GZIN; a.GMS = L.GMS; a.GZC = L.GZC; a.G5 = L.G[5]; a.bnb_part5 = L.bnb_part[5];
    a.T = L.T; a.c_mean = L.c_mean; a.c_iv = L.c_iv;
    a.am1 = (float)(d.A > 1 ? d.A - 1 : 1); a.beta = c.h.beta; a.lam = c.h.lam;
    a.bn_part5 = c.h.training ? L.bn_part[4] : -1;
    a.bn5_n = L.nblkf;   // (partial-array form: chain_rows_fwd == CHAIN_ROWS)
    a.acc_bn5 = (c.h.training && c.use_acc()) ? acc_set_off(L, d.A, 4) : -1;
    a.acc_bnb5 = c.use_acc() ? acc_set_off(L, d.A, ACC_BWD + 4) : -1;
    a.acc_c = (c.h.training && c.use_acc()) ? acc_set_off(L, d.A, ACC_C) : -1;
    a.acc_T = (c.h.training && c.use_acc()) ? acc_set_off(L, d.A, ACC_T) : -1;
    a.run_mean_off = c.po.bn_mean[4]; a.run_var_off = c.po.bn_var[4]; a.run_arm_stride = c.po.bn_per_arm;
    a.bn_momentum = c.h.bn_momentum;
    return a;
}

// dynamic LDS of the four latent kernels: what lat_stage_weights stages
inline size_t lat_smem_bytes(const mmvae_dims& d) { return (size_t)(d.C * d.L + 2 * d.S * (d.L + d.C)) * sizeof(float); }

}  // namespace mmvae
#endif  // MMVAE_LAT_FWD_HPP

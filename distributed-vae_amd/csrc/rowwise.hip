// Row-wise (one wavefront or half of one per cell) kernels and the small reductions between them:
//
//   (batch statistics: every consumer recombines the producers' per-row-block (mean, M2) partials itself,
//    common.hpp stats_from_partials -- BatchNorm1d incl. running statistics, nn_model.py:208-255, and
//    inv_var, nn_model.py:75-77; eval mode: k_stats_from_running)
//   k_lat_fwd[_h]     x_low = BN5(R5); c_prob = softmax(fcc x_low); c = softmax(c_prob/tau);
//                     Gumbel-softmax sample; state head; reparameterise; decoder input
//                     (nn_model.py:268-269, :337-351, :413-493)
//   k_couple          pairwise coupling terms over arms (nn_model.py:558-569)
//   k_loss_finalize   scalars of nn_model.py:542-598
//   k_lat_bwd[_h]     autograd of k_lat_fwd + coupling / entropy / KL terms
//                     (one body each, lat_fwd / lat_bwd<W, NW>; _h: a cell on W = 32 lanes, see LatCell;
//                      the forward kernel lives in lat_fwd.hpp, which encode.hip instantiates too)
//   k_reduce          slabs -> flat gradient buffer;  k_adam: torch.optim.Adam(W) update
//   k_intermed        mu = fc_mu(y), var = sigmoid(fc_sigma(y)) on the caller's rows (nn_model.py:271-275)
//
// Wave reductions only (no MFMA): these tensors are [B, <=128] and HBM/L2 resident.
#include "common.hpp"
#include "couple.hpp"
#include "lat_fwd.hpp"
#include <type_traits>
#include <math.h>
#include <stdlib.h>

namespace mmvae {


NoiseDev make_noise_dev(const mmvae_noise* nz, const mmvae_hyper& h) {
    NoiseDev n{};
    n.mode = nz ? nz->mode : 0;
    if (nz) {
        n.x_mask = nz->x_mask; n.u_gumbel = nz->u_gumbel; n.u_state = nz->u_state; n.s_mask = nz->s_mask;
        n.k0 = (uint32_t)nz->seed; n.k1 = (uint32_t)(nz->seed >> 32);
        n.step_lo = (uint32_t)nz->offset; n.step_hi = (uint32_t)(nz->offset >> 32);
    }
    // smallest field width that represents the 16-bit keep threshold exactly (0 and 65536: one bit, thr 0 / 2)
    const uint32_t t16 = keep_threshold16(h.x_drop);
    uint32_t ml = 0;
    while (ml < 4 && (t16 & ((65536u >> (1u << ml)) - 1u)) != 0) ++ml;
    n.x_mlog2 = ml;
    n.x_thr = t16 >> (16u - (1u << ml));
    n.s_keep_thr = keep_threshold(h.s_drop);
    return n;
}

// eval mode: statistics come from the running buffers.  One launch for the five BatchNorm layers: grid (A, 5).
struct EvalStatArgs { int64_t run_mean[5], run_var[5], mean_out[5], rstd_out[5]; int W[5]; };
__global__ void k_stats_from_running(const float* __restrict__ bn_running, int64_t run_arm_stride, EvalStatArgs a, float eps,
                                     float* __restrict__ ws) {
    const int arm = blockIdx.x, layer = blockIdx.y, col = threadIdx.x;
    const int W = a.W[layer];
    if (col < W) {
        ws[a.mean_out[layer] + arm * W + col] = bn_running[a.run_mean[layer] + arm * run_arm_stride + col];
        ws[a.rstd_out[layer] + arm * W + col] = 1.0f / sqrtf(bn_running[a.run_var[layer] + arm * run_arm_stride + col] + eps);
    }
}

constexpr auto k_lat_fwd = k_lat_fwd_g<64, LAT_NW>, k_lat_fwd_h = k_lat_fwd_g<32, LH_NW>;

// ---------------------------------------------------------------------------------------------
// coupling: for every cell, over all arms.  u_a = log(c_a + eps) * iv_a
//   dist += sum_{a<b} |u_a - u_b|^2 ;  l2 += sum_{a<b} |c_smp_a - c_smp_b|^2
//   T_part[a][k] += G_a[k] * log(c_a[k] + eps),  G_a = (2 lam / B) (A u_a - sum_b u_b)
// grid (ceil(B/32)), 256 threads.
// ---------------------------------------------------------------------------------------------
// AT: the number of arms (a template parameter: every loop over arms is static, so that all loads of a batch of rows
// issue before the first use -- with a run-time arm count inside the row loop the kernel waited for every row in turn:
// 54 us).  c_acc / t_acc != null: the statistics of c come from the accumulator set the latent forward kernels added to,
// and this kernel adds its T sums to another (the latent backward reads W numbers; no reduction launch); else the
// partial arrays (c_part recombined here, T_part summed by k_loss_finalize).
template <int AT>
__global__ __launch_bounds__(256) void k_couple(int B, int C, float eps, float lam, const float* __restrict__ CCp,
                                                const float* __restrict__ CSMPp, const float* __restrict__ c_part, int c_n,
                                                const long long* __restrict__ c_acc, float* __restrict__ c_mean,
                                                float* __restrict__ c_iv, float* __restrict__ couple_part,
                                                float* __restrict__ T_part, long long* __restrict__ t_acc) {
    // (the arithmetic lives in couple.hpp: the decoder chain's launch of the fused train step runs it as one of its roles)
    __shared__ __attribute__((aligned(16))) float shT[4 * AT * CPL * 64];
    __shared__ float sh_red[8], sh_iv[AT * CPL * 64];
    __shared__ __attribute__((aligned(16))) float sh_scr[3 * PART_MAXG * CPL * 64];
    couple_body<AT>(blockIdx.x, true, threadIdx.x, B, C, eps, lam, CCp, CSMPp, c_part, c_n, c_acc, c_mean, c_iv, couple_part, T_part,
                    t_acc, shT, sh_red, sh_iv, sh_scr);
}

// ---------------------------------------------------------------------------------------------
// loss scalars (one block).  Sums the per-block partials in double.
// ---------------------------------------------------------------------------------------------
__device__ double block_sum_d(double v, double* sh) {
    const int tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) sh[tid] += sh[tid + o];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(256) void k_loss_finalize(int A, int B, int D, int C, float beta, float lam,
                                                       const float* __restrict__ fc11_part, int n11,
                                                       const float* __restrict__ lat_part, int nlat, int nblk,
                                                       const float* __restrict__ couple_part,
                                                       const float* __restrict__ T_part, float* __restrict__ T,
                                                       float* __restrict__ out, int mode, const double* __restrict__ zrec) {
    // zrec != null: rec[a] = zrec[a] (mmvae_zinb_train_step, mmvae_zinb_objective); ll keeps the reference's expression
    // mode 0: block 0 the scalars, blocks 1.. the T sums; 1: T sums only (every block; they need the coupling kernel's
    // output alone and the latent backward waits for them); 2: scalars only (one block; they need fc11's loss partials)
    __shared__ double sh[256];
    const int tid = threadIdx.x;
    const int bx = mode == 1 ? (int)blockIdx.x + 1 : (int)blockIdx.x;
    if (bx > 0) {
        // blocks 1.. : T[a][k] = sum over row blocks of T_part[blk][a][k]  (8 block groups x 32 columns)
        const int c = tid & 31, g = tid >> 5, i = (bx - 1) * 32 + c, n = A * C;
        double s = 0.0;
        if (i < n)
            for (int b = g; b < nblk; b += 8) s += T_part[(int64_t)b * n + i];
        sh[g * 32 + c] = s;
        __syncthreads();
        if (g == 0 && i < n) {
            for (int k = 1; k < 8; ++k) s += sh[k * 32 + c];
            T[i] = (float)s;
        }
        return;
    }
    const double PI2 = 6.283185307179586;
    double sum_ind = 0.0, sum_ent = 0.0;
    for (int a = 0; a < A; ++a) {
        double se = 0.0, mm = 0.0, kl = 0.0, en = 0.0;
        for (int i = tid; i < n11; i += 256) {
            se += fc11_part[((int64_t)a * n11 + i) * 2];
            mm += fc11_part[((int64_t)a * n11 + i) * 2 + 1];
        }
        for (int i = tid; i < nlat; i += 256) {
            kl += lat_part[((int64_t)a * nlat + i) * 2];
            en += lat_part[((int64_t)a * nlat + i) * 2 + 1];
        }
        se = block_sum_d(se, sh); mm = block_sum_d(mm, sh); kl = block_sum_d(kl, sh); en = block_sum_d(en, sh);
        const double rec = zrec ? zrec[a] : 0.5 * se / B + 0.5 * (100.0 * mm / ((double)B * D));   // nn_model.py:544-546
        const double ll = se / ((double)B * D) + B * log(PI2);                     // :542
        const double klv = -0.5 * kl / B;                                          // :43-44
        if (tid == 0) {
            out[MMVAE_LOSS_REC0 + a] = (float)rec;
            out[MMVAE_LOSS_REC0 + A + a] = (float)klv;
            out[MMVAE_LOSS_REC0 + 2 * A + a] = (float)ll;
        }
        sum_ind += rec + beta * klv;
        sum_ent += en / B;
    }
    double ds = 0.0, l2 = 0.0;
    for (int i = tid; i < nblk; i += 256) { ds += couple_part[i * 2]; l2 += couple_part[i * 2 + 1]; }
    ds = block_sum_d(ds, sh) / B;
    l2 = block_sum_d(l2, sh) / B;
    const double npairs = A > 1 ? A * (A - 1) / 2.0 : 1.0;
    const double sum_c_ents = (A - 1) * sum_ent;   // every arm is in A-1 pairs
    const double joint = lam * ds + sum_c_ents + npairs * ((C / 2.0) * log(PI2) - 0.5 * log(2.0 * lam));   // :581-586
    const double total = (A > 1 ? A - 1 : 1) * sum_ind + joint;                                           // :587
    if (tid == 0) {
        out[MMVAE_LOSS_TOTAL] = (float)total;
        out[MMVAE_LOSS_JOINT] = (float)joint;
        out[MMVAE_LOSS_CENT] = (float)(sum_c_ents / npairs);
        out[MMVAE_LOSS_CDIST] = (float)(ds / npairs);
        out[MMVAE_LOSS_CL2] = (float)(l2 / npairs);
    }
}

// ---------------------------------------------------------------------------------------------
// backward of the latent block.  grid (ceil(B/LAT_ROWS_BWD), A), 64 NW threads, the geometries of the forward (LatCell).
// ---------------------------------------------------------------------------------------------
// AT: the number of arms, a template parameter as k_couple's: the per-arm registers (call, ivall) are AT deep, not
// MMVAE_MAX_ARMS, and no arm loop is predicated.  Every per-cell load goes through lat_ld (lat_fwd.hpp): a lane without an
// element (column >= C, sub >= S / L) reads 0 without a branch.
template <int W, int NW, int AT>
__global__ __launch_bounds__(64 * NW) void k_lat_bwd_g(const LatArgs a_in, const NoiseDev nz_in, const float* __restrict__ params,
                                                      float* __restrict__ ws) {
    using Cell = LatCell<W>;
    constexpr int CPW = Cell::CPW, CP = Cell::CP, NR = LAT_ROWS_BWD / (NW * CPW);
    static_assert(NR * NW * CPW == LAT_ROWS_BWD, "cells per workgroup");
    static_assert(AT >= 1 && AT <= MMVAE_MAX_ARMS, "arms");
    const LatArgs a = a_in;
    const NoiseDev nz = nz_in;
    extern __shared__ __attribute__((aligned(16))) float lat_smem[];
    __shared__ float sh_s[NW][2][64];
    const int arm = blockIdx.y, blk = blockIdx.x, b0 = blk * LAT_ROWS_BWD;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int sub = Cell::sub(lane), base = Cell::base(lane), cell = Cell::cell(lane);
    constexpr int A = AT;
    const int B = a.B, L = a.L, C = a.C, S = a.S;
    const float* P = params + (int64_t)arm * a.per_arm;
    float* WcT = lat_smem;            // [L][C]
    float* Wms = lat_smem + C * L;    // [2S][L+C]
    lat_stage_weights(WcT, Wms, P + a.o_wc, P + a.o_wms, L, C, S);
    const int64_t ab0 = (int64_t)arm * B + b0;       // the workgroup's first cell
    const int nrows = min(LAT_ROWS_BWD, B - b0);     // its cells within the batch
    const float eps = a.eps, invB = 1.f / (float)B;
    const float coefG = 2.f * a.lam * invB;

    bool vcol[CP];
    uint32_t cob[CP];   // byte offset of column `sub + W t` within a row; LAT_OOB beyond C
    int colw[CP];       // the column whose staged weights the lane reads: its own, or column 0 beyond C (a finite weight
                        // that meets an exact 0 there, or feeds a value nothing reads) -- no branch around the LDS reads
    float Tk[CP], cmean[CP], ivm[CP], ivall[AT][CP];
    {
        const auto rT = lat_rsrc(ws + a.T, A, C), rM = lat_rsrc(ws + a.c_mean, A, C), rV = lat_rsrc(ws + a.c_iv, A, C);
#pragma unroll
        for (int t = 0; t < CP; ++t) {
            const int col = sub + W * t;
            vcol[t] = col < C;
            cob[t] = vcol[t] ? (uint32_t)col * 4u : LAT_OOB;
            colw[t] = vcol[t] ? col : 0;
            Tk[t] = lat_ld(rT, (uint32_t)(arm * C) * 4u + cob[t]);
            if (a.acc_T >= 0 && vcol[t]) {
                double s1, s2;
                acc_get(reinterpret_cast<const long long*>(ws + a.acc_T) + (int64_t)arm * ACC_SET_I64, col, s1, s2);
                Tk[t] = (float)s1;
            }
            cmean[t] = lat_ld(rM, (uint32_t)(arm * C) * 4u + cob[t]);
            ivm[t] = lat_ld(rV, (uint32_t)(arm * C) * 4u + cob[t]);
#pragma unroll
            for (int aa = 0; aa < AT; ++aa) ivall[aa][t] = lat_ld(rV, (uint32_t)(aa * C) * 4u + cob[t]);
        }
    }
    float s1 = 0.f, s2 = 0.f;   // BN5 backward sums for column `sub` (< L), this lane group's cells

    int bb[NR];
    bool okr[NR];
    float gs_l[NR], mu_l[NR], lv_l[NR], sg_l[NR], xlow_l[NR];
    float cc[NR][CP], ys[NR][CP], gz[NR][CP], cp[NR][CP], call[NR][AT][CP];
    {
        const auto rGZ = lat_rsrc(ws + a.GZIN + ab0 * (C + S), nrows, C + S), rMU = lat_rsrc(ws + a.MU + ab0 * S, nrows, S),
                   rLV = lat_rsrc(ws + a.LV + ab0 * S, nrows, S), rMS = lat_rsrc(ws + a.MS + ab0 * 2 * S, nrows, 2 * S),
                   rXL = lat_rsrc(ws + a.XLOW + ab0 * L, nrows, L), rYS = lat_rsrc(ws + a.YSOFT + ab0 * C, nrows, C),
                   rCP = lat_rsrc(ws + a.CPROB + ab0 * C, nrows, C), rCC = lat_rsrc(ws + a.CC + ab0 * C, nrows, C);
        const uint32_t sob = sub < S ? (uint32_t)sub * 4u : LAT_OOB, lob = sub < L ? (uint32_t)sub * 4u : LAT_OOB;
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            bb[r] = b0 + r * (NW * CPW) + wv * CPW + cell;
            okr[r] = bb[r] < B;                                     // per cell
            const uint32_t rl = (uint32_t)(min(bb[r], B - 1) - b0);   // cells beyond the batch recompute the last cell; nothing is stored
            gs_l[r] = lat_ld(rGZ, (rl * (uint32_t)(C + S) + (uint32_t)C) * 4u + sob);
            mu_l[r] = lat_ld(rMU, rl * (uint32_t)S * 4u + sob);
            lv_l[r] = lat_ld(rLV, rl * (uint32_t)S * 4u + sob);
            sg_l[r] = lat_ld(rMS, (rl * (uint32_t)(2 * S) + (uint32_t)S) * 4u + sob);
            xlow_l[r] = lat_ld(rXL, rl * (uint32_t)L * 4u + lob);
#pragma unroll
            for (int t = 0; t < CP; ++t) {
                const uint32_t o = rl * (uint32_t)C * 4u + cob[t];
                cc[r][t] = lat_ld(rCC, o);
                ys[r][t] = lat_ld(rYS, o);
                cp[r][t] = lat_ld(rCP, o);
                gz[r][t] = lat_ld(rGZ, rl * (uint32_t)(C + S) * 4u + cob[t]);
            }
#pragma unroll
            for (int aa = 0; aa < AT; ++aa) {   // c of every arm at this cell
                const auto rCa = lat_rsrc(ws + a.CC + ((int64_t)aa * B + b0) * C, nrows, C);
#pragma unroll
                for (int t = 0; t < CP; ++t) call[r][aa][t] = lat_ld(rCa, rl * (uint32_t)C * 4u + cob[t]);
            }
        }
    }
    const float inv_temp = 1.f / a.temp, inv_tau = 1.f / a.tau, inv_bm1 = 1.f / (float)(B - 1);
    float* const pGMS = ws + a.GMS + ab0 * 2 * S;   // stores: the workgroup's first row + a 32-bit byte offset
    float* const pGZC = ws + a.GZC + ab0 * C;
    float* const pG5 = ws + a.G5 + ab0 * L;
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const int b = min(bb[r], B - 1);
        const uint32_t rl = (uint32_t)(b - b0);
        // ---- state head backward (lanes sub < S of each cell)
        float gms = 0.f;   // sub = o < 2S: d loss / d MS[o]
        {
            float gmu = 0.f, gsig = 0.f;
            if (sub < S) {
                float gs = gs_l[r];
                if (a.training && a.s_drop > 0.f)
                    gs = state_keep(nz, arm, B, S, b, sub) ? gs / (1.f - a.s_drop) : 0.f;
                const float mu = mu_l[r], lv = lv_l[r], sg = sg_l[r];
                const float var = 1.f / (1.f + expf(-sg));
                const float U = state_u(nz, arm, B, S, b, sub);
                const float elv = expf(lv);
                gmu = gs + a.am1 * a.beta * mu * invB;
                const float glv = gs * U * 0.5f * sqrtf(elv) + a.am1 * a.beta * (-0.5f * invB) * (1.f - elv);
                const float gvar = glv / (var + eps);
                gsig = gvar * var * (1.f - var);
            }
            const float gsig_sh = __shfl(gsig, base + ((sub - S) & (W - 1)), 64);   // sub S+s takes sub s's gsig
            if (sub < S) gms = gmu;
            else if (sub < 2 * S) gms = gsig_sh;
            if (okr[r] && sub < 2 * S) lat_st(pGMS, (rl * (uint32_t)(2 * S) + (uint32_t)sub) * 4u, gms);
        }
        // ---- gy = gms [Wmu; Wsigma]
        float gxl = 0.f, gcs[CP];
        const int subl = sub < L ? sub : 0;
#pragma unroll
        for (int t = 0; t < CP; ++t) gcs[t] = 0.f;
        for (int o = 0; o < 2 * S; ++o) {
            const float go = __shfl(gms, base + o, 64);
            const float* w = Wms + (int64_t)o * (L + C);
            gxl += go * w[subl];                                               // (lanes sub >= L: read by nothing)
#pragma unroll
            for (int t = 0; t < CP; ++t) gcs[t] += go * w[L + colw[t]];       // (columns >= C: dropped below)
        }
        // ---- gradient w.r.t. the sample, through the Gumbel softmax to c
        float lc[CP], gc[CP], usum[CP], rcc[CP];
        float dot = 0.f;
#pragma unroll
        for (int t = 0; t < CP; ++t) {
            lc[t] = gc[t] = usum[t] = 0.f;
            rcc[t] = 1.f / (cc[r][t] + eps);
            if (vcol[t]) {
                gcs[t] += gz[r][t];
                dot += ys[r][t] * gcs[t];
#pragma unroll
                for (int aa = 0; aa < AT; ++aa) {
                    const float l_aa = logf(call[r][aa][t] + eps);
                    usum[t] = __builtin_fmaf(l_aa, ivall[aa][t], usum[t]);   // fused, as the per-arm blocks of the run-time arm
                                                                              // count compiled (packed across arms the products
                                                                              // would round on their own)
                    if (aa == arm) lc[t] = l_aa;
                }
            }
        }
        if (a.eval_flag) {
#pragma unroll
            for (int t = 0; t < CP; ++t) gc[t] = gcs[t];
        } else {
            dot = Cell::sum(dot);
#pragma unroll
            for (int t = 0; t < CP; ++t) gc[t] = (ys[r][t] * (gcs[t] - dot) * inv_temp) * rcc[t];
        }
        // ---- coupling / entropy terms on c (nn_model.py:558-569)
        float dot2 = 0.f;
#pragma unroll
        for (int t = 0; t < CP; ++t) {
            if (vcol[t]) {
                const float G = coefG * ((float)A * lc[t] * ivm[t] - usum[t]);
                gc[t] += (float)(A - 1) * (lc[t] + cc[r][t] * rcc[t]) * invB;
                gc[t] += G * ivm[t] * rcc[t];
                gc[t] += (Tk[t] * (-0.5f) * ivm[t] * ivm[t] * ivm[t]) * 2.f * (cc[r][t] - cmean[t]) * inv_bm1;
                dot2 += cc[r][t] * gc[t];
            } else {
                gc[t] = 0.f;
            }
        }
        dot2 = Cell::sum(dot2);
        // ---- double softmax backward
        float gq[CP], dot3 = 0.f;
#pragma unroll
        for (int t = 0; t < CP; ++t) {
            gq[t] = cc[r][t] * (gc[t] - dot2) * inv_tau;
            dot3 += cp[r][t] * gq[t];
        }
        dot3 = Cell::sum(dot3);
        float gzc[CP];
#pragma unroll
        for (int t = 0; t < CP; ++t) {
            gzc[t] = cp[r][t] * (gq[t] - dot3);
            if (okr[r] && vcol[t]) lat_st(pGZC, (rl * (uint32_t)C + (uint32_t)(sub + W * t)) * 4u, gzc[t]);
        }
        // ---- g5 = gy[:, :L] + gzc Wc
        float g5 = 0.f;
        for (int k = 0; k < L; ++k) {
            float p = 0.f;
#pragma unroll
            for (int t = 0; t < CP; ++t) p = __builtin_fmaf(gzc[t], WcT[k * C + colw[t]], p);   // columns >= C: gzc = cp (..) = 0 exactly
            p = Cell::sum(p);
            if (sub == k) g5 = gxl + p;
        }
        if (okr[r] && sub < L) {
            lat_st(pG5, (rl * (uint32_t)L + (uint32_t)sub) * 4u, g5);
            s1 += g5;
            s2 += g5 * xlow_l[r];
        }
    }
    sh_s[wv][0][lane] = s1;
    sh_s[wv][1][lane] = s2;
    lds_barrier();
    if (threadIdx.x < L) {
        const int k = threadIdx.x;
        float* p = ws + a.bnb_part5 + (((int64_t)arm * gridDim.x + blk) * 2) * L;
        float k0 = 0.f, k1 = 0.f;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            float c0 = sh_s[w][0][k], c1 = sh_s[w][1][k];       // the CPW lane groups hold different cells: their sum
#pragma unroll
            for (int h = 1; h < CPW; ++h) { c0 += sh_s[w][0][W * h + k]; c1 += sh_s[w][1][W * h + k]; }   // first, then the wave's
            k0 += c0;
            k1 += c1;
        }
        if (a.acc_bnb5 >= 0) {
            acc_add_sums(reinterpret_cast<long long*>(ws + a.acc_bnb5) + (int64_t)arm * ACC_SET_I64, k, k0, k1);
        } else {
            p[k] = k0;
            p[L + k] = k1;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// slabs -> flat gradient buffer
// ---------------------------------------------------------------------------------------------
struct RedDesc {
    const float* slab; int64_t ks_stride, arm_stride; int ld, col0;
    int rows, cols;
    int64_t dst_off; int dst_ld;
    float scale;
    int ks;   // slabs to sum
};
constexpr int MAX_RED = 28;
struct RedDescs { RedDesc d[MAX_RED]; int first[MAX_RED + 1]; int n; };   // descriptor i owns blocks [first[i], first[i + 1]) of grid.x

struct AdamArgs {
    float* p; float* m; float* v;        // null p: gradients only
    float lr_bc1, inv_sqrt_bc2, b1, b2, eps, wd, lr;
    int decoupled;
};

// grid (blocks, ndesc, A): descriptor y, arm z.  With
// adam.p != null the Adam/AdamW update of the element is applied in the same pass (single-GPU step).
// HBM-bound (every slab element is read once): VEC threads own four consecutive columns (16-byte loads), the
// slab loads of an element are issued sixteen at a time before the first add (a `for k < KS` loop with a
// running sum waits for one memory latency per slab), and the index arithmetic is 32-bit.
__device__ __forceinline__ float adam_update1(const AdamArgs& adam, int64_t o, float gi) {
    float pi = adam.p[o];
    if (adam.wd != 0.f) {
        if (adam.decoupled) pi *= (1.f - adam.lr * adam.wd);
        else gi += adam.wd * pi;
    }
    const float mi = adam.b1 * adam.m[o] + (1.f - adam.b1) * gi;
    const float vi = adam.b2 * adam.v[o] + (1.f - adam.b2) * gi * gi;
    adam.m[o] = mi;
    adam.v[o] = vi;
    return pi - adam.lr_bc1 * (mi / (sqrtf(vi) * adam.inv_sqrt_bc2 + adam.eps));
}

template <bool VEC>
__device__ __forceinline__ void reduce_desc(const RedDesc& d, int KS, int arm, float* __restrict__ grads, int64_t per_arm,
                                            const AdamArgs& adam, uint32_t bx, uint32_t nbx) {
    constexpr int E = VEC ? 4 : 1;
    const uint32_t cpr = (uint32_t)d.cols / E;                       // work items per row
    const uint32_t n = (uint32_t)d.rows * cpr;
    const float* base = d.slab + (int64_t)arm * d.arm_stride + d.col0;
    for (uint32_t i = bx * blockDim.x + threadIdx.x; i < n; i += nbx * blockDim.x) {
        const uint32_t r = i / cpr, cidx = (i - r * cpr) * E;
        const float* p = base + (int64_t)r * d.ld + cidx;
        const int64_t o = (int64_t)arm * per_arm + d.dst_off + (int64_t)r * d.dst_ld + cidx;
        // the parameter and its moments are requested WITH the slabs (one memory round trip per item instead of two)
        float4 pi = make_float4(0.f, 0.f, 0.f, 0.f), mi = pi, vi = pi;
        if constexpr (VEC) {
            if (adam.p) {
                pi = *reinterpret_cast<const float4*>(adam.p + o);
                mi = *reinterpret_cast<const float4*>(adam.m + o);
                vi = *reinterpret_cast<const float4*>(adam.v + o);
            }
        }
        float s[E];
#pragma unroll
        for (int e = 0; e < E; ++e) s[e] = 0.f;
        // slab loads in flight per item: the smallest of 4 / 8 / 16 that covers KS (the clamped duplicates of the last slab
        // each cost a pass through the vector-memory pipe: 16 issued for 4 or 6 slabs were 2.7 - 4 x the loads needed);
        // the sum runs over the slabs in the same order whatever the chunk
        auto add_slabs = [&](auto chunk, int kbeg, int kend) __attribute__((always_inline)) {
            constexpr int CHK = decltype(chunk)::value;
            for (int k0 = kbeg; k0 < kend; k0 += CHK) {
                float v[CHK][E];
#pragma unroll
                for (int k = 0; k < CHK; ++k) {
                    const float* q = p + (int64_t)min(k0 + k, KS - 1) * d.ks_stride;
                    if constexpr (VEC) {
                        const float4 t = *reinterpret_cast<const float4*>(q);
                        v[k][0] = t.x; v[k][1] = t.y; v[k][2] = t.z; v[k][3] = t.w;
                    } else {
                        v[k][0] = *q;
                    }
                }
#pragma unroll
                for (int k = 0; k < CHK; ++k)
#pragma unroll
                    for (int e = 0; e < E; ++e) s[e] += (k0 + k < KS) ? v[k][e] : 0.f;
            }
        };
        // (whole sixteens first, then the smallest chunk that covers the rest: 20 slabs -- the small-layer products at the benchmark
        // shape -- are 16 + 4 loads, not 32)
        const int k16 = KS > 8 ? (KS & ~15) : 0, rest = KS - k16;
        if (k16 > 0) add_slabs(std::integral_constant<int, 16>{}, 0, k16);
        if (rest > 8) add_slabs(std::integral_constant<int, 16>{}, k16, KS);
        else if (rest > 4) add_slabs(std::integral_constant<int, 8>{}, k16, KS);
        else if (rest > 0) add_slabs(std::integral_constant<int, 4>{}, k16, KS);
        float g[E];
#pragma unroll
        for (int e = 0; e < E; ++e) g[e] = s[e] * d.scale;
        if constexpr (VEC) {
            *reinterpret_cast<float4*>(grads + o) = make_float4(g[0], g[1], g[2], g[3]);
            if (adam.p) {
                const float pin[4] = {pi.x, pi.y, pi.z, pi.w}, min_[4] = {mi.x, mi.y, mi.z, mi.w}, vin[4] = {vi.x, vi.y, vi.z, vi.w};
                float po[4], mo[4], vo[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float pe = pin[e], ge = g[e];
                    if (adam.wd != 0.f) {
                        if (adam.decoupled) pe *= (1.f - adam.lr * adam.wd);
                        else ge += adam.wd * pe;
                    }
                    mo[e] = adam.b1 * min_[e] + (1.f - adam.b1) * ge;
                    vo[e] = adam.b2 * vin[e] + (1.f - adam.b2) * ge * ge;
                    po[e] = pe - adam.lr_bc1 * (mo[e] / (sqrtf(vo[e]) * adam.inv_sqrt_bc2 + adam.eps));
                }
                *reinterpret_cast<float4*>(adam.m + o) = make_float4(mo[0], mo[1], mo[2], mo[3]);
                *reinterpret_cast<float4*>(adam.v + o) = make_float4(vo[0], vo[1], vo[2], vo[3]);
                *reinterpret_cast<float4*>(adam.p + o) = make_float4(po[0], po[1], po[2], po[3]);
            }
        } else {
            grads[o] = g[0];
            if (adam.p) adam.p[o] = adam_update1(adam, o, g[0]);
        }
    }
}

__global__ __launch_bounds__(256) void k_reduce(const RedDescs ds, float* __restrict__ grads, int64_t per_arm,
                                                const AdamArgs adam_in) {
    // grid (blocks of all descriptors, 1, A): large and small tensors in ONE launch -- the three D x H tensors want thousands of
    // workgroups, the 23 small ones sixteen each, and as two launches the small one (latency-bound) cost as much as the large
    int di = 0;
    while (di + 1 < ds.n && (int)blockIdx.x >= ds.first[di + 1]) ++di;
    const int arm = blockIdx.z;
    const uint32_t bx = blockIdx.x - ds.first[di], nbx = ds.first[di + 1] - ds.first[di];
    const RedDesc& dr = ds.d[di];
    const RedDesc d = {dr.slab, dr.ks_stride, dr.arm_stride, dr.ld, dr.col0, dr.rows, dr.cols, dr.dst_off, dr.dst_ld, dr.scale, dr.ks};
    const AdamArgs adam = adam_in;
    const int KS = d.ks;
    // 16-byte path: four-column groups aligned in every slab, in the gradient and in the parameter / moment buffers
    const bool vec = ((d.cols | d.ld | d.col0 | d.dst_ld) & 3) == 0 && ((d.ks_stride | d.arm_stride | d.dst_off | per_arm) & 3) == 0 &&
                     ((reinterpret_cast<uintptr_t>(d.slab) | reinterpret_cast<uintptr_t>(grads) |
                       reinterpret_cast<uintptr_t>(adam.p) | reinterpret_cast<uintptr_t>(adam.m) |
                       reinterpret_cast<uintptr_t>(adam.v)) & 15) == 0;
    if (vec) reduce_desc<true>(d, KS, arm, grads, per_arm, adam, bx, nbx);
    else reduce_desc<false>(d, KS, arm, grads, per_arm, adam, bx, nbx);
}

__global__ void k_adam(int64_t n, float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                       float* __restrict__ v, float lr_bc1, float inv_sqrt_bc2, float b1, float b2, float eps,
                       float wd, float lr, int decoupled) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        float pi = p[i], gi = g[i];
        if (wd != 0.f) {
            if (decoupled) pi *= (1.f - lr * wd);
            else gi += wd * pi;
        }
        const float mi = b1 * m[i] + (1.f - b1) * gi;
        const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
        m[i] = mi;
        v[i] = vi;
        const float denom = sqrtf(vi) * inv_sqrt_bc2 + eps;
        p[i] = pi - lr_bc1 * (mi / denom);
    }
}

__global__ void k_dump_noise(NoiseDev nz, int A, int B, int D, int C, int S, uint8_t* x_mask, float* u_gumbel,
                             float* u_state, uint8_t* s_mask) {
    const int64_t nx = (int64_t)A * B * D, ng = (int64_t)A * B * C, ns = (int64_t)A * B * S;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x_mask)
        for (int64_t i = i0; i < nx; i += stride) {
            const int arm = (int)(i / ((int64_t)B * D));
            const int64_t e = i % ((int64_t)B * D);
            x_mask[i] = xmask_keep(nz, arm, (int)(e / D), (int)(e % D)) ? 1 : 0;
        }
    if (u_gumbel)
        for (int64_t i = i0; i < ng; i += stride) {
            const int arm = (int)(i / ((int64_t)B * C));
            u_gumbel[i] = noise_uniform(nz, arm, STREAM_GUMBEL, (uint64_t)(i % ((int64_t)B * C)));
        }
    for (int64_t i = i0; i < ns; i += stride) {
        const int arm = (int)(i / ((int64_t)B * S));
        if (u_state) u_state[i] = noise_uniform(nz, arm, STREAM_STATE, (uint64_t)(i % ((int64_t)B * S)));
        if (s_mask) s_mask[i] = noise_keep(nz, arm, STREAM_SMASK, (uint64_t)(i % ((int64_t)B * S)), nz.s_keep_thr) ? 1 : 0;
    }
}

// ---------------------------------------------------------------------------------------------
// host launchers
// ---------------------------------------------------------------------------------------------
// eval mode: BatchNorm `layer` (0..4) normalises with the running buffers; in training mode the kernel that
// consumes the layer recombines the batch statistics itself and nothing is launched here
int launch_bn_eval_stats(const Ctx& c, const float* bn_running) {
    const mmvae_dims& d = c.d;
    const Layout& L = c.lay;
    if (c.h.training) return 0;
    if (!bn_running) { set_error("eval-mode forward needs bn_running"); return MMVAE_E_BADARG; }
    EvalStatArgs a{};
    for (int layer = 0; layer < 5; ++layer) {
        a.run_mean[layer] = c.po.bn_mean[layer];
        a.run_var[layer] = c.po.bn_var[layer];
        a.mean_out[layer] = L.bn_mean[layer];
        a.rstd_out[layer] = L.bn_rstd[layer];
        a.W[layer] = (layer == 4) ? d.L : d.H;
    }
    hipLaunchKernelGGL(k_stats_from_running, dim3(d.A, 5), dim3(128), 0, c.stream, bn_running, c.po.bn_per_arm, a, c.h.eps, c.ws);
    HIP_LAUNCH_CHECK("k_stats_from_running");
    return 0;
}

int launch_lat_fwd(const Ctx& c, const mmvae_noise* nz, const float* params, float* bn_running, int64_t* nbt,
                   int32_t* labels) {
    LatArgs a = make_lat_args(c);
    a.labels = labels;
    NoiseDev nd = make_noise_dev(nz, c.h);
    const size_t shm = lat_smem_bytes(c.d);
    if (c.plan.lat_half) {
        // (lat_fork_rides implies lat_half, i.e. this launch)
        launch_k(c, c.plan.lat_fork_rides ? c.ev(EV_LAT) : nullptr, k_lat_fwd_h, dim3(c.lay.nblkl, c.d.A), dim3(64 * LH_NW), shm, a, nd, params, c.ws, bn_running, nbt);
        HIP_LAUNCH_CHECK("k_lat_fwd_h");
        return 0;
    }
    hipLaunchKernelGGL(k_lat_fwd, dim3(c.lay.nblkl, c.d.A), dim3(64 * LAT_NW), shm, c.stream, a, nd, params, c.ws,
                       bn_running, nbt);
    HIP_LAUNCH_CHECK("k_lat_fwd");
    return 0;
}

int launch_couple(const Ctx& c) {
    const mmvae_dims& d = c.d;
    const Layout& L = c.lay;
    const bool acc = c.h.training && c.use_acc();
    long long* t_acc = acc ? reinterpret_cast<long long*>(c.ws + acc_set_off(L, d.A, ACC_T)) : nullptr;
    const long long* c_acc = acc ? reinterpret_cast<const long long*>(c.ws + acc_set_off(L, d.A, ACC_C)) : nullptr;
    if (acc) {   // the T sums start at zero every time the coupling runs (it may run more than once per forward pass)
        hipError_t e = hipMemsetAsync(t_acc, 0, sizeof(float) * (size_t)d.A * ACC_SET_FLOATS, c.stream);
        if (e != hipSuccess) { set_error("memset: %s", hipGetErrorString(e)); return MMVAE_E_LAUNCH; }
    }
#define MMVAE_COUPLE(AT)                                                                                               \
    hipLaunchKernelGGL(k_couple<AT>, dim3(L.nblk32), dim3(256), 0, c.stream, d.B, d.C, c.h.eps, c.h.lam, c.ws + L.CC,    \
                       c.ws + L.CSMP, c.ws + L.c_part, L.nblkl, c_acc, c.ws + L.c_mean, c.ws + L.c_iv,                    \
                       c.ws + L.couple_part, c.ws + L.T_part, t_acc)
    switch (d.A) {
        case 1: MMVAE_COUPLE(1); break;
        case 2: MMVAE_COUPLE(2); break;
        case 3: MMVAE_COUPLE(3); break;
        case 4: MMVAE_COUPLE(4); break;
        case 5: MMVAE_COUPLE(5); break;
        case 6: MMVAE_COUPLE(6); break;
        case 7: MMVAE_COUPLE(7); break;
        default: MMVAE_COUPLE(8); break;
    }
#undef MMVAE_COUPLE
    HIP_LAUNCH_CHECK("k_couple");
    return 0;
}

int launch_loss_finalize(const Ctx& c, float* loss_out, int mode, const double* zrec) {
    const mmvae_dims& d = c.d;
    const Layout& L = c.lay;
    if (c.h.training && c.use_acc()) {   // the coupling kernel has added the T sums to their accumulator set itself
        if (mode == 1) return 0;
        mode = 2;
    }
    const int nT = cdiv(d.A * d.C, 32);
    hipLaunchKernelGGL(k_loss_finalize, dim3(mode == 0 ? 1 + nT : (mode == 1 ? nT : 1)), dim3(256), 0, c.stream, d.A, d.B, d.D, d.C,
                       c.h.beta, c.h.lam, c.ws + L.fc11_part, L.n11, c.ws + L.lat_part, L.nblkl, L.nblk32, c.ws + L.couple_part,
                       c.ws + L.T_part, c.ws + L.T, loss_out, mode, zrec);
    HIP_LAUNCH_CHECK("k_loss_finalize");
    return 0;
}

int launch_lat_bwd(const Ctx& c, const mmvae_noise* nz, const float* params) {
    LatArgs a = make_lat_args(c);
    NoiseDev nd = make_noise_dev(nz, c.h);
    const size_t shm = lat_smem_bytes(c.d);
    const dim3 grid(cdiv(c.d.B, LAT_ROWS_BWD), c.d.A);
    // k_lat_bwd_h: the half-wave form, k_lat_bwd: the wave form; the arm count is a template parameter (check_dims: 1 .. 8)
#define MMVAE_LAT_BWD(AT)                                                                                                  \
    if (c.plan.lat_half)                                                                                                   \
        hipLaunchKernelGGL((k_lat_bwd_g<32, LBH_NW, AT>), grid, dim3(64 * LBH_NW), shm, c.stream, a, nd, params, c.ws);    \
    else                                                                                                                   \
        hipLaunchKernelGGL((k_lat_bwd_g<64, LATB_NW, AT>), grid, dim3(64 * LATB_NW), shm, c.stream, a, nd, params, c.ws)
    static_assert(MMVAE_MAX_ARMS == 8, "one case per arm count");
    switch (c.d.A) {
        case 1: MMVAE_LAT_BWD(1); break;
        case 2: MMVAE_LAT_BWD(2); break;
        case 3: MMVAE_LAT_BWD(3); break;
        case 4: MMVAE_LAT_BWD(4); break;
        case 5: MMVAE_LAT_BWD(5); break;
        case 6: MMVAE_LAT_BWD(6); break;
        case 7: MMVAE_LAT_BWD(7); break;
        case 8: MMVAE_LAT_BWD(8); break;
        default: set_error("k_lat_bwd: A = %d outside [1, %d]", c.d.A, MMVAE_MAX_ARMS); return MMVAE_E_UNSUPPORTED;
    }
#undef MMVAE_LAT_BWD
    HIP_LAUNCH_CHECK(c.plan.lat_half ? "k_lat_bwd_h" : "k_lat_bwd");
    return 0;
}

// which: bit 0 = fc11.weight / fc11.bias (final as soon as the dW11 GEMM is), bit 1 = everything else
int launch_reduce_grads(const Ctx& c, float* grads, float gscale, const AdamHost* ah, int which) {
    const mmvae_dims& d = c.d;
    const Layout& L = c.lay;
    const int A = d.A, H = d.H, D = d.D, Ld = d.L, C = d.C, S = d.S;
    RedDescs ds{};
    int n = 0;
    const float xscale = c.dropout() ? 1.f / (1.f - c.h.x_drop) : 1.f;
    // big: fc1.w, fc11.w, fc11.b
    const int ks11 = c.plan.dw11_slabs;
    ds.d[n++] = RedDesc{c.ws + L.dw1_slab, (int64_t)A * H * D, (int64_t)H * D, D, 0, H, D, c.po.o[0], D, gscale * xscale, L.sp.ks_dw};
    ds.d[n++] = RedDesc{c.ws + L.dw11_slab, (int64_t)A * D * DW11_LD, (int64_t)D * DW11_LD, DW11_LD, 0, D, H, c.po.o[26], H, gscale, ks11};
    ds.d[n++] = RedDesc{c.ws + L.dw11_slab, (int64_t)A * D * DW11_LD, (int64_t)D * DW11_LD, DW11_LD, H, D, 1, c.po.o[27], 1, gscale, ks11};
    const int nbig = n;
    const int64_t sks = (int64_t)A * N_SMALL * NP * SMALL_LD, sarm = (int64_t)N_SMALL * NP * SMALL_LD;
    auto small = [&](int i, int N, int K, int64_t w_off, int64_t b_off) {
        const float* s = c.ws + L.small_slab + (int64_t)i * NP * SMALL_LD;
        if (K > 0) ds.d[n++] = RedDesc{s, sks, sarm, SMALL_LD, 0, N, K, w_off, K, gscale, L.sp.ks_small};
        ds.d[n++] = RedDesc{s, sks, sarm, SMALL_LD, K, N, 1, b_off, 1, gscale, L.sp.ks_small};
    };
    small(0, H, H, c.po.o[2], c.po.o[3]);
    small(1, H, H, c.po.o[4], c.po.o[5]);
    small(2, H, H, c.po.o[6], c.po.o[7]);
    small(3, Ld, H, c.po.o[8], c.po.o[9]);
    small(4, C, Ld, c.po.o[10], c.po.o[11]);
    small(5, 2 * S, Ld + C, c.po.o[12], c.po.o[14]);   // fc_mu / fc_sigma are adjacent in the flat layout
    small(6, Ld, C + S, c.po.o[16], c.po.o[17]);
    small(7, H, Ld, c.po.o[18], c.po.o[19]);
    small(8, H, H, c.po.o[20], c.po.o[21]);
    small(9, H, H, c.po.o[22], c.po.o[23]);
    small(10, H, H, c.po.o[24], c.po.o[25]);
    small(11, H, 0, 0, c.po.o[1]);                     // fc1.b = column sums of dZ1
    AdamArgs aa{};
    if (ah && ah->p) {
        const double bc1 = 1.0 - pow((double)ah->b1, (double)ah->step);
        const double bc2 = 1.0 - pow((double)ah->b2, (double)ah->step);
        aa = AdamArgs{ah->p, ah->m, ah->v, (float)(ah->lr / bc1), (float)(1.0 / sqrt(bc2)), ah->b1, ah->b2, ah->eps,
                      ah->wd, ah->lr, ah->decoupled};
    }
    // which: 1 = the fc11 tensors (behind dW11, on whatever stream that ran), 2 = fc1.w and the small tensors, 3 = everything
    const int64_t big_elems = (int64_t)max(H, 1) * D;
    const int gx = (int)imin64(2048, cdiv64(big_elems / 4, 256));
    RedDescs out{};
    int no = 0, blocks = 0;
    auto add = [&](const RedDesc& r, int nb) { out.d[no] = r; out.first[no++] = blocks; blocks += nb; };
    if (which & 2) add(ds.d[0], gx);
    if (which & 1) { add(ds.d[1], gx); add(ds.d[2], cdiv(D, 256)); }
    if (which & 2)
        for (int i = nbig; i < n; ++i) add(ds.d[i], 16);
    out.first[no] = blocks;
    out.n = no;
    if (no) hipLaunchKernelGGL(k_reduce, dim3(blocks, 1, A), dim3(256), 0, c.stream, out, grads, c.po.per_arm, aa);
    HIP_LAUNCH_CHECK("k_reduce");
    return 0;
}

int launch_adam(int64_t n, float* p, const float* g, float* m, float* v, int64_t step, float lr, float b1, float b2,
                float eps, float wd, int decoupled, hipStream_t s) {
    const double bc1 = 1.0 - pow((double)b1, (double)step);
    const double bc2 = 1.0 - pow((double)b2, (double)step);
    const int blocks = (int)imin64(4096, cdiv64(n, 256));
    hipLaunchKernelGGL(k_adam, dim3(blocks), dim3(256), 0, s, n, p, g, m, v, (float)(lr / bc1), (float)(1.0 / sqrt(bc2)),
                       b1, b2, eps, wd, lr, decoupled);
    HIP_LAUNCH_CHECK("k_adam");
    return 0;
}

int launch_dump_noise(const mmvae_dims& d, const mmvae_hyper& h, const mmvae_noise* nz, uint8_t* x_mask,
                      float* u_gumbel, float* u_state, uint8_t* s_mask, hipStream_t s) {
    NoiseDev nd = make_noise_dev(nz, h);
    hipLaunchKernelGGL(k_dump_noise, dim3(2048), dim3(256), 0, s, nd, d.A, d.B, d.D, d.C, d.S, x_mask, u_gumbel, u_state,
                       s_mask);
    HIP_LAUNCH_CHECK("k_dump_noise");
    return 0;
}

// ---------------------------------------------------------------------------------------------
// decoder input rows [c | s] (ZinBuild, common.hpp), one element per thread.  Decode copies the caller's c and s.  The
// traversal (mixVAE_model.state_changes, nn_model.py:370-411) writes row r = samp * B + b of arm a as the encoder's c_smp of
// cell b and s = mu of cell b, except s[d_s] = u * sqrt(exp(log(v))) + mu[d_s] with v = sigmoid(fc_sigma(y))[d_s] recomputed
// in fp32 from y = [x_low | c] (the latent kernel keeps log(v + eps), not v; the reference's reparameterize takes log(v)
// without eps), the product and the sum rounded separately as torch's eps.mul(std).add(mu) does.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_zin_build(const ZinBuild z, const NoiseDev nd) {
    const int W = z.C + z.S;
    const int64_t n = (int64_t)z.A * z.R * W;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int col = (int)(i % W);
        const int64_t ar = i / W;
        const int r = (int)(ar % z.R), a = (int)(ar / z.R);
        float v;
        if (!z.enc_ws) {
            v = col < z.C ? z.c[a * z.c_arm + (int64_t)r * z.C + col] : z.s[a * z.s_arm + (int64_t)r * z.S + (col - z.C)];
        } else {
            const int64_t ab = (int64_t)a * z.B + r % z.B;
            if (col < z.C) {
                v = z.enc_ws[z.csmp + ab * z.C + col];
            } else {
                const int j = col - z.C;
                const float mu = z.enc_ws[z.mu + ab * z.S + j];
                if (j != z.d_s) {
                    v = mu;
                } else {
                    const int K = z.L + z.C;
                    const float* y = z.enc_ws + z.y + ab * K;
                    const float* w = z.params + a * z.per_arm + z.o_wsig + (int64_t)z.d_s * K;
                    float acc = 0.f;
                    for (int k = 0; k < K; ++k) acc = fmaf(y[k], w[k], acc);
                    acc += z.params[a * z.per_arm + z.o_bsig + z.d_s];
                    const float var = 1.f / (1.f + expf(-acc));
                    const float sd = sqrtf(expf(logf(var)));
                    const float u = z.u ? z.u[(int64_t)a * z.R + r] : noise_uniform(nd, a, STREAM_STATE, (uint64_t)r);
                    v = __fadd_rn(__fmul_rn(u, sd), mu);
                }
            }
        }
        z.zin[i] = v;
    }
}

int launch_zin_build(const ZinBuild& z, const mmvae_noise* nz, const mmvae_hyper& h, hipStream_t s) {
    const int64_t n = (int64_t)z.A * z.R * (z.C + z.S);
    const NoiseDev nd = make_noise_dev(nz, h);
    hipLaunchKernelGGL(k_zin_build, dim3((unsigned)imin64(4096, cdiv64(n, 256))), dim3(256), 0, s, z, nd);
    HIP_LAUNCH_CHECK("k_zin_build");
    return 0;
}

// ---------------------------------------------------------------------------------------------
// mixVAE_model.intermed (nn_model.py:271-275) on the caller's rows: mu = fc_mu(y), var = sigmoid(fc_sigma(y)), y [A][N][K],
// K = L + C <= 192 (the log with eps belongs to forward, :350).  The state head [fc_mu.w; fc_sigma.w] is one [2 S][K] matrix
// in the parameter buffer (make_poff), the biases one [2 S] vector: both are staged in LDS once per workgroup, which then
// walks row groups grid-stride.  A wave owns IM_RPW rows at a time: lane l holds y[row][l + 64 t], t < IM_KT, in registers,
// output o is a wavefront reduction of the lanes' partial products (lane o keeps it), lane s < S stores mu and var.
// grid (row groups, A), 64 IM_NW threads.
// ---------------------------------------------------------------------------------------------
constexpr int IM_NW = 4, IM_RPW = 4, IM_KT = 4;   // 16 rows per workgroup pass; 64 IM_KT >= 192 inputs
__global__ __launch_bounds__(64 * IM_NW) void k_intermed(int N, int K, int S, const float* __restrict__ params, int64_t per_arm,
                                                         int64_t o_wms, int64_t o_bms, const float* __restrict__ y,
                                                         int64_t y_arm_stride, float* __restrict__ mu, float* __restrict__ var) {
    extern __shared__ __attribute__((aligned(16))) float im_smem[];   // [2S][K] weights, [2S] biases
    const int arm = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const float* P = params + (int64_t)arm * per_arm;
    float* Wms = im_smem;
    float* bms = im_smem + 2 * S * K;
    for (int i = threadIdx.x; i < 2 * S * K; i += blockDim.x) Wms[i] = P[o_wms + i];
    for (int i = threadIdx.x; i < 2 * S; i += blockDim.x) bms[i] = P[o_bms + i];
    __syncthreads();
    const float* ya = y + (int64_t)arm * y_arm_stride;
    const int64_t ngroups = ((int64_t)N + IM_NW * IM_RPW - 1) / (IM_NW * IM_RPW);
    for (int64_t g = blockIdx.x; g < ngroups; g += gridDim.x) {
        const int64_t row0 = g * (IM_NW * IM_RPW) + wv * IM_RPW;
        float yv[IM_RPW][IM_KT];
#pragma unroll
        for (int r = 0; r < IM_RPW; ++r)
#pragma unroll
            for (int t = 0; t < IM_KT; ++t) {
                const int k = lane + 64 * t;
                yv[r][t] = (row0 + r < N && k < K) ? ya[(row0 + r) * K + k] : 0.f;
            }
        float ms[IM_RPW];
#pragma unroll
        for (int r = 0; r < IM_RPW; ++r) ms[r] = 0.f;
        for (int o = 0; o < 2 * S; ++o) {
            float w[IM_KT];
#pragma unroll
            for (int t = 0; t < IM_KT; ++t) w[t] = lane + 64 * t < K ? Wms[o * K + lane + 64 * t] : 0.f;
            const float bo = bms[o];
#pragma unroll
            for (int r = 0; r < IM_RPW; ++r) {
                float pr = 0.f;
#pragma unroll
                for (int t = 0; t < IM_KT; ++t) pr = fmaf(yv[r][t], w[t], pr);
                const float pv = wave_sum(pr) + bo;
                if (lane == o) ms[r] = pv;
            }
        }
#pragma unroll
        for (int r = 0; r < IM_RPW; ++r) {
            const float sg = __shfl(ms[r], (lane + S) & 63, 64);   // lane s reads fc_sigma's output s
            if (row0 + r < N && lane < S) {
                const int64_t o = ((int64_t)arm * N + row0 + r) * S + lane;
                mu[o] = ms[r];
                var[o] = 1.f / (1.f + expf(-sg));
            }
        }
    }
}

int launch_intermed(const mmvae_dims& d, const POff& po, const float* params, const float* y, int64_t y_arm_stride, float* mu,
                    float* var, hipStream_t s) {
    const int K = d.L + d.C;
    const size_t shm = (size_t)(2 * d.S * K + 2 * d.S) * sizeof(float);   // at most 2 x 32 x (64 + 128) + 64 floats = 48 KB
    const int64_t ngroups = cdiv64(d.B, IM_NW * IM_RPW);
    hipLaunchKernelGGL(k_intermed, dim3((unsigned)imin64(1024, ngroups), d.A), dim3(64 * IM_NW), shm, s, d.B, K, d.S, params,
                       po.per_arm, po.o[12], po.o[14], y, y_arm_stride, mu, var);
    HIP_LAUNCH_CHECK("k_intermed");
    return 0;
}

}  // namespace mmvae

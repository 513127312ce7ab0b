// The 64 x 64 tile that zinb.hip, zinb_grad.hip and countdist.hip share: the heads' pre-activations of a tile (zb_run: the
// one weight staging and the one run of matrix instructions; zb_products is zb_run on chunks of d10, the gradient kernels
// run it on d10 rows that stay in LDS) and the per-cell / per-gene sums of a wave's 32 x 32 sub-tile (zb_reduce).  A
// workgroup of four waves owns 64 cells x 64 genes, wave w the 32 x 32 sub-tile (w & 1, w >> 1); the layout, the K chunks and
// the sums are described at the top of zinb.hip.  The partials that zb_reduce leaves are added by zb_finish (zinb.hip;
// declared in common.hpp, as ZbHeads is).
#pragma once
#include "common.hpp"

namespace mmvae {

constexpr int ZB_T = 64;             // cells and genes of a workgroup's tile
constexpr int ZB_THREADS = 256;

constexpr int ZB_KC = 32;            // the K extent of one LDS chunk (even: whole steps of the instruction's k = 2)
constexpr int ZB_P = ZB_KC + 1;      // the LDS row pitch in floats, odd

template <int NH>
constexpr size_t zb_lds_bytes(bool dump) {
    const size_t stage = (size_t)(ZB_T + ZB_T * NH) * ZB_P;
    const size_t regs = dump ? (size_t)4 * NH * 16 * 64 : 0;
    return sizeof(float) * (stage > regs ? stage : regs);
}

// the row of the wave's 32 x 32 sub-tile that register g of lane half h holds (the 32x32 C/D map; the column is lane & 31)
__device__ __forceinline__ int zb_row(int g, int h) { return (g & 3) + 8 * (g >> 2) + 4 * h; }

// K chunk k0 .. k0 + 31 of the weights into LDS: rows 64 j .. 64 j + 63 of `rows` the weights of head j's genes, at pitch ZB_P;
// genes past D and k >= H are zero
template <int NH>
__device__ __forceinline__ void zb_stage_weights(float* rows, const ZbHeads<NH>& hd, int64_t gene0, int D, int H, int k0) {
#pragma unroll
    for (int j = 0; j < NH; ++j) {
        float* dst = rows + ZB_T * j * ZB_P;
        for (int idx = threadIdx.x; idx < ZB_T * ZB_KC; idx += ZB_THREADS) {
            const int r = idx / ZB_KC, k = idx % ZB_KC;
            const int64_t gene = gene0 + r;
            dst[r * ZB_P + k] = (gene < D && k0 + k < H) ? hd.W[j][gene * H + k0 + k] : 0.f;
        }
    }
}

// the wave's 32 x 32 pre-activations of every head: A = d10 (lane l: cell l & 31, k = l >> 5), B = the weights (gene
// l & 31, k = l >> 5), C = the gene's bias; chunk after chunk, k rising.  `a` is the lane's first A element in LDS, and
// chunk k0 of its row starts a_step k0 floats on: 0 where stage_a(k0) stages the chunk afresh (zb_products), 1 where the
// row is resident whole (zinb_grad.hip).  `rows` takes the weight chunks.  Ends behind a barrier: the chunks are free again.
template <int NH, class StageA>
__device__ __forceinline__ void zb_run(const float* a, int a_step, StageA&& stage_a, float* rows, const ZbHeads<NH>& hd, int64_t gene0, int D,
                                       int H, int wn, int lane, const float (&bias)[NH], f32x16 (&acc)[NH]) {
#pragma unroll
    for (int j = 0; j < NH; ++j)
#pragma unroll
        for (int g = 0; g < 16; ++g) acc[j][g] = bias[j];
    const float* b = rows + (wn * 32 + (lane & 31)) * ZB_P + (lane >> 5);
    for (int k0 = 0; k0 < H; k0 += ZB_KC) {
        stage_a(k0);
        zb_stage_weights<NH>(rows, hd, gene0, D, H, k0);
        __syncthreads();
        const int kc = H - k0 < ZB_KC ? (H - k0 + 1) & ~1 : ZB_KC;
        for (int k = 0; k < kc; k += 2) {
            const float av = a[a_step * k0 + k];
#pragma unroll
            for (int j = 0; j < NH; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b[j * ZB_T * ZB_P + k], acc[j], 0, 0, 0);
        }
        __syncthreads();                 // every wave is done with the chunk
    }
}

// the bias of the lane's gene under every head, 0 past D: C of zb_run
template <int NH>
__device__ __forceinline__ void zb_bias(const ZbHeads<NH>& hd, int64_t gene, int D, float (&bias)[NH]) {
#pragma unroll
    for (int j = 0; j < NH; ++j) bias[j] = gene < D ? hd.b[j][gene] : 0.f;
}

// zb_run on chunks of d10: rows 0..63 of `lds` take the cells' chunk (cells past N and k >= H zero), the rows behind them
// the weights
template <int NH>
__device__ inline void zb_products(float* lds, const float* __restrict__ d10, int64_t ldh, int64_t cell0, int64_t N, const ZbHeads<NH>& hd,
                                   int64_t gene0, int D, int H, int wm, int wn, int lane, f32x16 (&acc)[NH]) {
    float bias[NH];
    zb_bias<NH>(hd, gene0 + wn * 32 + (lane & 31), D, bias);
    zb_run<NH>(
        lds + (wm * 32 + (lane & 31)) * ZB_P + (lane >> 5), 0,
        [&](int k0) {
            for (int idx = threadIdx.x; idx < ZB_T * ZB_KC; idx += ZB_THREADS) {
                const int r = idx / ZB_KC, k = idx % ZB_KC;
                const int64_t cell = cell0 + r;
                lds[r * ZB_P + k] = (cell < N && k0 + k < H) ? d10[cell * ldh + k0 + k] : 0.f;
            }
        },
        lds + ZB_T * ZB_P, hd, gene0, D, H, wn, lane, bias, acc);
}

// The sums of the wave's sub-tile.  term(g, cell, gene) is asked for the valid elements only; the others count an exact 0.
// gene partial: the lane's cells in register order from 0.0, then lane + (lane xor 32).  cell partial of register g: the
// 32 genes by c <- c + c(lane xor s), s = 16, 8, 4, 2, 1.
template <class Term>
__device__ inline void zb_reduce(Term&& term, int lane, int64_t cell0, int64_t gene0, int64_t N, int D, double* __restrict__ ws_cell,
                                 double* __restrict__ ws_gene) {
    const int h = lane >> 5;
    const int64_t gene = gene0 + (lane & 31);
    double gsum = 0.0, mine = 0.0;
#pragma unroll 1
    for (int g = 0; g < 16; ++g) {
        const int64_t cell = cell0 + zb_row(g, h);
        double t = 0.0;
        if (cell < N && gene < D) t = term(g, cell, gene);
        gsum += t;
        for (int s = 16; s > 0; s >>= 1) t += __shfl_xor(t, s);
        if ((lane & 15) == g) mine = t;
    }
    gsum += __shfl_xor(gsum, 32);
    if (lane < 32 && gene < D) ws_gene[(cell0 >> 5) * D + gene] = gsum;
    const int64_t cell = cell0 + zb_row(lane & 15, h);
    if ((lane & 31) < 16 && cell < N) ws_cell[(gene0 >> 5) * N + cell] = mine;
}

}  // namespace mmvae

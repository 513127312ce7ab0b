// The 64 x 64 tile that zinb.hip and countdist.hip share: the heads' products of a tile from d10 (zb_products) and the
// per-cell / per-gene sums of a wave's 32 x 32 sub-tile (zb_reduce).  A workgroup of four waves owns 64 cells x 64 genes,
// wave w the 32 x 32 sub-tile (w & 1, w >> 1); the layout, the K chunks and the sums are described at the top of zinb.hip.
// The partials that zb_reduce leaves are added by zb_finish (zinb.hip; declared in common.hpp).
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

template <int NH>
struct ZbHeads {
    const float* W[NH];      // [D, H] each, nn.Linear's layout
    const float* b[NH];      // [D]
};

// the row of the wave's 32 x 32 sub-tile that register g of lane half h holds (the 32x32 C/D map; the column is lane & 31)
__device__ __forceinline__ int zb_row(int g, int h) { return (g & 3) + 8 * (g >> 2) + 4 * h; }

// K chunk k0 .. k0 + 31 of the tile's operands into LDS: rows 0..63 the cells' d10, rows 64 + 64 j .. the weights of head
// j's genes; cells past N, genes past D and k >= H are zero
template <int NH>
__device__ inline void zb_stage(float* lds, const float* __restrict__ d10, int64_t ldh, int64_t cell0, int64_t N, const ZbHeads<NH>& hd,
                                int64_t gene0, int D, int H, int k0) {
    for (int idx = threadIdx.x; idx < ZB_T * ZB_KC; idx += ZB_THREADS) {
        const int r = idx / ZB_KC, k = idx % ZB_KC;
        const int64_t cell = cell0 + r;
        lds[r * ZB_P + k] = (cell < N && k0 + k < H) ? d10[cell * ldh + k0 + k] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < NH; ++j) {
        float* dst = lds + (ZB_T + ZB_T * j) * ZB_P;
        for (int idx = threadIdx.x; idx < ZB_T * ZB_KC; idx += ZB_THREADS) {
            const int r = idx / ZB_KC, k = idx % ZB_KC;
            const int64_t gene = gene0 + r;
            dst[r * ZB_P + k] = (gene < D && k0 + k < H) ? hd.W[j][gene * H + k0 + k] : 0.f;
        }
    }
}

// the wave's 32 x 32 pre-activations of every head: A = d10 (lane l: cell l & 31, k = l >> 5), B = the weights (gene
// l & 31, k = l >> 5), C = the gene's bias; chunk after chunk, k rising.  Ends behind a barrier: LDS is free again.
template <int NH>
__device__ inline void zb_products(float* lds, const float* __restrict__ d10, int64_t ldh, int64_t cell0, int64_t N, const ZbHeads<NH>& hd,
                                   int64_t gene0, int D, int H, int wm, int wn, int lane, f32x16 (&acc)[NH]) {
    const int i = lane & 31, kh = lane >> 5;
    const int64_t gene = gene0 + wn * 32 + i;
#pragma unroll
    for (int j = 0; j < NH; ++j) {
        const float bj = gene < D ? hd.b[j][gene] : 0.f;
#pragma unroll
        for (int g = 0; g < 16; ++g) acc[j][g] = bj;
    }
    const float* a = lds + (wm * 32 + i) * ZB_P + kh;
    const float* b = lds + (ZB_T + wn * 32 + i) * ZB_P + kh;
    for (int k0 = 0; k0 < H; k0 += ZB_KC) {
        zb_stage<NH>(lds, d10, ldh, cell0, N, hd, gene0, D, H, k0);
        __syncthreads();
        const int kc = H - k0 < ZB_KC ? (H - k0 + 1) & ~1 : ZB_KC;
        for (int k = 0; k < kc; k += 2) {
            const float av = a[k];
#pragma unroll
            for (int j = 0; j < NH; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b[j * ZB_T * ZB_P + k], acc[j], 0, 0, 0);
        }
        __syncthreads();                 // every wave is done with the chunk
    }
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

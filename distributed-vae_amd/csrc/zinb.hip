// Zero-inflated negative binomial inference (mmidas/nn_model.py: decoder_zinb :289-295, zinb_loss :642-676; include/mmvae.h,
// DESIGN.md section 9k).  Three entry points share one tile shape, one term and one reduction:
//   mmvae_zinb_heads   x_p = sigmoid(fc11_p(d10)), x_r = sigmoid(fc11_r(d10)), written out;
//   mmvae_zinb_nll     the three heads of a tile from d10, the term of every element in the epilogue, per-cell and per-gene
//                      sums; no head is written;
//   mmvae_zinb_terms   the same sums from heads the caller gives, the terms optionally written.
// A workgroup of four waves owns 64 cells x 64 genes, wave w the 32 x 32 sub-tile (w & 1, w >> 1).  The d10 tile and the
// heads' weight tiles pass through LDS in K chunks of 32 (rows of an odd pitch, 33 floats): H <= 128 would fit whole, 103 KB
// at H = 100, but then a CU holds one workgroup and nothing overlaps its staging, its products and its fp64 epilogue; in
// chunks the tiles take 34 KB, the accumulator image of the epilogue 48 KB, and three workgroups share a CU.  The products
// are one run of v_mfma_f32_32x32x2_f32 per head with the bias as C, k rising through the chunks: every pre-activation is
// the k-ordered fp32 fma chain fma(h_{H-1}, w_{H-1}, ... fma(h_0, w_0, b)), whatever the other rows and columns of the call are.
// The term and everything behind the fp32 pre-activation is fp64.  Sums: a sub-tile leaves, for each of its cells, the sum
// over its 32 genes (a butterfly over the lanes: the pairwise tree on the gene index), and for each of its genes the sum over
// its 32 cells (a lane's 16 cells in register order, then the two lane halves); k_zb_finish adds the sub-tiles' partials
// in tile order.  No atomics: bit-identical from run to run, and a cell's sum depends on that cell's row alone.
// The tile's products and sums (zb_run under zb_products, zb_reduce) live in zb_tile.hpp, which countdist.hip and zinb_grad.hip
// share; the element's term, its gates and what they read from the pre-activations (zinb_term, zb_gate, zb_operands) in
// zinb_core.hpp, which zinb_grad.hip and the host's restatement share.
#include "zb_tile.hpp"
#include "zinb_core.hpp"

namespace mmvae {

__global__ __launch_bounds__(ZB_THREADS) void k_zb_heads(const float* __restrict__ d10, int64_t ldh, int64_t N, int H, int D, ZbHeads<2> hd,
                                                         float* __restrict__ x_p, float* __restrict__ x_r, int64_t ldo, int tiles_n) {
    __shared__ float zb_lds[zb_lds_bytes<2>(false) / sizeof(float)];
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wm = w & 1, wn = w >> 1;
    const int64_t cell0 = (int64_t)(blockIdx.x / tiles_n) * ZB_T, gene0 = (int64_t)(blockIdx.x % tiles_n) * ZB_T;
    const int64_t gene = gene0 + wn * 32 + (lane & 31);
    f32x16 acc[2];
    zb_products<2>(zb_lds, d10, ldh, cell0, N, hd, gene0, D, H, wm, wn, lane, acc);
    if (gene >= D) return;
#pragma unroll
    for (int g = 0; g < 16; ++g) {
        const int64_t cell = cell0 + wm * 32 + zb_row(g, lane >> 5);
        if (cell < N) {
            // sigmoid in fp64, rounded once
            x_p[cell * ldo + gene] = (float)(1.0 / (1.0 + exp(-(double)acc[0][g])));
            x_r[cell * ldo + gene] = (float)(1.0 / (1.0 + exp(-(double)acc[1][g])));
        }
    }
}

__global__ __launch_bounds__(ZB_THREADS) void k_zb_nll(const float* __restrict__ d10, int64_t ldh, int64_t N, int H, int D, ZbHeads<3> hd,
                                                       const float* __restrict__ X, int64_t ldx, double eps, double* __restrict__ ws_cell,
                                                       double* __restrict__ ws_gene, int tiles_n) {
    __shared__ float zb_lds[zb_lds_bytes<3>(true) / sizeof(float)];
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wm = w & 1, wn = w >> 1;
    const int64_t cell0 = (int64_t)(blockIdx.x / tiles_n) * ZB_T, gene0 = (int64_t)(blockIdx.x % tiles_n) * ZB_T;
    f32x16 acc[3];
    zb_products<3>(zb_lds, d10, ldh, cell0, N, hd, gene0, D, H, wm, wn, lane, acc);
    // every wave is done with the operands: LDS now holds the accumulators, [head][register][lane] per wave, so that the
    // term loop can stay rolled (unrolled, 16 copies of the fp64 term would not fit the instruction cache)
    float* mine = zb_lds + w * (3 * 16 * 64) + lane;
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int g = 0; g < 16; ++g) mine[(j * 16 + g) * 64] = acc[j][g];
    const int64_t wc0 = cell0 + wm * 32, wg0 = gene0 + wn * 32;
    if (wc0 >= N || wg0 >= D) return;                  // (no barrier follows)
    zb_reduce(
        [&](int g, int64_t cell, int64_t gene) {
            const float a_rec = mine[g * 64], a_p = mine[(16 + g) * 64], a_r = mine[(32 + g) * 64];
            return zinb_term(zb_operands(X[cell * ldx + gene], a_rec, a_p, a_r, eps));
        },
        lane, wc0, wg0, N, D, ws_cell, ws_gene);
}

__global__ __launch_bounds__(ZB_THREADS) void k_zb_terms(const float* __restrict__ x_rec, int64_t ld_rec, const float* __restrict__ x_p,
                                                         int64_t ld_p, const float* __restrict__ x_r, int64_t ld_r,
                                                         const float* __restrict__ X, int64_t ldx, int64_t N, int D, double eps,
                                                         double* __restrict__ ws_cell, double* __restrict__ ws_gene,
                                                         float* __restrict__ terms, int64_t ld_t, int tiles_n) {
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t wc0 = (int64_t)(blockIdx.x / tiles_n) * ZB_T + (w & 1) * 32, wg0 = (int64_t)(blockIdx.x % tiles_n) * ZB_T + (w >> 1) * 32;
    if (wc0 >= N || wg0 >= D) return;
    zb_reduce(
        [&](int, int64_t cell, int64_t gene) {
            const double p = (1.0 - eps) * ((double)x_p[cell * ld_p + gene] + eps);
            const double z = (1.0 - eps) * ((double)x_r[cell * ld_r + gene] + eps);
            const double t = zinb_term((double)X[cell * ldx + gene], (double)x_rec[cell * ld_rec + gene] + eps, p, 1.0 - p, z, 1.0 - z);
            if (terms) terms[cell * ld_t + gene] = (float)t;
            return t;
        },
        lane, wc0, wg0, N, D, ws_cell, ws_gene);
}

// cell_sum[i] = the partials of the cell over the 32-gene sub-tiles, gene_sum[d] = those of the gene over the 32-cell
// sub-tiles, each added in tile order from 0.0
__global__ __launch_bounds__(256) void k_zb_finish(const double* __restrict__ ws_cell, const double* __restrict__ ws_gene, int64_t N, int D,
                                                   double* __restrict__ cell_sum, double* __restrict__ gene_sum) {
    const int64_t n_gt = cdiv64(D, 32), n_ct = cdiv64(N, 32);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < N + D; i += (int64_t)gridDim.x * 256) {
        double s = 0.0;
        if (i < N) {
            for (int64_t t = 0; t < n_gt; ++t) s += ws_cell[t * N + i];
            cell_sum[i] = s;
        } else {
            for (int64_t t = 0; t < n_ct; ++t) s += ws_gene[t * D + (i - N)];
            gene_sum[i - N] = s;
        }
    }
}

size_t zb_ws_bytes(int64_t N, int D) {
    return bytes_or_0(8 * ((unsigned __int128)cdiv64(D, 32) * (unsigned __int128)N + (unsigned __int128)cdiv64(N, 32) * (unsigned __int128)D));
}

// the tiles of one grid, 0 where a grid cannot hold them
int64_t zb_tiles(int64_t N, int D) {
    const unsigned __int128 t = (unsigned __int128)cdiv64(N, ZB_T) * (unsigned __int128)cdiv64(D, ZB_T);
    return t > (unsigned __int128)INT32_MAX ? 0 : (int64_t)t;
}

int zb_finish(void* ws, int64_t N, int D, double* cell_sum, double* gene_sum, hipStream_t st) {
    double* ws_cell = static_cast<double*>(ws);
    const unsigned gx = (unsigned)imin64(cdiv64(N + D, 256), 1 << 20);
    hipLaunchKernelGGL(k_zb_finish, dim3(gx), dim3(256), 0, st, ws_cell, ws_cell + cdiv64(D, 32) * N, N, D, cell_sum, gene_sum);
    HIP_LAUNCH_CHECK("k_zb_finish");
    return 0;
}

int launch_zinb_heads(const float* d10, int64_t ldh, int64_t N, int H, int D, const float* Wp, const float* bp, const float* Wr,
                      const float* br, float* x_p, float* x_r, int64_t ldo, hipStream_t st) {
    ZbHeads<2> hd{{Wp, Wr}, {bp, br}};
    hipLaunchKernelGGL(k_zb_heads, dim3((unsigned)zb_tiles(N, D)), dim3(ZB_THREADS), 0, st, d10, ldh, N, H, D, hd, x_p, x_r, ldo,
                       (int)cdiv64(D, ZB_T));
    HIP_LAUNCH_CHECK("k_zb_heads");
    return 0;
}

int launch_zinb_nll(const ZinbIn& in, void* ws, double* cell_sum, double* gene_sum, hipStream_t st) {
    double* ws_cell = static_cast<double*>(ws);
    hipLaunchKernelGGL(k_zb_nll, dim3((unsigned)zb_tiles(in.N, in.D)), dim3(ZB_THREADS), 0, st, in.d10, in.ldh, in.N, in.H, in.D, in.hd, in.X,
                       in.ldx, in.eps, ws_cell, ws_cell + cdiv64(in.D, 32) * in.N, (int)cdiv64(in.D, ZB_T));
    HIP_LAUNCH_CHECK("k_zb_nll");
    return zb_finish(ws, in.N, in.D, cell_sum, gene_sum, st);
}

int launch_zinb_terms(const float* x_rec, int64_t ld_rec, const float* x_p, int64_t ld_p, const float* x_r, int64_t ld_r, const float* X,
                      int64_t ldx, int64_t N, int D, double eps, void* ws, double* cell_sum, double* gene_sum, float* terms,
                      int64_t ld_t, hipStream_t st) {
    double* ws_cell = static_cast<double*>(ws);
    hipLaunchKernelGGL(k_zb_terms, dim3((unsigned)zb_tiles(N, D)), dim3(ZB_THREADS), 0, st, x_rec, ld_rec, x_p, ld_p, x_r, ld_r, X, ldx, N,
                       D, eps, ws_cell, ws_cell + cdiv64(D, 32) * N, terms, ld_t, (int)cdiv64(D, ZB_T));
    HIP_LAUNCH_CHECK("k_zb_terms");
    return zb_finish(ws, N, D, cell_sum, gene_sum, st);
}

}  // namespace mmvae

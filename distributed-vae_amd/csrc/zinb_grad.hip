// Gradients of the ZINB term with respect to the three decoder heads and to their input d10 (include/mmvae.h, DESIGN.md
// sections 9m, 9n, 9o).  Four entries:
//   mmvae_zinb_head_grads   dW_j [D, H], db_j [D] of fc11, fc11_p, fc11_r from d10 and X, and the per-cell / per-gene sums
//                           of the term itself, the bits of mmvae_zinb_nll; no N x D array is written;
//   mmvae_zinb_d10_grad     gd10 [N, H], the gradient with respect to d10 through the selected heads (k_zg_d10, below);
//   mmvae_zinb_terms_grad   the elementwise gradient with respect to heads the caller gives;
//   mmvae_zinb_step_grads   the first two from one evaluation of g (k_zg_heads<true>, "k_zg_step"): what the ZINB train step runs.
// The pieces that k_zg_heads and k_zg_d10 share are written once: the pre-activations are zb_run (zb_tile.hpp, which
// mmvae_zinb_nll runs too: the same operands in the same order, the same bits), the element is zg_element (one body in
// zinb_core.hpp, which the host runs too), and zg_load_tile and zg_gd10_pair are below.  The store of gd10's 2 x 16
// accumulators stays written out in both kernels: as a shared routine it cost k_zg_heads<true> 32 more bytes of scratch.
// k_zg_heads: a workgroup of four waves owns 64 genes and a segment of cell tiles (64 cells each) and walks them in order.
// Per cell tile:
//   1. the cells' d10 rows go to LDS whole ([64][PH], PH = H rounded up to even, plus 1: an odd pitch; zg_load_tile), the
//      three heads' weights in K chunks of 32 to the start of `work`; the pre-activations are zb_run on the resident rows
//      (wave w the 32 x 32 sub-tile (w & 1, w >> 1), the bias as C, k rising);
//   2. the accumulators go to LDS as k_zb_nll dumps them ([wave][head][register][lane]); zb_reduce runs the term over them
//      (its cell and gene partials land where k_zb_nll's do) and the same pass replaces each pre-activation, in place, by
//      g = d term / d pre-activation: fp64, rounded once to float32; an element past N or D gets an exact 0;
//   3. that image is the A operand of the second run: dW_j[gene, h] += sum_cell g_j[cell, gene] d10[cell, h], wave w the
//      32 columns h = 32 w .. of every head and both gene halves (2 x 3 accumulators of 32 x 32 that live across the
//      segment's cell tiles), the cells of the tile in rising order; B is the d10 tile of step 1, still in LDS.  db_j[gene]
//      is a thread's sum down the image's column, cells rising, in fp64: the addends of a gate's db all have one sign, and
//      a float32 chain over a few hundred of them would not hold section 9m's gate.
// A segment's dW is one float32 chain over its cells in rising order, its db the fp64 sum rounded once.  The segments'
// partials ([S][3][D][H + 1] float32, column H the bias) are added by k_zg_finish in segment order in fp64, scaled and
// rounded once.  No atomics: bit-identical from run to run, and a gene's row depends on that gene's column of X and its
// weights alone.
// LDS: 4 (64 PH + 12288) bytes, 75 KB at H = 100: two workgroups a CU, which the launch bounds hold the registers to (256,
// with 96 bytes of scratch a lane).  From H = 111 on the tile passes 80 KB and a CU holds one workgroup: there the register
// cap and its scratch buy nothing, and the segment rule below (sized for two workgroups on each of 256 CUs) makes two
// rounds of the grid.  Only H = 100 was timed; H = 128 is covered by the tests for its results, not for its speed.
#include "zb_tile.hpp"
#include "zinb_core.hpp"

namespace mmvae {

constexpr int ZG_WORK = 4 * 3 * 16 * 64;          // floats of the accumulator image; the weight chunks (3 x 64 x 33) alias it
static_assert(3 * ZB_T * ZB_P <= ZG_WORK, "the weight chunks must fit the accumulator image");

__host__ __device__ constexpr int zg_pitch(int H) { return ((H + 1) & ~1) + 1; }
static size_t zg_lds_bytes(int H) { return sizeof(float) * ((size_t)ZB_T * zg_pitch(H) + ZG_WORK); }

// the image's slot of g_j[cell c of the tile][gene gl of the tile], the inverse of zb_row: sub-tile (c >> 5, gl >> 5),
// register (rr & 3) + 4 (rr >> 3) of lane half (rr >> 2) & 1 with rr = c & 31
__device__ __forceinline__ int zg_slot(int j, int c, int gl) {
    const int rr = c & 31;
    return ((c >> 5) + 2 * (gl >> 5)) * (3 * 16 * 64) + (j * 16 + (rr & 3) + 4 * (rr >> 3)) * 64 + ((rr >> 2) & 1) * 32 + (gl & 31);
}

// One element: g = d term / d (a_rec, a_p, a_r), rounded once, and with TERM the term (k_zg_d10 has no use for it).  A real
// call: inlined into the kernels its fp64 temporaries compete with the accumulators (the 96 of dW in k_zg_heads) for the
// registers of two waves a SIMD.  The three g are written before the term is formed: behind it, the caller would wait for
// the stores (head_grads_ms 2.56 against 2.53).
template <bool TERM>
__device__ __attribute__((noinline)) double zg_element(float X, float a_rec, float a_p, float a_r, double eps, float& g0, float& g1, float& g2) {
    double g[3];
    const ZbOperands o = zinb_element_grad(X, a_rec, a_p, a_r, eps, g);
    g0 = (float)g[0];
    g1 = (float)g[1];
    g2 = (float)g[2];
    return TERM ? zinb_term(o) : 0.0;
}

// the d10 rows of 64 cells whole: [64][PH], cells past N and columns >= H zero
__device__ __forceinline__ void zg_load_tile(float* tile, int PH, const float* __restrict__ d10, int64_t ldh, int64_t cell0, int64_t N, int H) {
    for (int idx = threadIdx.x; idx < ZB_T * PH; idx += ZB_THREADS) {
        const int r = idx / PH, k = idx % PH;
        const int64_t cell = cell0 + r;
        tile[idx] = (cell < N && k < H) ? d10[cell * ldh + k] : 0.f;
    }
}

// One step of gd10[cell, h] += sum_gene g_j[cell, gene] W_j[gene, h] on v_mfma_f32_32x32x2_f32: the gene pair k, k + 1 of
// the tile (lane half kh the gene k + kh), the selected heads in the order rec, p, r, each one instruction for each of the
// wave's two cell halves.  g(j, ch, k) is the lane's A element, g_j[cell 32 ch + (lane & 31)][gene k + kh], read from the
// kernel's image; B the wave's column hcol of W_j from global memory (two rows of 128 bytes a load).
template <class G>
__device__ __forceinline__ void zg_gd10_pair(G&& g, const ZbHeads<3>& hd, int64_t gene0, int D, int H, int hcol, bool hok, int k, int kh,
                                             int mask, f32x16 (&gd)[2]) {
    const int64_t gk = gene0 + k + kh;
    const bool ok = hok && gk < D;
#pragma unroll
    for (int j = 0; j < 3; ++j)
        if (mask >> j & 1) {
            const float bv = ok ? hd.W[j][gk * H + hcol] : 0.f;
#pragma unroll
            for (int ch = 0; ch < 2; ++ch) gd[ch] = __builtin_amdgcn_mfma_f32_32x32x2f32(g(j, ch, k), bv, gd[ch], 0, 0, 0);
        }
}

// STEP (k_zg_step, mmvae_zinb_step_grads): the same walk also leaves the tile's share of gd10.  After step 3, with g's image
// still in LDS, wave w multiplies it the other way round (M = cell, K = gene) into the 32 columns h = 32 w .. of the 64 genes'
// rows of W_j, both cell halves: two accumulators of 32 x 32 that live for this tile only (the 48 of step 1 are dead by
// then: the kernel's peak stays at step 1's 96 + 48).  The chain of one gd10[cell, h] of the tile is k_zg_d10's
// (zg_gd10_pair, gene pairs rising).  The 64 x H partial goes to part_d [gene tile][cell][H], which k_zd_finish adds in
// rising order of the gene tiles: what mmvae_zinb_d10_grad computes with one segment a gene tile, bit for bit.  The image
// is read with the cell on the lane here, 16 lanes to a bank (it is laid out for step 3, gene on the lane): the reads hide
// behind the matrix instructions of the other waves, and the fp64 epilogue bounds the kernel either way
// (profiles/zinb_step_time.json).
template <bool STEP>
__global__ __launch_bounds__(ZB_THREADS, 2) void k_zg_heads(const float* __restrict__ d10, int64_t ldh, int64_t N, int H, int D, ZbHeads<3> hd,
                                                         const float* __restrict__ X, int64_t ldx, double eps, int mask,
                                                         double* __restrict__ ws_cell, double* __restrict__ ws_gene,
                                                         float* __restrict__ part, int tiles_n, int tiles_per_seg,
                                                         float* __restrict__ part_d) {
    extern __shared__ __attribute__((aligned(16))) float zg_lds[];
    const int PH = zg_pitch(H);
    float* tile = zg_lds;                              // [64][PH] the cell tile's d10, columns >= H zero
    float* work = zg_lds + ZB_T * PH;                  // the weight chunks, then the accumulator image
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wm = w & 1, wn = w >> 1, i = lane & 31, kh = lane >> 5;
    const int seg = blockIdx.x / tiles_n;
    const int64_t gene0 = (int64_t)(blockIdx.x % tiles_n) * ZB_T;
    const int64_t n_ct = cdiv64(N, ZB_T);
    const int64_t ct0 = (int64_t)seg * tiles_per_seg, ct1 = imin64(ct0 + tiles_per_seg, n_ct);
    const int nhb = (H + 31) >> 5;                     // the 32-column blocks of H; wave w owns block w
    const int64_t gene = gene0 + wn * 32 + i;
    float bias[3];                                     // read once a workgroup
    zb_bias<3>(hd, gene, D, bias);

    f32x16 dw[3][2];
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int gh = 0; gh < 2; ++gh)
#pragma unroll
            for (int g = 0; g < 16; ++g) dw[j][gh][g] = 0.f;
    double db = 0.0;                                   // thread t < 192: head t >> 6, gene t & 63 of the tile

    for (int64_t ct = ct0; ct < ct1; ++ct) {
        const int64_t cell0 = ct * ZB_T;
        // 1. the d10 tile whole, then the pre-activations chunk after chunk
        zg_load_tile(tile, PH, d10, ldh, cell0, N, H);
        f32x16 acc[3];
        zb_run<3>(tile + (wm * 32 + i) * PH + kh, 1, [](int) {}, work, hd, gene0, D, H, wn, lane, bias, acc);
        // 2. the accumulator image, the term's sums, g in place
        float* mine = work + w * (3 * 16 * 64) + lane;
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int g = 0; g < 16; ++g) mine[(j * 16 + g) * 64] = acc[j][g];
        const int64_t wc0 = cell0 + wm * 32, wg0 = gene0 + wn * 32;
        if (wc0 < N && wg0 < D)
            zb_reduce(
                [&](int g, int64_t cell, int64_t gn) {
                    const float a_rec = mine[g * 64], a_p = mine[(16 + g) * 64], a_r = mine[(32 + g) * 64];
                    float g0, g1, g2;
                    const double t = zg_element<true>(X[cell * ldx + gn], a_rec, a_p, a_r, eps, g0, g1, g2);
                    mine[g * 64] = g0;
                    mine[(16 + g) * 64] = g1;
                    mine[(32 + g) * 64] = g2;
                    return t;
                },
                lane, wc0, wg0, N, D, ws_cell, ws_gene);
        for (int g = 0; g < 16; ++g)
            if (wc0 + zb_row(g, kh) >= N || gene >= D) mine[g * 64] = mine[(16 + g) * 64] = mine[(32 + g) * 64] = 0.f;
        __syncthreads();
        // 3. dW += g^T d10 over the tile's cells; db down the image's columns
        const int kmax = (int)imin64(ZB_T, (N - cell0 + 1) & ~(int64_t)1);
        if (w < nhb) {
            const int col = w * 32 + i < PH - 1 ? w * 32 + i : PH - 1;       // columns past H read the zero column
            for (int k = 0; k < kmax; k += 2) {
                const int c = k + kh;
                const float bv = tile[c * PH + col];
#pragma unroll
                for (int j = 0; j < 3; ++j)
                    if (mask >> j & 1) {
#pragma unroll
                        for (int gh = 0; gh < 2; ++gh)
                            dw[j][gh] = __builtin_amdgcn_mfma_f32_32x32x2f32(work[zg_slot(j, c, gh * 32 + i)], bv, dw[j][gh], 0, 0, 0);
                    }
            }
        }
        if (threadIdx.x < 192 && (mask >> (threadIdx.x >> 6) & 1))
            for (int c = 0; c < kmax; ++c) db += (double)work[zg_slot(threadIdx.x >> 6, c, threadIdx.x & 63)];
        if constexpr (STEP) {
            // 3b. the tile's gd10 = g W over its genes
            const int hcol = w * 32 + i;
            const bool hok = hcol < H;
            if (w < nhb) {
                f32x16 gd[2];
#pragma unroll
                for (int ch = 0; ch < 2; ++ch)
#pragma unroll
                    for (int g = 0; g < 16; ++g) gd[ch][g] = 0.f;
                const int gmax = (int)imin64(ZB_T, (D - gene0 + 1) & ~(int64_t)1);
                for (int k = 0; k < gmax; k += 2)
                    zg_gd10_pair([&](int j, int ch, int kk) { return work[zg_slot(j, ch * 32 + i, kk + kh)]; }, hd, gene0, D, H, hcol, hok, k,
                                 kh, mask, gd);
                if (hok) {
                    float* pd = part_d + (gene0 / ZB_T) * N * H;
#pragma unroll
                    for (int ch = 0; ch < 2; ++ch)
#pragma unroll
                        for (int g = 0; g < 16; ++g) {
                            const int64_t cell = cell0 + ch * 32 + zb_row(g, kh);
                            if (cell < N) pd[cell * H + hcol] = gd[ch][g];
                        }
                }
            }
        }
        __syncthreads();                               // the image and the tile are free again
    }

    // the segment's partials: [seg][head][gene][H + 1]
    const int64_t row = (int64_t)H + 1;
    if (w < nhb) {
        const int h = w * 32 + i;
#pragma unroll
        for (int j = 0; j < 3; ++j)
            if (mask >> j & 1) {
#pragma unroll
                for (int gh = 0; gh < 2; ++gh)
#pragma unroll
                    for (int g = 0; g < 16; ++g) {
                        const int64_t gn = gene0 + gh * 32 + zb_row(g, kh);
                        if (gn < D && h < H) part[(((int64_t)seg * 3 + j) * D + gn) * row + h] = dw[j][gh][g];
                    }
            }
    }
    if (threadIdx.x < 192 && (mask >> (threadIdx.x >> 6) & 1)) {
        const int64_t gn = gene0 + (threadIdx.x & 63);
        if (gn < D) part[(((int64_t)seg * 3 + (threadIdx.x >> 6)) * D + gn) * row + H] = (float)db;
    }
}

struct ZgOut {
    float* dW[3];
    float* db[3];
};

// dW_j, db_j = scale x the segments' partials added in segment order from 0.0 in fp64, rounded once
__global__ __launch_bounds__(256) void k_zg_finish(const float* __restrict__ part, int nseg, int D, int H, int mask, double scale, ZgOut out) {
    const int64_t row = (int64_t)H + 1, per_head = (int64_t)D * row;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < 3 * per_head; idx += (int64_t)gridDim.x * 256) {
        const int j = (int)(idx / per_head);
        if (!(mask >> j & 1)) continue;
        const int64_t e = idx % per_head, gn = e / row, h = e % row;
        double s = 0.0;
        for (int sg = 0; sg < nseg; ++sg) s += (double)part[(int64_t)sg * 3 * per_head + idx];
        const float v = (float)(scale * s);
        if (h < H) out.dW[j][gn * H + h] = v;
        else out.db[j][gn] = v;
    }
}

// ---- the gradient with respect to d10: gd10[i, h] = scale sum_j sum_d g_j[i, d] W_j[d, h] ----
// k_zg_d10 is k_zg_heads turned round: a workgroup owns 64 cells and a segment of the gene tiles and walks them in rising
// order.  The cells' d10 tile ([64][PH]) is loaded once and stays in LDS.  Per gene tile:
//   1. the pre-activations as k_zg_heads forms them (step 1 above, the bias read once a gene tile);
//   2. the element pass straight from the accumulator registers (no sums of the term are wanted here, so nothing goes
//      through zb_reduce and there is no accumulator image): g in fp64, rounded once, an exact 0 past N or D, written
//      cell-major, [head][cell][ZD_PG] with the odd pitch 65: the write has the gene on the lane, the read of step 3 the cell,
//      and both are free of bank conflicts (bank = cell + gene mod 64);
//   3. gd10[cell, h] += sum_gene g_j[cell, gene] W_j[gene, h] (zg_gd10_pair): A the image (M = cell, K = gene), B the wave's
//      32 columns h = 32 w .. of W_j read from global memory (the three heads' weights are 6 MB at D = 5032 and stay in
//      L2), wave w both cell halves: two accumulators of 32 x 32 that live across the segment's gene tiles.
// The chain of one gd10[cell, h] of a segment, in float32: gene tiles rising; within a tile the gene pairs k = 0, 2, ..
// rising; within a pair the selected heads in the order rec, p, r, each one instruction (its two genes as the instruction
// adds them).  The segments' partials ([S][N][H] float32) are added by k_zd_finish in segment order in fp64, scaled and
// rounded once.  No atomics; with D and the segments fixed a cell's row depends on that cell's rows of d10 and X and on the
// weights alone.
// LDS: 4 (64 PH + 3 x 64 x 65) bytes: 75.8 KB at H = 100 (two workgroups a CU, up to H = 124), 82.9 KB at H = 128 (one).
constexpr int ZD_PG = ZB_T + 1;                   // the pitch of g's cell-major image, odd
constexpr int ZD_WORK = 3 * ZB_T * ZD_PG;         // floats of that image; the weight chunks (3 x 64 x 33) alias it
static_assert(3 * ZB_T * ZB_P <= ZD_WORK, "the weight chunks must fit g's image");
static size_t zd_lds_bytes(int H) { return sizeof(float) * ((size_t)ZB_T * zg_pitch(H) + ZD_WORK); }

__global__ __launch_bounds__(ZB_THREADS, 2) void k_zg_d10(const float* __restrict__ d10, int64_t ldh, int64_t N, int H, int D, ZbHeads<3> hd,
                                                       const float* __restrict__ X, int64_t ldx, double eps, int mask,
                                                       float* __restrict__ part, int tiles_c, int tiles_per_seg) {
    extern __shared__ __attribute__((aligned(16))) float zd_lds[];
    const int PH = zg_pitch(H);
    float* tile = zd_lds;                              // [64][PH] the cells' d10, columns >= H zero
    float* work = zd_lds + ZB_T * PH;                  // the weight chunks, then g's image
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wm = w & 1, wn = w >> 1, i = lane & 31, kh = lane >> 5;
    const int seg = blockIdx.x / tiles_c;
    const int64_t cell0 = (int64_t)(blockIdx.x % tiles_c) * ZB_T;
    const int64_t n_gt = cdiv64(D, ZB_T);
    const int64_t gt0 = (int64_t)seg * tiles_per_seg, gt1 = imin64(gt0 + tiles_per_seg, n_gt);
    const int nhb = (H + 31) >> 5;                     // the 32-column blocks of H; wave w owns block w
    const int hcol = w * 32 + i;
    const bool hok = hcol < H;

    zg_load_tile(tile, PH, d10, ldh, cell0, N, H);
    f32x16 gd[2];
#pragma unroll
    for (int ch = 0; ch < 2; ++ch)
#pragma unroll
        for (int g = 0; g < 16; ++g) gd[ch][g] = 0.f;

    for (int64_t gt = gt0; gt < gt1; ++gt) {
        const int64_t gene0 = gt * ZB_T;
        const int64_t gene = gene0 + wn * 32 + i;
        // 1. the pre-activations, chunk after chunk (the first barrier also covers the d10 tile)
        float bias[3];
        zb_bias<3>(hd, gene, D, bias);
        f32x16 acc[3];
        zb_run<3>(tile + (wm * 32 + i) * PH + kh, 1, [](int) {}, work, hd, gene0, D, H, wn, lane, bias, acc);
        // 2. g from the registers to the cell-major image
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            const int cl = wm * 32 + zb_row(g, kh);
            const int64_t cell = cell0 + cl;
            float g0 = 0.f, g1 = 0.f, g2 = 0.f;
            if (cell < N && gene < D) zg_element<false>(X[cell * ldx + gene], acc[0][g], acc[1][g], acc[2][g], eps, g0, g1, g2);
            float* dst = work + cl * ZD_PG + wn * 32 + i;
            dst[0] = g0;
            dst[ZB_T * ZD_PG] = g1;
            dst[2 * ZB_T * ZD_PG] = g2;
        }
        __syncthreads();
        // 3. gd10 += g W over the tile's genes
        const int kmax = (int)imin64(ZB_T, (D - gene0 + 1) & ~(int64_t)1);
        if (w < nhb) {
            const float* ga = work + i * ZD_PG + kh;
#pragma unroll 4
            for (int k = 0; k < kmax; k += 2)
                zg_gd10_pair([&](int j, int ch, int kk) { return ga[(j * ZB_T + ch * 32) * ZD_PG + kk]; }, hd, gene0, D, H, hcol, hok, k, kh, mask,
                             gd);
        }
        __syncthreads();                               // the image is free again
    }

    // the segment's partials: [seg][cell][H]
    if (w < nhb && hok) {
#pragma unroll
        for (int ch = 0; ch < 2; ++ch)
#pragma unroll
            for (int g = 0; g < 16; ++g) {
                const int64_t cell = cell0 + ch * 32 + zb_row(g, kh);
                if (cell < N) part[((int64_t)seg * N + cell) * H + hcol] = gd[ch][g];
            }
    }
}

// gd10 = scale x the segments' partials added in segment order from 0.0 in fp64, rounded once
__global__ __launch_bounds__(256) void k_zd_finish(const float* __restrict__ part, int nseg, int64_t N, int H, double scale,
                                                   float* __restrict__ gd10, int64_t ldg) {
    const int64_t total = N * H;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        double s = 0.0;
        for (int sg = 0; sg < nseg; ++sg) s += (double)part[(int64_t)sg * total + idx];
        gd10[(idx / H) * ldg + idx % H] = (float)(scale * s);
    }
}

// The elementwise gradient with respect to given heads: r = x_rec + eps (no relu: the subgradient is the reference's, which
// takes rec_x as given), d p / d x_p = d z / d x_r = 1 - eps.  The loads and the tile of k_zb_terms.
__global__ __launch_bounds__(ZB_THREADS) void k_zg_terms(const float* __restrict__ x_rec, int64_t ld_rec, const float* __restrict__ x_p,
                                                         int64_t ld_p, const float* __restrict__ x_r, int64_t ld_r,
                                                         const float* __restrict__ X, int64_t ldx, int64_t N, int D, double eps,
                                                         double scale, float* __restrict__ g_rec, float* __restrict__ g_p,
                                                         float* __restrict__ g_r, int64_t ld_g, int tiles_n) {
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t wc0 = (int64_t)(blockIdx.x / tiles_n) * ZB_T + (w & 1) * 32, wg0 = (int64_t)(blockIdx.x % tiles_n) * ZB_T + (w >> 1) * 32;
    const int64_t gene = wg0 + (lane & 31);
    if (wc0 >= N || gene >= D) return;
#pragma unroll 1
    for (int g = 0; g < 16; ++g) {
        const int64_t cell = wc0 + zb_row(g, lane >> 5);
        if (cell >= N) continue;
        const double p = (1.0 - eps) * ((double)x_p[cell * ld_p + gene] + eps);
        const double z = (1.0 - eps) * ((double)x_r[cell * ld_r + gene] + eps);
        double gr, gp, gz;
        zinb_term_grad((double)X[cell * ldx + gene], (double)x_rec[cell * ld_rec + gene] + eps, p, 1.0 - p, z, 1.0 - z, gr, gp, gz);
        g_rec[cell * ld_g + gene] = (float)(scale * gr);
        g_p[cell * ld_g + gene] = (float)(scale * ((1.0 - eps) * gp));
        g_r[cell * ld_g + gene] = (float)(scale * ((1.0 - eps) * gz));
    }
}

// The segments of a call.  A workgroup owns one tile of one extent (own_tiles of them: the gene tiles of k_zg_heads, the cell
// tiles of k_zg_d10) and walks a segment of the other's (walked_tiles).  asked = 0 is the launcher's rule, as many segments as
// keep the grid within 512 workgroups (two for each of the MI355X's 256 CUs: one round at H <= 110, see above; the count is
// a constant, not read from the device, so that the results do not depend on where a call runs); at most one segment a
// walked tile.  A segment is tiles_per_seg whole tiles, the last may be shorter; the count is what that leaves.
static int64_t zg_split(int64_t own_tiles, int64_t walked_tiles, int asked, int64_t* tiles_per_seg) {
    int64_t s = asked > 0 ? asked : (512 / own_tiles > 1 ? 512 / own_tiles : 1);
    s = imin64(s, walked_tiles);
    *tiles_per_seg = cdiv64(walked_tiles, s);
    return cdiv64(walked_tiles, *tiles_per_seg);
}

// the workgroups of one grid, 0 where a grid cannot hold them
static int64_t zg_grid(int64_t segments, int64_t own_tiles) {
    const unsigned __int128 t = (unsigned __int128)segments * (unsigned __int128)own_tiles;
    return t > (unsigned __int128)INT32_MAX ? 0 : (int64_t)t;
}

// mmvae_zinb_head_grads: segments of the cell tiles (a segment's tiles clamped to what an int holds)
int zg_segments(int64_t N, int D, int asked, int* tiles_per_seg) {
    int64_t tps;
    const int s = (int)zg_split(cdiv64(D, ZB_T), cdiv64(N, ZB_T), asked, &tps);
    if (tiles_per_seg) *tiles_per_seg = (int)imin64(tps, INT32_MAX);
    return s;
}

// mmvae_zinb_d10_grad: segments of the gene tiles
int zd_segments(int64_t N, int D, int asked, int* tiles_per_seg) {
    int64_t tps;
    const int s = (int)zg_split(cdiv64(N, ZB_T), cdiv64(D, ZB_T), asked, &tps);
    if (tiles_per_seg) *tiles_per_seg = (int)tps;
    return s;
}

int64_t zg_tiles(int64_t N, int D, int asked) { return zg_grid(zg_segments(N, D, asked, nullptr), cdiv64(D, ZB_T)); }
int64_t zd_tiles(int64_t N, int D, int asked) { return zg_grid(zd_segments(N, D, asked, nullptr), cdiv64(N, ZB_T)); }

// zb_ws_bytes(N, D), then the segments' partials, [S][3][D][H + 1] float32 (whole 8 bytes)
size_t zg_ws_bytes(int64_t N, int D, int H, int asked) {
    const unsigned __int128 floats = (unsigned __int128)zg_segments(N, D, asked, nullptr) * 3 * (unsigned __int128)D * (unsigned __int128)(H + 1);
    const size_t sums = zb_ws_bytes(N, D);
    const size_t part = bytes_or_0(8 * ((floats + 1) / 2));
    return sums && part && sums + part > sums ? sums + part : 0;
}

// the segments' partials, [S][N][H] float32 (whole 8 bytes)
size_t zd_ws_bytes(int64_t N, int D, int H, int asked) {
    return bytes_or_0(8 * (((unsigned __int128)zd_segments(N, D, asked, nullptr) * (unsigned __int128)N * (unsigned __int128)H + 1) / 2));
}

// mmvae_zinb_step_grads: zg_ws_bytes(N, D, H, asked), then the gene tiles' partials of gd10, [ceil(D / 64)][N][H] float32
// (zd_ws_bytes with a segment a gene tile)
size_t zs_ws_bytes(int64_t N, int D, int H, int asked) {
    const size_t heads = zg_ws_bytes(N, D, H, asked);
    const size_t d10 = zd_ws_bytes(N, D, H, (int)imin64(cdiv64(D, ZB_T), INT32_MAX));
    return heads && d10 && heads + d10 > heads ? heads + d10 : 0;
}

static int zd_finish(const float* part, int nseg, const ZinbIn& in, float* gd10, int64_t ldg, hipStream_t st) {
    const unsigned gx = (unsigned)imin64(cdiv64(in.N * in.H, 256), 1 << 20);
    hipLaunchKernelGGL(k_zd_finish, dim3(gx), dim3(256), 0, st, part, nseg, in.N, in.H, in.scale, gd10, ldg);
    HIP_LAUNCH_CHECK("k_zd_finish");
    return 0;
}

int launch_zinb_head_grads(const ZinbIn& in, void* ws, const ZinbGradOut& out, hipStream_t st) {
    const int64_t N = in.N;
    const int D = in.D, H = in.H;
    const bool step = out.gd10 != nullptr;
    int tps = 1;
    const int nseg = zg_segments(N, D, in.segments, &tps);
    const int tiles_n = (int)cdiv64(D, ZB_T);
    double* ws_cell = static_cast<double*>(ws);
    float* part = reinterpret_cast<float*>(static_cast<char*>(ws) + zb_ws_bytes(N, D));
    float* part_d = step ? reinterpret_cast<float*>(static_cast<char*>(ws) + zg_ws_bytes(N, D, H, in.segments)) : nullptr;
    const auto kernel = step ? k_zg_heads<true> : k_zg_heads<false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)zg_tiles(N, D, in.segments)), dim3(ZB_THREADS), zg_lds_bytes(H), st, in.d10, in.ldh, N, H, D,
                       in.hd, in.X, in.ldx, in.eps, in.mask, ws_cell, ws_cell + cdiv64(D, 32) * N, part, tiles_n, tps, part_d);
    HIP_LAUNCH_CHECK(step ? "k_zg_step" : "k_zg_heads");
    const ZgOut o{{out.dW[0], out.dW[1], out.dW[2]}, {out.db[0], out.db[1], out.db[2]}};
    const unsigned gx = (unsigned)imin64(cdiv64((int64_t)3 * D * (H + 1), 256), 1 << 20);
    hipLaunchKernelGGL(k_zg_finish, dim3(gx), dim3(256), 0, st, part, nseg, D, H, in.mask, in.scale, o);
    HIP_LAUNCH_CHECK("k_zg_finish");
    if (step)
        if (int rc = zd_finish(part_d, tiles_n, in, out.gd10, out.ldg, st)) return rc;
    return zb_finish(ws, N, D, out.cell_sum, out.gene_sum, st);
}

int launch_zinb_d10_grad(const ZinbIn& in, void* ws, float* gd10, int64_t ldg, hipStream_t st) {
    int tps = 1;
    const int nseg = zd_segments(in.N, in.D, in.segments, &tps);
    float* part = static_cast<float*>(ws);
    hipLaunchKernelGGL(k_zg_d10, dim3((unsigned)zd_tiles(in.N, in.D, in.segments)), dim3(ZB_THREADS), zd_lds_bytes(in.H), st, in.d10, in.ldh,
                       in.N, in.H, in.D, in.hd, in.X, in.ldx, in.eps, in.mask, part, (int)cdiv64(in.N, ZB_T), tps);
    HIP_LAUNCH_CHECK("k_zg_d10");
    return zd_finish(part, nseg, in, gd10, ldg, st);
}

int launch_zinb_terms_grad(const float* x_rec, int64_t ld_rec, const float* x_p, int64_t ld_p, const float* x_r, int64_t ld_r,
                           const float* X, int64_t ldx, int64_t N, int D, double eps, double scale, float* g_rec, float* g_p, float* g_r,
                           int64_t ld_g, hipStream_t st) {
    hipLaunchKernelGGL(k_zg_terms, dim3((unsigned)zb_tiles(N, D)), dim3(ZB_THREADS), 0, st, x_rec, ld_rec, x_p, ld_p, x_r, ld_r, X, ldx, N, D,
                       eps, scale, g_rec, g_p, g_r, ld_g, (int)cdiv64(D, ZB_T));
    HIP_LAUNCH_CHECK("k_zg_terms");
    return 0;
}

// zinb_loss of every arm from the per-cell sums (mmvae_zinb_train_step, mmvae_zinb_objective): one workgroup an arm; thread
// t adds cells t, t + 256, .. in rising order, the 256 sums fold in halves (128, 64, ..): one fixed order in fp64, then one
// division by N D.  The loss finalisation rounds it to float32.
__global__ __launch_bounds__(256) void k_zinb_rec(const double* __restrict__ cell_sum, int64_t N, int D, double* __restrict__ zrec) {
    __shared__ double sh[256];
    const double* cs = cell_sum + (int64_t)blockIdx.x * N;
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < N; i += 256) s += cs[i];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) zrec[blockIdx.x] = sh[0] / ((double)N * (double)D);
}

int launch_zinb_rec(const double* cell_sum, int A, int64_t N, int D, double* zrec, hipStream_t st) {
    hipLaunchKernelGGL(k_zinb_rec, dim3((unsigned)A), dim3(256), 0, st, cell_sum, N, D, zrec);
    HIP_LAUNCH_CHECK("k_zinb_rec");
    return 0;
}

// The element code on the host: g [3][n] = d term / d (a_rec, a_p, a_r) as the kernels form it before the rounding, term [n]
void host_zinb_grad(int64_t n, const float* X, const float* a_rec, const float* a_p, const float* a_r, double eps, double* g, double* term) {
    for (int64_t e = 0; e < n; ++e) {
        double ge[3];
        const ZbOperands o = zinb_element_grad(X[e], a_rec[e], a_p[e], a_r[e], eps, ge);
        for (int j = 0; j < 3; ++j) g[j * n + e] = ge[j];
        if (term) term[e] = zinb_term(o);
    }
}

void host_digamma(int64_t n, const double* x, double* out) {
    for (int64_t e = 0; e < n; ++e) out[e] = zb_digamma(x[e]);
}

}  // namespace mmvae

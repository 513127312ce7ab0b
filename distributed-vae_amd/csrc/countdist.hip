// Count distributions on the device (mmidas/utils/distributions.py; include/mmvae.h): the scVI
// likelihoods log_nb_positive, log_zinb_positive, log_mixture_nb (mmvae_count_logp), one draw per element of NB / ZINB
// (mmvae_count_sample) and the draws of a checkpoint's three heads fused behind their products (mmvae_zinb_sample).
// The arithmetic of one element is countdist_core.hpp, shared with the host-only debug entries below.
//   k_cd_logp    the tile of zb_tile.hpp: a workgroup owns 64 x 64 elements, a wave a 32 x 32 sub-tile, and the sums are
//                zb_reduce's partials added by zb_finish -- the scheme of mmvae_zinb_terms, no atomics.
//   k_cd_sample  one thread an element.  A draw is a function of (seed, offset, logical index, parameters) alone, so the
//                launch geometry is free; rows are walked by a 2-D grid-stride loop.
//   k_cd_zinb_sample  zb_products for the three heads of a tile, rounded to float32 as mmvae_zinb_heads and the decode round
//                them, then cd_heads_to_params and cd_draw in the epilogue.
// The one atomic is the exhaustion counter, an integer that only a draw whose 64 attempts all failed touches.
#include "countdist_core.hpp"
#include "zb_tile.hpp"

namespace mmvae {

// theta of a [D] vector is read with a row pitch of 0
__host__ __device__ __forceinline__ double cd_logp_at(const mmvae_count_logp_t& a, int64_t cell, int64_t gene) {
    const double x = (double)a.x[cell * a.ldx + gene], mu = (double)a.mu[cell * a.ld_mu + gene];
    const double th = (double)a.theta[cell * a.ld_theta + gene];
    if (a.kind == CD_NB) return cd_log_nb(x, mu, th, a.eps);
    const double pi = (double)a.pi[cell * a.ld_pi + gene];
    if (a.kind == CD_ZINB) return cd_log_zinb(x, mu, th, pi, a.eps);
    const double th2 = a.theta2 ? (double)a.theta2[cell * a.ld_theta2 + gene] : th;
    return cd_log_mix(x, mu, (double)a.mu2[cell * a.ld_mu2 + gene], th, th2, pi, a.eps);
}

template <bool SUMS>
__global__ __launch_bounds__(ZB_THREADS) void k_cd_logp(mmvae_count_logp_t a, double* __restrict__ ws_cell, double* __restrict__ ws_gene,
                                                        int tiles_n) {
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t wc0 = (int64_t)(blockIdx.x / tiles_n) * ZB_T + (w & 1) * 32, wg0 = (int64_t)(blockIdx.x % tiles_n) * ZB_T + (w >> 1) * 32;
    if (wc0 >= a.N || wg0 >= a.D) return;
    auto term = [&](int, int64_t cell, int64_t gene) {
        const double t = cd_logp_at(a, cell, gene);
        if (a.terms) a.terms[cell * a.ld_t + gene] = (float)t;
        return t;
    };
    if constexpr (SUMS) {
        zb_reduce(term, lane, wc0, wg0, a.N, a.D, ws_cell, ws_gene);
        return;
    }
    const int64_t gene = wg0 + (lane & 31);
    if (gene >= a.D) return;
#pragma unroll 1
    for (int g = 0; g < 16; ++g) {
        const int64_t cell = wc0 + zb_row(g, lane >> 5);
        if (cell < a.N) term(g, cell, gene);
    }
}

// one element of mmvae_count_sample; returns 1 where a bounded loop ran out
__host__ __device__ inline int cd_sample_at(const mmvae_count_sample_t& s, int64_t row, int64_t gene) {
    int exhausted = 0;
    double mu, th, zi = 0.0;
    int zk = s.zi_kind;
    if (s.param == 1) {
        cd_heads_to_params(s.a[row * s.ld_a + gene], s.b[row * s.ld_b + gene], s.zi[row * s.ld_zi + gene], s.eps, mu, th, zi);
        zk = CD_ZI_PROB;
    } else {
        mu = (double)s.a[row * s.ld_a + gene];
        th = (double)s.b[row * s.ld_b + gene];
        if (zk != CD_ZI_NONE) zi = (double)s.zi[row * s.ld_zi + gene];
    }
    const uint64_t idx = (uint64_t)(s.cell0 + row) * (uint64_t)s.D + (uint64_t)gene;
    cd_store(s.out, row * s.ld_out + gene, cd_draw(mu, th, zi, zk, idx, s.seed, s.offset, exhausted), s.out_int32, s.log1p);
    return exhausted;
}

constexpr int CD_S_THREADS = 256;
__global__ __launch_bounds__(CD_S_THREADS) void k_cd_sample(mmvae_count_sample_t s) {
    int exhausted = 0;
    for (int64_t row = blockIdx.y; row < s.N; row += gridDim.y)
        for (int64_t gene = (int64_t)blockIdx.x * CD_S_THREADS + threadIdx.x; gene < s.D; gene += (int64_t)gridDim.x * CD_S_THREADS)
            exhausted += cd_sample_at(s, row, gene);
    if (exhausted) atomicAdd(s.exhausted, exhausted);
}

__global__ __launch_bounds__(ZB_THREADS) void k_cd_zinb_sample(const float* __restrict__ d10, int64_t ldh, int64_t N, int H, int D,
                                                               ZbHeads<3> hd, mmvae_count_sample_t s, int tiles_n) {
    __shared__ float zb_lds[zb_lds_bytes<3>(true) / sizeof(float)];
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wm = w & 1, wn = w >> 1;
    const int64_t cell0 = (int64_t)(blockIdx.x / tiles_n) * ZB_T, gene0 = (int64_t)(blockIdx.x % tiles_n) * ZB_T;
    f32x16 acc[3];
    zb_products<3>(zb_lds, d10, ldh, cell0, N, hd, gene0, D, H, wm, wn, lane, acc);
    // LDS now holds the accumulators, [head][register][lane] per wave, so that the draw loop can stay rolled (k_zb_nll's reason)
    float* mine = zb_lds + w * (3 * 16 * 64) + lane;
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int g = 0; g < 16; ++g) mine[(j * 16 + g) * 64] = acc[j][g];
    const int64_t gene = gene0 + wn * 32 + (lane & 31);
    if (gene >= D) return;                             // (no barrier follows)
    int exhausted = 0;
#pragma unroll 1
    for (int g = 0; g < 16; ++g) {
        const int64_t cell = cell0 + wm * 32 + zb_row(g, lane >> 5);
        if (cell >= N) continue;
        // the heads as float32, rounded as the decode (relu) and mmvae_zinb_heads (the fp64 sigmoid, rounded once) write them
        const float x_rec = fmaxf(mine[g * 64], 0.f);
        const float x_p = (float)(1.0 / (1.0 + exp(-(double)mine[(16 + g) * 64])));
        const float x_r = (float)(1.0 / (1.0 + exp(-(double)mine[(32 + g) * 64])));
        double mu, th, z;
        cd_heads_to_params(x_rec, x_p, x_r, s.eps, mu, th, z);
        const uint64_t idx = (uint64_t)(s.cell0 + cell) * (uint64_t)D + (uint64_t)gene;
        int ex = 0;
        cd_store(s.out, cell * s.ld_out + gene, cd_draw(mu, th, z, CD_ZI_PROB, idx, s.seed, s.offset, ex), s.out_int32, s.log1p);
        exhausted += ex;
    }
    if (exhausted) atomicAdd(s.exhausted, exhausted);
}

int launch_count_logp(const mmvae_count_logp_t& a, void* ws, hipStream_t st) {
    double* ws_cell = a.cell_sum ? static_cast<double*>(ws) : nullptr;
    hipLaunchKernelGGL(a.cell_sum ? k_cd_logp<true> : k_cd_logp<false>, dim3((unsigned)zb_tiles(a.N, a.D)), dim3(ZB_THREADS), 0, st, a,
                       ws_cell, ws_cell ? ws_cell + cdiv64(a.D, 32) * a.N : nullptr, (int)cdiv64(a.D, ZB_T));
    HIP_LAUNCH_CHECK("k_cd_logp");
    return a.cell_sum ? zb_finish(ws, a.N, a.D, a.cell_sum, a.gene_sum, st) : 0;
}

static int cd_zero_counter(int* exhausted, hipStream_t st) {
    const hipError_t e = hipMemsetAsync(exhausted, 0, sizeof(int), st);
    if (e != hipSuccess) { set_error("count_sample: memset: %s", hipGetErrorString(e)); return MMVAE_E_LAUNCH; }
    return 0;
}

int launch_count_sample(const mmvae_count_sample_t& s, hipStream_t st) {
    if (int rc = cd_zero_counter(s.exhausted, st)) return rc;
    const dim3 grid((unsigned)imin64(cdiv64(s.D, CD_S_THREADS), 1 << 16), (unsigned)imin64(s.N, 65535));
    hipLaunchKernelGGL(k_cd_sample, grid, dim3(CD_S_THREADS), 0, st, s);
    HIP_LAUNCH_CHECK("k_cd_sample");
    return 0;
}

int launch_zinb_sample(const float* d10, int64_t ldh, int H, const float* W, const float* b, const float* Wp, const float* bp,
                       const float* Wr, const float* br, const mmvae_count_sample_t& s, hipStream_t st) {
    if (int rc = cd_zero_counter(s.exhausted, st)) return rc;
    ZbHeads<3> hd{{W, Wp, Wr}, {b, bp, br}};
    hipLaunchKernelGGL(k_cd_zinb_sample, dim3((unsigned)zb_tiles(s.N, s.D)), dim3(ZB_THREADS), 0, st, d10, ldh, s.N, H, s.D, hd, s,
                       (int)cdiv64(s.D, ZB_T));
    HIP_LAUNCH_CHECK("k_cd_zinb_sample");
    return 0;
}

// the same elements on the host, one after the other: no GPU call
void host_count_logp(const mmvae_count_logp_t& a) {
    for (int64_t cell = 0; cell < a.N; ++cell)
        for (int64_t gene = 0; gene < a.D; ++gene) a.terms[cell * a.ld_t + gene] = (float)cd_logp_at(a, cell, gene);
}

void host_count_sample(const mmvae_count_sample_t& s) {
    *s.exhausted = 0;
    for (int64_t row = 0; row < s.N; ++row)
        for (int64_t gene = 0; gene < s.D; ++gene) *s.exhausted += cd_sample_at(s, row, gene);
}

}  // namespace mmvae

// mmvae_prune_apply: exact zeros at the parameter positions of the pruned categories (the five masks of the reference's
// pruning phase, mmidas/cpl_mixvae.py:1124-1128, applied at :1153-1161), in up to four flat buffers of the parameter layout
// at once.  A translation unit of its own: rowwise.hip and every other unit compile exactly as they did without it.
#include "common.hpp"

namespace mmvae {

// Per arm and pruned category k: fcc.weight[k, :] (L), fcc.bias[k] (1), fc_mu.weight[:, L + k] (S),
// fc_sigma.weight[:, L + k] (S), fc6.weight[:, k] (L rows) -- y = [x_low | c_smp] and the decoder input is [c_smp | s].
struct PruneArgs {
    float* buf[4];
    int64_t per_arm, o_fccw, o_fccb, o_mu, o_sig, o_fc6;
    int32_t A, L, C, S, n_cat;
    uint8_t cat[128];   // the pruned categories, ascending (C <= 128 by mmvae_check_dims)
};

__global__ void __launch_bounds__(256) k_prune_apply(const PruneArgs p) {
    const int per_cat = 2 * p.L + 1 + 2 * p.S;
    const int per_arm_el = p.n_cat * per_cat;
    const int total = p.A * per_arm_el;
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
        const int a = e / per_arm_el, r = e - a * per_arm_el;
        const int j = r / per_cat, i = r - j * per_cat;
        const int64_t k = p.cat[j];
        int64_t off;
        if (i < p.L) off = p.o_fccw + k * p.L + i;
        else if (i == p.L) off = p.o_fccb + k;
        else if (i < p.L + 1 + p.S) off = p.o_mu + (int64_t)(i - p.L - 1) * (p.L + p.C) + p.L + k;
        else if (i < p.L + 1 + 2 * p.S) off = p.o_sig + (int64_t)(i - p.L - 1 - p.S) * (p.L + p.C) + p.L + k;
        else off = p.o_fc6 + (int64_t)(i - p.L - 1 - 2 * p.S) * (p.C + p.S) + k;
        off += a * p.per_arm;
#pragma unroll
        for (int b = 0; b < 4; ++b)
            if (p.buf[b]) p.buf[b][off] = 0.f;
    }
}

// cat_mask: bit k set = category k kept (bits at or above C ignored); the caller has checked that one category is kept, and
// a mask that keeps all of them launches nothing
int launch_prune_apply(const mmvae_dims& d, const POff& po, const uint32_t cat_mask[4], float* params, float* grads,
                       float* exp_avg, float* exp_avg_sq, hipStream_t s) {
    PruneArgs p{};
    p.buf[0] = params; p.buf[1] = grads; p.buf[2] = exp_avg; p.buf[3] = exp_avg_sq;
    p.per_arm = po.per_arm;
    p.o_fccw = po.o[10]; p.o_fccb = po.o[11]; p.o_mu = po.o[12]; p.o_sig = po.o[13]; p.o_fc6 = po.o[16];
    p.A = d.A; p.L = d.L; p.C = d.C; p.S = d.S;
    for (int k = 0; k < d.C; ++k)
        if (!((cat_mask[k >> 5] >> (k & 31)) & 1u)) p.cat[p.n_cat++] = (uint8_t)k;
    if (p.n_cat == 0) return 0;
    const int total = d.A * p.n_cat * (2 * d.L + 1 + 2 * d.S);
    hipLaunchKernelGGL(k_prune_apply, dim3(min(cdiv(total, 256), 256)), dim3(256), 0, s, p);
    HIP_LAUNCH_CHECK("k_prune_apply");
    return 0;
}

}  // namespace mmvae

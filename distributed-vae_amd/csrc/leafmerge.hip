// Leaf posteriors merged up a tree (mmidas/utils/analysis_tree_helpers.py: predict_leaf_gmm; include/mmvae.h, DESIGN.md
// section 9j).  mmvae_gauss_scores leaves every cell's score (log weight + log density) under each of the L leaf Gaussians;
// the two launches here carry what follows it: the scores of a cell become its posterior over the leaves, normalised in the
// log domain, and for every merge level of the tree the posteriors of the leaves under each label are added and the label
// with the largest sum is taken.  Both kernels give one wave to a cell: the cell's L values are one short row (115 leaves:
// 920 bytes) that the wave's lanes read together, and no value of a cell depends on another cell.  No LDS, no atomics.
#include "common.hpp"

namespace mmvae {

__device__ inline int lm_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// np.argmax's order: a NaN is above every number and NaNs are equal
__device__ inline bool lm_above(double x, double y) { return x > y || (x != x && y == y); }

// One wave a row, lane j the columns j, j + 64, ...  m: the row's largest score (exact, whatever the order).  e_l =
// exp(s_l - m) is kept in the row between the passes (a lane reads back only what it wrote).  Z: lane j adds its e in
// column order from 0.0, then six butterfly steps z_j <- z_j + z_(j xor h), h = 32, 16, 8, 4, 2, 1 (an fp64 add
// commutes, so every lane holds the same bits); p_l = e_l / Z, a correctly rounded division.  A row of -inf only has
// s - m = NaN and comes out NaN throughout.
__global__ __launch_bounds__(64 * LM_WAVES) void k_lm_normalise(double* __restrict__ p, int64_t ldp, int64_t n, int L) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int64_t r = (int64_t)blockIdx.x * LM_WAVES + wave; r < n; r += (int64_t)gridDim.x * LM_WAVES) {
        double* row = p + r * ldp;
        double m = -__builtin_inf();
        for (int l = lane; l < L; l += 64) {
            const double s = row[l];
            m = s > m ? s : m;
        }
        for (int h = 32; h > 0; h >>= 1) {
            const double o = __shfl_xor(m, h);
            m = o > m ? o : m;
        }
        double z = 0.0;
        for (int l = lane; l < L; l += 64) {
            const double e = exp(row[l] - m);
            row[l] = e;
            z += e;
        }
        for (int h = 32; h > 0; h >>= 1) z += __shfl_xor(z, h);
        for (int l = lane; l < L; l += 64) row[l] = row[l] / z;
    }
}

// One wave a (cell, level), lane j the labels j, j + 64, ... of the level.  P_k: the posteriors of label k's leaves added
// one by one, in list order, from 0.0.  Every lane keeps the best two sums of its labels (the lowest label on ties), the
// wave merges them in six butterfly steps; the order is lm_above's, so the label is np.argmax's and prob np.max's.  Every
// index read from a table is clamped to its array.
__global__ __launch_bounds__(64 * LM_WAVES) void k_lm_merge(
    const double* __restrict__ p, int64_t ldp, int64_t n, int L, const int* __restrict__ level_start, const int* __restrict__ start,
    int K_total, int K_max, const int* __restrict__ leaf, int nnz, int* __restrict__ label, double* __restrict__ prob,
    double* __restrict__ second, double* __restrict__ merged, int K0) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int t = blockIdx.y;
    const int ls0 = lm_clamp(level_start[t], 0, K_total), ls1 = lm_clamp(level_start[t + 1], ls0, K_total);
    const int K = ls1 - ls0 < K_max ? ls1 - ls0 : K_max;
    const bool keep = merged != nullptr && t == 0;
    const double ninf = -__builtin_inf();
    for (int64_t r = (int64_t)blockIdx.x * LM_WAVES + wave; r < n; r += (int64_t)gridDim.x * LM_WAVES) {
        const double* row = p + r * ldp;
        double b1 = ninf, b2 = ninf;            // below every sum: a sum is >= 0 or NaN
        int i1 = INT32_MAX;
        for (int k = lane; k < K; k += 64) {
            const int a = lm_clamp(start[ls0 + k], 0, nnz), b = lm_clamp(start[ls0 + k + 1], a, nnz);
            double acc = 0.0;
            for (int j = a; j < b; ++j) acc += row[lm_clamp(leaf[j], 0, L - 1)];
            if (keep && k < K0) merged[r * K0 + k] = acc;
            if (lm_above(acc, b1)) {
                b2 = b1;
                b1 = acc;
                i1 = k;
            } else if (lm_above(acc, b2)) {
                b2 = acc;
            }
        }
        if (keep)
            for (int k = K + lane; k < K0; k += 64) merged[r * K0 + k] = 0.0;
        for (int h = 32; h > 0; h >>= 1) {
            const double o1 = __shfl_xor(b1, h), o2 = __shfl_xor(b2, h);
            const int oi = __shfl_xor(i1, h);
            if (lm_above(o1, b1) || (!lm_above(b1, o1) && oi < i1)) {       // the other lane's best wins
                b2 = lm_above(b1, o2) ? b1 : o2;
                b1 = o1;
                i1 = oi;
            } else {
                b2 = lm_above(o1, b2) ? o1 : b2;
            }
        }
        if (lane == 0) {
            const int64_t out = (int64_t)t * n + r;
            label[out] = K > 0 ? i1 : 0;
            prob[out] = K > 0 ? b1 : 0.0;
            if (second) second[out] = K > 1 ? b2 : 0.0;
        }
    }
}

int launch_leaf_merge(double* p, int64_t ldp, int64_t n, int L, const int* level_start, int T, const int* start, int K_total,
                      int K_max, const int* leaf, int nnz, int* label, double* prob, double* second, double* merged, int K0,
                      hipStream_t st) {
    const unsigned gx = (unsigned)imin64(cdiv64(n, LM_WAVES), LM_MAX_GRID);
    hipLaunchKernelGGL(k_lm_normalise, dim3(gx), dim3(64 * LM_WAVES), 0, st, p, ldp, n, L);
    HIP_LAUNCH_CHECK("k_lm_normalise");
    hipLaunchKernelGGL(k_lm_merge, dim3(gx, (unsigned)T), dim3(64 * LM_WAVES), 0, st, p, ldp, n, L, level_start, start, K_total, K_max,
                       leaf, nnz, label, prob, second, merged, K0);
    HIP_LAUNCH_CHECK("k_lm_merge");
    return 0;
}

}  // namespace mmvae

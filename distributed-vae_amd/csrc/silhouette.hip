// Silhouette samples on the device.
//
// The reference scores the clusterability of the latents with sklearn's silhouette_samples(X, labels, metric="euclidean")
// (mmidas/utils/cluster_analysis.py: get_SilhScore, cluster_compare): for cell i with label l_i and cluster sizes f_k,
//   S(i, k) = sum over the cells j of cluster k of |x_i - x_j|,  a_i = S(i, l_i) / (f_{l_i} - 1),
//   b_i = min over k != l_i of S(i, k) / f_k,  s_i = (b_i - a_i) / max(a_i, b_i),  0 for a singleton and for a_i = b_i = 0.
// That is n^2 distances.  The caller hands the cells sorted by label, so a cluster is a run of columns; the runs are cut into
// segments of at most SIL_SEG_COLS columns (k_segments, segments.hip: the scheme is described once, in common.hpp above
// launch_segments; cseg here is its gseg), one workgroup adds one segment's distances for 256 rows
// (k_sil_partial: one thread per row, the segment's columns staged in LDS and read by all lanes at one address) and a last
// launch adds every cluster's segments in order and forms a, b and s (k_sil_finish).  Distances are fp32 in difference form
// (pairdist.hpp: subtract, fma the squares in coordinate order; then v_sqrt_f32), everything after them fp64.  No atomics:
// every sum has one owner and a fixed order, so the result is the same bits on every run.
#include "pairdist.hpp"

namespace mmvae {

// grid (nseg_max segments, row tiles of SIL_ROW_TILE), 256 threads: part[s][i] = the sum over the columns j of segment s of
// |x_i - x_j|, added in column order into one fp64 register per row; four columns per iteration, their distances independent.
// DV: float4 pieces per point (pairdist.hpp).  x_i sits in registers, the columns in LDS (SIL_LDS_FLOATS / (4 DV) per pass,
// every lane reading the same address: a broadcast, no bank conflict).
template <int DV>
__global__ __launch_bounds__(256) void k_sil_partial(const float* __restrict__ x, int64_t ld, int64_t n, int d,
                                                     const int* __restrict__ cseg, int K, const int64_t* __restrict__ seg_begin,
                                                     double* __restrict__ part) {
    constexpr int CT = SIL_LDS_FLOATS / (4 * DV);   // columns per pass
    __shared__ float4 cols[SIL_LDS_FLOATS / 4];
    const int seg = blockIdx.x;
    if (seg >= cseg[K]) return;                     // the whole workgroup
    int64_t c0, c1;
    seg_range(seg_begin, seg, n, SIL_SEG_COLS, c0, c1);
    const int tid = threadIdx.x;
    for (int64_t rt = blockIdx.y; rt * SIL_ROW_TILE < n; rt += gridDim.y) {
        const int64_t row = rt * SIL_ROW_TILE + tid;
        const bool valid = row < n;
        float4 xi[DV];
        pd_load<DV>(x, ld, row, d, valid, xi);
        double acc = 0.0;
        for (int64_t cb = c0; cb < c1; cb += CT) {
            const int m = (int)imin64(CT, c1 - cb);
            __syncthreads();                        // the pass before has been read
            pd_stage<DV, 256>(x, ld, cb, m, d, cols, tid);
            __syncthreads();
            auto dist = [&](int j) { return __builtin_amdgcn_sqrtf(pd_dist2<DV>(xi, cols, j)); };   // v_sqrt_f32: 1 ulp
            int j = 0;
            for (; j + 4 <= m; j += 4) {
                const float r0 = dist(j), r1 = dist(j + 1), r2 = dist(j + 2), r3 = dist(j + 3);
                acc += (double)r0;
                acc += (double)r1;
                acc += (double)r2;
                acc += (double)r3;
            }
            for (; j < m; ++j) acc += (double)dist(j);
        }
        if (valid) part[(int64_t)seg * n + row] = acc;
    }
}

// One thread per sorted row r: its cluster by bisection of the offsets, every cluster's segments added in order, the means,
// the minimum and s, written to s[perm[r]] (perm null: s[r]).  All lanes walk the same clusters and segments, so the reads of
// part[s][.] are consecutive across a wave.
__global__ __launch_bounds__(256) void k_sil_finish(const double* __restrict__ part, const int64_t* __restrict__ offsets, int K,
                                                    int64_t n, const int* __restrict__ cseg, int64_t nseg_max,
                                                    const int64_t* __restrict__ perm, double* __restrict__ s) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    int lo = 0, hi = K;                             // the last k with offsets[k] <= r
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (offsets[mid] <= r) lo = mid;
        else hi = mid;
    }
    const int own = lo;
    double a = 0.0, b = __builtin_inf();
    int64_t f_own = 0;
    for (int k = 0; k < K; ++k) {
        const int64_t f = offsets[k + 1] - offsets[k];
        if (f <= 0) continue;
        const int s0 = cseg[k];
        const int s1 = (int)imin64(cseg[k + 1], nseg_max);
        double sum = 0.0;
        for (int sg = s0; sg < s1; ++sg) sum += part[(int64_t)sg * n + r];
        if (k == own) {
            f_own = f;
            a = f > 1 ? sum / (double)(f - 1) : 0.0;
        } else {
            const double mean = sum / (double)f;
            b = mean < b ? mean : b;
        }
    }
    double out = 0.0;                               // a singleton, no other cluster, or a = b = 0
    if (f_own > 1 && b < __builtin_inf()) {
        const double m = a > b ? a : b;
        if (m > 0.0) out = (b - a) / m;
    }
    int64_t dst = perm ? perm[r] : r;
    if (dst < 0 || dst >= n) dst = r;               // a permutation that is none must not write outside s
    s[dst] = out;
}

int sil_dv(int d) {
    for (int i = 0; i < SIL_N_DV; ++i)
        if (4 * SIL_DV[i] >= d) return SIL_DV[i];
    return 0;
}

// ws: part double [nseg_max][n], seg_begin int64 [nseg_max + 1], cseg int32 [K + 1] (mmvae_silhouette_workspace_bytes)
int launch_silhouette(const float* x, int64_t ld, int64_t n, int d, const int64_t* offsets, int K, const int64_t* perm, void* ws,
                      double* s, hipStream_t st) {
    const int64_t nseg = nseg_max(n, K, SIL_SEG_COLS);
    const SegWs w = seg_ws_carve(ws, nseg, n);
    if (int rc = launch_segments(offsets, K, n, SIL_SEG_COLS, nseg, w.gseg, w.seg_begin, st)) return rc;
    const dim3 grid((unsigned)nseg, (unsigned)imin64(cdiv64(n, SIL_ROW_TILE), 65535)), block(256);
    if (int rc = pd_dispatch("silhouette", d, [&](auto dv) {
            hipLaunchKernelGGL(k_sil_partial<decltype(dv)::value>, grid, block, 0, st, x, ld, n, d, w.gseg, K, w.seg_begin, w.part);
        }))
        return rc;
    HIP_LAUNCH_CHECK("k_sil_partial");
    hipLaunchKernelGGL(k_sil_finish, dim3((unsigned)cdiv64(n, 256)), dim3(256), 0, st, w.part, offsets, K, n, w.gseg, nseg, perm, s);
    HIP_LAUNCH_CHECK("k_sil_finish");
    return 0;
}

}  // namespace mmvae

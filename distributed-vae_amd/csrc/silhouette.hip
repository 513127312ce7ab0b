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
// (subtract, fma the squares in coordinate order, v_sqrt_f32), everything after them fp64.  No atomics: every sum has one
// owner and a fixed order, so the result is the same bits on every run.
#include "common.hpp"

namespace mmvae {

// grid (nseg_max segments, row tiles of SIL_ROW_TILE), 256 threads: part[s][i] = the sum over the columns j of segment s of
// |x_i - x_j|, added in column order into one fp64 register per row; four columns per iteration, their distances independent.
// DV: float4 pieces per point, 4 DV >= d; the coordinates d .. 4 DV - 1 are zeros on both sides, and fma(0, 0, acc) = acc
// exactly, so a row's bits do not depend on DV.  x_i sits in registers, the columns in LDS (SIL_LDS_FLOATS / (4 DV) per
// pass, every lane reading the same address: a broadcast, no bank conflict).
template <int DV>
__global__ __launch_bounds__(256) void k_sil_partial(const float* __restrict__ x, int64_t ld, int64_t n, int d,
                                                     const int* __restrict__ cseg, int K, const int64_t* __restrict__ seg_begin,
                                                     double* __restrict__ part) {
    constexpr int W = 4 * DV;                       // floats per staged column
    constexpr int CT = SIL_LDS_FLOATS / W;          // columns per pass
    __shared__ float4 cols[SIL_LDS_FLOATS / 4];
    const int seg = blockIdx.x;
    if (seg >= cseg[K]) return;                     // the whole workgroup
    int64_t c0, c1;
    seg_range(seg_begin, seg, n, SIL_SEG_COLS, c0, c1);
    const int tid = threadIdx.x;
    float* cf = reinterpret_cast<float*>(cols);
    for (int64_t rt = blockIdx.y; rt * SIL_ROW_TILE < n; rt += gridDim.y) {
        const int64_t row = rt * SIL_ROW_TILE + tid;
        const bool valid = row < n;
        float4 xi[DV];
#pragma unroll
        for (int v = 0; v < DV; ++v) {
            float t[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) t[e] = valid && 4 * v + e < d ? x[row * ld + 4 * v + e] : 0.f;
            xi[v] = make_float4(t[0], t[1], t[2], t[3]);
        }
        double acc = 0.0;
        for (int64_t cb = c0; cb < c1; cb += CT) {
            const int m = (int)imin64(CT, c1 - cb);
            __syncthreads();                        // the pass before has been read
            for (int e = tid; e < m * W; e += 256) {
                const int c = e / W, k = e - c * W;
                cf[e] = k < d ? x[(cb + c) * ld + k] : 0.f;
            }
            __syncthreads();
            auto dist = [&](int j) {
                float q = 0.f;
#pragma unroll
                for (int v = 0; v < DV; ++v) {
                    const float4 y = cols[j * DV + v];
                    const float d0 = xi[v].x - y.x, d1 = xi[v].y - y.y, d2 = xi[v].z - y.z, d3 = xi[v].w - y.w;
                    q = __builtin_fmaf(d0, d0, q);
                    q = __builtin_fmaf(d1, d1, q);
                    q = __builtin_fmaf(d2, d2, q);
                    q = __builtin_fmaf(d3, d3, q);
                }
                return __builtin_amdgcn_sqrtf(q);   // v_sqrt_f32: 1 ulp
            };
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
    const auto [part, seg_begin, cseg] = seg_ws_carve(ws, nseg, n);
    if (int rc = launch_segments(offsets, K, n, SIL_SEG_COLS, nseg, cseg, seg_begin, st)) return rc;
    const dim3 grid((unsigned)nseg, (unsigned)imin64(cdiv64(n, SIL_ROW_TILE), 65535)), block(256);
#define SIL_CASE(V)                                                                                              \
    case V:                                                                                                      \
        hipLaunchKernelGGL(k_sil_partial<V>, grid, block, 0, st, x, ld, n, d, cseg, K, seg_begin, part);         \
        break;
    switch (sil_dv(d)) {
        SIL_CASE(1) SIL_CASE(2) SIL_CASE(3) SIL_CASE(4) SIL_CASE(6) SIL_CASE(8) SIL_CASE(12) SIL_CASE(16) SIL_CASE(24) SIL_CASE(32)
        default: set_error("silhouette: no kernel for d = %d", d); return MMVAE_E_UNSUPPORTED;
    }
#undef SIL_CASE
    HIP_LAUNCH_CHECK("k_sil_partial");
    hipLaunchKernelGGL(k_sil_finish, dim3((unsigned)cdiv64(n, 256)), dim3(256), 0, st, part, offsets, K, n, cseg, nseg, perm, s);
    HIP_LAUNCH_CHECK("k_sil_finish");
    return 0;
}

}  // namespace mmvae

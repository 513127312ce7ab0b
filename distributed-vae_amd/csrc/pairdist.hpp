// The fp32 squared distance in difference form of k_sil_partial (silhouette.hip) and k_knn_partial (knn.hip): a point is DV
// float4 pieces, 4 DV >= d, the coordinates from d on zeros.  Subtract, fma the squares in rising coordinate order from +0;
// the padding adds fma(0, 0, acc) = acc exactly, so a pair's bits do not depend on DV.  The instances are those of SIL_DV.
#pragma once
#include <type_traits>
#include "common.hpp"

namespace mmvae {

// row `row` of x as xi; zeros where !valid (a thread past the last row still meets the barriers)
template <int DV>
__device__ __forceinline__ void pd_load(const float* __restrict__ x, int64_t ld, int64_t row, int d, bool valid, float4 (&xi)[DV]) {
#pragma unroll
    for (int v = 0; v < DV; ++v) {
        float t[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) t[e] = valid && 4 * v + e < d ? x[row * ld + 4 * v + e] : 0.f;
        xi[v] = make_float4(t[0], t[1], t[2], t[3]);
    }
}

// the rows cb .. cb + m - 1 of x as the columns 0 .. m - 1 of cols, by the NT threads of the workgroup (tid: this one)
template <int DV, int NT>
__device__ __forceinline__ void pd_stage(const float* __restrict__ x, int64_t ld, int64_t cb, int m, int d, float4* cols, int tid) {
    float* cf = reinterpret_cast<float*>(cols);
    for (int e = tid; e < m * 4 * DV; e += NT) {
        const int c = e / (4 * DV), k = e - c * 4 * DV;
        cf[e] = k < d ? x[(cb + c) * ld + k] : 0.f;
    }
}

// |xi - column j|^2
template <int DV>
__device__ __forceinline__ float pd_dist2(const float4 (&xi)[DV], const float4* cols, int j) {
    float a = 0.f;
#pragma unroll
    for (int v = 0; v < DV; ++v) {
        const float4 y = cols[j * DV + v];
        const float d0 = xi[v].x - y.x, d1 = xi[v].y - y.y, d2 = xi[v].z - y.z, d3 = xi[v].w - y.w;
        a = __builtin_fmaf(d0, d0, a);
        a = __builtin_fmaf(d1, d1, a);
        a = __builtin_fmaf(d2, d2, a);
        a = __builtin_fmaf(d3, d3, a);
    }
    return a;
}

// f(std::integral_constant<int, DV>) for the DV of SIL_DV that holds d coordinates; the refusal of `who` where none does
template <int I = 0, class F>
inline int pd_dispatch(const char* who, int d, F f) {
    if constexpr (I < SIL_N_DV)
        return sil_dv(d) == SIL_DV[I] ? (f(std::integral_constant<int, SIL_DV[I]>{}), 0) : pd_dispatch<I + 1>(who, d, f);
    set_error("%s: no kernel for d = %d", who, d);
    return MMVAE_E_UNSUPPORTED;
}

}  // namespace mmvae

// The segment table of the grouped reductions: silhouette.hip, statecorr.hip and gaussclf.hip cut
// their groups of rows with this one kernel; the scheme and the workspace it lives in are described in common.hpp, above
// launch_segments.
#include "common.hpp"

namespace mmvae {

// One workgroup.  offsets [G + 1] non-decreasing from 0 to n (the caller's contract; null: one group, 0 and n).  Thread t
// owns the groups t per .. t per + per - 1, per = ceil(G / 256): it counts their segments, thread 0 turns the 256 counts into
// first-segment numbers, and every thread writes its groups' entries.  Every offset is clamped to [0, n]: offsets that break
// the contract give a table that is wrong but stays inside [0, nseg_max] x [0, n], and the later launches clamp as well
// (seg_range).
__global__ __launch_bounds__(256) void k_segments(const int64_t* __restrict__ offsets, int G, int64_t n, int seg_len,
                                                  int64_t nseg_max, int* __restrict__ gseg, int64_t* __restrict__ seg_begin) {
    __shared__ int64_t part[257];
    const int tid = threadIdx.x;
    const int per = (G + 255) / 256;
    const int k0 = (int)imin64((int64_t)tid * per, G), k1 = (int)imin64((int64_t)k0 + per, G);
    auto off = [&](int k) { return offsets ? clamp64(offsets[k], 0, n) : (k == 0 ? (int64_t)0 : n); };
    int64_t cnt = 0;
    for (int k = k0; k < k1; ++k) {
        const int64_t f = off(k + 1) - off(k);
        // ceil(f / seg_len) in 32-bit unsigned arithmetic: f <= n <= 2^31, so f + seg_len - 1 < 2^32, and a 64-bit division by
        // a value the compiler does not know is a long routine
        if (f > 0) cnt += ((uint32_t)f + (uint32_t)seg_len - 1u) / (uint32_t)seg_len;
    }
    part[tid] = cnt;
    __syncthreads();
    if (tid == 0) {
        int64_t run = 0;
        for (int t = 0; t < 256; ++t) {
            const int64_t c = part[t];
            part[t] = run;
            run += c;
        }
        part[256] = run;
    }
    __syncthreads();
    int64_t s = part[tid];
    for (int k = k0; k < k1; ++k) {
        gseg[k] = (int)imin64(s, nseg_max);
        const int64_t beg = off(k), f = off(k + 1) - beg;
        for (int64_t c = 0; c < f && s < nseg_max; c += seg_len, ++s) seg_begin[s] = beg + c;
    }
    if (tid == 0) {
        const int64_t total = imin64(part[256], nseg_max);
        gseg[G] = (int)total;
        seg_begin[total] = off(G);
    }
}

int launch_segments(const int64_t* offsets, int G, int64_t n, int seg_len, int64_t nseg_max, int* gseg, int64_t* seg_begin,
                    hipStream_t st) {
    hipLaunchKernelGGL(k_segments, dim3(1), dim3(256), 0, st, offsets, G, n, seg_len, nseg_max, gseg, seg_begin);
    HIP_LAUNCH_CHECK("k_segments");
    return 0;
}

}  // namespace mmvae

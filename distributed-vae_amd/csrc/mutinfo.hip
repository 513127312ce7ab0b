// Mutual-information evaluation on the device.
//
// The reference scores a trained model with evaluation.py::mutinfo: for every cell-type column f of the one-hot targets and
// every occupied cluster c it calls sklearn's adjusted_mutual_info_score on two length-N binary labelings, u = targets[:, f]
// and v = [label == c].  A pair of binary labelings is three integers, n11 = #(u & v), t = #u, p = #v, and N; so the whole
// job is one contingency count (k_mi_counts) and one batch of 2 x 2 adjusted-MI evaluations from counts (k_ami_binary).
#include "common.hpp"

namespace mmvae {

constexpr int MI_CHUNK = 1024;                 // cells per workgroup of k_mi_counts: a 32-bit LDS count cannot overflow

// grid (cell chunks of MI_CHUNK, arms), 256 threads.  labels [A][n]; targets row-major [n][ldt], columns 0..F-1 used, T the
// element type (uint8_t or int32_t); counts [A][F][C], p_sum [A][C], t_sum [F] (added by the workgroups of arm 0 alone).
// LDS = true: the workgroup counts its cells in 32-bit LDS histograms (F*C + C + F words) and adds the non-zero entries to
// the global 64-bit counts at the end; LDS = false (the histograms do not fit): every count is a global atomic.  All adds are
// integer atomics, so the result does not depend on their order.
template <bool LDS, typename T>
__global__ __launch_bounds__(256) void k_mi_counts(const int32_t* __restrict__ labels, int64_t n, int C,
                                                   const T* __restrict__ targets, int64_t ldt, int F,
                                                   unsigned long long* __restrict__ counts,
                                                   unsigned long long* __restrict__ t_sum,
                                                   unsigned long long* __restrict__ p_sum) {
    extern __shared__ unsigned int mi_hist[];  // [F*C] counts, [C] p, [F] t
    const int a = blockIdx.y;
    const int FC = F * C;
    unsigned int* h_p = mi_hist + FC;
    unsigned int* h_t = h_p + C;
    if (LDS) {
        for (int e = threadIdx.x; e < FC + C + F; e += blockDim.x) mi_hist[e] = 0u;
        __syncthreads();
    }
    const int64_t beg = (int64_t)blockIdx.x * MI_CHUNK;
    const int64_t end = beg + MI_CHUNK < n ? beg + MI_CHUNK : n;
    const int32_t* lab = labels + (int64_t)a * n;
    unsigned long long* cnt = counts + (int64_t)a * FC;
    unsigned long long* ps = p_sum + (int64_t)a * C;
    for (int64_t i = beg + threadIdx.x; i < end; i += blockDim.x) {
        const int l = lab[i];
        if ((unsigned)l < (unsigned)C) {
            if (LDS) atomicAdd(h_p + l, 1u);
            else atomicAdd(ps + l, 1ull);
        }
    }
    // the chunk's target entries in memory order: consecutive lanes read consecutive columns of a row
    const int m = (int)(end - beg) * F;        // <= 1024 * 4096
    for (int e = threadIdx.x; e < m; e += blockDim.x) {
        const int r = e / F, f = e - r * F;
        const int64_t cell = beg + r;
        if (targets[cell * ldt + f] != 0) {
            if (a == 0) {
                if (LDS) atomicAdd(h_t + f, 1u);
                else atomicAdd(t_sum + f, 1ull);
            }
            const int l = lab[cell];
            if ((unsigned)l < (unsigned)C) {
                if (LDS) atomicAdd(mi_hist + f * C + l, 1u);
                else atomicAdd(cnt + (int64_t)f * C + l, 1ull);
            }
        }
    }
    if (LDS) {
        __syncthreads();
        for (int e = threadIdx.x; e < FC; e += blockDim.x) {
            const unsigned int v = mi_hist[e];
            if (v) atomicAdd(cnt + e, (unsigned long long)v);
        }
        for (int e = threadIdx.x; e < C; e += blockDim.x) {
            const unsigned int v = h_p[e];
            if (v) atomicAdd(ps + e, (unsigned long long)v);
        }
        if (a == 0)
            for (int e = threadIdx.x; e < F; e += blockDim.x) {
                const unsigned int v = h_t[e];
                if (v) atomicAdd(t_sum + e, (unsigned long long)v);
            }
    }
}

// ws[k] = lgamma(k + 1), ws[N + 1 + k] = log(k) (0 at k = 0, never read), k = 0..N
__global__ __launch_bounds__(256) void k_mi_table(double* __restrict__ ws, int64_t N) {
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k <= N; k += (int64_t)gridDim.x * blockDim.x) {
        ws[k] = lgamma((double)k + 1.0);
        ws[N + 1 + k] = k ? log((double)k) : 0.0;
    }
}

template <bool TAB>
__device__ __forceinline__ double mi_lg(const double* __restrict__ lg, int64_t k) {   // lgamma(k + 1)
    return TAB ? lg[k] : lgamma((double)k + 1.0);
}
template <bool TAB>
__device__ __forceinline__ double mi_log(const double* __restrict__ lk, int64_t k) {
    return TAB ? lk[k] : log((double)k);
}

// One wave per table (a, f, c); 256 threads = 4 tables per workgroup.  sklearn.metrics.adjusted_mutual_info_score
// (average_method="arithmetic") of two binary labelings, from n11 = counts[a][f][c], t = t_sum[f], p = p_sum[a][c] and N:
//   contingency n = [[N-t-p+n11, p-n11], [t-n11, n11]], row sums a = [N-t, t], column sums b = [N-p, p];
//   both labelings single-valued: 1; exactly one: 0; else (MI - EMI) / ((H(u) + H(v)) / 2 - EMI), numerator and denominator
//   pushed away from zero by 2^-52 with their sign; MI terms below 2^-52 in magnitude dropped, MI clipped at 0.
// EMI (sklearn/metrics/cluster/_expected_mutual_info_fast.pyx) is a sum over the four cells and over
// nij = max(1, a_i + b_j - N) .. min(a_i, b_j) of (nij / N) (log(N nij) - log a_i - log b_j) exp(nine log-gammas), in the
// .pyx's operation order per term.  The lanes stride over nij inside each cell, every lane adds its terms in increasing
// (cell, nij) order and the 64 partial sums are combined by a fixed butterfly: the same bits on every run.
// TAB: log-gamma and log come from the table k_mi_table left in the workspace; else they are evaluated per term.
// p == 0 (not a cluster) or counts that are no contingency table of N cells: NaN -- the latter check also keeps every table
// index inside [0, N].
template <bool TAB>
__global__ __launch_bounds__(256) void k_ami_binary(const long long* __restrict__ n11s, const long long* __restrict__ t_sum,
                                                    const long long* __restrict__ p_sum, int64_t total, int F, int C,
                                                    int64_t N, const double* __restrict__ ws, double* __restrict__ ami) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= total) return;                                        // the whole wave
    const int c = (int)(w % C);
    const int f = (int)((w / C) % F);
    const int64_t arm = w / ((int64_t)F * C);
    const int64_t n11 = n11s[w], t = t_sum[f], p = p_sum[arm * C + c];
    const double* lg = TAB ? ws : nullptr;               // per term: no workspace, neither pointer is used
    const double* lk = TAB ? ws + (N + 1) : nullptr;
    double out;
    const bool table_ok = n11 >= 0 && n11 <= t && n11 <= p && t <= N && p <= N && t + p - n11 <= N;
    if (p == 0 || !table_ok) {
        out = __builtin_nan("");
    } else {
        const bool one_u = t == 0 || t == N, one_v = p == N;
        if (one_u && one_v) out = 1.0;
        else if (one_u || one_v) out = 0.0;
        else {                                                     // wave-uniform: every lane is here
            const int64_t av[2] = {N - t, t}, bv[2] = {N - p, p};
            const int64_t nn[2][2] = {{N - t - p + n11, p - n11}, {t - n11, n11}};
            const double dN = (double)N;
            const double logN = mi_log<TAB>(lk, N), glN = mi_lg<TAB>(lg, N);
            double acc = 0.0;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int64_t ai = av[i], bj = bv[j];
                    const double log_a = mi_log<TAB>(lk, ai), log_b = mi_log<TAB>(lk, bj);
                    const double g4 = mi_lg<TAB>(lg, ai) + mi_lg<TAB>(lg, bj) + mi_lg<TAB>(lg, N - ai) + mi_lg<TAB>(lg, N - bj);
                    const int64_t lo = ai + bj - N > 1 ? ai + bj - N : 1;
                    const int64_t hi = ai < bj ? ai : bj;
                    for (int64_t nij = lo + lane; nij <= hi; nij += 64) {
                        const double term1 = (double)nij / dN;
                        const double term2 = (logN + mi_log<TAB>(lk, nij)) - log_a - log_b;
                        const double gln = g4 - (mi_lg<TAB>(lg, nij) + glN) - mi_lg<TAB>(lg, ai - nij) - mi_lg<TAB>(lg, bj - nij) -
                                           mi_lg<TAB>(lg, N - ai - bj + nij);
                        acc += term1 * term2 * exp(gln);
                    }
                }
#pragma unroll
            for (int o = 32; o; o >>= 1) acc += __shfl_xor(acc, o);
            const double emi = acc;
            double mi = 0.0;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int64_t v = nn[i][j];
                    if (v > 0) {
                        const double cnm = (double)v / dN;
                        double term = cnm * (log((double)v) - logN) + cnm * (-log((double)(av[i] * bv[j])) + logN + logN);
                        if (fabs(term) < 0x1p-52) term = 0.0;
                        mi += term;
                    }
                }
            mi = mi > 0.0 ? mi : 0.0;
            const double hu = -((double)av[0] / dN * (log((double)av[0]) - logN) + (double)av[1] / dN * (log((double)av[1]) - logN));
            const double hv = -((double)bv[0] / dN * (log((double)bv[0]) - logN) + (double)bv[1] / dN * (log((double)bv[1]) - logN));
            double den = (hu + hv) / 2.0 - emi;
            den = den < 0.0 ? fmin(den, -0x1p-52) : fmax(den, 0x1p-52);
            double num = mi - emi;
            num = num < 0.0 ? fmin(num, -0x1p-52) : fmax(num, 0x1p-52);
            out = num / den;
        }
    }
    if (lane == 0) ami[w] = out;
}

// path: -1 the rule below, 0 the LDS histograms, 1 global atomics (both stay callable: tests and the timing tool run each on
// the same input).  tsize: bytes per target element, 1 or 4 (validated by the caller).
int launch_mi_counts(const int32_t* labels, int A, int64_t n, int C, const void* targets, int tsize, int64_t ldt, int F,
                     int64_t* counts, int64_t* t_sum, int64_t* p_sum, int path, hipStream_t s) {
    // MI_LDS_MAX_WORDS = 16384 32-bit counts = the 64 KiB of LDS a workgroup gets without asking: F = 115 cell types x C = 92
    // categories need 10 787 words (43 KB), so three workgroups share a CU's 160 KB of LDS
    const int64_t words = (int64_t)F * C + C + F;
    const bool fits = words <= MI_LDS_MAX_WORDS;
    if (path == 0 && !fits) {
        set_error("mutinfo_counts: no LDS histogram for F * C + C + F = %lld > %d", (long long)words, MI_LDS_MAX_WORDS);
        return MMVAE_E_UNSUPPORTED;
    }
    const bool lds = path < 0 ? fits : path == 0;
    const dim3 grid((unsigned)cdiv64(n, MI_CHUNK), A), block(256);
    const size_t shm = lds ? (size_t)words * sizeof(unsigned int) : 0;
    auto* cnt = reinterpret_cast<unsigned long long*>(counts);
    auto* ts = reinterpret_cast<unsigned long long*>(t_sum);
    auto* ps = reinterpret_cast<unsigned long long*>(p_sum);
    if (tsize == 1) {
        const auto* tg = static_cast<const uint8_t*>(targets);
        if (lds) hipLaunchKernelGGL((k_mi_counts<true, uint8_t>), grid, block, shm, s, labels, n, C, tg, ldt, F, cnt, ts, ps);
        else hipLaunchKernelGGL((k_mi_counts<false, uint8_t>), grid, block, shm, s, labels, n, C, tg, ldt, F, cnt, ts, ps);
    } else {
        const auto* tg = static_cast<const int32_t*>(targets);
        if (lds) hipLaunchKernelGGL((k_mi_counts<true, int32_t>), grid, block, shm, s, labels, n, C, tg, ldt, F, cnt, ts, ps);
        else hipLaunchKernelGGL((k_mi_counts<false, int32_t>), grid, block, shm, s, labels, n, C, tg, ldt, F, cnt, ts, ps);
    }
    HIP_LAUNCH_CHECK("k_mi_counts");
    return 0;
}

// ws: 2 (N + 1) doubles for the table, or null: log-gamma and log per term
int launch_ami_binary(const int64_t* n11, const int64_t* t_sum, const int64_t* p_sum, int A, int F, int C, int64_t N, double* ws,
                      double* ami, hipStream_t s) {
    const int64_t total = (int64_t)A * F * C;
    const auto* q = reinterpret_cast<const long long*>(n11);
    const auto* ts = reinterpret_cast<const long long*>(t_sum);
    const auto* ps = reinterpret_cast<const long long*>(p_sum);
    const dim3 grid((unsigned)cdiv64(total, 4)), block(256);
    if (ws) {
        hipLaunchKernelGGL(k_mi_table, dim3((unsigned)imin64(1024, cdiv64(N + 1, 256))), dim3(256), 0, s, ws, N);
        HIP_LAUNCH_CHECK("k_mi_table");
        hipLaunchKernelGGL(k_ami_binary<true>, grid, block, 0, s, q, ts, ps, total, F, C, N, ws, ami);
    } else {
        hipLaunchKernelGGL(k_ami_binary<false>, grid, block, 0, s, q, ts, ps, total, F, C, N, ws, ami);
    }
    HIP_LAUNCH_CHECK("k_ami_binary");
    return 0;
}

}  // namespace mmvae

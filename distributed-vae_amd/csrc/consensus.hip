// Evaluation labels and the between-arm consensus on the device.
//
// Every epoch the reference re-runs the training set through the model in eval mode, copies the categorical
// probabilities c of every arm to the host, takes argmax (`classify`, mmidas/_utils.py:79-80), builds one
// C x C confusion matrix per arm pair with np.add.at (`compute_confmat`, :84-95), normalises it by
// max(row sum, column sum) (`confmat_normalize`, :98-100) and averages its diagonal (`confmat_mean`, :128-129)
// -- mmidas/cpl_mixvae.py:563-657.  Here the labels never leave the device: k_classify reads c from the workspace
// of the (encoder + latent block only) eval forward, k_confmat accumulates integer counts with atomics, and
// k_consensus does the normalisation and the mean in fp64 in numpy's summation order, so the result is bit-identical
// to the reference's host arithmetic (counts are integers; the only rounding is the division and the mean).
#include "common.hpp"

namespace mmvae {

// labels[a][b] = argmax_k c[a][b][k], first maximum on ties (np.argmax).  One wave per cell; grid-stride.
__global__ __launch_bounds__(256) void k_classify(const float* __restrict__ cc, int64_t n_cells, int C,
                                                  int32_t* __restrict__ labels) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t nwave = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t cell = wave; cell < n_cells; cell += nwave) {
        const float* p = cc + cell * C;
        float best = -INFINITY;
        int arg = 1 << 30;
        for (int k = lane; k < C; k += 64) {
            const float v = p[k];
            if (v > best) { best = v; arg = k; }   // strictly greater: the lane keeps its first maximum
        }
        const float m = wave_max(best);
        const int cand = wave_min_i(best == m ? arg : (1 << 30));
        if (lane == 0) labels[cell] = cand;
    }
}

// counts[pair(a,b)][labels[a][i]][labels[b][i]] += 1 for a < b, pairs in the reference's loop order
// (cpl_mixvae.py:644-653: for a in range(A): for b in range(a+1, A)).  labels: [A][n].
// Cells of one batch pile onto a few (label, label) cells -- arms that agree put everything on the diagonal -- so
// global atomics serialise (14.7 us for 5000 cells x 1 pair).  With `lds_pairs` > 0 a workgroup first counts its cells
// in an LDS histogram (32-bit, lds_pairs x C x C) and then adds its non-zero cells to the global counts.
__global__ __launch_bounds__(256) void k_confmat(const int32_t* __restrict__ labels, int A, int64_t n, int C,
                                                 unsigned long long* __restrict__ counts, int lds_pairs) {
    extern __shared__ unsigned int hist[];
    const int npairs = A * (A - 1) / 2;
    const bool use_lds = lds_pairs >= npairs;
    const int cells = npairs * C * C;
    if (use_lds) {
        for (int i = threadIdx.x; i < cells; i += blockDim.x) hist[i] = 0u;
        __syncthreads();
    }
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        int pair = 0;
        for (int a = 0; a < A; ++a) {
            const int la = labels[(int64_t)a * n + i];
            for (int b = a + 1; b < A; ++b, ++pair) {
                const int lb = labels[(int64_t)b * n + i];
                if ((unsigned)la < (unsigned)C && (unsigned)lb < (unsigned)C) {
                    const int64_t cell = ((int64_t)pair * C + la) * C + lb;
                    if (use_lds) atomicAdd(&hist[cell], 1u);
                    else atomicAdd(counts + cell, 1ull);
                }
            }
        }
    }
    if (use_lds) {
        __syncthreads();
        for (int i = threadIdx.x; i < cells; i += blockDim.x) {
            const unsigned int v = hist[i];
            if (v) atomicAdd(counts + i, (unsigned long long)v);
        }
    }
}

// numpy's pairwise summation of n <= 128 doubles with element stride `st` (numpy/core/src/umath/loops_utils.h,
// pairwise_sum: < 8 elements sequentially; else eight running sums, combined as a balanced tree, then the tail)
__device__ double np_pairwise_sum(const double* a, int n, int st) {
    if (n < 8) {
        double res = 0.0;
        for (int i = 0; i < n; ++i) res += a[i * st];
        return res;
    }
    double r[8];
    for (int k = 0; k < 8; ++k) r[k] = a[k * st];
    int i = 8;
    for (; i < n - (n % 8); i += 8)
        for (int k = 0; k < 8; ++k) r[k] += a[(i + k) * st];
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += a[i * st];
    return res;
}

// grid (npairs), 128 threads, C <= 128.  maxes[j] = max(column sum j, row sum j); norm[i][j] = cm[i][j] / maxes[j]
// where maxes[j] != 0 else 0 (np.divide broadcasts `maxes` along the last axis); consensus = mean(diag(norm)).
__global__ __launch_bounds__(128) void k_consensus(const unsigned long long* __restrict__ counts, int C,
                                                   double* __restrict__ cm_norm, double* __restrict__ consensus) {
    __shared__ double sh_max[128], sh_diag[128];
    const int pair = blockIdx.x, j = threadIdx.x;
    const unsigned long long* cm = counts + (int64_t)pair * C * C;
    if (j < C) {
        unsigned long long cs = 0, rs = 0;   // integer sums are exact (and equal numpy's float sums below 2^53)
        for (int i = 0; i < C; ++i) { cs += cm[(int64_t)i * C + j]; rs += cm[(int64_t)j * C + i]; }
        const double mx = (double)(cs > rs ? cs : rs);
        sh_max[j] = mx;
        sh_diag[j] = mx != 0.0 ? (double)cm[(int64_t)j * C + j] / mx : 0.0;
    }
    __syncthreads();
    if (cm_norm) {
        double* out = cm_norm + (int64_t)pair * C * C;
        for (int e = j; e < C * C; e += blockDim.x) {
            const double mx = sh_max[e % C];
            out[e] = mx != 0.0 ? (double)cm[e] / mx : 0.0;
        }
    }
    if (j == 0) consensus[pair] = np_pairwise_sum(sh_diag, C, 1) / (double)C;
}

// ---- cross-run evaluation: confusion counts plus a probability distance per matrix cell -------------------------------
// mmidas/_evals.py::evals2 compares the arms of two trained runs: for an arm pair and every cell i it adds 1 to
// pm[i1][i2] and sqrt((qa[i1] - qb[i2])^2) to emp[i1][i2], where i1 / i2 are the two arms' labels of the cell and qa / qb
// float64 copies of the fp32 probability rows of two arms -- not always the arms the labels came from (the within-run
// loops of _evals.py:98-143 and :145-191 take the second probability row from the enumerate index), so a pair names four
// arm indices (lab1, prob1, lab2, prob2) into [T] = run a's arms followed by run b's.  sqrt(x^2) of a double difference is
// |fl64(qa - qb)| exactly (radix 2), so that is the term.
//
// The distance sum must not depend on the arrival order, so it is a fixed-point integer sum (the idea of acc_add in
// common.hpp, with a window cut for probabilities): a term d (a double, 0 <= d < 2) becomes t = trunc(d * 2^52) < 2^53, at
// most 2^-52 below d (exact for d >= 1/2).  Sums of t are integers and commute.  The global accumulator of a matrix cell is
// two 64-bit slots (hi, lo): a partial sum S < 2^64 (one workgroup's LDS sum of <= PS_CHUNK = 2^11 terms, or one wave's
// sum of <= 64) adds S >> 32 to hi and S & (2^32 - 1) to lo; the value is (hi * 2^32 + lo) * 2^-52.  Every partial sum
// covers at least one cell, so after n <= 2^31 cells lo < 2^31 * 2^32 = 2^63 and hi <= (2^31 * 2^53) >> 32 = 2^52: neither
// slot overflows, and no carry is needed between them before the read.  A term outside the window (d >= 2, NaN, Inf: not a
// difference of probabilities) sets bit 62 of hi with an atomic OR, which the adds never reach and so commutes with them;
// k_pair_finish then returns NaN for that cell, as the reference's float sum would be useless there too.
constexpr int PS_CHUNK = 2048;                 // cells per workgroup: 2^11 terms below 2^53 fit an unsigned 64-bit LDS sum
constexpr int PS_MAX_PAIRS = 128;              // pairs per launch (the table travels as a kernel argument)
constexpr unsigned long long PS_POISON = 1ull << 62;
struct PairTab { uint32_t p[PS_MAX_PAIRS]; };  // lab1 | prob1 << 8 | lab2 << 16 | prob2 << 24

__device__ __forceinline__ void ps_flush(unsigned long long* __restrict__ cnt, unsigned long long* __restrict__ acc,
                                         int64_t e, unsigned long long k, unsigned long long S) {
    atomicAdd(cnt + e, k);
    const unsigned long long hi = S >> 32, lo = S & 0xFFFFFFFFull;
    if (hi) atomicAdd(acc + 2 * e, hi);
    if (lo) atomicAdd(acc + 2 * e + 1, lo);
}

// grid (cell chunks of PS_CHUNK, pairs), 256 threads.
// LDS = true: the workgroup's C x C histogram (64-bit distance sum + 32-bit count, 12 bytes per matrix cell) lives in LDS
//   and its non-zero cells are added to the global accumulators at the end: three global atomics per touched matrix cell and
//   workgroup, however many cells piled onto it.
// LDS = false (the histogram does not fit: C > PS_LDS_MAX_C): every wave takes 64 cells at a time, the lanes that share
//   (i1, i2) are combined with a ballot and an integer wave sum, and one lane issues the atomics of each distinct key.
template <bool LDS>
__global__ __launch_bounds__(256) void k_pair_stats(const int32_t* __restrict__ labels, const float* __restrict__ probs,
                                                    int64_t n, int C, PairTab tab, int pair0,
                                                    unsigned long long* __restrict__ counts,
                                                    unsigned long long* __restrict__ dist_acc) {
    extern __shared__ unsigned long long ps_sum[];           // [C*C] sums, then [C*C] 32-bit counts
    const int CC = C * C;
    unsigned int* ps_cnt = reinterpret_cast<unsigned int*>(ps_sum + CC);
    const uint32_t pw = tab.p[blockIdx.y];
    const int64_t l1 = pw & 255u, p1 = (pw >> 8) & 255u, l2 = (pw >> 16) & 255u, p2 = pw >> 24;
    const int64_t out0 = (int64_t)(pair0 + blockIdx.y) * CC;
    unsigned long long* cnt = counts + out0;
    unsigned long long* acc = dist_acc + 2 * out0;
    if (LDS) {
        for (int e = threadIdx.x; e < CC; e += blockDim.x) { ps_sum[e] = 0ull; ps_cnt[e] = 0u; }
        __syncthreads();
    }
    const int64_t beg = (int64_t)blockIdx.x * PS_CHUNK;
    const int64_t end = beg + PS_CHUNK < n ? beg + PS_CHUNK : n;
    // every lane of a wave runs the same number of rounds (the wave path votes); i >= end is an inactive lane
    for (int64_t i0 = beg; i0 < end; i0 += blockDim.x) {
        const int64_t i = i0 + threadIdx.x;
        int key = -1;
        unsigned long long t = 0ull;
        if (i < end) {
            const int i1 = labels[l1 * n + i], i2 = labels[l2 * n + i];
            if ((unsigned)i1 < (unsigned)C && (unsigned)i2 < (unsigned)C) {
                key = i1 * C + i2;
                const double d = fabs((double)probs[(p1 * n + i) * C + i1] - (double)probs[(p2 * n + i) * C + i2]);
                if (d < 2.0) t = (unsigned long long)(d * 0x1p52);
                else atomicOr(acc + 2 * (int64_t)key, PS_POISON);
            }
        }
        if (LDS) {
            if (key >= 0) {
                atomicAdd(ps_cnt + key, 1u);
                if (t) atomicAdd(ps_sum + key, t);
            }
        } else {
            const int lane = threadIdx.x & 63;
            unsigned long long todo = __ballot(key >= 0);
            while (todo) {
                const int lead = __ffsll((long long)todo) - 1;
                const int k = __shfl(key, lead);
                const bool mine = key == k;
                const unsigned long long same = __ballot(mine);
                unsigned long long S = mine ? t : 0ull;      // <= 64 terms below 2^53
#pragma unroll
                for (int o = 32; o; o >>= 1) S += __shfl_xor(S, o);
                if (lane == lead) ps_flush(cnt, acc, k, (unsigned long long)__popcll(same), S);
                todo &= ~same;
            }
        }
    }
    if (LDS) {
        __syncthreads();
        for (int e = threadIdx.x; e < CC; e += blockDim.x) {
            const unsigned int k = ps_cnt[e];
            if (k) ps_flush(cnt, acc, e, k, ps_sum[e]);
        }
    }
}

// grid (n_pairs), 128 threads, C <= 128; per pair, in fp64:
//   smp[j] = max(row sum j, column sum j) (integer sums, as k_consensus); cm_norm = counts / smp[j] along the last axis, 0
//   where smp[j] == 0 (the same bits as k_consensus's cm_norm); emp = the distance sums; dist_norm = emp / smp[j] by the
//   same rule; diag_mean = np.mean(np.diag(cm_norm)) in numpy's order; diag_min = np.min(np.diag(cm_norm)).
__global__ __launch_bounds__(128) void k_pair_finish(const unsigned long long* __restrict__ counts,
                                                     const unsigned long long* __restrict__ dist_acc, int C,
                                                     double* __restrict__ cm_norm, double* __restrict__ emp,
                                                     double* __restrict__ dist_norm, double* __restrict__ diag_mean,
                                                     double* __restrict__ diag_min) {
    __shared__ double sh_max[128], sh_diag[128];
    const int pair = blockIdx.x, j = threadIdx.x;
    const int64_t off = (int64_t)pair * C * C;
    const unsigned long long* cm = counts + off;
    if (j < C) {
        unsigned long long cs = 0, rs = 0;
        for (int i = 0; i < C; ++i) { cs += cm[(int64_t)i * C + j]; rs += cm[(int64_t)j * C + i]; }
        const double mx = (double)(cs > rs ? cs : rs);
        sh_max[j] = mx;
        sh_diag[j] = mx != 0.0 ? (double)cm[(int64_t)j * C + j] / mx : 0.0;
    }
    __syncthreads();
    for (int e = j; e < C * C; e += blockDim.x) {
        const double mx = sh_max[e % C];
        cm_norm[off + e] = mx != 0.0 ? (double)cm[e] / mx : 0.0;
        unsigned long long hi = dist_acc[2 * (off + e)], lo = dist_acc[2 * (off + e) + 1];
        const bool bad = hi & PS_POISON;
        hi += lo >> 32;                          // < 2^53: the conversion below is exact
        lo &= 0xFFFFFFFFull;
        // hi * 2^32 and lo are exact doubles: their sum rounds the exact fixed-point total once
        const double v = bad ? __builtin_nan("") : ((double)hi * 0x1p32 + (double)lo) * 0x1p-52;
        emp[off + e] = v;
        dist_norm[off + e] = mx != 0.0 ? v / mx : 0.0;
    }
    if (j == 0) {
        diag_mean[pair] = np_pairwise_sum(sh_diag, C, 1) / (double)C;
        double mn = sh_diag[0];
        for (int k = 1; k < C; ++k) mn = sh_diag[k] < mn ? sh_diag[k] : mn;
        diag_min[pair] = mn;
    }
}

int launch_classify(const float* cc, int64_t n_cells, int C, int32_t* labels, hipStream_t s) {
    const int blocks = (int)imin64(2048, cdiv64(n_cells, 4));
    hipLaunchKernelGGL(k_classify, dim3(blocks), dim3(256), 0, s, cc, n_cells, C, labels);
    HIP_LAUNCH_CHECK("k_classify");
    return 0;
}

int launch_confmat(const int32_t* labels, int A, int64_t n, int C, int64_t* counts, hipStream_t s) {
    if (A < 2) return 0;
    const int npairs = A * (A - 1) / 2;
    const size_t shm = (size_t)npairs * C * C * sizeof(unsigned int);
    const bool lds = shm <= 64 * 1024;                      // 92 x 92 categories: one pair 34 KB (A = 2)
    // few, fat workgroups when counting in LDS (each flushes its whole histogram), many thin ones otherwise
    const int blocks = lds ? (int)imin64(32, cdiv64(n, 1024)) : (int)imin64(1024, cdiv64(n, 256));
    hipLaunchKernelGGL(k_confmat, dim3(blocks > 0 ? blocks : 1), dim3(256), lds ? shm : 0, s, labels, A, n, C,
                       reinterpret_cast<unsigned long long*>(counts), lds ? npairs : 0);
    HIP_LAUNCH_CHECK("k_confmat");
    return 0;
}

int launch_consensus(const int64_t* counts, int npairs, int C, double* cm_norm, double* consensus, hipStream_t s) {
    hipLaunchKernelGGL(k_consensus, dim3(npairs), dim3(128), 0, s, reinterpret_cast<const unsigned long long*>(counts), C,
                       cm_norm, consensus);
    HIP_LAUNCH_CHECK("k_consensus");
    return 0;
}

// path: -1 the rule below, 0 the LDS histogram, 1 the wave-combined atomics (both are kept callable: tests and the
// timing tool run each on the same input).  pairs: host, [n_pairs][4], validated by the caller.
int launch_pair_stats(const int32_t* labels, const float* probs, int64_t n, int C, const int32_t* pairs, int n_pairs,
                      int64_t* counts, int64_t* dist_acc, int path, hipStream_t s) {
    const size_t shm = (size_t)C * C * 12;
    // PS_LDS_MAX_C = 116: 116^2 x 12 B = 161 472 B is the last histogram below the 163 840 B of a CU's LDS.  Measured at
    // C = 92, 22 365 cells, 15 pairs (profiles/evals2_time.json): histogram 28 / 27 / 45 us, wave-combined 34 / 26 / 179 us
    // for few labels / identical arms / labels spread over all categories: the histogram runs wherever it fits.
    const bool fits = C <= PS_LDS_MAX_C;
    if (path == 0 && !fits) { set_error("pair_stats: no LDS histogram for C = %d > %d", C, PS_LDS_MAX_C); return MMVAE_E_UNSUPPORTED; }
    const bool lds = path < 0 ? fits : path == 0;
    if (lds && shm > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_pair_stats<true>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm);
        if (e != hipSuccess) {
            set_error("pair_stats: %zu bytes of dynamic LDS refused: %s", shm, hipGetErrorString(e));
            return MMVAE_E_LAUNCH;
        }
    }
    const int64_t chunks = cdiv64(n, PS_CHUNK);
    for (int p0 = 0; p0 < n_pairs; p0 += PS_MAX_PAIRS) {
        const int np = n_pairs - p0 < PS_MAX_PAIRS ? n_pairs - p0 : PS_MAX_PAIRS;
        PairTab tab;
        for (int p = 0; p < np; ++p) {
            const int32_t* q = pairs + 4 * (int64_t)(p0 + p);
            tab.p[p] = (uint32_t)q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16 | (uint32_t)q[3] << 24;
        }
        for (int p = np; p < PS_MAX_PAIRS; ++p) tab.p[p] = 0u;
        auto* cnt = reinterpret_cast<unsigned long long*>(counts);
        auto* acc = reinterpret_cast<unsigned long long*>(dist_acc);
        if (lds) hipLaunchKernelGGL(k_pair_stats<true>, dim3((unsigned)chunks, np), dim3(256), shm, s, labels, probs, n, C, tab, p0, cnt, acc);
        else hipLaunchKernelGGL(k_pair_stats<false>, dim3((unsigned)chunks, np), dim3(256), 0, s, labels, probs, n, C, tab, p0, cnt, acc);
        HIP_LAUNCH_CHECK("k_pair_stats");
    }
    return 0;
}

int launch_pair_finish(const int64_t* counts, const int64_t* dist_acc, int n_pairs, int C, double* cm_norm, double* emp,
                       double* dist_norm, double* diag_mean, double* diag_min, hipStream_t s) {
    hipLaunchKernelGGL(k_pair_finish, dim3(n_pairs), dim3(128), 0, s, reinterpret_cast<const unsigned long long*>(counts),
                       reinterpret_cast<const unsigned long long*>(dist_acc), C, cm_norm, emp, dist_norm, diag_mean, diag_min);
    HIP_LAUNCH_CHECK("k_pair_finish");
    return 0;
}

}  // namespace mmvae

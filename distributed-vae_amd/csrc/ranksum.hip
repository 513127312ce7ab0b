// Wilcoxon rank sums of every gene, each group of cells against the rest.
//
// For every gene the n selected cells' values are ranked among themselves (ties: the average rank) and the ranks of each
// group's cells are added.  Twice a mid-rank is the integer lo + hi + 1 (lo values below, hi values not above), so the rank
// sums, the tie term and the counts are integers and exact; only the groups' value sums are floating point, added in a fixed
// order.  Two kernels per chunk of RS_CHUNK genes:
//   k_rs_stage  transposes the chunk through LDS into a gene-major staging copy [genes of the chunk][n] (the row map is
//               applied here, once), so that a gene's column is contiguous for the two passes that follow;
//   k_rs_rank   one workgroup a gene: the n values become order-preserving 32-bit keys (rs_key), padded to a power of two P
//               with keys above every value, and are sorted in LDS (rs_sort: a bitonic network).  Every cell then searches its
//               own key in the sorted array for lo and hi.  A group of at most RS_BIG cells is reduced by one wave, a larger
//               one by the whole workgroup (wave partials added in wave order): lanes in a fixed butterfly, so the sums are
//               the same bits on every run (rs_walk).  A cell tied with t - 1 others adds t^2 - 1 to the tie term: a run of t
//               equal values adds t (t^2 - 1) = t^3 - t.
// No floating-point atomics, no communication between workgroups; integer LDS atomics collect the tie term and the list of
// large groups.  NaN is not checked for: a NaN's key is ordered somewhere and the gene's results are then unspecified (never an
// access outside the buffers: every search stays inside [0, n]).  Offsets that do not ascend from 0 to n are the caller's
// contract (include/mmvae.h): the tie term adds up the cells that lie in some group, and more than RS_MAX_N / RS_BIG groups
// above RS_BIG cells, which ascending offsets cannot hold, leave the groups past that number unwritten.
// Above RS_MAX_N cells, up to RSB_MAX_N: the blocked path at the end of this file (k_rsb_sort, k_rsb_rank, k_rsb_reduce), which
// sorts with the same rs_sort and adds with the same rs_walk, handed its own way to find the large groups (a plain walk, no
// list and no cap); the launchers share rs_allow_lds and rs_chunks.
#include "common.hpp"

namespace mmvae {

// grid ceil(n / 64) x ceil(gc / 64), 256 threads: a tile of 64 cells x 64 genes, read along the rows (64 consecutive genes of
// a row: 256 contiguous bytes), written along the cells.  stage [gc][n].
__global__ __launch_bounds__(256) void k_rs_stage(const float* __restrict__ x, int64_t ld, int64_t n_total,
                                                  const int64_t* __restrict__ rows, int n, int g0, int gc,
                                                  float* __restrict__ stage) {
    __shared__ float tile[64][65];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int c0 = blockIdx.x * 64, q0 = blockIdx.y * 64;
    for (int r = ty; r < 64; r += 4) {
        float v = 0.f;
        if (c0 + r < n && q0 + tx < gc) v = x[src_row(rows, c0 + r, n_total) * ld + g0 + q0 + tx];
        tile[r][tx] = v;
    }
    __syncthreads();
    for (int q = ty; q < 64; q += 4)
        if (q0 + q < gc && c0 + tx < n) stage[(int64_t)(q0 + q) * n + c0 + tx] = tile[tx][q];
}

// The sort both paths share: the len values of col become keys, padded to the power of two P with keys above every value, and
// are sorted in place by a bitonic network.  Every thread of the workgroup; ends on a barrier, which also publishes whatever
// the caller wrote to LDS before the call.
__device__ inline void rs_sort(const float* __restrict__ col, int len, int P, uint32_t* keys) {
    const int T = blockDim.x, t = threadIdx.x;
    for (int i = t; i < P; i += T) keys[i] = i < len ? rs_key(col[i]) : 0xFFFFFFFFu;
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int idx = t; idx < (P >> 1); idx += T) {
                const int i = ((idx & ~(j - 1)) << 1) | (idx & (j - 1)), l = i | j;
                const uint32_t a = keys[i], b = keys[l];
                if ((a > b) == ((i & k) == 0)) { keys[i] = b; keys[l] = a; }
            }
            __syncthreads();
        }
}

struct RsAcc { long long r2, tie; int np; double s; };

// The group walk both paths share, every thread of the workgroup.  off: the G + 1 offsets in LDS, clamped to [0, n]; a range
// that runs backwards is empty.  cell(i, a) adds cell i of the gene to a: twice its mid-rank, x > eps, its value and, where
// the caller counts ties here, t^2 - 1.  A group of at most RS_BIG cells is reduced by one wave (wave w: the groups w, w + W,
// ...); big(body) calls body(g) for the larger groups g, the same ones in the same order in every thread, and each is reduced
// by the whole workgroup, its wave partials added in wave order; lanes in a fixed butterfly.  Writes rank_sum2, n_pos and sum
// of every group that is visited; returns the thread's share of the tie counts.
template <class Cell, class Big>
__device__ inline long long rs_walk(const int* off, int G, int gene, int D, Cell cell, Big big, int64_t* __restrict__ rank_sum2,
                                    int64_t* __restrict__ n_pos, double* __restrict__ sum) {
    __shared__ long long w_r2[RS_THREADS / 64];
    __shared__ double w_s[RS_THREADS / 64];
    __shared__ int w_np[RS_THREADS / 64];
    const int T = blockDim.x, t = threadIdx.x, lane = t & 63, w = t >> 6, W = T >> 6;
    long long tie = 0;
    auto cells = [&](int c0, int c1, int first, int step) {                // the cells c0 + first, c0 + first + step, ... below c1
        RsAcc a{0, 0, 0, 0.0};
        for (int i = c0 + first; i < c1; i += step) cell(i, a);
        tie += a.tie;
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            a.r2 += __shfl_xor(a.r2, m);
            a.np += __shfl_xor(a.np, m);
            a.s += __shfl_xor(a.s, m);
        }
        return a;
    };
    auto put = [&](int g, long long r2, int np, double s) {
        const int64_t o = (int64_t)g * D + gene;
        rank_sum2[o] = r2;
        n_pos[o] = np;
        sum[o] = s;
    };
    for (int g = w; g < G; g += W) {
        const int c0 = off[g], c1 = off[g + 1];
        if (c1 - c0 > RS_BIG) continue;
        const RsAcc a = cells(c0, c1, lane, 64);
        if (lane == 0) put(g, a.r2, a.np, a.s);
    }
    big([&](int g) {
        const RsAcc a = cells(off[g], off[g + 1], t, T);
        if (lane == 0) { w_r2[w] = a.r2; w_np[w] = a.np; w_s[w] = a.s; }
        __syncthreads();
        if (t == 0) {
            long long r2 = 0;
            int np = 0;
            double s = 0.0;
            for (int v = 0; v < W; ++v) { r2 += w_r2[v]; np += w_np[v]; s += w_s[v]; }
            put(g, r2, np, s);
        }
        __syncthreads();
    });
    return tie;
}

// grid gc workgroups of T = min(RS_THREADS, P / 2) threads; dynamic LDS: keys uint32 [P], then the group offsets int32 [G + 1]
// (each clamped to [0, n]; a range that runs backwards is empty).  col = stage + blockIdx.x * n; the outputs of gene g0 + blockIdx.x.
__global__ __launch_bounds__(RS_THREADS) void k_rs_rank(const float* __restrict__ stage, int n, int P,
                                                        const int64_t* __restrict__ offsets, int G, uint32_t eps_key, int g0, int D,
                                                        int64_t* __restrict__ rank_sum2, int64_t* __restrict__ tie_term,
                                                        int64_t* __restrict__ n_pos, double* __restrict__ sum) {
    extern __shared__ uint32_t rs_lds[];
    uint32_t* keys = rs_lds;
    int* off = reinterpret_cast<int*>(rs_lds + P);
    __shared__ unsigned long long tie_all;
    __shared__ int big[RS_MAX_N / RS_BIG], n_big;
    const int T = blockDim.x, t = threadIdx.x;
    const int gene = g0 + blockIdx.x;
    const float* col = stage + (int64_t)blockIdx.x * n;
    if (t == 0) { tie_all = 0; n_big = 0; }
    for (int g = t; g <= G; g += T) off[g] = (int)clamp64(offsets[g], 0, n);
    rs_sort(col, n, P, keys);
    // the groups above RS_BIG cells, in any order: each is reduced on its own
    for (int g = t; g < G; g += T)
        if (off[g + 1] - off[g] > RS_BIG) {                               // at most n / RS_BIG of them where the offsets ascend
            const int slot = atomicAdd(&n_big, 1);
            if (slot < RS_MAX_N / RS_BIG) big[slot] = g;
        }
    __syncthreads();
    long long tie = rs_walk(off, G, gene, D, [&](int i, RsAcc& a) {       // the cell searches its own key for lo and hi
        const float v = col[i];
        const uint32_t k = rs_key(v);
        int lo = 0, len = n;
        while (len > 0) {
            const int half = len >> 1;
            if (keys[lo + half] < k) { lo += half + 1; len -= half + 1; } else len = half;
        }
        int hi = lo;
        len = n - lo;
        while (len > 0) {
            const int half = len >> 1;
            if (keys[hi + half] <= k) { hi += half + 1; len -= half + 1; } else len = half;
        }
        const long long r = hi - lo;
        a.r2 += lo + hi + 1;
        a.tie += r * r - 1;
        a.np += k > eps_key ? 1 : 0;
        a.s += (double)v;
    }, [&](auto body) {                                                   // the listed ones (nb is the same in every thread)
        const int nb = n_big < RS_MAX_N / RS_BIG ? n_big : RS_MAX_N / RS_BIG;
        for (int b = 0; b < nb; ++b) body(big[b]);
    }, rank_sum2, n_pos, sum);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) tie += __shfl_xor(tie, m);
    if ((t & 63) == 0) atomicAdd(&tie_all, (unsigned long long)tie);
    __syncthreads();
    if (t == 0) tie_term[gene] = (int64_t)tie_all;
}

int rs_pow2(int64_t n) {
    int P = 128;
    while (P < n) P <<= 1;
    return P;
}

// more than 64 KiB of dynamic LDS needs the runtime's permission, for each kernel that is launched with it (also: or null)
static int rs_allow_lds(const char* who, size_t shm, const void* kernel, const void* also = nullptr) {
    if (shm <= 64 * 1024) return 0;
    hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm);
    if (e == hipSuccess && also) e = hipFuncSetAttribute(also, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm);
    if (e == hipSuccess) return 0;
    set_error("%s: %zu bytes of dynamic LDS refused: %s", who, shm, hipGetErrorString(e));
    return MMVAE_E_LAUNCH;
}

// the genes in chunks: k_rs_stage fills stage [gc][n] with the genes g0 .. g0 + gc - 1, then rest(g0, gc) launches what reads it
template <class Rest>
static int rs_chunks(const float* x, int64_t ld, int64_t n_total, int D, const int64_t* rows, int n, int chunk, float* stage,
                     hipStream_t st, Rest rest) {
    for (int64_t g0 = 0; g0 < D; g0 += chunk) {
        const int gc = D - g0 < chunk ? (int)(D - g0) : chunk;
        hipLaunchKernelGGL(k_rs_stage, dim3((unsigned)cdiv(n, 64), (unsigned)cdiv(gc, 64)), dim3(256), 0, st, x, ld, n_total, rows, n,
                           (int)g0, gc, stage);
        HIP_LAUNCH_CHECK("k_rs_stage");
        if (int rc = rest((int)g0, gc)) return rc;
    }
    return 0;
}

// ws: the staging copy float [min(D, RS_CHUNK)][n] (mmvae_rank_sum_workspace_bytes)
int launch_rank_sum(const float* x, int64_t ld, int64_t n_total, int D, const int64_t* rows, int n, const int64_t* offsets, int G,
                    float eps, void* ws, int64_t* rank_sum2, int64_t* tie_term, int64_t* n_pos, double* sum, hipStream_t st) {
    const int P = rs_pow2(n), T = P / 2 < RS_THREADS ? P / 2 : RS_THREADS;
    const size_t shm = rs_lds_bytes(n, G);
    if (int rc = rs_allow_lds("rank_sum", shm, reinterpret_cast<const void*>(&k_rs_rank))) return rc;
    float* stage = static_cast<float*>(ws);
    const uint32_t eps_key = rs_key(eps);
    return rs_chunks(x, ld, n_total, D, rows, n, RS_CHUNK, stage, st, [&](int g0, int gc) -> int {
        hipLaunchKernelGGL(k_rs_rank, dim3((unsigned)gc), dim3((unsigned)T), shm, st, stage, n, P, offsets, G, eps_key, g0, D,
                           rank_sum2, tie_term, n_pos, sum);
        HIP_LAUNCH_CHECK("k_rs_rank");
        return 0;
    });
}

// ---- the blocked path: up to RSB_MAX_N cells -----------------------------------------------------------
// The n cells of a gene, in the call's order, are cut into blocks of L (the last one shorter); every block is sorted on its
// own, and a cell's lo and hi are the sums over the blocks of its key's lower and upper bound in each: the integers of
// k_rs_rank.  k_rsb_reduce then adds the cells of every group with k_rs_rank's own walk, so that for n <= RS_MAX_N all four
// outputs are k_rs_rank's bits.

// grid ceil(n / L) x gc, min(RS_THREADS, L / 2) threads, dynamic LDS uint32 [L]: block blockIdx.x of gene blockIdx.y of the
// chunk.  Its len <= L keys, padded to the power of two P from 128 up that holds them, are sorted (rs_sort); the len real ones
// are written to sorted [gc][n] at the block's place.
__global__ __launch_bounds__(RS_THREADS) void k_rsb_sort(const float* __restrict__ stage, int n, int L, uint32_t* __restrict__ sorted) {
    extern __shared__ uint32_t rs_lds[];
    uint32_t* keys = rs_lds;
    const int T = blockDim.x, t = threadIdx.x;
    const int b0 = blockIdx.x * L;
    const int len = n - b0 < L ? n - b0 : L;
    int P = 128;
    while (P < len) P <<= 1;                                              // (P <= L: L is a power of two from 128 up)
    rs_sort(stage + (int64_t)blockIdx.y * n + b0, len, P, keys);
    uint32_t* out = sorted + (int64_t)blockIdx.y * n + b0;
    for (int i = t; i < len; i += T) out[i] = keys[i];
}

// The lower and the upper bound of RSB_CELLS keys in the sorted blk[0 .. len), len >= 1, added to lo and hi.  The number of
// steps depends on len alone, so the 2 RSB_CELLS searches of a thread advance together, their reads independent of one
// another; every read lies in [0, len) whatever the keys are.
__device__ inline void rsb_bounds(const uint32_t* blk, int len, const uint32_t (&k)[RSB_CELLS], int (&lo)[RSB_CELLS],
                                  int (&hi)[RSB_CELLS]) {
    int bl[RSB_CELLS], bh[RSB_CELLS];
#pragma unroll
    for (int j = 0; j < RSB_CELLS; ++j) bl[j] = bh[j] = 0;
    int m = len;
    while (m > 1) {
        const int half = m >> 1;
#pragma unroll
        for (int j = 0; j < RSB_CELLS; ++j) {
            const uint32_t a = blk[bl[j] + half - 1], b = blk[bh[j] + half - 1];
            bl[j] += a < k[j] ? half : 0;
            bh[j] += b <= k[j] ? half : 0;
        }
        m -= half;
    }
#pragma unroll
    for (int j = 0; j < RSB_CELLS; ++j) {
        lo[j] += bl[j] + (blk[bl[j]] < k[j] ? 1 : 0);
        hi[j] += bh[j] + (blk[bh[j]] <= k[j] ? 1 : 0);
    }
}

// grid ceil(n / RSB_TILE) x gc, RSB_THREADS threads: the cells tile0 + t + j RSB_THREADS, j < RSB_CELLS, of one gene keep
// their key, lo and hi in registers while the workgroup walks the sorted blocks.  STAGED: block b's keys are copied to LDS
// (dynamic, uint32 [L]) between two barriers and searched there; otherwise they are searched where they lie.  Writes
// lo + hi + 1 of every cell to twice [gc][n] and the tile's sum of t^2 - 1 to tie_part [gc][tiles].
template <bool STAGED>
__global__ __launch_bounds__(RSB_THREADS) void k_rsb_rank(const float* __restrict__ stage, const uint32_t* __restrict__ sorted, int n,
                                                          int L, uint32_t* __restrict__ twice, int64_t* __restrict__ tie_part) {
    extern __shared__ uint32_t rs_lds[];
    __shared__ long long w_tie[RSB_THREADS / 64];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int64_t base = (int64_t)blockIdx.y * n;
    const int c0 = blockIdx.x * RSB_TILE + t;
    uint32_t k[RSB_CELLS];
    int lo[RSB_CELLS], hi[RSB_CELLS];
#pragma unroll
    for (int j = 0; j < RSB_CELLS; ++j) {
        const int c = c0 + j * RSB_THREADS;
        k[j] = c < n ? rs_key(stage[base + c]) : 0u;                       // (a cell past n searches like any other; nothing of it is kept)
        lo[j] = hi[j] = 0;
    }
    for (int b0 = 0; b0 < n; b0 += L) {
        const int len = n - b0 < L ? n - b0 : L;
        const uint32_t* blk = sorted + base + b0;
        if (STAGED) {
            for (int i = t; i < len; i += RSB_THREADS) rs_lds[i] = blk[i];
            __syncthreads();
            rsb_bounds(rs_lds, len, k, lo, hi);
            __syncthreads();
        } else {
            rsb_bounds(blk, len, k, lo, hi);
        }
    }
    long long tie = 0;
#pragma unroll
    for (int j = 0; j < RSB_CELLS; ++j) {
        const int c = c0 + j * RSB_THREADS;
        if (c < n) {
            const long long r = hi[j] - lo[j];
            twice[base + c] = (uint32_t)(lo[j] + hi[j] + 1);
            tie += r * r - 1;
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) tie += __shfl_xor(tie, m);
    if (lane == 0) w_tie[w] = tie;
    __syncthreads();
    if (t == 0) {
        long long all = 0;
        for (int v = 0; v < RSB_THREADS / 64; ++v) all += w_tie[v];
        tie_part[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = all;
    }
}

// grid gc workgroups of T = min(RS_THREADS, rs_pow2(n) / 2) threads, k_rs_rank's number; dynamic LDS: the group offsets int32
// [G + 1], clamped to [0, n].  k_rs_rank's walk (rs_walk) with the search replaced by the stored lo + hi + 1: the same cells,
// lanes and waves in the same order; the tile partials of the tie term are added in tile order.
__global__ __launch_bounds__(RS_THREADS) void k_rsb_reduce(const float* __restrict__ stage, const uint32_t* __restrict__ twice,
                                                           const int64_t* __restrict__ tie_part, int n, int tiles,
                                                           const int64_t* __restrict__ offsets, int G, uint32_t eps_key, int g0, int D,
                                                           int64_t* __restrict__ rank_sum2, int64_t* __restrict__ tie_term,
                                                           int64_t* __restrict__ n_pos, double* __restrict__ sum) {
    extern __shared__ uint32_t rs_lds[];
    int* off = reinterpret_cast<int*>(rs_lds);
    const int T = blockDim.x, t = threadIdx.x;
    const int gene = g0 + blockIdx.x;
    const float* col = stage + (int64_t)blockIdx.x * n;
    const uint32_t* tw = twice + (int64_t)blockIdx.x * n;
    for (int g = t; g <= G; g += T) off[g] = (int)clamp64(offsets[g], 0, n);
    __syncthreads();
    rs_walk(off, G, gene, D, [&](int i, RsAcc& a) {
        const float v = col[i];
        a.r2 += tw[i];
        a.np += rs_key(v) > eps_key ? 1 : 0;
        a.s += (double)v;
    }, [&](auto body) {                                                   // every group above RS_BIG cells, in rising order
        for (int g = 0; g < G; ++g)
            if (off[g + 1] - off[g] > RS_BIG) body(g);
    }, rank_sum2, n_pos, sum);
    if (t == 0) {
        long long tie = 0;
        for (int i = 0; i < tiles; ++i) tie += tie_part[(int64_t)blockIdx.x * tiles + i];
        tie_term[gene] = tie;
    }
}

// ws (mmvae_rank_sum_blocked_workspace_bytes), gc = rsb_chunk(n, D): tie_part int64 [gc][tiles], then stage float, sorted
// uint32 and twice uint32, [gc][n] each.  form: RSB_FORM_AUTO the launcher's rule, else that form of k_rsb_rank; phases: 0 all
// four kernels, 1 .. 3 only the first so many of a chunk (a timing split: the outputs are then not written).
int launch_rank_sum_blocked(const float* x, int64_t ld, int64_t n_total, int D, const int64_t* rows, int n, const int64_t* offsets,
                            int G, float eps, int L, void* ws, int64_t* rank_sum2, int64_t* tie_term, int64_t* n_pos, double* sum,
                            int form, int phases, hipStream_t st) {
    if (L > rs_pow2(n)) L = rs_pow2(n);                                   // one block either way: no LDS beyond its keys
    if (form == RSB_FORM_AUTO) form = RSB_FORM_STAGED;
    const int P = rs_pow2(n), T = P / 2 < RS_THREADS ? P / 2 : RS_THREADS;
    const int Ts = L / 2 < RS_THREADS ? L / 2 : RS_THREADS;
    const int tiles = (int)cdiv(n, RSB_TILE), B = (int)cdiv(n, L), chunk = rsb_chunk(n, D);
    const size_t shm = (size_t)L * 4;
    if (int rc = rs_allow_lds("rank_sum_blocked", shm, reinterpret_cast<const void*>(&k_rsb_sort),
                              form == RSB_FORM_STAGED ? reinterpret_cast<const void*>(&k_rsb_rank<true>) : nullptr))
        return rc;
    int64_t* tie_part = static_cast<int64_t*>(ws);
    float* stage = reinterpret_cast<float*>(tie_part + (int64_t)chunk * tiles);
    uint32_t* sorted = reinterpret_cast<uint32_t*>(stage + (int64_t)chunk * n);
    uint32_t* twice = sorted + (int64_t)chunk * n;
    const uint32_t eps_key = rs_key(eps);
    return rs_chunks(x, ld, n_total, D, rows, n, chunk, stage, st, [&](int g0, int gc) -> int {
        if (phases == 1) return 0;
        hipLaunchKernelGGL(k_rsb_sort, dim3((unsigned)B, (unsigned)gc), dim3((unsigned)Ts), shm, st, stage, n, L, sorted);
        HIP_LAUNCH_CHECK("k_rsb_sort");
        if (phases == 2) return 0;
        if (form == RSB_FORM_STAGED)
            hipLaunchKernelGGL(k_rsb_rank<true>, dim3((unsigned)tiles, (unsigned)gc), dim3(RSB_THREADS), shm, st, stage, sorted, n, L,
                               twice, tie_part);
        else
            hipLaunchKernelGGL(k_rsb_rank<false>, dim3((unsigned)tiles, (unsigned)gc), dim3(RSB_THREADS), 0, st, stage, sorted, n, L,
                               twice, tie_part);
        HIP_LAUNCH_CHECK("k_rsb_rank");
        if (phases == 3) return 0;
        hipLaunchKernelGGL(k_rsb_reduce, dim3((unsigned)gc), dim3((unsigned)T), 4 * ((size_t)G + 1), st, stage, twice, tie_part, n, tiles,
                           offsets, G, eps_key, g0, D, rank_sum2, tie_term, n_pos, sum);
        HIP_LAUNCH_CHECK("k_rsb_reduce");
        return 0;
    });
}

}  // namespace mmvae

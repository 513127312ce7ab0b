// k nearest neighbours on the device.
//
// For every query point q_i the k admitted reference points r_j with the smallest squared distance, where reference j is
// admitted for query i iff no groups are given or rgroup[j] != qgroup[i] (no groups: a plain query; groups = arange on one
// set: the k-NN graph without the cell itself; groups = the fold of each cell: a test cell sees training cells only).  The
// squared distance is fp32 in difference form, k_sil_partial's own (pairdist.hpp states its order and its padding rule).
// Candidates are ordered by the 64-bit key (bits of the squared distance) << 32 | j: a sum of squares is never -0, so its
// bits order as unsigned integers, and j breaks ties.  The order is total, hence the k smallest keys of a query are a pure
// function of the inputs: the same bits on every run, whatever the cut of the work, whatever the other queries.  No atomics.
//
// Partition.  The reference columns are cut into segments of seg_cols; one workgroup of one wave owns (segment, tile of
// T = KNN_TILE = 64 queries), one thread per query (k_knn_partial).  A thread keeps its query in registers and its sorted list of k keys in
// LDS, slot s of thread t at lst[s T + t] (consecutive lanes, consecutive 8-byte words: no bank conflict), and the key of
// the list's last slot in a register: a candidate is compared with that register and only a smaller key touches the list
// (knn_insert: one branch-free pass over its slots).  The segment's columns are staged in LDS and read by all lanes at one
// address.  With one
// segment the lists are the result; with more, every (segment, query) list goes to the workspace, part[seg][slot][query],
// and k_knn_merge inserts a query's lists in segment order into one list, leaving a sorted list at its first key that
// does not enter.  The lists of a workgroup are k T keys of dynamic LDS, 32 KiB at k = 64.
//
// k_knn_votes: one thread per query, the labels of its valid neighbours in LDS, counted pair by pair (k^2 integer
// compares; no table of n_classes counters per thread).
#include "pairdist.hpp"

namespace mmvae {

constexpr uint64_t KNN_NONE = ~(uint64_t)0;     // an empty slot: above every key; its low half is idx = -1

// mine: the thread's slot 0; slot s at mine[s * T].  key < worst = mine[(k - 1) T] on entry.  With a the sorted list and
// a[-1] = 0, the list after the insertion is b[p] = max(a[p - 1], min(a[p], key)): a[p] where a[p] <= key, key at the first
// slot above it, a[p - 1] beyond.  No step depends on the one before, so the LDS reads of eight slots are in flight together,
// where a walk from the tail to the key's place waits for every read before it takes the next (measured: section 9t).  From
// the tail down, so that a chunk's a[p0 - 1] is read before the chunk below overwrites it.
__device__ inline void knn_insert(uint64_t* mine, int k, uint64_t key, uint64_t& worst) {
    constexpr int T = KNN_TILE;
    for (int p0 = (k - 1) & ~7; p0 >= 0; p0 -= 8) {
        uint64_t a[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            const int p = p0 - 1 + i;
            a[i] = p < 0 ? 0 : p < k ? mine[p * T] : KNN_NONE;
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const uint64_t lo = a[i + 1] < key ? a[i + 1] : key;
            if (p0 + i < k) mine[(p0 + i) * T] = a[i] > lo ? a[i] : lo;
        }
    }
    worst = mine[(k - 1) * T];
}

__device__ inline void knn_emit(const uint64_t* mine, int k, int* __restrict__ idx, float* __restrict__ dist2) {
    constexpr int T = KNN_TILE;
    for (int s = 0; s < k; ++s) {
        const uint64_t key = mine[s * T];
        const bool none = key == KNN_NONE;
        idx[s] = none ? -1 : (int)(uint32_t)key;
        dist2[s] = none ? __builtin_inff() : __builtin_bit_cast(float, (uint32_t)(key >> 32));
    }
}

// grid (segments, query tiles of T = KNN_TILE), T threads.  DV: float4 pieces per point, 4 DV >= d.
template <int DV>
__global__ __launch_bounds__(KNN_TILE) void k_knn_partial(const float* __restrict__ q, int64_t ldq, int64_t nq,
                                                     const float* __restrict__ r, int64_t ldr, int64_t nr, int d, int k,
                                                     const int* __restrict__ qgroup, const int* __restrict__ rgroup,
                                                     int64_t seg_cols, int64_t nseg, uint64_t* __restrict__ part,
                                                     int* __restrict__ idx, float* __restrict__ dist2) {
    constexpr int CT = KNN_LDS_FLOATS / (4 * DV);   // columns per pass (at most KNN_LDS_FLOATS / 4)
    __shared__ float4 cols[KNN_LDS_FLOATS / 4];
    __shared__ int grp[KNN_LDS_FLOATS / 4];
    extern __shared__ uint64_t lst[];               // k T keys (launch_knn)
    constexpr int T = KNN_TILE;
    const int tid = threadIdx.x;
    const int64_t seg = blockIdx.x;
    const int64_t c0 = seg * seg_cols, c1 = imin64(c0 + seg_cols, nr);
    const int64_t row = (int64_t)blockIdx.y * T + tid;
    const bool valid = row < nq;
    const bool grouped = qgroup != nullptr;
    const int qg = valid && grouped ? qgroup[row] : 0;
    float4 xi[DV];
    pd_load<DV>(q, ldq, row, d, valid, xi);
    uint64_t* mine = lst + tid;
    for (int s = 0; s < k; ++s) mine[s * T] = KNN_NONE;
    uint64_t worst = KNN_NONE;
    for (int64_t cb = c0; cb < c1; cb += CT) {
        const int m = (int)imin64(CT, c1 - cb);
        __syncthreads();                            // the pass before has been read
        pd_stage<DV, T>(r, ldr, cb, m, d, cols, tid);
        if (grouped)
            for (int c = tid; c < m; c += T) grp[c] = rgroup[cb + c];
        __syncthreads();
        if (!valid) continue;                       // (the barriers above are reached by every thread of every pass)
        auto dist = [&](int j) { return pd_dist2<DV>(xi, cols, j); };
        auto offer = [&](int j, float a) {
            const uint64_t key = ((uint64_t)__builtin_bit_cast(uint32_t, a) << 32) | (uint64_t)(uint32_t)(cb + j);
            if (key < worst && (!grouped || grp[j] != qg)) knn_insert(mine, k, key, worst);
        };
        int j = 0;
        if constexpr (DV <= 12) {                   // four independent distances at a time, where the registers hold them
            for (; j + 4 <= m; j += 4) {
                const float a0 = dist(j), a1 = dist(j + 1), a2 = dist(j + 2), a3 = dist(j + 3);
                offer(j, a0);
                offer(j + 1, a1);
                offer(j + 2, a2);
                offer(j + 3, a3);
            }
        }
        for (; j < m; ++j) offer(j, dist(j));
    }
    if (!valid) return;
    if (nseg == 1) {
        knn_emit(mine, k, idx + row * k, dist2 + row * k);
        return;
    }
    for (int s = 0; s < k; ++s) part[(seg * k + s) * nq + row] = mine[s * T];
}

// grid (query tiles of T = KNN_TILE), T threads: a query's nseg sorted lists, inserted in segment order.  A list is left
// at its first key that does not enter: every later one is larger still (and an empty slot is above every key).
__global__ __launch_bounds__(KNN_TILE) void k_knn_merge(const uint64_t* __restrict__ part, int64_t nseg, int64_t nq, int k,
                                                   int* __restrict__ idx, float* __restrict__ dist2) {
    extern __shared__ uint64_t lst[];               // k T keys (launch_knn)
    constexpr int T = KNN_TILE;
    const int tid = threadIdx.x;
    const int64_t row = (int64_t)blockIdx.x * T + tid;
    if (row >= nq) return;                          // (no barrier in this kernel)
    uint64_t* mine = lst + tid;
    for (int s = 0; s < k; ++s) mine[s * T] = KNN_NONE;
    uint64_t worst = KNN_NONE;
    for (int64_t seg = 0; seg < nseg; ++seg)
        for (int s = 0; s < k; ++s) {
            const uint64_t key = part[(seg * k + s) * nq + row];
            if (key >= worst) break;
            knn_insert(mine, k, key, worst);
        }
    knn_emit(mine, k, idx + row * k, dist2 + row * k);
}

// grid (query tiles of KNN_VOTE_TILE), KNN_VOTE_TILE threads, one query each.  A neighbour is valid where 0 <= idx < nr and
// its label lies in [0, n_classes).  pred: the label with the most valid neighbours, the smallest such label on ties, -1
// without a valid neighbour; top2 (optional) [nq, 2]: those votes and the most votes of another label; purity (optional,
// with qlabel): valid neighbours labelled qlabel[i] over valid neighbours, NaN without one.
__global__ __launch_bounds__(KNN_VOTE_TILE) void k_knn_votes(const int* __restrict__ idx, int64_t nq, int k,
                                                             const int* __restrict__ rlabel, int64_t nr, int n_classes,
                                                             const int* __restrict__ qlabel, int* __restrict__ pred,
                                                             double* __restrict__ purity, int* __restrict__ top2) {
    __shared__ int lab[KNN_MAX_K * KNN_VOTE_TILE];
    const int tid = threadIdx.x;
    const int64_t row = (int64_t)blockIdx.x * KNN_VOTE_TILE + tid;
    if (row >= nq) return;                          // (no barrier in this kernel)
    int* mine = lab + tid;
    int n_valid = 0;
    for (int s = 0; s < k; ++s) {
        const int j = idx[row * k + s];
        int l = -1;
        if (j >= 0 && j < nr) {
            l = rlabel[j];
            if (l < 0 || l >= n_classes) l = -1;
        }
        n_valid += l >= 0;
        mine[s * KNN_VOTE_TILE] = l;
    }
    auto votes_of = [&](int l) {
        int c = 0;
        for (int b = 0; b < k; ++b) c += mine[b * KNN_VOTE_TILE] == l;
        return c;
    };
    int best = 0, best_l = -1;
    for (int a = 0; a < k; ++a) {
        const int l = mine[a * KNN_VOTE_TILE];
        if (l < 0) continue;
        const int c = votes_of(l);
        if (c > best || (c == best && l < best_l)) { best = c; best_l = l; }
    }
    pred[row] = best_l;
    if (top2) {
        int second = 0;
        for (int a = 0; a < k; ++a) {
            const int l = mine[a * KNN_VOTE_TILE];
            if (l < 0 || l == best_l) continue;
            const int c = votes_of(l);
            second = c > second ? c : second;
        }
        top2[2 * row] = best;
        top2[2 * row + 1] = second;
    }
    if (purity) {
        const int ql = qlabel[row];
        const int same = ql >= 0 ? votes_of(ql) : 0;
        purity[row] = n_valid ? (double)same / (double)n_valid : __builtin_nan("");
    }
}

// ws: part uint64 [nseg][k][nq] where nseg = ceil(nr / seg_cols) > 1; not read or written with one segment
int launch_knn(const float* q, int64_t ldq, int64_t nq, const float* r, int64_t ldr, int64_t nr, int d, int k, const int* qgroup,
               const int* rgroup, int64_t seg_cols, void* ws, int* idx, float* dist2, int phases, hipStream_t st) {
    constexpr int T = KNN_TILE;
    const size_t lds = (size_t)k * T * sizeof(uint64_t);      // the lists: 32 KiB at k = 64
    const int64_t nseg = cdiv64(nr, seg_cols);
    uint64_t* part = static_cast<uint64_t*>(ws);
    const dim3 grid((unsigned)nseg, (unsigned)cdiv64(nq, T)), block(T);
    if (phases != KNN_PHASE_MERGE) {
        if (int rc = pd_dispatch("knn", d, [&](auto dv) {
                hipLaunchKernelGGL(k_knn_partial<decltype(dv)::value>, grid, block, lds, st, q, ldq, nq, r, ldr, nr, d, k, qgroup,
                                   rgroup, seg_cols, nseg, part, idx, dist2);
            }))
            return rc;
        HIP_LAUNCH_CHECK("k_knn_partial");
    }
    if (nseg > 1 && phases != KNN_PHASE_PARTIAL) {
        hipLaunchKernelGGL(k_knn_merge, dim3((unsigned)cdiv64(nq, T)), block, lds, st, part, nseg, nq, k, idx, dist2);
        HIP_LAUNCH_CHECK("k_knn_merge");
    }
    return 0;
}

int launch_knn_votes(const int* idx, int64_t nq, int k, const int* rlabel, int64_t nr, int n_classes, const int* qlabel, int* pred,
                     double* purity, int* top2, hipStream_t st) {
    hipLaunchKernelGGL(k_knn_votes, dim3((unsigned)cdiv64(nq, KNN_VOTE_TILE)), dim3(KNN_VOTE_TILE), 0, st, idx, nq, k, rlabel, nr,
                       n_classes, qlabel, pred, purity, top2);
    HIP_LAUNCH_CHECK("k_knn_votes");
    return 0;
}

}  // namespace mmvae

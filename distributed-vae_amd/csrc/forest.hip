// Random forest on 256-bin features (the contract is stated in include/mmvae.h).
//
// The reference's RF_classifier (mmidas/utils/cluster_analysis.py) fits sklearn's default forest to every fold of a k-fold
// split and scores the held-out cells.  On features quantised to 256 rank bins a tree is integer work: per node and feature a
// class x bin histogram in LDS, a prefix along the bins, sum_k L_k^2 and sum_k R_k^2 in uint64 and one fp64 quotient pair per
// candidate bin.  k_rf_train_rows lists every fold's training rows in ascending order; k_rf_fit grows one tree a workgroup
// (bootstrap, then the nodes off a stack in the contract's order, the node's rows partitioned stably between two index lists);
// k_rf_predict walks a held-out row down the trees of its fold, one tree a lane, and counts hard votes.  The LDS atomics only
// add integers, every other sum has one owner and every arg-max a total order, so a tree is the same bits on every run and
// is the tree tests/forest_restatement.py grows on the host.
#include "common.hpp"

namespace mmvae {

__device__ __forceinline__ int rf_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ uint64_t rf_shfl_xor_u64(uint64_t v, int mask) {
    const int lo = __shfl_xor((int)(uint32_t)v, mask, 64), hi = __shfl_xor((int)(uint32_t)(v >> 32), mask, 64);
    return ((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo;
}

// (a, b) is better than (a2, b2): a larger a, or the same a and a smaller b -- a total order, so a reduction under it gives
// the same pair in any order.  The scores' a is the bit pattern of a positive double, which orders as the double does.
__device__ __forceinline__ bool rf_better(uint64_t a, int b, uint64_t a2, int b2) { return a > a2 || (a == a2 && b < b2); }

// The best pair of the workgroup (RF_THREADS threads), in every thread.  red_a / red_b: one slot a wave; the caller leaves
// them alone until its next barrier.
__device__ inline void rf_block_best(uint64_t& a, int& b, uint64_t* red_a, int* red_b) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const uint64_t a2 = rf_shfl_xor_u64(a, m);
        const int b2 = __shfl_xor(b, m, 64);
        if (rf_better(a2, b2, a, b)) { a = a2; b = b2; }
    }
    const int wave = threadIdx.x >> 6;
    __syncthreads();                                // the slots' last readers are done
    if ((threadIdx.x & 63) == 0) { red_a[wave] = a; red_b[wave] = b; }
    __syncthreads();
    a = red_a[0];
    b = red_b[0];
#pragma unroll
    for (int w = 1; w < RF_THREADS / 64; ++w)
        if (rf_better(red_a[w], red_b[w], a, b)) { a = red_a[w]; b = red_b[w]; }
}

// train [F][n]: the rows whose fold is not f, ascending; nf [F] their number.  One workgroup a fold.
__global__ __launch_bounds__(RF_THREADS) void k_rf_train_rows(const int* __restrict__ fold, int n, int* __restrict__ train,
                                                              int* __restrict__ nf) {
    __shared__ int wcount[RF_THREADS / 64];
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int* out = train + (int64_t)f * n;
    int running = 0;
    for (int i0 = 0; i0 < n; i0 += RF_THREADS) {
        const int i = i0 + tid;
        const bool keep = i < n && fold[i] != f;
        const uint64_t mask = __ballot(keep);
        if (lane == 0) wcount[wave] = __popcll(mask);
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < RF_THREADS / 64; ++w) {
            const int c = wcount[w];
            before += w < wave ? c : 0;
            all += c;
        }
        if (keep) out[running + before + __popcll(mask & (((uint64_t)1 << lane) - 1))] = i;
        running += all;
        __syncthreads();
    }
    if (tid == 0) nf[f] = running;
}

// One workgroup grows tree g = g0 + blockIdx.x of fold f = g / T.  Its slices of the workspace: nodes int4 [cap], stack
// int4 [n] (node, first, last + 1, list), lists int [2][n].  Dynamic LDS: hist uint32 [kp][256] of the node's kp present
// classes (at most K), then the waves' partial sums per bin (uint64 [4][256] twice, uint32 [4][256]) and nL uint32 [256].
// A lane of the scan owns four consecutive bins, a wave every fourth present class: a class row is one 16-byte LDS read a
// lane, conflict-free, and the prefix along the bins a wave scan of the lanes' sums.
__global__ __launch_bounds__(RF_THREADS) void k_rf_fit(const uint8_t* __restrict__ bins, int64_t ld, int n, int d,
                                                       const int* __restrict__ codes, int K, int T, int mtry, uint32_t k0,
                                                       uint32_t k1, int g0, const int* __restrict__ train,
                                                       const int* __restrict__ nf, int4* __restrict__ nodes_all,
                                                       int4* __restrict__ stack_all, int* __restrict__ lists_all,
                                                       int* __restrict__ count) {
    extern __shared__ uint32_t rf_lds[];
    constexpr int NW = RF_THREADS / 64;
    uint32_t* hist = rf_lds;
    uint64_t* pSL2 = reinterpret_cast<uint64_t*>(hist + K * RF_BINS);        // (K 1024 bytes: 8-byte aligned)
    uint64_t* pSR2 = pSL2 + NW * RF_BINS;
    uint32_t* pnL = reinterpret_cast<uint32_t*>(pSR2 + NW * RF_BINS);
    uint32_t* nLs = pnL + NW * RF_BINS;
    __shared__ uint32_t tot[RF_MAX_K];              // the node's rows of every class
    __shared__ int cls[RF_MAX_K];                   // its present classes, ascending
    __shared__ int clsmap[RF_MAX_K];                // class -> index in cls
    __shared__ int perm[RF_MAX_D];
    __shared__ uint64_t red_a[NW];
    __shared__ int red_b[NW];
    __shared__ int wcl[NW], wcr[NW];
    __shared__ int sh_bhi;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = g0 + blockIdx.x, f = g / T;
    const int cap = 2 * n;
    int4* nodes = nodes_all + (int64_t)blockIdx.x * cap;
    int4* stk = stack_all + (int64_t)blockIdx.x * n;
    int* listA = lists_all + (int64_t)blockIdx.x * 2 * n;
    int* listB = listA + n;
    const int* tr = train + (int64_t)f * n;
    const int m0 = rf_clampi(nf[f], 0, n);

    // the bootstrap: draw 4 i + j is word j of the call with counter (i, g, 0, 0)
    for (int i = tid; i < (m0 + 3) / 4; i += RF_THREADS) {
        const u32x4 r = philox4x32((uint32_t)i, (uint32_t)g, 0u, 0u, k0, k1);
        const uint32_t u[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (4 * i + j < m0) listA[4 * i + j] = tr[(int)(((uint64_t)u[j] * (uint64_t)m0) >> 32)];
    }
    if (tid == 0) stk[0] = make_int4(0, 0, m0, 0);
    int sp = 1, n_nodes = 1;
    __syncthreads();

    while (sp > 0) {
        const int4 e = stk[--sp];                   // the same entry in every thread
        const int node = e.x, lo = e.y, hi = e.z, m = hi - lo;
        const int* src = e.w ? listB : listA;
        int* dst = e.w ? listA : listB;

        // the class counts, the present classes in order, the majority (the lowest code on ties)
        for (int k = tid; k < K; k += RF_THREADS) tot[k] = 0;
        __syncthreads();
        for (int i = lo + tid; i < hi; i += RF_THREADS) atomicAdd(&tot[rf_clampi(codes[src[i]], 0, K - 1)], 1u);
        __syncthreads();
        const uint32_t mine = tid < K ? tot[tid] : 0u;                      // K <= RF_MAX_K = 128: waves 0 and 1
        const uint64_t present = __ballot(mine > 0);
        if (lane == 0) wcl[wave] = __popcll(present);
        uint64_t ma = mine;
        int mb = tid;
        rf_block_best(ma, mb, red_a, red_b);        // (its barriers publish wcl)
        const int majority = mb;
        const int kp = wcl[0] + wcl[1];
        if (mine > 0) {
            const int at = (wave ? wcl[0] : 0) + __popcll(present & (((uint64_t)1 << lane) - 1));
            cls[at] = tid;
            clsmap[tid] = at;
        }
        for (int j = tid; j < d; j += RF_THREADS) perm[j] = j;

        uint64_t best_a = 0;                        // the bits of the best score so far; 0: no candidate yet
        int best_f = 0, best_lo = 0, best_hi = 0, best_nl = 0;
        const bool can_split = kp > 1 && n_nodes + 2 <= cap && sp + 2 <= n;
        for (int s = 0; can_split && s < d; ++s) {
            __syncthreads();                        // perm, cls, clsmap written; the last feature's LDS reads done
            if (tid == 0) {                         // step s of the lazy Fisher-Yates: draw s is word s & 3 of call s >> 2
                const u32x4 r = philox4x32((uint32_t)(s >> 2), (uint32_t)g, (uint32_t)node, 1u, k0, k1);
                const uint32_t w[4] = {r.x, r.y, r.z, r.w};
                const int j = s + (int)(((uint64_t)w[s & 3] * (uint64_t)(d - s)) >> 32);
                const int t = perm[s];
                perm[s] = perm[j];
                perm[j] = t;
                sh_bhi = RF_BINS;
            }
            for (int idx = tid; idx < kp * (RF_BINS / 4); idx += RF_THREADS)
                reinterpret_cast<uint4*>(hist)[idx] = make_uint4(0u, 0u, 0u, 0u);
            __syncthreads();
            const int feat = perm[s];
            for (int i = lo + tid; i < hi; i += RF_THREADS) {
                const int r = src[i];
                const int kl = clsmap[rf_clampi(codes[r], 0, K - 1)];
                atomicAdd(&hist[kl * RF_BINS + bins[(int64_t)r * ld + feat]], 1u);
            }
            __syncthreads();
            uint64_t sl2[4] = {0, 0, 0, 0}, sr2[4] = {0, 0, 0, 0};
            uint32_t nl[4] = {0, 0, 0, 0};
            for (int kl = wave; kl < kp; kl += NW) {
                const uint4 h = reinterpret_cast<const uint4*>(hist + kl * RF_BINS)[lane];
                uint32_t p[4];
                p[0] = h.x;
                p[1] = p[0] + h.y;
                p[2] = p[1] + h.z;
                p[3] = p[2] + h.w;
                uint32_t incl = p[3];               // inclusive scan of the lanes' sums
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    const uint32_t up = (uint32_t)__shfl_up((int)incl, off, 64);
                    if (lane >= off) incl += up;
                }
                const uint32_t before = incl - p[3], tk = tot[cls[kl]];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint32_t L = before + p[j], R = tk - L;
                    sl2[j] += (uint64_t)L * L;
                    sr2[j] += (uint64_t)R * R;
                    nl[j] += L;
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                pSL2[wave * RF_BINS + 4 * lane + j] = sl2[j];
                pSR2[wave * RF_BINS + 4 * lane + j] = sr2[j];
                pnL[wave * RF_BINS + 4 * lane + j] = nl[j];
            }
            __syncthreads();
            uint64_t SL2 = 0, SR2 = 0;              // thread b = tid: bin b
            uint32_t nL = 0;
#pragma unroll
            for (int w = 0; w < NW; ++w) {
                SL2 += pSL2[w * RF_BINS + tid];
                SR2 += pSR2[w * RF_BINS + tid];
                nL += pnL[w * RF_BINS + tid];
            }
            nLs[tid] = nL;
            __syncthreads();
            const bool occupied = nL > (tid ? nLs[tid - 1] : 0u);
            uint64_t a = 0;
            int b = tid;
            if (occupied && nL < (uint32_t)m) {     // a later bin is occupied too: a candidate
                const double left = __ddiv_rn((double)SL2, (double)nL);
                const double right = __ddiv_rn((double)SR2, (double)((uint32_t)m - nL));
                a = (uint64_t)__double_as_longlong(__dadd_rn(left, right));
            }
            rf_block_best(a, b, red_a, red_b);
            if (a > best_a) {                       // strictly larger: the first best in visiting order stands
                if (occupied && tid > b) atomicMin(&sh_bhi, tid);
                __syncthreads();
                best_a = a;
                best_f = feat;
                best_lo = b;
                best_hi = sh_bhi;
                best_nl = (int)nLs[b];
            }
            if (s + 1 >= mtry && best_a != 0) break;
        }

        if (best_a == 0) {                          // a leaf: pure, or no feature with two occupied bins
            if (tid == 0) nodes[node] = make_int4(-1, majority, 0, m);
            __syncthreads();                        // tot, wcl and the lists before the next node
            continue;
        }
        const int thr = (best_lo + best_hi) >> 1, left = n_nodes;
        n_nodes += 2;
        // the stable partition: the rows with bin <= thr to dst[lo ..], the others to dst[lo + best_nl ..], both in order
        int run_l = lo, run_r = lo + best_nl;
        for (int i0 = lo; i0 < hi; i0 += RF_THREADS) {
            const int i = i0 + tid;
            const bool valid = i < hi;
            const int r = valid ? src[i] : 0;
            const bool go_l = valid && bins[(int64_t)r * ld + best_f] <= thr;
            const bool go_r = valid && !go_l;
            const uint64_t ml = __ballot(go_l), mr = __ballot(go_r);
            __syncthreads();                        // the counts of the chunk before have been read
            if (lane == 0) { wcl[wave] = __popcll(ml); wcr[wave] = __popcll(mr); }
            __syncthreads();
            int bl = 0, br = 0, al = 0, ar = 0;
#pragma unroll
            for (int w = 0; w < NW; ++w) {
                bl += w < wave ? wcl[w] : 0;
                br += w < wave ? wcr[w] : 0;
                al += wcl[w];
                ar += wcr[w];
            }
            const uint64_t below = ((uint64_t)1 << lane) - 1;
            if (go_l) dst[rf_clampi(run_l + bl + __popcll(ml & below), lo, hi - 1)] = r;
            if (go_r) dst[rf_clampi(run_r + br + __popcll(mr & below), lo, hi - 1)] = r;
            run_l += al;
            run_r += ar;
        }
        if (tid == 0) {
            nodes[node] = make_int4(best_f, thr, left, m);
            stk[sp] = make_int4(left + 1, lo + best_nl, hi, e.w ^ 1);       // right first: left leaves the stack first
            stk[sp + 1] = make_int4(left, lo, lo + best_nl, e.w ^ 1);
        }
        sp += 2;
        __syncthreads();
    }
    if (tid == 0) count[blockIdx.x] = n_nodes;
}

// The node tables of a chunk's trees to the caller's arrays, one workgroup a tree: the count and the count's nodes.  The rows
// of the workspace table past the count were never written by k_rf_fit and stay where they are: entries past the count are
// not written (include/mmvae.h).
__global__ __launch_bounds__(RF_THREADS) void k_rf_copy_trees(const int4* __restrict__ nodes_all, const int* __restrict__ count, int cap,
                                                              int* __restrict__ out_count, int* __restrict__ out_nodes) {
    const int g = blockIdx.x;
    const int c = count[g];
    if (threadIdx.x == 0) out_count[g] = c;
    const int m = rf_clampi(c, 0, cap);
    const int* src = reinterpret_cast<const int*>(nodes_all + (int64_t)g * cap);
    int* dst = out_nodes + (int64_t)g * cap * 4;       // (int by int: the caller's array need not be 16-byte aligned)
    for (int j = threadIdx.x; j < 4 * m; j += RF_THREADS) dst[j] = src[j];
}

// One wave a held-out row, one tree a lane: the trees g0 .. g0 + gc - 1 of the workspace that belong to the row's fold vote,
// the votes add to votes [n][K] (first: they start at zero) and, with last, the arg-max (the lowest code on ties), its count
// and the largest count among the other classes are written.  fold values are clamped to [0, F - 1], a walk takes at most
// count[tree] steps and stays inside the tree's cap nodes.
__global__ __launch_bounds__(RF_THREADS) void k_rf_predict(const uint8_t* __restrict__ bins, int64_t ld, int n, int d,
                                                           const int* __restrict__ fold, int F, int K, int T, int g0, int gc,
                                                           const int4* __restrict__ nodes_all, const int* __restrict__ count,
                                                           int first, int last, int* __restrict__ votes, int* __restrict__ label,
                                                           int* __restrict__ best, int* __restrict__ second) {
    constexpr int NW = RF_THREADS / 64;
    __shared__ int vh[NW][RF_MAX_K];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t row64 = (int64_t)blockIdx.x * NW + wave;
    const bool valid = row64 < n;
    const int row = valid ? (int)row64 : n - 1;
    const int cap = 2 * n;
    for (int k = lane; k < K; k += 64) vh[wave][k] = 0;
    __syncthreads();
    const int f = rf_clampi(fold[row], 0, F - 1);
    const int t0 = f * T > g0 ? f * T : g0, t1 = (f + 1) * T < g0 + gc ? (f + 1) * T : g0 + gc;
    const uint8_t* x = bins + (int64_t)row * ld;
    for (int g = t0 + lane; g < t1; g += 64) {
        const int4* nt = nodes_all + (int64_t)(g - g0) * cap;
        const int steps = rf_clampi(count[g - g0], 1, cap);
        int at = 0, c = 0;
        for (int s = 0; s < steps; ++s) {
            const int4 e = nt[at];
            if (e.x < 0) { c = e.y; break; }
            at = rf_clampi(e.z + (x[e.x < d ? e.x : d - 1] <= e.y ? 0 : 1), 0, cap - 1);
        }
        atomicAdd(&vh[wave][rf_clampi(c, 0, K - 1)], 1);
    }
    __syncthreads();
    uint64_t a = 0;
    int b = K;
    for (int k = lane; k < K; k += 64) {
        const int v = vh[wave][k] + (first ? 0 : votes[(int64_t)row * K + k]);
        vh[wave][k] = v;
        if (valid) votes[(int64_t)row * K + k] = v;
        if (rf_better((uint64_t)v, k, a, b)) { a = (uint64_t)v; b = k; }
    }
    if (!last) return;                              // (the whole workgroup)
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const uint64_t a2 = rf_shfl_xor_u64(a, m);
        const int b2 = __shfl_xor(b, m, 64);
        if (rf_better(a2, b2, a, b)) { a = a2; b = b2; }
    }
    int runner = 0;
    for (int k = lane; k < K; k += 64)
        if (k != b && vh[wave][k] > runner) runner = vh[wave][k];
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const int o = __shfl_xor(runner, m, 64);
        runner = o > runner ? o : runner;
    }
    if (valid && lane == 0) {
        label[row] = b;
        best[row] = (int)a;
        second[row] = runner;
    }
}

// the trees of one chunk of launches: as many as RF_CHUNK_BYTES of per-tree tables hold, at least one, at most all F T
int rf_chunk(int64_t n, int F, int T) {
    const int64_t per = RF_TREE_BYTES_PER_ROW * n + 4, all = (int64_t)F * T;
    const int64_t fit = RF_CHUNK_BYTES / per;
    return (int)(fit < 1 ? 1 : (fit > all ? all : fit));
}

// ws: nodes int4 [chunk][2 n], stack int4 [chunk][n], lists int [chunk][2][n], train int [F][n], votes int [n][K], count int
// [chunk], nf int [F] (mmvae_forest_workspace_bytes)
size_t rf_ws_bytes(int64_t n, int F, int K, int T) {
    const unsigned __int128 c = (unsigned __int128)rf_chunk(n, F, T), nn = (unsigned __int128)n;
    const unsigned __int128 b = c * (RF_TREE_BYTES_PER_ROW * nn + 4) + 4 * nn * (unsigned)F + 4 * nn * (unsigned)K + 4 * (unsigned)F;
    return bytes_or_0((b + 15) / 16 * 16);
}

static size_t rf_fit_lds(int K) { return (size_t)K * RF_BINS * 4 + (size_t)(RF_THREADS / 64) * RF_BINS * 20 + RF_BINS * 4; }

int launch_forest(const uint8_t* bins, int64_t ld, int64_t n, int d, const int* codes, const int* fold, int K, int F, int T,
                  int mtry, uint64_t seed, void* ws, int* label, int* best, int* second, int* votes, int* tree_count,
                  int* tree_nodes, hipStream_t st) {
    const int chunk = rf_chunk(n, F, T), G = F * T;
    int4* nodes = static_cast<int4*>(ws);
    int4* stack = nodes + (int64_t)chunk * 2 * n;
    int* lists = reinterpret_cast<int*>(stack + (int64_t)chunk * n);
    int* train = lists + (int64_t)chunk * 2 * n;
    int* ws_votes = train + (int64_t)F * n;
    int* count = ws_votes + n * K;
    int* nf = count + chunk;
    int* v = votes ? votes : ws_votes;
    const size_t shm = rf_fit_lds(K);
    if (shm > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_rf_fit), hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm);
        if (e != hipSuccess) {
            set_error("forest: %zu bytes of dynamic LDS refused: %s", shm, hipGetErrorString(e));
            return MMVAE_E_LAUNCH;
        }
    }
    hipLaunchKernelGGL(k_rf_train_rows, dim3((unsigned)F), dim3(RF_THREADS), 0, st, fold, (int)n, train, nf);
    HIP_LAUNCH_CHECK("k_rf_train_rows");
    for (int g0 = 0; g0 < G; g0 += chunk) {
        const int gc = G - g0 < chunk ? G - g0 : chunk;
        hipLaunchKernelGGL(k_rf_fit, dim3((unsigned)gc), dim3(RF_THREADS), shm, st, bins, ld, (int)n, d, codes, K, T, mtry,
                           (uint32_t)seed, (uint32_t)(seed >> 32), g0, train, nf, nodes, stack, lists, count);
        HIP_LAUNCH_CHECK("k_rf_fit");
        if (tree_count) {
            hipLaunchKernelGGL(k_rf_copy_trees, dim3((unsigned)gc), dim3(RF_THREADS), 0, st, nodes, count, (int)(2 * n), tree_count + g0,
                               tree_nodes + (int64_t)g0 * 2 * n * 4);
            HIP_LAUNCH_CHECK("k_rf_copy_trees");
        }
        hipLaunchKernelGGL(k_rf_predict, dim3((unsigned)cdiv64(n, RF_THREADS / 64)), dim3(RF_THREADS), 0, st, bins, ld, (int)n, d,
                           fold, F, K, T, g0, gc, nodes, count, g0 == 0 ? 1 : 0, g0 + gc == G ? 1 : 0, v, label, best, second);
        HIP_LAUNCH_CHECK("k_rf_predict");
    }
    return 0;
}

}  // namespace mmvae

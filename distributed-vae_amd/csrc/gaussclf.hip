// Gaussian classifiers on the device.
//
// The reference's clusterability analysis (mmidas/utils/cluster_analysis.py: QDA_classifier, LDA_classifier) fits, for every
// fold of a k-fold split, one Gaussian per cell type to the training cells and scores the held-out cells under each.  Two
// launches carry the dense part of that.  mmvae_group_moments: the first and second moments about one pivot of every
// (class, fold) group of cells in one pass -- the rows arrive ordered by group, are cut into segments of at most GC_SEG_ROWS
// that never cross a group boundary (k_segments, segments.hip: the scheme is described once, in common.hpp), a workgroup owns one segment and all d (d + 3) / 2 of
// its sums (k_gc_partial), and a last launch adds each group's segments in order (k_gc_finish).  Moments about one pivot are
// additive over groups, so the host forms every fold's training moments from them without a second pass.
// mmvae_gauss_scores: score(i, k) = c0[m, k] - |W_mk^T (x_i - mu_mk)|^2 / 2 of every cell under every class of the model m
// of its own fold, and the arg-max (k_gc_scores: 64 cells a workgroup, the classes split over its waves).  Everything is
// fp64 on fp32 points.  No atomics: every sum has one owner and a fixed order, so the results are the same bits on every
// run, a group's moments are those of a call on its rows alone, and a cell's scores do not depend on the cells beside it.
#include "common.hpp"

namespace mmvae {

// The first row of packed upper-triangle row i of a d x d matrix: i d - i (i - 1) / 2.
__device__ inline int gc_tri_row(int i, int d) { return i * (2 * d - i + 1) / 2; }

// One workgroup of 256 threads per segment.  The segment's rows are staged GC_ROW_CHUNK at a time in LDS as the fp64
// differences t = (double)x - (double)pivot with a column of ones behind them (row pitch d + 1), and thread t owns the sums
// q = t, t + 256, ...  of the Q = d + d (d + 1) / 2 of the segment: q < d is sum t_q (the product with the column of ones,
// exact), q >= d the pair (i, j), i <= j, of packed index q - d.  Every sum is one fma chain in row order, whatever the
// instance: DMAX (the largest d of the instance) only sizes the LDS tile and the registers, so the instances give the same
// bits.  part [segment][Q].
template <int DMAX>
__global__ __launch_bounds__(256) void k_gc_partial(const float* __restrict__ x, int64_t ld, int64_t n, int d,
                                                    const float* __restrict__ pivot, const int* __restrict__ gseg, int G,
                                                    const int64_t* __restrict__ seg_begin, double* __restrict__ part) {
    constexpr int NPT = (DMAX * (DMAX + 3) / 2 + 255) / 256;
    __shared__ double tile[GC_ROW_CHUNK * (DMAX + 1)];
    const int seg = blockIdx.x;
    if (seg >= gseg[G]) return;                     // the whole workgroup
    int64_t c0, c1;
    seg_range(seg_begin, seg, n, GC_SEG_ROWS, c0, c1);
    const int tid = threadIdx.x;
    const int Q = d * (d + 3) / 2, pitch = d + 1;
    int ia[NPT], ja[NPT];
    double acc[NPT];
#pragma unroll
    for (int e = 0; e < NPT; ++e) {
        const int q = tid + 256 * e;
        int i = d, j = d;                           // q >= Q: the ones column with itself; never written
        if (q < d) {
            i = q;
        } else if (q < Q) {
            const int p = q - d;
            const float b = (float)(2 * d + 1);
            i = (int)((b - __builtin_sqrtf(b * b - 8.f * (float)p)) * 0.5f);
            i = i < 0 ? 0 : (i > d - 1 ? d - 1 : i);
            while (i + 1 < d && gc_tri_row(i + 1, d) <= p) ++i;
            while (i > 0 && gc_tri_row(i, d) > p) --i;
            j = i + p - gc_tri_row(i, d);
            j = j > d - 1 ? d - 1 : j;
        }
        ia[e] = i;
        ja[e] = j;
        acc[e] = 0.0;
    }
    for (int64_t r0 = c0; r0 < c1; r0 += GC_ROW_CHUNK) {
        const int nr = (int)imin64(GC_ROW_CHUNK, c1 - r0);
        __syncthreads();                            // the chunk before this one has been read
        for (int idx = tid; idx < nr * pitch; idx += 256) {
            const int rr = idx / pitch, cc = idx - rr * pitch;
            tile[idx] = cc < d ? (double)x[(r0 + rr) * ld + cc] - (double)pivot[cc] : 1.0;
        }
        __syncthreads();
        for (int rr = 0; rr < nr; ++rr) {
            const double* t = tile + rr * pitch;
#pragma unroll
            for (int e = 0; e < NPT; ++e) acc[e] = __builtin_fma(t[ia[e]], t[ja[e]], acc[e]);
        }
    }
    double* base = part + (int64_t)seg * Q;
#pragma unroll
    for (int e = 0; e < NPT; ++e) {
        const int q = tid + 256 * e;
        if (q < Q) base[q] = acc[e];
    }
}

// One thread per (group, sum): the group's segments added in order.  s [G][d], M [G][d (d + 1) / 2].
__global__ __launch_bounds__(256) void k_gc_finish(const double* __restrict__ part, const int* __restrict__ gseg, int G,
                                                   int64_t nseg_max, int d, int tiles, double* __restrict__ s,
                                                   double* __restrict__ M) {
    const int g = blockIdx.x / tiles;
    const int q = (blockIdx.x - g * tiles) * 256 + threadIdx.x;
    const int Q = d * (d + 3) / 2;
    if (q >= Q) return;
    const int64_t sg0 = clamp64(gseg[g], 0, nseg_max), sg1 = clamp64(gseg[g + 1], sg0, nseg_max);
    double a = 0.0;
    for (int64_t sg = sg0; sg < sg1; ++sg) a += part[sg * Q + q];
    if (q < d) s[(int64_t)g * d + q] = a;
    else M[(int64_t)g * (Q - d) + (q - d)] = a;
}

// CB columns c0 .. c0 + CB - 1 of W_mk^T (x - mu_mk) for the lane's cell, each inner product one fma chain in coordinate
// order, then their squares added to q in column order.  xd: the lane's column of the staged points (pitch GC_ROW_TILE);
// mu and W are the same addresses for every lane of the wave.
template <int CB>
__device__ inline double gc_columns(const double* xd, const double* __restrict__ mu, const double* __restrict__ W, int d, int c0,
                                    double q) {
    double acc[CB];
#pragma unroll
    for (int b = 0; b < CB; ++b) acc[b] = 0.0;
    for (int j = 0; j < d; ++j) {
        const double t = xd[j * GC_ROW_TILE] - mu[j];
        const double* w = W + (int64_t)j * d + c0;
#pragma unroll
        for (int b = 0; b < CB; ++b) acc[b] = __builtin_fma(w[b], t, acc[b]);
    }
#pragma unroll
    for (int b = 0; b < CB; ++b) q = __builtin_fma(acc[b], acc[b], q);
    return q;
}

// One workgroup per GC_ROW_TILE consecutive cells, one cell a lane, and up to GC_SCORE_WAVES waves that share the cells and
// split the classes: wave w owns the w-th run of ceil(K / waves) consecutive classes.  The cells' points are staged once as
// doubles in LDS ([d][GC_ROW_TILE]: conflict-free, a lane reads only its own column).  A wave walks the models that one of
// the cells names (one, where the cells are sorted by model and the tile does not straddle two folds) and, for each, its
// classes in order: mu, W and c0 of (model, class) are wave-uniform reads.  A class whose c0 is -inf scores -inf and costs
// nothing.  Each wave keeps the best two scores of its classes; wave 0 merges the waves in class order through LDS, so the
// arg-max takes the lowest index on ties and best / second are the largest two scores counted with multiplicity, whatever
// the number of waves.  model values are clamped to [0, F - 1], perm values to [0, n - 1].
__global__ __launch_bounds__(GC_ROW_TILE * GC_SCORE_WAVES) void k_gc_scores(
    const float* __restrict__ x, int64_t ld, int64_t n, int d, const int* __restrict__ model, int F, int K,
    const double* __restrict__ mu, const double* __restrict__ W, const double* __restrict__ c0, const int64_t* __restrict__ perm,
    int* __restrict__ label, double* __restrict__ best, double* __restrict__ second, double* __restrict__ scores) {
    extern __shared__ double xs[];                  // [d][GC_ROW_TILE]; afterwards the waves' best two and labels
    const int lane = threadIdx.x & (GC_ROW_TILE - 1);
    const int nw = blockDim.x / GC_ROW_TILE;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / GC_ROW_TILE);    // wave-uniform, and known to be
    const int64_t r = (int64_t)blockIdx.x * GC_ROW_TILE + lane;
    const bool valid = r < n;
    const int64_t rr = valid ? r : n - 1;           // a row that exists; its results are not written
    for (int idx = threadIdx.x; idx < d * GC_ROW_TILE; idx += blockDim.x) {
        const int64_t row = imin64((int64_t)blockIdx.x * GC_ROW_TILE + (idx & (GC_ROW_TILE - 1)), n - 1);
        xs[idx] = (double)x[row * ld + (idx / GC_ROW_TILE)];
    }
    __syncthreads();
    int mine = model[rr];
    mine = mine < 0 ? 0 : (mine > F - 1 ? F - 1 : mine);
    const int64_t out = perm ? clamp64(perm[rr], 0, n - 1) : rr;
    const double* xd = xs + lane;
    const double ninf = -__builtin_inf();
    const int per = (K + nw - 1) / nw;
    const int k0 = wave * per < K ? wave * per : K, k1 = k0 + per < K ? k0 + per : K;
    double b1 = ninf, b2 = ninf;
    int lab = 0;
    for (int m = 0; m < F; ++m) {
        if (__ballot(mine == m) == 0) continue;     // wave-uniform, and the same in every wave of the workgroup
        const bool take = mine == m;
        for (int k = k0; k < k1; ++k) {
            const int64_t mk = (int64_t)m * K + k;
            const double ck = c0[mk];
            double sc = ninf;
            if (ck != ninf) {                       // wave-uniform
                const double* muk = mu + mk * d;
                const double* Wk = W + mk * d * d;
                double q = 0.0;
                int c = 0;
                for (; c + GC_COL_BLOCK <= d; c += GC_COL_BLOCK) q = gc_columns<GC_COL_BLOCK>(xd, muk, Wk, d, c, q);
                for (; c < d; ++c) q = gc_columns<1>(xd, muk, Wk, d, c, q);
                sc = ck - 0.5 * q;
            }
            if (take) {
                if (scores && valid) scores[out * K + k] = sc;
                if (sc > b1) {
                    b2 = b1;
                    b1 = sc;
                    lab = k;
                } else if (sc > b2) {
                    b2 = sc;
                }
            }
        }
    }
    __syncthreads();                                // every wave has read its last point
    double* wb1 = xs;                               // [nw][GC_ROW_TILE] each
    double* wb2 = xs + nw * GC_ROW_TILE;
    int* wlab = reinterpret_cast<int*>(xs + 2 * nw * GC_ROW_TILE);
    wb1[threadIdx.x] = b1;
    wb2[threadIdx.x] = b2;
    wlab[threadIdx.x] = lab;
    __syncthreads();
    if (wave != 0 || !valid) return;
    for (int w = 1; w < nw; ++w) {                  // in class order: a later wave wins only with a larger score
        const double o1 = wb1[w * GC_ROW_TILE + lane], o2 = wb2[w * GC_ROW_TILE + lane];
        if (o1 > b1) {
            b2 = b1 > o2 ? b1 : o2;
            b1 = o1;
            lab = wlab[w * GC_ROW_TILE + lane];
        } else if (o1 > b2) {
            b2 = o1;
        }
    }
    label[out] = lab;
    best[out] = b1;
    second[out] = b2;
}

// the instance of k_gc_partial that runs dimension d: the first entry of GC_DC that holds it
int gc_dclass(int d) {
    for (int c = 0; c < GC_N_DC; ++c)
        if (d <= GC_DC[c]) return c;
    return GC_N_DC - 1;
}

// dclass: the instance of k_gc_partial (the caller has checked d <= GC_DC[dclass]); equal bits.
// ws: part double [nseg_max][d (d + 3) / 2], seg_begin int64 [nseg_max + 1], gseg int32 [G + 1]
// (mmvae_group_moments_workspace_bytes)
int launch_group_moments(const float* x, int64_t ld, int64_t n, int d, const int64_t* offsets, int G, const float* pivot, void* ws,
                         double* s, double* M, int dclass, hipStream_t st) {
    const int64_t nseg = nseg_max(n, G, GC_SEG_ROWS);
    const int Q = d * (d + 3) / 2;
    const auto [part, seg_begin, gseg] = seg_ws_carve(ws, nseg, Q);
    if (int rc = launch_segments(offsets, G, n, GC_SEG_ROWS, nseg, gseg, seg_begin, st)) return rc;
    const dim3 grid((unsigned)nseg), block(256);
    switch (dclass) {
        case 0: hipLaunchKernelGGL((k_gc_partial<GC_DC[0]>), grid, block, 0, st, x, ld, n, d, pivot, gseg, G, seg_begin, part); break;
        case 1: hipLaunchKernelGGL((k_gc_partial<GC_DC[1]>), grid, block, 0, st, x, ld, n, d, pivot, gseg, G, seg_begin, part); break;
        case 2: hipLaunchKernelGGL((k_gc_partial<GC_DC[2]>), grid, block, 0, st, x, ld, n, d, pivot, gseg, G, seg_begin, part); break;
        default: hipLaunchKernelGGL((k_gc_partial<GC_DC[3]>), grid, block, 0, st, x, ld, n, d, pivot, gseg, G, seg_begin, part); break;
    }
    HIP_LAUNCH_CHECK("k_gc_partial");
    const int tiles = (int)cdiv64(Q, 256);
    hipLaunchKernelGGL(k_gc_finish, dim3((unsigned)((int64_t)G * tiles)), dim3(256), 0, st, part, gseg, G, nseg, d, tiles, s, M);
    HIP_LAUNCH_CHECK("k_gc_finish");
    return 0;
}

int launch_gauss_scores(const float* x, int64_t ld, int64_t n, int d, const int* model, int F, int K, const double* mu,
                        const double* W, const double* c0, const int64_t* perm, int* label, double* best, double* second,
                        double* scores, hipStream_t st) {
    const int nw = K < GC_SCORE_WAVES ? K : GC_SCORE_WAVES;
    // the staged points, reused for the waves' results: at most 64 KiB (d = GC_MAX_D)
    const size_t pts = (size_t)d * GC_ROW_TILE * sizeof(double), res = (size_t)nw * GC_ROW_TILE * (2 * sizeof(double) + sizeof(int));
    hipLaunchKernelGGL(k_gc_scores, dim3((unsigned)cdiv64(n, GC_ROW_TILE)), dim3(GC_ROW_TILE * nw), pts > res ? pts : res, st, x, ld,
                       n, d, model, F, K, mu, W, c0, perm, label, best, second, scores);
    HIP_LAUNCH_CHECK("k_gc_scores");
    return 0;
}

}  // namespace mmvae

// Data preparation on the device.
//
// The reference's mmidas/utils/tools.py turns a count matrix into the matrix the model trains on with sklearn's
// normalize(x, axis=1, norm="l1") and np.log1p(. * scaler) (normalize_cellxgene, logcpm), and ranks the genes by the spread
// of the binarised expression (reorder_genes): three full-size float64 copies on the host, of which the data-prep notebooks
// keep a ninth.  Here a workgroup owns one SELECTED row: it streams the row's G values once for the norm sum |x| over ALL
// genes (k_cpm_dense pass 1: 16-byte loads, a sum per thread in a fixed order, a fixed LDS tree) and writes only the
// selected columns, out[r, j] = f(x[row, genes[j]]), f(v) = log1p(v / norm * scaler), every step one IEEE double operation
// (pass 2: a gather from a row that went through the L2 a moment ago, coalesced stores).  k_cpm_csr does the same from a
// canonical CSR matrix and gives the same bits: it rebuilds windows of the dense row in LDS so that its sum runs in the
// dense kernel's order.  k_gs_partial / k_gs_finish are the per-gene count of x > eps and the fp64 mean and spread about a
// pivot, rows cut into segments that are added in order (the traversal of k_sc_partial, statecorr.hip).  No atomics anywhere:
// every sum has one owner and a fixed order, so every result is the same bits on every run.
#include "common.hpp"

namespace mmvae {

// the accumulator of a norm: integer counts add exactly in int64 (G <= 2^20 values below 2^31: below 2^51), floats in fp64
template <typename T> struct CpmAcc { typedef double type; };
template <> struct CpmAcc<int> { typedef int64_t type; };
__device__ inline int64_t cpm_abs(int v) { return v < 0 ? -(int64_t)v : (int64_t)v; }
__device__ inline double cpm_abs(float v) { return (double)__builtin_fabsf(v); }
__device__ inline double cpm_abs(double v) { return __builtin_fabs(v); }

// The fixed tree over the CPM_THREADS per-thread sums; every thread returns the total.
template <typename A>
__device__ inline A cpm_tree(A mine, A* red) {
    const int tid = threadIdx.x;
    red[tid] = mine;
    __syncthreads();
#pragma unroll
    for (int s = CPM_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    const A total = red[0];
    __syncthreads();
    return total;
}

// f of the file comment.  A zero stays the zero it is (log1p is not asked); nothing here can contract: there is no addition.
template <typename O>
__device__ inline O cpm_value(double v, double norm, double scaler, int log_mode) {
    const double a = v / norm;
    const double b = a * scaler;
    const double r = (log_mode && b != 0.0) ? log1p(b) : b;
    return (O)r;
}

// grid n workgroups of CPM_THREADS, workgroup r the selected row rows[r] (null: r), clamped to [0, n_total - 1].
// Pass 1: the row as pieces of V = 16 / sizeof(T) consecutive values, piece p to thread p % CPM_THREADS; a piece's values are
// added in column order (values past G count as 0), the pieces of a thread in order, the threads by cpm_tree.  WIDE: the
// base and the row pitch allow one 16-byte load for a whole piece; a piece that reaches past G, and every piece of the narrow
// form, is loaded value by value: the same map and order, hence the same bits.  Four pieces a thread are in flight.
// Pass 2: out[r][j] = f(x[row][genes[j]]), j = 0..ng-1 (genes null: column j), a gene index clamped to [0, G - 1].
// norms[r] = the sum as a double (0 for a zero row, which is then divided by 1).
template <typename T, typename O, bool WIDE>
__global__ __launch_bounds__(CPM_THREADS) void k_cpm_dense(const T* __restrict__ x, int64_t ld, int64_t n_total, int G,
                                                           const int64_t* __restrict__ rows, const int* __restrict__ genes, int ng,
                                                           double scaler, int log_mode, O* __restrict__ out,
                                                           double* __restrict__ norms) {
    typedef typename CpmAcc<T>::type A;
    constexpr int V = 16 / (int)sizeof(T);
    struct alignas(16) Piece { T v[V]; };
    __shared__ A red[CPM_THREADS];
    const int tid = threadIdx.x;
    const int64_t r = blockIdx.x;
    const int64_t row = src_row(rows, r, n_total);
    const T* xr = x + row * ld;
    const int pieces = (G + V - 1) / V;
    A acc = 0;
    for (int p0 = tid; p0 < pieces; p0 += 4 * CPM_THREADS) {
        Piece pc[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int p = p0 + u * CPM_THREADS;
            const int c = p * V;
            if (WIDE && p < pieces && c + V <= G) {
                pc[u] = *reinterpret_cast<const Piece*>(xr + c);
            } else {
#pragma unroll
                for (int e = 0; e < V; ++e) pc[u].v[e] = (p < pieces && c + e < G) ? xr[c + e] : (T)0;
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            A s = cpm_abs(pc[u].v[0]);
#pragma unroll
            for (int e = 1; e < V; ++e) s += cpm_abs(pc[u].v[e]);
            acc += s;
        }
    }
    const A total = cpm_tree<A>(acc, red);
    const double raw = (double)total;
    if (tid == 0) norms[r] = raw;
    const double norm = raw == 0.0 ? 1.0 : raw;
    O* orow = out + r * (int64_t)ng;
    for (int j = tid; j < ng; j += CPM_THREADS) {
        const int g = genes ? (int)clamp64(genes[j], 0, G - 1) : j;       // (genes null: ng == G, the launcher's check)
        orow[j] = cpm_value<O>((double)xr[g], norm, scaler, log_mode);
    }
}

// The same from CSR: indptr int64 [n_total + 1], indices int32 and data T [nnz], the indices of a row strictly increasing
// (the caller's contract).  inv int32 [G]: the output column of a gene, or -1.  The workgroup first writes its output row's
// zeros.  The norm: windows of CPM_WINDOW columns of the dense row are rebuilt in LDS (zeros, then the row's entries that
// fall in the window -- they are consecutive in the row, and the workgroup walks them CPM_THREADS at a time), and the threads
// add the window's pieces in k_cpm_dense's map and order; a zero adds nothing to a sum of magnitudes, so the sum is that
// kernel's to the bit.  Then every entry is scattered: out[r][inv[col]] = f(value).  Every position read from indptr is
// clamped to [0, nnz]; an entry whose column is outside [0, G) or outside the window being built is not used and never
// written; an inv value outside [0, ng) is not written.
template <typename T, typename O>
__global__ __launch_bounds__(CPM_THREADS) void k_cpm_csr(const int64_t* __restrict__ indptr, const int* __restrict__ indices,
                                                         const T* __restrict__ data, int64_t nnz, int64_t n_total, int G,
                                                         const int64_t* __restrict__ rows, const int* __restrict__ inv, int ng,
                                                         double scaler, int log_mode, O* __restrict__ out,
                                                         double* __restrict__ norms) {
    typedef typename CpmAcc<T>::type A;
    constexpr int V = 16 / (int)sizeof(T);
    static_assert(CPM_WINDOW % (CPM_THREADS * 4) == 0, "a window is whole sweeps of every value type");
    __shared__ A win[CPM_WINDOW];
    __shared__ A red[CPM_THREADS];
    const int tid = threadIdx.x;
    const int64_t r = blockIdx.x;
    const int64_t row = src_row(rows, r, n_total);
    const int64_t e0 = clamp64(indptr[row], 0, nnz), e1 = clamp64(indptr[row + 1], e0, nnz);
    O* orow = out + r * (int64_t)ng;
    for (int j = tid; j < ng; j += CPM_THREADS) orow[j] = (O)0;
    A acc = 0;
    int64_t pos = e0;
    for (int w0 = 0; w0 < G; w0 += CPM_WINDOW) {
        const int w1 = (int)imin64((int64_t)w0 + CPM_WINDOW, G);
        for (int i = tid; i < CPM_WINDOW; i += CPM_THREADS) win[i] = 0;
        __syncthreads();
        for (;;) {                                                   // (pos and taken are the same in every thread)
            const int64_t k = pos + tid;
            int col = -1;
            if (k < e1) col = indices[k];
            const bool before = k < e1 && col < w1;
            if (before && col >= w0) win[col - w0] = cpm_abs(data[k]);
            const int taken = __syncthreads_count(before);
            pos += taken;
            if (taken < CPM_THREADS || pos >= e1) break;              // the next entry belongs to a later window, or none is left
        }
        __syncthreads();
        // the window's pieces in the dense order: window offsets are multiples of V * CPM_THREADS, so piece p of the row is
        // piece p - w0 / V of the window and belongs to the same thread
        const int wp = (w1 - w0 + V - 1) / V;
        for (int p = tid; p < wp; p += CPM_THREADS) {
            A s = win[p * V];
#pragma unroll
            for (int e = 1; e < V; ++e) s += win[p * V + e];          // (past the row's end the window holds zeros)
            acc += s;
        }
        __syncthreads();
    }
    const A total = cpm_tree<A>(acc, red);                           // (its barriers also order the zeros above before the scatter)
    const double raw = (double)total;
    if (tid == 0) norms[r] = raw;
    const double norm = raw == 0.0 ? 1.0 : raw;
    for (int64_t k = e0 + tid; k < e1; k += CPM_THREADS) {
        const int col = indices[k];
        if (col < 0 || col >= G) continue;
        const int j = inv[col];
        if (j < 0 || j >= ng) continue;
        orow[j] = cpm_value<O>((double)data[k], norm, scaler, log_mode);
    }
}

// vtype 0 int32, 1 float, 2 double; otype 0 float, 1 double (checked by the caller)
template <typename T, typename O>
static int cpm_dense_t(const void* x, int64_t ld, int64_t n_total, int G, const int64_t* rows, int64_t n, const int* genes, int ng,
                       double scaler, int log_mode, void* out, double* norms, bool wide, hipStream_t st) {
    const dim3 grid((unsigned)n), block(CPM_THREADS);
    if (wide)
        hipLaunchKernelGGL((k_cpm_dense<T, O, true>), grid, block, 0, st, static_cast<const T*>(x), ld, n_total, G, rows, genes, ng,
                           scaler, log_mode, static_cast<O*>(out), norms);
    else
        hipLaunchKernelGGL((k_cpm_dense<T, O, false>), grid, block, 0, st, static_cast<const T*>(x), ld, n_total, G, rows, genes, ng,
                           scaler, log_mode, static_cast<O*>(out), norms);
    HIP_LAUNCH_CHECK("k_cpm_dense");
    return 0;
}

int launch_cpm_dense(const void* x, int vtype, int64_t ld, int64_t n_total, int G, const int64_t* rows, int64_t n, const int* genes,
                     int ng, double scaler, int log_mode, void* out, int otype, double* norms, bool wide, hipStream_t st) {
#define CPM_CASE(VT, T, OT, O) \
    if (vtype == VT && otype == OT) return cpm_dense_t<T, O>(x, ld, n_total, G, rows, n, genes, ng, scaler, log_mode, out, norms, wide, st)
    CPM_CASE(0, int, 0, float);
    CPM_CASE(0, int, 1, double);
    CPM_CASE(1, float, 0, float);
    CPM_CASE(1, float, 1, double);
    CPM_CASE(2, double, 0, float);
    CPM_CASE(2, double, 1, double);
#undef CPM_CASE
    set_error("cpm_dense: no kernel for value type %d and output type %d", vtype, otype);
    return MMVAE_E_BADARG;
}

template <typename T, typename O>
static int cpm_csr_t(const int64_t* indptr, const int* indices, const void* data, int64_t nnz, int64_t n_total, int G,
                     const int64_t* rows, int64_t n, const int* inv, int ng, double scaler, int log_mode, void* out, double* norms,
                     hipStream_t st) {
    hipLaunchKernelGGL((k_cpm_csr<T, O>), dim3((unsigned)n), dim3(CPM_THREADS), 0, st, indptr, indices, static_cast<const T*>(data),
                       nnz, n_total, G, rows, inv, ng, scaler, log_mode, static_cast<O*>(out), norms);
    HIP_LAUNCH_CHECK("k_cpm_csr");
    return 0;
}

int launch_cpm_csr(const int64_t* indptr, const int* indices, const void* data, int vtype, int64_t nnz, int64_t n_total, int G,
                   const int64_t* rows, int64_t n, const int* inv, int ng, double scaler, int log_mode, void* out, int otype,
                   double* norms, hipStream_t st) {
#define CPM_CASE(VT, T, OT, O) \
    if (vtype == VT && otype == OT) return cpm_csr_t<T, O>(indptr, indices, data, nnz, n_total, G, rows, n, inv, ng, scaler, log_mode, out, norms, st)
    CPM_CASE(0, int, 0, float);
    CPM_CASE(0, int, 1, double);
    CPM_CASE(1, float, 0, float);
    CPM_CASE(1, float, 1, double);
    CPM_CASE(2, double, 0, float);
    CPM_CASE(2, double, 1, double);
#undef CPM_CASE
    set_error("cpm_csr: no kernel for value type %d and output type %d", vtype, otype);
    return MMVAE_E_BADARG;
}

// ---- per-gene count, mean and spread ---------------------------------------------------------------------------------------
// grid segments x tiles workgroups (segment-major), one wave each: lane l owns the genes tile * GS_TILE + 4 l .. + 3 and walks
// the rows seg * GS_SEG_ROWS .. of the selection in order, four rows' loads in flight.  WIDE: the base and the row pitch allow
// 16-byte loads of the lane's four genes (one for floats, two for doubles); a lane whose four genes reach past D, and every
// lane of the narrow form, loads them one by one -- the same map and order, hence the same bits.  Per gene: the number of rows
// with x > eps (eps rounded to T: the comparison numpy makes), sum (x - p) and sum (x - p)^2 in fp64 with p the gene's value
// in the FIRST selected row.  part [segment][3][D] doubles (a count is exact in one).  A row index read from `rows` is
// clamped to [0, n_total - 1].
template <typename T, bool WIDE>
__global__ __launch_bounds__(64) void k_gs_partial(const T* __restrict__ data, int64_t ld, int64_t n_total, int D,
                                                   const int64_t* __restrict__ rows, int64_t n, double eps, int tiles,
                                                   double* __restrict__ part) {
    constexpr int V = 16 / (int)sizeof(T);
    struct alignas(16) Piece { T v[V]; };
    const int seg = blockIdx.x / tiles, tile = blockIdx.x - seg * tiles;
    const int64_t c0 = (int64_t)seg * GS_SEG_ROWS, c1 = imin64(c0 + GS_SEG_ROWS, n);
    const int g0 = tile * GS_TILE + 4 * threadIdx.x;
    const bool quad = WIDE && g0 + 4 <= D;
    const T epst = (T)eps;
    auto load4 = [&](const T* p, T* v) {
        if (quad) {
#pragma unroll
            for (int q = 0; q < 4 / V; ++q) {
                const Piece pc = *reinterpret_cast<const Piece*>(p + g0 + q * V);
#pragma unroll
                for (int e = 0; e < V; ++e) v[q * V + e] = pc.v[e];
            }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = g0 + e < D ? p[g0 + e] : (T)0;
        }
    };
    T piv[4];
    load4(data + src_row(rows, 0, n_total) * ld, piv);
    double cnt[4], s1[4], s2[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) cnt[e] = s1[e] = s2[e] = 0.0;
    for (int64_t i = c0; i < c1; i += 4) {
        T xv[4][4];
        bool valid[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            valid[u] = i + u < c1;
            const int64_t pos = valid[u] ? i + u : c0;                       // c0 < c1 <= n here: a row that exists
            load4(data + src_row(rows, pos, n_total) * ld, xv[u]);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double t = valid[u] ? (double)xv[u][e] - (double)piv[e] : 0.0;
                cnt[e] += (valid[u] && xv[u][e] > epst) ? 1.0 : 0.0;
                s1[e] += t;
                s2[e] = __builtin_fma(t, t, s2[e]);
            }
        }
    }
    double* base = part + (int64_t)seg * 3 * D;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int g = g0 + e;
        if (g >= D) continue;
        base[g] = cnt[e];
        base[(int64_t)D + g] = s1[e];
        base[2 * (int64_t)D + g] = s2[e];
    }
}

// One thread per gene: the segments added in order; mean = p + s1 / n, var = (s2 - s1 s1 / n) / n (not below 0), std = sqrt.
template <typename T>
__global__ __launch_bounds__(256) void k_gs_finish(const T* __restrict__ data, int64_t ld, int64_t n_total, int D,
                                                   const int64_t* __restrict__ rows, int64_t n, int nseg,
                                                   const double* __restrict__ part, int64_t* __restrict__ n_above,
                                                   double* __restrict__ mean, double* __restrict__ sd) {
    const int d = blockIdx.x * 256 + threadIdx.x;
    if (d >= D) return;
    double c = 0.0, s1 = 0.0, s2 = 0.0;
    for (int sg = 0; sg < nseg; ++sg) {
        const double* b = part + (int64_t)sg * 3 * D + d;
        c += b[0];
        s1 += b[(int64_t)D];
        s2 += b[2 * (int64_t)D];
    }
    const double p = (double)data[src_row(rows, 0, n_total) * ld + d];
    const double nn = (double)n;
    const double m = s1 / nn;
    double var = (s2 - s1 * m) / nn;
    var = var > 0.0 ? var : 0.0;                                     // (a NaN, from non-finite data, becomes 0: inputs must be finite)
    n_above[d] = (int64_t)c;
    mean[d] = p + m;
    sd[d] = __builtin_sqrt(var);
}

int64_t gs_nseg(int64_t n) { return cdiv64(n, GS_SEG_ROWS); }

template <typename T>
static int gene_stats_t(const void* data, int64_t ld, int64_t n_total, int D, const int64_t* rows, int64_t n, double eps, void* ws,
                        int64_t* n_above, double* mean, double* sd, bool wide, hipStream_t st) {
    const T* x = static_cast<const T*>(data);
    double* part = static_cast<double*>(ws);
    const int nseg = (int)gs_nseg(n), tiles = (int)cdiv64(D, GS_TILE);
    const dim3 grid((unsigned)((int64_t)nseg * tiles)), block(64);
    if (wide)
        hipLaunchKernelGGL((k_gs_partial<T, true>), grid, block, 0, st, x, ld, n_total, D, rows, n, eps, tiles, part);
    else
        hipLaunchKernelGGL((k_gs_partial<T, false>), grid, block, 0, st, x, ld, n_total, D, rows, n, eps, tiles, part);
    HIP_LAUNCH_CHECK("k_gs_partial");
    hipLaunchKernelGGL((k_gs_finish<T>), dim3((unsigned)cdiv64(D, 256)), dim3(256), 0, st, x, ld, n_total, D, rows, n, nseg, part,
                       n_above, mean, sd);
    HIP_LAUNCH_CHECK("k_gs_finish");
    return 0;
}

// vtype 1 float, 2 double.  ws: part double [segments][3][D] (mmvae_gene_stats_workspace_bytes)
int launch_gene_stats(const void* data, int vtype, int64_t ld, int64_t n_total, int D, const int64_t* rows, int64_t n, double eps,
                      void* ws, int64_t* n_above, double* mean, double* sd, bool wide, hipStream_t st) {
    if (vtype == 1) return gene_stats_t<float>(data, ld, n_total, D, rows, n, eps, ws, n_above, mean, sd, wide, st);
    if (vtype == 2) return gene_stats_t<double>(data, ld, n_total, D, rows, n, eps, ws, n_above, mean, sd, wide, st);
    set_error("gene_stats: no kernel for value type %d", vtype);
    return MMVAE_E_BADARG;
}

}  // namespace mmvae

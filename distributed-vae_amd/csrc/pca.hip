// Principal components on the device.
//
// The reference's clusterability analysis (mmidas/utils/cluster_analysis.py: cluster_compare) scores the cell types on the
// top principal components of the expression matrix.  Three launches carry the dense part of that.  mmvae_gram: the first
// and second moments of the fp32 matrix about one pivot, s = sum t and G = sum t t^T with t = (double)x - (double)pivot, on
// the fp64 MFMA (v_mfma_f64_16x16x4_f64): a workgroup owns one 64 x 64 tile of G with tile_i <= tile_j and one segment of
// the rows (k_gram_partial), and a last launch adds the segments in order, mirrors the upper triangle into the lower and, on
// request, turns G into the covariance (k_gram_finish).  mmvae_symm_mul: Y = C Q for a block Q of at most 64 columns, one
// read of C (the product of a subspace iteration).  mmvae_pca_project: Z = ((double)x - mean) V.  The last two are one
// kernel (k_rows_mul): each output is one fp64 fma chain in coordinate order.  No atomics anywhere: every sum has one owner
// and a fixed order, so the results are the same bits on every run.
#include "common.hpp"

namespace mmvae {

typedef double f64x4 __attribute__((ext_vector_type(4)));

// The four floats at p[c] .. p[c + 3] of a row of D columns; a column at or past D reads as its pivot would make t = 0
// (the caller masks it).  WIDE: one 16-byte load where all four columns exist, else one float at a time: the same values.
template <bool WIDE>
__device__ inline void gram_load4(const float* __restrict__ p, int c, int D, float (&v)[4]) {
    if (WIDE && c + 4 <= D) {
        const float4 q = *reinterpret_cast<const float4*>(p + c);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = c + e < D ? p[c + e] : 0.f;
    }
}

// grid (T, T, nseg), T = ceil(D / 64): workgroup (x = tile_j, y = tile_i, z = segment); tile_i > tile_j leaves at once.
// 256 threads, four waves in 2 x 2, each wave a 32 x 32 piece of the tile as 2 x 2 MFMA tiles of 16 x 16.  The segment's
// rows are staged GRAM_KC at a time in LDS as doubles t = (double)x - (double)pivot, [row][column] with pitch GRAM_PITCH,
// one image for the tile's row block of columns (I) and one for its column block (J; the same image on the diagonal).
// The next chunk's floats are loaded into registers before the current one is multiplied.  v_mfma_f64_16x16x4_f64 takes
// A[i = lane & 15][k = lane >> 4] and B[k = lane >> 4][j = lane & 15], so both operands are read from their image at
// [k0 + (lane >> 4)][column (lane & 15)]; its result register reg of lane l is C[i = (l >> 4) + 4 reg][j = l & 15] -- the
// f64 map, not the f32 one.  A row past the segment's end and a column at or past D are staged as t = 0.  Rows read from
// `rows` are clamped to [0, n_total - 1].  On the diagonal the first wave also adds up the columns of the image, row by
// row: the segment's part of s.  out: the segment's D x D matrix (pitch D), upper tiles only; sout its s [D].
template <bool WIDE>
__global__ __launch_bounds__(256) void k_gram_partial(const float* __restrict__ data, int64_t ld, int64_t n_total,
                                                      const int64_t* __restrict__ rows, int64_t n, int D,
                                                      const float* __restrict__ pivot, int64_t seg_rows, double* __restrict__ G,
                                                      double* __restrict__ ws_mat, double* __restrict__ ws_s) {
    const int tj = blockIdx.x, ti = blockIdx.y, seg = blockIdx.z;
    if (ti > tj) return;                            // the whole workgroup
    __shared__ double img[2][GRAM_KC * GRAM_PITCH];
    const bool diag = ti == tj;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wi = wave >> 1, wj = wave & 1;
    const int64_t r_begin = (int64_t)seg * seg_rows, r_end = imin64(r_begin + seg_rows, n);
    const int i0 = ti * GRAM_TILE, j0 = tj * GRAM_TILE;
    // staging: thread t owns rows (t >> 4) and (t >> 4) + 16 of the chunk and the four columns 4 (t & 15) .. + 3
    const int sr = tid >> 4, sc = 4 * (tid & 15);
    double pivI[4], pivJ[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        pivI[e] = i0 + sc + e < D ? (double)pivot[i0 + sc + e] : 0.0;
        pivJ[e] = j0 + sc + e < D ? (double)pivot[j0 + sc + e] : 0.0;
    }
    float xI[2][4], xJ[2][4];
    bool live[2];
    auto fetch = [&](int64_t r0) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int64_t pos = r0 + sr + 16 * h;
            live[h] = pos < r_end;
            const int64_t at = live[h] ? pos : r_begin;                   // r_begin < r_end <= n: a row that exists
            const int64_t row = src_row(rows, at, n_total);
            const float* p = data + row * ld;
            gram_load4<WIDE>(p, i0 + sc, D, xI[h]);
            if (!diag) gram_load4<WIDE>(p, j0 + sc, D, xJ[h]);
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            double* dI = &img[0][(sr + 16 * h) * GRAM_PITCH + sc];
            double* dJ = &img[1][(sr + 16 * h) * GRAM_PITCH + sc];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                dI[e] = live[h] && i0 + sc + e < D ? (double)xI[h][e] - pivI[e] : 0.0;
                if (!diag) dJ[e] = live[h] && j0 + sc + e < D ? (double)xJ[h][e] - pivJ[e] : 0.0;
            }
        }
    };
    f64x4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = f64x4{0.0, 0.0, 0.0, 0.0};
    double ssum = 0.0;
    const double* imI = img[0];
    const double* imJ = diag ? img[0] : img[1];
    const int frag = (lane >> 4) * GRAM_PITCH + (lane & 15);
    if (r_begin < r_end) fetch(r_begin);
    for (int64_t r0 = r_begin; r0 < r_end; r0 += GRAM_KC) {
        __syncthreads();                            // the chunk before this one has been read
        stage();
        __syncthreads();
        if (r0 + GRAM_KC < r_end) fetch(r0 + GRAM_KC);
        if (diag && wave == 0) {
#pragma unroll 8
            for (int k = 0; k < GRAM_KC; ++k) ssum += imI[k * GRAM_PITCH + lane];
        }
#pragma unroll
        for (int k0 = 0; k0 < GRAM_KC; k0 += 4) {
            double a[2], b[2];
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                a[m] = imI[k0 * GRAM_PITCH + frag + wi * 32 + m * 16];
                b[m] = imJ[k0 * GRAM_PITCH + frag + wj * 32 + m * 16];
            }
#pragma unroll
            for (int ma = 0; ma < 2; ++ma)
#pragma unroll
                for (int mb = 0; mb < 2; ++mb)
                    acc[ma][mb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ma], b[mb], acc[ma][mb], 0, 0, 0);
        }
    }
    double* out = seg == 0 ? G : ws_mat + (int64_t)(seg - 1) * D * D;
#pragma unroll
    for (int ma = 0; ma < 2; ++ma)
#pragma unroll
        for (int mb = 0; mb < 2; ++mb) {
            const int j = j0 + wj * 32 + mb * 16 + (lane & 15);
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int i = i0 + wi * 32 + ma * 16 + (lane >> 4) + 4 * reg;
                if (i < D && j < D) out[(int64_t)i * D + j] = acc[ma][mb][reg];
            }
        }
    if (diag && wave == 0 && i0 + lane < D) ws_s[(int64_t)seg * D + i0 + lane] = ssum;
}

// grid (ceil(D / 256), D): one thread per (i = blockIdx.y, j), j >= i: the segments' entries added in segment order, then
// on request cov = (G - s_i s_j / n) / (n - 1), written to (i, j) and (j, i): the same bits on both sides.  An entry below
// the diagonal is never read, so the launch can work in place.  The thread of (i, i) writes s_i, the segments' sums added
// in the same order.
__global__ __launch_bounds__(256) void k_gram_finish(double* __restrict__ G, const double* __restrict__ ws_mat,
                                                     const double* __restrict__ ws_s, int D, int nseg, int64_t n, int cov,
                                                     double* __restrict__ s) {
    const int i = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    if (j >= D || j < i) return;
    double v = G[(int64_t)i * D + j];
    for (int sg = 1; sg < nseg; ++sg) v += ws_mat[(int64_t)(sg - 1) * D * D + (int64_t)i * D + j];
    double si = 0.0, sj = 0.0;
    for (int sg = 0; sg < nseg; ++sg) {
        si += ws_s[(int64_t)sg * D + i];
        sj += ws_s[(int64_t)sg * D + j];
    }
    if (cov) v = (v - si * sj / (double)n) / (double)(n - 1);
    G[(int64_t)i * D + j] = v;
    G[(int64_t)j * D + i] = v;
    if (i == j) s[i] = si;
}

// Z = (X - mean) V, X [n, D] of float or double, V [D, k] double, k <= 64.  A workgroup owns RM_ROWS = 16 consecutive rows:
// wave w the rows 4 w .. 4 w + 3, lane c the column c of V (lanes at or past k stage and do not multiply).  The coordinates
// are walked 64 at a time: the rows' pieces (as doubles, mean subtracted: one rounding) and V's piece -- 64 k consecutive
// doubles of V -- are staged in LDS, the next piece loaded into registers while the current one is multiplied, and output
// (row, c) is one fma chain in coordinate order whatever the workgroup, so a row's values do not depend on the rows beside
// it.  A row past n and a coordinate past D are staged as zeros.  Rows read from `rows` are clamped to [0, n_total - 1].
template <typename T>
__global__ __launch_bounds__(256) void k_rows_mul(const T* __restrict__ X, int64_t ld, int64_t n_total,
                                                  const int64_t* __restrict__ rows, int64_t n, int D,
                                                  const double* __restrict__ mean, const double* __restrict__ V, int k,
                                                  double* __restrict__ Z) {
    constexpr int VPT = RM_CHUNK * RM_CHUNK / 256;  // entries of V's piece a thread stages at most
    __shared__ double xs[RM_ROWS][RM_CHUNK];
    __shared__ double vs[RM_CHUNK][RM_CHUNK + 1];
    const int tid = threadIdx.x, c = tid & 63, w = tid >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * RM_ROWS;
    const int nv = RM_CHUNK * k;                    // V's piece: entry idx is coordinate idx / k, column idx % k
    const int64_t vend = (int64_t)D * k;
    int64_t rowoff[4];
    bool live[4];
    int voff[VPT];
#pragma unroll
    for (int h = 0; h < 4; ++h) {
        const int64_t pos = r0 + 4 * w + h;
        live[h] = pos < n;
        // (src_row's clamp, around the choice of a row past n as well: this form keeps the kernel's schedule as it was)
        rowoff[h] = clamp64(live[h] ? (rows ? rows[pos] : pos) : 0, 0, n_total - 1) * ld;
    }
#pragma unroll
    for (int e = 0; e < VPT; ++e) {
        const int idx = tid + 256 * e, jj = idx / k;
        voff[e] = jj * (RM_CHUNK + 1) + (idx - jj * k);
    }
    double xv[4], vv[VPT];
    auto fetch = [&](int j0) {
        const int j = j0 + c;
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            xv[h] = 0.0;
            if (live[h] && j < D) {
                xv[h] = (double)X[rowoff[h] + j];
                if (mean) xv[h] -= mean[j];
            }
        }
        const int64_t vbase = (int64_t)j0 * k;
#pragma unroll
        for (int e = 0; e < VPT; ++e) {
            const int idx = tid + 256 * e;
            vv[e] = idx < nv && vbase + idx < vend ? V[vbase + idx] : 0.0;
        }
    };
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    double* vflat = &vs[0][0];
    fetch(0);
    for (int j0 = 0; j0 < D; j0 += RM_CHUNK) {
        __syncthreads();                            // the piece before this one has been read
#pragma unroll
        for (int h = 0; h < 4; ++h) xs[4 * w + h][c] = xv[h];
#pragma unroll
        for (int e = 0; e < VPT; ++e)
            if (tid + 256 * e < nv) vflat[voff[e]] = vv[e];
        __syncthreads();
        if (j0 + RM_CHUNK < D) fetch(j0 + RM_CHUNK);
        if (c < k) {
#pragma unroll 8
            for (int jj = 0; jj < RM_CHUNK; ++jj) {
                const double v = vs[jj][c];
#pragma unroll
                for (int h = 0; h < 4; ++h) acc[h] = __builtin_fma(xs[4 * w + h][jj], v, acc[h]);
            }
        }
    }
    if (c < k) {
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            const int64_t pos = r0 + 4 * w + h;
            if (pos < n) Z[pos * k + c] = acc[h];
        }
    }
}

// the segments of mmvae_gram: one where the upper tiles alone fill the chip, else at most GRAM_MAX_SEGS of at least
// GRAM_SEG_ROWS rows (the last may be shorter); past GRAM_MAX_SEGS GRAM_SEG_ROWS rows the segments grow, in whole chunks
int gram_segments(int64_t n, int D, int64_t* seg_rows) {
    const int64_t T = cdiv64(D, GRAM_TILE);
    int nseg = 1;
    int64_t len = n;
    if (T * (T + 1) / 2 < GRAM_FILL_TILES && n > GRAM_SEG_ROWS) {
        if (n <= (int64_t)GRAM_MAX_SEGS * GRAM_SEG_ROWS) {
            len = GRAM_SEG_ROWS;
        } else {
            len = cdiv64(cdiv64(n, GRAM_MAX_SEGS), GRAM_KC) * GRAM_KC;
        }
        nseg = (int)cdiv64(n, len);
    }
    if (seg_rows) *seg_rows = len;
    return nseg;
}

// ws: ws_mat double [nseg - 1][D][D], ws_s double [nseg][D] (mmvae_gram_workspace_bytes)
int launch_gram(const float* data, int64_t ld, int64_t n_total, const int64_t* rows, int64_t n, int D, const float* pivot, void* ws,
                double* s, double* G, int cov, bool wide, hipStream_t st) {
    int64_t seg_rows = 0;
    const int nseg = gram_segments(n, D, &seg_rows);
    double* ws_mat = static_cast<double*>(ws);
    double* ws_s = ws_mat + (int64_t)(nseg - 1) * D * D;
    const unsigned T = (unsigned)cdiv64(D, GRAM_TILE);
    const dim3 grid(T, T, (unsigned)nseg), block(256);
    if (wide)
        hipLaunchKernelGGL((k_gram_partial<true>), grid, block, 0, st, data, ld, n_total, rows, n, D, pivot, seg_rows, G, ws_mat, ws_s);
    else
        hipLaunchKernelGGL((k_gram_partial<false>), grid, block, 0, st, data, ld, n_total, rows, n, D, pivot, seg_rows, G, ws_mat, ws_s);
    HIP_LAUNCH_CHECK("k_gram_partial");
    hipLaunchKernelGGL(k_gram_finish, dim3((unsigned)cdiv64(D, 256), (unsigned)D), dim3(256), 0, st, G, ws_mat, ws_s, D, nseg, n, cov, s);
    HIP_LAUNCH_CHECK("k_gram_finish");
    return 0;
}

int launch_symm_mul(const double* C, int64_t ldc, int D, const double* Q, int b, double* Y, hipStream_t st) {
    hipLaunchKernelGGL((k_rows_mul<double>), dim3((unsigned)cdiv64(D, RM_ROWS)), dim3(256), 0, st, C, ldc, (int64_t)D, nullptr,
                       (int64_t)D, D, nullptr, Q, b, Y);
    HIP_LAUNCH_CHECK("k_rows_mul<double>");
    return 0;
}

int launch_pca_project(const float* data, int64_t ld, int64_t n_total, const int64_t* rows, int64_t n, int D, const double* mean,
                       const double* V, int k, double* Z, hipStream_t st) {
    hipLaunchKernelGGL((k_rows_mul<float>), dim3((unsigned)cdiv64(n, RM_ROWS)), dim3(256), 0, st, data, ld, n_total, rows, n, D, mean,
                       V, k, Z);
    HIP_LAUNCH_CHECK("k_rows_mul<float>");
    return 0;
}

}  // namespace mmvae

// State-gene correlation on the device.
//
// The reference's continuous-variable analysis (mmidas/utils/tree_based_analysis.py: corr_analysis) takes, for every state
// dimension s and every gene g, the Pearson correlation of the state with the gene's expression over the cells that express
// the gene (x > 0, more than four of them): S x D calls of scipy.stats.pearsonr, each with a boolean mask over all cells, and
// once more per category.  Here it is one pass over the fp32 matrix, read where it lies: a wave owns SC_TILE = 256
// consecutive genes (four a lane, one float4 a row) and one segment of at most SC_SEG_ROWS rows, and keeps per gene the
// masked count, sum x, sum x^2, min x, max x and per (gene, state) sum s, sum s^2, sum x s, min s, max s -- all sums fp64,
// every product of two fp32 values exact in fp64 (k_sc_partial).  The rows arrive ordered by group and the segments never
// cross a group boundary (k_segments, segments.hip: the scheme is described once, in common.hpp); a last launch adds each group's segments in order
// and forms r in fp64 (k_sc_finish).  No atomics: every sum has one owner and a fixed order, so the result is the same bits
// on every run, and a group's values are those of a call on that group's rows alone.
#include "common.hpp"

namespace mmvae {

// grid nseg_max x tiles workgroups (segment-major, so that neighbours read neighbouring pieces of the same rows), one wave
// each: lane l owns the genes tile * SC_TILE + 4 l .. + 3 and walks the segment's rows in order, four rows' loads in flight.
// WIDE: the row pitch and the base allow a 16-byte load of the lane's four genes; a lane whose four genes reach past D, and
// every lane of the narrow form, loads them one by one.  The lane-to-gene map and the row order are the same, so both forms
// give the same bits.  NS states a pass, s0 the first of them; the x moments are written by the pass with write_x only.
// part [segment][5 + 5 S][D]: rows 0..4 count, sum x, sum x^2, min x, max x; rows 5 + 5 s .. of state s: sum s, sum s^2,
// sum x s, min s, max s -- all as doubles (counts, minima and maxima are exact in them).  A row index read from `rows` is
// clamped to [0, n_total - 1]; a row past the segment's end is given x = 0, which the mask drops.
template <int NS, bool WIDE>
__global__ __launch_bounds__(64) void k_sc_partial(const float* __restrict__ data, int64_t ld, int64_t n_total, int D,
                                                   const int64_t* __restrict__ rows, const float* __restrict__ state, int64_t lds,
                                                   int64_t n, int s0, int S, int write_x, const int* __restrict__ gseg, int G,
                                                   const int64_t* __restrict__ seg_begin, int tiles, double* __restrict__ part) {
    const int seg = blockIdx.x / tiles, tile = blockIdx.x - seg * tiles;
    if (seg >= gseg[G]) return;                     // the whole workgroup
    int64_t c0, c1;
    seg_range(seg_begin, seg, n, SC_SEG_ROWS, c0, c1);
    const int g0 = tile * SC_TILE + 4 * threadIdx.x;
    const bool quad = WIDE && g0 + 4 <= D;
    double cnt[4], sx[4], sxx[4], ss[NS][4], sss[NS][4], sxs[NS][4];
    float minx[4], maxx[4], mins[NS][4], maxs[NS][4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        cnt[e] = sx[e] = sxx[e] = 0.0;
        minx[e] = __builtin_inff();
        maxx[e] = -__builtin_inff();
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            ss[k][e] = sss[k][e] = sxs[k][e] = 0.0;
            mins[k][e] = __builtin_inff();
            maxs[k][e] = -__builtin_inff();
        }
    }
    for (int64_t i = c0; i < c1; i += 4) {
        float x[4][4], sv[4][NS];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const bool valid = i + u < c1;
            const int64_t pos = valid ? i + u : c0;                       // c0 < c1 <= n here: a row that exists
            const int64_t row = src_row(rows, pos, n_total);
            const float* p = data + row * ld;
            if (quad) {
                const float4 v = *reinterpret_cast<const float4*>(p + g0);
                x[u][0] = v.x; x[u][1] = v.y; x[u][2] = v.z; x[u][3] = v.w;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) x[u][e] = g0 + e < D ? p[g0 + e] : 0.f;
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) x[u][e] = valid ? x[u][e] : 0.f;
#pragma unroll
            for (int k = 0; k < NS; ++k) sv[u][k] = state[pos * lds + s0 + k];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float xf = x[u][e];
                const bool m = xf > 0.f;
                const double xd = m ? (double)xf : 0.0;
                cnt[e] += m ? 1.0 : 0.0;
                sx[e] += xd;
                sxx[e] = __builtin_fma(xd, xd, sxx[e]);
                minx[e] = m ? __builtin_fminf(minx[e], xf) : minx[e];
                maxx[e] = m ? __builtin_fmaxf(maxx[e], xf) : maxx[e];
#pragma unroll
                for (int k = 0; k < NS; ++k) {
                    const float sf = sv[u][k];
                    const double sd = (double)sf;
                    ss[k][e] += m ? sd : 0.0;
                    sss[k][e] += m ? sd * sd : 0.0;
                    sxs[k][e] = __builtin_fma(xd, sd, sxs[k][e]);
                    mins[k][e] = m ? __builtin_fminf(mins[k][e], sf) : mins[k][e];
                    maxs[k][e] = m ? __builtin_fmaxf(maxs[k][e], sf) : maxs[k][e];
                }
            }
        }
    }
    const int Q = 5 + 5 * S;
    double* base = part + (int64_t)seg * Q * D;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int g = g0 + e;
        if (g >= D) continue;
        if (write_x) {
            base[0 * (int64_t)D + g] = cnt[e];
            base[1 * (int64_t)D + g] = sx[e];
            base[2 * (int64_t)D + g] = sxx[e];
            base[3 * (int64_t)D + g] = (double)minx[e];
            base[4 * (int64_t)D + g] = (double)maxx[e];
        }
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            double* q = base + (int64_t)(5 + 5 * (s0 + k)) * D + g;
            q[0 * (int64_t)D] = ss[k][e];
            q[1 * (int64_t)D] = sss[k][e];
            q[2 * (int64_t)D] = sxs[k][e];
            q[3 * (int64_t)D] = (double)mins[k][e];
            q[4 * (int64_t)D] = (double)maxs[k][e];
        }
    }
}

// One thread per (group, gene): the group's segments added in order, then per state
//   r = (sum xs - sum x sum s / c) / sqrt((sum x^2 - (sum x)^2 / c) (sum s^2 - (sum s)^2 / c)), clipped to [-1, 1];
// exactly 0 where the count c <= 4 (the reference's rule; an all-zero or negative gene has c = 0); NaN where x or s is constant
// over the mask (scipy's constant-input result), decided by min == max, which raw moments cannot decide.
__global__ __launch_bounds__(256) void k_sc_finish(const double* __restrict__ part, const int* __restrict__ gseg, int G,
                                                   int64_t nseg_max, int D, int S, int tiles, double* __restrict__ r,
                                                   int64_t* __restrict__ count) {
    const int g = blockIdx.x / tiles;
    const int d = (blockIdx.x - g * tiles) * 256 + threadIdx.x;
    if (d >= D) return;
    const int64_t sg0 = clamp64(gseg[g], 0, nseg_max), sg1 = clamp64(gseg[g + 1], sg0, nseg_max);
    const int Q = 5 + 5 * S;
    const int64_t segstride = (int64_t)Q * D;
    double c = 0.0, sx = 0.0, sxx = 0.0, minx = __builtin_inf(), maxx = -__builtin_inf();
    for (int64_t sg = sg0; sg < sg1; ++sg) {
        const double* b = part + sg * segstride + d;
        c += b[0];
        sx += b[(int64_t)D];
        sxx += b[2 * (int64_t)D];
        minx = __builtin_fmin(minx, b[3 * (int64_t)D]);
        maxx = __builtin_fmax(maxx, b[4 * (int64_t)D]);
    }
    count[(int64_t)g * D + d] = (int64_t)c;
    for (int s = 0; s < S; ++s) {
        double ss = 0.0, sss = 0.0, sxs = 0.0, mins = __builtin_inf(), maxs = -__builtin_inf();
        for (int64_t sg = sg0; sg < sg1; ++sg) {
            const double* b = part + sg * segstride + (int64_t)(5 + 5 * s) * D + d;
            ss += b[0];
            sss += b[(int64_t)D];
            sxs += b[2 * (int64_t)D];
            mins = __builtin_fmin(mins, b[3 * (int64_t)D]);
            maxs = __builtin_fmax(maxs, b[4 * (int64_t)D]);
        }
        double out = 0.0;
        if (c > 4.0) {
            if (minx == maxx || mins == maxs) {
                out = __builtin_nan("");
            } else {
                const double vx = sxx - sx * sx / c, vs = sss - ss * ss / c, cov = sxs - sx * ss / c;
                out = cov / __builtin_sqrt(vx * vs);
                out = out > 1.0 ? 1.0 : (out < -1.0 ? -1.0 : out);     // a NaN (variance rounded to <= 0) stays a NaN
            }
        }
        r[((int64_t)g * S + s) * D + d] = out;
    }
}

// wide: the 16-byte loads (the caller has checked wide16), else the narrow ones; equal bits.
// ws: part double [nseg_max][5 + 5 S][D], seg_begin int64 [nseg_max + 1], gseg int32 [G + 1]
// (mmvae_state_corr_workspace_bytes)
int launch_state_corr(const float* data, int64_t ld, int64_t n_total, int D, const int64_t* rows, const float* state, int64_t lds,
                      int64_t n, int S, const int64_t* offsets, int G, void* ws, double* r, int64_t* count, bool wide, hipStream_t st) {
    const int64_t nseg = nseg_max(n, G, SC_SEG_ROWS);
    const auto [part, seg_begin, gseg] = seg_ws_carve(ws, nseg, (5 + 5 * (int64_t)S) * D);
    if (int rc = launch_segments(offsets, G, n, SC_SEG_ROWS, nseg, gseg, seg_begin, st)) return rc;
    const int tiles = (int)cdiv64(D, SC_TILE);
    const dim3 grid((unsigned)(nseg * tiles)), block(64);
#define SC_PASS(NS)                                                                                                          \
    do {                                                                                                                     \
        if (wide)                                                                                                            \
            hipLaunchKernelGGL((k_sc_partial<NS, true>), grid, block, 0, st, data, ld, n_total, D, rows, state, lds, n, s0, S,  \
                               s0 == 0 ? 1 : 0, gseg, G, seg_begin, tiles, part);                                            \
        else                                                                                                                 \
            hipLaunchKernelGGL((k_sc_partial<NS, false>), grid, block, 0, st, data, ld, n_total, D, rows, state, lds, n, s0, S, \
                               s0 == 0 ? 1 : 0, gseg, G, seg_begin, tiles, part);                                            \
        HIP_LAUNCH_CHECK("k_sc_partial");                                                                                    \
        s0 += NS;                                                                                                            \
    } while (0)
    int s0 = 0;
    while (S - s0 >= 4) SC_PASS(4);
    if (S - s0 >= 2) SC_PASS(2);
    if (S - s0 >= 1) SC_PASS(1);
#undef SC_PASS
    const int ftiles = (int)cdiv64(D, 256);
    hipLaunchKernelGGL(k_sc_finish, dim3((unsigned)((int64_t)G * ftiles)), dim3(256), 0, st, part, gseg, G, nseg, D, S, ftiles, r,
                       count);
    HIP_LAUNCH_CHECK("k_sc_finish");
    return 0;
}

}  // namespace mmvae

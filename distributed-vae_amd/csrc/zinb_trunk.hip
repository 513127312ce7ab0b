// The backward of one arm's decoder trunk fc6 .. fc10 from the gradient with respect to d10 (include/mmvae.h:
// mmvae_decoder_trunk_grads).  The activations are those an eval forward or mmvae_decode leaves: zin
// [N, Z], d6 = relu(fc6(zin)) [N, L], d7 .. d10 [N, H]; the weights in nn.Linear's layout ([out, in]).
//   dZ10 = gd10 * [d10 > 0];  G_l-1 = dZ_l W_l;  dZ_l-1 = G_l-1 * [d_l-1 > 0];  gzin = dZ6 W6 (on request)
//   dW_l = dZ_l^T in_l,  db_l = sum_i dZ_l[i]
// Three launches:
//   k_tr_chain   a workgroup owns 32 cells and walks the five layers down; dZ_l of the cells sits in LDS, W_l is read from
//                global memory (40 KB a layer: L2), a thread owns one input column k and 16 cells; every dZ_l goes to the
//                workspace ([N, width], float32) for the next launch;
//   k_tr_dw      a workgroup owns 16 x 128 entries of one layer's dW (and the 16 entries of db beside them, where it has
//                the first column block) and one segment of the cells, which it walks in rising order in chunks of 32;
//   k_tr_finish  adds the segments' partials in segment order and rounds once.
// Every product is fp32 x fp32 formed exactly in fp64, every sum an fp64 fma chain in a fixed order (the fan-out of the layer
// rising, the cells rising), rounded to float32 once where a value is stored: these five layers are under 1 % of the fit's
// arithmetic and fp64 costs them nothing that shows, while a float32 chain over a few hundred cells of one sign (db, as
// section 9m found) does not hold the error gate.  No atomics: bit-identical from run to run.
// This is deliberately not the train step's k_chain_bwd<dec>: that kernel lives in the step's Ctx / Layout / plan
// machinery, which carries no ZINB call kind; it can be shared when ZINB enters the step.
#include "common.hpp"

namespace mmvae {

constexpr int TR_TC = 32;                 // cells of a k_tr_chain workgroup, and of one chunk of k_tr_dw
constexpr int TR_P = TR_MAX_W + 1;        // the LDS pitch of a row of dZ
constexpr int TR_TO = 16;                 // rows of dW a k_tr_dw workgroup owns
constexpr int TR_TK = 128;                // columns of dW a k_tr_dw workgroup owns

struct TrChain {
    const float* act[6];                  // zin, d6 .. d10 (act[0] is not read: the chain needs the relu masks only)
    int64_t ld[6];
    int width[6];                         // Z, L, H, H, H, H
    const float* W[5];                    // fc6 .. fc10: [width[l + 1], width[l]]
    float* dz[5];                         // dZ6 .. dZ10 in the workspace, [N, width[l + 1]]
};

__global__ __launch_bounds__(256) void k_tr_chain(TrChain a, int64_t N, const float* __restrict__ gd10, int64_t ldg, float* __restrict__ gzin,
                                                  int64_t ldgz) {
    __shared__ float buf[2][TR_TC * TR_P];
    const int t = threadIdx.x, kk = t & 127, cg = t >> 7;
    const int64_t c0 = (int64_t)blockIdx.x * TR_TC;
    float* cur = buf[0];
    float* nxt = buf[1];
    {
        const int Wd = a.width[5];
        for (int idx = t; idx < TR_TC * Wd; idx += 256) {
            const int c = idx / Wd, k = idx % Wd;
            const int64_t cell = c0 + c;
            float v = 0.f;
            if (cell < N) {
                v = a.act[5][cell * a.ld[5] + k] > 0.f ? gd10[cell * ldg + k] : 0.f;
                a.dz[4][cell * Wd + k] = v;
            }
            cur[c * TR_P + k] = v;
        }
    }
    __syncthreads();
    for (int l = 4; l >= 0; --l) {        // through fc(6 + l): dZ of width[l + 1] in, width[l] out
        if (l == 0 && !gzin) break;
        const int O = a.width[l + 1], K = a.width[l];
        const float* __restrict__ W = a.W[l];
        for (int k = kk; k < K; k += 128) {
            double acc[16];
#pragma unroll
            for (int m = 0; m < 16; ++m) acc[m] = 0.0;
            for (int o = 0; o < O; ++o) {
                const double wv = (double)W[(int64_t)o * K + k];
#pragma unroll
                for (int m = 0; m < 16; ++m) acc[m] = fma((double)cur[(cg + 2 * m) * TR_P + o], wv, acc[m]);
            }
#pragma unroll
            for (int m = 0; m < 16; ++m) {
                const int c = cg + 2 * m;
                const int64_t cell = c0 + c;
                if (l > 0) {               // K <= TR_MAX_W here: one column a thread
                    float v = 0.f;
                    if (cell < N) {
                        v = a.act[l][cell * a.ld[l] + k] > 0.f ? (float)acc[m] : 0.f;
                        a.dz[l - 1][cell * K + k] = v;
                    }
                    nxt[c * TR_P + k] = v;
                } else if (cell < N) {
                    gzin[cell * ldgz + k] = (float)acc[m];
                }
            }
        }
        __syncthreads();
        float* s = cur;
        cur = nxt;
        nxt = s;
    }
}

struct TrLayer {
    const float* dz;                      // [N, O]
    const float* in;                      // [N, ldin]
    int64_t ldin, poff;                   // poff: where the layer's dW [O, K], then db [O], start in a segment's partials
    int O, K, tile0, kblocks;
};
struct TrLayers {
    TrLayer l[5];
};

__global__ __launch_bounds__(256) void k_tr_dw(TrLayers a, int64_t N, int64_t cells_per_seg, int64_t P, double* __restrict__ part) {
    __shared__ float dz_s[TR_TC][TR_TO];
    __shared__ float in_s[TR_TC][TR_TK];
    int li = 0;
    while (li < 4 && (int)blockIdx.x >= a.l[li + 1].tile0) ++li;
    const TrLayer L = a.l[li];
    const int rel = (int)blockIdx.x - L.tile0;
    const int o0 = (rel / L.kblocks) * TR_TO, k0 = (rel % L.kblocks) * TR_TK;
    const bool first = rel % L.kblocks == 0;
    const int t = threadIdx.x, kk = t & 127, og = t >> 7;
    const int64_t cb = (int64_t)blockIdx.y * cells_per_seg, ce = imin64(cb + cells_per_seg, N);
    double acc[8], db = 0.0;
#pragma unroll
    for (int m = 0; m < 8; ++m) acc[m] = 0.0;
    for (int64_t c0 = cb; c0 < ce; c0 += TR_TC) {
        for (int idx = t; idx < TR_TC * TR_TO; idx += 256) {
            const int c = idx / TR_TO, o = idx % TR_TO;
            dz_s[c][o] = (c0 + c < ce && o0 + o < L.O) ? L.dz[(c0 + c) * L.O + o0 + o] : 0.f;
        }
        for (int idx = t; idx < TR_TC * TR_TK; idx += 256) {
            const int c = idx / TR_TK, k = idx % TR_TK;
            in_s[c][k] = (c0 + c < ce && k0 + k < L.K) ? L.in[(c0 + c) * L.ldin + k0 + k] : 0.f;
        }
        __syncthreads();
#pragma unroll 4
        for (int c = 0; c < TR_TC; ++c) {
            const double av = (double)in_s[c][kk];
#pragma unroll
            for (int m = 0; m < 8; ++m) acc[m] = fma((double)dz_s[c][og + 2 * m], av, acc[m]);
        }
        if (first && t < TR_TO)
            for (int c = 0; c < TR_TC; ++c) db += (double)dz_s[c][t];
        __syncthreads();
    }
    double* mine = part + (int64_t)blockIdx.y * P + L.poff;
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        const int o = o0 + og + 2 * m, k = k0 + kk;
        if (o < L.O && k < L.K) mine[(int64_t)o * L.K + k] = acc[m];
    }
    if (first && t < TR_TO && o0 + t < L.O) mine[(int64_t)L.O * L.K + o0 + t] = db;
}

struct TrOut {
    float* p[10];                         // dW6, db6, .. dW10, db10
    int64_t end[10];                      // where each ends in a segment's partials
};

__global__ __launch_bounds__(256) void k_tr_finish(const double* __restrict__ part, int nseg, int64_t P, TrOut out) {
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < P; idx += (int64_t)gridDim.x * 256) {
        double s = 0.0;
        for (int sg = 0; sg < nseg; ++sg) s += part[(int64_t)sg * P + idx];
        int j = 0;
        while (j < 9 && idx >= out.end[j]) ++j;
        out.p[j][idx - (j ? out.end[j - 1] : 0)] = (float)s;
    }
}

// The cell segments of k_tr_dw: asked = 0 is the rule, one for every 512 cells and at most 32 (a constant, not read from the
// device); a segment is whole chunks of 32 cells, the last may be shorter; the count is what that leaves.
int tr_segments(int64_t N, int asked, int64_t* cells_per_seg) {
    const int64_t chunks = cdiv64(N, TR_TC);
    int64_t s = asked > 0 ? asked : imin64(cdiv64(N, 512), 32);
    s = imin64(s, chunks);
    const int64_t cps = cdiv64(chunks, s) * TR_TC;
    if (cells_per_seg) *cells_per_seg = cps;
    return (int)cdiv64(N, cps);
}

static int64_t tr_params(int Z, int L, int H) { return (int64_t)L * (Z + 1) + (int64_t)H * (L + 1) + 3 * (int64_t)H * (H + 1); }

// dZ6 .. dZ10 (float32, whole 8 bytes), then the segments' partials (fp64)
size_t tr_ws_bytes(int64_t N, int Z, int L, int H, int asked) {
    const unsigned __int128 dz = ((unsigned __int128)N * (unsigned __int128)(L + 4 * (int64_t)H) + 1) / 2 * 8;
    return bytes_or_0(dz + (unsigned __int128)8 * (unsigned __int128)tr_segments(N, asked, nullptr) * (unsigned __int128)tr_params(Z, L, H));
}

int launch_decoder_trunk_grads(int64_t N, int Z, int L, int H, const float* const* act, const int64_t* ld, const float* const* W,
                               const float* gd10, int64_t ldg, int segments, void* ws, float* const* grads, float* gzin, int64_t ldgz,
                               hipStream_t st) {
    TrChain ch;
    const int width[6] = {Z, L, H, H, H, H};
    float* dz = static_cast<float*>(ws);
    for (int l = 0; l < 6; ++l) { ch.act[l] = act[l]; ch.ld[l] = ld[l]; ch.width[l] = width[l]; }
    for (int l = 0; l < 5; ++l) {
        ch.W[l] = W[l];
        ch.dz[l] = dz;
        dz += N * width[l + 1];
    }
    hipLaunchKernelGGL(k_tr_chain, dim3((unsigned)cdiv64(N, TR_TC)), dim3(256), 0, st, ch, N, gd10, ldg, gzin, ldgz);
    HIP_LAUNCH_CHECK("k_tr_chain");

    int64_t cps = TR_TC;
    const int nseg = tr_segments(N, segments, &cps);
    const int64_t P = tr_params(Z, L, H);
    double* part = reinterpret_cast<double*>(static_cast<char*>(ws) + (N * (L + 4 * (int64_t)H) + 1) / 2 * 8);
    TrLayers tl;
    TrOut out;
    int64_t poff = 0;
    int tiles = 0;
    for (int l = 0; l < 5; ++l) {
        const int O = width[l + 1], K = width[l];
        const int kb = (K + TR_TK - 1) / TR_TK;
        tl.l[l] = TrLayer{ch.dz[l], act[l], ld[l], poff, O, K, tiles, kb};
        tiles += ((O + TR_TO - 1) / TR_TO) * kb;
        out.p[2 * l] = grads[2 * l];
        out.p[2 * l + 1] = grads[2 * l + 1];
        out.end[2 * l] = poff + (int64_t)O * K;
        out.end[2 * l + 1] = poff = poff + (int64_t)O * K + O;
    }
    hipLaunchKernelGGL(k_tr_dw, dim3((unsigned)tiles, (unsigned)nseg), dim3(256), 0, st, tl, N, cps, P, part);
    HIP_LAUNCH_CHECK("k_tr_dw");
    hipLaunchKernelGGL(k_tr_finish, dim3((unsigned)cdiv64(P, 256)), dim3(256), 0, st, part, nseg, P, out);
    HIP_LAUNCH_CHECK("k_tr_finish");
    return 0;
}

}  // namespace mmvae

// Augmenter training: the training-mode forward of Augmenter_smartseq (mmidas/augmentation/udagan.py:311-329) and one step of
// the reference's train_augmenter (mmidas/augmentation/train.py:10-157, MSE mode) on the device.
//
// In that loop only lambda[3] * 0.5 * mse_loss(fake_data2, real_data) has a gradient with respect to netA (every other term
// reaches netA through `0. * fake_data` followed by an in-place fill: exact zeros), so a step is
//   [statistics pass: one training-mode forward that only moves the BatchNorm running statistics]
//   forward (batch statistics), loss = weight * mean((x_aug - x)^2), backward through all 29 tensors, Adam.
//
// Every Linear layer -- the eleven large ones and the three of the latent block (noise, fc_mu, fc_sigma) -- is three products
// on the planes x planes engine (gemm_pp.hip, three exact bf16 slices, fp32 results):
//   forward  Y  = X W^T      A = planes(X)    [B rows, K]   B = planes(W)    [N rows, K]
//   dX          = dY W       A = planes(dY)   [B rows, N]   B = planes(W^T)  [K rows, N]
//   dW          = dY^T X     A = planes(dY^T) [N rows, B]   B = planes(X^T)  [K rows, B]     (K of the product = the batch)
// k_at_planes writes an operand's planes from its fp32 matrix, straight or transposed, with the ReLU of a saved normalised
// activation applied on the way (only y^ = (y - mean) rstd is stored per layer: h = relu(y^) and the ReLU decision y^ > 0 both
// come from it).  fc5's input cat(h4, elu(bnz(noise(z)))) is materialised ([B][N3 + NZ]) so that fc5 is one Linear like the rest.
//
// Batch sums (BatchNorm statistics, the two sums of its backward, bias gradients, the loss) are fp64 sums in a fixed order
// (row slices summed by one block each, the slices' sums added in slice order):
// no atomics anywhere, results are bit-identical from run to run.
#include "common.hpp"

namespace mmvae {
namespace {

typedef unsigned int u32x4t __attribute__((ext_vector_type(4)));

constexpr int AT_NL = 14;    // Linear layers: 0..10 fc1..fc11, 11 fc_mu, 12 fc_sigma, 13 noise
constexpr int AT_NBN = 12;   // BatchNorms: 0..9 batch_fc1..batch_fc10, 10 batch_fc_mu, 11 bnz
enum { ACT_NONE = 0, ACT_RELU = 1, ACT_ELU = 2 };

struct ATLin { int N, K; int64_t w, b; };      // offsets into the flat parameter buffer; b < 0: no bias
struct ATLayout {
    ATLin lin[AT_NL];
    int64_t bnz_w, bnz_b, total;
    int bn_n[AT_NBN];
    int64_t rm[AT_NBN], rv[AT_NBN], run_total;
};

inline int64_t pad4(int64_t n) { return (n + 3) & ~(int64_t)3; }

ATLayout at_layout(const mmvae_aug_dims& d) {
    ATLayout L{};
    const int D = d.D, N1 = d.N1, N3 = d.N3, N5 = d.N5, Z = d.Z, NZ = d.NZ;
    const int NK[AT_NL][2] = {{N1, D}, {N1, N1}, {N3, N1}, {N3, N3}, {N5, N3 + NZ}, {N5, Z}, {N3, N5}, {N3, N3}, {N1, N3}, {N1, N1},
                              {D, N1}, {Z, N5}, {Z, N5}, {NZ, NZ}};
    for (int i = 0; i < AT_NL; ++i) { L.lin[i].N = NK[i][0]; L.lin[i].K = NK[i][1]; }
    int64_t off = 0;
    auto take = [&](int64_t n) { const int64_t o = off; off += pad4(n); return o; };
    auto lin = [&](int i, bool bias) {
        L.lin[i].w = take((int64_t)L.lin[i].N * L.lin[i].K);
        L.lin[i].b = bias ? take(L.lin[i].N) : -1;
    };
    // the order of Augmenter_smartseq.parameters()
    lin(13, false);
    L.bnz_w = take(NZ);
    L.bnz_b = take(NZ);
    for (int i = 0; i < 5; ++i) lin(i, true);
    lin(11, true);
    lin(12, true);
    for (int i = 5; i < 11; ++i) lin(i, true);
    L.total = off;
    const int bn[AT_NBN] = {N1, N1, N3, N3, N5, N5, N3, N3, N1, N1, Z, NZ};
    off = 0;
    for (int i = 0; i < AT_NBN; ++i) { L.bn_n[i] = bn[i]; L.rm[i] = take(bn[i]); L.rv[i] = take(bn[i]); }
    L.run_total = off;
    return L;
}

struct ATWs {       // offsets in floats
    int64_t ones, xd, z0s, y[10], c5, zl, mul, sgm, rstd, ga, gb, g2, gz1, gz2, s1, s2, part, cr, pa, pb, scratch, total;
    int64_t scratch_floats;
    int maxn;
};
constexpr int AT_MSE_BLOCKS = 1024;

ATWs at_ws_layout(const mmvae_aug_dims& d) {
    ATWs w{};
    const ATLayout L = at_layout(d);
    int64_t off = 0;
    auto take = [&](int64_t n) { const int64_t o = off; off += (n + 63) & ~(int64_t)63; return o; };
    const int64_t B = d.B;
    int maxn = 0;
    int64_t pa = 0, pb = 0;
    for (int i = 0; i < AT_NL; ++i) {
        const int N = L.lin[i].N, K = L.lin[i].K;
        maxn = N > maxn ? N : maxn;
        maxn = K > maxn ? K : maxn;
        const int64_t a3[3] = {tp_plane_elems(d.B, K), tp_plane_elems(d.B, N), tp_plane_elems(N, d.B)};
        const int64_t b3[3] = {tp_plane_elems(N, K), tp_plane_elems(K, N), tp_plane_elems(K, d.B)};
        for (int j = 0; j < 3; ++j) { pa = a3[j] > pa ? a3[j] : pa; pb = b3[j] > pb ? b3[j] : pb; }
    }
    w.maxn = maxn;
    w.ones = take(maxn);
    w.xd = take(B * d.D);
    w.z0s = take(B * d.NZ);
    for (int i = 0; i < 10; ++i) w.y[i] = take(B * L.bn_n[i]);
    w.c5 = take(B * (d.N3 + d.NZ));
    w.zl = take(B * d.NZ);
    w.mul = take(B * d.Z);
    w.sgm = take(B * d.Z);
    w.rstd = take(2 * (int64_t)AT_NBN * maxn);      // doubles
    w.ga = take(B * maxn);
    w.gb = take(B * maxn);
    w.g2 = take(B * d.N5);
    w.gz1 = take(B * d.Z);
    w.gz2 = take(B * d.Z);
    w.s1 = take(2 * (int64_t)maxn);                 // doubles
    w.s2 = take(2 * (int64_t)maxn);
    w.part = take(4 * (int64_t)AT_MSE_BLOCKS);      // [blocks] double + [blocks] int64
    w.cr = take(2 * 2 * (int64_t)64 * maxn);       // two arrays of [slices][maxn] doubles (stage 1 of the column sums)
    w.pa = take(3 * pa / 2);
    w.pb = take(3 * pb / 2);
    w.scratch_floats = pp_scratch_floats();
    w.scratch = take(w.scratch_floats);
    w.total = off;
    return w;
}

int at_check_dims(const mmvae_aug_dims* d) {
    if (!d) { set_error("aug dims is null"); return MMVAE_E_BADARG; }
    if (d->A != 1) { set_error("augmenter training: one arm (the non-batched forward)"); return MMVAE_E_UNSUPPORTED; }
    if (d->B < 2) { set_error("augmenter training: batch statistics need at least two rows"); return MMVAE_E_BADARG; }
    if (d->D < 4 || d->N1 < 1 || d->N3 < 1 || d->N5 < 1 || d->Z < 1 || d->NZ < 1) { set_error("aug dims: non-positive size"); return MMVAE_E_BADARG; }
    if (d->D % 4 != 0) { set_error("augmenter: input_dim must be a multiple of 4 (16-byte row loads of x)"); return MMVAE_E_UNSUPPORTED; }
    if (d->N5 > 128 || d->NZ > 128 || d->Z > 64) { set_error("augmenter: n_dim/5 and noise_dim <= 128, latent_dim <= 64"); return MMVAE_E_UNSUPPORTED; }
    const int m = d->B > d->D ? d->B : d->D;
    if (d->B > (1 << 20) || d->D > (1 << 20) || tp_plane_elems(m, m) * 2 >= ((int64_t)1 << 32)) {
        set_error("augmenter training: an operand plane stays below 4 GB");
        return MMVAE_E_UNSUPPORTED;
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------
// operand planes (gemm_pp.hip's layout [plane][KT][Rp][16] bf16) of an fp32 matrix, three exact slices.
//   TRANS = false: element (r, k) = src[r * ld + k];  TRANS = true: element (r, k) = src[k * ld + r];  r < R, k < K,
// zeros for K <= k < 16 KT; relu: max(., 0) on the way.  A thread owns one row's 16 k of one K step: 32 bytes per plane.
// Rows R <= r < Rp are not written: a row of A reaches only its own row of C, a row of B only its own column, and the engine
// stores neither for r >= R.
// ---------------------------------------------------------------------------------------------
template <bool TRANS>
__global__ __launch_bounds__(256) void k_at_planes(const float* __restrict__ src, int64_t ld, int R, int K, int relu,
                                                   unsigned short* __restrict__ dst, int64_t plane, int Rp, int KT) {
    const int64_t n = (int64_t)R * KT;
    for (int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x; id < n; id += (int64_t)gridDim.x * 256) {
        int r, kt;
        if (TRANS) { kt = (int)(id / R); r = (int)(id - (int64_t)kt * R); }
        else { r = (int)(id / KT); kt = (int)(id - (int64_t)r * KT); }
        float v[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int k = kt * 16 + i;
            float t = 0.f;
            if (k < K) t = TRANS ? src[(int64_t)k * ld + r] : src[(int64_t)r * ld + k];
            v[i] = relu ? fmaxf(t, 0.f) : t;
        }
        unsigned w[3][8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            unsigned s[3];
            split3(v[2 * i], v[2 * i + 1], s);
            w[0][i] = s[0]; w[1][i] = s[1]; w[2][i] = s[2];
        }
        unsigned short* const o = dst + ((int64_t)kt * Rp + r) * 16;
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            u32x4t lo, hi;
#pragma unroll
            for (int e = 0; e < 4; ++e) { lo[e] = w[p][e]; hi[e] = w[p][4 + e]; }
            *reinterpret_cast<u32x4t*>(o + p * plane) = lo;
            *reinterpret_cast<u32x4t*>(o + p * plane + 8) = hi;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// per-column batch sums in two stages: a block owns 32 columns of one slice of rows, its 8 row groups stride over the slice's
// rows with fp64 accumulators and their sums are added in group order; one thread a column then adds the slices in slice order.
// ---------------------------------------------------------------------------------------------
constexpr int CR_COLS = 32, CR_GROUPS = 8, CR_SLICES = 64;
__device__ __forceinline__ void cr_finish(double (*sh)[CR_GROUPS][CR_COLS], double a, double b, int c, int g, double& sa, double& sb) {
    sh[0][g][c] = a;
    sh[1][g][c] = b;
    __syncthreads();
    sa = 0.0;
    sb = 0.0;
    if (g == 0)
        for (int i = 0; i < CR_GROUPS; ++i) { sa += sh[0][i][c]; sb += sh[1][i][c]; }
}

// (the element-wise arithmetic between two stored fp32 values runs in fp64 and rounds once, where it is stored)
__device__ __forceinline__ double act_grad(int act, float yh, float gamma, float beta) {
    if (act == ACT_RELU) return yh > 0.f ? 1.0 : 0.0;
    if (act == ACT_ELU) { const double zb = (double)yh * (double)gamma + (double)beta; return zb > 0.0 ? 1.0 : exp(zb); }
    return 1.0;
}

// Stage 1 of a column sum: grid (ceil(N / 32), S); slice s owns rows [s rps, (s + 1) rps) and writes its sums to pa / pb [s][N].
//   CR_STATS: a = y, b = y^2;  CR_BWD: a = g0 = dH act'(.), b = g0 y^;  CR_COLSUM: a = dY
enum { CR_STATS = 0, CR_BWD = 1, CR_COLSUM = 2 };
template <int MODE>
__global__ __launch_bounds__(256) void k_at_colred(const float* __restrict__ p, int64_t ldp, const float* __restrict__ yh, int64_t ldy, int B, int N,
                                                   int rps, int act, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                   double* __restrict__ pa, double* __restrict__ pb) {
    __shared__ double sh[2][CR_GROUPS][CR_COLS];
    const int c = threadIdx.x & 31, g = threadIdx.x >> 5, col = blockIdx.x * CR_COLS + c;
    const int r0 = blockIdx.y * rps, r1 = min(B, r0 + rps);
    double a = 0.0, b = 0.0;
    if (col < N) {
        const float ga = (MODE == CR_BWD && gamma) ? gamma[col] : 1.f, be = (MODE == CR_BWD && beta) ? beta[col] : 0.f;
        for (int r = r0 + g; r < r1; r += CR_GROUPS) {
            const float v = p[(int64_t)r * ldp + col];
            if (MODE == CR_STATS) { a += (double)v; b += (double)v * (double)v; }
            else if (MODE == CR_BWD) {
                const float y = yh[(int64_t)r * ldy + col];
                const double g0 = (double)v * act_grad(act, y, ga, be);
                a += g0;
                b += g0 * (double)y;
            } else a += (double)v;
        }
    }
    double sa, sb;
    cr_finish(sh, a, b, c, g, sa, sb);
    if (g == 0 && col < N) {
        pa[(int64_t)blockIdx.y * N + col] = sa;
        if (MODE != CR_COLSUM) pb[(int64_t)blockIdx.y * N + col] = sb;
    }
}

// Stage 2: the slices' sums added in slice order, one thread a column, and what the sums are for:
//   CR_STATS: batch mean and biased variance -> s1 = mean, s2 = rstd = 1 / sqrt(var + eps) (fp64); running statistics with the unbiased variance
//   CR_BWD: s1, s2 (for an affine BatchNorm also d beta, d gamma);  CR_COLSUM: out = the sum (a bias gradient)
template <int MODE>
__global__ __launch_bounds__(256) void k_at_colred_finish(const double* __restrict__ pa, const double* __restrict__ pb, int S, int N, int B,
                                                          float eps, float mom, float* __restrict__ rm, float* __restrict__ rv,
                                                          int64_t* __restrict__ nbt, float* __restrict__ o1, float* __restrict__ o2,
                                                          double* __restrict__ s1, double* __restrict__ s2) {
    const int col = blockIdx.x * 256 + threadIdx.x;
    if (MODE == CR_STATS && col == 0) nbt[0] += 1;
    if (col >= N) return;
    double sa = 0.0, sb = 0.0;
    for (int s = 0; s < S; ++s) {
        sa += pa[(int64_t)s * N + col];
        if (MODE != CR_COLSUM) sb += pb[(int64_t)s * N + col];
    }
    if (MODE == CR_STATS) {
        const double mean = sa / B;
        double var = sb / B - mean * mean;
        var = var > 0.0 ? var : 0.0;
        s1[col] = mean;
        s2[col] = 1.0 / sqrt(var + (double)eps);
        rm[col] = (float)((1.0 - (double)mom) * (double)rm[col] + (double)mom * mean);
        rv[col] = (float)((1.0 - (double)mom) * (double)rv[col] + (double)mom * var * ((double)B / (double)(B - 1)));
    } else if (MODE == CR_BWD) {
        s1[col] = sa;
        s2[col] = sb;
        if (o1) { o1[col] = (float)sb; o2[col] = (float)sa; }      // d gamma, d beta
    } else {
        o1[col] = (float)sa;
    }
}

// y <- y^ = (y - mean) rstd in place; out2 (optional) = act(y^ gamma + beta) (gamma null: y^)
__global__ __launch_bounds__(256) void k_at_bn_apply(float* __restrict__ y, int64_t ld, int B, int N, const double* __restrict__ mean,
                                                     const double* __restrict__ rstd, const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, float* __restrict__ out2, int64_t ld2, int act) {
    const int64_t n = (int64_t)B * N;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / N;
        const int c = (int)(i - r * N);
        const double yh = ((double)y[r * ld + c] - mean[c]) * rstd[c];
        y[r * ld + c] = (float)yh;
        if (out2) {
            double v = gamma ? yh * (double)gamma[c] + (double)beta[c] : yh;
            if (act == ACT_RELU) v = v > 0.0 ? v : 0.0;
            else if (act == ACT_ELU) v = v > 0.0 ? v : expm1(v);
            out2[r * ld2 + c] = (float)v;
        }
    }
}

// dH <- dY = rstd gamma (g0 - s1 / B - y^ s2 / B) in place
__global__ __launch_bounds__(256) void k_at_bn_bwd_apply(float* __restrict__ dh, int64_t ldh, const float* __restrict__ yh, int64_t ldy, int B,
                                                         int N, int act, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                         const double* __restrict__ rstd, const double* __restrict__ s1,
                                                         const double* __restrict__ s2) {
    const int64_t n = (int64_t)B * N;
    const double inv = 1.0 / (double)B;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / N;
        const int c = (int)(i - r * N);
        const float ga = gamma ? gamma[c] : 1.f, be = beta ? beta[c] : 0.f;
        const float y = yh[r * ldy + c];
        const double g0 = (double)dh[r * ldh + c] * act_grad(act, y, ga, be);
        dh[r * ldh + c] = (float)(rstd[c] * (double)ga * (g0 - s1[c] * inv - (double)y * (s2[c] * inv)));
    }
}

// ---------------------------------------------------------------------------------------------
// element-wise pieces
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_at_fill(float* __restrict__ p, int n, float v) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = v;
}
// xd = x mask / (1 - p) (nn.Dropout in training mode); z0s = scale z0
__global__ __launch_bounds__(256) void k_at_inputs(const float* __restrict__ x, const uint8_t* __restrict__ mask, float inv_keep, int64_t n,
                                                   float* __restrict__ xd, const float* __restrict__ z0, float scale, int64_t nz,
                                                   float* __restrict__ z0s) {
    const int64_t m = n > nz ? n : nz;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < m; i += (int64_t)gridDim.x * 256) {
        if (i < n) xd[i] = mask[i] ? x[i] * inv_keep : 0.f;
        if (i < nz) z0s[i] = scale * z0[i];
    }
}
// sigma = sigmoid(sg) in place, s = eps sigma + mu^   (aug_utils.py:51-65)
__global__ __launch_bounds__(256) void k_at_reparam(float* __restrict__ sg, const float* __restrict__ mu, const float* __restrict__ eps, int64_t n,
                                                    float* __restrict__ s) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double sig = 1.0 / (1.0 + exp(-(double)sg[i]));
    sg[i] = (float)sig;
    s[i] = (float)((double)eps[i] * sig + (double)mu[i]);
}
// d mu^ = ds;  d(fc_sigma's output) = ds eps sigma (1 - sigma)
__global__ __launch_bounds__(256) void k_at_reparam_bwd(const float* __restrict__ ds, int64_t ldds, int B, int Z, const float* __restrict__ eps,
                                                        const float* __restrict__ sig, float* __restrict__ dmu, float* __restrict__ dsg) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)B * Z) return;
    const int64_t r = i / Z;
    const float g = ds[r * ldds + (i - r * Z)];
    const double sv = (double)sig[i];
    dmu[i] = g;
    dsg[i] = (float)((double)g * (double)eps[i] * sv * (1.0 - sv));
}
// a[r][c] += b[r][c], both [B][N] with their own pitch
__global__ __launch_bounds__(256) void k_at_add(float* __restrict__ a, int64_t lda, const float* __restrict__ b, int64_t ldb, int B, int N) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)B * N) return;
    const int64_t r = i / N, c = i - r * N;
    a[r * lda + c] += b[r * ldb + c];
}
// the loss: per-block fp64 sums of (x_aug - x)^2 and counts of (x_aug > 1e-3) != (x > 1e-4); dY11 = coef (x_aug - x) [x_aug > 0]
__global__ __launch_bounds__(256) void k_at_mse(const float* __restrict__ xa, const float* __restrict__ x, int64_t n, float coef,
                                                float* __restrict__ dy, double* __restrict__ psum, long long* __restrict__ pcnt) {
    __shared__ double ss[256];
    __shared__ long long sc[256];
    double a = 0.0;
    long long m = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float v = xa[i], t = x[i], df = v - t;
        a += (double)df * (double)df;
        m += ((v > 1e-3f) != (t > 1e-4f)) ? 1 : 0;
        if (dy) dy[i] = v > 0.f ? coef * df : 0.f;
    }
    ss[threadIdx.x] = a;
    sc[threadIdx.x] = m;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (threadIdx.x < h) { ss[threadIdx.x] += ss[threadIdx.x + h]; sc[threadIdx.x] += sc[threadIdx.x + h]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { psum[blockIdx.x] = ss[0]; pcnt[blockIdx.x] = sc[0]; }
}
// out = [mse, mismatch, recon_loss = (mse + 100 mismatch / n) / 2]
__global__ __launch_bounds__(256) void k_at_mse_final(const double* __restrict__ psum, const long long* __restrict__ pcnt, int nb, int64_t n,
                                                      double* __restrict__ out) {
    __shared__ double ss[256];
    __shared__ long long sc[256];
    double a = 0.0;
    long long m = 0;
    for (int i = threadIdx.x; i < nb; i += 256) { a += psum[i]; m += pcnt[i]; }
    ss[threadIdx.x] = a;
    sc[threadIdx.x] = m;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (threadIdx.x < h) { ss[threadIdx.x] += ss[threadIdx.x + h]; sc[threadIdx.x] += sc[threadIdx.x + h]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double mse = ss[0] / (double)n, mis = (double)sc[0];
        out[0] = mse;
        out[1] = mis;
        out[2] = 0.5 * (mse + 100.0 * mis / (double)n);
    }
}

inline unsigned ew_blocks(int64_t n) { return (unsigned)imin64(cdiv64(n, 256), 16384); }

// ---------------------------------------------------------------------------------------------
// one call's context
// ---------------------------------------------------------------------------------------------
struct AT {
    mmvae_aug_dims d;
    ATLayout L;
    ATWs W;
    hipStream_t s;
    float* params;
    float* running;
    int64_t* nbt;
    float* w;          // workspace
    float* grads;
    int force;
    int n_gemm;

    // column sums: the batch in at most CR_SLICES slices of at least 64 rows
    int slices() const { const int n = cdiv(d.B, 64); return n < CR_SLICES ? n : CR_SLICES; }
    int rps() const { return cdiv(d.B, slices()); }
    double* cr_a() const { return reinterpret_cast<double*>(w + W.cr); }
    double* cr_b() const { return reinterpret_cast<double*>(w + W.cr) + (int64_t)CR_SLICES * W.maxn; }
    TPlanes pa(int R, int K) const { return tp_make(reinterpret_cast<unsigned short*>(w + W.pa), R, K); }
    TPlanes pb(int R, int K) const { return tp_make(reinterpret_cast<unsigned short*>(w + W.pb), R, K); }

    int planes(bool trans, const float* src, int64_t ld, int R, int K, bool relu, const TPlanes& t) const {
        const unsigned blocks = ew_blocks((int64_t)R * t.KT);
        if (trans) hipLaunchKernelGGL(k_at_planes<true>, dim3(blocks), dim3(256), 0, s, src, ld, R, K, relu ? 1 : 0, t.p, t.plane, t.Rp, t.KT);
        else hipLaunchKernelGGL(k_at_planes<false>, dim3(blocks), dim3(256), 0, s, src, ld, R, K, relu ? 1 : 0, t.p, t.plane, t.Rp, t.KT);
        HIP_LAUNCH_CHECK("k_at_planes");
        return 0;
    }
    // C [M][N] = relu?(A B^T + bias) from the operand planes; each launch names its own flag slot, the slots are zeroed every
    // PP_FLAG_SLOTS launches
    int gemm(const TPlanes& a, const TPlanes& b, int M, int N, const float* bias, bool relu, float* out, int64_t ldo) {
        const int slot = n_gemm % PP_FLAG_SLOTS;
        if (slot == 0)
            if (int rc = launch_pp_zero_flags(s, w + W.scratch)) return rc;
        ++n_gemm;
        return launch_pp_gemm(s, 3, a, b, M, N, w + W.ones, bias, bias != nullptr, relu, out, ldo, N, nullptr, w + W.scratch, W.scratch_floats,
                              slot, force);
    }
    int lin_fwd(int l, const float* x, int64_t ldx, bool relu_in, float* out, int64_t ldo, bool relu_out) {
        const ATLin& g = L.lin[l];
        const TPlanes a = pa(d.B, g.K), b = pb(g.N, g.K);
        if (int rc = planes(false, x, ldx, d.B, g.K, relu_in, a)) return rc;
        if (int rc = planes(false, params + g.w, g.K, g.N, g.K, false, b)) return rc;
        return gemm(a, b, d.B, g.N, g.b >= 0 ? params + g.b : nullptr, relu_out, out, ldo);
    }
    int bn_fwd(int bn, float* y, int64_t ld, float eps, float mom, const float* gamma, const float* beta, float* out2, int64_t ld2, int act) {
        const int N = L.bn_n[bn];
        double* const mean = reinterpret_cast<double*>(w + W.s1);      // (the backward's sums are not live during the forward)
        double* const rstd = reinterpret_cast<double*>(w + W.rstd) + (int64_t)bn * W.maxn;
        hipLaunchKernelGGL(k_at_colred<CR_STATS>, dim3(cdiv(N, CR_COLS), slices()), dim3(256), 0, s, y, ld, nullptr, 0, d.B, N, rps(), 0, nullptr,
                           nullptr, cr_a(), cr_b());
        hipLaunchKernelGGL(k_at_colred_finish<CR_STATS>, dim3(cdiv(N, 256)), dim3(256), 0, s, cr_a(), cr_b(), slices(), N, d.B, eps, mom,
                           running + L.rm[bn], running + L.rv[bn], nbt + bn, nullptr, nullptr, mean, rstd);
        hipLaunchKernelGGL(k_at_bn_apply, dim3(ew_blocks((int64_t)d.B * N)), dim3(256), 0, s, y, ld, d.B, N, mean, rstd, gamma, beta, out2, ld2, act);
        HIP_LAUNCH_CHECK("k_at_bn");
        return 0;
    }
    int bn_bwd(int bn, float* dh, int64_t ldh, const float* yh, int64_t ldy, int act, const float* gamma, const float* beta, float* dgamma,
               float* dbeta) {
        const int N = L.bn_n[bn];
        double* const s1 = reinterpret_cast<double*>(w + W.s1);
        double* const s2 = reinterpret_cast<double*>(w + W.s2);
        const double* rstd = reinterpret_cast<const double*>(w + W.rstd) + (int64_t)bn * W.maxn;
        hipLaunchKernelGGL(k_at_colred<CR_BWD>, dim3(cdiv(N, CR_COLS), slices()), dim3(256), 0, s, dh, ldh, yh, ldy, d.B, N, rps(), act, gamma, beta,
                           cr_a(), cr_b());
        hipLaunchKernelGGL(k_at_colred_finish<CR_BWD>, dim3(cdiv(N, 256)), dim3(256), 0, s, cr_a(), cr_b(), slices(), N, d.B, 0.f, 0.f, nullptr,
                           nullptr, nullptr, dgamma, dbeta, s1, s2);
        hipLaunchKernelGGL(k_at_bn_bwd_apply, dim3(ew_blocks((int64_t)d.B * N)), dim3(256), 0, s, dh, ldh, yh, ldy, d.B, N, act, gamma, beta, rstd,
                           s1, s2);
        HIP_LAUNCH_CHECK("k_at_bn_bwd");
        return 0;
    }
    // db, dW into grads; dX (optional) = dY W
    int lin_bwd(int l, const float* dy, int64_t ldy, const float* x, int64_t ldx, bool relu_x, float* dx, int64_t lddx) {
        const ATLin& g = L.lin[l];
        if (g.b >= 0) {
            hipLaunchKernelGGL(k_at_colred<CR_COLSUM>, dim3(cdiv(g.N, CR_COLS), slices()), dim3(256), 0, s, dy, ldy, nullptr, 0, d.B, g.N, rps(), 0,
                               nullptr, nullptr, cr_a(), cr_b());
            hipLaunchKernelGGL(k_at_colred_finish<CR_COLSUM>, dim3(cdiv(g.N, 256)), dim3(256), 0, s, cr_a(), cr_b(), slices(), g.N, d.B, 0.f, 0.f,
                               nullptr, nullptr, nullptr, grads + g.b, nullptr, nullptr, nullptr);
            HIP_LAUNCH_CHECK("k_at_colsum");
        }
        {
            const TPlanes a = pa(g.N, d.B), b = pb(g.K, d.B);
            if (int rc = planes(true, dy, ldy, g.N, d.B, false, a)) return rc;
            if (int rc = planes(true, x, ldx, g.K, d.B, relu_x, b)) return rc;
            if (int rc = gemm(a, b, g.N, g.K, nullptr, false, grads + g.w, g.K)) return rc;
        }
        if (dx) {
            const TPlanes a = pa(d.B, g.N), b = pb(g.K, g.N);
            if (int rc = planes(false, dy, ldy, d.B, g.N, false, a)) return rc;
            if (int rc = planes(true, params + g.w, g.K, g.K, g.N, false, b)) return rc;
            if (int rc = gemm(a, b, d.B, g.K, nullptr, false, dx, lddx)) return rc;
        }
        return 0;
    }

    int forward(const float* x, const uint8_t* mask, float p_drop, const float* z0, const float* eps_n, float scale, float* s_out, float* x_aug) {
        const int B = d.B, D = d.D, N1 = d.N1, N3 = d.N3, N5 = d.N5, Z = d.Z, NZ = d.NZ, C5 = N3 + NZ;
        const float bn_eps = 1e-10f, bn_mom = 0.01f;          // udagan.py:221-281
        int rc;
        hipLaunchKernelGGL(k_at_fill, dim3(cdiv(W.maxn, 256)), dim3(256), 0, s, w + W.ones, W.maxn, 1.f);
        hipLaunchKernelGGL(k_at_inputs, dim3(ew_blocks((int64_t)B * (D > NZ ? D : NZ))), dim3(256), 0, s, x, mask, 1.f / (1.f - p_drop), (int64_t)B * D, w + W.xd,
                           z0, scale, (int64_t)B * NZ, w + W.z0s);
        HIP_LAUNCH_CHECK("k_at_inputs");
        float* y[10];
        for (int i = 0; i < 10; ++i) y[i] = w + W.y[i];
        float* const c5 = w + W.c5;
        // z = elu(bnz(noise(scale z0))) into the right part of fc5's input (bnz: nn.BatchNorm1d defaults)
        if ((rc = lin_fwd(13, w + W.z0s, NZ, false, w + W.zl, NZ, false))) return rc;
        if ((rc = bn_fwd(11, w + W.zl, NZ, 1e-5f, 0.1f, params + L.bnz_w, params + L.bnz_b, c5 + N3, C5, ACT_ELU))) return rc;
        if ((rc = lin_fwd(0, w + W.xd, D, false, y[0], N1, false))) return rc;
        if ((rc = bn_fwd(0, y[0], N1, bn_eps, bn_mom, nullptr, nullptr, nullptr, 0, ACT_NONE))) return rc;
        if ((rc = lin_fwd(1, y[0], N1, true, y[1], N1, false))) return rc;
        if ((rc = bn_fwd(1, y[1], N1, bn_eps, bn_mom, nullptr, nullptr, nullptr, 0, ACT_NONE))) return rc;
        if ((rc = lin_fwd(2, y[1], N1, true, y[2], N3, false))) return rc;
        if ((rc = bn_fwd(2, y[2], N3, bn_eps, bn_mom, nullptr, nullptr, nullptr, 0, ACT_NONE))) return rc;
        if ((rc = lin_fwd(3, y[2], N3, true, y[3], N3, false))) return rc;
        if ((rc = bn_fwd(3, y[3], N3, bn_eps, bn_mom, nullptr, nullptr, c5, C5, ACT_RELU))) return rc;       // h4 into fc5's input
        if ((rc = lin_fwd(4, c5, C5, false, y[4], N5, false))) return rc;
        if ((rc = bn_fwd(4, y[4], N5, bn_eps, bn_mom, nullptr, nullptr, nullptr, 0, ACT_NONE))) return rc;
        if ((rc = lin_fwd(11, y[4], N5, true, w + W.mul, Z, false))) return rc;
        if ((rc = bn_fwd(10, w + W.mul, Z, bn_eps, bn_mom, nullptr, nullptr, nullptr, 0, ACT_NONE))) return rc;
        if ((rc = lin_fwd(12, y[4], N5, true, w + W.sgm, Z, false))) return rc;
        hipLaunchKernelGGL(k_at_reparam, dim3(cdiv(B * Z, 256)), dim3(256), 0, s, w + W.sgm, w + W.mul, eps_n, (int64_t)B * Z, s_out);
        HIP_LAUNCH_CHECK("k_at_reparam");
        if ((rc = lin_fwd(5, s_out, Z, false, y[5], N5, false))) return rc;
        if ((rc = bn_fwd(5, y[5], N5, bn_eps, bn_mom, nullptr, nullptr, nullptr, 0, ACT_NONE))) return rc;
        const int wid[10] = {N1, N1, N3, N3, N5, N5, N3, N3, N1, N1};
        for (int l = 6; l < 10; ++l) {
            if ((rc = lin_fwd(l, y[l - 1], wid[l - 1], true, y[l], wid[l], false))) return rc;
            if ((rc = bn_fwd(l, y[l], wid[l], bn_eps, bn_mom, nullptr, nullptr, nullptr, 0, ACT_NONE))) return rc;
        }
        return lin_fwd(10, y[9], N1, true, x_aug, D, true);
    }

    // needs forward's saved activations; grads: every tensor overwritten
    int backward(const float* x, const float* eps_n, float weight, const float* s_out, const float* x_aug, double* loss_out) {
        const int B = d.B, D = d.D, N1 = d.N1, N3 = d.N3, N5 = d.N5, Z = d.Z, NZ = d.NZ, C5 = N3 + NZ;
        const int64_t n = (int64_t)B * D;
        int rc;
        float* ga = w + W.ga;
        float* gb = w + W.gb;
        float* y[10];
        for (int i = 0; i < 10; ++i) y[i] = w + W.y[i];
        double* const psum = reinterpret_cast<double*>(w + W.part);
        long long* const pcnt = reinterpret_cast<long long*>(w + W.part + 2 * AT_MSE_BLOCKS);
        const int nb = (int)imin64(cdiv64(n, 256), AT_MSE_BLOCKS);
        hipLaunchKernelGGL(k_at_mse, dim3(nb), dim3(256), 0, s, x_aug, x, n, 2.f * weight / (float)n, ga, psum, pcnt);
        hipLaunchKernelGGL(k_at_mse_final, dim3(1), dim3(256), 0, s, psum, pcnt, nb, n, loss_out);
        HIP_LAUNCH_CHECK("k_at_mse");
        const int wid[10] = {N1, N1, N3, N3, N5, N5, N3, N3, N1, N1};
        if ((rc = lin_bwd(10, ga, D, y[9], N1, true, gb, N1))) return rc;
        float* cur = gb;
        float* oth = ga;
        for (int l = 9; l >= 5; --l) {
            if ((rc = bn_bwd(l, cur, wid[l], y[l], wid[l], ACT_RELU, nullptr, nullptr, nullptr, nullptr))) return rc;
            if (l > 5) { if ((rc = lin_bwd(l, cur, wid[l], y[l - 1], wid[l - 1], true, oth, wid[l - 1]))) return rc; }
            else if ((rc = lin_bwd(5, cur, N5, s_out, Z, false, oth, Z))) return rc;
            float* t = cur; cur = oth; oth = t;
        }
        // cur: ds [B][Z]
        float* const gz1 = w + W.gz1;
        float* const gz2 = w + W.gz2;
        hipLaunchKernelGGL(k_at_reparam_bwd, dim3(cdiv(B * Z, 256)), dim3(256), 0, s, cur, Z, B, Z, eps_n, w + W.sgm, gz1, gz2);
        HIP_LAUNCH_CHECK("k_at_reparam_bwd");
        if ((rc = bn_bwd(10, gz1, Z, w + W.mul, Z, ACT_NONE, nullptr, nullptr, nullptr, nullptr))) return rc;
        if ((rc = lin_bwd(11, gz1, Z, y[4], N5, true, cur, N5))) return rc;
        if ((rc = lin_bwd(12, gz2, Z, y[4], N5, true, w + W.g2, N5))) return rc;
        hipLaunchKernelGGL(k_at_add, dim3(cdiv(B * N5, 256)), dim3(256), 0, s, cur, N5, w + W.g2, N5, B, N5);
        HIP_LAUNCH_CHECK("k_at_add");
        if ((rc = bn_bwd(4, cur, N5, y[4], N5, ACT_RELU, nullptr, nullptr, nullptr, nullptr))) return rc;
        if ((rc = lin_bwd(4, cur, N5, w + W.c5, C5, false, oth, C5))) return rc;
        // oth: d cat(h4, z) [B][N3 + NZ]: the noise branch (bnz is affine: d gamma, d beta), then the trunk
        if ((rc = bn_bwd(11, oth + N3, C5, w + W.zl, NZ, ACT_ELU, params + L.bnz_w, params + L.bnz_b, grads + L.bnz_w, grads + L.bnz_b))) return rc;
        if ((rc = lin_bwd(13, oth + N3, C5, w + W.z0s, NZ, false, nullptr, 0))) return rc;
        if ((rc = bn_bwd(3, oth, C5, y[3], N3, ACT_RELU, nullptr, nullptr, nullptr, nullptr))) return rc;
        if ((rc = lin_bwd(3, oth, C5, y[2], N3, true, cur, N3))) return rc;
        if ((rc = bn_bwd(2, cur, N3, y[2], N3, ACT_RELU, nullptr, nullptr, nullptr, nullptr))) return rc;
        if ((rc = lin_bwd(2, cur, N3, y[1], N1, true, oth, N1))) return rc;
        if ((rc = bn_bwd(1, oth, N1, y[1], N1, ACT_RELU, nullptr, nullptr, nullptr, nullptr))) return rc;
        if ((rc = lin_bwd(1, oth, N1, y[0], N1, true, cur, N1))) return rc;
        if ((rc = bn_bwd(0, cur, N1, y[0], N1, ACT_RELU, nullptr, nullptr, nullptr, nullptr))) return rc;
        return lin_bwd(0, cur, N1, w + W.xd, D, false, nullptr, 0);
    }
};

int at_make(AT& c, const mmvae_aug_dims* d, float* params, float* running, int64_t* nbt, void* ws, size_t ws_bytes, const mmvae_exec* ex,
            void* stream) {
    if (int rc = at_check_dims(d)) return rc;
    c.d = *d;
    c.L = at_layout(*d);
    c.W = at_ws_layout(*d);
    if (!params || !running || !nbt || !ws) { set_error("aug_train: null argument"); return MMVAE_E_BADARG; }
    if (ws_bytes < (size_t)c.W.total * sizeof(float)) { set_error("aug_train: workspace too small"); return MMVAE_E_WORKSPACE; }
    if (reinterpret_cast<uintptr_t>(ws) & 15) { set_error("aug_train: the workspace is 16-byte aligned"); return MMVAE_E_BADARG; }
    c.s = reinterpret_cast<hipStream_t>(stream);
    c.params = params;
    c.running = running;
    c.nbt = nbt;
    c.w = reinterpret_cast<float*>(ws);
    c.grads = nullptr;
    c.force = ex ? ex->tune[MMVAE_TUNE_AUG_TILE] : 0;
    c.n_gemm = 0;
    return 0;
}

}  // namespace
}  // namespace mmvae

using namespace mmvae;

extern "C" {

int mmvae_aug_param_layout(const mmvae_aug_dims* d, mmvae_aug_train_layout* out) {
    if (int rc = at_check_dims(d)) return rc;
    if (!out) { set_error("aug_param_layout: null argument"); return MMVAE_E_BADARG; }
    const ATLayout L = at_layout(*d);
    const ATWs W = at_ws_layout(*d);
    for (int i = 0; i < AT_NL; ++i) { out->w_off[i] = L.lin[i].w; out->b_off[i] = L.lin[i].b; out->rows[i] = L.lin[i].N; out->cols[i] = L.lin[i].K; }
    out->bnz_w_off = L.bnz_w;
    out->bnz_b_off = L.bnz_b;
    out->total = L.total;
    for (int i = 0; i < AT_NBN; ++i) { out->rm_off[i] = L.rm[i]; out->rv_off[i] = L.rv[i]; out->bn_n[i] = L.bn_n[i]; }
    out->run_total = L.run_total;
    for (int i = 0; i < 10; ++i) out->act_off[i] = W.y[i];
    return 0;
}

size_t mmvae_aug_train_workspace_bytes(const mmvae_aug_dims* d) {
    if (at_check_dims(d)) return 0;
    return (size_t)at_ws_layout(*d).total * sizeof(float);
}

int mmvae_aug_train_forward(const mmvae_aug_dims* d, float* params, float* running, int64_t* nbt, const float* x, const uint8_t* mask,
                            float p_drop, const float* z0, const float* eps_n, float scale, void* ws, size_t ws_bytes, float* s_out,
                            float* x_aug, const mmvae_exec* ex, void* stream) {
    AT c;
    if (int rc = at_make(c, d, params, running, nbt, ws, ws_bytes, ex, stream)) return rc;
    if (!x || !mask || !z0 || !eps_n || !s_out || !x_aug) { set_error("aug_train_forward: null argument"); return MMVAE_E_BADARG; }
    if (!(p_drop >= 0.f && p_drop < 1.f)) { set_error("aug_train_forward: p_drop in [0, 1)"); return MMVAE_E_BADARG; }
    return c.forward(x, mask, p_drop, z0, eps_n, scale, s_out, x_aug);
}

int mmvae_aug_train_step(const mmvae_aug_dims* d, float* params, float* running, int64_t* nbt, const float* x, const uint8_t* mask,
                         float p_drop, const float* z0, const float* eps_n, const uint8_t* stat_mask, const float* stat_z0,
                         const float* stat_eps, float scale, float weight, void* ws, size_t ws_bytes, float* grads, float* s_out,
                         float* x_aug, double* loss_out, int do_adam, float* exp_avg, float* exp_avg_sq, int64_t step, float lr,
                         float beta1, float beta2, float adam_eps, float weight_decay, const mmvae_exec* ex, void* stream) {
    AT c;
    if (int rc = at_make(c, d, params, running, nbt, ws, ws_bytes, ex, stream)) return rc;
    if (!x || !mask || !z0 || !eps_n || !s_out || !x_aug || !grads || !loss_out) { set_error("aug_train_step: null argument"); return MMVAE_E_BADARG; }
    if (!(p_drop >= 0.f && p_drop < 1.f)) { set_error("aug_train_step: p_drop in [0, 1)"); return MMVAE_E_BADARG; }
    if (do_adam && (!exp_avg || !exp_avg_sq || step < 1)) { set_error("aug_train_step: Adam needs its moments and step >= 1"); return MMVAE_E_BADARG; }
    c.grads = grads;
    if (stat_mask) {
        if (!stat_z0 || !stat_eps) { set_error("aug_train_step: the statistics pass needs its own noise"); return MMVAE_E_BADARG; }
        if (int rc = c.forward(x, stat_mask, p_drop, stat_z0, stat_eps, scale, s_out, x_aug)) return rc;
    }
    if (int rc = c.forward(x, mask, p_drop, z0, eps_n, scale, s_out, x_aug)) return rc;
    if (int rc = c.backward(x, eps_n, weight, s_out, x_aug, loss_out)) return rc;
    if (do_adam)
        return mmvae_adam_step(c.L.total, params, grads, exp_avg, exp_avg_sq, step, lr, beta1, beta2, adam_eps, weight_decay, 0, stream);
    return 0;
}

}  // extern "C"

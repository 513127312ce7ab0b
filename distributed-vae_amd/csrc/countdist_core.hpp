// Count distributions, the per-element core (mmidas/utils/distributions.py; include/mmvae.h).
// Everything here is __host__ __device__ and fp64: the kernels of countdist.hip and the host-only debug entries run the same
// text, and tests/countdist_restatement.py restates it in numpy decision for decision.  The translation unit is built with
// -ffp-contract=off: a product and a sum are two roundings, as they are in numpy.
#pragma once
#include "common.hpp"

namespace mmvae {

enum { CD_NB = 0, CD_ZINB = 1, CD_MIX = 2 };                       // the likelihood's kind
enum { CD_ST_GAMMA = 0, CD_ST_BOOST = 1, CD_ST_POISSON = 2, CD_ST_INFL = 3 };   // the stage of a draw's Philox counter
enum { CD_ZI_NONE = 0, CD_ZI_LOGIT = 1, CD_ZI_PROB = 2 };
constexpr int CD_ATTEMPTS = 64;        // attempts of a rejection sampler at most
constexpr int CD_INV_KMAX = 64;        // sequential inversion stops here: P(Poisson(10) > 64) < 1e-29
constexpr double CD_LAM_MAX = 1e8;     // the reference's clamp of the Poisson mean
constexpr double CD_LAM_PTRS = 10.0;   // below: inversion; from here: PTRS

#define CD_HD __host__ __device__ inline
// The likelihood functions stay real calls on the device: inlined into k_cd_logp they take 240-250 registers (two waves a
// SIMD), as calls 90-105 (four or five), and the kernel waits on the VALU's fp64 latency.  (The sampler's functions were
// tried the same way and gained nothing: their reference argument goes through scratch.)
#define CD_CALL __host__ __device__ __attribute__((noinline)) inline

// ---- likelihoods ----
// log(1 + exp(a)) without a threshold: max(a, 0) + log1p(exp(-|a|))
CD_HD double cd_softplus(double a) { return fmax(a, 0.0) + log1p(exp(-fabs(a))); }

// log_nb_positive, the reference's evaluation order
CD_CALL double cd_log_nb(double x, double mu, double th, double eps) {
    const double ltm = log(th + mu + eps);
    return th * (log(th + eps) - ltm) + x * (log(mu + eps) - ltm) + lgamma(x + th) - lgamma(th) - lgamma(x + 1.0);
}

// log_zinb_positive: only the branch that x < eps or x > eps selects; x == eps gives 0 (the reference's two masks are both 0
// there), a NaN x gives NaN
CD_CALL double cd_log_zinb(double x, double mu, double th, double pi, double eps) {
    const double sp = cd_softplus(-pi);
    const double ltm = log(th + mu + eps);
    const double ptl = -pi + th * (log(th + eps) - ltm);
    if (x < eps) return cd_softplus(ptl) - sp;
    if (x > eps) return -sp + ptl + x * (log(mu + eps) - ltm) + lgamma(x + th) - lgamma(th) - lgamma(x + 1.0);
    return x == eps ? 0.0 : x;
}

// log_mixture_nb: logsumexp(l1, l2 - pi) about its maximum, minus softplus(-pi)
CD_CALL double cd_log_mix(double x, double mu1, double mu2, double th1, double th2, double pi, double eps) {
    const double l1 = cd_log_nb(x, mu1, th1, eps), b = cd_log_nb(x, mu2, th2, eps) - pi;
    const double m = fmax(l1, b);
    // equal infinities: the difference is NaN where the sum is the infinity itself
    const double lse = (l1 == b) ? m + log(2.0) : m + log1p(exp(-fabs(l1 - b)));
    return lse - cd_softplus(-pi);
}

// ---- the sampler ----
// Counter of a draw: words 0, 1 = the low and high word of the element's logical index (cell0 + row) D + gene; word 2 =
// (stage + 4 attempt) ^ (offset_hi << 8); word 3 = offset_lo; key = seed.  stage < 4 and attempt < 64 fill the low 8 bits,
// offset < 2^56 the rest.
CD_HD u32x4 cd_words(uint64_t idx, uint64_t seed, uint64_t off, int stage, int attempt) {
    return philox4x32((uint32_t)idx, (uint32_t)(idx >> 32), (uint32_t)(stage + 4 * attempt) ^ ((uint32_t)(off >> 32) << 8), (uint32_t)off,
                      (uint32_t)seed, (uint32_t)(seed >> 32));
}
// Words to uniforms, both exact in fp64 and strictly inside (0, 1):
//   u52(lo, hi) = (((hi << 32 | lo) >> 12) + 0.5) 2^-52        u32(w) = (w + 0.5) 2^-32
CD_HD double cd_u52(uint32_t lo, uint32_t hi) { return ((double)((((uint64_t)hi << 32) | lo) >> 12) + 0.5) * (1.0 / 4503599627370496.0); }
CD_HD double cd_u32(uint32_t w) { return ((double)w + 0.5) * (1.0 / 4294967296.0); }

// Gamma(shape, 1), shape >= 1, Marsaglia-Tsang without the squeeze.  Attempt t takes one call: the normal is the Box-Muller
// cosine n = sqrt(-2 log u52(w0, w1)) cos(2 pi u32(w2)), the accept uniform u32(w3).  With y = c n the candidate is d (1 + y)^3
// and the accept test log u < n^2 / 2 + d - d v + d log v is evaluated as n^2 / 2 + d (3 log1p(y) - y (3 + y (3 + y))),
// which does not cancel at a large d.  Exhausted: the mean, shape.
CD_HD double cd_gamma(double shape, uint64_t idx, uint64_t seed, uint64_t off, int& exhausted) {
    const double d = shape - 1.0 / 3.0, c = 1.0 / sqrt(9.0 * d);
    for (int t = 0; t < CD_ATTEMPTS; ++t) {
        const u32x4 w = cd_words(idx, seed, off, CD_ST_GAMMA, t);
        const double n = sqrt(-2.0 * log(cd_u52(w.x, w.y))) * cos(6.283185307179586 * cd_u32(w.z));
        const double y = c * n;
        if (y <= -1.0) continue;
        if (log(cd_u32(w.w)) < 0.5 * n * n + d * (3.0 * log1p(y) - y * (3.0 + y * (3.0 + y)))) {
            const double v1 = 1.0 + y;
            return d * (v1 * v1 * v1);
        }
    }
    exhausted = 1;
    return shape;
}

// Poisson(lam), 0 <= lam < 10: sequential inversion of u = u52(w0, w1) of the call (poisson, attempt 0), up to k = 64
CD_HD double cd_poisson_inv(double lam, uint64_t idx, uint64_t seed, uint64_t off, int& exhausted) {
    const u32x4 w = cd_words(idx, seed, off, CD_ST_POISSON, 0);
    const double u = cd_u52(w.x, w.y);
    double p = exp(-lam), s = p;
    int k = 0;
    while (u > s) {
        if (k == CD_INV_KMAX) { exhausted = 1; return floor(lam); }
        ++k;
        p = p * lam / (double)k;
        s = s + p;
    }
    return (double)k;
}

// Poisson(lam), lam >= 10: Hoermann's PTRS (1993).  Attempt t takes U = u52(w0, w1) - 0.5 and V = u52(w2, w3) of the call
// (poisson, t).  Exhausted: floor(lam).
CD_HD double cd_poisson_ptrs(double lam, uint64_t idx, uint64_t seed, uint64_t off, int& exhausted) {
    const double slam = sqrt(lam), loglam = log(lam);
    const double b = 0.931 + 2.53 * slam, a = -0.059 + 0.02483 * b;
    const double invalpha = 1.1239 + 1.1328 / (b - 3.4), vr = 0.9277 - 3.6224 / (b - 2.0);
    for (int t = 0; t < CD_ATTEMPTS; ++t) {
        const u32x4 w = cd_words(idx, seed, off, CD_ST_POISSON, t);
        const double U = cd_u52(w.x, w.y) - 0.5, V = cd_u52(w.z, w.w);
        const double us = 0.5 - fabs(U);
        const double k = floor((2.0 * a / us + b) * U + lam + 0.43);
        if (us >= 0.07 && V <= vr) return k;
        if (k < 0.0 || (us < 0.013 && V > us)) continue;
        if (log(V) + log(invalpha) - log(a / (us * us) + b) <= -lam + k * loglam - lgamma(k + 1.0)) return k;
    }
    exhausted = 1;
    return floor(lam);
}

// One draw of NB(mu, theta) or ZINB(mu, theta, zp): w ~ Gamma(theta, rate theta / mu), count ~ Poisson(min(w, 1e8)), 0 where
// u <= zp.  NaN for parameters outside the support (mu < 0, theta <= 0, not finite, zp NaN), before any loop; mu = 0 gives 0.
// zi_kind: CD_ZI_NONE, or zi is a logit (zp = 1 / (1 + exp(-zi))) or the probability itself.
CD_HD double cd_draw(double mu, double th, double zi, int zi_kind, uint64_t idx, uint64_t seed, uint64_t off, int& exhausted) {
    if (!(mu >= 0.0) || !(th > 0.0) || mu > 1.7976931348623157e308 || th > 1.7976931348623157e308 || (zi_kind != CD_ZI_NONE && zi != zi))
        return NAN;
    if (mu == 0.0) return 0.0;
    double g = cd_gamma(th < 1.0 ? th + 1.0 : th, idx, seed, off, exhausted);
    if (th < 1.0) {                                      // Gamma(theta) = Gamma(theta + 1) U^(1 / theta)
        const u32x4 w = cd_words(idx, seed, off, CD_ST_BOOST, 0);
        g = g * exp(log(cd_u52(w.x, w.y)) / th);
    }
    const double lam = fmin(g / (th / mu), CD_LAM_MAX);
    double k = lam < CD_LAM_PTRS ? cd_poisson_inv(lam, idx, seed, off, exhausted) : cd_poisson_ptrs(lam, idx, seed, off, exhausted);
    if (zi_kind != CD_ZI_NONE) {
        const double zp = zi_kind == CD_ZI_LOGIT ? 1.0 / (1.0 + exp(-zi)) : zi;
        const u32x4 w = cd_words(idx, seed, off, CD_ST_INFL, 0);
        if (cd_u52(w.x, w.y) <= zp) k = 0.0;
    }
    return k;
}

// (mu, theta, z) of the model's three heads under zinb_loss's eps guards: theta = r = x_rec + eps, p = (1 - eps)(x_p + eps),
// mu = r p / (1 - p), z = (1 - eps)(x_r + eps), from the float32 heads in fp64
CD_HD void cd_heads_to_params(float x_rec, float x_p, float x_r, double eps, double& mu, double& th, double& z) {
    th = (double)x_rec + eps;
    const double p = (1.0 - eps) * ((double)x_p + eps);
    mu = th * p / (1.0 - p);
    z = (1.0 - eps) * ((double)x_r + eps);
}

// what one element of the output holds: the count as float32 (log1p of it on request) or as int32, -1 for NaN
CD_HD void cd_store(void* out, int64_t at, double k, int out_int32, int want_log1p) {
    if (out_int32) static_cast<int32_t*>(out)[at] = k != k ? -1 : (int32_t)k;
    else static_cast<float*>(out)[at] = (float)(want_log1p ? log1p(k) : k);
}

}  // namespace mmvae

// The ZINB term of one element, its gates and its gradient (mmidas/nn_model.py: zinb_loss :642-676; DESIGN.md sections 9k,
// 9m; include/mmvae.h).  Everything here is __host__ __device__ and fp64: the kernels of zinb.hip and zinb_grad.hip and the
// host-only debug entries run the same text.  tests/zinb_grad_restatement.py restates the gradient in torch.
#pragma once
#include "common.hpp"

namespace mmvae {

#define ZB_HD __host__ __device__ inline

// One element's term.  r = x_rec + eps, p and z the two probabilities after the eps guard, q = 1 - p, y = 1 - z.  Only the
// branch that [X > 0] selects is evaluated (the reference multiplies the other by an exact 0, which differs only where that
// other branch is not finite).
ZB_HD double zinb_term(double X, double r, double p, double q, double z, double y) {
    if (X > 0.0) {
        const double k = exp(X) - 1.0;
        return -lgamma(k + r) + lgamma(r) - k * log(p) - r * log(q) - log(y);
    }
    return -log(z + y * exp(r * log(q)));
}

// sigmoid(a) after the guard, and one minus it, from the pre-activation: with e = exp(-|a|) the larger of s, 1 - s is
// 1 / (1 + e) and the smaller e / (1 + e), neither formed by a cancelling subtraction;
// 1 - (1 - eps)(s + eps) = (1 - eps)(1 - s) + eps^2.
ZB_HD void zb_gate(float a, double eps, double& p, double& q) {
    const double e = exp(-fabs((double)a));
    const double big = 1.0 / (1.0 + e), small = e * big;
    const double s = a >= 0.f ? big : small, c = a >= 0.f ? small : big;
    p = (1.0 - eps) * (s + eps);
    q = (1.0 - eps) * c + eps * eps;
}

// d p / d a of zb_gate: (1 - eps) s (1 - s), the two factors formed as zb_gate forms them
ZB_HD double zb_gate_slope(float a, double eps) {
    const double e = exp(-fabs((double)a));
    const double big = 1.0 / (1.0 + e);
    return (1.0 - eps) * (big * (e * big));
}

// psi(x), x > 0: the recurrence psi(x) = psi(x + 1) - 1 / x up to ZB_PSI_SERIES, the asymptotic series from there on:
// psi(x) ~ log x - 1 / (2 x) - sum_n B_2n / (2 n x^2n), through x^-14; the first term left out is 3617 / (8160 x^16),
// below 5e-17 at x >= 10.  The reciprocals of the recurrence are added from the largest argument down to the smallest, so
// that the pole's 1 / x at a tiny x meets a sum that is already complete.  x = +inf gives +inf, x = 0 the pole's -inf, and
// a negative x, -inf or a NaN gives NaN: the reflection is not built (r = x_rec + eps of a given head may be anything, and
// the recurrence must not be walked up from there), so the loop below never takes more than ZB_PSI_STEPS steps.
constexpr double ZB_PSI_SERIES = 10.0;
constexpr int ZB_PSI_STEPS = 10;
ZB_HD double zb_digamma(double x) {
    if (!(x > 0.0)) return x == 0.0 ? -HUGE_VAL : NAN;
    int n = 0;
    while (n < ZB_PSI_STEPS && x + n < ZB_PSI_SERIES) ++n;
    const double xs = x + n;
    double rec = 0.0;
    for (int i = n - 1; i >= 0; --i) rec += 1.0 / (x + i);
    const double v = 1.0 / (xs * xs);
    const double tail = v * (1.0 / 12.0 - v * (1.0 / 120.0 - v * (1.0 / 252.0 - v * (1.0 / 240.0 - v * (1.0 / 132.0 - v * (691.0 / 32760.0 - v * (1.0 / 12.0)))))));
    return (log(xs) - 0.5 / xs - tail) - rec;
}

// The gradient of zinb_term with respect to r, p and z (q and y move with p and z: d q = -d p, d y = -d z), for the
// selected branch only.
//   X > 0:   d/dr = -psi(k + r) + psi(r) - log q     d/dp = -k / p + r / q          d/dz = 1 / y
//   X <= 0:  with w = q^r = exp(r log q), u = z + y w
//            d/dr = -y w log q / u                    d/dp = y r w / (q u)           d/dz = expm1(r log q) / u
ZB_HD void zinb_term_grad(double X, double r, double p, double q, double z, double y, double& gr, double& gp, double& gz) {
    const double lq = log(q);
    if (X > 0.0) {
        const double k = exp(X) - 1.0;
        gr = -zb_digamma(k + r) + zb_digamma(r) - lq;
        gp = -k / p + r / q;
        gz = 1.0 / y;
        return;
    }
    const double w = exp(r * lq), u = z + y * w;
    gr = -(y * w * lq) / u;
    gp = (y * r * w) / (q * u);
    gz = expm1(r * lq) / u;
}

// One element of the kernels on d10: what zinb_term reads, from X and the float32 pre-activations of the three heads.
// r = relu(a_rec) + eps; the gates of a_p and a_r.
struct ZbOperands {
    double x, r, p, q, z, y;
};
ZB_HD ZbOperands zb_operands(float X, float a_rec, float a_p, float a_r, double eps) {
    ZbOperands o;
    zb_gate(a_p, eps, o.p, o.q);
    zb_gate(a_r, eps, o.z, o.y);
    o.x = (double)X;
    o.r = (double)fmaxf(a_rec, 0.f) + eps;
    return o;
}
ZB_HD double zinb_term(const ZbOperands& o) { return zinb_term(o.x, o.r, o.p, o.q, o.z, o.y); }

// g = d term / d (a_rec, a_p, a_r) of that element in fp64, before any rounding: zinb_term_grad through the relu's and the
// gates' slopes.  Returns the operands, from which zinb_term gives the element's term (two lgamma: the caller asks for it or
// not).  The one body of the gradient kernels (zinb_grad.hip: zg_element) and of the host's restatement (host_zinb_grad).
ZB_HD ZbOperands zinb_element_grad(float X, float a_rec, float a_p, float a_r, double eps, double (&g)[3]) {
    const ZbOperands o = zb_operands(X, a_rec, a_p, a_r, eps);
    double gr, gp, gz;
    zinb_term_grad(o.x, o.r, o.p, o.q, o.z, o.y, gr, gp, gz);
    g[0] = a_rec > 0.f ? gr : 0.0;
    g[1] = gp * zb_gate_slope(a_p, eps);
    g[2] = gz * zb_gate_slope(a_r, eps);
    return o;
}

}  // namespace mmvae

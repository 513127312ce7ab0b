"""Host restatement of the count distributions (numpy fp64 only): the three scVI likelihoods, the NB / ZINB sampler step for
step on the Philox stream of include/mmvae.h ("count distributions"), the exact NB / ZINB pmf and Pearson's statistic.

Likelihoods.  The truth of a term is the reference's formula (mmidas/utils/distributions.py) in fp64, in the reference's order
of operations, except for the two cancellation-free forms the library states: softplus(a) = max(a, 0) + log1p(exp(-|a|)) (no
switch to the identity above 20) and the two-term logsumexp about its maximum.  ``magnitudes_*`` give M_e, the sum of the
absolute values of the formula's addends with every product multiplied out (theta log(theta + eps) and theta log(theta + mu +
eps) count separately: their difference cancels when mu << theta).

Sampler.  ``sample`` follows csrc/countdist_core.hpp decision for decision and returns, per element, the draw and the smallest
relative margin among the comparisons taken on the way -- each |lhs - rhs| over the sum of the magnitudes of the addends on
both sides (for a plain a < b: max(|a|, |b|)), the distance of a PTRS candidate to the next integer over max(1, |candidate|),
|lam - 10| / 10 for the choice of the Poisson algorithm.  An element whose margin is below 1e-9 is one that another fp64 libm
(log, exp, cos, lgamma differ by ulps between numpy and the device) may decide differently.
"""
import math

import numpy as np

from noise_restatement import key_of, philox4x32_10

ST_GAMMA, ST_BOOST, ST_POISSON, ST_INFL = 0, 1, 2, 3
ATTEMPTS, INV_KMAX, LAM_MAX, LAM_PTRS = 64, 64, 1e8, 10.0
_LO = np.uint64(0xFFFFFFFF)

lgamma = np.vectorize(math.lgamma, otypes=[np.float64])


# ---- likelihoods -----------------------------------------------------------------------------------------------------------------
def softplus(a):
    a = np.asarray(a, dtype=np.float64)
    return np.maximum(a, 0.0) + np.log1p(np.exp(-np.abs(a)))


def _f64(*arrays):
    return [None if a is None else np.asarray(a, dtype=np.float64) for a in arrays]


def log_nb(x, mu, theta, eps=1e-8):
    x, mu, theta = _f64(x, mu, theta)
    ltm = np.log(theta + mu + eps)
    return theta * (np.log(theta + eps) - ltm) + x * (np.log(mu + eps) - ltm) + lgamma(x + theta) - lgamma(theta) - lgamma(x + 1.0)


def magnitudes_nb(x, mu, theta, eps=1e-8):
    x, mu, theta = _f64(x, mu, theta)
    ltm = np.abs(np.log(theta + mu + eps))
    return (np.abs(theta * np.log(theta + eps)) + np.abs(theta) * ltm + np.abs(x * np.log(mu + eps)) + np.abs(x) * ltm
            + np.abs(lgamma(x + theta)) + np.abs(lgamma(theta)) + np.abs(lgamma(x + 1.0)))


def log_zinb(x, mu, theta, pi, eps=1e-8):
    x, mu, theta, pi = _f64(x, mu, theta, pi)
    sp = softplus(-pi)
    ltm = np.log(theta + mu + eps)
    ptl = -pi + theta * (np.log(theta + eps) - ltm)
    zero = softplus(ptl) - sp
    pos = -sp + ptl + x * (np.log(mu + eps) - ltm) + lgamma(x + theta) - lgamma(theta) - lgamma(x + 1.0)
    return np.where(x < eps, zero, np.where(x > eps, pos, np.where(x == eps, 0.0, np.nan)))


def magnitudes_zinb(x, mu, theta, pi, eps=1e-8):
    x, mu, theta, pi = _f64(x, mu, theta, pi)
    sp = softplus(-pi)
    ltm = np.abs(np.log(theta + mu + eps))
    ptl_m = np.abs(pi) + np.abs(theta * np.log(theta + eps)) + np.abs(theta) * ltm
    ptl = -pi + theta * (np.log(theta + eps) - np.log(theta + mu + eps))
    zero = ptl_m + softplus(ptl) + sp
    pos = (ptl_m + sp + np.abs(x * np.log(mu + eps)) + np.abs(x) * ltm + np.abs(lgamma(x + theta)) + np.abs(lgamma(theta))
           + np.abs(lgamma(x + 1.0)))
    return np.where(x < eps, zero, np.where(x > eps, pos, 0.0))


def log_mixture(x, mu1, mu2, theta1, theta2, pi, eps=1e-8):
    x, mu1, mu2, theta1, theta2, pi = _f64(x, mu1, mu2, theta1, theta2, pi)
    l1 = log_nb(x, mu1, theta1, eps)
    b = log_nb(x, mu2, theta1 if theta2 is None else theta2, eps) - pi
    return np.maximum(l1, b) + np.log1p(np.exp(-np.abs(l1 - b))) - softplus(-pi)


def magnitudes_mixture(x, mu1, mu2, theta1, theta2, pi, eps=1e-8):
    x, mu1, mu2, theta1, theta2, pi = _f64(x, mu1, mu2, theta1, theta2, pi)
    th2 = theta1 if theta2 is None else theta2
    l1, b = log_nb(x, mu1, theta1, eps), log_nb(x, mu2, th2, eps) - pi
    return (magnitudes_nb(x, mu1, theta1, eps) + magnitudes_nb(x, mu2, th2, eps) + np.abs(pi) + np.maximum(np.abs(l1), np.abs(b))
            + np.log1p(np.exp(-np.abs(l1 - b))) + softplus(-pi))


# ---- the sampler -----------------------------------------------------------------------------------------------------------------
def words(idx, seed, offset, stage, attempt):
    """uint32 [n, 4]: the Philox call of elements ``idx`` (uint64 [n]) at (stage, attempt)."""
    idx = np.asarray(idx, dtype=np.uint64)
    offset = int(offset)
    w2 = ((stage + 4 * attempt) ^ (((offset >> 32) << 8) & 0xFFFFFFFF)) & 0xFFFFFFFF
    c = np.stack([idx & _LO, idx >> np.uint64(32), np.full_like(idx, w2), np.full_like(idx, offset & 0xFFFFFFFF)], axis=-1)
    return philox4x32_10(c, key_of(seed)).reshape(-1, 4)


def u52(lo, hi):
    a = (hi.astype(np.uint64) << np.uint64(32)) | lo.astype(np.uint64)
    return ((a >> np.uint64(12)).astype(np.float64) + 0.5) * 2.0 ** -52


def u32(w):
    return (w.astype(np.float64) + 0.5) * 2.0 ** -32


def _rel(a, b):
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.abs(a - b) / np.maximum(np.abs(a), np.abs(b))


class _State:
    def __init__(self, n):
        self.margin = np.full(n, np.inf)
        self.calls = np.zeros(n, dtype=np.int64)
        self.exhausted = np.zeros(n, dtype=bool)

    def note(self, at, m):
        self.margin[at] = np.minimum(self.margin[at], m)


def _gamma(shape, at, idx, seed, offset, st):
    """Gamma(shape, 1) for shape >= 1 (Marsaglia-Tsang); ``at`` are the elements' positions in the state arrays."""
    d = shape - 1.0 / 3.0
    c = 1.0 / np.sqrt(9.0 * d)
    res = shape.copy()
    pend = np.arange(shape.size)
    for t in range(ATTEMPTS):
        if pend.size == 0:
            break
        w = words(idx[pend], seed, offset, ST_GAMMA, t)
        st.calls[at[pend]] += 1
        n = np.sqrt(-2.0 * np.log(u52(w[:, 0], w[:, 1]))) * np.cos(6.283185307179586 * u32(w[:, 2]))
        y = c[pend] * n
        rej = y <= -1.0
        st.note(at[pend], np.abs(y + 1.0) / np.maximum(1.0, np.abs(y)))
        ys = np.where(rej, 0.0, y)
        l1p, poly, dd = np.log1p(ys), ys * (3.0 + ys * (3.0 + ys)), d[pend]
        lhs = np.log(u32(w[:, 3]))
        rhs = 0.5 * n * n + dd * (3.0 * l1p - poly)
        scale = np.abs(lhs) + 0.5 * n * n + dd * (3.0 * np.abs(l1p) + np.abs(poly))
        st.note(at[pend], np.where(rej, np.inf, np.abs(lhs - rhs) / scale))
        acc = ~rej & (lhs < rhs)
        v1 = 1.0 + y[acc]
        res[pend[acc]] = dd[acc] * (v1 * v1 * v1)
        pend = pend[~acc]
    st.exhausted[at[pend]] = True
    return res


def _poisson_inv(lam, at, idx, seed, offset, st):
    w = words(idx, seed, offset, ST_POISSON, 0)
    st.calls[at] += 1
    u = u52(w[:, 0], w[:, 1])
    p = np.exp(-lam)
    s = p.copy()
    k = np.zeros(lam.size)
    st.note(at, _rel(u, s))
    active = u > s
    for _ in range(INV_KMAX):
        i = np.flatnonzero(active)
        if i.size == 0:
            break
        k[i] += 1.0
        p[i] = p[i] * lam[i] / k[i]
        s[i] = s[i] + p[i]
        st.note(at[i], _rel(u[i], s[i]))
        active[i] = u[i] > s[i]
    st.exhausted[at[active]] = True
    return np.where(active, np.floor(lam), k)


def _poisson_ptrs(lam, at, idx, seed, offset, st):
    slam, loglam = np.sqrt(lam), np.log(lam)
    b = 0.931 + 2.53 * slam
    a = -0.059 + 0.02483 * b
    invalpha = 1.1239 + 1.1328 / (b - 3.4)
    vr = 0.9277 - 3.6224 / (b - 2.0)
    res = np.floor(lam)
    pend = np.arange(lam.size)
    for t in range(ATTEMPTS):
        if pend.size == 0:
            break
        w = words(idx[pend], seed, offset, ST_POISSON, t)
        st.calls[at[pend]] += 1
        U, V = u52(w[:, 0], w[:, 1]) - 0.5, u52(w[:, 2], w[:, 3])
        us = 0.5 - np.abs(U)
        ap, bp, lp = a[pend], b[pend], lam[pend]
        val = (2.0 * ap / us + bp) * U + lp + 0.43
        k = np.floor(val)
        st.note(at[pend], np.minimum(val - k, k + 1.0 - val) / np.maximum(1.0, np.abs(val)))
        wide = us >= 0.07
        st.note(at[pend], np.abs(us - 0.07) / 0.07)
        st.note(at[pend], np.where(wide, _rel(V, vr[pend]), np.inf))
        quick = wide & (V <= vr[pend])
        rest = ~quick
        st.note(at[pend], np.where(rest, np.abs(us - 0.013) / 0.013, np.inf))
        narrow = us < 0.013
        st.note(at[pend], np.where(rest & (k >= 0.0) & narrow, _rel(V, us), np.inf))
        again = rest & ((k < 0.0) | (narrow & (V > us)))
        test = rest & ~again
        kk = np.where(test, k, 0.0)
        t1, t2, t3 = np.log(V), np.log(invalpha[pend]), np.log(ap / (us * us) + bp)
        r2, r3 = kk * loglam[pend], lgamma(kk + 1.0)
        lhs, rhs = t1 + t2 - t3, -lp + r2 - r3
        st.note(at[pend], np.where(test, np.abs(lhs - rhs) / (np.abs(t1) + np.abs(t2) + np.abs(t3) + lp + np.abs(r2) + np.abs(r3)), np.inf))
        acc = quick | (test & (lhs <= rhs))
        res[pend[acc]] = k[acc]
        pend = pend[~acc]
    st.exhausted[at[pend]] = True
    return res


def heads_to_params(x_rec, x_p, x_r, eps=1e-6):
    """(mu, theta, z) of the model's float32 heads under zinb_loss's eps guards, in fp64."""
    x_rec, x_p, x_r = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in (x_rec, x_p, x_r))
    th = x_rec + eps
    p = (1.0 - eps) * (x_p + eps)
    return th * p / (1.0 - p), th, (1.0 - eps) * (x_r + eps)


def sample(mu, theta, zi=None, zi_kind=None, seed=0, offset=0, cell0=0):
    """One draw per element of mu [n, D] (theta [D] or [n, D]; zi with zi_kind "logits" or "probs" for ZINB), all taken as
    fp64 values.  Returns {"draw": float64 [n, D] (NaN for invalid parameters), "margin": [n, D], "calls": Philox calls per
    element [n, D], "exhausted": the number of elements that ran out of attempts}."""
    mu = np.asarray(mu, dtype=np.float64)
    n, D = mu.shape
    shape2 = mu.shape
    th = np.broadcast_to(np.asarray(theta, dtype=np.float64), shape2).reshape(-1)
    mu = mu.reshape(-1)
    z = None if zi is None else np.broadcast_to(np.asarray(zi, dtype=np.float64), shape2).reshape(-1)
    idx = ((np.uint64(cell0) + np.arange(n, dtype=np.uint64))[:, None] * np.uint64(D) + np.arange(D, dtype=np.uint64)[None, :]).reshape(-1)
    st = _State(mu.size)
    out = np.full(mu.size, np.nan)
    with np.errstate(invalid="ignore"):
        valid = (mu >= 0.0) & (th > 0.0) & np.isfinite(mu) & np.isfinite(th)
    if z is not None:
        valid &= ~np.isnan(z)
    out[valid & (mu == 0.0)] = 0.0
    at = np.flatnonzero(valid & (mu > 0.0))
    if at.size:
        t, m, ix = th[at], mu[at], idx[at]
        g = _gamma(np.where(t < 1.0, t + 1.0, t), at, ix, seed, offset, st)
        small = np.flatnonzero(t < 1.0)
        if small.size:
            w = words(ix[small], seed, offset, ST_BOOST, 0)
            st.calls[at[small]] += 1
            with np.errstate(under="ignore"):
                g[small] = g[small] * np.exp(np.log(u52(w[:, 0], w[:, 1])) / t[small])
        lam = np.minimum(g / (t / m), LAM_MAX)
        st.note(at, np.abs(lam - LAM_PTRS) / LAM_PTRS)
        k = np.empty(at.size)
        lo = lam < LAM_PTRS
        if lo.any():
            k[lo] = _poisson_inv(lam[lo], at[lo], ix[lo], seed, offset, st)
        if (~lo).any():
            k[~lo] = _poisson_ptrs(lam[~lo], at[~lo], ix[~lo], seed, offset, st)
        if z is not None:
            zz = z[at]
            zp = 1.0 / (1.0 + np.exp(-zz)) if zi_kind == "logits" else zz
            w = words(ix, seed, offset, ST_INFL, 0)
            st.calls[at] += 1
            u = u52(w[:, 0], w[:, 1])
            st.note(at, _rel(u, zp))
            k = np.where(u <= zp, 0.0, k)
        out[at] = k
    return {"draw": out.reshape(shape2), "margin": st.margin.reshape(shape2), "calls": st.calls.reshape(shape2),
            "exhausted": int(st.exhausted.sum())}


# ---- the exact pmf and Pearson's statistic ---------------------------------------------------------------------------------------
def nb_logpmf(k, mu, theta):
    """log P(K = k) of NB(mu, theta) via math.lgamma, the two logarithms as log1p of a ratio."""
    return (math.lgamma(k + theta) - math.lgamma(theta) - math.lgamma(k + 1.0) - theta * math.log1p(mu / theta)
            - k * math.log1p(theta / mu))


def zinb_pmf_table(mu, theta, z=0.0, tail=1e-10, kmax=4_000_000):
    """P(K = k) for k = 0 .. K of ZINB(mu, theta, zero-inflation probability z), K the first k behind which less than ``tail``
    of the mass is left."""
    p, cum, k = [], 0.0, 0
    while cum < 1.0 - tail and k < kmax:
        v = math.exp(nb_logpmf(float(k), mu, theta))
        p.append(v)
        cum += v
        k += 1
    p = (1.0 - z) * np.array(p)
    p[0] += z
    return p


def pearson(values, counts, pmf, min_expected=20.0):
    """(statistic, dof) of a histogram (``counts[i]`` draws of value ``values[i]``) against ``pmf`` [K + 1]: consecutive values
    are pooled from 0 upwards until a bin expects ``min_expected`` draws; what is left at the top (the pmf's tail beyond K
    included) joins the last bin."""
    values, counts = np.asarray(values, dtype=np.int64), np.asarray(counts, dtype=np.float64)
    n = counts.sum()
    obs_k = np.zeros(pmf.size)
    inside = values < pmf.size
    np.add.at(obs_k, values[inside], counts[inside])
    over = counts[~inside].sum()
    exp_bins, obs_bins, e, o = [], [], 0.0, 0.0
    for k in range(pmf.size):
        e += n * pmf[k]
        o += obs_k[k]
        if e >= min_expected:
            exp_bins.append(e)
            obs_bins.append(o)
            e = o = 0.0
    e += n * max(0.0, 1.0 - float(pmf.sum()))
    o += over
    if exp_bins:
        exp_bins[-1] += e
        obs_bins[-1] += o
    else:
        exp_bins, obs_bins = [e], [o]
    E, O = np.array(exp_bins), np.array(obs_bins)
    return float(((O - E) ** 2 / E).sum()), len(E) - 1


def wilson_hilferty_gate(dof):
    """The chi-square quantile at six normal deviations by Wilson-Hilferty: dof (1 - 2 / (9 dof) + 6 sqrt(2 / (9 dof)))^3."""
    return dof * (1.0 - 2.0 / (9.0 * dof) + 6.0 * math.sqrt(2.0 / (9.0 * dof))) ** 3


def histogram(draws):
    """(values, counts) of an array of non-negative integer draws."""
    v, c = np.unique(np.asarray(draws).astype(np.int64).reshape(-1), return_counts=True)
    return v, c

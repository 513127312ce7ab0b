"""The rank-sum test of every gene restated in numpy alone (no scipy, no torch): what mmvae_rank_sum and
utils/marker_analysis.py must give.

Per gene: ``np.sort`` of the column, ``searchsorted`` left and right for lo (values below) and hi (values not above), twice the
mid-rank = lo + hi + 1, integer sums per group, run lengths of the sorted column for the tie term.  numpy compares -0.0 and
+0.0 equal and orders the infinities, which is the kernel's contract.  The sums of the values are ``np.longdouble``."""
import math

import numpy as np


def rank_sums(x, codes, n_groups, eps=0.0):
    """x [n, D] (any float dtype, no NaN), codes int [n] in [0, n_groups) ->
    (rank_sum2 int64 [G, D], tie_term int64 [D], n_pos int64 [G, D], sum longdouble [G, D], sum_abs longdouble [G, D])."""
    x = np.asarray(x)
    codes = np.asarray(codes)
    n, D = x.shape
    r2 = np.zeros((n_groups, D), dtype=np.int64)
    tie = np.zeros(D, dtype=np.int64)
    pos = np.zeros((n_groups, D), dtype=np.int64)
    tot = np.zeros((n_groups, D), dtype=np.longdouble)
    tot_abs = np.zeros((n_groups, D), dtype=np.longdouble)
    eps32 = np.float32(eps)
    for d in range(D):
        col = x[:, d]
        s = np.sort(col)
        lo = np.searchsorted(s, col, side="left").astype(np.int64)
        hi = np.searchsorted(s, col, side="right").astype(np.int64)
        twice = lo + hi + 1
        starts = np.flatnonzero(np.concatenate([[True], s[1:] != s[:-1]]))
        t = np.diff(np.concatenate([starts, [n]])).astype(np.int64)
        tie[d] = int((t ** 3 - t).sum())
        for g in range(n_groups):
            m = codes == g
            r2[g, d] = int(twice[m].sum())
            pos[g, d] = int((col[m] > eps32).sum())
            with np.errstate(invalid="ignore"):                             # +inf and -inf in one group: NaN, as on the device
                tot[g, d] = col[m].astype(np.longdouble).sum()
            tot_abs[g, d] = np.abs(col[m]).astype(np.longdouble).sum()
    return r2, tie, pos, tot, tot_abs


def z_score(rank_sum2, tie_term, n_g, n):
    """(U, z) float64 [G, D]: U = R - n_g (n_g + 1) / 2, z = (U - n_g (n - n_g) / 2) / sqrt(n_g (n - n_g) / 12 ((n + 1) -
    T / (n (n - 1)))); z = 0 where the variance is 0.  Scalar Python floats element by element: fp64, one rounding an
    operation."""
    G, D = rank_sum2.shape
    U = np.zeros((G, D))
    z = np.zeros((G, D))
    for g in range(G):
        n1 = float(n_g[g])
        n2 = float(n) - n1
        for d in range(D):
            U[g, d] = float(rank_sum2[g, d]) / 2.0 - n1 * (n1 + 1.0) / 2.0
            if n < 2:
                continue
            var = n1 * n2 / 12.0 * ((n + 1.0) - float(tie_term[d]) / (float(n) * (n - 1.0)))
            if var > 0.0:
                z[g, d] = (U[g, d] - n1 * n2 / 2.0) / math.sqrt(var)
    return U, z


def p_value(z):
    """erfc(|z| / sqrt 2) by math.erfc (the C library's), element by element."""
    return np.vectorize(lambda v: math.erfc(abs(v) / math.sqrt(2.0)), otypes=[np.float64])(np.asarray(z, dtype=np.float64))


def benjamini_hochberg(p):
    """One vector of p-values: sorted ascending, p m / rank, made monotone from the largest down, clipped to 1."""
    p = np.asarray(p, dtype=np.float64)
    m = len(p)
    order = np.argsort(p)
    adj = np.empty(m)
    running = np.inf
    for rank in range(m, 0, -1):
        i = order[rank - 1]
        running = min(running, p[i] * m / rank)
        adj[i] = min(running, 1.0)
    return adj


def log1p_like(rng, n, D, zero_frac):
    """float32 [n, D]: log1p of Poisson-ish counts with about ``zero_frac`` zeros, so that ties are everywhere."""
    counts = rng.poisson(3.0, size=(n, D)) * (rng.random((n, D)) >= zero_frac)
    return np.log1p(counts * rng.choice([1.0, 1.5, 2.25], size=(1, D))).astype(np.float32)


def special_columns(x, rng):
    """Plants, where the matrix has the columns: an all-tied gene, a gene rounded to integers, a -0.0 beside +0.0, an
    all-distinct gene with negative values.  In place; returns x."""
    n, D = x.shape
    if D > 1:
        x[:, 1] = np.float32(0.75)
    if D > 2:
        x[:, 2] = np.round(x[:, 2])
    if D > 3:
        x[:, 3] = np.where(np.arange(n) % 3 == 0, np.float32(-0.0), x[:, 3] * (np.arange(n) % 2))
    if D > 4:
        x[:, 4] = (rng.permutation(n).astype(np.float32) - n // 2) / 4
    return x

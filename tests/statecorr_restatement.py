"""The state-gene correlation of the reference's ``corr_analysis`` (mmidas/utils/tree_based_analysis.py), restated in numpy
fp64 in the two-pass form: per (group, gene) the mask x > 0 and its count c; exactly 0 where c <= 4; NaN where x or the state
takes one value over the mask (what ``scipy.stats.pearsonr`` returns for a constant input, and the reference stores); else
centre both, r = sum(xm sm) / sqrt(sum(xm^2) sum(sm^2)), clipped to [-1, 1] as scipy clips.  Beside r it returns the counts
and, per entry, kappa = max(1 + mean_x^2 / var_x, 1 + mean_s^2 / var_s) over the mask, the condition number of the raw-moment
form, which the device's error bound is stated in.  No scipy."""
import numpy as np

U = 2.0 ** -53


def encode(groups):
    """(classes, codes) by ``np.unique(return_inverse=True)``."""
    classes, codes = np.unique(np.asarray(groups), return_inverse=True)
    return classes, codes.reshape(-1)


def state_corr(state, cell, codes=None, n_groups=None):
    """(r float64 [G, S, D], count int64 [G, D], kappa float64 [G, S, D]) of ``state`` [n, S] and ``cell`` [n, D] in fp64
    on the values as they are; ``codes`` [n] ints in [0, n_groups) or None for one group.  kappa is 1 where r is 0 by the
    count rule and inf where r is NaN."""
    s_all, x_all = np.asarray(state, dtype=np.float64), np.asarray(cell, dtype=np.float64)
    n, S = s_all.shape
    D = x_all.shape[1]
    assert x_all.shape[0] == n
    if codes is None:
        codes, n_groups = np.zeros(n, dtype=np.int64), 1
    G = int(n_groups)
    r, cnt, kap = np.zeros((G, S, D)), np.zeros((G, D), dtype=np.int64), np.ones((G, S, D))
    for g in range(G):
        members = np.flatnonzero(np.asarray(codes) == g)
        xg, sg = x_all[members], s_all[members]
        for d in range(D):
            mask = xg[:, d] > 0
            c = int(mask.sum())
            cnt[g, d] = c
            if c <= 4:
                continue
            x, s = xg[mask, d], sg[mask]
            const = (x == x[0]).all() | (s == s[0]).all(axis=0)             # [S]
            mx, ms = x.mean(), s.mean(axis=0)
            xm, sm = x - mx, s - ms
            vx, vs = np.dot(xm, xm), np.einsum("is,is->s", sm, sm)
            with np.errstate(divide="ignore", invalid="ignore"):
                val = np.clip((xm @ sm) / np.sqrt(vx * vs), -1.0, 1.0)
                k = np.maximum(1.0 + mx * mx / (vx / c), 1.0 + ms * ms / (vs / c))
            r[g, :, d] = np.where(const, np.nan, val)
            kap[g, :, d] = np.where(const, np.inf, k)
    return r, cnt, kap


def tolerance(count, kappa):
    """The derived bound on |device r - this restatement| for fp64 raw moments: 8 (c + 1) kappa 2^-53, elementwise for
    count [G, D] against kappa [G, S, D].  Entries that are 0 or NaN by rule are compared exactly, not
    by this."""
    return 8.0 * (np.asarray(count, dtype=np.float64)[:, None, :] + 1.0) * np.asarray(kappa) * U


def corr_analysis(state, cell):
    """The reference's two returns: per state the sorted |r| and the genes in that order (numpy puts NaN last)."""
    r = state_corr(state, cell)[0][0]
    return [np.sort(np.abs(v)) for v in r], [np.argsort(np.abs(v)) for v in r]

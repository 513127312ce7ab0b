"""numpy restatement of the principal-component path (utils/pca.py over csrc/pca.hip) -- the "exact" side of the PCA tests.

The designed inputs: X = U diag(sqrt(lambda (n - 1))) W^T + offsets, rounded to float32, with U [n, r] orthonormal and
orthogonal to the ones vector and W [D, r] orthonormal, r = min(n - 1, D): the sample covariance of X (before the rounding)
has exactly the eigenvalues lambda.  ``tools/gen_golden_pca.py`` records them, with sklearn's PCA(svd_solver="full") of each,
in tests/golden/pca_cases.npz; the tests read X from there.

Two references for the subspace, both numpy fp64 on the float32 values: ``eigh_route`` (two-pass covariance, np.linalg.eigh)
and ``svd_route`` (np.linalg.svd of the centred matrix, what sklearn does).  Their distance from each other, e_ref, is the
reference's own error; the gates add it to the Davis-Kahan term 2 residual / gap of the fit under test.

The kernels' arithmetic is restated in np.longdouble on the same doubles t = (double)x - (double)pivot, with the sums of
magnitudes that the derived bounds (include/mmvae.h) are multiples of."""
import numpy as np

U = 2.0 ** -53

# name: (n, D, k)
CASES = {"gap": (600, 80, 5), "geo": (600, 80, 5), "wide": (300, 260, 10), "n<D": (20, 50, 5), "flat": (600, 80, 5)}
CONVERGING = ("gap", "geo", "wide", "n<D")


def spectrum(name, r):
    j = np.arange(r, dtype=np.float64)
    if name == "gap":
        head, tail = [100.0, 81.0, 64.0, 49.0, 36.0], 4.0 * 0.9 ** j
    elif name == "geo":
        head, tail = [], 0.97 ** j
    elif name == "wide":
        head, tail = list(np.linspace(50.0, 3.0, 10)), 0.98 ** j
    elif name == "n<D":
        head, tail = [9.0, 7.0, 5.0, 3.0, 2.0], 0.5 * 0.8 ** j
    elif name == "flat":
        head, tail = [], 0.999 ** j
    else:
        raise KeyError(name)
    return np.concatenate([head, tail])[:r]


def design(name):
    """The designed input ``name``: float32 [n, D]."""
    n, D, _ = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name) + 20)
    r = min(n - 1, D)
    A = rng.normal(size=(n, r))
    Uo, _ = np.linalg.qr(A - A.mean(axis=0))
    W, _ = np.linalg.qr(rng.normal(size=(D, r)))
    lam = spectrum(name, r)
    X = (Uo * np.sqrt(lam * (n - 1))) @ W.T + 3.0 * rng.normal(size=D)
    return X.astype(np.float32)


# ---- the references -------------------------------------------------------------------------------------------------------------
def covariance(X):
    """(mean, two-pass unbiased covariance) in fp64 on the values of X."""
    h = np.asarray(X, dtype=np.float64)
    mean = h.mean(axis=0)
    c = h - mean
    return mean, c.T @ c / (h.shape[0] - 1)


def moments_about(X, pivot):
    """What mmvae_gram computes, in numpy's summation order: (s, G, covariance) about the float32 ``pivot``."""
    t = np.asarray(X, dtype=np.float64) - np.asarray(pivot, dtype=np.float32).astype(np.float64)
    n = t.shape[0]
    s, G = t.sum(axis=0), t.T @ t
    G = 0.5 * (G + G.T)
    return s, G, (G - np.outer(s, s) / n) / (n - 1)


def sign_flip(components):
    """sklearn's svd_flip(u_based_decision=False): in every row the entry of largest magnitude positive, the lowest index
    on ties."""
    c = np.array(components, dtype=np.float64)
    at = np.argmax(np.abs(c), axis=1)
    sg = np.sign(c[np.arange(c.shape[0]), at])
    sg[sg == 0] = 1.0
    return c * sg[:, None]


def eigh_route(X, k):
    """(mean, components [k, D] sign-fixed, all eigenvalues descending) from np.linalg.eigh of the two-pass covariance."""
    mean, C = covariance(X)
    lam, V = np.linalg.eigh(C)
    return mean, sign_flip(V[:, ::-1][:, :k].T), lam[::-1]


def svd_route(X, k):
    """The same from np.linalg.svd of the centred matrix (sklearn's PCA(svd_solver="full"))."""
    h = np.asarray(X, dtype=np.float64)
    mean = h.mean(axis=0)
    _, sv, vt = np.linalg.svd(h - mean, full_matrices=False)
    lam = np.zeros(h.shape[1])
    lam[:len(sv)] = sv ** 2 / (h.shape[0] - 1)
    return mean, sign_flip(vt[:k]), lam


def transform(X, mean, components):
    return (np.asarray(X, dtype=np.float64) - mean) @ np.asarray(components).T


def subspace_distance(A, B):
    """|A A^T - B B^T|_2 for two orthonormal bases [k, D] of subspaces of the same dimension: the sine of the largest
    principal angle, formed as |(I - B^T B) A^T|_2 so that a distance of 1e-12 is not lost against 1."""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    return float(np.linalg.norm(A.T - B.T @ (B @ A.T), 2))


def reference_errors(X, k):
    """The distance of the two references from each other: subspace, eigenvalues, components entrywise, transform entrywise."""
    m1, c1, l1 = eigh_route(X, k)
    m2, c2, l2 = svd_route(X, k)
    return {"subspace": subspace_distance(c1, c2), "values": float(np.abs(l1[:k] - l2[:k]).max()),
            "components": float(np.abs(c1 - c2).max()), "transform": float(np.abs(transform(X, m1, c1) - transform(X, m2, c2)).max()),
            "ratio": float(np.abs(l1[:k] / l1.sum() - l2[:k] / l2.sum()).max())}


def davis_kahan(fit):
    """2 residual / gap of a fit: the Davis-Kahan bound on the sine of the largest angle between the computed subspace and
    the invariant one, doubled because the gap is a Ritz estimate.  0 where the block is the whole space (gap NaN: k = D)."""
    if np.isnan(fit.gap):
        return 0.0
    return 2.0 * fit.residual / fit.gap


def subspace_gate(fit, e_ref):
    return davis_kahan(fit) + 4.0 * e_ref


def value_gate(D, lam1):
    """Eigenvalues against eigh's: 16 D u lambda_1."""
    return 16.0 * D * U * lam1


# ---- the kernels in extended precision --------------------------------------------------------------------------------------
def t_of(X, pivot):
    """The doubles t = (double)x - (double)pivot the kernels form (one fp64 rounding each), as the device forms them."""
    return np.asarray(X, dtype=np.float32).astype(np.float64) - np.asarray(pivot, dtype=np.float32).astype(np.float64)


def gram_exact(t):
    """(s, G, A) in np.longdouble from the doubles t: s = sum t, G = sum t t^T, A = sum |t_i t_j| (the bound's scale)."""
    tl = t.astype(np.longdouble)
    return tl.sum(axis=0), tl.T @ tl, np.abs(tl).T @ np.abs(tl)


def gram_gate(n, A):
    """|G_ij - exact| <= (n + 2) u sum_r |t_ri t_rj|."""
    return (n + 2) * U * np.asarray(A, dtype=np.float64)


def covariance_exact(t):
    """(covariance of the doubles t in np.longdouble, var, kappa) -- kappa_i = 1 + mean_i^2 / var_i about the pivot (t is
    already the difference from it)."""
    tl = t.astype(np.longdouble)
    n = tl.shape[0]
    m = tl.mean(axis=0)
    c = tl - m
    cov = c.T @ c / (n - 1)
    var = (c * c).sum(axis=0) / n
    kappa = 1.0 + (m * m) / np.where(var > 0, var, 1.0)
    return cov, var.astype(np.float64), kappa.astype(np.float64)


def covariance_gate(n, var, kappa):
    """The bound derived for mmvae_group_moments in include/mmvae.h with N = n, ddof = 1:
    4 (n + 2) kappa u sqrt(var_i var_j) n / (n - 1), kappa = sqrt(kappa_i kappa_j)."""
    return 4.0 * (n + 2) * np.sqrt(np.outer(kappa, kappa)) * U * np.sqrt(np.outer(var, var)) * n / (n - 1.0)


def mul_exact(M, Q):
    """(M Q, |M| |Q|) in np.longdouble."""
    Ml, Ql = np.asarray(M).astype(np.longdouble), np.asarray(Q).astype(np.longdouble)
    return Ml @ Ql, np.abs(Ml) @ np.abs(Ql)


def symm_mul_gate(D, A):
    return (D + 1) * U * np.asarray(A, dtype=np.float64)


def project_gate(D, A):
    return (D + 2) * U * np.asarray(A, dtype=np.float64)


# ---- integer inputs: every sum exact ------------------------------------------------------------------------------------------
def integer_matrix(n, D, shift=0):
    """x[r, j] = (3 r + 5 j + r j + shift) mod 7 - 3: asymmetric small integers, float32."""
    r, j = np.arange(n, dtype=np.int64)[:, None], np.arange(D, dtype=np.int64)[None, :]
    return ((3 * r + 5 * j + r * j + shift) % 7 - 3).astype(np.float32)

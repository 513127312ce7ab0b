"""numpy restatement of sklearn's ``silhouette_samples(x, labels, metric="euclidean")`` in fp64 and in difference form -- the
"exact" side of the silhouette tests.  ``x`` is taken as given (its values converted to float64 exactly), every distance is
sqrt(sum_k (x_ik - x_jk)^2) with no Gram expansion, rows are processed in chunks so that nothing of size n x n exists.

  S(i, k) = sum over the cells j with label k of |x_i - x_j|;  a_i = S(i, l_i) / (f_{l_i} - 1);
  b_i = min over k != l_i of S(i, k) / f_k;  s_i = (b_i - a_i) / max(a_i, b_i);
  s_i = 0 for a singleton cluster and for max(a_i, b_i) = 0 (sklearn: 0 / 0 -> nan_to_num)."""
import numpy as np


def encode(labels):
    classes, codes = np.unique(np.asarray(labels), return_inverse=True)
    return classes, codes.reshape(-1)


def cluster_sums(x, codes, n_classes, rows=None):
    """S [n, K] in fp64 (``rows``: a slice, for those rows only); the rows go in chunks of about 2^24 differences."""
    x = np.asarray(x, dtype=np.float64)
    n, d = x.shape
    onehot = np.zeros((n, n_classes))
    onehot[np.arange(n), codes] = 1.0
    first, last, _ = (rows or slice(None)).indices(n)
    chunk = max(1, (1 << 24) // (n * d))
    out = np.empty((last - first, n_classes))
    for r in range(first, last, chunk):
        diff = x[r:min(r + chunk, last), None, :] - x[None, :, :]
        out[r - first:r - first + diff.shape[0]] = np.sqrt(np.einsum("ijk,ijk->ij", diff, diff)) @ onehot
    return out


def samples_from_sums(S, codes_of_rows, f):
    """The samples of the rows whose cluster sums are ``S``; f the cluster sizes."""
    rows = np.arange(len(codes_of_rows))
    f_own = f[codes_of_rows]
    a = np.where(f_own > 1, S[rows, codes_of_rows] / np.maximum(f_own - 1, 1), 0.0)
    means = S / f
    means[rows, codes_of_rows] = np.inf
    b = means.min(axis=1)
    m = np.maximum(a, b)
    return np.where((f_own > 1) & (m > 0), (b - a) / np.where(m > 0, m, 1.0), 0.0)


def silhouette_samples(x, labels, rows=None):
    _, codes = encode(labels)
    K = int(codes.max()) + 1
    f = np.bincount(codes, minlength=K).astype(np.float64)
    return samples_from_sums(cluster_sums(x, codes, K, rows), codes[rows or slice(None)], f)


def silhouette_score(x, labels):
    return float(np.mean(silhouette_samples(x, labels)))


def class_means(s, labels):
    """(mean sample per class in np.unique order, class sizes)."""
    classes, codes = encode(labels)
    return (np.array([np.mean(s[codes == k]) for k in range(len(classes))]),
            np.array([float(np.sum(codes == k)) for k in range(len(classes))]))


def get_silh_score(x, labels):
    s = silhouette_samples(x, labels)
    return class_means(s, labels)[0], np.mean(s)


def pca_project(data, num_pc):
    """The centred data on its top principal components by exact SVD (what PCA(svd_solver="full") gives up to signs)."""
    h = np.asarray(data, dtype=np.float64)
    h = h - h.mean(axis=0)
    _, _, vt = np.linalg.svd(h, full_matrices=False)
    return h @ vt[:num_pc].T


def tolerance(d):
    """The gate of the device against this restatement on the same float32 values: an fp32 difference-form distance is off by
    at most (d / 2 + 2) 2^-24 relatively (subtraction, d non-negative squares, a square root of 1 ulp), a and b inherit it, and
    s = 1 - a / b or b / a - 1 with the ratio at most 1, so |ds| <= (d + 4) 2^-24; doubled for a 1-ulp square root."""
    return (d + 4) * 2.0 ** -23

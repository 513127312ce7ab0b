"""The Gaussian classifiers of the reference's ``mmidas/utils/cluster_analysis.py`` (``QDA_classifier``, ``LDA_classifier``)
restated in numpy fp64, without sklearn: the k-fold split of ``KFold(n_splits, shuffle=True, random_state=seed)``, a two-pass
``np.cov`` on every fold's training rows, the two models as sklearn builds them, and

    score(x, k) = c0_k - |W_k^T (x - mu_k)|^2 / 2,   prediction = np.argmax over k, margin = best - second.

QDA is ``QuadraticDiscriminantAnalysis(reg_param)``: with lam, V the eigen-pairs of the unbiased class covariance,
S2 = (1 - reg) lam + reg, W = V S2^(-1/2), c0 = -sum(log S2) / 2 + log(N_k / N); a class with one training cell raises sklearn's
ValueError.  sklearn takes the SVD of the centred rows, which for N_k > d gives the same lam and V (up to signs, which the
square does not see); for N_k <= d it keeps min(N_k, d) directions, the last of them arbitrary -- here all d eigen-directions
are used (the package's documented departure).  LDA is ``LinearDiscriminantAnalysis()``, solver ``svd``: the pooled
within-class scatter Sw, std = sqrt(diag Sw / N), C = Sw / (N - K_present) scaled by 1 / std on both sides, the eigen-pairs
of C with singular values S = sqrt(lam) > tol = 1e-4 kept, W = (V / std) / S shared by the classes, c0 = log(N_k / N).  sklearn's
``decision_function`` is these scores plus a term that is the same for every class of a cell (its second SVD over the
class means drops only directions in which all classes score alike), so it is compared after each row's maximum is taken
off.

Beside the scores the functions return what the derived bounds (``tolerance_*``) are stated in.  u = 2^-53."""
import numpy as np

U = 2.0 ** -53
QDA_REG = 1e-2
LDA_TOL = 1e-4


def encode(labels):
    """(classes, codes) by ``np.unique(return_inverse=True)`` -- sklearn's LabelEncoder."""
    classes, codes = np.unique(np.asarray(labels), return_inverse=True)
    return classes, codes.reshape(-1)


def fold_split(n, kfold, seed):
    """fold int64 [n]: the fold whose test set holds cell i under ``KFold(kfold, shuffle=True, random_state=seed)``: a
    ``RandomState(seed).shuffle`` of ``arange(n)`` cut into kfold consecutive pieces, the first n % kfold one longer.  sklearn
    yields every test set (and every training set) in ascending order of the index."""
    idx = np.arange(n)
    np.random.RandomState(seed).shuffle(idx)
    sizes = np.full(kfold, n // kfold, dtype=np.int64)
    sizes[:n % kfold] += 1
    fold = np.empty(n, dtype=np.int64)
    fold[idx] = np.repeat(np.arange(kfold), sizes)
    return fold


def two_pass(x):
    """(N, mean [d], scatter [d, d]) of the rows of x in fp64, centred before the products."""
    x = np.asarray(x, dtype=np.float64)
    if x.shape[0] == 0:
        return 0, np.zeros(x.shape[1]), np.zeros((x.shape[1], x.shape[1]))
    mean = x.mean(axis=0)
    xc = x - mean
    return x.shape[0], mean, xc.T @ xc


def qda_from_stats(counts, means, scatters, reg=QDA_REG, classes=None):
    """(mu [K, d], W [K, d, d], c0 [K], info) from per-class counts, means and scatter matrices (sum of centred outer
    products).  info: per class the smallest S2, the Frobenius norm of the regularised covariance and the covariance's trace."""
    K, d = means.shape
    N = float(np.sum(counts))
    mu, W, c0 = np.array(means, dtype=np.float64), np.zeros((K, d, d)), np.full(K, -np.inf)
    lam_min, frob, trace = np.ones(K), np.zeros(K), np.zeros(K)
    for k in range(K):
        if counts[k] == 0:
            continue
        if counts[k] == 1:
            name = k if classes is None else classes[k]
            raise ValueError("y has only 1 sample in class %s, covariance is ill defined." % str(name))
        cov = scatters[k] / (counts[k] - 1.0)
        lam, V = np.linalg.eigh(cov)
        S2 = (1.0 - reg) * lam + reg
        W[k] = V * S2 ** -0.5
        c0[k] = -0.5 * np.sum(np.log(S2)) + np.log(counts[k] / N)
        lam_min[k], frob[k], trace[k] = S2.min(), np.sqrt(np.sum(((1.0 - reg) * cov + reg * np.eye(d)) ** 2)), np.trace(cov)
    return mu, W, c0, {"lam_min": lam_min, "frob": frob, "trace": trace, "scale": np.ones((K, d))}


def lda_from_stats(counts, means, scatters, tol=LDA_TOL):
    """The same for LDA: one W for all classes, from the pooled scatter."""
    K, d = means.shape
    present = np.asarray(counts) > 0
    N, Kp = float(np.sum(counts)), int(present.sum())
    Sw = np.sum(scatters[present], axis=0)
    std = np.sqrt(np.diag(Sw) / N)
    std[std == 0] = 1.0
    fac = 1.0 / (N - Kp)
    Cm = fac * Sw / np.outer(std, std)
    lam, V = np.linalg.eigh(Cm)
    lam, V = lam[::-1], V[:, ::-1]
    S = np.sqrt(np.maximum(lam, 0.0))
    rank = int(np.sum(S > tol))
    Wone = np.zeros((d, d))
    Wone[:, :rank] = (V[:, :rank] / std[:, None]) / S[:rank]
    mu = np.array(means, dtype=np.float64)
    W = np.broadcast_to(Wone, (K, d, d)).copy()
    c0 = np.full(K, -np.inf)
    c0[present] = np.log(np.asarray(counts, dtype=np.float64)[present] / N)
    kept = S[:rank] ** 2
    info = {"lam_min": np.full(K, kept.min() if rank else 1.0), "frob": np.full(K, np.sqrt(np.sum(Cm ** 2))),
            "trace": np.full(K, d * fac * N), "scale": np.broadcast_to(1.0 / std, (K, d)).copy(), "rank": rank}
    return mu, W, c0, info


def scores(x, mu, W, c0):
    """(score [n, K], A [n, K]) of the rows of x under one model: A = sum_c (sum_j |W[j, c] t_j|)^2, the magnitude the
    summation-order bound is stated in.  A class with c0 = -inf scores -inf."""
    x = np.asarray(x, dtype=np.float64)
    t = x[:, None, :] - mu[None]                                            # [n, K, d]
    y = np.einsum("nkj,kjc->nkc", t, W)
    q = np.sum(y * y, axis=2)
    A = np.sum(np.einsum("nkj,kjc->nkc", np.abs(t), np.abs(W)) ** 2, axis=2)
    with np.errstate(invalid="ignore"):
        sc = np.where(np.isneginf(c0)[None], -np.inf, c0[None] - 0.5 * q)
    return sc, A


def best_two(sc):
    """(arg-max, best, second) of every row: ``np.argmax`` (the lowest index on ties), the largest and the second largest
    score counting multiplicity, -inf where there is none."""
    pred = np.argmax(sc, axis=1)
    srt = np.sort(sc, axis=1)
    best = srt[:, -1]
    second = srt[:, -2] if sc.shape[1] > 1 else np.full(sc.shape[0], -np.inf)
    return pred, best, second


def fold_stats(x, codes, K, fold, f):
    """(counts [K], means [K, d], scatters [K, d, d]) of the training set of fold f (the cells of the other folds)."""
    x = np.asarray(x, dtype=np.float64)
    d = x.shape[1]
    counts, means, scat = np.zeros(K, dtype=np.int64), np.zeros((K, d)), np.zeros((K, d, d))
    train = fold != f
    for k in range(K):
        counts[k], means[k], scat[k] = two_pass(x[train & (codes == k)])
    return counts, means, scat


def cv_predict(x, labels, kfold, seed, kind="qda", reg=QDA_REG):
    """The whole cross-validation on the values of x as they are: dict with classes, codes, fold [n], pred [n] (codes), best,
    second [n], scores and A [n, K], mu [F, K, d], W [F, K, d, d], c0 [F, K], counts [F, K] and the per-model info arrays."""
    x = np.asarray(x, dtype=np.float64)
    n, d = x.shape
    classes, codes = encode(labels)
    K = len(classes)
    fold = fold_split(n, kfold, seed)
    out = {"classes": classes, "codes": codes, "fold": fold, "pred": np.zeros(n, dtype=np.int64), "best": np.zeros(n),
           "second": np.zeros(n), "scores": np.zeros((n, K)), "A": np.zeros((n, K)), "mu": np.zeros((kfold, K, d)),
           "W": np.zeros((kfold, K, d, d)), "c0": np.zeros((kfold, K)), "counts": np.zeros((kfold, K), dtype=np.int64),
           "lam_min": np.ones((kfold, K)), "frob": np.zeros((kfold, K)), "trace": np.zeros((kfold, K)),
           "scale": np.ones((kfold, K, d)), "raw2": np.zeros((kfold, K, d)), "absmax": np.abs(x).max(axis=0)}
    for f in range(kfold):
        counts, means, scat = fold_stats(x, codes, K, fold, f)
        if kind == "qda":
            mu, W, c0, info = qda_from_stats(counts, means, scat, reg, classes)
        elif kind == "lda":
            mu, W, c0, info = lda_from_stats(counts, means, scat)
        else:
            raise ValueError(f"kind = {kind!r}")
        test = np.flatnonzero(fold == f)
        sc, A = scores(x[test], mu, W, c0)
        out["scores"][test], out["A"][test] = sc, A
        out["pred"][test], out["best"][test], out["second"][test] = best_two(sc)
        out["mu"][f], out["W"][f], out["c0"][f], out["counts"][f] = mu, W, c0, counts
        for name in ("lam_min", "frob", "trace", "scale"):
            out[name][f] = info[name]
        out["raw2"][f] = scat.diagonal(axis1=1, axis2=2) / np.maximum(counts, 1)[:, None]          # the variances (ddof 0)
    return out


def accuracy(ref, pred):
    """sklearn's ``accuracy_score`` of two label arrays: ``float(np.average(ref == pred))``."""
    return float(np.average(np.asarray(ref) == np.asarray(pred)))


def classifier(x, labels_dict, kfold, seed, kind):
    """The reference's returns ``(acc, ref_labels, pred_labels)``: dicts over the keys of ``labels_dict`` of lists over the
    folds, every test set in ascending order of the index."""
    acc, ref, pred = {}, {}, {}
    for key in labels_dict:
        y = np.asarray(labels_dict[key])
        r = cv_predict(x, y, kfold, seed, kind)
        acc[key], ref[key], pred[key] = [], [], []
        for f in range(kfold):
            test = np.flatnonzero(r["fold"] == f)
            p = r["classes"][r["pred"][test]]
            acc[key].append(accuracy(y[test], p))
            ref[key].append(y[test])
            pred[key].append(p)
    return acc, ref, pred


# ---- the derived bounds ---------------------------------------------------------------------------------------------------------
def tolerance_moments(N, raw2, pivot, absmax):
    """(bound on |mean - two-pass mean| [d], bound on |scatter - two-pass scatter| [d, d]) for the device's moments of N rows
    about ``pivot``; raw2 [d] = mean of (x - pivot)^2 = kappa var.  Every difference carries one rounding and a chain of N
    terms at most N u times the sum of the magnitudes; sum |t_i t_j| <= N sqrt(raw2_i raw2_j) and sum |t_i| <= N sqrt(raw2_i).
    That puts M_ij within (N + 2) u of that scale, s_i s_j / N within (2 N + 5) u and the subtraction one more: together at
    most 4 (N + 2) u N sqrt(raw2_i raw2_j); a fifth unit covers the two-pass reference's own rounding, which is smaller.
    The mean pivot + s / N is within (N + 2) u sqrt(raw2_i) + u |mean_i|, the reference's within N u max |x_i|."""
    r = np.sqrt(np.asarray(raw2, dtype=np.float64))
    scatter = 5.0 * (N + 2.0) * U * N * np.outer(r, r)
    mean = 2.0 * (N + 3.0) * U * (r + np.abs(pivot) + np.asarray(absmax))
    return mean, scatter


def tolerance_sum(d, A, c0):
    """The bound on |score - the same formula summed in another order| (both sides fp64, the same t = x - mu): an inner
    product of d terms is within d u sum_j |W[j, c] t_j| = d u a_c on each side, its square within 2 d u a_c^2 (+ u), the sum
    of the d squares within (d + 1) u sum a_c^2: (3 d + 2) u A for q, half of it for the score, on each of the two sides, and
    2 u (|c0| + q / 2) for the last subtraction: at most (3 d + 4) u (A + |c0|)."""
    c = np.where(np.isfinite(c0), np.abs(c0), 0.0)
    return (3.0 * d + 4.0) * U * (np.asarray(A) + c)


def tolerance_cv(res, pivot, kind):
    """The bound [n, K] on |device score - ``cv_predict`` score| for the whole path (device moments about ``pivot``, host
    eigh, device scores) against this restatement (two-pass covariance, eigh, numpy scores).  First order in the
    perturbation of the factorised matrix B (QDA: the regularised class covariance; LDA: the scaled pooled covariance),
    doubled for the higher orders: with q = t^T B^+ t, rho = |dB|_F / lam_min (lam_min the smallest kept eigenvalue),
        |d score| <= (rho q + rho d) / 2 + sqrt(q / lam_min) |d mu| + the summation bound,
    where |dB|_F is the moments' entrywise bound summed over the matrix (eps tr, eps = 4 (N + 2) kappa u N / (N - 1) with
    kappa the largest over the coordinates; LDA: 2 eps d on the unit-diagonal matrix, and eps q more for the 1 / std
    scaling) plus 16 d u |B|_F for each of the two eigh calls (LAPACK's backward error with a generous constant), and
    |d mu| the norm of the mean bound in the factor's coordinates.  -inf scores are compared exactly, not by this."""
    n, K = res["scores"].shape
    d = res["mu"].shape[2]
    gate = np.zeros((n, K))
    for f in range(res["mu"].shape[0]):
        test = np.flatnonzero(res["fold"] == f)
        cnt = res["counts"][f].astype(np.float64)
        off2 = (res["mu"][f] - pivot[None]) ** 2
        var = np.maximum(res["raw2"][f], 1e-300)
        kappa = (1.0 + off2 / var).max(axis=1)                                                  # [K]
        if kind == "lda":
            cnt_eff, kappa_eff = np.full(K, cnt.max()), np.full(K, kappa[cnt > 0].max())
        else:
            cnt_eff, kappa_eff = cnt, kappa
        eps = 4.0 * (cnt_eff + 2.0) * kappa_eff * U * cnt_eff / np.maximum(cnt_eff - 1.0, 1.0)
        dB = (2.0 * eps * d if kind == "lda" else eps * res["trace"][f]) + 32.0 * d * U * res["frob"][f]
        rho = dB / res["lam_min"][f]
        mean_tol = 2.0 * (cnt[:, None] + 3.0) * U * (np.sqrt(var + off2) + np.abs(pivot)[None] + res["absmax"][None])
        dmu = np.sqrt(np.sum((mean_tol * res["scale"][f]) ** 2, axis=1))                         # [K]
        sc = res["scores"][test]
        c0 = res["c0"][f]
        with np.errstate(invalid="ignore"):
            q = np.where(np.isfinite(sc), 2.0 * (c0[None] - sc), 0.0)
        first = 0.5 * (rho[None] * q + rho[None] * d) + np.sqrt(q / res["lam_min"][f][None]) * dmu[None]
        if kind == "lda":
            first = first + eps[None] * q
        gate[test] = 2.0 * first + tolerance_sum(d, res["A"][test], c0[None])
    return gate

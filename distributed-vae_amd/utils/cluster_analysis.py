"""The clusterability analysis of the reference's ``mmidas/utils/cluster_analysis.py``: ``get_SilhScore``,
``cluster_compare``, the two Gaussian classifiers ``QDA_classifier`` / ``LDA_classifier`` and ``RF_classifier``, on the
device, without sklearn.  The principal components that ``cluster_compare`` scores on are the one O(N D^2) step of the analysis: at the data
set's size a minute of host SVD in front of a silhouette of milliseconds.  ``cluster_compare(pca="device")`` takes them from
``utils/pca.py`` (``mmvae_gram`` on the fp64 MFMA, subspace iteration, ``mmvae_pca_project``); the
default ``pca="host"`` is numpy's exact SVD, kept as it was.

The reference calls ``sklearn.metrics.silhouette_samples`` / ``silhouette_score`` (euclidean) on the latents: n^2 distances,
which sklearn computes on the host in float64 through the Gram expansion.  Here the cells are sorted by label on the host,
uploaded once, and ``mmvae_silhouette`` (csrc/silhouette.hip) forms every distance in fp32 in difference
form and everything after it in fp64; the per-cell scores come back as float64 and the means are numpy's, over the classes
in ``np.unique`` order.

The classifiers answer how well the cell types are recovered from the latents under k-fold cross-validation.  One pass of
``mmvae_group_moments`` (csrc/gaussclf.hip) gives the moments of every (class, fold) group of cells
about one pivot; moments about one pivot add, so every fold's training set is a sum of groups.  The models are sklearn's,
built on the host in fp64 (F K eigen-decompositions of d x d matrices, plumbing), and ``mmvae_gauss_scores`` scores every
cell under every class of its own fold's model and takes the arg-max.  ``gaussian_cv_predict`` is the one function under
both; it also returns the two best scores of every cell, whose difference is a confidence the reference does not offer.

``RF_classifier`` is the sixth function of that module and the one its published figure is made with.  A forest on exact
thresholds is not a regular computation; on features quantised to 256 rank bins (``quantile_bins``) it is: per node and
feature a class x bin histogram of integers in LDS and a scan of it (``mmvae_forest_cv``, csrc/forest.hip; DESIGN.md section
9i).  ``forest_cv_predict`` is the function under it; it is seeded and gives the same bits on every run, which the
reference's own call does not.

``K_selection`` of that module is not part of this package.  ``custom_QDA`` and ``predict_leaf_gmm`` of the reference's
``analysis_tree_helpers.py`` are in ``utils/analysis_tree_helpers.py``."""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from .. import _native as N
from .. import dist as D
from .._utils import float32_on_device


def _encode(labels, n: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
    """(classes, code of every cell) by ``np.unique(return_inverse=True)`` -- sklearn's LabelEncoder -- after sklearn's
    condition on the number of labels."""
    y = np.asarray(labels)
    if y.ndim != 1:
        raise ValueError(f"labels of shape {y.shape} are not 1-D")
    if n is not None and y.shape[0] != n:
        raise ValueError(f"{y.shape[0]} labels for {n} samples")
    classes, codes = np.unique(y, return_inverse=True)
    if not 1 < len(classes) < y.shape[0]:
        raise ValueError(f"Number of labels is {len(classes)}. Valid values are 2 to n_samples - 1 (inclusive)")
    return classes, codes.reshape(-1)


def _points_on_device(x, device) -> torch.Tensor:
    """float32 [n, d] on ``device``, finite (a device tensor is checked too)."""
    return float32_on_device(x, device, "x", "[n, d]", check_device_finite=True)


def _samples(x_dev: torch.Tensor, codes: np.ndarray, n_classes: int) -> np.ndarray:
    """The silhouette samples of points already on the device under the encoded labels ``codes``."""
    order = np.argsort(codes, kind="stable")
    offsets = np.concatenate([[0], np.cumsum(np.bincount(codes, minlength=n_classes))]).astype(np.int64)
    perm = torch.from_numpy(order.astype(np.int64)).to(x_dev.device)
    s = N.silhouette(x_dev.index_select(0, perm), torch.from_numpy(offsets).to(x_dev.device), perm)
    return s.cpu().numpy()


def _class_means(s: np.ndarray, codes: np.ndarray, n_classes: int) -> Tuple[np.ndarray, np.ndarray]:
    """(``np.mean`` of the samples of every class, the class sizes as floats), classes in ``np.unique`` order."""
    members = [np.flatnonzero(codes == k) for k in range(n_classes)]
    return np.array([np.mean(s[m]) for m in members]), np.array([float(len(m)) for m in members])


def silhouette_samples(x, labels, device=None) -> np.ndarray:
    """sklearn's ``silhouette_samples(x, labels)`` (euclidean): float64 [n].

    ``x``: array-like or tensor [n, d], 1 <= d <= 128.  A float32 tensor on the GPU (what ``encode_dataset`` returns) is used
    where it lies; anything else is converted to float32 -- FLOAT64 INPUT IS ROUNDED to float32 -- and uploaded.  Every
    distance is an fp32 difference-form distance (relative error at most (d / 2 + 2) 2^-24), everything after it fp64, so a
    sample differs from the exact value on the float32 points by at most (d + 4) 2^-24.  ``labels``: any 1-D array of ints
    or hashables, encoded by ``np.unique(return_inverse=True)`` as sklearn's LabelEncoder does.  ValueError as in sklearn
    unless the number of distinct labels is in [2, n - 1]; ValueError on a length mismatch and on a non-finite ``x``."""
    if D.is_dist():
        raise NotImplementedError("silhouette_samples is not data-parallel: run it on one rank, outside the process group")
    n = int(x.shape[0]) if hasattr(x, "shape") else len(x)
    classes, codes = _encode(labels, n)
    return _samples(_points_on_device(x, device), codes, len(classes))


def silhouette_score(x, labels, device=None) -> float:
    """sklearn's ``silhouette_score(x, labels)``: ``np.mean`` of the samples, on the host copy."""
    return float(np.mean(silhouette_samples(x, labels, device)))


def get_SilhScore(x, labels):
    """The reference's ``get_SilhScore`` (cluster_analysis.py:201-211): ``(mean_smp_sc, sil_score)`` -- the mean silhouette
    sample of every class of ``np.unique(labels)``, in that order, and the mean over all cells.  The samples are computed
    once on the device (the reference computes them twice on the host); both means are ``np.mean`` on the host copy."""
    if D.is_dist():
        raise NotImplementedError("get_SilhScore is not data-parallel: run it on one rank, outside the process group")
    n = int(x.shape[0]) if hasattr(x, "shape") else len(x)
    classes, codes = _encode(labels, n)
    s = _samples(_points_on_device(x, None), codes, len(classes))
    return _class_means(s, codes, len(classes))[0], np.mean(s)


def _project(data, num_pc: int) -> np.ndarray:
    """The centred data on its top ``num_pc`` principal components, float64 [n, num_pc], by numpy's exact SVD."""
    h = data.detach().cpu().numpy() if isinstance(data, torch.Tensor) else np.asarray(data)
    h = np.asarray(h, dtype=np.float64)
    if h.ndim != 2 or not 0 < num_pc <= min(h.shape):
        raise ValueError(f"cluster_compare: num_pc = {num_pc} components of data of shape {h.shape}")
    h = h - h.mean(axis=0)
    _, _, vt = np.linalg.svd(h, full_matrices=False)
    return h @ vt[:num_pc].T


def _figure(curves, num_pc):
    """One line per label set: the class means in ascending order (the picture the reference draws); None without
    matplotlib, which is imported here and not with the module."""
    try:
        import matplotlib.pyplot as plt
    except ImportError:
        return None
    fig, ax = plt.subplots(figsize=(10, 5))
    for name, ordered_means in curves:
        ax.plot(range(len(ordered_means)), ordered_means, label=name)
    ax.set(title=f"{num_pc} PCs", xlabel="Ordered clusters", ylabel="Ave. Silhouette scores")
    ax.title.set_fontsize(18)
    ax.legend(prop={"size": 12})
    fig.tight_layout()
    return fig


def cluster_compare(data, labels, num_pc=0, saving_path='', pca="host"):
    """The reference's ``cluster_compare`` (cluster_analysis.py:87-120): ``(fig, silh_smp_score, sil_score, c_size)`` for the
    dict ``labels`` of label arrays -- per entry the per-class mean silhouette samples (classes in ``np.unique`` order), the
    overall score, and the class sizes ordered by ascending mean score -- all on the projection of ``data`` onto its top
    ``num_pc`` principal components.

    ``pca="host"`` (the default): numpy's exact SVD of the centred data in fp64 on the host, which is what sklearn's
    ``PCA(svd_solver="full")`` computes (the silhouette does not see the components' signs); O(N D^2) on the host, about a
    minute at the data set's size.  ``pca="device"``: ``utils.pca.pca_project`` -- the covariance, the subspace iteration's
    products and the projection on the device in fp64 on the float32 values of ``data`` (FLOAT64 INPUT IS ROUNDED to
    float32), the projected points handed to the silhouette without leaving the device; ``num_pc`` <= 32 there (the
    iteration's block holds at most 64 vectors).  sklearn's default solver is a randomised one at large sizes, so at those
    sizes the reference's own numbers are not reproducible either.  The projected points are rounded to float32 and scored
    for every entry of ``labels``.  ``fig`` shows what the reference's figure shows, or is None when matplotlib is not
    installed.  Departure: ``num_pc == 0`` raises ValueError (the reference fails there with an unbound local).
    ``saving_path`` is unused, as in the reference."""
    if num_pc <= 0:
        raise ValueError("cluster_compare: num_pc must be positive (the reference computes nothing for num_pc = 0)")
    if pca not in ("host", "device"):
        raise ValueError(f"cluster_compare: pca = {pca!r}: one of 'host', 'device'")
    if D.is_dist():
        raise NotImplementedError("cluster_compare is not data-parallel: run it on one rank, outside the process group")
    if pca == "device":
        shape = tuple(data.shape) if hasattr(data, "shape") else np.asarray(data).shape
        if len(shape) != 2 or not 0 < num_pc <= min(shape):
            raise ValueError(f"cluster_compare: num_pc = {num_pc} components of data of shape {shape}")
        encoded = {key: _encode(labels[key], shape[0]) for key in labels}         # every refusal before any device work
        from .pca import pca_project
        z_dev = pca_project(data, num_pc, out="device")
    else:
        z = _project(data, num_pc)
        encoded = {key: _encode(labels[key], z.shape[0]) for key in labels}       # every refusal before any device work
        z_dev = _points_on_device(z, None)
    silh_smp_score, sil_score, c_size, curves = [], [], [], []
    for key, (classes, codes) in encoded.items():
        s = _samples(z_dev, codes, len(classes))
        means, sizes = _class_means(s, codes, len(classes))
        ascending = np.argsort(means)
        silh_smp_score.append(means)
        sil_score.append(np.mean(s))
        c_size.append(sizes[ascending])
        curves.append((key, means[ascending]))
    return _figure(curves, num_pc), silh_smp_score, sil_score, c_size


# ---- the Gaussian classifiers ---------------------------------------------------------------------------------------------
QDA_REG_PARAM = 1e-2            # the reference's QuadraticDiscriminantAnalysis(reg_param=1e-2)
LDA_TOL = 1e-4                  # sklearn's LinearDiscriminantAnalysis(tol=1e-4): singular values at or below it are dropped


def kfold_of(n: int, kfold: int, seed) -> np.ndarray:
    """The fold whose test set holds every cell under sklearn's ``KFold(n_splits=kfold, shuffle=True, random_state=seed)``,
    int64 [n]: ``np.random.RandomState(seed).shuffle`` of ``arange(n)``, cut into ``kfold`` consecutive pieces of which the
    first ``n % kfold`` are one longer.  sklearn yields every test set in ascending order of the index."""
    idx = np.arange(n)
    np.random.RandomState(seed).shuffle(idx)
    sizes = np.full(kfold, n // kfold, dtype=np.int64)
    sizes[:n % kfold] += 1
    fold = np.empty(n, dtype=np.int64)
    fold[idx] = np.repeat(np.arange(kfold), sizes)
    return fold


def _qda_models(counts, scatter, reg):
    """(W [K, d, d], c0 [K]) of sklearn's QDA from per-class training counts [K] and scatter matrices [K, d, d]."""
    K, d = scatter.shape[:2]
    N = float(counts.sum())
    W, c0 = np.zeros((K, d, d)), np.full(K, -np.inf)
    have = counts > 0
    cov = scatter[have] / (counts[have] - 1.0)[:, None, None]
    lam, V = np.linalg.eigh(cov)
    S2 = (1.0 - reg) * lam + reg
    W[have] = V * (S2 ** -0.5)[:, None, :]
    c0[have] = -0.5 * np.sum(np.log(S2), axis=1) + np.log(counts[have] / N)
    return W, c0


def _lda_models(counts, scatter):
    """(W [K, d, d], c0 [K]) of sklearn's LDA (solver "svd"): one factor of the pooled within-class covariance for all."""
    K, d = scatter.shape[:2]
    have = counts > 0
    N = float(counts.sum())
    Sw = np.sum(scatter[have], axis=0)
    std = np.sqrt(np.diag(Sw) / N)
    std[std == 0] = 1.0
    Cm = Sw / np.outer(std, std) / (N - int(have.sum()))
    lam, V = np.linalg.eigh(Cm)
    lam, V = lam[::-1], V[:, ::-1]
    S = np.sqrt(np.maximum(lam, 0.0))
    rank = int(np.sum(S > LDA_TOL))
    Wone = np.zeros((d, d))
    Wone[:, :rank] = (V[:, :rank] / std[:, None]) / S[:rank]
    c0 = np.full(K, -np.inf)
    c0[have] = np.log(counts[have] / N)
    return np.broadcast_to(Wone, (K, d, d)), c0


def fold_training_moments(s, M, counts):
    """The training moments of every fold, one fold at a time, from the moments of the K x F (class, fold) groups about one
    pivot: ``s`` [K, F, d], ``M`` [K, F, d (d + 1) / 2] (``mmvae_group_moments``), ``counts`` [K, F].  The training set of
    fold f is the sum of the groups of the other folds, added in fold order from zeros with no subtraction (F = 1: the one
    group is the training set).  Yields, fold after fold, for all K classes: (the training count N [K], the mean's offset
    from the pivot s / max(N, 1) [K, d], scatter = M - s s^T / max(N, 1) [K, d, d]).  Every builder of fold models reads
    these sums, so the order of the additions, which decides the bits, is stated once; one fold's [K, d, d] is alive at a
    time, never all folds'."""
    K, F, d = s.shape
    iu = np.triu_indices(d)
    for f in range(F):
        cnt, s_tr, M_tr = np.zeros(K), np.zeros((K, d)), np.zeros((K, M.shape[2]))
        for g in range(F):
            if g != f or F == 1:
                cnt += counts[:, g]
                s_tr += s[:, g]
                M_tr += M[:, g]
        Nk = np.maximum(cnt, 1.0)[:, None]
        full = np.zeros((K, d, d))
        full[:, iu[0], iu[1]] = M_tr
        full[:, iu[1], iu[0]] = M_tr
        yield cnt, s_tr / Nk, full - s_tr[:, :, None] * s_tr[:, None, :] / Nk[:, :, None]


def models_from_moments(s, M, counts, pivot, kind, reg_param=QDA_REG_PARAM):
    """The F models of a k-fold cross-validation from the moments of the K x F (class, fold) groups about ``pivot``:
    ``s`` [K, F, d], ``M`` [K, F, d (d + 1) / 2] (``mmvae_group_moments``), ``counts`` [K, F] -> (mu [F, K, d],
    W [F, K, d, d], c0 [F, K]) in fp64.  The training set of fold f is the sum of the groups of the other folds, added in
    fold order with no subtraction; mean = pivot + s / N, scatter = M - s s^T / N."""
    K, F, d = s.shape
    pivot = np.asarray(pivot, dtype=np.float64)
    mu, W, c0 = np.zeros((F, K, d)), np.zeros((F, K, d, d)), np.zeros((F, K))
    for f, (cnt, offset, scatter) in enumerate(fold_training_moments(s, M, counts)):
        mu[f] = pivot[None] + offset
        if kind == "qda":
            W[f], c0[f] = _qda_models(cnt, scatter, reg_param)
        else:
            W[f], c0[f] = _lda_models(cnt, scatter)
    return mu, W, c0


def _moments_on_device(x_dev, codes, K, fold, F):
    """One ``group_moments`` launch over the rows of ``x_dev`` that have a code (``codes`` in [0, K); -1: the row is left
    out), stable-sorted by (code, fold) (``fold`` None: F = 1, by code alone) -> (s [K, F, d], M [K, F, d (d + 1) / 2],
    counts [K, F], fp64 numpy; the pivot, on the device): the mean of ALL rows of ``x_dev``.  No row with a code: zeros and
    no launch."""
    d, dev = int(x_dev.shape[1]), x_dev.device
    group = (codes + 1) * F + (fold if fold is not None else 0)                    # class-major: [1 + K, F], code -1 first
    counts = np.bincount(group, minlength=(K + 1) * F).astype(np.int64)
    order = np.argsort(group, kind="stable")[counts[:F].sum():]                    # without the rows that have no code
    counts = counts[F:]
    pivot = x_dev.mean(dim=0)                               # any pivot gives the same moments in exact arithmetic; the data's
    if order.size:                                          # mean keeps kappa = 1 + (mean - pivot)^2 / var as small as one pivot can
        offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        perm = torch.from_numpy(order.astype(np.int64)).to(dev)
        s, M = N.group_moments(x_dev.index_select(0, perm), torch.from_numpy(offsets).to(dev), pivot)
        s, M = s.cpu().numpy().reshape(K, F, d), M.cpu().numpy().reshape(K, F, -1)
    else:
        s, M = np.zeros((K, F, d)), np.zeros((K, F, d * (d + 1) // 2))
    return s, M, counts.reshape(K, F).astype(np.float64), pivot


def _scores_by_fold(x_dev, mu, W, c0, fold, return_scores):
    """``gauss_scores``' (label, best, second, scores) in the caller's order for the host models ``mu`` [F, K, d], ``W``
    [F, K, d, d], ``c0`` [F, K]: every cell under its own fold's model (the rows go to the kernel sorted by fold, with the
    permutation), or with ``fold`` None all of them under model 0."""
    dev = x_dev.device
    mu, W, c0 = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (mu, W, c0))
    if fold is None:
        model = torch.zeros(int(x_dev.shape[0]), dtype=torch.int32, device=dev)
        return N.gauss_scores(x_dev, model, mu, W, c0, None, return_scores)
    by_fold = np.argsort(fold, kind="stable")
    perm = torch.from_numpy(by_fold.astype(np.int64)).to(dev)
    model = torch.from_numpy(fold[by_fold].astype(np.int32)).to(dev)
    return N.gauss_scores(x_dev.index_select(0, perm), model, mu, W, c0, perm, return_scores)


def _cv_on_device(x_dev, codes, classes, fold, kfold, kind, reg_param, return_scores):
    """The two launches and the host factorisations between them, for points already on the device."""
    s, M, counts, pivot = _moments_on_device(x_dev, codes, len(classes), fold, kfold)
    mu, W, c0 = models_from_moments(s, M, counts, pivot.cpu().numpy(), kind, reg_param)
    label, best, second, scores = _scores_by_fold(x_dev, mu, W, c0, fold, return_scores)
    out = {"pred": label.cpu().numpy().astype(np.int64), "fold": fold, "best": best.cpu().numpy(),
           "second": second.cpu().numpy(), "classes": classes}
    if return_scores:
        out["scores"] = scores.cpu().numpy()
    return out


def _label_refusals(labels, n, kfold):
    """The labels as an array, after the refusals every cross-validated classifier begins with."""
    y = np.asarray(labels)
    if y.ndim != 1:
        raise ValueError(f"labels of shape {y.shape} are not 1-D")
    if y.shape[0] != n:
        raise ValueError(f"{y.shape[0]} labels for {n} samples")
    if int(kfold) != kfold or not 2 <= kfold <= n:
        raise ValueError(f"kfold = {kfold} outside [2, n = {n}]")
    return y


def _cv_refusals(labels, n, kfold, seed, kind):
    """(classes, codes, fold) after every refusal that needs no device."""
    if kind not in ("qda", "lda"):
        raise ValueError(f"kind = {kind!r}: one of 'qda', 'lda'")
    y = _label_refusals(labels, n, kfold)
    classes, codes = np.unique(y, return_inverse=True)
    codes = codes.reshape(-1)
    if len(classes) < 2:
        raise ValueError(f"The number of classes has to be greater than one; got {len(classes)} class")
    if len(classes) > N.GAUSSCLF_MAX_K or kfold > N.GAUSSCLF_MAX_F:
        raise NotImplementedError(f"{len(classes)} classes and {kfold} folds: at most {N.GAUSSCLF_MAX_K} and {N.GAUSSCLF_MAX_F}")
    fold = kfold_of(n, int(kfold), seed)
    if kind == "qda":
        per = np.bincount(codes * int(kfold) + fold, minlength=len(classes) * int(kfold)).reshape(len(classes), int(kfold))
        train = per.sum(axis=1, keepdims=True) - per
        bad = np.argwhere(train == 1)
        if len(bad):
            raise ValueError("y has only 1 sample in class %s, covariance is ill defined." % str(classes[bad[0][0]]))
    return classes, codes, fold


def _shape_of(x, max_d, max_n=None, min_n=0, who="", name="x"):
    """(n, d) of the points ``x`` after the refusals of its shape: 1 <= d <= ``max_d``, ``min_n`` <= n <= ``max_n``.  The
    messages begin with the function's name ``who``, where one is given, and call ``x`` ``name``."""
    lead = f"{who}: " if who else ""
    if not hasattr(x, "shape"):
        x = np.asarray(x)
    if len(x.shape) != 2:
        raise ValueError(f"{lead}{name} of shape {tuple(x.shape)} is not [n, d]")
    n, d = int(x.shape[0]), int(x.shape[1])
    if not 1 <= d <= max_d:
        raise NotImplementedError(f"{lead}d = {d} outside [1, {max_d}]")
    if max_n is not None and n > max_n:
        raise NotImplementedError(f"{lead}n = {n} above {max_n}")
    if n < min_n:
        raise ValueError(f"{lead}{name} has no rows")
    return n, d


def gaussian_cv_predict(x, labels, kfold, seed, kind="qda", reg_param=QDA_REG_PARAM, return_scores=False, device=None):
    """k-fold cross-validated prediction of ``labels`` from the points ``x`` by a Gaussian classifier, every cell scored
    under the model fitted to the folds it is not in.

    ``kind="qda"``: sklearn's ``QuadraticDiscriminantAnalysis(reg_param)`` -- per class the eigen-pairs lam, V of the
    unbiased covariance, S2 = (1 - reg) lam + reg, score = -|S2^(-1/2) V^T (x - mu)|^2 / 2 - sum(log S2) / 2 + log(N_k / N);
    a class with exactly one training cell in some fold raises sklearn's ValueError.  DEPARTURE: for a class with at most
    d training cells sklearn keeps only min(N_k, d) singular directions of the centred rows, the last of them an arbitrary
    vector of the null space, so the reference's own prediction there is not reproducible; this function uses all d
    eigen-directions of the regularised covariance (S2 = reg in the null space).  ``kind="lda"``: sklearn's
    ``LinearDiscriminantAnalysis()`` (solver "svd") -- the pooled within-class covariance over N - K_present, scaled by
    the within-class standard deviations, directions with a singular value <= 1e-4 dropped (which is what makes
    probabilities on the simplex work), score = -|W^T (x - mu)|^2 / 2 + log(N_k / N).  sklearn's second SVD over the class
    means only drops directions in which all classes score alike; it is not restated, so these scores differ from its
    ``decision_function`` by a term that is the same for every class of a cell.

    ``x``: array-like or tensor [n, d], d <= 128; a float32 tensor on the GPU is used where it lies, anything else is
    ROUNDED to float32 and uploaded.  ``labels``: 1-D, ints or hashables, encoded by ``np.unique``.  The folds are those
    of ``KFold(n_splits=kfold, shuffle=True, random_state=seed)`` (``kfold_of``).  Returns a dict: ``pred`` int64 [n] the
    predicted code (``classes[pred]`` the label), ``fold`` int64 [n], ``best`` and ``second`` float64 [n] the largest
    and second largest score (``best - second`` is the margin), ``classes``, and with ``return_scores`` the float64
    ``scores`` [n, K] (-inf for a class that the cell's fold never saw in training).  Everything on the device is fp64 on
    the float32 points, in an order fixed by the inputs: the same bits on every run.

    ValueError for fewer than two classes, ``kfold`` outside [2, n], a label length mismatch, non-finite ``x``;
    NotImplementedError under a process group and past d = 128, 4096 classes or 64 folds."""
    if D.is_dist():
        raise NotImplementedError("gaussian_cv_predict is not data-parallel: run it on one rank, outside the process group")
    n, _ = _shape_of(x, N.GAUSSCLF_MAX_D)
    classes, codes, fold = _cv_refusals(labels, n, kfold, seed, kind)
    return _cv_on_device(_points_on_device(x, device), codes, classes, fold, int(kfold), kind, float(reg_param), return_scores)


def _fold_lists(y, classes, pred, fold, kfold):
    """(acc, ref_labels, pred_labels) of the predicted codes ``pred``: lists over the folds, every test set in ascending order
    of the cell index."""
    acc, ref_labels, pred_labels = [], [], []
    for f in range(int(kfold)):
        test = np.flatnonzero(fold == f)
        predicted = classes[pred[test]]
        acc.append(float(np.average(y[test] == predicted)))                        # sklearn's accuracy_score
        pred_labels.append(predicted)
        ref_labels.append(y[test])
    return acc, ref_labels, pred_labels


def classify_points(x_dev, y, kfold, seed, kind, checked=None):
    """One label set on points already on the device: (acc, ref_labels, pred_labels, the ``gaussian_cv_predict`` dict), the
    first three lists over the folds with every test set in ascending order of the cell index."""
    y = np.asarray(y)
    classes, codes, fold = checked if checked is not None else _cv_refusals(y, int(x_dev.shape[0]), kfold, seed, kind)
    res = _cv_on_device(x_dev, codes, classes, fold, int(kfold), kind, QDA_REG_PARAM, False)
    return (*_fold_lists(y, classes, res["pred"], fold, kfold), res)


def _classifier(data, labels, kfold, seed, kind):
    """The three classifiers over a dict of label sets, ``kind`` "qda", "lda" or "rf": every key's refusals before any device
    work, one upload (and for the forest one binning) for all keys, then the keys in the dict's order."""
    if D.is_dist():
        raise NotImplementedError(f"{kind.upper()}_classifier is not data-parallel: run it on one rank, outside the process group")
    forest = kind == "rf"
    n, d = _shape_of(data, N.FOREST_MAX_D, N.FOREST_MAX_N) if forest else _shape_of(data, N.GAUSSCLF_MAX_D)
    checked = {key: _forest_refusals(labels[key], n, d, kfold, seed, FOREST_TREES, "sqrt") if forest
               else _cv_refusals(labels[key], n, kfold, seed, kind) for key in labels}
    points = _points_on_device(data, None)
    if forest:
        points = _bins_on_device(points)
    acc, ref_labels, pred_labels = {}, {}, {}
    for key in checked:
        if forest:
            out = classify_forest_points(points, labels[key], kfold, seed, FOREST_TREES, checked[key])
        else:
            out = classify_points(points, labels[key], kfold, seed, kind, checked[key])
        acc[key], ref_labels[key], pred_labels[key], _ = out
    return acc, ref_labels, pred_labels


def QDA_classifier(data, labels, kfold, seed):
    """The reference's ``QDA_classifier`` (cluster_analysis.py:62-83): ``(acc, ref_labels, pred_labels)``, dicts over the
    keys of the dict ``labels``, each a list over the folds of ``KFold(n_splits=kfold, random_state=seed, shuffle=True)``:
    the accuracy (a Python float), the held-out cells' labels and their predictions, in the caller's label values and in
    ascending order of the cell index.  ``data`` is uploaded once for all keys (a float32 device tensor is used where it
    lies; anything else is rounded to float32).  The model, its one departure from sklearn (classes of at most d
    training cells) and the refusals are those of ``gaussian_cv_predict(kind="qda")``."""
    return _classifier(data, labels, kfold, seed, "qda")


def LDA_classifier(data, labels, kfold, seed):
    """The reference's ``LDA_classifier`` (cluster_analysis.py:38-59): as ``QDA_classifier`` with
    ``gaussian_cv_predict(kind="lda")``."""
    return _classifier(data, labels, kfold, seed, "lda")


# ---- the random forest ----------------------------------------------------------------------------------------------------
FOREST_TREES = 100              # sklearn's RandomForestClassifier(n_estimators=100), the reference's default forest


def _bins_on_device(x_dev: torch.Tensor) -> torch.Tensor:
    """uint8 [n, d] on the device: per column, (the rank of a value's first occurrence in the sorted column * 256) // n."""
    n, d = (int(v) for v in x_dev.shape)
    sv, idx = torch.sort(x_dev + 0.0, dim=0, stable=True)                            # (+ 0.0: -0.0 becomes 0.0, one key)
    pos = torch.arange(n, dtype=torch.int64, device=x_dev.device).unsqueeze(1).repeat(1, d)
    pos[1:][sv[1:] == sv[:-1]] = 0
    first = torch.cummax(pos, dim=0).values
    out = torch.empty(n, d, dtype=torch.uint8, device=x_dev.device)
    out.scatter_(0, idx, ((first * N.FOREST_BINS) // n).to(torch.uint8))
    return out


def quantile_bins(x, device=None) -> torch.Tensor:
    """The forest's features: uint8 [n, d] on the device, per column ``bin = (r * 256) // n`` with r the rank of the value's
    first occurrence in the stably sorted column.  Equal values share a bin (-0.0 == 0.0), bins rise with the values, and
    with n <= 256 every distinct value has its own bin.  Integer arithmetic on ranks: the host restatement gives the same
    entries.  ``x`` as for ``silhouette_samples`` (FLOAT64 INPUT IS ROUNDED to float32 first); ValueError on NaN or
    infinity.  The sort is ``torch.sort`` on the device."""
    return _bins_on_device(_points_on_device(x, device))


def _forest_refusals(labels, n, d, kfold, seed, n_trees, max_features):
    """(classes, codes, fold, mtry) after every refusal that needs no device."""
    y = _label_refusals(labels, n, kfold)
    if int(n_trees) != n_trees or n_trees < 1:
        raise ValueError(f"n_trees = {n_trees} below 1")
    if max_features == "sqrt":
        mtry = max(1, int(np.floor(np.sqrt(d))))
    elif isinstance(max_features, (int, np.integer)) and 1 <= max_features <= d:
        mtry = int(max_features)
    else:
        raise ValueError(f"max_features = {max_features!r}: 'sqrt' or an int in [1, d = {d}]")
    classes, codes = np.unique(y, return_inverse=True)
    if len(classes) < 2:
        raise ValueError(f"The number of classes has to be greater than one; got {len(classes)} class")
    if len(classes) > N.FOREST_MAX_K or kfold > N.FOREST_MAX_F or n_trees > N.FOREST_MAX_T:
        raise NotImplementedError(f"{len(classes)} classes, {kfold} folds and {n_trees} trees: at most {N.FOREST_MAX_K}, "
                                  f"{N.FOREST_MAX_F} and {N.FOREST_MAX_T}")
    return classes, codes.reshape(-1), kfold_of(n, int(kfold), seed), mtry


def _forest_on_device(bins_dev, checked, kfold, n_trees, forest_seed, return_votes=False, return_trees=False):
    """The launches, for bins already on the device."""
    classes, codes, fold, mtry = checked
    dev = bins_dev.device
    label, best, second, votes, trees = N.forest_cv(bins_dev, torch.from_numpy(codes.astype(np.int32)).to(dev),
                                                    torch.from_numpy(fold.astype(np.int32)).to(dev), len(classes), int(kfold),
                                                    int(n_trees), mtry, forest_seed, return_votes, return_trees)
    out = {"pred": label.cpu().numpy().astype(np.int64), "fold": fold, "best": best.cpu().numpy(),
           "second": second.cpu().numpy(), "classes": classes}
    if return_votes:
        out["votes"] = votes.cpu().numpy()
    if return_trees:
        out["trees"] = {"count": trees["count"].cpu().numpy(), "nodes": trees["nodes"].cpu().numpy()}
    return out


def forest_cv_predict(x, labels, kfold, seed, n_trees=FOREST_TREES, max_features="sqrt", forest_seed=None, return_votes=False,
                      return_trees=False, device=None):
    """k-fold cross-validated prediction of ``labels`` from the points ``x`` by a random forest, every cell voted on by the
    ``n_trees`` trees grown on the folds it is not in (``mmvae_forest_cv``, csrc/forest.hip; the contract is stated in
    include/mmvae.h and DESIGN.md section 9i).

    The forest is sklearn's ``RandomForestClassifier(n_estimators=n_trees)``: bootstrap samples of the training rows, at every
    node ``max_features`` ("sqrt": max(1, floor(sqrt(d))); or an int in [1, d]) features drawn without replacement -- more
    while none of them can split --, the Gini-best split among them, the midpoint between adjacent training values as the
    threshold, trees grown until the leaves are pure.  DEPARTURES from sklearn: (1) the features are their 256 rank bins
    (``quantile_bins``), so thresholds are bin boundaries and not exact values; (2) every tree casts one hard vote, where
    sklearn averages the trees' leaf distributions -- the two are equal where leaves are pure, which they are unless rows
    with different labels share every bin; (3) the random numbers are Philox4x32-10 streams keyed by ``forest_seed``, not
    MT19937; (4) the forest is seeded: ``forest_seed`` defaults to ``seed``, and the same inputs give the same bits on every
    run, where the reference's ``RandomForestClassifier()`` draws from numpy's global state.

    ``x``: array-like or tensor [n, d], d <= 128; a float32 tensor on the GPU is used where it lies, anything else is
    ROUNDED to float32 and uploaded.  ``labels``: 1-D, ints or hashables, encoded by ``np.unique``; at most 128 classes.
    The folds are those of ``KFold(n_splits=kfold, shuffle=True, random_state=seed)`` (``kfold_of``); a class absent from a
    fold's training rows gets no votes in that fold.  Returns a dict: ``pred`` int64 [n] the predicted code
    (``classes[pred]`` the label; the lowest code on ties), ``fold`` int64 [n], ``best`` and ``second`` int32 [n] the votes
    of the prediction and the most votes among the other classes, ``classes``, with ``return_votes`` the int32 ``votes``
    [n, K], and with ``return_trees`` ``trees`` = {"count": int32 [kfold * n_trees], "nodes": int32 [kfold * n_trees, 2 n,
    4]}, tree f * n_trees + t the t-th of fold f, node j = (feature, thr, left child, rows) or (-1, class, 0, rows).

    ValueError for fewer than two classes, ``kfold`` outside [2, n], ``n_trees`` < 1, a bad ``max_features``, a label length
    mismatch, non-finite ``x``; NotImplementedError under a process group and past d = 128, 128 classes, 64 folds, 4096
    trees a fold or 2^24 cells."""
    if D.is_dist():
        raise NotImplementedError("forest_cv_predict is not data-parallel: run it on one rank, outside the process group")
    n, d = _shape_of(x, N.FOREST_MAX_D, N.FOREST_MAX_N)
    checked = _forest_refusals(labels, n, d, kfold, seed, n_trees, max_features)
    bins_dev = _bins_on_device(_points_on_device(x, device))
    return _forest_on_device(bins_dev, checked, kfold, n_trees, seed if forest_seed is None else forest_seed, return_votes,
                             return_trees)


def classify_forest_points(bins_dev, y, kfold, seed, n_trees, checked):
    """One label set on bins already on the device: (acc, ref_labels, pred_labels, the ``forest_cv_predict`` dict), the first
    three lists over the folds with every test set in ascending order of the cell index."""
    y = np.asarray(y)
    classes, fold = checked[0], checked[2]
    res = _forest_on_device(bins_dev, checked, kfold, n_trees, seed)
    return (*_fold_lists(y, classes, res["pred"], fold, kfold), res)


def RF_classifier(data, labels, kfold, seed):
    """The reference's ``RF_classifier`` (cluster_analysis.py:14-35): ``(acc, ref_labels, pred_labels)``, dicts over the keys
    of the dict ``labels``, each a list over the folds of ``KFold(n_splits=kfold, random_state=seed, shuffle=True)``: the
    accuracy (a Python float), the held-out cells' labels and their predictions, in the caller's label values and in
    ascending order of the cell index.  ``data`` is uploaded and binned once for all keys (a float32 device tensor is used
    where it lies; anything else is rounded to float32).  The forest is ``forest_cv_predict``'s with 100 trees and
    ``forest_seed = seed``; its departures from sklearn's forest are stated there: 256 rank bins instead of exact
    thresholds, hard votes instead of averaged leaf distributions, Philox instead of MT19937 streams, and a seeded forest
    -- the reference's own call draws from numpy's global state and cannot be reproduced; this one can."""
    return _classifier(data, labels, kfold, seed, "rf")

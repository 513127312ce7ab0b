"""The clusterability scores of the reference's ``mmidas/utils/cluster_analysis.py``: ``get_SilhScore`` and the silhouette
half of ``cluster_compare``, on the device, without sklearn.

The reference calls ``sklearn.metrics.silhouette_samples`` / ``silhouette_score`` (euclidean) on the latents: n^2 distances,
which sklearn computes on the host in float64 through the Gram expansion.  Here the cells are sorted by label on the host,
uploaded once, and ``mmvae_silhouette`` (csrc/silhouette.hip) forms every distance in fp32 in difference
form and everything after it in fp64; the per-cell scores come back as float64 and the means are numpy's, over the classes
in ``np.unique`` order.  ``K_selection`` and the RF / LDA / QDA classifiers of that module are not part of this package."""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from .. import _native as N
from .. import dist as D
from ..cpl_mixvae import get_device


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
    """float32 [n, d] on ``device``: a float32 device tensor as it is, anything else converted (float64 is rounded)."""
    if isinstance(x, torch.Tensor) and x.dtype == torch.float32 and x.device.type == "cuda":
        if x.dim() != 2:
            raise ValueError(f"x of shape {tuple(x.shape)} is not [n, d]")
        if not bool(torch.isfinite(x).all()):
            raise ValueError("x holds NaN or infinity")
        return x
    h = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    if h.ndim != 2:
        raise ValueError(f"x of shape {h.shape} is not [n, d]")
    with np.errstate(over="ignore"):
        h = np.ascontiguousarray(h, dtype=np.float32)
    if not np.isfinite(h).all():
        raise ValueError("x holds NaN or infinity (or a value float32 cannot hold)")
    return torch.from_numpy(h).to(get_device(device))


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


def cluster_compare(data, labels, num_pc=0, saving_path=''):
    """The reference's ``cluster_compare`` (cluster_analysis.py:87-120): ``(fig, silh_smp_score, sil_score, c_size)`` for the
    dict ``labels`` of label arrays -- per entry the per-class mean silhouette samples (classes in ``np.unique`` order), the
    overall score, and the class sizes ordered by ascending mean score -- all on the projection of ``data`` onto its top
    ``num_pc`` principal components.

    The projection is plumbing, not a hot path: numpy's exact SVD of the centred data in fp64 on the host, which is what
    sklearn's ``PCA(svd_solver="full")`` computes (the silhouette does not see the components' signs).  sklearn's default
    solver is a randomised one at large sizes, so at those sizes the reference's own numbers are not reproducible either.
    The projected points are rounded to float32, uploaded once and scored for every entry of ``labels``.  ``fig`` shows what
    the reference's figure shows, or is None when matplotlib is not installed.  Departure: ``num_pc == 0`` raises ValueError
    (the reference fails there with an unbound local).  ``saving_path`` is unused, as in the reference."""
    if num_pc <= 0:
        raise ValueError("cluster_compare: num_pc must be positive (the reference computes nothing for num_pc = 0)")
    if D.is_dist():
        raise NotImplementedError("cluster_compare is not data-parallel: run it on one rank, outside the process group")
    z = _project(data, num_pc)
    encoded = {key: _encode(labels[key], z.shape[0]) for key in labels}           # every refusal before any device work
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

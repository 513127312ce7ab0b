"""Principal components on the device: the linear baseline of the reference's clusterability analysis
(``cluster_compare(data, labels, num_pc)`` of ``mmidas/utils/cluster_analysis.py`` and "Linear vs Non-linear embedding" of
``notebooks/4_clusterability.ipynb``), exact and deterministic, without sklearn and without a host copy of the matrix.

The reference calls ``sklearn.decomposition.PCA``, which at the data set's size (22 365 cells x 5032 genes) switches to a
randomised solver, so its own numbers are not reproducible there; an exact SVD of the centred matrix on the host is
O(N D^2) in fp64 and takes about a minute.  Here the covariance is one pass over the fp32 matrix where it lies
(``mmvae_gram``, csrc/pca.hip, on the fp64 MFMA), the top-k subspace comes from block subspace
iteration with Rayleigh-Ritz whose only large product, covariance times block, is ``mmvae_symm_mul``, and the projection is
``mmvae_pca_project``.  What stays on the host is a D x b QR and a b x b ``eigh`` per iteration (b <= 64): plumbing.

``subspace_iteration`` is written over a multiply callable so that it can be driven by numpy (tests) or by the device
(``pca_fit``).  The result is a function of the inputs alone: the start block is a seeded numpy normal matrix, every device
sum has a fixed order, so two fits of the same input give the same bits."""
from __future__ import annotations

import warnings
from dataclasses import dataclass
from typing import Callable, Optional

import numpy as np
import torch

from .. import _native as N
from .. import dist as D
from .._utils import float32_on_device

MAX_COMPONENTS = N.PCA_MAX_BLOCK      # the widest block of mmvae_symm_mul and mmvae_pca_project


@dataclass
class PCAFit:
    """What ``pca_fit`` returns.  ``mean`` float64 [D]; ``components`` float64 [k, D], orthonormal rows, in each the entry of
    largest magnitude positive (the lowest index on ties); ``explained_variance`` float64 [k] (ddof 1), descending;
    ``explained_variance_ratio`` = explained_variance / total_variance; ``total_variance`` the covariance's trace;
    ``residual`` the Frobenius norm of C V - V diag(theta) over the k columns; ``gap`` theta_k - theta_(k+1), the Ritz estimate
    of the spectral gap behind the subspace (NaN when the block holds no (k+1)-th value); ``iterations`` of the subspace
    iteration (0 for ``solver="eigh"``); ``converged`` whether that iteration met ``tol``; ``solver_used`` "subspace" or
    "eigh"."""
    mean: np.ndarray
    components: np.ndarray
    explained_variance: np.ndarray
    explained_variance_ratio: np.ndarray
    total_variance: float
    residual: float
    gap: float
    iterations: int
    converged: bool
    solver_used: str


def sign_flip(components: np.ndarray) -> np.ndarray:
    """sklearn's ``svd_flip(u_based_decision=False)``: every row's entry of largest magnitude made positive (``np.argmax``:
    the lowest index on ties)."""
    components = np.array(components, dtype=np.float64)
    at = np.argmax(np.abs(components), axis=1)
    signs = np.sign(components[np.arange(components.shape[0]), at])
    signs[signs == 0] = 1.0
    return components * signs[:, None]


def subspace_iteration(mul: Callable[[np.ndarray], np.ndarray], dim: int, k: int, b: int, tol: float = 1e-10,
                       max_iter: int = 300, seed: int = 0) -> dict:
    """Block subspace iteration with Rayleigh-Ritz for the top ``k`` eigen-pairs of the symmetric positive semi-definite
    ``dim`` x ``dim`` matrix C given only as ``mul``: Q [dim, b] -> C Q.  The start block is
    ``np.random.RandomState(seed).standard_normal((dim, b))``, QR-factored.  Each iteration: Y = C Q; T = Q^T Y, symmetrised;
    (theta, W) = eigh(T), descending; V = Q W; R = Y W - V diag(theta); converged when max_{j < k} |r_j|_2 <= tol theta_1;
    else Q = qr(Y).  Returns ``{"V" [dim, k], "theta" [b], "residual", "gap", "iterations", "converged"}`` of the last
    iteration made, converged or not: the caller decides what an unconverged subspace is worth."""
    if not 1 <= k <= b <= dim:
        raise ValueError(f"subspace_iteration: need 1 <= k = {k} <= b = {b} <= dim = {dim}")
    Q, _ = np.linalg.qr(np.random.RandomState(seed).standard_normal((dim, b)))
    out = None
    for it in range(1, int(max_iter) + 1):
        Y = np.asarray(mul(Q), dtype=np.float64)
        T = Q.T @ Y
        theta, W = np.linalg.eigh(0.5 * (T + T.T))
        theta, W = theta[::-1], W[:, ::-1]
        V = Q @ W
        R = Y @ W - V * theta
        norms = np.sqrt(np.sum(R[:, :k] ** 2, axis=0))
        done = bool(norms.max() <= tol * theta[0])
        out = {"V": V[:, :k], "theta": theta, "residual": float(np.sqrt(np.sum(norms ** 2))),
               "gap": float(theta[k - 1] - theta[k]) if b > k else float("nan"), "iterations": it, "converged": done}
        if done:
            break
        Q, _ = np.linalg.qr(Y)
    return out


def eigh_top(C: np.ndarray, k: int) -> dict:
    """The same dict from ``np.linalg.eigh`` of the whole matrix: the exact route, O(dim^3) on the host."""
    C = np.asarray(C, dtype=np.float64)
    lam, U = np.linalg.eigh(C)
    lam, U = lam[::-1], U[:, ::-1]
    V = U[:, :k]
    R = C @ V - V * lam[:k]
    return {"V": V, "theta": lam, "residual": float(np.sqrt(np.sum(R ** 2))),
            "gap": float(lam[k - 1] - lam[k]) if C.shape[0] > k else float("nan"), "iterations": 0, "converged": True}


def fit_from_covariance(mul, C_host: Callable[[], np.ndarray], mean, total_variance: float, k: int, solver: str = "subspace",
                        oversample: Optional[int] = None, tol: float = 1e-10, max_iter: int = 300, seed: int = 0) -> PCAFit:
    """``pca_fit`` after the covariance exists: ``mul`` multiplies by it, ``C_host()`` fetches it (called only on the
    ``eigh`` route).  The subspace route that has not converged by ``max_iter`` falls back to ``eigh`` with a warning; an
    unconverged subspace is never returned."""
    dim = int(np.asarray(mean).shape[0])
    if solver not in ("subspace", "eigh"):
        raise ValueError(f"solver = {solver!r}: one of 'subspace', 'eigh'")
    if not 1 <= k <= dim:
        raise ValueError(f"n_components = {k} outside [1, D = {dim}]")
    iterations, converged, used = 0, False, solver
    if solver == "subspace":
        if oversample is None:
            oversample = max(8, k)
        b = min(dim, k + int(oversample))
        if b > MAX_COMPONENTS:
            raise NotImplementedError(f"a block of {b} = n_components + oversample vectors: at most {MAX_COMPONENTS}")
        res = subspace_iteration(mul, dim, k, b, tol, max_iter, seed)
        iterations, converged = res["iterations"], res["converged"]
        if not converged:
            warnings.warn(f"pca_fit: subspace iteration has not converged in {max_iter} iterations (residual "
                          f"{res['residual']:.3e}, gap {res['gap']:.3e}); falling back to eigh of the covariance", RuntimeWarning)
            used = "eigh"
    if used == "eigh":
        res = eigh_top(C_host(), k)
        if solver == "eigh":
            converged = True
    theta = np.array(res["theta"][:k], dtype=np.float64)
    return PCAFit(mean=np.asarray(mean, dtype=np.float64), components=sign_flip(res["V"].T), explained_variance=theta,
                  explained_variance_ratio=theta / total_variance if total_variance > 0 else np.full(k, np.nan),
                  total_variance=float(total_variance), residual=res["residual"], gap=res["gap"], iterations=int(iterations),
                  converged=bool(converged), solver_used=used)


def _matrix_on_device(data, device) -> torch.Tensor:
    """float32 [n_total, D] on the device (its values are checked later, in chunks: ``_pivot``)."""
    return float32_on_device(data, device, "data", "[n, D]")


def _rows_on_device(rows, n_total: int, device) -> Optional[torch.Tensor]:
    if rows is None:
        return None
    r = rows if isinstance(rows, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(rows), dtype=np.int64))
    r = r.to(device=device, dtype=torch.int64).reshape(-1)
    if r.numel() and (int(r.min()) < 0 or int(r.max()) >= n_total):
        raise IndexError(f"rows outside [0, {n_total})")
    return r


ROW_CHUNK = 8192      # rows gathered at a time for the pivot and the finiteness check: 165 MB at D = 5032


def _pivot(x: torch.Tensor, rows: Optional[torch.Tensor]) -> torch.Tensor:
    """The fp32 column means of the selected rows, by torch, a chunk of rows at a time; ValueError on a non-finite value."""
    n = int(x.shape[0]) if rows is None else int(rows.numel())
    total = torch.zeros(x.shape[1], dtype=torch.float64, device=x.device)
    for i in range(0, n, ROW_CHUNK):
        piece = x[i:i + ROW_CHUNK] if rows is None else x.index_select(0, rows[i:i + ROW_CHUNK])
        total += piece.sum(dim=0, dtype=torch.float64)
    if not bool(torch.isfinite(total).all()):
        raise ValueError("data holds NaN or infinity")
    return (total / n).to(torch.float32)


def pca_fit(data, n_components: int, rows=None, solver: str = "subspace", oversample: Optional[int] = None, tol: float = 1e-10,
            max_iter: int = 300, seed: int = 0, device=None) -> PCAFit:
    """The top ``n_components`` principal components of ``data`` [n_total, D] (of its rows ``rows``, in any order, where
    given): what sklearn's ``PCA(n_components, svd_solver="full")`` computes, on the device.

    ``data``: a float32 tensor on the GPU is read where it lies; anything else is converted to float32 -- FLOAT64 INPUT IS
    ROUNDED to float32 -- and uploaded.  The covariance is exact fp64 arithmetic on those float32 values about the pivot
    (their fp32 column means, by torch): ``mmvae_gram``; any pivot gives the same covariance up to rounding, and the error
    bound grows with kappa = 1 + (mean - pivot)^2 / variance only.  ``solver="subspace"``: block subspace iteration with
    Rayleigh-Ritz on a block of b = min(D, n_components + oversample) vectors (``oversample`` defaults to
    max(8, n_components); b <= 64), the start block ``np.random.RandomState(seed)``'s, converged when every one of the first
    n_components residual columns is at most ``tol`` times the largest eigenvalue.  The iteration converges at the rate
    lambda_(b+1) / lambda_k: a flat spectrum does not converge, and by ``max_iter`` the fit FALLS BACK to ``np.linalg.eigh``
    of the device-made covariance on the host (O(D^3)), says so through ``solver_used = "eigh"`` and a RuntimeWarning, and never
    returns an unconverged subspace.  ``solver="eigh"`` takes that route directly.  Returns a ``PCAFit``.

    ValueError for non-finite data, fewer than two rows, n_components outside [1, D]; NotImplementedError under a process
    group, for D > 32768 and for a block wider than 64."""
    if D.is_dist():
        raise NotImplementedError("pca_fit is not data-parallel: run it on one rank, outside the process group")
    k = int(n_components)
    shape = tuple(data.shape) if hasattr(data, "shape") else np.asarray(data).shape
    if len(shape) != 2:
        raise ValueError(f"data of shape {shape} is not [n, D]")
    if not 1 <= k <= shape[1]:
        raise ValueError(f"n_components = {n_components} outside [1, D = {shape[1]}]")
    if solver not in ("subspace", "eigh"):
        raise ValueError(f"solver = {solver!r}: one of 'subspace', 'eigh'")
    if shape[1] > N.GRAM_MAX_D:
        raise NotImplementedError(f"D = {shape[1]} above {N.GRAM_MAX_D}")
    if solver == "subspace" and min(shape[1], k + (max(8, k) if oversample is None else int(oversample))) > MAX_COMPONENTS:
        raise NotImplementedError(f"n_components + oversample above {MAX_COMPONENTS}")
    n = shape[0] if rows is None else int(len(rows))
    if n < 2:
        raise ValueError(f"{n} rows: a covariance needs at least two")
    x = _matrix_on_device(data, device)
    r = _rows_on_device(rows, int(x.shape[0]), x.device)
    pivot = _pivot(x, r)
    s, C = N.gram(x, pivot, r, cov=True)
    mean = pivot.double().cpu().numpy() + s.cpu().numpy() / n
    total = float(torch.diagonal(C).sum().item())

    def mul(Q):
        return N.symm_mul(C, torch.from_numpy(np.ascontiguousarray(Q)).to(x.device)).cpu().numpy()

    return fit_from_covariance(mul, lambda: C.cpu().numpy(), mean, total, k, solver, oversample, tol, max_iter, seed)


def pca_transform(fit: PCAFit, data, rows=None, out: str = "numpy", device=None):
    """``data`` (its rows ``rows`` where given, in that order) on the components of ``fit``: ((double)x - mean) V in fp64 on
    the device (``mmvae_pca_project``).  ``out="numpy"``: float64 numpy [n, k].  ``out="device"``: the same values rounded to
    float32, as a device tensor that ``classify_points`` and the silhouette take as they are.  ``data`` as for ``pca_fit``
    (FLOAT64 INPUT IS ROUNDED to float32)."""
    if out not in ("numpy", "device"):
        raise ValueError(f"out = {out!r}: one of 'numpy', 'device'")
    if D.is_dist():
        raise NotImplementedError("pca_transform is not data-parallel: run it on one rank, outside the process group")
    x = _matrix_on_device(data, device)
    if int(x.shape[1]) != fit.mean.shape[0]:
        raise ValueError(f"data of {int(x.shape[1])} columns on a fit of {fit.mean.shape[0]}")
    r = _rows_on_device(rows, int(x.shape[0]), x.device)
    Z = N.pca_project(x, torch.from_numpy(fit.mean).to(x.device),
                      torch.from_numpy(np.ascontiguousarray(fit.components.T)).to(x.device), r)
    return Z.cpu().numpy() if out == "numpy" else Z.to(torch.float32)


def pca_project(data, num_pc: int, rows=None, out: str = "numpy", **kw):
    """``pca_fit`` followed by ``pca_transform`` of the same rows: the matrix is uploaded once.  Keywords as ``pca_fit``."""
    if D.is_dist():
        raise NotImplementedError("pca_project is not data-parallel: run it on one rank, outside the process group")
    if out not in ("numpy", "device"):
        raise ValueError(f"out = {out!r}: one of 'numpy', 'device'")
    device = kw.pop("device", None)
    if not (isinstance(data, torch.Tensor) and data.dtype == torch.float32 and data.device.type == "cuda"):
        shape = tuple(data.shape) if hasattr(data, "shape") else np.asarray(data).shape      # the refusals that need no device
        if len(shape) != 2 or not 1 <= int(num_pc) <= shape[1]:
            raise ValueError(f"num_pc = {num_pc} components of data of shape {shape}")
        data = _matrix_on_device(data, device)
    fit = pca_fit(data, num_pc, rows=rows, **kw)
    return pca_transform(fit, data, rows=rows, out=out)

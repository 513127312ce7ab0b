"""Consensus utilities of mmidas/_utils.py:68-129 on the device.

Same names and meaning as the reference; inputs and outputs are CUDA tensors instead of numpy arrays, the arithmetic
runs in the HIP library (csrc/consensus.hip) and the values are bit-identical to the reference's numpy code
(integer counts; fp64 division and numpy's summation order for the mean).  No CPU fallback.

``reassign`` and ``mk_masks`` (_utils.py:68-75) are host functions on small numpy arrays, as in the reference.
"""
from typing import Optional

import numpy as np
import torch

from . import _native as N


def classify(probs: torch.Tensor) -> torch.Tensor:
    """_utils.py:79-80 ``np.argmax(probs, axis=-1)``: int32 labels, first maximum on ties."""
    return N.classify(probs)


def confmat_counts(n_arm: int, K: int, device) -> torch.Tensor:
    """Zeroed int64 [n_arm (n_arm - 1) / 2, K, K] accumulator for ``mixVAE_model.eval_labels(..., counts=)``."""
    return torch.zeros(max(n_arm * (n_arm - 1) // 2, 1), K, K, dtype=torch.int64, device=device)


def compute_confmat(labels1: torch.Tensor, labels2: torch.Tensor, K: Optional[int] = None) -> torch.Tensor:
    """_utils.py:84-95: K x K float64 matrix with ``m[labels1[i], labels2[i]] += 1``.  K None: number of distinct
    labels of the fuller side, as the reference."""
    assert len(labels1) == len(labels2)
    assert labels1.dim() == labels2.dim() == 1
    assert labels1.dtype == labels2.dtype and labels1.dtype in (torch.int64, torch.int32)
    if K is None:
        K = max(int(torch.unique(labels1).numel()), int(torch.unique(labels2).numel()))
    lab = torch.stack([labels1, labels2]).to(torch.int32)
    return N.confmat_accumulate(lab, K)[0].to(torch.float64)


def confmat_normalize(cm: torch.Tensor) -> torch.Tensor:
    """_utils.py:98-100: divide column j by max(column sum j, row sum j), 0 where that is 0."""
    counts = cm.to(torch.int64).unsqueeze(0)
    if not torch.equal(counts[0].to(cm.dtype), cm):
        raise ValueError("confmat_normalize on the device takes a matrix of counts (integers)")
    return N.consensus(counts, want_norm=True)[1][0]


def confmat_mean(cm: torch.Tensor) -> torch.Tensor:
    """_utils.py:128-129: mean of the diagonal (fp64, numpy's pairwise summation order), a 0-d device tensor."""
    d = torch.diagonal(cm).to(torch.float64)
    return _np_pairwise_sum(d) / d.numel()


def _np_pairwise_sum(v: torch.Tensor) -> torch.Tensor:
    """numpy's pairwise_sum on a 1-D fp64 device tensor, same association order (bit-identical result)."""
    n = v.numel()
    if n < 8:
        r = torch.zeros((), dtype=torch.float64, device=v.device)
        for i in range(n):
            r = r + v[i]
        return r
    if n > 128:
        n2 = n // 2
        n2 -= n2 % 8
        return _np_pairwise_sum(v[:n2]) + _np_pairwise_sum(v[n2:])
    m = n - n % 8
    acc = v[0:8].clone()
    for i in range(8, m, 8):
        acc = acc + v[i:i + 8]
    res = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]))
    for i in range(m, n):
        res = res + v[i]
    return res


def consensus_from_counts(counts: torch.Tensor) -> torch.Tensor:
    """``confmat_mean(confmat_normalize(cm))`` for every arm pair in one launch: float64 [pairs]."""
    return N.consensus(counts)


def float32_on_device(a, device, what: str, shape_words: str, check_device_finite: bool = False) -> torch.Tensor:
    """``a`` as float32 [., .] on ``device`` for the analysis routines of ``utils/``: a float32 device tensor as it is (with
    its stride), anything else rounded to float32 and uploaded (a read-only array through a copy).  ``what`` and
    ``shape_words`` name the argument and its shape in the messages.  Host input is always checked for NaN and infinity; a
    device tensor only with ``check_device_finite`` (otherwise finite values are the caller's side of the kernel's contract)."""
    if isinstance(a, torch.Tensor) and a.dtype == torch.float32 and a.device.type == "cuda":
        if a.dim() != 2:
            raise ValueError(f"{what} of shape {tuple(a.shape)} is not {shape_words}")
        if check_device_finite and not bool(torch.isfinite(a).all()):
            raise ValueError(f"{what} holds NaN or infinity")
        return a
    from .cpl_mixvae import get_device          # (cpl_mixvae imports this module, inside its functions)
    h = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    if h.ndim != 2:
        raise ValueError(f"{what} of shape {h.shape} is not {shape_words}")
    with np.errstate(over="ignore"):
        h = np.ascontiguousarray(h, dtype=np.float32)
    if not np.isfinite(h).all():
        raise ValueError(f"{what} holds NaN or infinity (or a value float32 cannot hold)")
    return torch.from_numpy(h if h.flags.writeable else h.copy()).to(get_device(device))


def mk_masks(bias):
    """_utils.py:74-75: ``(pruning_mask, inds_prune)`` = the indices of the non-zero / zero entries of a bias vector
    (the categories a pruned model keeps / has dropped), int64 numpy arrays."""
    b = bias.detach().cpu().numpy() if isinstance(bias, torch.Tensor) else np.asarray(bias)
    return np.where(b != 0)[0], np.where(b == 0)[0]


def _assign_min(cost: np.ndarray) -> np.ndarray:
    """Minimum-cost assignment of a square matrix by shortest augmenting paths with row / column potentials (the
    Hungarian method in its O(K^3) form; the scan over the columns is vectorised): ``col[i]`` = the column of row i."""
    n = cost.shape[0]
    u, v = np.zeros(n + 1), np.zeros(n + 1)
    p = np.zeros(n + 1, dtype=np.int64)             # p[j]: the row (1-based) matched to column j; column 0 is virtual
    way = np.zeros(n + 1, dtype=np.int64)
    for i in range(1, n + 1):
        p[0] = i
        j0 = 0
        minv = np.full(n + 1, np.inf)
        used = np.zeros(n + 1, dtype=bool)
        while True:
            used[j0] = True
            i0 = p[j0]
            cur = cost[i0 - 1] - u[i0] - v[1:]
            upd = ~used[1:] & (cur < minv[1:])
            minv[1:][upd] = cur[upd]
            way[1:][upd] = j0
            cand = np.where(used[1:], np.inf, minv[1:])
            j1 = int(np.argmin(cand)) + 1
            delta = cand[j1 - 1]
            u[p[used]] += delta
            v[used] -= delta
            minv[~used] -= delta
            j0 = j1
            if p[j0] == 0:
                break
        while j0:
            j1 = way[j0]
            p[j0] = p[j1]
            j0 = j1
    col = np.zeros(n, dtype=np.int64)
    col[p[1:] - 1] = np.arange(n)
    return col


def reassign(x):
    """_utils.py:68-70: the columns of the square matrix x permuted by a maximum-weight assignment
    (``linear_sum_assignment(-x)``), solved here in numpy (the package does not import scipy).  Which of several optimal
    assignments is taken may differ from scipy's; ``np.mean(np.diag(reassign(x)))`` -- all any caller uses -- is the optimal
    value over K either way."""
    x = np.asarray(x)
    if x.ndim != 2 or x.shape[0] != x.shape[1]:
        raise ValueError(f"reassign takes a square matrix, got {x.shape}")
    n = x.shape[0]
    if n == 0:
        return x
    w = x.astype(np.float64)
    rows, cols = np.flatnonzero(w.any(axis=1)), np.flatnonzero(w.any(axis=0))
    if (len(rows) == n and len(cols) == n) or (w < 0).any():
        return x[:, _assign_min(-w)]
    # A non-negative matrix with all-zero rows or columns (a confusion matrix of arms that use a few of K categories; the
    # solver walks K^2 ties there: 99 ms at K = 92 with three labels): those rows and columns add nothing whichever way they
    # are matched, so the assignment is solved on the rest, padded square with zeros (an unmatched row or column of the rest
    # costs nothing either), and the remaining rows take the remaining columns in order.
    m = max(len(rows), len(cols))
    sub = np.zeros((m, m))
    sub[:len(rows), :len(cols)] = w[np.ix_(rows, cols)]
    col = np.full(n, -1, dtype=np.int64)
    if m:
        c = _assign_min(-sub)[:len(rows)]
        real = c < len(cols)
        col[rows[real]] = cols[c[real]]
    col[col < 0] = np.setdiff1d(np.arange(n), col[col >= 0])
    return x[:, col]

"""Marker genes of the categories: the Wilcoxon rank-sum (Mann-Whitney) test of every gene, each group of cells against the
rest, on the device, without scipy.

``scipy.stats.mannwhitneyu(x[group], x[rest], use_continuity=False, method="asymptotic")`` gene by gene, or scanpy's
``rank_genes_groups(method="wilcoxon", tie_correct=True)``, sort every gene's column on the host.  Here ``mmvae_rank_sum``
(csrc/ranksum.hip) ranks every gene in one workgroup's LDS and returns, for every group at once, TWICE
the rank sums, the tie term and the counts as exact integers; the statistic, its p-value and the Benjamini-Hochberg
adjustment are then formed in numpy float64 on the host from those integers.  At most ``MAX_CELLS`` = 32768 cells a call and
``MAX_GROUPS`` = 4096 groups; NaN is refused in host input and not checked for in a device tensor (a gene that holds one gets
unspecified results).  With ``block_cells`` (``"auto"`` or a block size) ``mmvae_rank_sum_blocked`` takes
up to ``MAX_CELLS_BLOCKED`` = 1048576 cells: the cells are cut into blocks that are sorted one by one, and a cell's rank is
added up over the blocks -- the same integers.  Not offered: more cells than that, a default that changes paths by itself,
data-parallel use, other tests, the continuity correction, and group-against-group tests."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from .. import _native as N
from .. import dist as D

MAX_CELLS = 32768      # MMVAE_RANKSUM_MAX_N (include/mmvae.h): the keys of one gene fill 128 KiB of a workgroup's LDS
MAX_CELLS_BLOCKED = 1 << 20   # MMVAE_RANKSUM_BLOCKED_MAX_N: n^3 - n, the tie term of an all-tied gene, stays below 2^60
MIN_BLOCK = 128        # RSB_MIN_BLOCK: the smallest block of the blocked path; the largest is MAX_CELLS
MAX_GROUPS = 4096      # RS_MAX_G (csrc/common.hpp)
CHUNK = 512            # RS_CHUNK: genes of the gene-major staging copy, which is the workspace

_bound = [False]


def _lib():
    """The library with the rank-sum entries' signatures declared (here, as augmentation.py declares its own)."""
    L = N.lib()
    if not _bound[0]:
        vp, i64, i32 = C.c_void_p, C.c_int64, C.c_int
        L.mmvae_rank_sum_workspace_bytes.argtypes = [i64, i32, i32]
        L.mmvae_rank_sum_workspace_bytes.restype = C.c_size_t
        L.mmvae_rank_sum.argtypes = [vp, i64, i64, i32, vp, i64, vp, i32, C.c_float, vp, C.c_size_t, vp, vp, vp, vp, vp]
        L.mmvae_rank_sum_blocked_workspace_bytes.argtypes = [i64, i32, i32, i32]
        L.mmvae_rank_sum_blocked_workspace_bytes.restype = C.c_size_t
        L.mmvae_rank_sum_blocked.argtypes = [vp, i64, i64, i32, vp, i64, vp, i32, C.c_float, i32, vp, C.c_size_t, vp, vp, vp, vp, vp]
        L.mmvae_debug_rank_sum_blocked.argtypes = [vp, i64, i64, i32, vp, i64, vp, i32, C.c_float, i32, vp, C.c_size_t, vp, vp, vp, vp,
                                                   i32, i32, vp]
        _bound[0] = True
    return L


def _block_of(block_cells, n: int, who: str):
    """None for the one-call path, else the ``block`` argument of mmvae_rank_sum_blocked (0: its default); the refusals of
    ``block_cells`` and of ``n`` cells, which come before any device work."""
    if block_cells is None or (isinstance(block_cells, str) and block_cells == "auto" and n <= MAX_CELLS):
        if n > MAX_CELLS:
            why = " (the keys of one gene must fit one workgroup's LDS)" if who == "rank_sum_test" else ""
            raise NotImplementedError(f"{who}: {n} cells above the {MAX_CELLS} of one call{why}; block_cells=\"auto\" takes up to "
                                      f"{MAX_CELLS_BLOCKED}")
        return None
    if isinstance(block_cells, str) and block_cells == "auto":
        block = 0
    else:
        if isinstance(block_cells, (str, bool)) or not isinstance(block_cells, (int, np.integer)):
            raise ValueError(f"{who}: block_cells = {block_cells!r} is not None, \"auto\" or an int")
        block = int(block_cells)
        if not (MIN_BLOCK <= block <= MAX_CELLS and block & (block - 1) == 0):
            raise ValueError(f"{who}: block_cells = {block} is not a power of two in [{MIN_BLOCK}, {MAX_CELLS}]")
    if n > MAX_CELLS_BLOCKED:
        raise NotImplementedError(f"{who}: {n} cells above the {MAX_CELLS_BLOCKED} of the blocked path")
    return block


def _buffer(shape, dtype, device) -> torch.Tensor:
    """An uninitialised 8-byte-element device buffer: a view of a ``_native._workspace``, so that it is guarded with it."""
    numel = int(np.prod(shape))
    return N._workspace(8 * numel, device)[:numel].view(dtype).view(*shape)


def rank_sums(x: torch.Tensor, rows: Optional[torch.Tensor], offsets: torch.Tensor, eps: float = 0.0, block_cells=None):
    """mmvae_rank_sum on device tensors: float32 ``x`` [n_total, D] (rows may be strided, columns not; read where it lies),
    the int64 row map ``rows`` [n] ordered by group (None: the rows 0..n-1, n = offsets[-1]) and int64 ``offsets`` [G + 1] ->
    (rank_sum2 int64 [G, D], tie_term int64 [D], n_pos int64 [G, D], sum float64 [G, D]) on the device.  ``offsets`` is read
    on the host only for its last entry when ``rows`` is None.  ``block_cells``: None the one-call path (at most 32768 cells);
    "auto" that path up to 32768 cells and mmvae_rank_sum_blocked with its default block above, up to 1048576 cells; an int
    (a power of two in [128, 32768]) mmvae_rank_sum_blocked with blocks of that many cells, at any n up to 1048576 -- the
    same integers, and up to 32768 cells the same bits."""
    N._need_cuda("rank_sum", x, rows, offsets)
    if x.dtype != torch.float32 or x.dim() != 2:
        raise TypeError("rank_sum: x must be float32 [n_total, D]")
    if offsets.dtype != torch.int64 or offsets.dim() != 1 or offsets.numel() < 2:
        raise TypeError("rank_sum: offsets must be int64 [G + 1]")
    n_total, Dm = (int(v) for v in x.shape)
    xm = N._row_major(x)
    if rows is not None:
        if rows.dtype != torch.int64 or rows.dim() != 1:
            raise TypeError("rank_sum: rows must be int64 [n]")
        rows = rows.contiguous()
        n = int(rows.numel())
    else:
        n = int(offsets[-1])
    offsets = offsets.contiguous()
    G = int(offsets.numel()) - 1
    block = _block_of(block_cells, n, "rank_sum")
    L = _lib()
    dev = xm.device
    rank_sum2 = _buffer((G, Dm), torch.int64, dev)
    n_pos = _buffer((G, Dm), torch.int64, dev)
    tie_term = _buffer((Dm,), torch.int64, dev)
    total = _buffer((G, Dm), torch.float64, dev)
    if block is not None:
        ws_bytes = int(L.mmvae_rank_sum_blocked_workspace_bytes(n, Dm, G, block))
        ws = N._workspace(ws_bytes, dev)
        N.check(L.mmvae_rank_sum_blocked(N._ptr(xm), int(xm.stride(0)), n_total, Dm, N._ptr(rows), n, N._ptr(offsets), G, float(eps),
                                         block, N._ptr(ws), ws_bytes, N._ptr(rank_sum2), N._ptr(tie_term), N._ptr(n_pos),
                                         N._ptr(total), N._stream(dev)), "mmvae_rank_sum_blocked")
        return rank_sum2, tie_term, n_pos, total
    ws_bytes = int(L.mmvae_rank_sum_workspace_bytes(n, Dm, G))
    ws = N._workspace(ws_bytes, dev)
    N.check(L.mmvae_rank_sum(N._ptr(xm), int(xm.stride(0)), n_total, Dm, N._ptr(rows), n, N._ptr(offsets), G, float(eps), N._ptr(ws),
                             ws_bytes, N._ptr(rank_sum2), N._ptr(tie_term), N._ptr(n_pos), N._ptr(total), N._stream(dev)),
            "mmvae_rank_sum")
    return rank_sum2, tie_term, n_pos, total


def benjamini_hochberg(p: np.ndarray) -> np.ndarray:
    """Benjamini-Hochberg adjusted p-values along the last axis (``scipy.stats.false_discovery_control``'s default)."""
    p = np.asarray(p, dtype=np.float64)
    m = p.shape[-1]
    order = np.argsort(p, axis=-1)
    ps = np.take_along_axis(p, order, axis=-1) * (m / np.arange(1, m + 1))
    ps = np.minimum.accumulate(ps[..., ::-1], axis=-1)[..., ::-1]
    out = np.empty_like(ps)
    np.put_along_axis(out, order, np.clip(ps, 0.0, 1.0), axis=-1)
    return out


def z_and_p(rank_sum2: np.ndarray, tie_term: np.ndarray, n_g: np.ndarray, n: int):
    """(U, z, pval) float64 [G, D] from the exact integers: U = R - n_g (n_g + 1) / 2 with R = rank_sum2 / 2;
    z = (U - n_g (n - n_g) / 2) / sqrt(n_g (n - n_g) / 12 ((n + 1) - T / (n (n - 1)))), scipy's asymptotic statistic without the
    continuity correction; where that variance is 0 (every value tied, n_g = 0 or n_g = n) z = 0 and p = 1 (scanpy's
    choice).  p = erfc(|z| / sqrt 2), two-sided."""
    n1 = np.asarray(n_g, dtype=np.float64)[:, None]
    n2 = float(n) - n1
    U = np.asarray(rank_sum2, dtype=np.float64) / 2.0 - n1 * (n1 + 1.0) / 2.0
    T = np.asarray(tie_term, dtype=np.float64)[None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        var = n1 * n2 / 12.0 * ((n + 1.0) - (T / (float(n) * (n - 1.0)) if n > 1 else 0.0))
        ok = (var > 0.0) & (n > 1)
        z = np.where(ok, (U - n1 * n2 / 2.0) / np.sqrt(np.where(ok, var, 1.0)), 0.0)
    p = torch.special.erfc(torch.from_numpy(np.abs(z) / np.sqrt(2.0))).numpy()
    return U, z, p


def _host(a) -> np.ndarray:
    return np.asarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a)


def _float32_device(x, device) -> torch.Tensor:
    """``x`` as float32 [n_total, D] on the GPU: a float32 device tensor as it is, anything else rounded to float32 and
    uploaded.  Host input is checked for NaN (infinities rank like any value and pass)."""
    if isinstance(x, torch.Tensor) and x.dtype == torch.float32 and x.device.type == "cuda":
        if x.dim() != 2:
            raise ValueError(f"x of shape {tuple(x.shape)} is not 2-D")
        return x
    from ..cpl_mixvae import get_device          # (cpl_mixvae imports this module, inside its functions)
    h = _host(x)
    if h.ndim != 2:
        raise ValueError(f"x of shape {h.shape} is not 2-D")
    with np.errstate(over="ignore"):
        h = np.ascontiguousarray(h, dtype=np.float32)
    if np.isnan(h).any():
        raise ValueError("x holds NaN")
    return torch.from_numpy(h if h.flags.writeable else h.copy()).to(get_device(device))


def rank_sum_test(x, labels, groups=None, rows=None, eps: float = 0.0, device=None, block_cells=None) -> dict:
    """The rank-sum test of every gene (column of ``x``), each group of cells against all the others.

    ``x`` [n_total, D]: a float32 tensor on the GPU is used where it lies, with its row stride (a ``DeviceLoader``'s resident
    matrix); anything else is converted to float32 -- FLOAT64 INPUT IS ROUNDED -- and uploaded.  ``labels`` [n]: per-cell
    codes or any hashable labels.  ``groups``: the labels to test, in this order (default: ``np.unique(labels)``); cells with
    another label belong to every group's rest, and a label that no cell carries is an empty group.  ``rows``: int indices
    [n] into ``x``: ``labels[r]`` belongs to ``x[rows[r]]``; without it n must equal n_total.  ``eps``: a cell expresses a gene
    where x > eps.  At most 32768 cells and 4096 groups; with ``block_cells`` = "auto" (the blocked path above 32768 cells) or
    a block size (a power of two in [128, 32768]: the blocked path at any n) at most 1048576 cells, the same integers.

    The cells are sorted by group on the host (stable), ``mmvae_rank_sum`` returns the exact integers, and the rest is numpy
    float64: with N the number of cells, n_g the group's size and T the tie term,
      U = rank_sum2 / 2 - n_g (n_g + 1) / 2,   z = (U - n_g (N - n_g) / 2) / sqrt(n_g (N - n_g) / 12 ((N + 1) - T / (N (N - 1))))
    (no continuity correction; z = 0 and p = 1 where the variance is 0), ``pval`` = erfc(|z| / sqrt 2), ``pval_adj`` its
    Benjamini-Hochberg adjustment over the D genes of each group.  Returns a dict of numpy arrays: ``groups`` [G], ``n`` int64
    [G], ``rank_sum2`` int64 [G, D], ``tie_term`` int64 [D], ``U``, ``z``, ``pval``, ``pval_adj``, ``mean``, ``mean_rest``,
    ``frac``, ``frac_rest`` (the share of cells with x > eps) and ``logfc`` = mean - mean_rest, float64 [G, D]; the means and
    shares of an empty group (or an empty rest) are NaN."""
    if D.is_dist():
        raise NotImplementedError("rank_sum_test is not data-parallel: run it on one rank, outside the process group")
    lab = _host(labels)
    if lab.ndim != 1:
        raise ValueError(f"labels of shape {lab.shape} are not 1-D")
    n = int(lab.shape[0])
    n_total = int(x.shape[0])
    if n < 1:
        raise ValueError("rank_sum_test needs at least one cell")
    _block_of(block_cells, n, "rank_sum_test")
    if not np.isfinite(float(eps)):
        raise ValueError(f"eps = {eps} is not finite")
    rows_h = None
    if rows is not None:
        rows_h = _host(rows)
        if rows_h.ndim != 1 or rows_h.shape[0] != n or rows_h.dtype.kind not in "iu":
            raise ValueError(f"rows must be {n} integers")
        if rows_h.min() < 0 or rows_h.max() >= n_total:
            raise IndexError("row index out of range")
        rows_h = rows_h.astype(np.int64)
    elif n != n_total:
        raise ValueError(f"{n} labels for {n_total} cells (and no rows=)")
    classes, codes = np.unique(lab, return_inverse=True)
    codes = codes.reshape(-1).astype(np.int64)
    if groups is None:
        names = classes
        group_of_class = np.arange(len(classes), dtype=np.int64)
    else:
        names = np.asarray(list(groups))
        if names.ndim != 1 or len(names) < 1 or len(set(names.tolist())) != len(names):
            raise ValueError("groups must be a non-empty list of distinct labels")
        where = {v: k for k, v in enumerate(names.tolist())}
        group_of_class = np.array([where.get(c, len(names)) for c in classes.tolist()], dtype=np.int64)
    G = len(names)
    codes = group_of_class[codes]
    G_all = G + (1 if bool((codes == G).any()) else 0)               # the cells of no tested group: a last group of their own
    if G_all > MAX_GROUPS:
        raise NotImplementedError(f"rank_sum_test: {G_all} groups above {MAX_GROUPS}")
    order = np.argsort(codes, kind="stable")
    sizes = np.bincount(codes, minlength=G_all).astype(np.int64)
    offsets = np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(sizes)])
    rows_sorted = order.astype(np.int64) if rows_h is None else rows_h[order]
    xd = _float32_device(x, device)
    dev = xd.device
    r2_d, tie_d, pos_d, sum_d = rank_sums(xd, torch.from_numpy(rows_sorted).to(dev), torch.from_numpy(offsets).to(dev), eps,
                                         block_cells)
    r2, tie, pos, tot = (t.cpu().numpy() for t in (r2_d, tie_d, pos_d, sum_d))
    U, z, p = z_and_p(r2[:G], tie, sizes[:G], n)
    n1 = sizes[:G].astype(np.float64)[:, None]
    n2 = float(n) - n1
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = tot[:G] / n1
        mean_rest = (tot.sum(axis=0)[None, :] - tot[:G]) / n2
        frac = pos[:G] / n1
        frac_rest = (pos.sum(axis=0)[None, :] - pos[:G]) / n2
    return {"groups": names, "n": sizes[:G].copy(), "rank_sum2": r2[:G].copy(), "tie_term": tie, "U": U, "z": z, "pval": p,
            "pval_adj": benjamini_hochberg(p), "mean": mean, "mean_rest": mean_rest, "frac": frac, "frac_rest": frac_rest,
            "logfc": mean - mean_rest}


def marker_genes(result: dict, n_top: int = 20, gene_names=None, min_frac: float = 0.0) -> list:
    """The ``n_top`` genes of every group of a ``rank_sum_test`` result by z, descending; genes of equal z in the order of
    their index (a stable sort).  ``min_frac`` > 0 keeps only the genes that at least this share of the group's cells
    express.  Returns one dict a group: ``group``, ``genes`` (int64 indices), ``names`` (``gene_names`` at those indices, or
    None) and the genes' ``z``, ``pval``, ``pval_adj``, ``logfc``, ``mean``, ``mean_rest``, ``frac``, ``frac_rest``."""
    z = np.asarray(result["z"])
    if int(n_top) < 1:
        raise ValueError(f"n_top = {n_top} below 1")
    if gene_names is not None:
        gene_names = np.asarray(gene_names)
        if gene_names.shape != (z.shape[1],):
            raise ValueError(f"{gene_names.shape} gene names for {z.shape[1]} genes")
    out = []
    for g in range(z.shape[0]):
        order = np.argsort(-z[g], kind="stable")
        if min_frac > 0.0:
            order = order[np.asarray(result["frac"])[g][order] >= min_frac]
        top = order[:int(n_top)].astype(np.int64)
        entry = {"group": result["groups"][g], "genes": top, "names": None if gene_names is None else gene_names[top]}
        for k in ("z", "pval", "pval_adj", "logfc", "mean", "mean_rest", "frac", "frac_rest"):
            entry[k] = np.asarray(result[k])[g][top]
        out.append(entry)
    return out

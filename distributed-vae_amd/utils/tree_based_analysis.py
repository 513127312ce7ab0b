"""The continuous-variable analysis of the reference's ``mmidas/utils/tree_based_analysis.py``: ``corr_analysis``, on the
device, without scipy.

The reference takes, for every state dimension and every gene, ``scipy.stats.pearsonr`` of the state with the gene's expression
over the cells that express the gene (``cell[:, g] > 0``, more than four of them) -- S x D calls, each with a boolean mask over
all cells, and once more per category -- and returns the genes ordered by |r|.  Here ``mmvae_state_corr``
(csrc/statecorr.hip) makes one pass over the float32 matrix where it lies, for every group of cells at
once, with fp64 moments; the signed r comes back as float64 and the ordering is numpy's, on the host.  ``get_merged_types``
of that module (pandas tree handling) is not part of this package."""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from .. import _native as N
from .. import dist as D
from .._utils import float32_on_device


def grouped_state_corr(state: torch.Tensor, data: torch.Tensor, rows: Optional[torch.Tensor], codes: Optional[torch.Tensor],
                       n_groups: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(r float64 [G, S, D], count int64 [G, D]) on the device, of device tensors: ``state`` float32 [n, S], ``data`` float32
    [n_total, D], ``rows`` int64 [n] or None (the rows 0..n-1), ``codes`` int64 [n] in [0, n_groups) or None (one group).  The
    cells are stable-sorted by code on the device (torch plumbing: a sort, a bincount, two gathers of n-row arrays), so that
    within a group they keep their order; nothing is read on the host."""
    if codes is None:
        return N.state_corr(data, state, rows)
    order = torch.sort(codes, stable=True).indices
    sizes = torch.bincount(codes, minlength=n_groups)[:n_groups]
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64, device=codes.device), torch.cumsum(sizes, 0)])
    return N.state_corr(data, state.index_select(0, order), order if rows is None else rows.index_select(0, order), offsets)


def _ordered(r: np.ndarray):
    """The reference's two returns for one group's r [S, D]: (all_corr, all_geneID), NaN last as numpy places it."""
    return [np.sort(np.abs(v)) for v in r], [np.argsort(np.abs(v)) for v in r]


def corr_analysis(state, cell, groups=None, rows=None, return_r: bool = False, device=None):
    """The reference's ``corr_analysis(state, cell)`` (tree_based_analysis.py:7-59): ``(all_corr, all_geneID)``, two lists of
    S arrays, ``all_corr[s] = np.sort(np.abs(r_s))`` (float64) and ``all_geneID[s] = np.argsort(np.abs(r_s))``, where
    ``r_s[g]`` is the Pearson correlation of ``state[:, s]`` with ``cell[:, g]`` over the cells with ``cell[:, g] > 0``:
    exactly 0 where at most four cells express the gene, NaN where the expression or the state is constant over them (scipy's
    constant-input result, which the reference stores; numpy sorts NaN last).

    ``state`` [n, S] and ``cell`` [n_total, D]: a float32 tensor on the GPU is used where it lies, with its row stride (the
    resident matrix of a ``DeviceLoader``, the ``s_mean`` of an encode); anything else is converted to float32 -- FLOAT64
    INPUT IS ROUNDED -- and uploaded.  Inputs must be finite: host arrays are checked (ValueError), device tensors are not.
    r is computed from fp64 raw moments in one pass: within 8 (c + 1) kappa 2^-53 of the exact value on the float32 inputs,
    c the number of expressing cells and kappa = max(1 + mean^2 / var) of the two variables over them.

    Extensions.  ``groups``: labels [n] of any dtype, encoded by ``np.unique``: every group in one device pass -- the
    reference's "S conditioning on Z = k" -- and both returns become lists over the groups (in ``np.unique`` order) of the
    lists above.  ``rows``: int row indices [n] into ``cell`` (a loader's index): ``state[r]`` belongs to ``cell[rows[r]]``;
    without it n must equal n_total.  ``return_r=True``: returns ``(all_corr, all_geneID, r, counts)`` with the signed r
    float64 [G, S, D] and the counts int64 [G, D] (G = 1 without ``groups``)."""
    if D.is_dist():
        raise NotImplementedError("corr_analysis is not data-parallel: run it on one rank, outside the process group")
    n = int(state.shape[0])
    n_total = int(cell.shape[0])
    codes_h, n_groups = None, 1
    if groups is not None:
        g = np.asarray(groups.detach().cpu().numpy() if isinstance(groups, torch.Tensor) else groups)
        if g.ndim != 1 or g.shape[0] != n:
            raise ValueError(f"groups of shape {g.shape} for {n} cells")
        classes, codes_h = np.unique(g, return_inverse=True)
        codes_h, n_groups = codes_h.reshape(-1).astype(np.int64), len(classes)
    rows_h = None
    if rows is not None:
        rows_h = np.asarray(rows.detach().cpu().numpy() if isinstance(rows, torch.Tensor) else rows)
        if rows_h.ndim != 1 or rows_h.shape[0] != n or rows_h.dtype.kind not in "iu":
            raise ValueError(f"rows must be {n} integers")
        if n and (rows_h.min() < 0 or rows_h.max() >= n_total):
            raise IndexError("row index out of range")
        rows_h = rows_h.astype(np.int64)
    elif n != n_total:
        raise ValueError(f"{n} states for {n_total} cells (and no rows=)")
    if n < 1:
        raise ValueError("corr_analysis needs at least one cell")
    on_gpu = [t.device for t in (cell, state) if isinstance(t, torch.Tensor) and t.device.type == "cuda"]
    dev = on_gpu[0] if on_gpu and device is None else device
    data_d = float32_on_device(cell, dev, "cell", "2-D")
    state_d = float32_on_device(state, data_d.device, "state", "2-D")
    to_dev = lambda a: None if a is None else torch.from_numpy(a).to(data_d.device)
    r_d, c_d = grouped_state_corr(state_d, data_d, to_dev(rows_h), to_dev(codes_h), n_groups)
    r, counts = r_d.cpu().numpy(), c_d.cpu().numpy()
    if groups is None:
        all_corr, all_gene = _ordered(r[0])
    else:
        per_group = [_ordered(rg) for rg in r]
        all_corr, all_gene = [p[0] for p in per_group], [p[1] for p in per_group]
    return (all_corr, all_gene, r, counts) if return_r else (all_corr, all_gene)

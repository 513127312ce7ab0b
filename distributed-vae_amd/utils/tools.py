"""Data preparation on the device: the numeric functions of the reference's ``mmidas/utils/tools.py``.

``normalize_cellxgene`` (sklearn's ``normalize(x, axis=1, norm="l1")``), ``logcpm`` (``np.log1p`` of that times ``scaler``)
and ``reorder_genes`` (the genes ranked by the spread of the binarised expression) keep the reference's positional
signatures; everything else is keyword-only.  The reference makes three full-size float64 copies of the count matrix on the
host, of which the data-prep notebooks keep a selection of columns and rows and cast it to float32.  Here the counts, dense
or CSR, go to the device once; ``mmvae_cpm_dense`` / ``mmvae_cpm_csr`` (csrc/dataprep.hip) read only
the selected rows and write only the selected columns, in the reference's arithmetic (the row norm over ALL genes; every
step one IEEE double operation), and ``logcpm(counts, genes=..., cells=..., out="torch", dtype=torch.float32)`` is the tensor
``get_loaders`` takes as it is.  ``gene_stats`` (new) is the per-gene count above a threshold with the fp64 mean and
standard deviation -- what the reference's ``reorder_genes`` computes and drops (``g_std``).

Departures, all stated in the functions' docstrings: ``reorder_genes`` breaks ties between genes of equal spread by gene
index (the reference's order inside such a group is rounding noise of ``np.std``), ignores ``chunksize`` and does not
print.  Not mirrored: ``get_paths`` and ``parse_toml`` (they need ``toml``) and ``download_file`` (a network fetch).
scipy is optional: a CSR matrix is any object with ``indptr``, ``indices``, ``data``, ``shape``, or a tuple of those four."""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from .. import _native as N
from .. import dist as D
from ..cpl_mixvae import get_device

MAX_GENES = N.CPM_MAX_G


def _refuse_dist(what: str):
    if D.is_dist():
        raise NotImplementedError(f"{what} is not data-parallel: run it on one rank, outside the process group")


def _is_csr(x) -> bool:
    if isinstance(x, (np.ndarray, torch.Tensor)):
        return False
    if isinstance(x, tuple) and len(x) == 4:
        return True
    return all(hasattr(x, a) for a in ("indptr", "indices", "data", "shape"))


def _value_tensor(a, what: str) -> torch.Tensor:
    """The values of a matrix (dense or the data of a CSR one) as an int32, float32 or float64 tensor where they lie: other
    integer widths range-checked and cast to int32, half types cast to float32."""
    if isinstance(a, torch.Tensor):
        t = a.detach()
    else:
        a = np.asarray(a)
        if a.dtype.kind not in "biuf":
            raise TypeError(f"{what}: values of dtype {a.dtype} are not counts or floats")
        t = torch.from_numpy(a if all(s >= 0 for s in a.strides) and a.flags.writeable else np.ascontiguousarray(a).copy())
    if t.dtype in (torch.int32, torch.float32, torch.float64):
        return t
    if t.dtype in (torch.float16, torch.bfloat16):
        return t.to(torch.float32)
    if t.dtype == torch.bool:
        return t.to(torch.int32)
    if t.dtype.is_floating_point or t.dtype.is_complex:
        raise TypeError(f"{what}: values of dtype {t.dtype} are not counts or floats")
    if t.numel() and (int(t.min()) < -2 ** 31 or int(t.max()) > 2 ** 31 - 1):
        raise ValueError(f"{what}: integer values outside the int32 range")
    return t.to(torch.int32)


def _numpy_values(a):
    """numpy has unsigned widths torch lacks: bring them to int64 first."""
    if isinstance(a, np.ndarray) and a.dtype.kind == "u" and a.dtype.itemsize > 1:
        if a.size and int(a.max()) > 2 ** 31 - 1:
            raise ValueError("integer values outside the int32 range")
        return a.astype(np.int64)
    return a


def _index_array(idx, size: int, what: str, allow_mask: bool) -> np.ndarray:
    a = idx.detach().cpu().numpy() if isinstance(idx, torch.Tensor) else np.asarray(idx)
    if allow_mask and a.dtype == np.bool_:
        if a.shape != (size,):
            raise ValueError(f"{what}: a mask of shape {a.shape} on {size} entries")
        a = np.flatnonzero(a)
    if a.ndim != 1 or a.dtype.kind not in "iu":
        raise ValueError(f"{what}: an index array must be one-dimensional and integer (got shape {a.shape}, dtype {a.dtype})")
    if a.size == 0:
        raise ValueError(f"{what}: empty selection")
    a = a.astype(np.int64)
    if int(a.min()) < 0 or int(a.max()) >= size:
        raise ValueError(f"{what}: index outside [0, {size})")
    return a


def _check_canonical(indptr: torch.Tensor, indices: torch.Tensor, shape):
    """ValueError unless indptr runs from 0 to nnz without decreasing and every row's indices strictly increase inside
    [0, G) (torch operations where the arrays lie: on the host for host input)."""
    n, G = shape
    nnz = int(indices.numel())
    if int(indptr[0]) != 0 or int(indptr[-1]) != nnz or (n > 0 and bool((indptr[1:] < indptr[:-1]).any())):
        raise ValueError("CSR matrix: indptr must run from 0 to nnz without decreasing")
    if nnz == 0:
        return
    if int(indices.min()) < 0 or int(indices.max()) >= G:
        raise ValueError(f"CSR matrix: column index outside [0, {G})")
    if nnz > 1:
        bad = indices[1:] <= indices[:-1]                           # allowed only where a new row starts
        starts = indptr[1:-1]
        starts = starts[(starts > 0) & (starts < nnz)]
        bad[starts - 1] = False
        if bool(bad.any()):
            raise ValueError("CSR matrix is not canonical (indices must strictly increase in every row): call "
                             "sum_duplicates() (and sort_indices()) first")


class _Matrix:
    """The input of one call, checked on the host: ``kind`` "dense" (``x``) or "csr" (``indptr``, ``indices``, ``data``)."""

    def __init__(self, x, what: str):
        self.what = what
        if _is_csr(x):
            if not isinstance(x, tuple) and getattr(x, "format", "csr") != "csr":
                raise TypeError(f"{what}: a sparse matrix must be CSR (got format {x.format!r}): call .tocsr()")
            indptr, indices, data, shape = x if isinstance(x, tuple) else (x.indptr, x.indices, x.data, x.shape)
            if len(shape) != 2:
                raise ValueError(f"{what}: x of shape {tuple(shape)} is not [cells, genes]")
            self.kind, self.shape = "csr", (int(shape[0]), int(shape[1]))
            self.indptr = torch.as_tensor(indptr).to(torch.int64).reshape(-1)
            indices = torch.as_tensor(indices).reshape(-1)
            self.data = _value_tensor(_numpy_values(data), what).reshape(-1)
            on = [t.device for t in (self.indptr, indices, self.data) if t.device.type == "cuda"]
            if on:                                                        # arrays partly on the device: all of them there
                self.indptr, indices, self.data = self.indptr.to(on[0]), indices.to(on[0]), self.data.to(on[0])
            if self.indptr.numel() != self.shape[0] + 1 or indices.numel() != self.data.numel():
                raise ValueError(f"{what}: CSR arrays do not fit the shape {self.shape}")
            if self.shape[0] >= 1 and self.shape[1] >= 1:
                _check_canonical(self.indptr, indices, self.shape)
            self.indices = indices.to(torch.int32)
            self.device = self.data.device if self.data.device.type == "cuda" else None
        else:
            h = _numpy_values(x) if isinstance(x, (np.ndarray, torch.Tensor)) else np.asarray(x)
            if h.ndim != 2:
                raise ValueError(f"{what}: x of shape {tuple(h.shape)} is not [cells, genes]")
            self.kind, self.shape = "dense", (int(h.shape[0]), int(h.shape[1]))
            self.x = _value_tensor(h, what) if self.shape[0] and self.shape[1] else None
            self.device = self.x.device if self.x is not None and self.x.device.type == "cuda" else None
        if self.shape[0] < 1:
            raise ValueError(f"{what}: x has no rows")
        if self.shape[1] < 1:
            raise ValueError(f"{what}: x has no columns")
        if self.shape[1] > MAX_GENES:
            raise NotImplementedError(f"{what}: {self.shape[1]} genes above {MAX_GENES}")
        self.value_dtype = (self.x if self.kind == "dense" else self.data).dtype

    def to(self, device):
        dev = self.device if self.device is not None else get_device(device)
        if dev.type != "cuda":
            raise N.NativeError(f"{self.what} needs a GPU (no CPU fallback)")
        for name in ("x", "indptr", "indices", "data"):
            if getattr(self, name, None) is not None:
                setattr(self, name, getattr(self, name).to(dev))
        self.device = dev
        return dev


_OUT_DTYPES = {torch.float32: torch.float32, torch.float64: torch.float64, "float32": torch.float32, "float64": torch.float64}


def _out_dtype(dtype, value_dtype) -> torch.dtype:
    if dtype is None:
        return torch.float32 if value_dtype == torch.float32 else torch.float64
    if dtype in _OUT_DTYPES:
        return _OUT_DTYPES[dtype]
    try:
        return _OUT_DTYPES[np.dtype(dtype).name]
    except (TypeError, KeyError):
        raise ValueError(f"dtype = {dtype!r}: float32 or float64") from None


def _cpm(what, x, scaler, log, genes, cells, out, dtype, return_norms, device):
    _refuse_dist(what)
    if out not in ("numpy", "torch"):
        raise ValueError(f"out = {out!r}: one of 'numpy', 'torch'")
    scaler = float(scaler)
    if not np.isfinite(scaler):
        raise ValueError(f"scaler = {scaler} is not finite")
    m = _Matrix(x, what)
    n_total, G = m.shape
    odt = _out_dtype(dtype, m.value_dtype)
    g = c = None
    if genes is not None:
        g = _index_array(genes, G, f"{what}: genes", allow_mask=False)
        if np.unique(g).size != g.size:
            raise ValueError(f"{what}: genes holds duplicates")
    if cells is not None:
        c = _index_array(cells, n_total, f"{what}: cells", allow_mask=True)
    dev = m.to(device)                                                # ---- every refusal that needs no device is behind us
    rows = None if c is None else torch.from_numpy(c).to(dev)
    if m.kind == "dense":
        gl = None if g is None else torch.from_numpy(g.astype(np.int32)).to(dev)
        res, norms = N.cpm_dense(m.x, rows, gl, scaler, log, odt)
    else:
        inv = np.full(G, -1, dtype=np.int32)
        sel = np.arange(G) if g is None else g
        inv[sel] = np.arange(sel.size, dtype=np.int32)
        res, norms = N.cpm_csr(m.indptr, m.indices, m.data, m.shape, torch.from_numpy(inv).to(dev), int(sel.size), rows, scaler, log,
                               odt)
    if m.value_dtype != torch.int32 and not bool(torch.isfinite(norms).all()):
        raise ValueError(f"{what}: input contains NaN or infinity")
    if out == "numpy":
        res, norms = res.cpu().numpy(), norms.cpu().numpy()
    return (res, norms) if return_norms else res


def normalize_cellxgene(x, *, genes=None, cells=None, out="numpy", dtype=None, return_norms=False, device=None):
    """The reference's ``normalize_cellxgene``: every row of the cell x gene matrix divided by its sum of magnitudes (rows
    that sum to 0 stay 0), as sklearn's ``normalize(x, axis=1, norm="l1")``.  See ``logcpm`` for the arguments."""
    return _cpm("normalize_cellxgene", x, 1.0, False, genes, cells, out, dtype, return_norms, device)


def logcpm(x, scaler=1e6, *, genes=None, cells=None, out="numpy", dtype=None, return_norms=False, device=None):
    """The reference's ``logcpm``: ``np.log1p(normalize_cellxgene(x) * scaler)``, on the device.

    ``x``: a dense numpy array or torch tensor, host or device, of an integer type (int32 as it is; other widths are
    range-checked and cast to int32), float32 or float64 (half types are cast to float32), a row-strided device view read in
    place; or a canonical CSR matrix -- a ``scipy.sparse.csr_matrix``, any object with ``indptr``, ``indices``, ``data``,
    ``shape``, or a tuple of those four (ValueError, naming ``sum_duplicates()``, if a row's indices do not strictly
    increase).  The row norm is the sum of |x| over ALL genes of the row whatever ``genes`` selects, 1 where it is 0; each
    value is x / norm, times ``scaler``, then log1p, each one IEEE double operation; an exact zero gives an exact zero.

    ``genes``: unique column indices in any order (ValueError on duplicates or out-of-range entries); ``cells``: row indices
    in any order, or a boolean mask.  Only the selected rows are read and only the selected columns are written; the result is
    [len(cells), len(genes)].  ``out="numpy"`` or ``"torch"`` (the contiguous device tensor).  ``dtype`` float32 or float64;
    None: what the reference returns (float64 for integer and float64 input, float32 for float32 input); a float32 result is
    the fp64 value rounded once.  ``return_norms``: also the float64 sums of |x| of the selected rows (0 for a zero row).

    ValueError for input that is not 2-D, has no rows, or holds NaN or infinity (seen in the norms: no extra pass);
    NotImplementedError under a process group and for more than 2^20 genes."""
    return _cpm("logcpm", x, scaler, True, genes, cells, out, dtype, return_norms, device)


def _gene_stats(what: str, x, eps, rows, device) -> Tuple[dict, int]:
    _refuse_dist(what)
    if _is_csr(x):
        raise TypeError(f"{what}: a dense matrix is needed (the output of logcpm, not the sparse counts)")
    eps = float(eps)
    if np.isnan(eps):
        raise ValueError(f"{what}: eps is NaN")
    m = _Matrix(x, what)
    r = None if rows is None else _index_array(rows, m.shape[0], f"{what}: rows", allow_mask=True)
    dev = m.to(device)                                                # ---- every refusal that needs no device is behind us
    xd = m.x.to(torch.float64) if m.x.dtype == torch.int32 else m.x
    k, mean, sd = N.gene_stats(xd, eps, None if r is None else torch.from_numpy(r).to(dev))
    out = {"n_above": k.cpu().numpy(), "mean": mean.cpu().numpy(), "std": sd.cpu().numpy()}
    if not (np.isfinite(out["mean"]).all() and np.isfinite(out["std"]).all()):
        raise ValueError(f"{what}: input contains NaN or infinity")
    return out, (m.shape[0] if r is None else int(r.size))


def gene_stats(x, eps=1e-1, *, rows=None, device=None) -> dict:
    """Per gene of the dense cell x gene matrix ``x`` (float32 or float64; integers are cast to float64), over the rows
    ``rows`` (indices or a mask; None: all): ``{"n_above": int64 [D], "mean": float64 [D], "std": float64 [D]}`` as numpy
    arrays -- the exact number of cells with x > eps (compared in the matrix's own dtype with eps rounded to it, as numpy
    compares a float32 array with a Python float), the mean and the population standard deviation (``np.std``) from fp64
    moments about the first selected row (``mmvae_gene_stats``).  ValueError for non-finite data; NotImplementedError
    under a process group."""
    return _gene_stats("gene_stats", x, eps, rows, device)[0]


def order_from_counts(n_above, n: int, eps: float = 1e-1) -> np.ndarray:
    """The gene order of ``reorder_genes`` from k_g = the number of the ``n`` cells with x > eps: the binarised gene has the
    population std sqrt(k (n - k)) / n; the genes whose std exceeds ``eps``, by decreasing exact integer key k (n - k), equal
    keys by increasing gene index."""
    k = np.asarray(n_above, dtype=np.int64)
    key = k * (np.int64(n) - k)
    std = np.sqrt(key.astype(np.float64)) / float(n)
    kept = np.flatnonzero(std > eps)
    return kept[np.lexsort((kept, -key[kept]))]


def reorder_genes(x, chunksize=1000, eps=1e-1, *, rows=None, return_counts=False, device=None):
    """The reference's ``reorder_genes``: the genes of the dense matrix ``x`` whose binarised expression (x > eps) has a
    population std above ``eps``, most spread first, as an int64 numpy array.  The device counts k_g exactly
    (``gene_stats``); the host forms the exact key k (n - k) and the closed-form std.  DEPARTURE: genes of equal k (n - k) are
    returned by increasing index, where the reference's order is decided by rounding noise of ``np.std``; the kept set and the
    sequence of keys are the reference's.  ``chunksize`` is accepted and ignored; nothing is printed.  ``rows``: the cells to
    count over (indices or a mask); ``return_counts``: also k_g."""
    stats, n = _gene_stats("reorder_genes", x, eps, rows, device)
    order = order_from_counts(stats["n_above"], n, eps)
    return (order, stats["n_above"]) if return_counts else order

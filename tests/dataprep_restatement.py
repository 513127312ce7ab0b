"""Plain-numpy restatement of the reference's data preparation (mmidas/utils/tools.py: normalize_cellxgene, logcpm,
reorder_genes) and of the per-gene statistics, without sklearn or scipy: what tests/test_dataprep_cpu.py holds to the
reference's recorded returns (tests/golden/dataprep_kat.npz) and tests/test_gpu_dataprep.py holds the device to.

The arithmetic of ``cpm``: norm = sum |x| over all genes of the row (an integer row in int64, exactly; a float row in fp64),
1 where that is 0; value = x / norm, times scaler, then log1p -- each one IEEE double operation on float64 arrays."""
import numpy as np


def row_sums(x):
    """float64 [n]: sum |x| over every row of the dense matrix; integer input summed exactly in int64."""
    x = np.asarray(x)
    if x.dtype.kind in "iub":
        return np.abs(x.astype(np.int64)).sum(axis=1).astype(np.float64)
    return np.abs(x.astype(np.float64)).sum(axis=1)


def select(idx, size):
    """An index array from None (all), a boolean mask or indices."""
    if idx is None:
        return np.arange(size)
    a = np.asarray(idx)
    return np.flatnonzero(a) if a.dtype == np.bool_ else a.astype(np.int64)


def cpm(x, scaler=1.0, log=False, genes=None, cells=None):
    """(out float64 [len(cells), len(genes)], sums float64 [len(cells)]): the selected rows and columns of
    x / norm * scaler, or log1p of that, the norm over ALL genes."""
    x = np.asarray(x)
    r, g = select(cells, x.shape[0]), select(genes, x.shape[1])
    sums = row_sums(x[r])
    norm = np.where(sums == 0.0, 1.0, sums)
    arg = x[np.ix_(r, g)].astype(np.float64) / norm[:, None]
    arg = arg * np.float64(scaler)
    return (np.log1p(arg) if log else arg), sums


def normalize_cellxgene(x, **kw):
    return cpm(x, 1.0, False, **kw)[0]


def logcpm(x, scaler=1e6, **kw):
    return cpm(x, scaler, True, **kw)[0]


def to_csr(x):
    """(indptr int64, indices int32, data, shape) of the dense matrix: canonical CSR, without scipy."""
    x = np.asarray(x)
    nz = x != 0
    indptr = np.concatenate([[0], np.cumsum(nz.sum(axis=1))]).astype(np.int64)
    indices = np.nonzero(nz)[1].astype(np.int32)
    return indptr, indices, x[nz], x.shape


def counts_above(x, eps=1e-1, rows=None):
    """int64 [D]: the number of (selected) rows with x > eps, compared as numpy compares the array with a Python float:
    in the array's own dtype."""
    x = np.asarray(x)
    x = x[select(rows, x.shape[0])]
    return (x > (x.dtype.type(eps) if x.dtype.kind == "f" else eps)).sum(axis=0).astype(np.int64)


def keys(k, n):
    """The exact integer key k (n - k) of a gene with k of n cells above the threshold: its binarised population variance
    times n^2."""
    k = np.asarray(k, dtype=np.int64)
    return k * (np.int64(n) - k)


def reorder_genes(x, eps=1e-1, rows=None):
    """(order int64, k int64 [D]): the genes whose closed-form binarised std sqrt(k (n - k)) / n exceeds eps, by decreasing
    key, equal keys by increasing gene index."""
    k = counts_above(x, eps, rows)
    n = len(select(rows, np.asarray(x).shape[0]))
    key = keys(k, n)
    std = np.sqrt(key.astype(np.float64)) / float(n)
    kept = np.flatnonzero(std > eps)
    return kept[np.lexsort((kept, -key[kept]))], k


def gene_stats(x, eps=1e-1, rows=None):
    """{"n_above", "mean", "std", "kappa"}: the two-pass mean and population std of every gene in extended precision
    (np.longdouble), rounded to float64, and kappa = 1 + (mean - pivot)^2 / var for the pivot the device uses (the first
    selected row; 1 where var is 0: every deviation from the pivot is then exactly 0)."""
    x = np.asarray(x)
    r = select(rows, x.shape[0])
    xs = x[r].astype(np.longdouble)
    mean = xs.mean(axis=0)
    var = ((xs - mean) ** 2).mean(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        kappa = np.where(var > 0, 1.0 + (mean - xs[0]) ** 2 / var, 1.0).astype(np.float64)
    return {"n_above": counts_above(x, eps, rows), "mean": mean.astype(np.float64), "std": np.sqrt(var).astype(np.float64),
            "kappa": kappa}


def ulps(a, b):
    """|a - b| in units of b's float spacing, elementwise (arrays of one float dtype)."""
    a, b = np.asarray(a), np.asarray(b)
    with np.errstate(invalid="ignore"):
        return np.abs(a.astype(np.longdouble) - b.astype(np.longdouble)) / np.spacing(np.abs(b)).astype(np.longdouble)

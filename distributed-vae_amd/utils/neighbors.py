"""The k-nearest-neighbour graph of the cells in latent space, neighbourhood purity and the k-NN classifier, on the device,
without sklearn or scipy: ``knn``, ``knn_graph``, ``neighbor_purity``, ``knn_cv_predict`` and ``KNN_classifier`` (and under
them ``knn_device`` / ``knn_votes_device`` on device tensors, ``csr_from_neighbors`` and ``to_scipy``).

``sklearn.neighbors.NearestNeighbors`` / ``KNeighborsClassifier`` and scanpy's ``pp.neighbors`` find the neighbours on the
host; a torch composition (``cdist`` + ``topk``) materialises n x n floats.  Here ``mmvae_knn`` (csrc/knn.hip; DESIGN.md section
9t) forms every squared distance in fp32 in difference form and keeps, per query, the k smallest admitted candidates under the
total order (bits of the squared distance, then index): the same bits on every run, however the work is cut.  One admission
rule -- reference j is admitted for query i iff no groups are given or ``ref_groups[j] != groups[i]`` -- gives the plain query,
the graph without the cell itself (groups = arange) and the cross-validated classifier (groups = each cell's fold).  The
square root is taken by torch on the kernel's squared distances and is the correctly rounded float32 one, so the order stays.
``mmvae_knn_votes`` counts the neighbours' labels: the prediction (ties to the smallest label, sklearn's rule) and the purity,
the share of a cell's neighbours that carry its own label.

At most ``MAX_N`` = 1048576 points a side, ``MAX_K`` = 64 neighbours, ``MAX_D`` = 128 coordinates and ``MAX_CLASSES`` = 4096
labels.  NaN is refused in host input and not checked for in a device tensor (a point that holds one gets unspecified
neighbours).  Not offered: approximate neighbours, metrics other than Euclidean, distance-weighted votes, data-parallel use,
UMAP and Leiden themselves (the CSR graph is the hand-over)."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from .. import _native as N
from .. import dist as D

MAX_K = 64             # MMVAE_KNN_MAX_K (include/mmvae.h)
MAX_D = 128            # KNN_MAX_D (csrc/common.hpp)
MAX_N = 1 << 20        # MMVAE_KNN_MAX_N
MAX_CLASSES = 4096     # KNN_MAX_CLASSES

_ITEM = {torch.int32: 4, torch.float32: 4, torch.float64: 8}      # bytes of an element of the buffers handed out below

_bound = [False]


def _lib():
    """The library with the k-NN entries' signatures declared (here, as marker_analysis.py declares its own)."""
    L = N.lib()
    if not _bound[0]:
        vp, i64, i32 = C.c_void_p, C.c_int64, C.c_int
        L.mmvae_knn_workspace_bytes.argtypes = [i64, i64, i32, i32]
        L.mmvae_knn_workspace_bytes.restype = C.c_size_t
        L.mmvae_knn.argtypes = [vp, i64, i64, vp, i64, i64, i32, i32, vp, vp, vp, C.c_size_t, vp, vp, vp]
        L.mmvae_debug_knn.argtypes = [vp, i64, i64, vp, i64, i64, i32, i32, vp, vp, vp, C.c_size_t, vp, vp, i64, i32, vp]
        L.mmvae_knn_votes.argtypes = [vp, i64, i32, vp, i64, i32, vp, vp, vp, vp, vp]
        _bound[0] = True
    return L


def workspace_bytes(nq: int, nr: int, d: int, k: int) -> int:
    """``mmvae_knn_workspace_bytes``: host only; 0 for a shape that ``mmvae_knn`` refuses."""
    return int(_lib().mmvae_knn_workspace_bytes(int(nq), int(nr), int(d), int(k)))


def _refuse_dist(who: str):
    if D.is_dist():
        raise NotImplementedError(f"{who} is not data-parallel: run it on one rank, outside the process group")


def _check_shape(who: str, nq: int, nr: int, d: int, k) -> int:
    """The refusals of a shape, before any device work -> k as an int."""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
        raise ValueError(f"{who}: k = {k!r} is not an int")
    k = int(k)
    if k < 1:
        raise ValueError(f"{who}: k = {k} below 1")
    if k > MAX_K:
        raise NotImplementedError(f"{who}: k = {k} above {MAX_K}")
    if d < 1:
        raise ValueError(f"{who}: d = {d} below 1")
    if d > MAX_D:
        raise NotImplementedError(f"{who}: d = {d} above {MAX_D}")
    if nq < 1 or nr < 1:
        raise ValueError(f"{who}: {nq} queries against {nr} reference points: at least one of each")
    if nq > MAX_N or nr > MAX_N:
        raise NotImplementedError(f"{who}: n = {max(nq, nr)} above {MAX_N}")
    return k


def _shape2(who: str, name: str, x):
    shape = tuple(x.shape) if hasattr(x, "shape") else np.asarray(x).shape
    if len(shape) != 2:
        raise ValueError(f"{who}: {name} of shape {shape} is not [n, d]")
    return int(shape[0]), int(shape[1])


def _buffer(shape, dtype, device) -> torch.Tensor:
    """An uninitialised device buffer: a view of a ``_native._workspace``, so that it is guarded with it."""
    numel = int(np.prod(shape))
    nbytes = numel * _ITEM[dtype]
    return N._workspace(nbytes + 7, device).view(torch.uint8)[:nbytes].view(dtype).view(*shape)


def knn_device(q: torch.Tensor, r: torch.Tensor, k: int, qgroup: Optional[torch.Tensor] = None,
               rgroup: Optional[torch.Tensor] = None, seg_cols: Optional[int] = None, phases: int = 0, ws=None):
    """mmvae_knn on device tensors: float32 ``q`` [nq, d] and ``r`` [nr, d] (rows may be strided, columns not; read where
    they lie), optional int32 ``qgroup`` [nq] and ``rgroup`` [nr] (both or neither) -> (idx int32 [nq, k], dist2 float32
    [nq, k]) on the device: the k admitted references of every query with the smallest (squared-distance bits, index), the
    tail idx = -1, dist2 = +inf where fewer are admitted.  ``seg_cols``: mmvae_debug_knn with segments of that many reference
    columns (0: the entry's choice) -- the same bits; ``phases`` and ``ws`` (a workspace kept between calls) are its timing
    split (tools/time_knn.py)."""
    if (qgroup is None) != (rgroup is None):
        raise ValueError("knn: one group array without the other")
    N._need_cuda("knn", q, r, qgroup, rgroup)
    if q.dtype != torch.float32 or r.dtype != torch.float32 or q.dim() != 2 or r.dim() != 2:
        raise TypeError("knn: q and r must be float32 [n, d]")
    if int(q.shape[1]) != int(r.shape[1]):
        raise ValueError(f"knn: queries of {int(q.shape[1])} coordinates against references of {int(r.shape[1])}")
    nq, d = (int(v) for v in q.shape)
    nr = int(r.shape[0])
    k = _check_shape("knn", nq, nr, d, k)
    for g, n, name in ((qgroup, nq, "qgroup"), (rgroup, nr, "rgroup")):
        if g is not None and (g.dtype != torch.int32 or g.dim() != 1 or int(g.numel()) != n):
            raise TypeError(f"knn: {name} must be int32 [{n}]")
    qm, rm = N._row_major(q), N._row_major(r)
    if qgroup is not None:
        qgroup, rgroup = qgroup.contiguous(), rgroup.contiguous()
    L = _lib()
    dev = qm.device
    idx = _buffer((nq, k), torch.int32, dev)
    dist2 = _buffer((nq, k), torch.float32, dev)
    if seg_cols is None:
        ws_bytes = int(L.mmvae_knn_workspace_bytes(nq, nr, d, k))
    else:
        seg = int(seg_cols) if int(seg_cols) > 0 else None
        nseg = -(-nr // seg) if seg else 0
        ws_bytes = 8 * nseg * nq * k if nseg > 1 else max(int(L.mmvae_knn_workspace_bytes(nq, nr, d, k)), 8)
        if ws_bytes > (2 << 30):
            raise NotImplementedError(f"knn: segments of {seg} columns need a workspace above 2 GiB")
    if ws is None:
        ws = N._workspace(ws_bytes, dev)
    args = (N._ptr(qm), int(qm.stride(0)), nq, N._ptr(rm), int(rm.stride(0)), nr, d, k, N._ptr(qgroup), N._ptr(rgroup), N._ptr(ws),
            int(ws.numel()) * 8, N._ptr(idx), N._ptr(dist2))
    if seg_cols is None:
        N.check(L.mmvae_knn(*args, N._stream(dev)), "mmvae_knn")
    else:
        N.check(L.mmvae_debug_knn(*args, int(seg_cols), int(phases), N._stream(dev)), "mmvae_debug_knn")
    return idx, dist2


def knn_votes_device(idx: torch.Tensor, rlabel: torch.Tensor, n_classes: int, qlabel: Optional[torch.Tensor] = None,
                     top2: bool = False):
    """mmvae_knn_votes on device tensors: ``idx`` int32 [nq, k] (``knn_device``'s), ``rlabel`` int32 [nr] in
    [0, n_classes), optional ``qlabel`` int32 [nq] -> (pred int32 [nq], purity float64 [nq] or None, top2 int32 [nq, 2] or
    None): the label most valid neighbours carry (ties to the smallest, -1 without a neighbour), the share of the valid
    neighbours labelled ``qlabel[i]`` (NaN without one), and the votes of ``pred`` and of the runner-up."""
    N._need_cuda("knn_votes", idx, rlabel, qlabel)
    if idx.dtype != torch.int32 or idx.dim() != 2 or rlabel.dtype != torch.int32 or rlabel.dim() != 1:
        raise TypeError("knn_votes: idx must be int32 [nq, k] and rlabel int32 [nr]")
    nq, k = (int(v) for v in idx.shape)
    if qlabel is not None and (qlabel.dtype != torch.int32 or qlabel.dim() != 1 or int(qlabel.numel()) != nq):
        raise TypeError(f"knn_votes: qlabel must be int32 [{nq}]")
    if not 1 <= int(n_classes) <= MAX_CLASSES:
        raise NotImplementedError(f"knn_votes: {n_classes} classes outside [1, {MAX_CLASSES}]")
    idx, rlabel = idx.contiguous(), rlabel.contiguous()
    dev = idx.device
    pred = _buffer((nq,), torch.int32, dev)
    purity = _buffer((nq,), torch.float64, dev) if qlabel is not None else None
    t2 = _buffer((nq, 2), torch.int32, dev) if top2 else None
    N.check(_lib().mmvae_knn_votes(N._ptr(idx), nq, k, N._ptr(rlabel), int(rlabel.numel()), int(n_classes),
                                   N._ptr(None if qlabel is None else qlabel.contiguous()), N._ptr(pred), N._ptr(purity), N._ptr(t2),
                                   N._stream(dev)), "mmvae_knn_votes")
    return pred, purity, t2


def _sqrt32(dist2: torch.Tensor) -> torch.Tensor:
    """The float32 square root of float32 values, correctly rounded on every backend: taken in float64 and rounded once more
    (53 >= 2 * 24 + 2 bits, so the second rounding cannot change the result).  A backend's own float32 sqrt may be 1 ulp off."""
    return torch.sqrt(dist2.to(torch.float64)).to(torch.float32)


def _host(a) -> np.ndarray:
    return np.asarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a)


def _is_device(x) -> bool:
    return isinstance(x, torch.Tensor) and x.device.type == "cuda"


def _float32_device(x, device, who: str, name: str) -> torch.Tensor:
    """``x`` as float32 [n, d] on the GPU: a float32 device tensor as it is, anything else rounded to float32 and uploaded.
    Host input is checked for NaN (infinities are distances like any other and pass)."""
    if _is_device(x) and x.dtype == torch.float32:
        return x
    from ..cpl_mixvae import get_device          # (cpl_mixvae imports this module, inside its functions)
    with np.errstate(over="ignore"):
        h = np.ascontiguousarray(_host(x), dtype=np.float32)
    if np.isnan(h).any():
        raise ValueError(f"{who}: {name} holds NaN")
    return torch.from_numpy(h if h.flags.writeable else h.copy()).to(get_device(device))


def _groups_host(who: str, name: str, g, n: int) -> np.ndarray:
    h = _host(g)
    if h.ndim != 1 or h.shape[0] != n or h.dtype.kind not in "iu":
        raise ValueError(f"{who}: {name} must be {n} integers")
    if h.size and (h.min() < -(1 << 31) or h.max() >= (1 << 31)):
        raise ValueError(f"{who}: {name} outside int32")
    return h.astype(np.int32)


def knn(x, k, ref=None, groups=None, ref_groups=None, exclude_self=None, device=None):
    """The ``k`` nearest reference points of every row of ``x`` -> ``(indices int32 [n, k], distances float32 [n, k])``,
    Euclidean, every row by rising (distance, index); where fewer than ``k`` references are admitted the tail is -1 / +inf.

    ``x`` [n, d] and ``ref`` [m, d]: a float32 tensor on the GPU is read where it lies (with its row stride); anything else
    is converted to float32 -- FLOAT64 INPUT IS ROUNDED -- and uploaded, after a check for NaN (a device tensor is not
    checked).  ``ref=None``: the set against itself, and ``exclude_self`` then defaults to True: a cell is not its own
    neighbour (the k-NN graph).  ``groups`` [n] and ``ref_groups`` [m], integers, both or neither (with ``ref=None`` the
    one array ``groups`` serves both): reference j is admitted for query i iff ``ref_groups[j] != groups[i]`` -- with each
    cell's fold as its group a test cell sees training cells only (and never itself).  ``exclude_self`` needs ``ref=None``
    and no groups.  The outputs are torch tensors on the device where ``x`` is one, else numpy arrays.  The distances are
    float32 square roots (correctly rounded) of the kernel's float32 squared distances in difference form; the
    neighbours are the same bits on every run.  k <= 64, d <= 128, n and m <= 1048576."""
    who = "knn"
    _refuse_dist(who)
    n, d = _shape2(who, "x", x)
    m, dr = (n, d) if ref is None else _shape2(who, "ref", ref)
    k = _check_shape(who, n, m, d, k)
    if dr != d:
        raise ValueError(f"{who}: x has {d} coordinates and ref {dr}")
    if ref is not None and exclude_self:
        raise ValueError(f"{who}: exclude_self needs ref=None (state the groups instead)")
    if ref is None and groups is not None and ref_groups is None:
        ref_groups = groups
    if (groups is None) != (ref_groups is None):
        raise ValueError(f"{who}: one group array without the other: groups and ref_groups come together")
    if groups is not None and exclude_self:
        raise ValueError(f"{who}: exclude_self and groups together: a cell shares its own group and is excluded already")
    qg = rg = None
    if groups is not None:
        qg = _groups_host(who, "groups", groups, n)
        rg = qg if ref is None and ref_groups is groups else _groups_host(who, "ref_groups", ref_groups, m)
    elif ref is None and (exclude_self is None or exclude_self):
        qg = rg = np.arange(n, dtype=np.int32)
    xd = _float32_device(x, device, who, "x")
    rd = xd if ref is None else _float32_device(ref, xd.device, who, "ref")
    if qg is not None:
        shared = rg is qg
        qg = torch.from_numpy(qg).to(xd.device)
        rg = qg if shared else torch.from_numpy(rg).to(xd.device)
    idx, dist2 = knn_device(xd, rd, k, qg, rg)
    dist = _sqrt32(dist2)
    if _is_device(x):
        return idx, dist
    return idx.cpu().numpy(), dist.cpu().numpy()


def csr_from_neighbors(indices: np.ndarray, data: Optional[np.ndarray], n_cols: int):
    """The CSR arrays ``(indptr int64 [n + 1], indices int32 [nnz], data float32 [nnz])`` of the graph with one row a query
    and the entries of ``indices`` [n, k] its columns; -1 entries are no neighbours.  A row's columns ascend, as in scipy's
    canonical form.  ``data`` [n, k]: the entries' values (None: 1.0, the connectivity graph)."""
    idx = np.asarray(indices)
    if idx.ndim != 2:
        raise ValueError(f"indices of shape {idx.shape} are not [n, k]")
    valid = idx >= 0
    if valid.any() and int(idx.max()) >= int(n_cols):
        raise IndexError(f"neighbour index {int(idx.max())} outside the {n_cols} columns")
    vals = np.ones(idx.shape, dtype=np.float32) if data is None else np.asarray(data, dtype=np.float32)
    if vals.shape != idx.shape:
        raise ValueError(f"data of shape {vals.shape} for indices of shape {idx.shape}")
    key = np.where(valid, idx, np.iinfo(np.int64).max).astype(np.int64)       # the invalid entries sort to a row's end
    order = np.argsort(key, axis=1, kind="stable")
    cols = np.take_along_axis(idx, order, axis=1)
    vals = np.take_along_axis(vals, order, axis=1)
    keep = cols >= 0
    indptr = np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(keep.sum(axis=1), dtype=np.int64)])
    return indptr, cols[keep].astype(np.int32), vals[keep].astype(np.float32)


def to_scipy(indptr, indices, data, n: int):
    """``scipy.sparse.csr_matrix`` of ``knn_graph``'s arrays, where scipy can be imported (ImportError where not)."""
    from scipy.sparse import csr_matrix
    return csr_matrix((data, indices, indptr), shape=(int(n), int(n)))


def knn_graph(x, k, mode: str = "distance", device=None):
    """The k-NN graph of the rows of ``x`` as numpy CSR arrays ``(indptr int64 [n + 1], indices int32 [nnz], data float32
    [nnz])`` of an n x n matrix: row i holds cell i's ``k`` nearest other cells (``knn`` with ``exclude_self``), the columns
    in ascending order; ``mode="distance"`` stores the Euclidean distances (sklearn's ``kneighbors_graph(mode="distance")``,
    what UMAP and scanpy's ``pp.neighbors`` take), ``"connectivity"`` ones.  ``to_scipy`` wraps them where scipy is there."""
    _refuse_dist("knn_graph")
    if mode not in ("distance", "connectivity"):
        raise ValueError(f"knn_graph: mode = {mode!r}: one of 'distance', 'connectivity'")
    idx, dist = knn(x, k, device=device)
    if isinstance(idx, torch.Tensor):
        idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
    return csr_from_neighbors(idx, dist if mode == "distance" else None, idx.shape[0])


def _encode(who: str, labels, n: int):
    y = _host(labels)
    if y.ndim != 1:
        raise ValueError(f"{who}: labels of shape {y.shape} are not 1-D")
    if y.shape[0] != n:
        raise ValueError(f"{who}: {y.shape[0]} labels for {n} samples")
    classes, codes = np.unique(y, return_inverse=True)
    if len(classes) > MAX_CLASSES:
        raise NotImplementedError(f"{who}: {len(classes)} classes above {MAX_CLASSES}")
    return classes, codes.reshape(-1).astype(np.int32)


def neighbor_purity(x, labels, k, device=None) -> dict:
    """Neighbourhood purity: the share of a cell's ``k`` nearest other cells that carry its own label -- the local
    counterpart of the silhouette, with no assumption on a cluster's shape.  ``x`` as for ``knn``; ``labels`` [n], encoded
    by ``np.unique``.  Returns ``{"cell": float64 [n], "classes": the unique labels, "per_class": float64 [K] the mean over
    each class's cells, "mean": the mean over all cells}``.  With n <= k a cell has n - 1 neighbours and the share is of
    those; n >= 2."""
    who = "neighbor_purity"
    _refuse_dist(who)
    n, d = _shape2(who, "x", x)
    k = _check_shape(who, n, n, d, k)
    if n < 2:
        raise ValueError(f"{who}: one cell has no neighbour")
    classes, codes = _encode(who, labels, n)
    xd = _float32_device(x, device, who, "x")
    own = torch.arange(n, dtype=torch.int32, device=xd.device)
    idx, _ = knn_device(xd, xd, k, own, own)
    lab = torch.from_numpy(codes).to(xd.device)
    _, purity, _ = knn_votes_device(idx, lab, len(classes), lab)
    cell = purity.cpu().numpy()
    per_class = np.array([np.mean(cell[codes == c]) for c in range(len(classes))], dtype=np.float64)
    return {"cell": cell, "classes": classes, "per_class": per_class, "mean": float(np.mean(cell))}


def _cv_refusals(who: str, labels, n: int, kfold, seed, k: int):
    """(y, classes, codes, fold) after every refusal that needs no device."""
    from .cluster_analysis import _label_refusals, kfold_of
    y = _label_refusals(labels, n, kfold)
    classes, codes = _encode(who, y, n)
    fold = kfold_of(n, int(kfold), seed)
    train = n - np.bincount(fold, minlength=int(kfold))
    if int(train.min()) < k:
        f = int(np.argmin(train))
        raise ValueError(f"Expected n_neighbors <= n_samples_fit, but n_neighbors = {k}, n_samples_fit = {int(train[f])} "
                         f"(the training cells of fold {f})")
    return y, classes, codes, fold


def _cv_on_device(x_dev: torch.Tensor, k: int, classes, codes, fold) -> dict:
    """One mmvae_knn call with each cell's fold as its group and one mmvae_knn_votes call, for points on the device."""
    dev = x_dev.device
    g = torch.from_numpy(fold.astype(np.int32)).to(dev)
    idx, dist2 = knn_device(x_dev, x_dev, k, g, g)
    lab = torch.from_numpy(codes).to(dev)
    pred, purity, top2 = knn_votes_device(idx, lab, len(classes), lab, top2=True)
    t2 = top2.cpu().numpy().astype(np.int64)
    return {"pred": pred.cpu().numpy().astype(np.int64), "fold": fold, "classes": classes,
            "kth_distance": _sqrt32(dist2[:, k - 1]).cpu().numpy(), "purity": purity.cpu().numpy(),
            "best": t2[:, 0], "second": t2[:, 1]}


def knn_cv_predict(x, labels, kfold, seed, k=15, device=None) -> dict:
    """k-fold cross-validated prediction of ``labels`` from the points ``x`` by the ``k`` nearest training cells: sklearn's
    ``KNeighborsClassifier(n_neighbors=k)`` inside ``KFold(n_splits=kfold, shuffle=True, random_state=seed)``
    (``cluster_analysis.kfold_of``), every cell voted on by the cells of the folds it is not in -- one ``mmvae_knn`` call with
    each cell's fold as its group, one ``mmvae_knn_votes`` call.  Uniform votes; ties go to the smallest label, as sklearn's
    do; neighbours at equal float32 distance enter by rising index.  ``x`` as for ``knn``; ``labels`` 1-D, encoded by
    ``np.unique``.  Returns a dict: ``pred`` int64 [n] the predicted code (``classes[pred]`` the label), ``fold`` int64 [n],
    ``classes``, ``kth_distance`` float32 [n] (the distance of the k-th training neighbour), ``purity`` float64 [n] (the share
    of the k training neighbours with the cell's own label), ``best`` and ``second`` int64 [n] (the votes of the prediction
    and of the runner-up).  ValueError for a label length mismatch, ``kfold`` outside [2, n], NaN in host ``x`` and a fold
    that leaves fewer than ``k`` training cells (where sklearn raises); NotImplementedError under a process group and past
    k = 64, d = 128, 1048576 cells or 4096 classes."""
    who = "knn_cv_predict"
    _refuse_dist(who)
    n, d = _shape2(who, "x", x)
    k = _check_shape(who, n, n, d, k)
    _, classes, codes, fold = _cv_refusals(who, labels, n, kfold, seed, k)
    return _cv_on_device(_float32_device(x, device, who, "x"), k, classes, codes, fold)


def classify_points(x_dev: torch.Tensor, y, kfold, seed, k: int, checked=None):
    """One label set on points already on the device: (acc, ref_labels, pred_labels, the ``knn_cv_predict`` dict), the first
    three lists over the folds with every test set in ascending order of the cell index."""
    from .cluster_analysis import _fold_lists
    n, d = (int(v) for v in x_dev.shape)
    k = _check_shape("KNN_classifier", n, n, d, k)
    y, classes, codes, fold = checked if checked is not None else _cv_refusals("KNN_classifier", y, n, kfold, seed, k)
    res = _cv_on_device(x_dev, k, classes, codes, fold)
    return (*_fold_lists(y, classes, res["pred"], fold, kfold), res)


def KNN_classifier(data, labels, kfold, seed, k=15):
    """The k-NN member of the ``QDA_classifier`` / ``LDA_classifier`` / ``RF_classifier`` family: ``(acc, ref_labels,
    pred_labels)``, dicts over the keys of the dict ``labels``, each a list over the folds of ``KFold(n_splits=kfold,
    random_state=seed, shuffle=True)``: the accuracy (a Python float), the held-out cells' labels and their predictions, in
    the caller's label values and in ascending order of the cell index.  ``data`` is uploaded once for all keys.  The
    classifier and the refusals are those of ``knn_cv_predict``."""
    who = "KNN_classifier"
    _refuse_dist(who)
    n, d = _shape2(who, "data", data)
    k = _check_shape(who, n, n, d, k)
    checked = {key: _cv_refusals(who, labels[key], n, kfold, seed, k) for key in labels}
    points = _float32_device(data, None, who, "data")
    acc, ref_labels, pred_labels = {}, {}, {}
    for key in checked:
        acc[key], ref_labels[key], pred_labels[key], _ = classify_points(points, labels[key], kfold, seed, k, checked[key])
    return acc, ref_labels, pred_labels

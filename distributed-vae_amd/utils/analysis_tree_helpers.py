"""The tree-based analysis of the reference's ``mmidas/utils/analysis_tree_helpers.py``: ``predict_leaf_gmm``, ``custom_QDA``,
``get_merge_sequence``, ``do_merges``, ``get_descendants``, ``get_ancestors`` and ``parse_dend``, on the device, without scipy --
and ``merge_sweep``, which the reference does not have: the accuracy at EVERY merge level of the dendrogram from one fit, one
score launch and one merge launch, where the reference refits the same Gaussians and loops over the leaves' pdfs once per level.

``predict_leaf_gmm`` fits one Gaussian per leaf type to the training cells, turns a test cell's densities into probabilities
over the leaves, adds the probabilities of the leaves under each label of a coarser label set, and predicts the label with
the largest sum.  Here one pass of ``mmvae_group_moments`` (csrc/gaussclf.hip) gives every leaf's moments about one pivot,
the models are built on the host in fp64 (``leaf_gaussians``), ``mmvae_gauss_scores`` gives every cell's log weight + log
density under every leaf, and ``mmvae_leaf_merge`` (csrc/leafmerge.hip; include/mmvae.h) normalises them
IN THE LOG DOMAIN and merges them at all requested levels at once.  Departures, each stated where it applies: log-domain
normalisation (equal to the reference wherever its row sum neither underflows nor overflows, finite where it gives 0 / 0 =
NaN and then silently predicts column 0); no input is modified in place; ValueError where the reference stops in ``pdb``.

``get_cvfold``, ``get_cvfold_extended``, ``get_cca_projections``, ``plot_htree`` and the ``Node`` class of that module belong to
another model or to plotting and are not part of this package."""
from __future__ import annotations

from collections import deque

import numpy as np

from .. import _native as N
from .. import dist as D
from .._utils import float32_on_device
from .cluster_analysis import _moments_on_device, _scores_by_fold, _shape_of, fold_training_moments, kfold_of

LEAF_REG = 1e-4                 # the reference's cov + 1e-4 I (predict_leaf_gmm)
SINGULAR_EPS = 1e6 * 2.0 ** -52  # scipy's multivariate_normal: an eigenvalue at or below this share of the largest counts as 0
DEND_COLUMNS = ("x", "y", "leaf", "label", "parent", "col")     # the columns of the dendrogram's csv export that parse_dend keeps


# ---- the tree helpers (host, numpy) -------------------------------------------------------------------------------------
def get_descendants(child, parent, y, ancestor, leafonly=False):
    """The reference's ``get_descendants``: every descendant of ``ancestor``, a list in breadth-first order (a node's children
    in row order); with ``leafonly`` only those that are nobody's parent, here in the same order (the reference returns them
    in the arbitrary order of a set).  ``y`` is unused, as in the reference."""
    below = _children_by_parent(child, parent)
    found = _reach(below, _plain(ancestor))
    return [name for name in found if name not in below] if leafonly else found


def _reach(below, top):
    """Every node under ``top`` in the map node -> children: level by level, a node's children in their order."""
    found, queue = [], deque([top])
    while queue:
        kids = below.get(queue.popleft(), ())
        found.extend(kids)
        queue.extend(kids)
    return found


def _plain(name):
    """A numpy scalar as the Python value it holds: dictionary keys and list entries are plain values."""
    return name.item() if isinstance(name, np.generic) else name


def _children_by_parent(child, parent):
    """{node: the names of its children, in row order} of a tree given as one row per node."""
    below = {}
    for name, above in zip(np.asarray(child).tolist(), np.asarray(parent).tolist()):
        below.setdefault(above, []).append(name)
    return below


def get_ancestors(node, child, parent):
    """The reference's ``get_ancestors``: the parents of ``node`` up to the root, nearest first; the root's name is ``'n1'``, as
    the reference fixes it.  ValueError for a node that is no child (the reference fails there with an IndexError)."""
    above_of = {}
    for name, above in zip(np.asarray(child).tolist(), np.asarray(parent).tolist()):
        above_of.setdefault(name, above)
    chain, at = [], _plain(node)
    while at != 'n1':
        if at not in above_of or len(chain) > len(above_of):
            raise ValueError(f"get_ancestors: {at!r} is not a child in this tree and not the root 'n1'")
        at = above_of[at]
        chain.append(at)
    return chain


def get_merge_sequence(child, parent, y):
    """The reference's ``get_merge_sequence``: ``list_changes``, one ``[children, parent, remaining nodes]`` per merge.  The
    internal nodes (a height that is neither 0 nor NaN) merge in ascending order of (height, row) -- the reference's repeated
    ``np.nanargmin`` takes the first of equal heights --, a node's children, in row order, all in one step however many
    there are; ``remaining nodes`` counts the distinct names still in the tree after the step, and the sequence ends when one
    is left.  A node that was merged away as a child before its turn never merges.  DEPARTURE: ``y`` is not modified (the
    reference writes NaN into the caller's array).  ValueError where the rows are not one tree."""
    names = np.asarray(child).tolist()
    above = np.asarray(parent).tolist()
    height = np.array(y, dtype=np.float64)
    height[height == 0] = np.nan
    rows_under = {}
    for row, p in enumerate(above):
        rows_under.setdefault(p, []).append(row)
    in_tree = [True] * len(names)
    how_many = {}
    for name in names:
        how_many[name] = how_many.get(name, 0) + 1
    merged, sequence = set(), []
    for row in np.argsort(height, kind="stable").tolist():               # NaN heights sort last
        if len(how_many) <= 1 or np.isnan(height[row]):
            break
        if not in_tree[row] or names[row] in merged:
            continue
        node = names[row]
        gone = [r for r in rows_under.get(node, ()) if in_tree[r]]
        if not gone:
            raise ValueError(f"get_merge_sequence: {node!r} has a height and no children")
        for r in gone:
            in_tree[r] = False
            how_many[names[r]] -= 1
            if how_many[names[r]] == 0:
                del how_many[names[r]]
        merged.add(node)
        sequence.append([[names[r] for r in gone], node, len(how_many)])
    if len(how_many) > 1:
        raise ValueError("get_merge_sequence: nodes remain and none of them has a height: not one tree")
    return sequence


def _roomy(labels: np.ndarray, names) -> np.ndarray:
    """A copy of ``labels`` that can hold every one of ``names``: a fixed-width string array is widened (numpy would cut a
    longer name to the array's width without a word)."""
    labels = np.array(labels)
    if labels.dtype.kind in "US" and len(names):
        width = max(len(str(v)) for v in names)
        if labels.dtype.kind == "U" and labels.dtype.itemsize // 4 < width:
            labels = labels.astype(f"<U{width}")
        elif labels.dtype.kind == "S" and labels.dtype.itemsize < width:
            labels = labels.astype(f"S{width}")
    return labels


def do_merges(labels, list_changes=[], n_merges=0):
    """The reference's ``do_merges``: ``labels`` after the first ``n_merges`` merges of ``list_changes``, every child's name
    replaced by its parent's, merge after merge (all of them, with a printed note, where there are fewer).  DEPARTURES: a
    relabelled COPY is returned and ``labels`` is left as it was; a string array too narrow for a parent's name is widened
    (the reference cuts the name)."""
    steps = list_changes[:max(int(n_merges), 0)]
    if n_merges > len(list_changes):
        print(f"do_merges: {n_merges} merges asked for, the sequence has {len(list_changes)}: all of them performed")
    return _relabel(labels, [(kid, step[1]) for step in steps for kid in step[0]])


def _relabel(labels, pairs):
    """A copy of ``labels`` after the replacements ``pairs`` = (from, to), ... applied one after the other, each to the labels
    as the earlier ones left them.  The pairs are first folded into one table name -> final name (a name that reaches
    ``from`` by earlier replacements follows it to ``to``), which is then applied to the distinct labels once."""
    holds, left = {}, set()                                     # current name -> the original names that now carry it;
                                                                # the names whose own cells have moved on
    def carriers(name):
        return holds.pop(name) if name in holds else ([] if name in left else [name])

    for src, dst in pairs:
        src, dst = _plain(src), _plain(dst)
        if src != dst:
            holds[dst] = carriers(dst) + carriers(src)
            left.add(src)
    final = {orig: now for now, origs in holds.items() for orig in origs}
    out = _roomy(labels, list(final.values()))
    distinct, where = np.unique(out, return_inverse=True)
    renamed = [final.get(v, v) for v in distinct.tolist()]
    if renamed != distinct.tolist():
        table = np.array(renamed, dtype=out.dtype if out.dtype.kind in "USO" else None)
        out = table[where.reshape(-1)].reshape(out.shape)
    return out


def labels_at(leaves, list_changes, n_merges):
    """The label set after ``n_merges`` merges: ``np.unique(do_merges(leaves, list_changes, n_merges))``, sorted as
    ``predict_leaf_gmm`` takes it for ``unique_dataset_lbl``."""
    return np.unique(do_merges(np.unique(leaves), list_changes, n_merges))


def descendants_at(list_changes, n_merges):
    """``descendant_dict`` for ``predict_leaf_gmm`` at the level after ``n_merges`` merges: every merged node that is a label
    of that level -> all nodes merged into it, directly or through its children."""
    below, alive = {}, {}
    for i in range(min(int(n_merges), len(list_changes))):
        kids, node = list_changes[i][0], list_changes[i][1]
        below[node] = [g for c in kids for g in [c] + below.get(c, [])]
        for c in kids:
            alive.pop(c, None)
        alive[node] = below[node]
    return alive


def parse_dend(htree_file):
    """The reference's ``parse_dend``: ``(list_changes, descendants, treeobj, leaves, child, parent)`` from the csv export of
    the dendrogram (columns x, y, leaf, label, parent, col), rows sorted by (y, x) and leaves given the height NaN.  pandas
    is imported here and not with the module."""
    try:
        import pandas as pd
    except ImportError as e:
        raise ImportError("parse_dend reads the dendrogram with pandas, which is not installed") from e
    raw = pd.read_csv(htree_file)
    missing = [c for c in DEND_COLUMNS if c not in raw.columns]
    if missing:
        raise ValueError(f"parse_dend: {htree_file} has no column {missing}")
    height = raw["y"].to_numpy(dtype=np.float64)
    order = np.lexsort((raw["x"].to_numpy(dtype=np.float64), height))            # by height, then by x
    is_leaf = raw["leaf"].eq(True).to_numpy()[order]                             # the export leaves the others' flag empty
    treeobj = raw.loc[:, list(DEND_COLUMNS)].iloc[order].reset_index(drop=True)
    treeobj["leaf"] = is_leaf
    treeobj["y"] = np.where(is_leaf, np.nan, height[order])
    child, parent = treeobj["label"].to_numpy(), treeobj["parent"].to_numpy()
    list_changes = get_merge_sequence(child, parent, treeobj["y"].to_numpy())
    below = _children_by_parent(child, parent)
    nodes = dict.fromkeys(child.tolist() + [p for p in parent.tolist() if p == p])   # (a missing parent is NaN: p != p)
    descendants = {node: _reach(below, node) for node in nodes}
    return list_changes, descendants, treeobj, child[is_leaf], child, parent


# ---- the leaf models ------------------------------------------------------------------------------------------------------
def _labels_of(lbl, n, who, name):
    y = np.asarray(lbl)
    if y.ndim != 1 or y.shape[0] != n:
        raise ValueError(f"{who}: {name} of shape {y.shape} for {n} cells")
    return y


def _leaf_refusals(who, unique_leaf_lbl, label_weight, n_per_class_thr):
    """(the leaves in ``np.unique`` order, log weight [L]) after the refusals that need no device."""
    leaves = np.unique(np.asarray(unique_leaf_lbl))
    L = len(leaves)
    if L < 1:
        raise ValueError(f"{who}: unique_leaf_lbl is empty")
    if L > N.LEAFMERGE_MAX_L:
        raise NotImplementedError(f"{who}: {L} leaves: at most {N.LEAFMERGE_MAX_L}")
    if n_per_class_thr < 1:
        raise ValueError(f"{who}: n_per_class_thr = {n_per_class_thr} below 1: a covariance needs two cells")
    if label_weight is None or len(label_weight) == 0:
        return leaves, np.zeros(L)
    w = np.asarray(label_weight, dtype=np.float64).reshape(-1)
    if w.shape[0] != L:
        raise ValueError(f"{who}: {w.shape[0]} label weights for {L} leaves")
    if not np.isfinite(w).all() or (w < 0).any():
        raise ValueError(f"{who}: label weights must be finite and not negative")
    with np.errstate(divide="ignore"):
        return leaves, np.log(w)


def models_from_leaf_moments(s, M, counts, pivot, logw, n_per_class_thr, diag_cov_n_sample_thr, reg, who="leaf_gaussians",
                             names=None):
    """The F leaf models from the moments of the L x F (leaf, fold) groups about ``pivot``: ``s`` [L, F, d], ``M``
    [L, F, d (d + 1) / 2], ``counts`` [L, F] -> (mu [F, L, d], W [F, L, d, d], c0 [F, L], training counts [F, L]) in fp64.
    F = 1: the one group is the training set; F > 1: the training set of fold f is the sum of the other folds' groups, added
    in fold order with no subtraction.  mean = pivot + s / N; C = (M - s s^T / N) / (N - 1) + reg I, its diagonal alone for
    N < diag_cov_n_sample_thr; W = V lam^(-1/2) of eigh(C); c0 = log weight - sum(log lam) / 2 - (d / 2) log(2 pi), -inf for
    N <= n_per_class_thr.  ValueError naming the leaf (``names[l]``, or its index) where C is singular by scipy's rule for
    ``multivariate_normal`` (smallest eigenvalue <= 1e6 x 2^-52 x the largest), where the reference raises ``LinAlgError``."""
    L, F, d = s.shape
    pivot = np.asarray(pivot, dtype=np.float64)
    mu, W, c0 = np.zeros((F, L, d)), np.zeros((F, L, d, d)), np.full((F, L), -np.inf)
    train = np.zeros((F, L), dtype=np.int64)
    for f, (cnt, offset, scatter) in enumerate(fold_training_moments(s, M, counts)):
        train[f] = cnt.astype(np.int64)
        have = np.flatnonzero(cnt > n_per_class_thr)
        if have.size == 0:
            continue
        mu[f, have] = pivot[None] + offset[have]
        C = scatter[have] / (cnt[have][:, None, None] - 1.0) + reg * np.eye(d)[None]
        diag = cnt[have] < diag_cov_n_sample_thr
        C[diag] = C[diag] * np.eye(d)[None]
        lam, V = np.linalg.eigh(C)
        bad = np.flatnonzero(~(lam[:, 0] > SINGULAR_EPS * np.abs(lam).max(axis=1)))
        if bad.size:
            which = have[bad[0]] if names is None else names[have[bad[0]]]
            raise ValueError(f"{who}: the covariance of label {str(which)!r} is singular")
        W[f, have] = V * (lam ** -0.5)[:, None, :]
        c0[f, have] = logw[have] - 0.5 * np.sum(np.log(lam), axis=1) - 0.5 * d * np.log(2.0 * np.pi)
    return mu, W, c0, train


def _fit(train_dev, codes, L, fold, F, logw, n_per_class_thr, diag_cov_n_sample_thr, reg, who, names):
    """One ``group_moments`` launch over the training cells of the leaves (``codes`` >= 0) sorted by (leaf, fold) and the host
    models of it; ``pivot`` is the mean of all training cells."""
    s, M, counts, pivot = _moments_on_device(train_dev, codes, L, fold, F)
    mu, W, c0, train = models_from_leaf_moments(s, M, counts, pivot.cpu().numpy(), logw, n_per_class_thr, diag_cov_n_sample_thr,
                                                reg, who, names)
    return {"mu": mu, "W": W, "c0": c0, "counts": train, "pivot": pivot.cpu().numpy().astype(np.float64)}


def _codes_of(lbl, leaves):
    """The index of every label in the sorted ``leaves``, -1 for a label that is none of them."""
    pos = np.searchsorted(leaves, lbl)
    pos[pos >= len(leaves)] = 0
    return np.where(leaves[pos] == lbl, pos, -1).astype(np.int64)


def leaf_gaussians(train_z, true_train_lbl, unique_leaf_lbl, n_per_class_thr=6, diag_cov_n_sample_thr=12, reg=LEAF_REG,
                   label_weight=None, fold=None, device=None):
    """One Gaussian per leaf type, the reference's (``predict_leaf_gmm``): for a leaf with more than ``n_per_class_thr``
    training cells the mean and ``np.cov`` (ddof = 1) + ``reg`` I -- its diagonal alone below ``diag_cov_n_sample_thr`` cells --
    as W = V lam^(-1/2) and c0 = log weight - sum(log lam) / 2 - (d / 2) log(2 pi), so that c0 - |W^T (x - mean)|^2 / 2 is the
    log of weight x density; c0 = -inf (no model) for a leaf with fewer cells, and for a weight of 0.

    The training cells are sorted by (leaf[, fold]) and ONE ``mmvae_group_moments`` launch gives every group's moments about
    the training cells' mean; the models are built from them on the host in fp64.  ``fold``: int [n], the fold of every
    training cell; the model of fold f is then fitted to the cells of the OTHER folds (sums of groups), as the classifiers of
    ``cluster_analysis`` do it.  Training cells whose label is no leaf are not used.  ``train_z``: array-like or tensor
    [n, d], d <= 128; a float32 tensor on the GPU is used where it lies, anything else is ROUNDED to float32 and uploaded.

    Returns a dict: ``leaves`` (``np.unique(unique_leaf_lbl)``), ``mu`` [F, L, d], ``W`` [F, L, d, d], ``c0`` [F, L],
    ``counts`` int64 [F, L] (the training cells of every model) and ``pivot`` [d], F = 1 without ``fold``.  ValueError for
    negative or non-finite weights, a weight count other than L, mismatched lengths, non-finite points, and a covariance that
    is not positive definite (``reg`` = 0); NotImplementedError under a process group, for d outside [1, 128], more than
    4096 leaves or more than 64 folds."""
    who = "leaf_gaussians"
    if D.is_dist():
        raise NotImplementedError(f"{who} is not data-parallel: run it on one rank, outside the process group")
    n, d = _shape_of(train_z, N.GAUSSCLF_MAX_D, min_n=1, who=who, name="train_z")
    lbl = _labels_of(true_train_lbl, n, who, "true_train_lbl")
    leaves, logw = _leaf_refusals(who, unique_leaf_lbl, label_weight, n_per_class_thr)
    F = 1
    if fold is not None:
        fold = np.asarray(fold)
        if fold.shape != (n,) or fold.dtype.kind not in "iu" or fold.min() < 0:
            raise ValueError(f"{who}: fold must be a non-negative int array [{n}]")
        F = int(fold.max()) + 1
        if not 2 <= F <= N.GAUSSCLF_MAX_F:
            raise NotImplementedError(f"{who}: {F} folds outside [2, {N.GAUSSCLF_MAX_F}]")
        fold = fold.astype(np.int64)
    x_dev = float32_on_device(train_z, device, "train_z", "[n, d]", check_device_finite=True)
    out = _fit(x_dev, _codes_of(lbl, leaves), len(leaves), fold, F, logw, n_per_class_thr, diag_cov_n_sample_thr, float(reg), who,
               leaves)
    out["leaves"] = leaves
    return out


def _scores(x_dev, models, fold=None):
    """float64 [n, L] on the device: every cell's log weight + log density under every leaf (of its fold's model)."""
    return _scores_by_fold(x_dev, models["mu"], models["W"], models["c0"], fold, True)[3]


def _label_lists(who, dataset_lbl, leaves, descendant_dict):
    """The reference's rule for the columns of the merged matrix, as lists of leaf indices in increasing order."""
    has_map = any(bool(v) for v in descendant_dict.values()) if descendant_dict else False
    lists = []
    for lab in dataset_lbl:
        own = np.flatnonzero(leaves == lab)
        if own.size:
            lists.append([int(own[0])])
        elif has_map:
            lists.append([int(i) for i in np.flatnonzero(np.isin(leaves, list(descendant_dict.get(lab) or [])))])
        else:
            raise ValueError(f"{who}: label {lab!r} is no leaf and there is no descendant_dict to merge it from")
    return lists


# ---- the public functions -------------------------------------------------------------------------------------------------
def predict_leaf_gmm(train_z, true_train_lbl, test_z, true_test_lbl=None, n_per_class_thr=6, diag_cov_n_sample_thr=12,
                     unique_dataset_lbl=[], unique_leaf_lbl=[], descendant_dict={}, label_weight=[], device=None):
    """The reference's ``predict_leaf_gmm``: ``(true_test_lbl, pred_test_lbl, n_excluded_cells, n_classes_predicted,
    n_classes_removed, pred_probability)``.  One Gaussian per leaf of ``unique_leaf_lbl`` (``leaf_gaussians``: more than
    ``n_per_class_thr`` training cells, diagonal below ``diag_cov_n_sample_thr``, + 1e-4 I), a test cell's weighted densities
    normalised over the leaves, added over the leaves of every label of ``unique_dataset_lbl`` -- a label that is a leaf takes
    that leaf alone, any other the leaves among ``descendant_dict[label]``, a label with neither a zero column -- and the label
    with the largest sum predicted (``np.argmax``: the first on ties); ``pred_probability`` is that sum.  Test cells whose true
    label is a leaf without a model are dropped from every return and counted in ``n_excluded_cells``; the true labels of the
    others are relabelled ``from -> to`` for every (key, member) of ``descendant_dict`` in its order, as the reference does.
    The path is ``mmvae_group_moments`` -> host models -> ``mmvae_gauss_scores`` -> ``mmvae_leaf_merge``.

    DEPARTURES.  (1) The normalisation is done in the log domain: the posterior is exp(s - max s) / sum, which equals the
    reference's pdf / sum(pdf) wherever that sum neither underflows nor overflows; for a cell far from every class the
    reference computes 0 / 0 = NaN and then labels it with column 0, this function gives the finite posterior.  A cell is NaN
    here only when no leaf has a model.  (2) ``true_test_lbl`` is not modified in place, and a string array too narrow for a
    merged name is widened, not cut.  (3) ``true_test_lbl=None`` (or empty): nothing is dropped and None is returned for it
    (the reference's own default ``[]`` fails).  (4) ValueError where the reference stops in ``pdb`` (a label that is no leaf
    without a ``descendant_dict``), where its ``assert`` fires (``descendant_dict`` without ``unique_dataset_lbl``), and for an
    empty ``unique_dataset_lbl``.  (5) The points are float32 on the device (FLOAT64 INPUT IS ROUNDED).

    ValueError also for mismatched lengths or dimensions, non-finite points, and bad weights; NotImplementedError under a
    process group, for d outside [1, 128] and for more than 4096 leaves or labels -- all before any device work."""
    who = "predict_leaf_gmm"
    if D.is_dist():
        raise NotImplementedError(f"{who} is not data-parallel: run it on one rank, outside the process group")
    prep = _prepare(who, train_z, true_train_lbl, test_z, true_test_lbl, unique_leaf_lbl, label_weight, n_per_class_thr)
    leaves, logw, train_lbl, test_lbl = prep
    dataset_lbl = np.array(unique_dataset_lbl)
    if dataset_lbl.ndim != 1 or dataset_lbl.size == 0:
        raise ValueError(f"{who}: unique_dataset_lbl should not be empty" + (" if descendant_dict is provided" if descendant_dict else ""))
    if dataset_lbl.size > N.LEAFMERGE_MAX_K:
        raise NotImplementedError(f"{who}: {dataset_lbl.size} labels: at most {N.LEAFMERGE_MAX_K}")
    lists = _label_lists(who, dataset_lbl, leaves, descendant_dict)
    train_dev = float32_on_device(train_z, device, "train_z", "[n, d]", check_device_finite=True)
    test_dev = float32_on_device(test_z, train_dev.device, "test_z", "[n, d]", check_device_finite=True)
    models = _fit(train_dev, _codes_of(train_lbl, leaves), len(leaves), None, 1, logw, n_per_class_thr, diag_cov_n_sample_thr,
                  LEAF_REG, who, leaves)
    post = _scores(test_dev, models)
    label, _, _, merged = N.leaf_merge(post, *N.merge_tables([lists]), return_second=False, return_merged=True)
    no_model = leaves[models["counts"][0] <= n_per_class_thr]
    dropped = np.zeros(int(test_dev.shape[0]), dtype=bool) if test_lbl is None else np.isin(test_lbl, no_model)
    kept = np.flatnonzero(~dropped)
    chosen = label.cpu().numpy()[0].astype(np.int64)[kept]
    prob = merged.cpu().numpy()[kept, chosen]
    true = None
    if test_lbl is not None:
        true = _relabel(test_lbl[kept], [(member, key) for key, members in descendant_dict.items() for member in members or ()])
    lost = int(np.count_nonzero(np.isin(dataset_lbl, no_model)))
    return true, dataset_lbl[chosen], int(dropped.sum()), len(dataset_lbl) - lost, lost, prob


def _prepare(who, train_z, true_train_lbl, test_z, true_test_lbl, unique_leaf_lbl, label_weight, n_per_class_thr):
    """(leaves, log weights, training labels, test labels or None) after the refusals that need no device."""
    n, d = _shape_of(train_z, N.GAUSSCLF_MAX_D, min_n=1, who=who, name="train_z")
    n_test, d_test = _shape_of(test_z, N.GAUSSCLF_MAX_D, min_n=1, who=who, name="test_z")
    if d_test != d:
        raise ValueError(f"{who}: test_z has {d_test} columns and train_z {d}")
    train_lbl = _labels_of(true_train_lbl, n, who, "true_train_lbl")
    test_lbl = None
    if true_test_lbl is not None and len(true_test_lbl) > 0:
        test_lbl = _labels_of(true_test_lbl, n_test, who, "true_test_lbl")
    leaves, logw = _leaf_refusals(who, unique_leaf_lbl, label_weight, n_per_class_thr)
    return leaves, logw, train_lbl, test_lbl


def custom_QDA(train_z, true_train_lbl, test_z, true_test_lbl, n_per_class_thr=6, diag_cov_n_sample_thr=12, device=None):
    """The reference's ``custom_QDA``: ``(true_test_lbl, pred_test_lbl)``.  One Gaussian per class of the union of the train
    and test labels with more than ``n_per_class_thr`` training cells -- ``np.cov``, its diagonal alone below
    ``diag_cov_n_sample_thr`` cells, NO regulariser, no class weights -- and the class of the largest density predicted; the
    arg-max is taken over the log densities.  A class without a model is never predicted.  The exclusion step -- both returns read
    ``'excluded'`` for the test cells whose true class has no model -- runs whenever ``true_test_lbl`` is given: the
    reference's own ``if true_test_lbl:`` raises ValueError on any array of more than one element and skips the step for a
    list, so the reference can only run with list labels and no excluded class.  DEPARTURES: ``true_test_lbl`` is not
    modified in place; a singular covariance raises ValueError naming the label (scipy raises ``LinAlgError``).
    Refusals as ``predict_leaf_gmm``."""
    who = "custom_QDA"
    if D.is_dist():
        raise NotImplementedError(f"{who} is not data-parallel: run it on one rank, outside the process group")
    if true_test_lbl is None:
        raise ValueError(f"{who}: true_test_lbl is needed: the classes are those of the train and the test labels")
    n_test, _ = _shape_of(test_z, N.GAUSSCLF_MAX_D, min_n=1, who=who, name="test_z")
    test_all = _labels_of(true_test_lbl, n_test, who, "true_test_lbl")
    classes = np.unique(np.concatenate([np.asarray(true_train_lbl).reshape(-1), test_all]))
    leaves, logw, train_lbl, test_lbl = _prepare(who, train_z, true_train_lbl, test_z, test_all, classes, None, n_per_class_thr)
    train_dev = float32_on_device(train_z, device, "train_z", "[n, d]", check_device_finite=True)
    test_dev = float32_on_device(test_z, train_dev.device, "test_z", "[n, d]", check_device_finite=True)
    models = _fit(train_dev, _codes_of(train_lbl, leaves), len(leaves), None, 1, logw, n_per_class_thr, diag_cov_n_sample_thr, 0.0,
                  who, leaves)
    label = _scores_by_fold(test_dev, models["mu"], models["W"], models["c0"], None, False)[0]
    excluded = leaves[models["counts"][0] <= n_per_class_thr]
    pred = _roomy(leaves[label.cpu().numpy().astype(np.int64)], ["excluded"] if len(excluded) else [])
    true = _roomy(test_all, ["excluded"] if len(excluded) else [])
    gone = np.isin(test_all, excluded)
    if gone.any():
        if pred.dtype.kind not in "USO":
            pred, true = pred.astype(object), true.astype(object)
        pred[gone] = 'excluded'
        true[gone] = 'excluded'
    return true, pred


def _sweep_levels(who, leaves, list_changes, levels):
    """(the levels as numbers of merges; per level its label set, its lists of leaf indices and every leaf's label).  The
    merges are applied one after the other, once, and the requested levels are read off on the way."""
    if levels is not None:
        levels = [int(m) for m in levels]
        if not levels or any(not 0 <= m <= len(list_changes) for m in levels):
            raise ValueError(f"{who}: levels must be numbers of merges in [0, {len(list_changes)}], at least one")
    at = _roomy(leaves, [c[1] for c in list_changes])           # every leaf's label at the level reached
    seen = {}
    for m in range((len(list_changes) if levels is None else max(levels)) + 1):
        if m > 0:
            for c_node in list_changes[m - 1][0]:
                at[at == c_node] = list_changes[m - 1][1]
        if levels is None or m in levels:
            labs, inverse = np.unique(at, return_inverse=True)
            order = np.argsort(inverse.reshape(-1), kind="stable")
            cuts = np.cumsum(np.bincount(inverse.reshape(-1), minlength=len(labs)))[:-1]
            seen[m] = (labs, [part.tolist() for part in np.split(order, cuts)], at.copy())
    if levels is None:
        levels = [m for m in sorted(seen) if len(seen[m][0]) >= 2]
        if not levels:
            raise ValueError(f"{who}: no level of this tree has two labels")
    if len(levels) > N.LEAFMERGE_MAX_T:
        raise NotImplementedError(f"{who}: {len(levels)} levels: at most {N.LEAFMERGE_MAX_T}")
    return levels, [seen[m][0] for m in levels], [seen[m][1] for m in levels], [seen[m][2] for m in levels]


def _true_at(lbl, codes, at, list_changes, m):
    """The true labels after m merges: a cell of a leaf takes its leaf's label at that level; any other label is merged as
    ``do_merges`` merges it."""
    known = codes >= 0
    out = _roomy(np.array(lbl), at)
    out[known] = at[codes[known]]
    if not known.all():
        out[~known] = do_merges(out[~known], list_changes, m)
    return out


def merge_sweep(train_z, true_train_lbl, test_z, true_test_lbl, list_changes, leaves, levels=None, device=None, **leaf_kwargs):
    """``predict_leaf_gmm`` at every merge level of the dendrogram at once: one fit, one score launch and one
    ``mmvae_leaf_merge`` over all levels, where the reference refits and rescores per level.  ``list_changes``: the merge
    sequence (``get_merge_sequence`` / ``parse_dend``); ``leaves``: the leaf labels; ``levels``: the numbers of merges to
    evaluate, by default every one from 0 (all leaves) down to the last that leaves two labels.  ``leaf_kwargs``:
    ``n_per_class_thr``, ``diag_cov_n_sample_thr``, ``label_weight`` as in ``predict_leaf_gmm``.

    Level m is exactly ``predict_leaf_gmm(..., unique_dataset_lbl=labels_at(leaves, list_changes, m), unique_leaf_lbl=leaves,
    descendant_dict=descendants_at(list_changes, m))``: the levels of one ``mmvae_leaf_merge`` call do not build on each
    other.  Returns a dict: ``levels`` [T], ``n_classes`` int64 [T] the labels of every level, ``acc`` float64 [T] the
    accuracy over the kept cells (those whose leaf has a model; NaN where none is kept), ``pred`` [T, n_kept] the predicted
    labels, ``prob`` float64 [T, n_kept], ``true`` [T, n_kept] the merged true labels, ``keep`` bool [n_test] and
    ``n_excluded_cells``.  Refusals as ``predict_leaf_gmm``; ValueError for a level outside [0, len(list_changes)]."""
    who = "merge_sweep"
    if D.is_dist():
        raise NotImplementedError(f"{who} is not data-parallel: run it on one rank, outside the process group")
    bad = set(leaf_kwargs) - {"n_per_class_thr", "diag_cov_n_sample_thr", "label_weight"}
    if bad:
        raise TypeError(f"{who}: unexpected arguments {sorted(bad)}")
    thr, dthr = leaf_kwargs.get("n_per_class_thr", 6), leaf_kwargs.get("diag_cov_n_sample_thr", 12)
    if true_test_lbl is None:
        raise ValueError(f"{who}: true_test_lbl is needed for the accuracies")
    uleaves, logw, train_lbl, test_lbl = _prepare(who, train_z, true_train_lbl, test_z, true_test_lbl, leaves,
                                                  leaf_kwargs.get("label_weight"), thr)
    levels, label_sets, lists, at = _sweep_levels(who, uleaves, list_changes, levels)
    train_dev = float32_on_device(train_z, device, "train_z", "[n, d]", check_device_finite=True)
    test_dev = float32_on_device(test_z, train_dev.device, "test_z", "[n, d]", check_device_finite=True)
    models = _fit(train_dev, _codes_of(train_lbl, uleaves), len(uleaves), None, 1, logw, thr, dthr, LEAF_REG, who, uleaves)
    post = _scores(test_dev, models)
    label, prob, _, _ = N.leaf_merge(post, *N.merge_tables(lists), return_second=False)
    excluded = uleaves[models["counts"][0] <= thr]
    keep = np.invert(np.isin(test_lbl, excluded))
    label, prob = label.cpu().numpy().astype(np.int64)[:, keep], prob.cpu().numpy()[:, keep]
    pred = np.array([label_sets[t][label[t]] for t in range(len(levels))])
    kept_codes = _codes_of(test_lbl[keep], uleaves)
    true = np.array([_true_at(test_lbl[keep], kept_codes, at[t], list_changes, m) for t, m in enumerate(levels)])
    with np.errstate(invalid="ignore"):
        acc = np.array([np.mean(pred[t] == true[t]) if keep.any() else np.nan for t in range(len(levels))], dtype=np.float64)
    return {"levels": np.array(levels, dtype=np.int64), "n_classes": np.array([len(s) for s in label_sets], dtype=np.int64),
            "acc": acc, "pred": pred, "prob": prob, "true": true, "keep": keep, "n_excluded_cells": int(np.sum(~keep))}


def classify_tree_points(x_dev, y, list_changes, leaves, kfold, seed, levels=None, n_per_class_thr=6, diag_cov_n_sample_thr=12):
    """``merge_sweep`` under k-fold cross-validation on points already on the device: every cell is scored under the leaf
    models fitted to the folds it is not in (one ``mmvae_group_moments`` launch over the (leaf, fold) groups, one
    ``mmvae_gauss_scores`` launch with F = kfold models, one ``mmvae_leaf_merge``).  Returns ``n_classes`` [T], ``acc``
    [kfold, T] (over the fold's kept cells: those whose label is a leaf that has a model in their fold; NaN where a fold keeps
    none), ``pred`` [T, n] (labels), ``prob`` [T, n], ``keep`` [n], ``fold`` [n], ``levels``."""
    who = "classify_tree"
    y = np.asarray(y)
    n = int(x_dev.shape[0])
    if y.ndim != 1 or y.shape[0] != n:
        raise ValueError(f"{y.shape} labels for {n} samples")
    if int(kfold) != kfold or not 2 <= kfold <= n:
        raise ValueError(f"kfold = {kfold} outside [2, n = {n}]")
    if kfold > N.GAUSSCLF_MAX_F:
        raise NotImplementedError(f"{kfold} folds: at most {N.GAUSSCLF_MAX_F}")
    if not 1 <= int(x_dev.shape[1]) <= N.GAUSSCLF_MAX_D:
        raise NotImplementedError(f"d = {int(x_dev.shape[1])} outside [1, {N.GAUSSCLF_MAX_D}]")
    uleaves, logw = _leaf_refusals(who, leaves, None, n_per_class_thr)
    levels, label_sets, lists, at = _sweep_levels(who, uleaves, list_changes, levels)
    fold = kfold_of(n, int(kfold), seed)
    codes = _codes_of(y, uleaves)
    models = _fit(x_dev, codes, len(uleaves), fold, int(kfold), logw, n_per_class_thr, diag_cov_n_sample_thr, LEAF_REG, who, uleaves)
    post = _scores(x_dev, models, fold)
    label, prob, _, _ = N.leaf_merge(post, *N.merge_tables(lists), return_second=False)
    label, prob = label.cpu().numpy().astype(np.int64), prob.cpu().numpy()
    keep = (codes >= 0) & (models["counts"][fold, np.maximum(codes, 0)] > n_per_class_thr)
    pred = np.array([label_sets[t][label[t]] for t in range(len(levels))])
    acc = np.full((int(kfold), len(levels)), np.nan)
    for t, m in enumerate(levels):
        hit = pred[t] == _true_at(y, codes, at[t], list_changes, m)
        for f in range(int(kfold)):
            sel = keep & (fold == f)
            if sel.any():
                acc[f, t] = np.mean(hit[sel])
    return {"levels": np.array(levels, dtype=np.int64), "n_classes": np.array([len(s) for s in label_sets], dtype=np.int64),
            "acc": acc, "pred": pred, "prob": prob, "keep": keep, "fold": fold}

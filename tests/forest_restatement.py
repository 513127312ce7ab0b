"""Host restatement of the device random forest (numpy only), written from the contract's text in include/mmvae.h ("random
forest on 256-bin features") and DESIGN.md section 9i, not from the kernels.  Every tree it grows is the tree the device
grows, node for node and field for field; tests/test_gpu_forest.py holds the kernels to it.

The contract, in short.  bins uint8 [n, d], codes in [0, K), fold in [0, F); tree g = f T + t is trained on the rows whose fold
is not f, in ascending order (train_rows, n_f of them).
  Bins: per column, r = the rank of a value's first occurrence in the stably sorted column, bin = (r 256) // n.
  Randomness: Philox4x32-10, key = the two halves of the seed, counter (i, g, node, stream).  Stream 0 (node 0): call i gives
  the bootstrap draws 4 i .. 4 i + 3, row = train_rows[(u n_f) >> 32].  Stream 1: the feature order of node ``node``, a lazy
  Fisher-Yates: step s swaps position s with s + ((u (d - s)) >> 32), u = draw s (word s & 3 of call s >> 2).
  Nodes: node 0 the root; a split allocates its children at the next two indices, left then right; nodes leave a stack, right
  pushed before left.  A node is a leaf when one class holds all its rows, or when no feature has two occupied bins; its class
  is the arg-max of the class counts, the lowest code on ties.
  Split: features in the drawn order, stopping after mtry once a candidate has been seen.  A candidate is an occupied bin b_lo
  with a later occupied bin b_hi; score = double(sum_k L_k^2) / double(nL) + double(sum_k R_k^2) / double(nR); a strictly larger
  score wins.  thr = (b_lo + b_hi) >> 1; bin <= thr goes left.
  Prediction: one hard vote a tree; label = the arg-max of the votes, the lowest code on ties.
Node tables: int32 [count, 4] = (feature, thr, left child, rows) for a split, (-1, class, 0, rows) for a leaf."""
import numpy as np

_LO = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)
STREAM_BOOT, STREAM_FEAT = 0, 1


def philox(counter, seed):
    """uint32 [m, 4]: Philox4x32-10 of the counters [m, 4] (32-bit words) under key = (seed & 2^32 - 1, seed >> 32)."""
    c = np.asarray(counter).astype(np.uint64) & _LO
    c0, c1, c2, c3 = c[:, 0], c[:, 1], c[:, 2], c[:, 3]
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ np.uint64(k0), p1 & _LO, (p0 >> _S32) ^ c3 ^ np.uint64(k1), p0 & _LO
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], axis=1).astype(np.uint32)


def quantile_bins(x):
    """uint8 [n, d]: bin = (rank of the value's first occurrence in the stably sorted column * 256) // n."""
    x = np.asarray(x)
    if x.ndim != 2:
        raise ValueError(f"x of shape {x.shape} is not [n, d]")
    if not np.isfinite(x).all():
        raise ValueError("x contains NaN or infinity")
    n, d = x.shape
    out = np.empty((n, d), dtype=np.uint8)
    for j in range(d):
        order = np.argsort(x[:, j], kind="stable")
        v = x[order, j]
        first = np.arange(n, dtype=np.int64)
        first[1:][v[1:] == v[:-1]] = 0                  # (-0.0 == 0.0)
        first = np.maximum.accumulate(first)
        out[order, j] = (first * 256) // n
    return out


def default_mtry(d):
    return max(1, int(np.floor(np.sqrt(d))))


def train_rows(fold, f):
    return np.flatnonzero(np.asarray(fold) != f).astype(np.int64)


def bootstrap(rows, g, seed):
    """The n_f rows of tree g's sample, in drawing order."""
    nf = len(rows)
    calls = (nf + 3) // 4
    ctr = np.zeros((calls, 4), dtype=np.uint64)
    ctr[:, 0], ctr[:, 1], ctr[:, 3] = np.arange(calls), g, STREAM_BOOT
    u = philox(ctr, seed).reshape(-1)[:nf].astype(np.uint64)
    return rows[((u * np.uint64(nf)) >> _S32).astype(np.int64)]


class _FeatureDraws:
    """Draw s of node ``node`` of tree g, stream 1; a call serves every node of the tree at once and is kept."""

    def __init__(self, g, seed, n_nodes_max):
        self.g, self.seed, self.m, self.calls = g, seed, n_nodes_max, {}

    def draw(self, node, s):
        i = s >> 2
        if i not in self.calls:
            ctr = np.zeros((self.m, 4), dtype=np.uint64)
            ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3] = i, self.g, np.arange(self.m), STREAM_FEAT
            self.calls[i] = philox(ctr, self.seed)
        return int(self.calls[i][node, s & 3])


def feature_order(d, g, node, seed, steps=None):
    """The first ``steps`` (default d) features of node ``node`` of tree g in visiting order."""
    draws = _FeatureDraws(g, seed, node + 1)
    perm = list(range(d))
    steps = d if steps is None else steps
    for s in range(steps):
        j = s + ((draws.draw(node, s) * (d - s)) >> 32)
        perm[s], perm[j] = perm[j], perm[s]
    return perm[:steps]


def _best_of_feature(b, c_local, tot, kp):
    """(score, b_lo, b_hi) of the best candidate of one feature in a node, or None: b the rows' bins, c_local their class as
    an index into the node's kp present classes, tot their counts."""
    hist = np.bincount(c_local * 256 + b, minlength=kp * 256).reshape(kp, 256)
    cnt = hist.sum(axis=0)
    occ = np.flatnonzero(cnt)
    if len(occ) < 2:
        return None
    L = np.cumsum(hist[:, occ[:-1]], axis=1)            # the class counts at or below every candidate bin
    R = tot[:, None] - L
    nL = L.sum(axis=0)
    nR = int(tot.sum()) - nL
    score = (L * L).sum(axis=0).astype(np.float64) / nL.astype(np.float64) + \
            (R * R).sum(axis=0).astype(np.float64) / nR.astype(np.float64)
    a = int(np.argmax(score))                            # the first of the largest: the lowest b_lo
    return float(score[a]), int(occ[a]), int(occ[a + 1])


def grow(bins, codes, K, sample, g, mtry, seed, stats=None, midpoint=True):
    """The node table int32 [count, 4] of tree g grown on the rows ``sample`` (with multiplicity).  ``stats``: a dict that
    gathers, over the trees it is handed to, "depth" (the deepest node's), "visited" (the most features any node visited),
    "impure" (leaves of more than one class) and "tied" (those whose two largest classes are level).  ``midpoint=False`` is
    NOT the contract: thr = b_lo, kept so that tools/gen_golden_forest.py can record what the midpoint rule is worth."""
    d = bins.shape[1]
    draws = _FeatureDraws(g, seed, max(2 * len(sample) - 1, 1))
    nodes = [[-1, 0, 0, len(sample)]]
    stack = [(0, np.asarray(sample, dtype=np.int64), 0)]
    deepest = visited_max = impure = tied = 0
    while stack:
        node, rows, depth = stack.pop()
        deepest = max(deepest, depth)
        c = codes[rows]
        tot_all = np.bincount(c, minlength=K)
        present = np.flatnonzero(tot_all)
        nodes[node] = [-1, int(np.argmax(tot_all)), 0, len(rows)]
        if len(present) == 1:
            continue
        kp = len(present)
        c_local = np.searchsorted(present, c)
        tot = tot_all[present]
        perm = list(range(d))
        best = None
        for s in range(d):
            j = s + ((draws.draw(node, s) * (d - s)) >> 32)
            perm[s], perm[j] = perm[j], perm[s]
            f = perm[s]
            cand = _best_of_feature(bins[rows, f].astype(np.int64), c_local, tot, kp)
            if cand is not None and (best is None or cand[0] > best[0]):
                best = (cand[0], f, cand[1], cand[2])
            if s + 1 >= mtry and best is not None:
                break
        visited_max = max(visited_max, s + 1)
        if best is None:
            top = np.sort(tot)[::-1]
            impure, tied = impure + 1, tied + int(top[0] == top[1])
            continue
        _, f, b_lo, b_hi = best
        thr = (b_lo + b_hi) >> 1 if midpoint else b_lo
        left = len(nodes)
        nodes[node] = [f, thr, left, len(rows)]
        nodes.append(None)
        nodes.append(None)
        go_left = bins[rows, f] <= thr
        stack.append((left + 1, rows[~go_left], depth + 1))
        stack.append((left, rows[go_left], depth + 1))
    if stats is not None:
        stats["depth"], stats["visited"] = max(stats.get("depth", 0), deepest), max(stats.get("visited", 0), visited_max)
        stats["impure"], stats["tied"] = stats.get("impure", 0) + impure, stats.get("tied", 0) + tied
    return np.array(nodes, dtype=np.int32)


def predict_tree(nodes, bins):
    """int64 [m]: the class the tree votes for every row of ``bins``."""
    at = np.zeros(bins.shape[0], dtype=np.int64)
    rows = np.arange(bins.shape[0])
    while True:
        feat = nodes[at, 0]
        go = feat >= 0
        if not go.any():
            return nodes[at, 1].astype(np.int64)
        r = rows[go]
        left = bins[r, feat[go]] <= nodes[at[go], 1]
        at[r] = nodes[at[go], 2] + np.where(left, 0, 1)


def best_two(votes):
    """(label, best, second): the arg-max (lowest code on ties), its count and the largest count among the other classes."""
    label = np.argmax(votes, axis=1)
    best = votes[np.arange(len(votes)), label]
    rest = votes.copy()
    rest[np.arange(len(votes)), label] = -1
    return label.astype(np.int64), best, rest.max(axis=1)


def forest_cv(bins, codes, fold, K, F, T, mtry, seed, want_trees=True, stats=None, midpoint=True):
    """The cross-validated forest: dict of pred int64 [n], best / second int32 [n], votes int32 [n, K] and, with
    ``want_trees``, trees = {"count": int32 [F T], "nodes": list of int32 [count, 4]}.  ``stats``: as for ``grow``."""
    bins, codes, fold = np.asarray(bins), np.asarray(codes).astype(np.int64), np.asarray(fold).astype(np.int64)
    n = bins.shape[0]
    votes = np.zeros((n, K), dtype=np.int32)
    tables = []
    for f in range(F):
        tr = train_rows(fold, f)
        test = np.flatnonzero(fold == f)
        for t in range(T):
            g = f * T + t
            nodes = grow(bins, codes, K, bootstrap(tr, g, seed), g, mtry, seed, stats, midpoint)
            if want_trees:
                tables.append(nodes)
            if len(test):
                np.add.at(votes, (test, predict_tree(nodes, bins[test])), 1)
    label, best, second = best_two(votes)
    out = {"pred": label, "best": best.astype(np.int32), "second": second.astype(np.int32), "votes": votes, "fold": fold}
    if want_trees:
        out["trees"] = {"count": np.array([len(t) for t in tables], dtype=np.int32), "nodes": tables}
    return out


def fold_split(n, kfold, seed):
    """sklearn's KFold(n_splits=kfold, shuffle=True, random_state=seed): the fold whose test set holds every cell."""
    idx = np.arange(n)
    np.random.RandomState(seed).shuffle(idx)
    sizes = np.full(kfold, n // kfold, dtype=np.int64)
    sizes[:n % kfold] += 1
    fold = np.empty(n, dtype=np.int64)
    fold[idx] = np.repeat(np.arange(kfold), sizes)
    return fold


def cv_predict(x, labels, kfold, seed, n_trees=100, mtry=None, forest_seed=None, want_trees=False):
    """``forest_cv_predict`` of the package on the host: float32 rounding of x, bins, folds, forest."""
    x = np.asarray(x, dtype=np.float32)
    classes, codes = np.unique(np.asarray(labels), return_inverse=True)
    fold = fold_split(x.shape[0], kfold, seed)
    mtry = default_mtry(x.shape[1]) if mtry is None else mtry
    res = forest_cv(quantile_bins(x), codes.reshape(-1), fold, len(classes), kfold, n_trees, mtry,
                    seed if forest_seed is None else forest_seed, want_trees)
    res["classes"] = classes
    return res


def classifier(data, labels, kfold, seed, n_trees=100):
    """The reference's RF_classifier return, from the restated forest: (acc, ref_labels, pred_labels)."""
    acc, ref, pred = {}, {}, {}
    for key in labels:
        y = np.asarray(labels[key])
        res = cv_predict(data, y, kfold, seed, n_trees)
        acc[key], ref[key], pred[key] = [], [], []
        for f in range(kfold):
            test = np.flatnonzero(res["fold"] == f)
            p = res["classes"][res["pred"][test]]
            acc[key].append(float(np.average(y[test] == p)))
            pred[key].append(p)
            ref[key].append(y[test])
    return acc, ref, pred

"""numpy float64 / int64 restatement of the k-nearest-neighbour analysis (utils/neighbors.py, csrc/knn.hip): the neighbours
under the admission rule with ties by index, the votes with ties to the smallest label, purity, and the cross-validation
driver; the inputs the CPU and GPU tests share, and the gate of the float cases.

Gate (the issue's): gamma(d) = (d + 3) 2^-23 relative on a squared distance -- twice the first-order bound (d + 2) 2^-24 of
one rounded subtraction per coordinate and d rounded fma steps over non-negative addends.  A cell is UNAMBIGUOUS where its
(k+1)-th and k-th float64 squared distances (among the admitted references) differ by more than 2 gamma relative to the
larger: no fp32 evaluation inside the gate can then exchange a neighbour for a non-neighbour."""
import numpy as np


def gamma(d: int) -> float:
    return (d + 3) * 2.0 ** -23


def sqdist(q, r) -> np.ndarray:
    """float64 [nq, nr]: squared distances in difference form, coordinate by coordinate."""
    q = np.asarray(q, dtype=np.float64)
    r = np.asarray(r, dtype=np.float64)
    out = np.zeros((q.shape[0], r.shape[0]))
    for c in range(q.shape[1]):
        t = q[:, c, None] - r[None, :, c]
        out += t * t
    return out


def neighbors(q, r, k, qgroup=None, rgroup=None, d2=None):
    """(idx int64 [nq, k], dist2 float64 [nq, k], next float64 [nq]): the k admitted references of every query by rising
    (squared distance, index); -1 / +inf where fewer are admitted; ``next`` the (k+1)-th admitted squared distance (+inf
    where there is none).  Reference j is admitted for query i iff no groups are given or rgroup[j] != qgroup[i]."""
    d2 = sqdist(q, r) if d2 is None else d2
    nq, nr = d2.shape
    admitted = np.ones((nq, nr), dtype=bool) if qgroup is None else np.asarray(rgroup)[None, :] != np.asarray(qgroup)[:, None]
    masked = np.where(admitted, d2, np.inf)
    order = np.argsort(masked, axis=1, kind="stable")                    # ties by index; the inadmissible last
    count = admitted.sum(axis=1)
    kk = min(k + 1, nr)
    idx = np.full((nq, k + 1), -1, dtype=np.int64)
    dist2 = np.full((nq, k + 1), np.inf)
    idx[:, :kk] = order[:, :kk]
    dist2[:, :kk] = np.take_along_axis(masked, order[:, :kk], axis=1)
    tail = np.arange(k + 1)[None, :] >= count[:, None]
    idx[tail] = -1
    dist2[tail] = np.inf
    return idx[:, :k], dist2[:, :k], dist2[:, k]


def unambiguous(dist2, nxt, d: int) -> np.ndarray:
    """bool [nq]: the k-th and (k+1)-th squared distances differ by more than 2 gamma relative (or there is no (k+1)-th)."""
    kth = dist2[:, -1]
    with np.errstate(invalid="ignore"):
        return ~np.isfinite(nxt) | (nxt - kth > 2.0 * gamma(d) * nxt)


def votes(idx, rlabel, n_classes):
    """(pred int64 [nq], top2 int64 [nq, 2]): the label most valid (non-negative) neighbours carry, the smallest on ties, -1
    without one; the votes of it and the most votes of another label."""
    idx = np.asarray(idx)
    rlabel = np.asarray(rlabel)
    pred = np.full(idx.shape[0], -1, dtype=np.int64)
    top2 = np.zeros((idx.shape[0], 2), dtype=np.int64)
    for i, row in enumerate(idx):
        lab = rlabel[row[row >= 0]]
        if lab.size == 0:
            continue
        counts = np.bincount(lab, minlength=n_classes)
        pred[i] = int(np.argmax(counts))                                  # the first maximum: the smallest label
        top2[i, 0] = counts[pred[i]]
        counts[pred[i]] = 0
        top2[i, 1] = counts.max()
    return pred, top2


def purity(idx, rlabel, qlabel) -> np.ndarray:
    """float64 [nq]: valid neighbours with rlabel == qlabel[i] over valid neighbours; NaN without one."""
    idx = np.asarray(idx)
    valid = idx >= 0
    same = valid & (np.asarray(rlabel)[np.where(valid, idx, 0)] == np.asarray(qlabel)[:, None])
    with np.errstate(invalid="ignore", divide="ignore"):
        return same.sum(axis=1).astype(np.float64) / valid.sum(axis=1).astype(np.float64)


def kfold_of(n, kfold, seed) -> np.ndarray:
    """sklearn's KFold(n_splits=kfold, shuffle=True, random_state=seed): the fold whose test set holds every cell."""
    idx = np.arange(n)
    np.random.RandomState(seed).shuffle(idx)
    sizes = np.full(kfold, n // kfold, dtype=np.int64)
    sizes[:n % kfold] += 1
    fold = np.empty(n, dtype=np.int64)
    fold[idx] = np.repeat(np.arange(kfold), sizes)
    return fold


def cv_predict(x, labels, kfold, seed, k, d2=None) -> dict:
    """The cross-validation driver: every cell voted on by its k nearest cells of the other folds."""
    x = np.asarray(x, dtype=np.float64)
    classes, codes = np.unique(np.asarray(labels), return_inverse=True)
    codes = codes.reshape(-1)
    fold = kfold_of(x.shape[0], kfold, seed)
    idx, dist2, nxt = neighbors(x, x, k, fold, fold, d2=d2)
    pred, top2 = votes(idx, codes, len(classes))
    return {"pred": pred, "top2": top2, "fold": fold, "classes": classes, "codes": codes, "idx": idx, "dist2": dist2,
            "purity": purity(idx, codes, codes), "sure": unambiguous(dist2, nxt, x.shape[1])}


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def lattice(n, d, seed) -> np.ndarray:
    """float32 [n, d], integers in [-8, 8]: every squared distance an integer <= 128 * 256 < 2^24, exact in float32."""
    return np.random.default_rng(seed).integers(-8, 9, size=(n, d)).astype(np.float32)


# name: (n, d, k, centres)
FLOAT_CASES = {"n3000_d10_k15": (3000, 10, 15, 20), "n3000_d2_k5": (3000, 2, 5, 12), "n2000_d12_k30": (2000, 12, 30, 40),
               "n1000_d128_k15": (1000, 128, 15, 0)}


def mixture(name):
    """(x float32 [n, d], labels int64 [n] the centre of every point (zeros without centres), k)."""
    n, d, k, centres = FLOAT_CASES[name]
    rng = np.random.default_rng(1000 + sorted(FLOAT_CASES).index(name))
    if centres == 0:
        return rng.standard_normal((n, d)).astype(np.float32), np.zeros(n, dtype=np.int64), k
    mu = (3.0 * rng.standard_normal((centres, d))).astype(np.float32)
    labels = rng.integers(0, centres, n)
    x = mu[labels] + rng.standard_normal((n, d)).astype(np.float32)
    return x.astype(np.float32), labels.astype(np.int64), k

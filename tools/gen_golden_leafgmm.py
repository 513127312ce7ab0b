"""Build container only (scipy and the reference are present there): record what the reference's ``predict_leaf_gmm``,
``custom_QDA``, ``get_merge_sequence``, ``do_merges``, ``get_descendants`` and ``get_ancestors`` compute, as the data-only fixture
tests/golden/leafgmm_kat.npz (tests/test_leafgmm_cpu.py, tests/test_gpu_leafgmm.py).

The functions are the reference's own (mmidas/utils/analysis_tree_helpers.py).  The module does not import (feather and
seaborn are missing), so the needed functions are compiled in memory from the file where it lies (``ast``); ``source`` records
that and the scipy version.  Nothing of the reference is copied into the repository.

per case k (``cases``: n_train, n_test, d, L; ``kinds`` the cases' names):
  c<k>/train_z, /test_z          float32 points on a 1/4096 grid (the simplex case: float32 probabilities), passed as float64
  c<k>/train_lbl, /test_lbl      the leaf labels, unicode strings
  c<k>/leaves                    the leaf names;  c<k>/weight  float64 [L] or empty: label_weight
  c<k>/tree/child, /parent, /y   the synthetic dendrogram, rows sorted by height (leaves: height 0; the root's parent: '')
  c<k>/changes                   json: the reference's get_merge_sequence(child, parent, y)
  c<k>/descendants, /leafonly    json: the reference's get_descendants of every internal node (leafonly: sorted)
  c<k>/ancestors                 json: the reference's get_ancestors of every leaf
  c<k>/merged/<m>                the reference's do_merges(leaves, changes, m), m in c<k>/levels
  c<k>/levels                    the numbers of merges recorded; a last entry -1 is the case's hand-made label set (nested
                                 labels, a label with neither a leaf nor descendants)
and per recorded level m:
  c<k>/m<m>/dataset              unique_dataset_lbl;  c<k>/m<m>/desc  json: descendant_dict
  c<k>/m<m>/true, /pred          the reference's first two returns
  c<k>/m<m>/counts               int64 [3]: n_excluded_cells, n_classes_predicted, n_classes_removed
  c<k>/m<m>/prob                 float64: pred_probability
  c<k>/m<m>/nan_rows             int64: the kept rows whose reference probability is NaN (not zero only in the 'far' case)
  c<k>/e_ref                     max |pred_probability - tests/leafgmm_restatement.py| over all levels (NaN rows apart)
  c<k>/min_margin                the restatement's smallest best - second merged probability over all levels and kept cells
  c<k>/leaf_acc                  the reference's accuracy at level 0
  c<k>/m<m>/far_pred, /far_prob  the 'far' case: what the restatement gives on the nan_rows
  qda/...                        custom_QDA: train_z, test_z, train_lbl, test_lbl (the test labels passed as a list, the only
                                 way the reference's function runs; no excluded class), true, pred, min_margin
A case is refused when the reference has a NaN row (the 'far' case apart, which must have some), when a smallest margin is
below 1e-6, or when the restatement disagrees with the reference on a prediction, a count or a label; the whole set is refused
unless at least half the cases have a leaf-level accuracy strictly between 0.5 and 0.99.

    python -m tools.gen_golden_leafgmm
"""
import ast
import json
import os
import sys
import warnings

import numpy as np

from oracle import ref_loader as RL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import leafgmm_restatement as LR  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
_FILE = os.path.join(RL.REFERENCE_ROOT, "mmidas", "utils", "analysis_tree_helpers.py")
NAMES = ("get_descendants", "get_ancestors", "get_merge_sequence", "do_merges", "custom_QDA", "predict_leaf_gmm")
# (name, n_train, n_test, d, L, spread of the means, levels recorded (None: all))
CASES = (("plain12", 700, 250, 12, 6, 1.1, None),
         ("weights10", 900, 300, 10, 12, 1.0, (0, 1, 4, 8, 10)),
         ("nested2", 500, 200, 2, 8, 2.6, (0, 3, 6)),
         ("simplex10", 800, 250, 10, 8, 1.6, (0, 2, 5, 6)),
         ("wide2", 1500, 400, 2, 40, 7.0, (0, 1, 7, 20, 33, 37)),
         ("far10", 500, 200, 10, 6, 1.2, (0, 2, 4)))
GRID = 4096.0
MIN_MARGIN = 1e-6
SMALL, DIAG = 5, 9                       # training cells of the leaf without a model and of the diagonal leaf


def load_reference():
    import scipy
    with open(_FILE, "r") as fh:
        tree = ast.parse(fh.read(), filename=_FILE)
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in NAMES]
    assert len(keep) == len(NAMES)
    ns = {"np": np}
    exec(compile(ast.Module(body=keep, type_ignores=[]), _FILE, "exec"), ns)
    return ns, f"functions compiled from the reference file; scipy {scipy.__version__}, numpy {np.__version__}"


def make_tree(rng, leaves):
    """(child, parent, y) of a random dendrogram over ``leaves``: binary merges and one node with three children, strictly
    rising heights but for one pair of equal ones; internal nodes 'n<i>', the root 'n1'; rows sorted by height."""
    tops = list(leaves)
    merges = []
    triple_at = len(leaves) // 2
    while len(tops) > 1:
        take = 3 if len(tops) == triple_at and len(tops) >= 3 else 2
        pick = sorted(rng.choice(len(tops), size=take, replace=False).tolist(), reverse=True)
        merges.append([tops.pop(i) for i in pick][::-1])
        tops.append(f"#{len(merges) - 1}")                         # named below, once the number of nodes is known
    M = len(merges)
    name = {f"#{i}": f"n{M - i}" for i in range(M)}
    heights = np.cumsum(rng.uniform(0.02, 0.1, size=M))
    if M > 3:
        heights[2] = heights[1]                                    # equal heights: np.nanargmin takes the first
    child, parent, y = list(leaves), [None] * len(leaves), [0.0] * len(leaves)
    for i, kids in enumerate(merges):
        child.append(name[f"#{i}"])
        parent.append(None)
        y.append(float(heights[i]))
    for i, kids in enumerate(merges):
        for c in kids:
            parent[child.index(name.get(c, c))] = name[f"#{i}"]
    parent = ["" if p is None else p for p in parent]
    return np.array(child), np.array(parent), np.array(y)


def make_points(rng, kind, n_train, n_test, d, L, spread, leaves):
    """(train_z, train_lbl, test_z, test_lbl): a mixture of L Gaussians with their own covariances, close enough to overlap;
    leaf 1 has SMALL training cells (no model), leaf 2 DIAG (the diagonal branch); leaves 3 and 4 lie almost on each other."""
    means = rng.normal(size=(L, d)) * spread
    means[4] = means[3] + 0.3 * rng.normal(size=d)
    A = [rng.normal(size=(d, d)) * 0.35 + np.eye(d) * rng.uniform(0.6, 1.1) for _ in range(L)]
    A[4] = A[3]

    def draw(n, sizes_fixed):
        w = rng.uniform(0.5, 1.5, size=L)
        sizes = np.maximum(2 * d + 14, np.floor(n * w / w.sum()).astype(np.int64))
        for leaf, s in sizes_fixed.items():
            sizes[leaf] = s
        codes = rng.permutation(np.repeat(np.arange(L), sizes))
        x = np.empty((len(codes), d))
        for k in range(L):
            x[codes == k] = means[k] + rng.normal(size=(int(sizes[k]), d)) @ A[k].T
        return x, codes

    tr, ctr = draw(n_train, {1: SMALL, 2: DIAG})
    te, cte = draw(n_test, {1: 4, 2: 6})
    if kind == "far10":
        te[:7] += 400.0                                             # no leaf's density is above zero there
    if kind == "simplex10":
        def simplex(x):
            z = np.exp(0.7 * x - (0.7 * x).max(axis=1, keepdims=True))
            return (z / z.sum(axis=1, keepdims=True)).astype(np.float32)
        tr, te = simplex(tr), simplex(te)
    else:
        tr, te = ((np.round(x * GRID) / GRID).astype(np.float32) for x in (tr, te))
    return tr, leaves[ctr], te, leaves[cte]


def desc_at(changes, m):
    below, alive = {}, {}
    for kids, node, _ in changes[:m]:
        below[node] = [g for c in kids for g in [c] + below.get(c, [])]
        for c in kids:
            alive.pop(c, None)
        alive[node] = below[node]
    return alive


def main():
    ref, source = load_reference()
    rng = np.random.default_rng(20259)
    out = {"cases": np.array([c[1:5] for c in CASES], dtype=np.int64), "kinds": np.array([c[0] for c in CASES]),
           "source": np.array(source)}
    in_band = 0
    for k, (kind, n_train, n_test, d, L, spread, levels) in enumerate(CASES):
        leaves = np.array([f"L{i:02d}" for i in range(L)])
        child, parent, y = make_tree(rng, leaves)
        tr, ltr, te, lte = make_points(rng, kind, n_train, n_test, d, L, spread, leaves)
        weight = rng.uniform(0.5, 2.0, size=L) if kind == "weights10" else np.zeros(0)
        tr64, te64 = tr.astype(np.float64), te.astype(np.float64)
        changes = ref["get_merge_sequence"](child.copy(), parent.copy(), y.copy())
        mine = LR.get_merge_sequence(child, parent, y)
        if json.dumps(changes) != json.dumps(mine):
            raise SystemExit(f"case {k}: the restated merge sequence is not the reference's")
        internal = [c for c in child if c not in leaves]
        desc_all = {p: ref["get_descendants"](child, parent, y, p) for p in internal}
        leafonly = {p: sorted(ref["get_descendants"](child, parent, y, p, leafonly=True)) for p in internal}
        anc = {str(leaf): [str(a) for a in ref["get_ancestors"](leaf, child, parent)] for leaf in leaves}
        levels = list(range(len(changes))) if levels is None else list(levels)
        base = f"c{k}"
        out.update({f"{base}/train_z": tr, f"{base}/test_z": te, f"{base}/train_lbl": ltr, f"{base}/test_lbl": lte,
                    f"{base}/leaves": leaves, f"{base}/weight": weight, f"{base}/tree/child": child, f"{base}/tree/parent": parent,
                    f"{base}/tree/y": y, f"{base}/changes": np.array(json.dumps(changes)),
                    f"{base}/descendants": np.array(json.dumps(desc_all)), f"{base}/leafonly": np.array(json.dumps(leafonly)),
                    f"{base}/ancestors": np.array(json.dumps(anc))})
        sets = []
        for m in levels:
            merged = ref["do_merges"](leaves.copy(), changes, m)
            out[f"{base}/merged/{m}"] = merged
            sets.append((m, np.unique(merged), desc_at(changes, m)))
        if kind == "nested2":                                      # leaf 3 beside a node that holds it, and a label without leaves
            sets.append((-1, np.array(leaves.tolist() + ["X34", "ghost"]), {"X34": ["L03", "L04"], "ghost": []}))
        out[f"{base}/levels"] = np.array([s[0] for s in sets], dtype=np.int64)
        e_ref, margin, leaf_acc = 0.0, np.inf, None
        for m, dataset, desc in sets:
            kw = dict(n_per_class_thr=6, diag_cov_n_sample_thr=12, unique_dataset_lbl=dataset.tolist(),
                      unique_leaf_lbl=leaves.tolist(), descendant_dict=desc, label_weight=weight.tolist())
            with warnings.catch_warnings(), np.errstate(invalid="ignore", divide="ignore"):
                warnings.simplefilter("ignore")
                true, pred, n_exc, n_pred, n_rem, prob = ref["predict_leaf_gmm"](tr64, ltr.copy(), te64, lte.copy(), **kw)
            res = LR.predict_leaf_gmm(tr64, ltr, te64, lte, 6, 12, dataset, leaves, desc, weight if len(weight) else None)
            nan_rows = np.flatnonzero(np.isnan(prob))
            if (kind == "far10") != (len(nan_rows) > 0):
                raise SystemExit(f"case {k} level {m}: {len(nan_rows)} NaN rows in the reference")
            ok = ~np.isnan(prob)
            if (n_exc, n_pred, n_rem) != (res["n_excluded"], res["n_predicted"], res["n_removed"]):
                raise SystemExit(f"case {k} level {m}: the counts differ")
            if not np.array_equal(true, res["true"]) or not np.array_equal(pred[ok], res["pred"][ok]):
                raise SystemExit(f"case {k} level {m}: {int((pred[ok] != res['pred'][ok]).sum())} predictions differ")
            if not np.isfinite(res["prob"]).all():
                raise SystemExit(f"case {k} level {m}: the restatement is not finite")
            e_ref = max(e_ref, float(np.abs(prob[ok] - res["prob"][ok]).max()))
            if len(dataset) > 1:
                margin = min(margin, float((res["prob"] - res["second"]).min()))
            if m == 0:
                leaf_acc = float(np.mean(true == pred))
            out.update({f"{base}/m{m}/dataset": dataset, f"{base}/m{m}/desc": np.array(json.dumps(desc)), f"{base}/m{m}/true": true,
                        f"{base}/m{m}/pred": pred, f"{base}/m{m}/counts": np.array([n_exc, n_pred, n_rem], dtype=np.int64),
                        f"{base}/m{m}/prob": prob, f"{base}/m{m}/nan_rows": nan_rows.astype(np.int64)})
            if kind == "far10":
                out[f"{base}/m{m}/far_pred"], out[f"{base}/m{m}/far_prob"] = res["pred"][nan_rows], res["prob"][nan_rows]
        if margin < MIN_MARGIN:
            raise SystemExit(f"case {k}: smallest margin {margin:.2e} below {MIN_MARGIN}")
        in_band += 0.5 < leaf_acc < 0.99
        out.update({f"{base}/e_ref": np.float64(e_ref), f"{base}/min_margin": np.float64(margin), f"{base}/leaf_acc": np.float64(leaf_acc)})
        print(f"case {k} {kind} (n {n_train}/{n_test}, d {d}, L {L}): {len(changes)} merges, levels {[s[0] for s in sets]}, "
              f"leaf accuracy {leaf_acc:.3f}, e_ref {e_ref:.2e}, smallest margin {margin:.2e}")
    if 2 * in_band < len(CASES):
        raise SystemExit(f"only {in_band} of {len(CASES)} cases have a leaf accuracy in (0.5, 0.99)")
    # custom_QDA: list labels and no excluded class, the only way the reference's function runs
    leaves = np.array([f"Q{i}" for i in range(5)])
    tr, ltr, te, lte = make_points(rng, "qda", 400, 150, 3, 5, 1.6, leaves)
    big = ~np.isin(ltr, leaves[[1]])
    tr, ltr = tr[big], ltr[big]                                      # leaf 1 would be excluded: leave it out of both sets;
    te, lte = te[lte != leaves[1]], lte[lte != leaves[1]]            # leaf 2 keeps DIAG cells: the diagonal branch
    true, pred = ref["custom_QDA"](tr.astype(np.float64), ltr, te.astype(np.float64), lte.tolist())
    mt, mp, sc = LR.custom_qda(tr.astype(np.float64), ltr, te.astype(np.float64), lte)
    srt = np.sort(sc, axis=1)
    margin = float((srt[:, -1] - srt[:, -2]).min())
    if not np.array_equal(np.asarray(pred), mp) or not np.array_equal(np.asarray(true), mt) or margin < MIN_MARGIN:
        raise SystemExit(f"custom_QDA: the restatement disagrees, or the margin {margin:.2e} is too small")
    out.update({"qda/train_z": tr, "qda/test_z": te, "qda/train_lbl": ltr, "qda/test_lbl": lte, "qda/true": np.asarray(true),
                "qda/pred": np.asarray(pred), "qda/min_margin": np.float64(margin)})
    print(f"custom_QDA: accuracy {float(np.mean(np.asarray(true) == np.asarray(pred))):.3f}, smallest score margin {margin:.2e}")
    print(source)
    path = os.path.join(GOLDEN, "leafgmm_kat.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

"""Build container only (sklearn and the reference are present there): record what the reference's ``QDA_classifier`` and
``LDA_classifier`` compute, as the data-only fixture tests/golden/gaussclf_kat.npz (tests/test_gaussclf_cpu.py,
tests/test_gpu_gaussclf.py).

The two functions are the reference's own (mmidas/utils/cluster_analysis.py): the module is imported where that works; where
one of its imports is missing the two functions are compiled in memory from the file where it lies (``ast``) with the
installed sklearn names; ``source`` records which.  Nothing of the reference is copied into the repository.  sklearn's
``decision_function`` of every fold is recorded by a loop of this file's own over the same ``KFold``.

per case k (``cases``: n, d, kfold, seed; ``c<k>/keys`` the label sets' names): float32 points passed to sklearn as float64
  c<k>/x                         float32 [n, d]
  c<k>/y/<key>                   the labels (int64, or unicode strings)
and per classifier clf in (qda, lda) and label set:
  c<k>/<clf>/<key>/acc           float64 [kfold]          the reference's accuracies
  c<k>/<clf>/<key>/ref, /pred    the reference's ref_labels and pred_labels, the folds' lists concatenated in fold order
  c<k>/<clf>/<key>/sizes         int64 [kfold]            the folds' test-set sizes
  c<k>/<clf>/<key>/rows          int64 [m]                the cells whose decision_function row is recorded (every
                                 ceil(n K / 4000)-th, to keep the file small)
  c<k>/<clf>/<key>/dec           float64 [m, K]           sklearn's decision_function of those cells under their fold's model
  c<k>/<clf>/<key>/e_ref         max |dec - tests/gaussclf_restatement.py scores| over those rows (LDA: after each row's
                                 maximum is taken off both, see the restatement's docstring)
  c<k>/<clf>/<key>/min_margin    the restatement's smallest best - second over all cells
A case is refused when a smallest margin is below 1e-6, when a QDA training class has at most d cells, when the restatement
disagrees with sklearn on a prediction or a fold, or when a class is absent from a training set.

    python -m tools.gen_golden_gaussclf
"""
import ast
import importlib.util
import os
import sys
import warnings

import numpy as np

from oracle import ref_loader as RL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gaussclf_restatement as GR  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
_FILE = os.path.join(RL.REFERENCE_ROOT, "mmidas", "utils", "cluster_analysis.py")
# (n, d, kfold, seed, kind of data, {label set: K})
CASES = ((600, 2, 5, 0, "plain", {"T": 6}),
         (800, 10, 4, 3, "simplex", {"T": 8}),
         (700, 12, 3, 11, "strings", {"T": 6}),
         (900, 10, 10, 1, "plain", {"T": 7, "merged": 5}),
         (3000, 2, 10, 7, "plain", {"T": 40}),
         (1000, 12, 5, 2, "plain", {"T": 10}))
GRID = 4096.0
MIN_MARGIN = 1e-6


def load_reference():
    import sklearn
    try:
        spec = importlib.util.spec_from_file_location("_ref_cluster_analysis", _FILE)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod.QDA_classifier, mod.LDA_classifier, f"module imported; sklearn {sklearn.__version__}"
    except ImportError as e:
        from sklearn.discriminant_analysis import LinearDiscriminantAnalysis, QuadraticDiscriminantAnalysis
        from sklearn.metrics import accuracy_score
        from sklearn.model_selection import KFold
        with open(_FILE, "r") as fh:
            tree = ast.parse(fh.read(), filename=_FILE)
        keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in ("QDA_classifier", "LDA_classifier")]
        assert len(keep) == 2
        ns = {"np": np, "KFold": KFold, "accuracy_score": accuracy_score, "LinearDiscriminantAnalysis": LinearDiscriminantAnalysis,
              "QuadraticDiscriminantAnalysis": QuadraticDiscriminantAnalysis}
        exec(compile(ast.Module(body=keep, type_ignores=[]), _FILE, "exec"), ns)
        return ns["QDA_classifier"], ns["LDA_classifier"], f"functions compiled from the reference file ({e}); sklearn {sklearn.__version__}"


def make_case(rng, n, d, kind, sets):
    """(x float32 [n, d], {key: labels}): a mixture of K Gaussians with their own covariances, close enough to overlap."""
    K = sets["T"]
    weights = rng.uniform(0.5, 1.5, size=K)
    floor = 2 * d + 8                                                           # every class keeps more than d training cells
    sizes = floor + np.floor((n - K * floor) * weights / weights.sum()).astype(np.int64)
    sizes[0] += n - sizes.sum()
    codes = rng.permutation(np.repeat(np.arange(K), sizes))
    means = rng.normal(size=(K, d)) * (2.2 if d > 2 else 4.0)
    x = np.empty((n, d))
    for k in range(K):
        A = rng.normal(size=(d, d)) * 0.45 + np.eye(d) * rng.uniform(0.5, 1.2)
        x[codes == k] = means[k] + rng.normal(size=(int(sizes[k]), d)) @ A.T
    if kind == "simplex":
        z = np.exp(0.7 * x - (0.7 * x).max(axis=1, keepdims=True))
        x = (z / z.sum(axis=1, keepdims=True)).astype(np.float32)                 # probabilities: a singular covariance
    else:
        x = (np.round(x * GRID) / GRID).astype(np.float32)
    labels = {}
    for key, Kk in sets.items():
        c = codes if Kk == K else codes % Kk                                      # a coarser label set: classes merged
        if kind == "strings":
            labels[key] = np.array([f"type_{v:02d}" for v in c])
        else:
            labels[key] = (c * 3 + 1).astype(np.int64)                            # label values that are not the codes
    return x, labels


def sklearn_decisions(x64, y, kfold, seed, kind):
    """(decision_function of every cell under its own fold's model [n, K], fold [n], prediction [n])."""
    from sklearn.discriminant_analysis import LinearDiscriminantAnalysis, QuadraticDiscriminantAnalysis
    from sklearn.model_selection import KFold
    classes = np.unique(y)
    dec, fold, pred = np.zeros((len(y), len(classes))), np.zeros(len(y), dtype=np.int64), np.empty(len(y), dtype=y.dtype)
    for f, (tr, te) in enumerate(KFold(n_splits=kfold, random_state=seed, shuffle=True).split(x64)):
        m = QuadraticDiscriminantAnalysis(reg_param=1e-2) if kind == "qda" else LinearDiscriminantAnalysis()
        m.fit(x64[tr], y[tr])
        if len(m.classes_) != len(classes):
            raise SystemExit(f"a class is absent from the training set of fold {f}")
        dec[te], fold[te], pred[te] = m.decision_function(x64[te]), f, m.predict(x64[te])
    return dec, fold, pred


def main():
    qda_ref, lda_ref, source = load_reference()
    rng = np.random.default_rng(20252)
    out = {"cases": np.array([c[:4] for c in CASES], dtype=np.int64), "source": np.array(source)}
    for k, (n, d, kfold, seed, kind, sets) in enumerate(CASES):
        x, labels = make_case(rng, n, d, kind, sets)
        x64 = x.astype(np.float64)
        out[f"c{k}/x"] = x
        out[f"c{k}/keys"] = np.array(list(labels))
        for key in labels:
            out[f"c{k}/y/{key}"] = labels[key]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                                     # sklearn warns of collinear variables (simplex)
            returns = {"qda": qda_ref(x64, labels, kfold, seed), "lda": lda_ref(x64, labels, kfold, seed)}
            for clf, (acc, ref, pred) in returns.items():
                for key, y in labels.items():
                    res = GR.cv_predict(x64, y, kfold, seed, clf)
                    K = len(res["classes"])
                    if clf == "qda" and (res["counts"] <= d).any():
                        raise SystemExit(f"case {k} {key}: a QDA training class has at most d = {d} cells")
                    dec, fold, sk_pred = sklearn_decisions(x64, y, kfold, seed, clf)
                    margin = float((res["best"] - res["second"]).min())
                    if margin < MIN_MARGIN:
                        raise SystemExit(f"case {k} {clf} {key}: smallest margin {margin:.2e} below {MIN_MARGIN}")
                    if not np.array_equal(fold, res["fold"]):
                        raise SystemExit(f"case {k}: the restated folds are not sklearn's")
                    wrong = int((res["classes"][res["pred"]] != sk_pred).sum())
                    if wrong or not np.array_equal(np.concatenate(pred[key]), np.concatenate(
                            [sk_pred[fold == f] for f in range(kfold)])):
                        raise SystemExit(f"case {k} {clf} {key}: {wrong} predictions differ from sklearn's")
                    rows = np.arange(0, n, -(-n * K // 4000))
                    mine, theirs = res["scores"][rows], dec[rows]
                    if clf == "lda":
                        mine, theirs = mine - mine.max(axis=1, keepdims=True), theirs - theirs.max(axis=1, keepdims=True)
                    e_ref = float(np.abs(mine - theirs).max())
                    base = f"c{k}/{clf}/{key}"
                    out.update({f"{base}/acc": np.array(acc[key], dtype=np.float64), f"{base}/ref": np.concatenate(ref[key]),
                                f"{base}/pred": np.concatenate(pred[key]),
                                f"{base}/sizes": np.array([len(p) for p in pred[key]], dtype=np.int64), f"{base}/rows": rows,
                                f"{base}/dec": dec[rows], f"{base}/e_ref": np.float64(e_ref),
                                f"{base}/min_margin": np.float64(margin)})
                    print(f"case {k} {(n, d, kfold, seed, kind)} {clf} {key}: K {K}, accuracy {np.mean(acc[key]):.3f}, "
                          f"disagreements with sklearn {wrong}, e_ref {e_ref:.2e}, smallest margin {margin:.2e}, "
                          f"smallest training class {int(res['counts'][res['counts'] > 0].min())}")
    print(source)
    path = os.path.join(GOLDEN, "gaussclf_kat.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

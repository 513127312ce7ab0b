"""Build container only (sklearn is present there): record the accuracy of sklearn's random forest under k-fold
cross-validation, as the data-only fixture tests/golden/forest_kat.npz (tests/test_forest_cpu.py, tests/test_gpu_forest.py).

The reference's ``RF_classifier`` (mmidas/utils/cluster_analysis.py) runs ``RandomForestClassifier()`` on every fold of
``KFold(n_splits=kfold, shuffle=True, random_state=seed)`` and draws the forest from numpy's global state, so its own numbers
are not reproducible; what can be recorded is the distribution of its accuracy.  Per case this file runs
``RandomForestClassifier(n_estimators=100, random_state=s)`` for the SEEDS forest seeds s on the same folds.

``cases``: int64 [m, 4] = n, d, kfold, seed; ``seeds`` int64 [8]; ``sklearn`` the version; and per case k
  c<k>/x        float32 [n, d]      the points (sklearn is handed their float64 copy)
  c<k>/y        int64 [n]           the labels
  c<k>/acc      float64 [8, kfold]  sklearn's accuracy of every forest seed and fold
  c<k>/raw_bins float64 [2]         sklearn's mean accuracy (forest seed 0) on x, and on x replaced by its 256 rank bins:
                                    what the quantisation alone costs
  c1/thr_rule   float64 [2]         the restated forest's mean accuracy (tests/forest_restatement.py, 100 trees, forest seed =
                                    the case's seed) with thr = b_lo, which is not the contract, and with the midpoint, which is

    python -m tools.gen_golden_forest [another path for the file]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import forest_restatement as FR  # noqa: E402
import gaussclf_inputs as GI  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
# (n, d, K, spread, kfold, seed)
CASES = ((3000, 10, 40, 3.0, 3, 0), (3000, 10, 40, 1.0, 3, 1), (2000, 2, 20, 1.5, 3, 2), (2760, 10, 92, 2.0, 3, 3))
SEEDS = tuple(range(8))
THR_CASE = 1                    # the case on which the threshold rule's worth is recorded


def sklearn_acc(x, y, kfold, seed, forest_seed):
    from sklearn.ensemble import RandomForestClassifier
    from sklearn.model_selection import KFold
    acc = []
    for train, test in KFold(n_splits=kfold, shuffle=True, random_state=seed).split(x):
        clf = RandomForestClassifier(n_estimators=100, random_state=forest_seed).fit(x[train], y[train])
        acc.append(float(np.mean(clf.predict(x[test]) == y[test])))
    return acc


def main():
    import sklearn
    out = {"cases": np.array([(n, d, kfold, seed) for n, d, _, _, kfold, seed in CASES], dtype=np.int64),
           "seeds": np.array(SEEDS, dtype=np.int64), "sklearn": np.array(sklearn.__version__)}
    for k, (n, d, K, spread, kfold, seed) in enumerate(CASES):
        x, y = GI.points(n, d, K, spread=spread)
        x64 = x.astype(np.float64)
        acc = np.array([sklearn_acc(x64, y, kfold, seed, s) for s in SEEDS])
        binned = FR.quantile_bins(x).astype(np.float64)
        raw_bins = np.array([acc[0].mean(), np.mean(sklearn_acc(binned, y, kfold, seed, SEEDS[0]))])
        m = acc.mean(axis=1)
        print(f"c{k}: n {n} d {d} K {K} spread {spread}: sklearn mean {m.mean():.4f} sd over seeds {m.std(ddof=1):.4f} "
              f"range {m.min():.4f} .. {m.max():.4f}; on bins {raw_bins[1]:.4f} against {raw_bins[0]:.4f}", flush=True)
        out[f"c{k}/x"], out[f"c{k}/y"], out[f"c{k}/acc"], out[f"c{k}/raw_bins"] = np.array(x), np.array(y), acc, raw_bins
        if k == THR_CASE:
            fold = FR.fold_split(n, kfold, seed)
            rule = []
            for midpoint in (False, True):
                res = FR.forest_cv(binned.astype(np.uint8), y, fold, K, kfold, 100, FR.default_mtry(d), seed, want_trees=False,
                                   midpoint=midpoint)
                rule.append(np.mean([np.mean(res["pred"][fold == f] == y[fold == f]) for f in range(kfold)]))
            out[f"c{k}/thr_rule"] = np.array(rule)
            print(f"c{k}: restated forest with thr = b_lo {rule[0]:.4f}, with the midpoint {rule[1]:.4f}", flush=True)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(GOLDEN, "forest_kat.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

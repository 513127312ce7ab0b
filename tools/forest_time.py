"""Timing of the random forest at the SmartSeq size: n = 22 365 cells, K = 92 and 115 types of uneven sizes (at least 30 cells
each), kfold = 10, 100 trees a fold, for d = 2 (state), 10 (x_low) and 100 (PCs), on a synthetic mixture of K Gaussians.

per (K, d):
  * the HIP-event median of ``mmvae_forest_cv`` on bins already on the device (the training-row launch and, per chunk of trees,
    one fit and one predict launch), the workspace bytes and the trees' sizes;
  * ``quantile_bins`` (``torch.sort`` and the rank arithmetic), HIP events;
  * ``RF_classifier`` end to end from host arrays, wall clock;
  * for K = 92, d = 10 and where sklearn is importable: the reference's loop (``KFold`` x fit / predict of sklearn's
    ``RandomForestClassifier``) on the same host, run once, with ``n_jobs=1`` and ``n_jobs=16``, and both accuracies.
The fit and predict launches are timed apart by a kernel trace of a run of its own:
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/forest_time.py --launches-only
    python tools/forest_time.py --merge-trace DIR [--out profiles/forest_time.json]
(``--launches-only`` makes exactly ``TRACE_CALLS`` calls a shape and nothing else on the device, so the trace's launches are
attributed by counting ``k_rf_train_rows``.)  ``--launches-only --shape 92,10`` is the single shape for a counter run.

    python tools/forest_time.py [--repeats R] [--out profiles/forest_time.json] [--no-sklearn]
"""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import distributed_vae_amd  # noqa: F401,E402
from distributed_vae_amd import _native as N  # noqa: E402
from distributed_vae_amd.utils import cluster_analysis as CA  # noqa: E402

NC, KFOLD, SEED, TREES = 22365, 10, 0, 100
SHAPES = [(K, d) for K in (92, 115) for d in (2, 10, 100)]
TRACE_CALLS = 3


def data(K, d):
    rng = np.random.default_rng(546 + 1000 * K + d)
    weights = rng.dirichlet(np.full(K, 0.7))
    y = rng.permutation(np.concatenate([np.repeat(np.arange(K), 30), rng.choice(K, NC - 30 * K, p=weights)]))
    means = rng.normal(size=(K, d)) * 2.0
    scale = rng.uniform(0.5, 1.5, size=(K, d))
    return (means[y] + rng.normal(size=(NC, d)) * scale[y]).astype(np.float32), y


def _median_ms(fn, repeats, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        t.append(e0.elapsed_time(e1))
    t.sort()
    return t[len(t) // 2]


def _device_inputs(K, d, dev):
    x, y = data(K, d)
    bins = CA.quantile_bins(torch.from_numpy(x).to(dev))
    fold = CA.kfold_of(NC, KFOLD, SEED)
    return x, y, bins, torch.from_numpy(y.astype(np.int32)).to(dev), torch.from_numpy(fold.astype(np.int32)).to(dev)


def _sklearn_loop(x64, y, n_jobs):
    from sklearn.ensemble import RandomForestClassifier
    from sklearn.model_selection import KFold
    pred = np.empty_like(y)
    t0 = time.perf_counter()
    for tr, te in KFold(n_splits=KFOLD, random_state=SEED, shuffle=True).split(x64):
        m = RandomForestClassifier(n_estimators=TREES, random_state=SEED, n_jobs=n_jobs).fit(x64[tr], y[tr])
        pred[te] = m.predict(x64[te])
        print(f"  sklearn n_jobs={n_jobs}: a fold done at {time.perf_counter() - t0:.1f} s", flush=True)
    return (time.perf_counter() - t0) * 1e3, float(np.mean(pred == y))


def launches_only(shapes):
    dev = torch.device("cuda:0")
    for K, d in shapes:
        _, _, bins, codes, fold = _device_inputs(K, d, dev)
        torch.cuda.synchronize()
        for _ in range(TRACE_CALLS):
            N.forest_cv(bins, codes, fold, K, KFOLD, TREES, max(1, int(np.floor(np.sqrt(d)))), SEED)
        torch.cuda.synchronize()


def merge_trace(trace_dir, out_path):
    """Per shape, the medians over the traced calls of the summed fit, predict and training-row kernel times."""
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no kernel_trace.csv under {trace_dir}")
    rows = sorted(csv.DictReader(open(files[0])), key=lambda r: int(r["Start_Timestamp"]))
    calls = []
    for r in rows:
        name = r["Kernel_Name"]
        if "k_rf_" not in name:
            continue
        if "k_rf_train_rows" in name:
            calls.append({"fit": 0.0, "predict": 0.0, "train_rows": 0.0, "fit_launches": 0})
        if not calls:
            continue
        ms = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
        key = "fit" if "k_rf_fit" in name else ("predict" if "k_rf_predict" in name else "train_rows")
        calls[-1][key] += ms
        calls[-1]["fit_launches"] += key == "fit"
    if len(calls) != TRACE_CALLS * len(SHAPES):
        raise SystemExit(f"{len(calls)} traced calls, expected {TRACE_CALLS * len(SHAPES)}")
    res = json.load(open(out_path))
    for i, (K, d) in enumerate(SHAPES):
        mine = calls[i * TRACE_CALLS:(i + 1) * TRACE_CALLS]
        med = lambda key: sorted(c[key] for c in mine)[len(mine) // 2]
        res["shapes"][f"K{K}_d{d}"]["kernel_trace_ms"] = {"fit": med("fit"), "predict": med("predict"), "train_rows": med("train_rows"),
                                                         "fit_launches": mine[0]["fit_launches"], "calls": len(mine)}
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps({k: v["kernel_trace_ms"] for k, v in res["shapes"].items()}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "forest_time.json"))
    ap.add_argument("--no-sklearn", action="store_true")
    ap.add_argument("--launches-only", action="store_true")
    ap.add_argument("--shape", default=None, help="K,d: that shape only (with --launches-only)")
    ap.add_argument("--merge-trace", default=None)
    args = ap.parse_args()
    if args.merge_trace:
        return merge_trace(args.merge_trace, args.out)
    if args.launches_only:
        return launches_only([tuple(int(v) for v in args.shape.split(","))] if args.shape else SHAPES)
    dev = torch.device("cuda:0")
    try:
        import sklearn
        have_sklearn = None if args.no_sklearn else sklearn.__version__
    except ImportError:
        have_sklearn = None
    res = {"shape": {"n": NC, "kfold": KFOLD, "trees_a_fold": TREES, "chunk_trees": N.forest_chunk(NC, KFOLD, TREES)},
           "repeats": args.repeats, "sklearn": have_sklearn, "shapes": {}}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")

    for K, d in SHAPES:
        x, y, bins, codes, fold = _device_inputs(K, d, dev)
        mtry = CA._forest_refusals(y, NC, d, KFOLD, SEED, TREES, "sqrt")[3]
        xd = torch.from_numpy(x).to(dev)
        out = {"mtry": mtry, "workspace_bytes": int(N.lib().mmvae_forest_workspace_bytes(NC, d, KFOLD, K, TREES))}
        out["forest_cv_ms"] = _median_ms(lambda: N.forest_cv(bins, codes, fold, K, KFOLD, TREES, mtry, SEED), args.repeats)
        out["quantile_bins_ms"] = _median_ms(lambda: CA.quantile_bins(xd), args.repeats)
        _, _, _, _, trees = N.forest_cv(bins, codes, fold, K, KFOLD, 4, mtry, SEED, return_trees=True)
        cnt = trees["count"].cpu().numpy()
        out["nodes_a_tree"] = {"mean": float(cnt.mean()), "max": int(cnt.max())}
        del trees
        t = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            acc, _, _ = CA.RF_classifier(x, {"T": y}, KFOLD, SEED)
            t.append((time.perf_counter() - t0) * 1e3)
        out["rf_classifier_from_host_arrays_ms"] = sorted(t)[1]
        out["accuracy"] = float(np.mean(acc["T"]))
        res["shapes"][f"K{K}_d{d}"] = out
        print(f"K {K} d {d}: {json.dumps(out)}", flush=True)
        save()
    if have_sklearn:
        x, y = data(92, 10)
        x64 = x.astype(np.float64)
        for jobs in (16, 1):
            ms, acc = _sklearn_loop(x64, y, jobs)
            res["shapes"]["K92_d10"][f"sklearn_loop_n_jobs_{jobs}"] = {"ms": ms, "accuracy": acc}
            print(f"sklearn n_jobs={jobs}: {ms:.0f} ms, accuracy {acc:.4f}", flush=True)
            save()
    print(json.dumps(res))


if __name__ == "__main__":
    main()

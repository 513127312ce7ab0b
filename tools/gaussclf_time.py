"""Timing of the Gaussian classifiers at the SmartSeq size: n = 22 365 cells, K = 92 types of uneven sizes (at least 30 cells
each), kfold = 10, for d = 2 (state), 10 (x_low) and 92 (z_prob), on a synthetic mixture of K Gaussians.

per d:
  * the HIP-event median of ``mmvae_group_moments`` (its three launches; K x kfold = 920 groups, rows already ordered) and
    of ``mmvae_gauss_scores`` (one launch of 350 workgroups of 16 waves; rows ordered by fold), with the fp64 fused
    multiply-adds each performs (n d (d + 3) / 2, and n K d (d + 1)) as a fraction of the vector fp64 rate (78.6 TFLOP/s =
    39.3e12 fma/s);
  * the host factorisations between them (``models_from_moments``: kfold x K ``numpy.linalg.eigh`` of d x d), wall clock;
  * ``QDA_classifier`` and ``LDA_classifier`` end to end, from host arrays and from a resident device tensor, wall clock;
  * where sklearn is importable, the reference's loop (``KFold`` x fit / predict of sklearn's QDA and LDA) on the same host,
    and how many of its predictions the device's differ from.

    python tools/gaussclf_time.py [--repeats R] [--out profiles/gaussclf_time.json]
"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import distributed_vae_amd  # noqa: F401,E402
from distributed_vae_amd import _native as N  # noqa: E402
from distributed_vae_amd.utils import cluster_analysis as CA  # noqa: E402

NC, K, KFOLD, SEED = 22365, 92, 10, 0
FP64_FMA_PER_S = 39.3e12


def _median_ms(fn, repeats):
    for _ in range(3):
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


def _wall_ms(fn, repeats):
    fn()
    t = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    t.sort()
    return t[len(t) // 2]


def _sklearn_loop(x64, y, kind):
    from sklearn.discriminant_analysis import LinearDiscriminantAnalysis, QuadraticDiscriminantAnalysis
    from sklearn.model_selection import KFold
    pred = np.empty_like(y)
    t0 = time.perf_counter()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for tr, te in KFold(n_splits=KFOLD, random_state=SEED, shuffle=True).split(x64):
            m = QuadraticDiscriminantAnalysis(reg_param=1e-2) if kind == "qda" else LinearDiscriminantAnalysis()
            m.fit(x64[tr], y[tr])
            pred[te] = m.predict(x64[te])
    return (time.perf_counter() - t0) * 1e3, pred


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gaussclf_time.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(546)
    weights = rng.dirichlet(np.full(K, 0.7))
    y = rng.permutation(np.concatenate([np.repeat(np.arange(K), 30), rng.choice(K, NC - 30 * K, p=weights)]))
    sizes = np.bincount(y, minlength=K)
    fold = CA.kfold_of(NC, KFOLD, SEED)
    try:
        import sklearn
        have_sklearn = sklearn.__version__
    except ImportError:
        have_sklearn = None
    res = {"shape": {"n": NC, "K": K, "kfold": KFOLD, "largest_class": int(sizes.max()), "smallest_class": int(sizes.min())},
           "repeats": args.repeats, "fp64_fma_per_s_roof": FP64_FMA_PER_S, "sklearn": have_sklearn, "d": {}}
    for d in (2, 10, 92):
        means = rng.normal(size=(K, d)) * 2.0
        scale = rng.uniform(0.5, 1.5, size=(K, d))
        x_h = (means[y] + rng.normal(size=(NC, d)) * scale[y]).astype(np.float32)
        x = torch.from_numpy(x_h).to(dev)
        group = y * KFOLD + fold
        order = torch.from_numpy(np.argsort(group, kind="stable")).to(dev)
        counts = np.bincount(group, minlength=K * KFOLD)
        offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)).to(dev)
        xs, pivot = x.index_select(0, order), x.mean(dim=0)
        out = {"moments_path": N.gaussclf_dclass(d)}
        ms = _median_ms(lambda: N.group_moments(xs, offsets, pivot), args.repeats)
        fma = NC * d * (d + 3) // 2
        out["group_moments"] = {"ms": ms, "fma": fma, "fraction_of_fp64_roof": fma / (ms * 1e-3) / FP64_FMA_PER_S,
                                "segments_at_most": K * KFOLD + NC // N.GAUSSCLF_SEG_ROWS,
                                "workspace_bytes": int(N.lib().mmvae_group_moments_workspace_bytes(NC, d, K * KFOLD))}
        s, M = N.group_moments(xs, offsets, pivot)
        s_h, M_h = s.cpu().numpy().reshape(K, KFOLD, d), M.cpu().numpy().reshape(K, KFOLD, -1)
        cnt = counts.reshape(K, KFOLD).astype(np.float64)
        piv_h = pivot.cpu().numpy()
        by_fold = np.argsort(fold, kind="stable")
        perm2 = torch.from_numpy(by_fold).to(dev)
        x2, model = x.index_select(0, perm2), torch.from_numpy(fold[by_fold].astype(np.int32)).to(dev)
        for kind in ("qda", "lda"):
            t0 = time.perf_counter()
            mu, W, c0 = CA.models_from_moments(s_h, M_h, cnt, piv_h, kind)
            host_ms = (time.perf_counter() - t0) * 1e3
            mu_d, W_d, c0_d = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (mu, W, c0))
            ms = _median_ms(lambda: N.gauss_scores(x2, model, mu_d, W_d, c0_d, perm2), max(args.repeats // 3, 3))
            fma = NC * K * d * (d + 1)
            out[kind] = {"host_factorisations_ms": host_ms,
                         "gauss_scores": {"ms": ms, "fma": fma, "fraction_of_fp64_roof": fma / (ms * 1e-3) / FP64_FMA_PER_S,
                                          "workgroups": -(-NC // N.GAUSSCLF_ROW_TILE),
                                          "waves_per_workgroup": min(K, N.GAUSSCLF_SCORE_WAVES), "model_bytes": int(W.nbytes)}}
            fn = CA.QDA_classifier if kind == "qda" else CA.LDA_classifier
            out[kind]["end_to_end_ms"] = {"host_arrays": _wall_ms(lambda: fn(x_h, {"T": y}, KFOLD, SEED), 3),
                                          "resident_tensor": _wall_ms(lambda: fn(x, {"T": y}, KFOLD, SEED), 3)}
            print(f"d {d} {kind}: {json.dumps(out[kind])}", flush=True)
            if have_sklearn:
                ref_ms, ref_pred = _sklearn_loop(x_h.astype(np.float64), y, kind)
                got = CA.gaussian_cv_predict(x, y, KFOLD, SEED, kind=kind)
                small = bool((cnt.sum(axis=1, keepdims=True) - cnt <= d).any()) if kind == "qda" else False
                out[kind]["sklearn_loop"] = {"ms": ref_ms, "predictions_that_differ": int((got["classes"][got["pred"]] != ref_pred).sum()),
                                             "a_training_class_of_at_most_d_cells": small,
                                             "accuracy": float(np.mean(ref_pred == y))}
                print(f"d {d} {kind} sklearn: {json.dumps(out[kind]['sklearn_loop'])}", flush=True)
        res["d"][str(d)] = out
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

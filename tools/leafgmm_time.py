"""Timing of the tree-based analysis at the SmartSeq size: n = 22 365 cells with a 10 % test split, L = 115 leaf types of uneven
sizes (at least 30 cells each) under a random binary dendrogram (114 merges), for d = 2 (state) and 10 (x_low), on a synthetic
mixture of L Gaussians.

per d:
  * the HIP-event medians of ``mmvae_group_moments`` (the training cells ordered by leaf), of ``mmvae_gauss_scores`` (the test
    cells under the 115 leaf models, scores kept) and of ``mmvae_leaf_merge`` (its two launches) at T = 1 and T = 114 levels;
    for ``mmvae_leaf_merge`` the bytes its arithmetic needs (the score matrix read and written once, read once more per level,
    the outputs written) over the time, against the 6.3 TB/s a copy reaches on this part;
  * ``predict_leaf_gmm`` (one level) and ``merge_sweep`` (114 levels) end to end from host arrays, wall clock;
  * the analysis part of ``cpl_mixVAE.classify_tree`` at kfold = 10 on all n cells resident on the device, wall clock;
  * where scipy is importable, a host baseline of this tool's own (``scipy_baseline``: one level of the analysis with a scipy
    ``multivariate_normal`` per leaf, fitted and evaluated afresh per level as a caller without ``merge_sweep`` must): once
    for one level; for the sweep the levels in BASE_LEVELS are timed and the mean is multiplied by 114 -- an extrapolation,
    recorded as such.  It is a stand-in for the cost of a per-level host loop, not a run of the reference's code.

    python tools/leafgmm_time.py [--repeats R] [--out profiles/leafgmm_time.json]
"""
import argparse
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
from distributed_vae_amd.utils import analysis_tree_helpers as TH  # noqa: E402

NC, L, KFOLD, SEED, TEST_SHARE = 22365, 115, 10, 0, 0.1
COPY_BYTES_PER_S = 6.3e12
BASE_LEVELS = (0, 57, 113)


def _median_ms(fn, repeats, before=None):
    for _ in range(3):
        if before:
            before()
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(repeats):
        if before:
            before()
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


def random_merges(rng, leaves):
    """A merge sequence of a random binary dendrogram over ``leaves``, in the form ``get_merge_sequence`` returns."""
    tops, changes = list(leaves), []
    M = len(leaves) - 1
    for i in range(M):
        a, b = sorted(rng.choice(len(tops), size=2, replace=False).tolist(), reverse=True)
        kids = [tops.pop(a), tops.pop(b)]
        tops.append(f"n{M - i}")
        changes.append([kids, tops[-1], 2 * (M - i) - 1])
    return changes


def scipy_baseline(tr, ltr, te, leaves, dataset, desc):
    """The host baseline, this tool's own: one level of the analysis with scipy, every step of it done afresh as a caller
    without ``merge_sweep`` has to -- a frozen ``multivariate_normal`` per leaf with more than 6 training cells (covariance
    + 1e-4 I, its diagonal below 12 cells), the test cells' densities, each row divided by its sum, and the densities carried
    to the level's labels by a 0 / 1 leaf-by-label matrix -> (predicted labels, wall ms)."""
    from scipy.stats import multivariate_normal
    t0 = time.perf_counter()
    d = tr.shape[1]
    columns = []
    for leaf in leaves:
        cells = tr[ltr == leaf]
        if len(cells) <= 6:
            columns.append(np.zeros(len(te)))
            continue
        spread = np.cov(cells.T) + 1e-4 * np.identity(d)
        model = multivariate_normal(mean=cells.mean(axis=0), cov=np.diag(spread) if len(cells) < 12 else spread)
        columns.append(np.atleast_1d(model.pdf(te)))
    density = np.column_stack(columns)
    with np.errstate(invalid="ignore", divide="ignore"):
        share = density / density.sum(axis=1, keepdims=True)
    member = np.zeros((len(leaves), len(dataset)))
    position = {str(leaf): i for i, leaf in enumerate(leaves)}
    for k, lab in enumerate(dataset):
        for name in ([lab] if str(lab) in position else desc.get(str(lab), [])):
            if str(name) in position:
                member[position[str(name)], k] = 1.0
    pred = dataset[np.argmax(share @ member, axis=1)]
    return pred, (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "leafgmm_time.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(547)
    leaves = np.array([f"t{i:03d}" for i in range(L)])
    weights = rng.dirichlet(np.full(L, 0.7))
    y = rng.permutation(np.concatenate([np.repeat(np.arange(L), 30), rng.choice(L, NC - 30 * L, p=weights)]))
    is_test = np.zeros(NC, dtype=bool)
    is_test[rng.permutation(NC)[:int(round(NC * TEST_SHARE))]] = True
    changes = random_merges(rng, leaves.tolist())
    levels = list(range(L - 1))                                      # 0 .. 113: from 115 labels down to 2
    try:
        import scipy
        have_scipy = scipy.__version__
    except ImportError:
        have_scipy = None
    sizes = np.bincount(y[~is_test], minlength=L)
    res = {"shape": {"n": NC, "n_train": int((~is_test).sum()), "n_test": int(is_test.sum()), "L": L, "merges": len(changes),
                     "levels_of_the_sweep": len(levels), "kfold": KFOLD, "largest_training_leaf": int(sizes.max()),
                     "smallest_training_leaf": int(sizes.min())},
           "repeats": args.repeats, "copy_bytes_per_s": COPY_BYTES_PER_S, "scipy": have_scipy, "d": {}}
    lists_all = TH._sweep_levels("leafgmm_time", leaves, changes, levels)[2]
    for d in (2, 10):
        means = rng.normal(size=(L, d)) * 2.0
        scale = rng.uniform(0.5, 1.5, size=(L, d))
        x_h = (means[y] + rng.normal(size=(NC, d)) * scale[y]).astype(np.float32)
        lbl = leaves[y]
        tr_h, te_h, ltr, lte = x_h[~is_test], x_h[is_test], lbl[~is_test], lbl[is_test]
        tr, te = torch.from_numpy(tr_h).to(dev), torch.from_numpy(te_h).to(dev)
        n_test = int(te.shape[0])
        order = np.argsort(y[~is_test], kind="stable")
        offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)).to(dev)
        xs, pivot = tr.index_select(0, torch.from_numpy(order).to(dev)), tr.mean(dim=0)
        out = {"group_moments_ms": _median_ms(lambda: N.group_moments(xs, offsets, pivot), args.repeats)}
        models = TH.leaf_gaussians(tr, ltr, leaves)
        out["leaf_gaussians_ms"] = _wall_ms(lambda: TH.leaf_gaussians(tr, ltr, leaves), 5)
        mu, W, c0 = (torch.from_numpy(np.ascontiguousarray(models[k])).to(dev) for k in ("mu", "W", "c0"))
        model = torch.zeros(n_test, dtype=torch.int32, device=dev)
        out["gauss_scores_ms"] = _median_ms(lambda: N.gauss_scores(te, model, mu, W, c0, None, True), args.repeats)
        scores = N.gauss_scores(te, model, mu, W, c0, None, True)[3]
        p = scores.clone()
        for name, lists in (("T1", lists_all[:1]), ("T114", lists_all)):
            ls, st, lf = N.merge_tables(lists)
            T, K_max = len(lists), int(np.diff(ls).max())
            d_ls, d_st, d_lf = (torch.from_numpy(a).to(dev) for a in (ls, st, lf))        # the tables resident: the C entry alone
            label = torch.empty(T, n_test, dtype=torch.int32, device=dev)
            prob = torch.empty(T, n_test, dtype=torch.float64, device=dev)

            def entry():
                N.check(N.lib().mmvae_leaf_merge(p.data_ptr(), L, n_test, L, d_ls.data_ptr(), T, d_st.data_ptr(), len(st) - 1, K_max,
                                                 d_lf.data_ptr(), len(lf), None, 0, label.data_ptr(), prob.data_ptr(), None, None, 0,
                                                 torch.cuda.current_stream().cuda_stream), "mmvae_leaf_merge")
            ms = _median_ms(entry, args.repeats, before=lambda: p.copy_(scores))
            need = 2 * n_test * L * 8 + T * (n_test * L * 8 + n_test * 12)
            out[f"leaf_merge_{name}"] = {"ms": ms, "levels": T, "bytes": need, "bytes_per_s": need / (ms * 1e-3),
                                         "fraction_of_copy_rate": need / (ms * 1e-3) / COPY_BYTES_PER_S}
        dataset0, desc0 = TH.labels_at(leaves, changes, 0), TH.descendants_at(changes, 0)
        out["predict_leaf_gmm_end_to_end_ms"] = _wall_ms(lambda: TH.predict_leaf_gmm(
            tr_h, ltr, te_h, lte, unique_dataset_lbl=dataset0, unique_leaf_lbl=leaves, descendant_dict=desc0), 5)
        out["merge_sweep_end_to_end_ms"] = _wall_ms(lambda: TH.merge_sweep(tr_h, ltr, te_h, lte, changes, leaves), 5)
        x_all = torch.from_numpy(x_h).to(dev)
        out["classify_tree_analysis_ms"] = _wall_ms(lambda: TH.classify_tree_points(x_all, lbl, changes, leaves, KFOLD, SEED), 3)
        sweep = TH.merge_sweep(tr_h, ltr, te_h, lte, changes, leaves)
        out["accuracy"] = {"leaves": float(sweep["acc"][0]), "two_labels": float(sweep["acc"][-1])}
        print(f"d {d}: {json.dumps(out)}", flush=True)
        if have_scipy:
            tr64, te64 = tr_h.astype(np.float64), te_h.astype(np.float64)
            per_level, differ = [], 0
            for m in BASE_LEVELS:
                pred, ms = scipy_baseline(tr64, ltr, te64, leaves, TH.labels_at(leaves, changes, m), TH.descendants_at(changes, m))
                per_level.append(ms)
                differ += int((pred[sweep["keep"]] != sweep["pred"][m]).sum())
            out["scipy_baseline"] = {"one_level_ms": per_level[0], "levels_timed": list(BASE_LEVELS), "ms_of_those": per_level,
                                     "sweep_ms_extrapolated": float(np.mean(per_level)) * len(levels),
                                     "predictions_that_differ_at_those_levels": differ}
            print(f"d {d} scipy baseline: {json.dumps(out['scipy_baseline'])}", flush=True)
        res["d"][str(d)] = out
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

"""Timing of the silhouette samples at the SmartSeq size: n = 22 365 cells in K = 92 clusters, d in {2, 10, 92}, synthetic
blobs.  Per d: the HIP-event median of ``mmvae_silhouette`` (its three launches, on points already sorted on the device),
``get_SilhScore`` end to end from host arrays, and on the host of the same run the fp64 restatement
(tests/silhouette_restatement.py) on a SAMPLE of rows extrapolated to all of them (labelled ``extrapolated``) and, where
sklearn is importable, ``sklearn.metrics.silhouette_samples`` in full.  The device's samples of the sampled rows are compared
with the restatement's.

    python tools/silhouette_time.py [--repeats R] [--sample ROWS] [--out profiles/silhouette_time.json]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import distributed_vae_amd  # noqa: F401,E402
import silhouette_restatement as SR  # noqa: E402
from distributed_vae_amd import _native as N  # noqa: E402
from distributed_vae_amd.utils.cluster_analysis import get_SilhScore  # noqa: E402

NC, K, DIMS = 22365, 92, (2, 10, 92)
SKLEARN_BUILD_CONTAINER_S = 5.8      # sklearn 1.7.2 at d = 10 on the build container's CPUs, measured once; quoted where sklearn is absent


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--sample", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "silhouette_time.json"))
    args = ap.parse_args()
    try:
        from sklearn.metrics import silhouette_samples as sk_samples
    except ImportError:
        sk_samples = None
    rng = np.random.default_rng(546)
    # cluster sizes as uneven as a taxonomy's: a few large types, many small ones
    weights = rng.dirichlet(np.full(K, 0.7))
    labels = np.concatenate([np.arange(K), rng.choice(K, NC - K, p=weights)])
    labels = rng.permutation(labels)
    sizes = np.bincount(labels, minlength=K)
    res = {"shape": {"n": NC, "K": K, "largest_cluster": int(sizes.max()), "smallest_cluster": int(sizes.min())},
           "repeats": args.repeats, "segments": int(sum(-(-int(f) // N.SILHOUETTE_SEG_COLS) for f in sizes)),
           "workspace_bytes": int(N.lib().mmvae_silhouette_workspace_bytes(NC, K)), "pairs": NC * NC, "d": {}}
    order = np.argsort(labels, kind="stable")
    offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)).cuda()
    perm = torch.from_numpy(order).cuda()
    rows = slice(0, args.sample)
    for d in DIMS:
        x = (rng.normal(size=(K, d))[labels] * 1.5 + rng.normal(size=(NC, d))).astype(np.float32)
        xs = torch.from_numpy(x[order]).cuda()
        out = torch.empty(NC, dtype=torch.float64, device="cuda")
        r = {"instance_dv": N.silhouette_dv(d)}
        r["kernel_ms"] = _median_ms(lambda: N.silhouette(xs, offsets, perm, out=out), args.repeats)
        r["get_SilhScore_ms"] = _median_ms(lambda: get_SilhScore(x, labels), max(args.repeats // 4, 3))
        dev = N.silhouette(xs, offsets, perm).cpu().numpy()
        t0 = time.perf_counter()
        want = SR.silhouette_samples(x, labels, rows)
        r["host_restatement_s_extrapolated"] = (time.perf_counter() - t0) * NC / args.sample
        r["sample_rows"] = args.sample
        r["sample_worst_device_minus_restatement"] = float(np.abs(dev[rows] - want).max())
        r["gate"] = SR.tolerance(d)
        if sk_samples is not None:
            x64 = x.astype(np.float64)
            t0 = time.perf_counter()
            theirs = sk_samples(x64, labels)
            r["host_sklearn_s"] = time.perf_counter() - t0
            r["worst_device_minus_sklearn"] = float(np.abs(dev - theirs).max())
        else:
            r["host_sklearn_s_build_container_d10"] = SKLEARN_BUILD_CONTAINER_S
        res["d"][str(d)] = r
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

"""Timing of the device k-nearest-neighbour search (csrc/knn.hip), all from one run on one GPU.

Shapes: n = 22 365 cells with d in {2, 10, 92} and k = 15; n = 131 072 with d = 10, k = 15; n = 22 365 with d = 10, k = 64 --
Gaussian mixtures of 20 centres drawn here, every cell against all others (groups = arange), or the one shape of
``--synthetic N D K``.  Per shape, HIP-event medians after a warm-up, the variants timed in turn in one process (A / B / A / B,
so that what drifts over the run touches all alike):

  * ``mmvae_knn`` alone, through ctypes on buffers made beforehand (``knn_ms``), and its two launches apart
    (``mmvae_debug_knn``'s ``phases``: the segment launch, the merge of the lists it left);
  * the torch composition on the same GPU: row chunks of the difference-form squared distance, added coordinate by
    coordinate into a chunk x n buffer, the diagonal set to +inf, ``topk``; the chunk is sized to keep the temporaries below
    2 GB, and their peak is recorded.  ``topk`` breaks ties as it likes, so on an integer lattice of the same shape its
    squared distances are compared with the kernel's (``lattice_dist2_equal``), not its indices;
  * ``knn`` and ``KNN_classifier`` (10 folds) end to end from host arrays: wall clock, upload and download included;
  * where sklearn is importable and n <= 32 768: ``NearestNeighbors(algorithm="brute")`` and the ``KNeighborsClassifier`` loop
    over the same folds on the same host, run once.

    python tools/time_knn.py [--repeats R] [--synthetic N D K] [--out profiles/knn_time.json]
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
from distributed_vae_amd.utils import neighbors as NB  # noqa: E402
from distributed_vae_amd.utils.cluster_analysis import kfold_of  # noqa: E402

SHAPES = [(22365, 2, 15), (22365, 10, 15), (22365, 92, 15), (131072, 10, 15), (22365, 10, 64)]
TEMP_BYTES = 2 * 10 ** 9
KFOLD = 10


def _points(rng, n, d, lattice=False):
    if lattice:
        return rng.integers(-8, 9, size=(n, d)).astype(np.float32)
    labels = rng.integers(0, 20, n)
    mu = 3.0 * rng.standard_normal((20, d))
    return (mu[labels] + rng.standard_normal((n, d))).astype(np.float32), labels


def _alternating_ms(calls: dict, repeats, warm=1):
    for _ in range(warm):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in calls}
    for _ in range(repeats):
        for k, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            t[k].append(e0.elapsed_time(e1))
    return {k: sorted(v)[len(v) // 2] for k, v in t.items()}


def _wall_s(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def _entry_calls(x, k):
    """Closures around mmvae_debug_knn on buffers made here, once: the whole call (phases 0: mmvae_knn itself), the segment
    launch alone and the merge alone.  Returns (calls, idx, dist2, workspace bytes)."""
    n, d = (int(v) for v in x.shape)
    L, dev = NB._lib(), x.device
    own = torch.arange(n, dtype=torch.int32, device=dev)
    ws_bytes = int(L.mmvae_knn_workspace_bytes(n, n, d, k))
    ws = N._workspace(ws_bytes, dev)
    idx, dist2 = NB._buffer((n, k), torch.int32, dev), NB._buffer((n, k), torch.float32, dev)

    def call(phases):
        def run():
            N.check(L.mmvae_debug_knn(N._ptr(x), int(x.stride(0)), n, N._ptr(x), int(x.stride(0)), n, d, k, N._ptr(own), N._ptr(own),
                                      N._ptr(ws), int(ws.numel()) * 8, N._ptr(idx), N._ptr(dist2), 0, phases, N._stream(dev)),
                    "mmvae_debug_knn")
        return run
    calls = {"knn": call(0)}
    if ws_bytes > 8:
        calls["segments"], calls["merge"] = call(1), call(2)
    return calls, idx, dist2, ws_bytes


def torch_composition(x, k):
    """(idx int64 [n, k], dist2 float32 [n, k]) of every row against all others from torch ops, in row chunks."""
    n, d = (int(v) for v in x.shape)
    chunk = max(1, min(n, TEMP_BYTES // (10 * n)))                          # d2 and t (4 bytes each) and room for topk's sort
    xt = x.t().contiguous()
    idx = torch.empty(n, k, dtype=torch.int64, device=x.device)
    dist2 = torch.empty(n, k, dtype=torch.float32, device=x.device)
    for r0 in range(0, n, chunk):
        r1 = min(n, r0 + chunk)
        d2 = torch.zeros(r1 - r0, n, dtype=torch.float32, device=x.device)
        for c in range(d):
            t = xt[c, r0:r1, None] - xt[c, None, :]
            d2.addcmul_(t, t)
        d2[torch.arange(r1 - r0, device=x.device), torch.arange(r0, r1, device=x.device)] = float("inf")
        dist2[r0:r1], idx[r0:r1] = torch.topk(d2, k, dim=1, largest=False, sorted=True)
    return idx, dist2


def _torch_peak(x, k):
    dev = x.device
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    out = torch_composition(x, k)
    torch.cuda.synchronize()
    return out, int(torch.cuda.max_memory_allocated(dev) - base)


def measure(n, d, k, repeats, dev, rng):
    host, labels = _points(rng, n, d)
    x = torch.from_numpy(host).to(dev)
    calls, idx, dist2, ws_bytes = _entry_calls(x, k)
    calls["knn"]()
    (t_idx, t_d2), peak = _torch_peak(x, k)
    same_sets = float((torch.sort(t_idx, dim=1).values == torch.sort(idx.to(torch.int64), dim=1).values).all(dim=1).float().mean())
    lat = torch.from_numpy(_points(rng, min(n, 22365), d, lattice=True)).to(dev)
    l_idx, l_d2 = NB.knn_device(lat, lat, k, *(2 * [torch.arange(len(lat), dtype=torch.int32, device=dev)]))
    lattice_equal = bool(torch.equal(torch_composition(lat, k)[1], l_d2))
    del lat, l_idx, l_d2, t_idx, t_d2
    few = max(repeats // 2, 3) if n <= 32768 else 2
    ms = _alternating_ms(calls, repeats)
    both = _alternating_ms({"knn": calls["knn"], "torch_composition": lambda: torch_composition(x, k)}, few)
    row = {"n": n, "d": d, "k": k, "workspace_bytes": ws_bytes, "knn_ms": ms["knn"],
           "segments_ms": ms.get("segments"), "merge_ms": ms.get("merge"),
           "pairs_per_s": n * (n - 1) / (ms["knn"] * 1e-3),
           "alternating": {"knn_ms": both["knn"], "torch_composition_ms": both["torch_composition"],
                           "torch_over_knn": both["torch_composition"] / both["knn"]},
           "torch_peak_temporary_bytes": peak, "rows_with_the_kernels_neighbour_set": same_sets,
           "lattice_dist2_equal": lattice_equal}
    NB.knn(host, k, device=dev)
    row["knn_from_host_s"] = _wall_s(lambda: NB.knn(host, k, device=dev))
    if k <= (n - n // KFOLD - 1):
        NB.KNN_classifier(host, {"y": labels}, KFOLD, 0, k=k)
        row["KNN_classifier_from_host_s"] = _wall_s(lambda: NB.KNN_classifier(host, {"y": labels}, KFOLD, 0, k=k))
    try:
        from sklearn.neighbors import KNeighborsClassifier, NearestNeighbors
    except ImportError:
        row["host_sklearn"] = "not measured: sklearn is not importable on this host"
        return row
    if n > 32768:
        row["host_sklearn"] = "not measured above 32768 cells"
        return row
    x64 = host.astype(np.float64)
    t0 = time.perf_counter()
    NearestNeighbors(n_neighbors=k, algorithm="brute").fit(x64).kneighbors()
    t1 = time.perf_counter()
    fold = kfold_of(n, KFOLD, 0)
    for f in range(KFOLD):
        KNeighborsClassifier(n_neighbors=k, algorithm="brute").fit(x64[fold != f], labels[fold != f]).predict(x64[fold == f])
    row["host_sklearn"] = {"NearestNeighbors_s": t1 - t0, "KNeighborsClassifier_loop_s": time.perf_counter() - t1}
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--synthetic", type=int, nargs=3, metavar=("N", "D", "K"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_time.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(812)
    res = {"repeats": args.repeats, "device": torch.cuda.get_device_name(dev), "shapes": []}
    for n, d, k in ([tuple(args.synthetic)] if args.synthetic else SHAPES):
        res["shapes"].append(measure(n, d, k, args.repeats, dev, rng))
        print(json.dumps(res["shapes"][-1]), flush=True)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()

"""Timing of the device PCA at the SmartSeq size: n = 22 365 cells x D = 5032 genes, k = 10 components, on a synthetic
non-negative matrix with 30 decaying factors under noise (so that the subspace iteration has a spectrum to converge on).

  * the HIP-event median of the three launches, each alone: ``mmvae_gram`` (covariance; its two kernels), ``mmvae_symm_mul``
    at the iteration's block width, ``mmvae_pca_project``;
  * the Gram's useful flops (n D (D + 1): the entries with i <= j) and the flops it executes (whole 64 x 64 tiles, the
    diagonal ones in full) against the back-to-back issue rate of v_mfma_f64_16x16x4_f64, MEASURED in the same run by
    tools/micro/mfma_f64_bench (built beforehand; a child process);
  * ``pca_fit`` (iteration count, residual, gap) and ``cluster_compare(pca="device")`` end to end, wall clock, from the
    resident device tensor;
  * with ``--host``: the host path ``cluster_analysis._project`` (numpy's full SVD in fp64) on the same matrix on the same
    host, ONCE; without it the figure is extrapolated by N D^2 from a 6000 x 2500 SVD timed in the same run and is labelled so.

    python tools/pca_time.py [--repeats R] [--host] [--out profiles/pca_time.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import distributed_vae_amd  # noqa: F401,E402
from distributed_vae_amd import _native as N  # noqa: E402
from distributed_vae_amd.utils import cluster_analysis as CA  # noqa: E402
from distributed_vae_amd.utils import pca as P  # noqa: E402

NC, DM, K_PC, K_TYPES = 22365, 5032, 10, 92
MICRO = os.path.join(ROOT, "tools", "micro", "mfma_f64_bench")


def _median_ms(fn, repeats):
    for _ in range(2):
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


def _wall_s(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def _mfma_rate():
    """The last line of tools/micro/mfma_f64_bench: {"cus", "clock_mhz", "best_ns_per_mfma_per_simd", "best_tflops"}."""
    if not os.path.exists(MICRO):
        return None
    out = subprocess.run([MICRO], check=True, capture_output=True, text=True, timeout=120).stdout.strip().splitlines()
    words = out[-1].split()
    return {"lines": out[:-1], **{words[i]: float(words[i + 1]) for i in range(1, len(words), 2)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--host", action="store_true", help="time the host SVD path at full size once (about a minute)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pca_time.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"shape": {"n": NC, "D": DM, "k": K_PC}, "repeats": args.repeats, "mfma_f64_16x16x4": _mfma_rate()}
    g = torch.Generator(device=dev)
    g.manual_seed(546)
    scales = 3.0 * 0.85 ** torch.arange(30, device=dev, dtype=torch.float32)
    H = torch.randn(NC, 30, generator=g, device=dev) * scales
    W = torch.randn(30, DM, generator=g, device=dev) / 30 ** 0.5
    x = torch.relu(H @ W + 0.5 * torch.randn(NC, DM, generator=g, device=dev) + 0.3).contiguous()
    labels = {"types": torch.argmax(H[:, :7] @ torch.randn(7, K_TYPES, generator=g, device=dev), dim=1).cpu().numpy()}
    pivot = x.mean(dim=0)
    nseg, seg_rows = N.gram_segments(NC, DM)
    T = -(-DM // N.GRAM_TILE)
    useful, executed = NC * DM * (DM + 1), 2 * NC * (T * (T + 1) // 2) * N.GRAM_TILE ** 2
    ms = _median_ms(lambda: N.gram(x, pivot, cov=True), args.repeats)
    res["gram"] = {"ms": ms, "segments": nseg, "tiles": T * (T + 1) // 2, "workspace_bytes": int(N.lib().mmvae_gram_workspace_bytes(NC, DM)),
                   "path": "wide" if N.gram_wide(x) else "narrow", "useful_flops": useful, "executed_flops": executed,
                   "useful_tflops": useful / (ms * 1e-3) / 1e12, "executed_tflops": executed / (ms * 1e-3) / 1e12}
    if res["mfma_f64_16x16x4"]:
        res["gram"]["executed_fraction_of_measured_mfma_rate"] = res["gram"]["executed_tflops"] / res["mfma_f64_16x16x4"]["best_tflops"]
    print(f"gram: {json.dumps(res['gram'])}", flush=True)
    s, C = N.gram(x, pivot, cov=True)
    b = min(DM, K_PC + max(8, K_PC))
    Q = torch.randn(DM, b, generator=g, device=dev, dtype=torch.float64)
    ms = _median_ms(lambda: N.symm_mul(C, Q), args.repeats)
    res["symm_mul"] = {"ms": ms, "b": b, "bytes_of_C": 8 * DM * DM, "tb_per_s": 8 * DM * DM / (ms * 1e-3) / 1e12}
    mean = pivot.double() + s / NC
    V = torch.linalg.qr(torch.randn(DM, K_PC, generator=g, device=dev, dtype=torch.float64))[0].contiguous()
    ms = _median_ms(lambda: N.pca_project(x, mean, V), args.repeats)
    res["pca_project"] = {"ms": ms, "bytes_of_data": 4 * NC * DM, "tb_per_s": 4 * NC * DM / (ms * 1e-3) / 1e12}
    print(f"symm_mul: {json.dumps(res['symm_mul'])}  pca_project: {json.dumps(res['pca_project'])}", flush=True)
    P.pca_fit(x, K_PC)                                                         # warm: allocator, library load
    secs, fit = _wall_s(lambda: P.pca_fit(x, K_PC))
    res["pca_fit"] = {"s": secs, "iterations": fit.iterations, "converged": fit.converged, "solver_used": fit.solver_used,
                      "residual": fit.residual, "gap": fit.gap, "explained_variance_ratio_sum": float(fit.explained_variance_ratio.sum())}
    secs, out = _wall_s(lambda: CA.cluster_compare(x, labels, K_PC, pca="device"))
    res["cluster_compare_device"] = {"s": secs, "sil_score": float(out[2][0])}
    print(f"pca_fit: {json.dumps(res['pca_fit'])}  cluster_compare: {json.dumps(res['cluster_compare_device'])}", flush=True)
    x_h = x.cpu().numpy()
    if args.host:
        t0 = time.perf_counter()
        z = CA._project(x_h, K_PC)
        res["host_project"] = {"s": time.perf_counter() - t0, "extrapolated": False, "cpus": os.cpu_count(),
                               "threads": os.environ.get("OMP_NUM_THREADS")}
        zd = P.pca_transform(fit, x)
        res["host_project"]["worst_abs_difference_of_abs_projection"] = float(np.abs(np.abs(z) - np.abs(zd)).max())
    else:
        small = np.ascontiguousarray(x_h[:6000, :2500])
        t0 = time.perf_counter()
        CA._project(small, K_PC)
        t_small = time.perf_counter() - t0
        res["host_project"] = {"s": t_small * (NC * DM ** 2) / (6000 * 2500 ** 2), "extrapolated": True,
                               "from": {"shape": [6000, 2500], "s": t_small, "rule": "N D^2"}, "cpus": os.cpu_count(),
                               "threads": os.environ.get("OMP_NUM_THREADS")}
    res["speedup_project_end_to_end"] = res["host_project"]["s"] / res["pca_fit"]["s"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

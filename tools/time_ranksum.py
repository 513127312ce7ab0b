"""Timing of the rank-sum test of every gene at the SmartSeq size: N = 22 365 cells, D = 5032 genes, G = 92 groups of uneven
sizes, on synthetic-10x-style data (bench.py's ``synthetic_rows``: 20 % of the entries positive), all from one run.

  * the HIP-event median of ``mmvae_rank_sum`` alone, called through ctypes with the workspace and the four outputs made
    beforehand (``kernel_ms``: the entry's argument checks, its one ``hipFuncSetAttribute`` and its launches -- per chunk of
    512 genes one staging transpose and one rank kernel; the row map and offsets already on the device), and of the Python
    wrapper ``rank_sums`` around it, which allocates those five buffers on every call (``rank_sums_wrapper_ms``);
  * ``rank_sum_test`` end to end from the resident matrix (the host-side group sort, the launches, the copies of the integers
    to the host, the numpy float64 finish and Benjamini-Hochberg) and from host arrays (the upload of the matrix besides);
  * the same integers composed from torch ops on the same GPU -- ``torch.sort`` of the transposed matrix, two
    ``searchsorted``, ``index_add_`` -- with the peak of the memory they allocate, and whether they equal the kernel's;
  * on the host of the same run, where scipy is importable, ``scipy.stats.mannwhitneyu`` per (gene, group) on a SAMPLE of
    genes, extrapolated to all D (labelled ``extrapolated``);
  * the kernel at the cap, n = 32 768, on the same kind of data and on data without a single tie (the worst case: every search
    runs its full depth and nothing in the sort is already in place).

    python tools/time_ranksum.py [--repeats R] [--sample GENES] [--out profiles/ranksum_time.json]
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
from bench import synthetic_rows  # noqa: E402
from distributed_vae_amd import _native as N  # noqa: E402
from distributed_vae_amd.utils import marker_analysis as MA  # noqa: E402

NC, DG, K = 22365, 5032, 92


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


def _entry_call(data, order, offsets, eps=0.0):
    """A closure that calls mmvae_rank_sum on buffers made here, once: nothing but the C entry is inside a timing bracket."""
    n, G, Dm = int(order.numel()), int(offsets.numel()) - 1, int(data.shape[1])
    L, dev = MA._lib(), data.device
    ws_bytes = int(L.mmvae_rank_sum_workspace_bytes(n, Dm, G))
    ws = N._workspace(ws_bytes, dev)
    r2, pos, tot = (MA._buffer((G, Dm), dt, dev) for dt in (torch.int64, torch.int64, torch.float64))
    tie = MA._buffer((Dm,), torch.int64, dev)
    keep = (ws, r2, pos, tot, tie)

    def call():
        N.check(L.mmvae_rank_sum(N._ptr(data), int(data.stride(0)), int(data.shape[0]), Dm, N._ptr(order), n, N._ptr(offsets), G,
                                 float(eps), N._ptr(keep[0]), ws_bytes, N._ptr(r2), N._ptr(tie), N._ptr(pos), N._ptr(tot),
                                 N._stream(dev)), "mmvae_rank_sum")
    return call


def _groups(rng, n):
    weights = rng.dirichlet(np.full(K, 0.7))
    labels = rng.permutation(np.concatenate([np.arange(K), rng.choice(K, n - K, p=weights)]))
    sizes = np.bincount(labels, minlength=K)
    return labels, sizes


def _device_groups(labels, sizes, dev):
    order = torch.from_numpy(np.argsort(labels, kind="stable").astype(np.int64)).to(dev)
    offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)).to(dev)
    return order, offsets


def torch_composition(data, codes, G):
    """(rank_sum2 [G, D], tie_term [D]) from torch ops: the N x D sorted values, their N x D int64 indices (which torch.sort
    returns whether they are wanted or not) and the N x D int64 bounds are temporaries."""
    xt = data.t().contiguous()
    s = torch.sort(xt, dim=1).values
    lo = torch.searchsorted(s, xt, right=False)
    hi = torch.searchsorted(s, xt, right=True)
    t = hi - lo
    tie = (t * t - 1).sum(dim=1)
    twice = (lo + hi + 1).t().contiguous()
    r2 = torch.zeros(G, data.shape[1], dtype=torch.int64, device=data.device).index_add_(0, codes, twice)
    return r2, tie


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--sample", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ranksum_time.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(546)
    data = synthetic_rows(NC, DG, 546, dev)
    labels, sizes = _groups(rng, NC)
    order, offsets = _device_groups(labels, sizes, dev)
    res = {"shape": {"n": NC, "D": DG, "G": K, "positive_fraction": float((data > 0).float().mean()),
                     "largest_group": int(sizes.max()), "smallest_group": int(sizes.min())},
           "repeats": args.repeats, "matrix_bytes": NC * DG * 4,
           "workspace_bytes": int(MA._lib().mmvae_rank_sum_workspace_bytes(NC, DG, K))}
    res["kernel_ms"] = _median_ms(_entry_call(data, order, offsets), args.repeats)
    res["rank_sums_wrapper_ms"] = _median_ms(lambda: MA.rank_sums(data, order, offsets), args.repeats)
    res["genes_per_s"] = DG / (res["kernel_ms"] * 1e-3)
    few = max(args.repeats // 2, 3)
    res["rank_sum_test_ms"] = {"resident_matrix": _wall_ms(lambda: MA.rank_sum_test(data, labels), few)}
    host = data.cpu().numpy()
    res["rank_sum_test_ms"]["host_arrays"] = _wall_ms(lambda: MA.rank_sum_test(host, labels, device=dev), few)
    # the torch composition on the same GPU
    codes = torch.from_numpy(labels.astype(np.int64)).to(dev)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    r2_t, tie_t = torch_composition(data, codes, K)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(dev) - base
    r2_k, tie_k, _, _ = MA.rank_sums(data, order, offsets)
    res["torch_composition"] = {"ms": _median_ms(lambda: torch_composition(data, codes, K), few, warm=1),
                                "peak_temporary_bytes": int(peak),
                                "equals_the_kernel": bool(torch.equal(r2_t, r2_k) and torch.equal(tie_t, tie_k))}
    del r2_t, tie_t
    # scipy's loop on the host, on a sample of genes
    try:
        from scipy import stats
    except ImportError:
        stats = None
    if stats is None:
        res["host_scipy_loop"] = "not measured: scipy is not importable on this host"
    else:
        genes = np.sort(rng.choice(DG, args.sample, replace=False))
        r2_h = r2_k.cpu().numpy()
        t0 = time.perf_counter()
        exact = True
        for j in genes:
            col = host[:, j]
            for g in range(K):
                m = labels == g
                u = stats.mannwhitneyu(col[m], col[~m], use_continuity=False, method="asymptotic").statistic
                exact &= bool(u == r2_h[g, j] / 2.0 - sizes[g] * (sizes[g] + 1) / 2.0)
        dt = time.perf_counter() - t0
        res["host_scipy_loop"] = {"sample_genes": int(args.sample), "calls": int(args.sample) * K, "sample_s": dt,
                                  "s_extrapolated_all_genes": dt * DG / args.sample, "U_equals_the_kernel": exact}
    del host
    # the cap
    n_cap = MA.MAX_CELLS
    labels_c, sizes_c = _groups(rng, n_cap)
    order_c, offsets_c = _device_groups(labels_c, sizes_c, dev)
    tied = synthetic_rows(n_cap, DG, 547, dev)
    res["cap_n32768"] = {"workspace_bytes": int(MA._lib().mmvae_rank_sum_workspace_bytes(n_cap, DG, K)),
                         "kernel_ms": _median_ms(_entry_call(tied, order_c, offsets_c), few)}
    del tied
    perm = torch.stack([torch.randperm(n_cap, device=dev) for _ in range(64)], dim=1).to(torch.float32)
    distinct = (perm.repeat(1, (DG + 63) // 64)[:, :DG] + 0.25).contiguous()           # every column a permutation: no ties
    r2_d, tie_d, _, _ = MA.rank_sums(distinct, order_c, offsets_c)
    res["cap_n32768"]["no_ties_kernel_ms"] = _median_ms(_entry_call(distinct, order_c, offsets_c), few)
    res["cap_n32768"]["no_ties_tie_term_is_zero"] = bool((tie_d == 0).all())
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

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
    runs its full depth and nothing in the sort is already in place);
  * both entries (the blocked one with blocks of 32 768 cells) at the most groups a call takes: n = 8192, D = 512, G = 4096
    groups of two cells.

    python tools/time_ranksum.py [--repeats R] [--sample GENES] [--out profiles/ranksum_time.json]

``--blocked`` measures the blocked path instead (``mmvae_rank_sum_blocked``) and writes
profiles/ranksum_blocked_time.json; G = 92 throughout, the variants of one shape timed alternately in one process, medians:

  * N = 22 365, D = 5032: ``mmvae_rank_sum`` beside the blocked entry with the default block and with blocks of 8192 cells;
  * N = 131 072, D = 5032: both forms of ``k_rsb_rank`` (every block's keys copied to LDS; searched where they lie) and the
    split over the staging copy, the block sort, the ranks and the reduction, from calls cut short after each
    (``mmvae_debug_rank_sum_blocked``'s ``phases``);
  * N = 1 048 576, D = 512 (a 2.1 GB matrix; D = 5032 would be 21 GB);
  * beside each the torch composition in gene chunks, with the peak of its temporaries and whether its integers are equal.

    python tools/time_ranksum.py --blocked [--repeats R] [--out profiles/ranksum_blocked_time.json]
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


def _alternating_ms(calls: dict, repeats, warm=1):
    """HIP-event medians of several calls timed in turn, ``repeats`` rounds: what drifts over the run touches all alike."""
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


def _blocked_call(data, order, offsets, block, out=None, form=-1, phases=0):
    """A closure around mmvae_debug_rank_sum_blocked (form -1, phases 0: mmvae_rank_sum_blocked itself) on buffers made here;
    ``out``: the (ws, r2, tie, pos, tot) of an earlier closure of the same shape to share.  Returns (call, buffers)."""
    n, G, Dm = int(order.numel()), int(offsets.numel()) - 1, int(data.shape[1])
    L, dev = MA._lib(), data.device
    ws_bytes = int(L.mmvae_rank_sum_blocked_workspace_bytes(n, Dm, G, block))
    if out is None:
        r2, pos, tot = (MA._buffer((G, Dm), dt, dev) for dt in (torch.int64, torch.int64, torch.float64))
        out = (N._workspace(ws_bytes, dev), r2, MA._buffer((Dm,), torch.int64, dev), pos, tot)
    ws, r2, tie, pos, tot = out

    def call():
        N.check(L.mmvae_debug_rank_sum_blocked(N._ptr(data), int(data.stride(0)), int(data.shape[0]), Dm, N._ptr(order), n,
                                               N._ptr(offsets), G, 0.0, block, N._ptr(ws), ws_bytes, N._ptr(r2), N._ptr(tie),
                                               N._ptr(pos), N._ptr(tot), form, phases, N._stream(dev)),
                "mmvae_debug_rank_sum_blocked")
    return call, out


def _torch_chunked(data, codes, G, chunk):
    r2 = torch.empty(G, data.shape[1], dtype=torch.int64, device=data.device)
    tie = torch.empty(data.shape[1], dtype=torch.int64, device=data.device)
    for g0 in range(0, data.shape[1], chunk):
        r2[:, g0:g0 + chunk], tie[g0:g0 + chunk] = torch_composition(data[:, g0:g0 + chunk], codes, G)
    return r2, tie


def _torch_row(data, labels, G, chunk, r2_k, tie_k, repeats):
    """The torch composition in chunks of ``chunk`` genes: its time, the peak of what it allocates (its two results included)
    and whether its integers are the kernel's in every element."""
    dev = data.device
    codes = torch.from_numpy(labels.astype(np.int64)).to(dev)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    r2_t, tie_t = _torch_chunked(data, codes, G, chunk)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(dev) - base
    equal = bool(torch.equal(r2_t, r2_k) and torch.equal(tie_t, tie_k))
    del r2_t, tie_t
    return {"gene_chunk": chunk, "ms": _median_ms(lambda: _torch_chunked(data, codes, G, chunk), repeats, warm=0),
            "peak_temporary_bytes": int(peak), "equals_the_kernel": equal}


def main_blocked(args):
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(547)
    L = MA._lib()
    res = {"G": K, "repeats": args.repeats}
    few = max(args.repeats // 2, 3)
    # N = 22 365: the one-call entry beside the blocked one
    data = synthetic_rows(NC, DG, 546, dev)
    labels, sizes = _groups(rng, NC)
    order, offsets = _device_groups(labels, sizes, dev)
    b0, out = _blocked_call(data, order, offsets, 0)
    b8192, _ = _blocked_call(data, order, offsets, 8192, out)
    ms = _alternating_ms({"mmvae_rank_sum": _entry_call(data, order, offsets), "blocked_block_0": b0, "blocked_block_8192": b8192},
                         args.repeats)
    one = [t.clone() for t in MA.rank_sums(data, order, offsets)]
    same = all(torch.equal(a.view(torch.int64), b.view(torch.int64))
               for blk in (MA.MAX_CELLS, 8192) for a, b in zip(one, MA.rank_sums(data, order, offsets, block_cells=blk)))
    res["n22365_D5032"] = {"ms": ms, "blocked_bits_equal_the_one_call_path": bool(same),
                           "workspace_bytes": {"mmvae_rank_sum": int(L.mmvae_rank_sum_workspace_bytes(NC, DG, K)),
                                               "blocked": int(L.mmvae_rank_sum_blocked_workspace_bytes(NC, DG, K, 0))},
                           "torch_composition": _torch_row(data, labels, K, DG, one[0], one[1], few)}
    print(json.dumps(res["n22365_D5032"]), flush=True)
    del data, one, out
    # N = 131 072: the two forms of k_rsb_rank and the split over the four kernels
    n = 131072
    data = synthetic_rows(n, DG, 548, dev)
    labels, sizes = _groups(rng, n)
    order, offsets = _device_groups(labels, sizes, dev)
    calls, out = {}, None
    for name, form, phases in (("staged", 0, 0), ("in_place", 1, 0), ("through_stage", 0, 1), ("through_sort", 0, 2),
                               ("through_rank_staged", 0, 3), ("through_rank_in_place", 1, 3)):
        calls[name], out = _blocked_call(data, order, offsets, 0, out, form, phases)
    ms = _alternating_ms(calls, args.repeats)
    got = {}
    for name in ("staged", "in_place"):
        calls[name]()
        got[name] = [t.clone() for t in out[1:]]
    r2_k, tie_k = got["staged"][0], got["staged"][1]
    res["n131072_D5032"] = {
        "matrix_bytes": n * DG * 4, "workspace_bytes": int(L.mmvae_rank_sum_blocked_workspace_bytes(n, DG, K, 0)),
        "blocks": n // MA.MAX_CELLS, "ms": {"staged": ms["staged"], "in_place": ms["in_place"]},
        "split_ms": {"stage": ms["through_stage"], "sort": ms["through_sort"] - ms["through_stage"],
                     "rank_staged": ms["through_rank_staged"] - ms["through_sort"],
                     "rank_in_place": ms["through_rank_in_place"] - ms["through_sort"],
                     "reduce": ms["staged"] - ms["through_rank_staged"]},
        "forms_give_equal_bits": all(torch.equal(a.view(torch.int64), b.view(torch.int64))
                                     for a, b in zip(got["staged"], got["in_place"])),
        "torch_composition": _torch_row(data, labels, K, 256, r2_k, tie_k, 3)}
    print(json.dumps(res["n131072_D5032"]), flush=True)
    del data, got, out, calls, r2_k, tie_k
    torch.cuda.empty_cache()
    # N = 1 048 576, the cap, at D = 512
    n, Dm = MA.MAX_CELLS_BLOCKED, 512
    data = synthetic_rows(n, Dm, 549, dev)
    labels, sizes = _groups(rng, n)
    order, offsets = _device_groups(labels, sizes, dev)
    calls, out = {}, None
    for name, form in (("staged", 0), ("in_place", 1)):
        calls[name], out = _blocked_call(data, order, offsets, 0, out, form, 0)
    ms = _alternating_ms(calls, few)
    calls["staged"]()
    res["n1048576_D512"] = {"matrix_bytes": n * Dm * 4, "workspace_bytes": int(L.mmvae_rank_sum_blocked_workspace_bytes(n, Dm, K, 0)),
                            "blocks": n // MA.MAX_CELLS, "ms": ms,
                            "torch_composition": _torch_row(data, labels, K, 32, out[1].clone(), out[2].clone(), 3)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--sample", type=int, default=4)
    ap.add_argument("--blocked", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    args.out = args.out or os.path.join(ROOT, "profiles", "ranksum_blocked_time.json" if args.blocked else "ranksum_time.json")
    if args.blocked:
        return main_blocked(args)
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
    del distinct, perm
    # the most groups a call takes: every wave of the group walk owns 256 groups of two cells, none is a large one
    n_g, D_g, G_g = 8192, 512, MA.MAX_GROUPS
    many = synthetic_rows(n_g, D_g, 550, dev)
    order_g, offsets_g = _device_groups(np.repeat(np.arange(G_g), 2), np.full(G_g, 2), dev)
    res["g4096_n8192_D512"] = {"ms": _alternating_ms({"mmvae_rank_sum": _entry_call(many, order_g, offsets_g),
                                                      "blocked_block_32768": _blocked_call(many, order_g, offsets_g, 32768)[0]},
                                                     args.repeats)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

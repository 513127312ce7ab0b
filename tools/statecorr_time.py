"""Timing of the state-gene correlation at the SmartSeq size: N = 22 365 cells, D = 5032 genes, S = 2 states, on
synthetic-10x-style data (bench.py's ``synthetic_rows``: 20 % of the entries positive), the matrix resident on the device.

  * the HIP-event median of ``mmvae_state_corr`` alone (its launches, inputs already ordered by group) for G = 1 and for
    G = 92 groups of uneven sizes, and the fraction of the HBM roof that is: the matrix's bytes (N D 4, read once) over
    the time, against 8.0 TB/s (the specification) and 6.3 TB/s (what a float4 copy reaches);
  * ``corr_analysis`` end to end from the resident matrix and a device ``s_mean`` (the launches, the copy of r to the host,
    numpy's sorts), without and with ``groups=``;
  * on the host of the same run, where scipy is importable, the reference's loop -- one ``scipy.stats.pearsonr`` per (state,
    gene) over the masked cells -- on a SAMPLE of genes, extrapolated to all D (labelled ``extrapolated``; one category);
  * the device's r on the sampled genes against the fp64 restatement (tests/statecorr_restatement.py) and its gate.

    python tools/statecorr_time.py [--repeats R] [--sample GENES] [--out profiles/statecorr_time.json]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import distributed_vae_amd  # noqa: F401,E402
import statecorr_restatement as SR  # noqa: E402
from bench import synthetic_rows  # noqa: E402
from distributed_vae_amd import _native as N  # noqa: E402
from distributed_vae_amd.utils.tree_based_analysis import corr_analysis  # noqa: E402

NC, DG, S, K = 22365, 5032, 2, 92
HBM_SPEC, HBM_COPY = 8.0e12, 6.3e12


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
    ap.add_argument("--sample", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "statecorr_time.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    data = synthetic_rows(NC, DG, 546, dev)
    rng = np.random.default_rng(546)
    # states that some genes follow, offset from zero; group sizes as uneven as a taxonomy's
    state_h = (rng.normal(size=(NC, S)) * 0.7 + np.array([1.5, -2.0])).astype(np.float32)
    state = torch.from_numpy(state_h).to(dev)
    data[:, ::7] *= (1.0 + 0.3 * torch.tanh(state[:, :1]))
    weights = rng.dirichlet(np.full(K, 0.7))
    labels = rng.permutation(np.concatenate([np.arange(K), rng.choice(K, NC - K, p=weights)]))
    sizes = np.bincount(labels, minlength=K)
    order = torch.from_numpy(np.argsort(labels, kind="stable")).to(dev)
    offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)).to(dev)
    state_sorted = state.index_select(0, order)
    matrix_bytes = NC * DG * 4
    res = {"shape": {"n": NC, "D": DG, "S": S, "positive_fraction": float((data > 0).float().mean())},
           "repeats": args.repeats, "matrix_bytes": matrix_bytes, "wide_loads": bool(N.state_corr_wide(data)), "kernel": {}}
    for name, call, groups in (("G1", lambda: N.state_corr(data, state), 1),
                               ("G92", lambda: N.state_corr(data, state_sorted, order, offsets), K)):
        ms = _median_ms(call, args.repeats)
        res["kernel"][name] = {"groups": groups, "ms": ms, "matrix_bytes_per_s": matrix_bytes / (ms * 1e-3),
                               "fraction_of_hbm_spec_8.0TBs": matrix_bytes / (ms * 1e-3) / HBM_SPEC,
                               "fraction_of_hbm_copy_6.3TBs": matrix_bytes / (ms * 1e-3) / HBM_COPY,
                               "segments_at_most": groups + NC // N.STATECORR_SEG_ROWS,
                               "workspace_bytes": int(N.lib().mmvae_state_corr_workspace_bytes(NC, DG, S, groups))}
    res["kernel"]["G92"].update({"largest_group": int(sizes.max()), "smallest_group": int(sizes.min())})
    few = max(args.repeats // 4, 3)
    res["corr_analysis_ms"] = {"resident_matrix_no_groups": _median_ms(lambda: corr_analysis(state, data), few),
                               "resident_matrix_groups_92": _median_ms(lambda: corr_analysis(state, data, groups=labels), few)}
    # accuracy on a sample of genes, and the reference's loop on the same sample
    genes = np.sort(rng.choice(DG, args.sample, replace=False))
    r_dev = N.state_corr(data, state)[0][0].cpu().numpy()[:, genes]
    cell_h = data[:, torch.from_numpy(genes).to(dev)].cpu().numpy()
    want, cnt, kappa = SR.state_corr(state_h, cell_h)
    fin = np.isfinite(want[0])
    res["sample"] = {"genes": int(args.sample), "worst_device_minus_restatement": float(np.abs(r_dev - want[0])[fin].max()),
                     "largest_gate": float(SR.tolerance(cnt, kappa)[0][fin].max()),
                     "smallest_gate": float(SR.tolerance(cnt, kappa)[0][fin].min()),
                     "within_gate": bool((np.abs(r_dev - want[0])[fin] <= SR.tolerance(cnt, kappa)[0][fin]).all()),
                     "kappa_max": float(kappa[0][fin].max())}
    try:
        from scipy import stats
    except ImportError:
        stats = None
    if stats is None:
        res["host_reference_loop"] = "not measured: scipy is not importable on this host"
    else:
        t0 = time.perf_counter()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for s in range(S):
                for j in range(len(genes)):
                    hit = np.where(cell_h[:, j] > 0)[0]
                    if len(hit) > 4:
                        stats.pearsonr(state_h[hit, s], cell_h[hit, j])
        dt = time.perf_counter() - t0
        res["host_reference_loop"] = {"sample_genes": int(args.sample), "sample_s": dt, "s_extrapolated_all_genes": dt * DG / args.sample,
                                      "note": "one category; the reference repeats the loop per category on that category's cells"}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

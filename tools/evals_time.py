"""Timing of the cross-run evaluation (distributed_vae_amd._evals.evals2) on two synthetic-10x models at the SmartSeq cell
count: N = 22 365 cells, D = 5032, A = 3, C = 92, H = 100, L = 10, S = 2, batches of 5000 (the last one ragged).  HIP events
around ``evals2`` and its two phases: the encode share (both models over every batch) and the pair-statistics share (mmvae_pair_stats,
mmvae_pair_stats_finish and the one copy to the host) separately; the pair-statistics launch alone on each kernel path
(per-workgroup LDS histogram / wave-combined global atomics; C = 92 can run both) for random and for identical labels; and,
as the baseline, the host time of the reference's arithmetic (tests/evals_restatement.py::evals2, the Python loop over every
cell of every pair) on the same labels and probabilities.

    python tools/evals_time.py [--repeats R] [--out profiles/evals2_time.json]
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
import evals_restatement as ER  # noqa: E402
from distributed_vae_amd import _native as N  # noqa: E402
from distributed_vae_amd._evals import _encode_runs, evals2, pair_table  # noqa: E402
from distributed_vae_amd.nn_model import mixVAE_model  # noqa: E402
from distributed_vae_amd.utils.dataloader import DeviceLoader  # noqa: E402

NC, D, A, Cc, H, L, S, BATCH = 22365, 5032, 3, 92, 100, 10, 2, 5000


def _model(seed):
    torch.manual_seed(seed)
    m = mixVAE_model(input_dim=D, fc_dim=H, n_categories=Cc, state_dim=S, lowD_dim=L, x_drop=0.5, s_drop=0.2, n_arm=A, lam=1,
                     lam_pc=1, tau=0.005, beta=1.0, hard=False, variational=True, device="cuda", eps=1e-8, momentum=0.01,
                     ref_prior=False, loss_mode="MSE").cuda().eval()
    return m


def _median_ms(fn, repeats):
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
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "evals2_time.json"))
    args = ap.parse_args()
    fa, fb = _model(1), _model(2)
    g = torch.Generator("cpu").manual_seed(546)     # the synthetic input of SURVEY.md section 8d
    x = (torch.rand(NC, D, generator=g) < 0.2).float() * torch.randn(NC, D, generator=g).abs() * 3.0
    dl = DeviceLoader(x.cuda(), torch.arange(NC), BATCH, False, False)   # the resident matrix, batches gathered on the device
    res = {"shape": {"N": NC, "D": D, "A": A, "C": Cc, "H": H, "L": L, "S": S, "batch": BATCH},
           "pairs": A * A + A * (A - 1), "repeats": args.repeats}
    evals2(fa, fb, dl)                               # warm-up: engines, workspaces
    pairs, _ = pair_table(A, A)
    state = {}

    def encode():
        state["labels"], state["cs"], _ = _encode_runs(fa, fb, dl)

    def stats():                                     # evals2's device part behind the encode, and its one copy to the host
        counts, acc = N.pair_stats(state["labels"], state["cs"], pairs, Cc)
        fin = N.pair_stats_finish(counts, acc)
        return torch.cat((counts.to(torch.float64).reshape(-1), fin["packed"], state["cs"].to(torch.float64).reshape(-1))).cpu()

    def stats_no_probs():                            # the same without the probabilities in the copy
        counts, acc = N.pair_stats(state["labels"], state["cs"], pairs, Cc)
        fin = N.pair_stats_finish(counts, acc)
        return torch.cat((counts.to(torch.float64).reshape(-1), fin["packed"])).cpu()

    res["evals2_ms"] = _median_ms(lambda: evals2(fa, fb, dl), args.repeats)
    res["encode_ms"] = _median_ms(encode, args.repeats)
    res["pair_stats_and_copy_ms"] = _median_ms(stats, args.repeats)
    res["pair_stats_and_copy_without_probs_ms"] = _median_ms(stats_no_probs, args.repeats)
    labels, cs = state["labels"], state["cs"]
    same = labels[:1].expand(2 * A, -1).contiguous()           # every arm identical: all cells on the diagonals
    counts = torch.zeros(len(pairs), Cc, Cc, dtype=torch.int64, device="cuda")
    acc = torch.zeros(len(pairs), Cc, Cc, 2, dtype=torch.int64, device="cuda")
    rng = np.random.default_rng(0)                             # 60 % agreement over all 92 categories (tests/test_gpu_evals.py)
    base = rng.integers(0, Cc, NC)
    mixed = torch.from_numpy(np.stack([np.where(rng.random(NC) < 0.6, base, rng.integers(0, Cc - 2, NC))
                                       for _ in range(2 * A)]).astype(np.int32)).cuda()
    for name, lab in (("model_labels", labels), ("identical_labels", same), ("agree60_labels", mixed)):
        for path in ("lds", "wave"):
            res[f"pair_stats_{path}_{name}_us"] = 1e3 * _median_ms(
                lambda: N.pair_stats(lab, cs, pairs, Cc, counts, acc, path=path), 5 * args.repeats)
    res["pair_stats_finish_us"] = 1e3 * _median_ms(lambda: N.pair_stats_finish(counts, acc), 5 * args.repeats)
    res["distinct_labels_per_arm"] = [int(torch.unique(labels[a]).numel()) for a in range(2 * A)]
    # the baseline: the reference's host loops on the same labels and probabilities
    cs64 = cs.double().cpu().numpy()
    preds = labels.cpu().numpy().astype(np.float64) + 1.0
    try:
        import scipy.optimize  # noqa: F401  (the restatement's assignment solver beyond K = 7)
    except ImportError:
        from distributed_vae_amd._utils import reassign
        ER.reassign = reassign
    t0 = time.perf_counter()
    ER.evals2(preds[:A], preds[A:], cs64[:A], cs64[A:], np.zeros(0, np.int64), Cc)
    res["host_restatement_evals2_s"] = time.perf_counter() - t0
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

"""Timing of the mutual-information evaluation at the SmartSeq size: N = 22 365 cells, A = 3 arms, C = 92 categories, F = 115
cell types.  HIP-event medians of the counts launch (mmvae_mutinfo_counts on each kernel path), the adjusted-MI launch
(mmvae_ami_binary with the log-gamma table and with log-gamma per term), ``mutinfo_arms`` end to end from host arrays, and
``summarize_inference``'s post-processing for one file (a stub trainer that returns a ready ``eval_model`` dictionary, so only
the pair matrices and the assembly are timed).  Baselines of the same run: the host loops of tests/mutinfo_restatement.py --
``summarize`` for one file in full, the adjusted MI on a SAMPLE of the tables extrapolated to all of them -- and, where sklearn
is importable, the reference's per-call loop on a sample of tables, extrapolated likewise (both labelled ``extrapolated``).

    python tools/mutinfo_time.py [--repeats R] [--sample T] [--out profiles/mutinfo_time.json]
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
import mutinfo_restatement as MR  # noqa: E402
from distributed_vae_amd import _native as N  # noqa: E402
from distributed_vae_amd.eval_models import summarize_inference  # noqa: E402
from distributed_vae_amd.evaluation import mutinfo_arms  # noqa: E402

NC, A, Cc, F, S, L = 22365, 3, 92, 115, 2, 10


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


class _Stub:
    ref_prior, n_arm, n_categories = False, A, Cc

    def __init__(self, ev):
        self.ev, self.device = ev, torch.device("cuda")

    def load_model(self, file):
        pass

    def eval_model(self, dl):
        return self.ev


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--sample", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mutinfo_time.json"))
    args = ap.parse_args()
    rng = np.random.default_rng(546)
    cell_type = rng.integers(0, F, NC)
    targets = np.eye(F, dtype=np.uint8)[cell_type]
    z = rng.normal(size=(A, NC, Cc)).astype(np.float32)
    for a in range(A):                                        # 60 % of the cells follow their type, per arm
        hit = rng.random(NC) < 0.6
        z[a, hit, cell_type[hit] % Cc] += 4
    labels_h = np.argmax(z, -1)
    lab, tg = torch.from_numpy(labels_h.astype(np.int32)).cuda(), torch.from_numpy(targets).cuda()
    res = {"shape": {"N": NC, "A": A, "C": Cc, "F": F}, "repeats": args.repeats, "tables": A * F * Cc}
    out = N.mutinfo_counts(lab, tg, Cc)
    for path in ("lds", "global"):
        res[f"counts_{path}_us"] = 1e3 * _median_ms(lambda: N.mutinfo_counts(lab, tg, Cc, out=out, path=path), 5 * args.repeats)
    counts, t_sum, p_sum = N.mutinfo_counts(lab, tg, Cc)
    want = MR.counts(labels_h, targets, F, Cc)
    assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip((counts, t_sum, p_sum), want))
    c_h, t_h, p_h = want
    res["terms"] = int(sum(4 * min(int(t_h[f]), int(p_h[a, c])) for a in range(A) for f in range(F) for c in range(Cc)))
    res["ami_table_us"] = 1e3 * _median_ms(lambda: N.ami_binary(counts, t_sum, p_sum, NC, table=True), args.repeats)
    res["ami_per_term_us"] = 1e3 * _median_ms(lambda: N.ami_binary(counts, t_sum, p_sum, NC, table=False), args.repeats)
    z64 = z.astype(np.float64)
    res["mutinfo_arms_ms"] = _median_ms(lambda: mutinfo_arms(z64, targets), args.repeats)
    ev = {"state_mu": np.zeros((A, NC, S)), "state_var": np.zeros((A, NC, S)), "predicted_label": labels_h + 1.0,
          "total_loss_rec": np.ones(A), "total_dist_z": np.float64(0.1), "total_dist_qz": np.float64(0.2),
          "data_indx": np.arange(NC, dtype=np.float64), "z_prob": z64, "x_low": np.zeros((A, NC, L)),
          "prune_indx": np.array([3, 50])}
    stub = _Stub(ev)
    sys.stdout, keep = open(os.devnull, "w"), sys.stdout      # summarize_inference prints one line per file
    try:
        res["summarize_post_ms"] = _median_ms(lambda: summarize_inference(stub, ["run/model.pth"], None), args.repeats)
    finally:
        sys.stdout = keep
    # baselines on the host, same inputs
    t0 = time.perf_counter()
    MR.summarize([ev], A, Cc)
    res["host_restatement_summarize_s"] = time.perf_counter() - t0
    occupied = [(a, f, c) for a in range(A) for c in range(Cc) if p_h[a, c] for f in range(F)]
    pick = [occupied[i] for i in rng.choice(len(occupied), args.sample, replace=False)]
    t0 = time.perf_counter()
    mine = [MR.ami_2x2(c_h[a, f, c], t_h[f], p_h[a, c], NC)[0] for a, f, c in pick]
    per = (time.perf_counter() - t0) / len(pick)
    res["host_restatement_ami_s_extrapolated"] = per * len(occupied)
    dev = N.ami_binary(counts, t_sum, p_sum, NC).cpu().numpy()
    res["sample_worst_device_minus_restatement"] = float(max(abs(dev[a, f, c] - m) for (a, f, c), m in zip(pick, mine)))
    try:
        from sklearn.metrics import adjusted_mutual_info_score
    except ImportError:
        adjusted_mutual_info_score = None
    if adjusted_mutual_info_score is not None:
        t0 = time.perf_counter()
        theirs = [adjusted_mutual_info_score(targets[:, f], (labels_h[a] == c).astype(np.float64)) for a, f, c in pick]
        per = (time.perf_counter() - t0) / len(pick)
        res["host_sklearn_loop_s_extrapolated"] = per * len(occupied)
        res["sample_worst_device_minus_sklearn"] = float(max(abs(dev[a, f, c] - m) for (a, f, c), m in zip(pick, theirs)))
    res["sample_tables"] = len(pick)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

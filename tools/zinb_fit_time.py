"""Timing of the ZINB head fit on synthetic inputs of tools/zinb_time.py's kind (d10 = relu of
normals, layers spread to +-6.4, X = log1p(counts <= 1000) with about 70 % zeros).

  * HIP-event medians of ``mmvae_zinb_head_grads`` for one arm at N = 5000, D = 5032, H = 100 (all three heads, and the two
    gates alone), beside ``mmvae_zinb_nll`` on the same inputs (the forward half of the same work);
  * the same gradients composed from torch ops with autograd on the same GPU in float32 -- the reference's ``zinb_loss`` on
    ``F.linear`` heads, ``backward()`` -- with its peak allocation above the inputs.  This is a baseline, not library code;
  * wall clock of one epoch of ``cpl_mixVAE.fit_zinb_heads`` over a resident 22 365-cell matrix (``DeviceLoader``, batches of
    --batch cells, two arms), after one warm-up epoch.

    python tools/zinb_fit_time.py [--repeats R] [--only grads] [--segments S] [--out profiles/zinb_fit_time.json]

``--only grads`` runs the kernel a few times and writes nothing (the window a counter or kernel-trace run wants)."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import distributed_vae_amd  # noqa: F401,E402
from distributed_vae_amd import _native as N  # noqa: E402
import zinb_restatement as ZR  # noqa: E402

NB, NC, D, H, SEED = 5000, 22365, 5032, 100, 0
DEV = "cuda:0"


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


def _with_peak(fn, repeats):
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ms = _median_ms(fn, repeats)
    return {"ms": ms, "peak_bytes_above_inputs": int(torch.cuda.max_memory_allocated() - base)}


def _inputs(n):
    g = torch.Generator().manual_seed(SEED)
    d10 = torch.relu(torch.randn(n, H, generator=g))
    L = ZR.spread_layers(d10[:512], D, g)
    for j in (2, 4):
        L[j], L[j + 1] = L[j] * 0.8, L[j + 1] * 0.8
    return d10.to(DEV), [t.to(DEV) for t in L], ZR.counts_matrix(n, D, g).to(DEV)


def _torch_grads(d10, L, X):
    """The reference's arithmetic with autograd: float32 heads, zinb_loss, backward."""
    P = [t.detach().clone().requires_grad_() for t in L]
    ZR.terms(*ZR.heads(d10, *P), X).mean().backward()
    return [p.grad for p in P]


def grads(out, repeats, n, segments, only=False):
    d10, L, X = _inputs(n)
    if only:
        for _ in range(3):
            N.zinb_head_grads(d10, *L, X, segments=segments)
        torch.cuda.synchronize()
        return
    bufs = {h: (torch.empty(D, H, device=DEV), torch.empty(D, device=DEV)) for h in N.ZINB_HEADS}
    r = {"segments": N.zinb_head_grads_segments(n, D, segments),
         "workspace_bytes": int(N.lib().mmvae_zinb_head_grads_workspace_bytes(n, D, H, segments)),
         "head_grads_three_heads": _with_peak(lambda: N.zinb_head_grads(d10, *L, X, segments=segments, out=bufs), repeats),
         "head_grads_two_gates": _with_peak(lambda: N.zinb_head_grads(d10, *L, X, heads=("p", "r"), segments=segments, out=bufs), repeats),
         "zinb_nll": _with_peak(lambda: N.zinb_nll(d10, *L, X), repeats),
         "torch_autograd_float32": _with_peak(lambda: _torch_grads(d10, L, X), max(3, repeats // 3))}
    r["ratio_torch_over_kernel"] = r["torch_autograd_float32"]["ms"] / r["head_grads_three_heads"]["ms"]
    r["elements_per_s"] = n * D / (r["head_grads_three_heads"]["ms"] * 1e-3)
    # a check of the tool, not a gate: the two agree to float32's error on the largest entry of each gradient
    dev, _, _ = N.zinb_head_grads(d10, *L, X, segments=segments)
    ref = _torch_grads(d10, L, X)
    # (fc11's gradient is led by the few elements whose r is barely above eps, where psi(r) ~ -1 / r follows the last bits
    # of the float32 pre-activation: there the two float32 evaluations differ visibly, as either does from float64)
    r["largest_difference_from_torch_over_largest_entry"] = {
        h: max(float((dev[h][k] - ref[2 * j + k]).abs().max() / ref[2 * j + k].abs().max()) for k in (0, 1))
        for j, h in enumerate(N.ZINB_HEADS)}
    out["head_grads_one_arm"] = r


def epoch(out, n, batch):
    from distributed_vae_amd.cpl_mixvae import cpl_mixVAE
    from distributed_vae_amd.utils.dataloader import DeviceLoader
    torch.manual_seed(SEED)
    t = cpl_mixVAE(saving_folder="", device=0, save_flag=False)
    t.init_model(n_categories=92, state_dim=2, input_dim=D, fc_dim=H, lowD_dim=10, n_arm=2, temp=1.0, tau=0.005, mode="ZINB")
    data = ZR.counts_matrix(n, D, torch.Generator().manual_seed(SEED + 1)).to(DEV)
    dl = DeviceLoader(data, torch.arange(n), batch, False, False)
    res = t.fit_zinb_heads(dl, 1)
    w = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = t.fit_zinb_heads(dl, 1, state=res["state"])
        torch.cuda.synchronize()
        w.append((time.perf_counter() - t0) * 1e3)
    out["fit_zinb_heads_epoch"] = {"cells": n, "batch": batch, "batches": len(dl), "arms": 2, "wall_ms_median_of_3": sorted(w)[1],
                                   "train_loss_last_epoch": [float(v) for v in res["train_loss"][-1]]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--only", choices=["grads"], default=None)
    ap.add_argument("--segments", type=int, default=0)
    ap.add_argument("--cells", type=int, default=NC)
    ap.add_argument("--batch", type=int, default=NB)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "zinb_fit_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("zinb_fit_time needs a GPU")
    out = {"shape": {"N": a.batch, "D": D, "H": H}, "repeats": a.repeats, "device": torch.cuda.get_device_name(0)}
    if a.only == "grads":
        return grads(out, a.repeats, a.batch, a.segments, only=True)
    grads(out, a.repeats, a.batch, a.segments)
    epoch(out, a.cells, a.batch)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()

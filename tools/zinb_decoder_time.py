"""Timing of the ZINB decoder fit on synthetic inputs of tools/zinb_fit_time.py's kind (layers spread
to +-6.4, X = log1p(counts <= 1000) with about 70 % zeros), the trunk at ``nn.Linear``'s default initialisation on a
[softmax | normal] input of C + S = 94 columns.

  * HIP-event medians per launch for one arm at N = 5000, D = 5032, H = 100: ``mmvae_zinb_d10_grad`` (all three heads, and
    the two gates alone), ``mmvae_zinb_head_grads`` on the same inputs in the same run (the kernel it mirrors), and
    ``mmvae_decoder_trunk_grads`` with and without gzin;
  * the same gradients composed from torch ops with autograd on the same GPU in float32 -- gd10 alone, and the whole decoder
    (trunk, heads) from zin -- with the peak allocation above the inputs.  A baseline, not library code;
  * wall clock of one epoch of ``cpl_mixVAE.fit_zinb_decoder`` over a resident 22 365-cell matrix (``DeviceLoader``, batches
    of --batch cells, two arms), after one warm-up epoch, beside ``fit_zinb_heads`` on the same loader.

    python tools/zinb_decoder_time.py [--repeats R] [--only d10] [--segments S] [--out profiles/zinb_decoder_time.json]

``--only d10`` runs that kernel a few times and writes nothing (the window a counter or kernel-trace run wants)."""
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
import zinb_decoder_restatement as RD  # noqa: E402
import zinb_restatement as ZR  # noqa: E402
from zinb_fit_time import _median_ms, _with_peak  # noqa: E402

NB, NC, D, H, Z, LD, SEED = 5000, 22365, 5032, 100, 94, 10, 0
DEV = "cuda:0"


def _inputs(n):
    g = torch.Generator().manual_seed(SEED)
    zin = torch.cat([torch.softmax(2 * torch.randn(n, Z - 2, generator=g), 1), torch.randn(n, 2, generator=g)], 1)
    params = RD.default_trunk(Z, LD, H, SEED)
    acts = RD.forward(zin, params)
    L = ZR.spread_layers(acts[5][:512], D, g)
    for j in (2, 4):
        L[j], L[j + 1] = L[j] * 0.8, L[j + 1] * 0.8
    return [a.to(DEV) for a in acts], [p.to(DEV) for p in params], [t.to(DEV) for t in L], ZR.counts_matrix(n, D, g).to(DEV)


def _torch_gd10(d10, L, X):
    x = d10.detach().clone().requires_grad_()
    ZR.terms(*ZR.heads(x, *L), X).mean().backward()
    return x.grad


def _torch_decoder(zin, params, L, X):
    P = [t.detach().clone().requires_grad_() for t in params + L]
    ZR.terms(*ZR.heads(RD.forward(zin, P[:10])[5], *P[10:]), X).mean().backward()
    return [p.grad for p in P]


def launches(out, repeats, n, segments, only=False):
    acts, params, L, X = _inputs(n)
    d10 = acts[5]
    if only:
        for _ in range(3):
            N.zinb_d10_grad(d10, *L, X, segments=segments)
        torch.cuda.synchronize()
        return
    gd10 = torch.empty(n, H, device=DEV)
    bufs = {h: (torch.empty(D, H, device=DEV), torch.empty(D, device=DEV)) for h in N.ZINB_HEADS}
    tg = [torch.empty_like(p) for p in params]
    N.zinb_d10_grad(d10, *L, X, segments=segments, out=gd10)
    r = {"d10_segments": N.zinb_d10_grad_segments(n, D, segments),
         "d10_workspace_bytes": int(N.lib().mmvae_zinb_d10_grad_workspace_bytes(n, D, H, segments)),
         "trunk_segments": N.decoder_trunk_grads_segments(n),
         "trunk_workspace_bytes": int(N.lib().mmvae_decoder_trunk_grads_workspace_bytes(n, Z, LD, H, 0)),
         "d10_grad_three_heads": _with_peak(lambda: N.zinb_d10_grad(d10, *L, X, segments=segments, out=gd10), repeats),
         "d10_grad_two_gates": _with_peak(lambda: N.zinb_d10_grad(d10, *L, X, heads=("p", "r"), segments=segments, out=gd10), repeats),
         "head_grads_three_heads": _with_peak(lambda: N.zinb_head_grads(d10, *L, X, out=bufs), repeats),
         "trunk_grads_with_gzin": _with_peak(lambda: N.decoder_trunk_grads(acts, params, gd10, out=tg), repeats),
         "trunk_grads_without_gzin": _with_peak(lambda: N.decoder_trunk_grads(acts, params, gd10, out=tg, want_gzin=False), repeats),
         "torch_autograd_float32_gd10": _with_peak(lambda: _torch_gd10(d10, L, X), max(3, repeats // 3)),
         "torch_autograd_float32_whole_decoder": _with_peak(lambda: _torch_decoder(acts[0], params, L, X), max(3, repeats // 3))}
    r["device_whole_decoder_ms"] = r["head_grads_three_heads"]["ms"] + r["d10_grad_three_heads"]["ms"] + r["trunk_grads_with_gzin"]["ms"]
    r["ratio_torch_over_device_whole_decoder"] = r["torch_autograd_float32_whole_decoder"]["ms"] / r["device_whole_decoder_ms"]
    r["ratio_d10_over_head_grads"] = r["d10_grad_three_heads"]["ms"] / r["head_grads_three_heads"]["ms"]
    # a check of the tool, not a gate: device and torch agree to float32's error on the largest entry of each gradient
    N.zinb_d10_grad(d10, *L, X, segments=segments, out=gd10)
    dev, _ = N.decoder_trunk_grads(acts, params, gd10)
    ref = _torch_decoder(acts[0], params, L, X)
    r["largest_difference_from_torch_over_largest_entry"] = {
        "d10": float((gd10 - _torch_gd10(d10, L, X)).abs().max() / gd10.abs().max()),
        **{f"{RD.TRUNK[k // 2]}.{'bias' if k % 2 else 'weight'}": float((dev[k] - ref[k]).abs().max() / ref[k].abs().max()) for k in range(10)}}
    out["launches_one_arm"] = r


def epoch(out, n, batch):
    from distributed_vae_amd.cpl_mixvae import cpl_mixVAE
    from distributed_vae_amd.utils.dataloader import DeviceLoader
    data = ZR.counts_matrix(n, D, torch.Generator().manual_seed(SEED + 1)).to(DEV)
    dl = DeviceLoader(data, torch.arange(n), batch, False, False)
    for name in ("fit_zinb_decoder", "fit_zinb_heads"):
        torch.manual_seed(SEED)
        t = cpl_mixVAE(saving_folder="", device=0, save_flag=False)
        t.init_model(n_categories=92, state_dim=2, input_dim=D, fc_dim=H, lowD_dim=LD, n_arm=2, temp=1.0, tau=0.005, mode="ZINB")
        fit = getattr(t, name)
        res = fit(dl, 1)
        w = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = fit(dl, 1, state=res["state"])
            torch.cuda.synchronize()
            w.append((time.perf_counter() - t0) * 1e3)
        out[name + "_epoch"] = {"cells": n, "batch": batch, "batches": len(dl), "arms": 2, "wall_ms_median_of_3": sorted(w)[1],
                                "train_loss_last_epoch": [float(v) for v in res["train_loss"][-1]]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--only", choices=["d10"], default=None)
    ap.add_argument("--segments", type=int, default=0)
    ap.add_argument("--cells", type=int, default=NC)
    ap.add_argument("--batch", type=int, default=NB)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "zinb_decoder_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("zinb_decoder_time needs a GPU")
    out = {"shape": {"N": a.batch, "D": D, "H": H, "C+S": Z, "L": LD}, "repeats": a.repeats, "device": torch.cuda.get_device_name(0)}
    if a.only == "d10":
        return launches(out, a.repeats, a.batch, a.segments, only=True)
    launches(out, a.repeats, a.batch, a.segments)
    epoch(out, a.cells, a.batch)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()

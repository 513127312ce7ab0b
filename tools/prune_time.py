"""Timing of the masked fused train step of the pruning phase (mixVAE_model.fused_train_step(mask=): mmvae_train_step under
mmvae_hyper.cat_mask, then mmvae_prune_apply on parameters, gradients and both Adam moments) at the headline shape
(A = 2, B = D = 5000, H = 100, C = 92, S = 2, L = 10) with ten categories pruned, against the unmasked step of the same build
and against mmvae_prune_apply alone.  HIP events around blocks of steps on a resident batch, median over the blocks.

    python tools/prune_time.py [--steps K] [--blocks R] [--dtype fp32|bf16]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import distributed_vae_amd  # noqa: F401,E402
from distributed_vae_amd.cpl_mixvae import FusedAdam  # noqa: E402
from distributed_vae_amd.nn_model import mixVAE_model  # noqa: E402

A, B, D, H, L, Cc, S = 2, 5000, 5000, 100, 10, 92, 2
PRUNED = list(range(3, 92, 9))[:10]          # ten categories, both words of the mask's first 92 bits


def _block_ms(fn, steps, blocks):
    for _ in range(steps):                    # warm-up: engine, streams, clocks
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(blocks):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        t.append(e0.elapsed_time(e1) / steps)
    t.sort()
    return t[len(t) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--dtype", default="fp32")
    args = ap.parse_args()
    torch.manual_seed(0)
    m = mixVAE_model(input_dim=D, fc_dim=H, n_categories=Cc, state_dim=S, lowD_dim=L, x_drop=0.5, s_drop=0.2, n_arm=A, lam=1,
                     lam_pc=1, tau=0.005, beta=1.0, hard=False, variational=True, device="cuda", eps=1e-8, momentum=0.01,
                     ref_prior=False, loss_mode="MSE").cuda().train()
    m.gemm_dtype = args.dtype
    opt = FusedAdam(m, lr=1e-3)
    g = torch.Generator("cpu").manual_seed(546)     # the synthetic input of SURVEY.md section 8d
    x = ((torch.rand(B, D, generator=g) < 0.2).float() * torch.randn(B, D, generator=g).abs() * 3.0).cuda()
    xs = x.expand(A, -1, -1)
    kept = [k for k in range(Cc) if k not in PRUNED]
    res = {"shape": [A, B, D, H, L, Cc, S], "pruned": PRUNED, "dtype": args.dtype}
    # A / B / A: the unmasked step on either side of the masked one
    res["unmasked_ms"] = _block_ms(lambda: m.fused_train_step(xs, 1.0, opt, do_adam=True), args.steps, args.blocks)
    m.prune_apply(kept, opt)
    res["masked_ms"] = _block_ms(lambda: m.fused_train_step(xs, 1.0, opt, do_adam=True, mask=kept), args.steps, args.blocks)
    res["unmasked_again_ms"] = _block_ms(lambda: m.fused_train_step(xs, 1.0, opt, do_adam=True), args.steps, args.blocks)
    res["prune_apply_alone_us"] = 1e3 * _block_ms(lambda: m.prune_apply(kept, opt), 200, args.blocks)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

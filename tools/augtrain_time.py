#!/usr/bin/env python
"""Times the augmenter's training step on the device beside torch's float32 autograd of the same objective, same GPU, same
process, alternating A / B / A / B, medians of 5 windows (device events), and writes profiles/augtrain_time.json.

    python tools/augtrain_time.py                   # production shape: D 5032, B 5000, NZ 50, Z 10, n_dim 500
    python tools/augtrain_time.py --steps-only 3    # a few device steps and nothing else: the run to put under a kernel trace

The per-launch breakdown is not made here (tracing slows the host, so it is a run of its own): it is the kernel trace of the
second form,

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o aug -- python tools/augtrain_time.py --steps-only 3

whose OUT/aug_kernel_stats.csv, without torch's own kernels, is profiles/augtrain_kernel_stats.csv (calls and time per kernel
over the three steps)."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main(argv=None) -> int:
    p = argparse.ArgumentParser()
    p.add_argument("--shape", type=int, nargs=5, default=[50, 10, 5032, 500, 5000], metavar=("NZ", "Z", "D", "N_DIM", "B"))
    p.add_argument("--windows", type=int, default=5)
    p.add_argument("--steps", type=int, default=3, help="steps per window")
    p.add_argument("--steps-only", type=int, default=0)
    p.add_argument("--epoch-cells", type=int, default=22365)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "augtrain_time.json"))
    a = p.parse_args(argv)
    sys.path.insert(0, ROOT)
    import torch

    import distributed_vae_amd  # noqa: F401
    from distributed_vae_amd.augmentation import Augmenter_smartseq, train_augmenter
    from tests import augtrain_restatement as R
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    NZ, Z, D, n_dim, B = a.shape
    sd = R.random_state_dict(NZ, Z, D, n_dim, 1)
    x = R.synthetic_batch(B, D, 2).to(dev)
    net = Augmenter_smartseq(NZ, Z, D, n_dim)
    net.load_state_dict(sd)
    net.to(dev).train()
    state = net.train_state(dev)

    def dev_step(stat):
        net.train_step(x, state, stat_pass=stat)

    if a.steps_only:
        for _ in range(a.steps_only):
            dev_step(True)
        torch.cuda.synchronize()
        return 0

    ref = torch.nn.Module()
    P = {k: torch.nn.Parameter(v.to(dev)) for k, v in sd.items() if k in R.PARAM_ORDER}
    run = {k: v.to(dev) for k, v in sd.items() if k not in R.PARAM_ORDER}
    for i, (k, v) in enumerate(P.items()):
        ref.register_parameter(f"p{i}", v)
    opt = torch.optim.Adam(ref.parameters(), lr=1e-3)

    def torch_step(stat):
        nonlocal run
        for _ in range(2 if stat else 1):
            last = _ == (1 if stat else 0)
            mask = torch.rand(B, D, device=dev) >= 0.5
            z0, eps = torch.randn(B, NZ, device=dev), torch.randn(B, Z, device=dev)
            upd = {}
            if not last:
                with torch.no_grad():
                    R.forward(P, run, x, mask, z0, eps, 0.5, upd=upd)
            else:
                opt.zero_grad(set_to_none=True)
                _, xa = R.forward(P, run, x, mask, z0, eps, 0.5, upd=upd)
                (0.25 * ((xa - x) ** 2).mean()).backward()
                opt.step()
            run = upd

    def window(fn, stat):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.steps):
            fn(stat)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.steps

    res = {"shape": {"NZ": NZ, "Z": Z, "D": D, "n_dim": n_dim, "B": B}, "windows": a.windows, "steps_per_window": a.steps,
           "device": torch.cuda.get_device_name(0)}
    for stat in (True, False):
        for fn in (dev_step, torch_step):
            fn(stat)
            fn(stat)                    # warm-up: code objects, allocator, library algorithm choice
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        td, tt = [], []
        for _ in range(a.windows):
            td.append(window(dev_step, stat))
            tt.append(window(torch_step, stat))
        key = "with_stat_pass" if stat else "without_stat_pass"
        res[key] = {"device_ms": statistics.median(td), "device_ms_all": td, "torch_fp32_ms": statistics.median(tt), "torch_fp32_ms_all": tt,
                    "torch_over_device": statistics.median(tt) / statistics.median(td),
                    "peak_bytes_above_resident_both": torch.cuda.max_memory_allocated(dev) - base}
    # torch's peak temporaries alone
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    torch_step(True)
    torch.cuda.synchronize()
    res["torch_peak_temporaries_bytes"] = torch.cuda.max_memory_allocated(dev) - base
    res["device_workspace_bytes"] = net._tws.numel() * 4
    # coarse breakdown of the device step: the training-mode forward alone against the step
    net.set_explicit_noise(None, None)
    fwd = []
    for _ in range(a.windows):
        fwd.append(window(lambda s: net(x, False, 1.0), False))
    res["device_forward_only_ms"] = statistics.median(fwd)
    # an epoch over epoch_cells x D through the driver (full batches)
    n = a.epoch_cells
    data = R.synthetic_batch(n, D, 3).to(dev)
    loader = [(data[i * B:(i + 1) * B], None) for i in range(n // B)] + ([(data[(n // B) * B:], None)] if n % B >= 2 else [])
    par = {"num_epochs": 1, "learning_rate": 1e-3, "lambda": [1, 0.5, 0.1, 0.5], "batch_size": B, "save": False, "saving_path": "",
           "num_n": NZ, "num_z": Z, "n_features": D, "initial_w": False, "mode": "MSE"}
    train_augmenter(net, None, loader, par, dev)          # warm-up of the remainder batch's shape
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    train_augmenter(net, None, loader, par, dev)
    e1.record()
    torch.cuda.synchronize()
    res["epoch"] = {"cells": n, "batches": len(loader), "ms": e0.elapsed_time(e1)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""Per-call timing of mixVAE_model.decoder and state_changes (mmvae_decode / mmvae_state_changes) at the production shape
(A = 2, D = 5000, H = 100, C = 92, S = 2, L = 10): decode of N = 5000 rows per arm on each GEMM engine, and a traversal of
one cell with n_samp = 100.  Run under `rocprofv3 --kernel-trace --stats` for the per-kernel table (profiles/decode_*).

    python tools/decode_time.py [--reps R]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import distributed_vae_amd  # noqa: F401,E402
from distributed_vae_amd.nn_model import mixVAE_model  # noqa: E402

A, D, H, L, Cc, S, N = 2, 5000, 100, 10, 92, 2, 5000


def _events_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
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
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    torch.manual_seed(0)
    m = mixVAE_model(input_dim=D, fc_dim=H, n_categories=Cc, state_dim=S, lowD_dim=L, x_drop=0.5, s_drop=0.2, n_arm=A, lam=1,
                     lam_pc=1, tau=0.005, beta=1.0, hard=False, variational=True, device="cuda", eps=1e-8, momentum=0.01,
                     ref_prior=False, loss_mode="MSE").cuda().eval()
    c = torch.softmax(3 * torch.randn(N, Cc, device="cuda"), -1)
    s = torch.randn(N, S, device="cuda")
    x = torch.relu(torch.randn(1, D, device="cuda"))
    res = {}
    for engine in ("fp32_mfma", "bf16", "fp32x3"):
        m.gemm_dtype = engine
        # both arms, as the reference's callers decode them: one call per arm
        res[f"decode_{engine}_ms"] = _events_ms(lambda: [m.decoder(c, s, a) for a in range(A)], args.reps)
    m.gemm_dtype = "fp32"
    res["state_changes_ms"] = _events_ms(lambda: m.state_changes(x, 1, 1.0, n_samp=100), args.reps)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

"""Build container only: run the REAL reference (oracle/ref_loader) decoder and state_changes on a small model and commit
what it computed as the data-only fixture tests/golden/decode_a2.npz (tests/test_decode_cpu.py, tests/test_gpu_decode.py).

Holds, for one model (A = 2, D = 64, H = 16, L = 4, C = 6, S = 2; BatchNorm running statistics randomised so that eval
mode is not the identity), in fp64 and fp32:
  sd/<key>                 the state dict (parameters and BatchNorm buffers, fp64)
  dec/c, dec/s             decoder inputs per arm [A, N, C] / [A, N, S]
  <tag>/dec/out            decoder(c[a], s[a], a) per arm [A, N, D]
  sc/x, sc/u, sc/d_s       state_changes input (one cell), its recorded torch.rand_like draws [A, n_samp, 1], d_s
  <tag>/sc/recon           recon_x [A, n_samp, D] as returned (reordered)
  <tag>/sc/sorted          state_smp_sorted [A, n_samp]
  sc/perm                  torch.zeros(n_samp).sort() indices the reference applied

    python -m tools.gen_golden_decode
"""
import os

import numpy as np
import torch

from oracle import ref_loader as RL

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
A, D, H, L, C, S = 2, 64, 16, 4, 6, 2
N_DEC, N_SAMP, D_S = 9, 100, 1


def _model(ref, dtype):
    torch.manual_seed(5)
    m = ref.mixVAE_model(input_dim=D, fc_dim=H, n_categories=C, state_dim=S, lowD_dim=L, x_drop=0.5, s_drop=0.2, n_arm=A,
                         lam=1, lam_pc=1, tau=0.005, beta=1.0, hard=False, variational=True, device="cpu", eps=1e-8,
                         momentum=0.01, ref_prior=False, loss_mode="MSE")
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():
        for name, buf in m.named_buffers():
            if name.endswith("running_mean"):
                buf.copy_(0.3 * torch.randn(buf.shape, generator=g, dtype=torch.float64))
            elif name.endswith("running_var"):
                buf.copy_(0.5 + torch.rand(buf.shape, generator=g, dtype=torch.float64))
        for p in m.parameters():   # a little larger than the default init, so that the ReLUs see both signs
            p.mul_(1.5)
    return m.to(dtype).eval()


def main():
    ref = RL.load_reference_nn_model()
    g = torch.Generator().manual_seed(3)
    dec_c = torch.softmax(3 * torch.randn(A, N_DEC, C, generator=g, dtype=torch.float64), -1)
    dec_s = torch.randn(A, N_DEC, S, generator=g, dtype=torch.float64)
    x = torch.relu(torch.randn(1, D, generator=g, dtype=torch.float64)) * 2
    u = torch.rand(A, N_SAMP, 1, generator=g, dtype=torch.float64)
    out = {"dec/c": dec_c.numpy(), "dec/s": dec_s.numpy(), "sc/x": x.numpy(), "sc/u": u.numpy(), "sc/d_s": np.int64(D_S),
           "sc/perm": torch.zeros(N_SAMP).sort()[1].numpy(), "cfg": np.array([A, 1, D, H, L, C, S], np.int64)}
    for tag, dtype in (("f64", torch.float64), ("f32", torch.float32)):
        old = torch.get_default_dtype()
        torch.set_default_dtype(dtype)
        try:
            m = _model(ref, dtype)
            if tag == "f64":
                sd64 = {k: v.clone() for k, v in m.state_dict().items()}
                for k, v in sd64.items():
                    out[f"sd/{k}"] = v.detach().cpu().numpy().copy()
            else:   # the same model, rounded (init draws differ between dtypes)
                m.load_state_dict({k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd64.items()})
            with torch.no_grad():
                out[f"{tag}/dec/out"] = np.stack([m.decoder(dec_c[a].to(dtype), dec_s[a].to(dtype), a).numpy() for a in range(A)])
                draws = list(u.to(dtype).reshape(A * N_SAMP, 1))
                real = torch.rand_like
                torch.rand_like = lambda t, **kw: draws.pop(0).reshape(t.shape).to(t.dtype)
                try:
                    recon, srt = m.state_changes(x.to(dtype), D_S, 1.0, n_samp=N_SAMP)
                finally:
                    torch.rand_like = real
                assert not draws
            out[f"{tag}/sc/recon"] = recon.detach().numpy().astype(np.float64)
            out[f"{tag}/sc/sorted"] = srt.detach().numpy().astype(np.float64)
        finally:
            torch.set_default_dtype(old)
    np.savez_compressed(os.path.join(GOLDEN, "decode_a2.npz"), **out)
    print({k: np.asarray(v).shape for k, v in out.items() if not k.startswith("sd/")})


if __name__ == "__main__":
    main()

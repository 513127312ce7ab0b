"""Build container only: run the REAL reference (oracle/ref_loader) ``decoder_zinb`` and ``zinb_loss`` on small ZINB models and
commit what they computed as the data-only fixture tests/golden/zinb_kat.npz (tests/test_zinb_cpu.py, tests/test_gpu_zinb.py).

Per case ``<m>`` (``cases`` lists the names) and dtype tag f64 / f32:
  <m>/cfg                  A, N, D, H, L, C, S
  <m>/sd/<key>             the state dict (fp64; the f32 model is this one rounded).  fc11_p / fc11_r are scaled so that their
                           pre-activations on the decoded codes spread to +-8 and stay within it
  <m>/c, <m>/s             decoder inputs per arm [A, N, C] / [A, N, S]
  <m>/X                    log1p(counts) float32 [N, D]: counts <= 1000, about 70 % zeros, row 0 all zero, row 1 all positive
  <m>/<tag>/rec, p, r      decoder_zinb(c[a], s[a], a) per arm [A, N, D]
  <m>/<tag>/loss           zinb_loss(rec[a], p[a], r[a], X) per arm [A]
  <m>/<tag>/terms          zinb_loss of every single element (its mean is the element's term) [A, N, D]

    python -m tools.gen_golden_zinb
"""
import os

import numpy as np
import torch

from oracle import ref_loader as RL
from tests import zinb_restatement as ZR

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
#         A, N,  D,  H, L, C, S
CASES = {"m0": (2, 21, 70, 20, 4, 6, 2), "m1": (2, 5, 33, 7, 3, 4, 2)}
SPREAD = 8.0


def _model(ref, cfg, seed):
    A, _, D, H, L, C, S = cfg
    torch.manual_seed(seed)
    m = ref.mixVAE_model(input_dim=D, fc_dim=H, n_categories=C, state_dim=S, lowD_dim=L, x_drop=0.5, s_drop=0.2, n_arm=A,
                         lam=1, lam_pc=1, tau=0.005, beta=1.0, hard=False, variational=True, device="cpu", eps=1e-8,
                         momentum=0.01, ref_prior=False, loss_mode="ZINB")
    with torch.no_grad():
        for p in m.parameters():   # a little larger than the default init, so that the ReLUs see both signs
            p.mul_(1.5)
    return m.eval()


def main():
    ref = RL.load_reference_nn_model()
    out = {"cases": np.array(sorted(CASES))}
    for ci, (name, cfg) in enumerate(sorted(CASES.items())):
        A, N, D, H, L, C, S = cfg
        g = torch.Generator().manual_seed(17 + ci)
        c = torch.softmax(3 * torch.randn(A, N, C, generator=g, dtype=torch.float64), -1)
        s = torch.randn(A, N, S, generator=g, dtype=torch.float64)
        X = ZR.counts_matrix(N, D, g)
        out[f"{name}/cfg"] = np.array(cfg, np.int64)
        out[f"{name}/c"], out[f"{name}/s"], out[f"{name}/X"] = c.numpy(), s.numpy(), X.numpy()
        for tag, dtype in (("f64", torch.float64), ("f32", torch.float32)):
            old = torch.get_default_dtype()
            torch.set_default_dtype(dtype)
            try:
                m = _model(ref, cfg, 5 + ci)
                if tag == "f64":
                    with torch.no_grad():
                        for a in range(A):
                            h = m._decode(c[a], s[a], a)
                            for lin in (m.fc11_p[a], m.fc11_r[a]):
                                k = SPREAD * 0.98 / float(lin(h).abs().max())
                                lin.weight.mul_(k)
                                lin.bias.mul_(k)
                    sd64 = {k: v.clone() for k, v in m.state_dict().items()}
                    for k, v in sd64.items():
                        out[f"{name}/sd/{k}"] = v.detach().cpu().numpy().copy()
                else:   # the same model, rounded (init draws differ between dtypes)
                    m.load_state_dict({k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd64.items()})
                Xd = X.to(dtype)
                with torch.no_grad():
                    hd = [m.decoder_zinb(c[a].to(dtype), s[a].to(dtype), a) for a in range(A)]
                    assert all(float(F.abs().max()) <= SPREAD * 1.001 for a in range(A)
                               for F in (torch.logit(hd[a][1].double()), torch.logit(hd[a][2].double())))
                    for j, key in enumerate(("rec", "p", "r")):
                        out[f"{name}/{tag}/{key}"] = np.stack([hd[a][j].numpy() for a in range(A)])
                    out[f"{name}/{tag}/loss"] = np.array([float(ref.zinb_loss(*hd[a], Xd)) for a in range(A)])
                    t = torch.zeros(A, N, D, dtype=dtype)
                    for a in range(A):
                        for i in range(N):
                            for d in range(D):
                                t[a, i, d] = ref.zinb_loss(*(h[i:i + 1, d:d + 1].clone() for h in hd[a]), Xd[i:i + 1, d:d + 1].clone())
                    out[f"{name}/{tag}/terms"] = t.numpy()
                    assert np.isfinite(t.numpy()).all()
            finally:
                torch.set_default_dtype(old)
    np.savez_compressed(os.path.join(GOLDEN, "zinb_kat.npz"), **out)
    print({k: np.asarray(v).shape for k, v in out.items() if "/sd/" not in k})
    print(os.path.getsize(os.path.join(GOLDEN, "zinb_kat.npz")), "bytes")


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Records tests/golden/augtrain_ref.npz from the live reference classes (imported at run time from --reference).

Three steps of the body of the reference's train_augmenter (mmidas/augmentation/train.py:61-116, MSE mode) as far as the
augmenter goes: per step ``netA(x, False)`` twice in training mode, ``A_loss`` reduced to the one term that has a gradient with
respect to netA, ``lambda[3] * 0.5 * mse_loss(fake_data2, real_data)``, under ``torch.optim.Adam``.  Stored: the initial
state_dict, the batches, every forward's dropout keep-mask, ``z0`` and ``eps`` (re-drawn from the same seed in the reference's
draw order: randn [B, NZ], the dropout's bernoulli [B, D], randn [B, Z]; the mask is checked against a hook on ``dp``), step
1's 29 gradients, the logged ``recon_loss`` of every step, the final state_dict.

    python tools/gen_golden_augtrain.py --reference /path/to/reference
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "augtrain_ref.npz"))
    a = ap.parse_args()
    sys.path.insert(0, a.reference)
    from mmidas.augmentation.udagan import Augmenter_smartseq

    from tests import augtrain_cases as AC
    from tests import augtrain_restatement as R
    NZ, Z, D, n_dim, B = AC.CASES[0]
    lam3, lr, steps = 0.5, 1e-3, 3
    sd0 = R.random_state_dict(NZ, Z, D, n_dim, 101)
    net = Augmenter_smartseq(NZ, Z, D, n_dim, AC.P_DROP)
    net.load_state_dict(sd0)
    net.train()
    seen = []
    net.dp.register_forward_hook(lambda m, i, o: seen.append((i[0].clone(), o.clone())))
    opt = torch.optim.Adam([{"params": net.parameters()}], lr=lr)
    out = {"dims": np.array([NZ, Z, D, n_dim, B]), "lam3": np.array(lam3), "lr": np.array(lr), "p_drop": np.array(AC.P_DROP)}
    for k, v in sd0.items():
        out["sd0/" + k] = v.numpy()
    bce = torch.nn.BCELoss()
    for t in range(steps):
        x = R.synthetic_batch(B, D, 200 + t)
        out[f"x/{t}"] = x.numpy()
        torch.manual_seed(300 + t)
        opt.zero_grad()
        _, fake1 = net(x, False)
        _, fake2 = net(x, False)
        torch.manual_seed(300 + t)
        for f in range(2):
            z0 = torch.randn(B, NZ)
            mask = torch.empty(B, D).bernoulli_(1 - AC.P_DROP)
            eps = torch.randn(B, Z)
            xin, xout = seen[2 * t + f]
            assert torch.equal(xout, xin * mask / (1 - AC.P_DROP)), "the re-drawn mask is not the dropout's"
            out[f"mask/{t}/{f}"] = mask.to(torch.uint8).numpy()
            out[f"z0/{t}/{f}"] = z0.numpy()
            out[f"eps/{t}/{f}"] = eps.numpy()
        real_bin = (x > 1e-4).float()          # train.py:40-41 (the module's eps = 1e-4)
        fake_bin = (fake2 > 1e-3).float().detach()
        mse = torch.nn.functional.mse_loss(fake2, x)
        out[f"recon_loss/{t}"] = np.array(float((mse + bce(fake_bin, real_bin)) / 2))
        (lam3 * 0.5 * mse).backward()
        if t == 0:
            for k, p in net.named_parameters():
                out["grad0/" + k] = p.grad.numpy().copy()
        opt.step()
    for k, v in net.state_dict().items():
        out["sd1/" + k] = v.numpy()
    np.savez_compressed(a.out, **out)
    print(a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()

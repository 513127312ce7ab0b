"""TEST INFRASTRUCTURE ONLY -- CPU restatement of the pruning phase (mmidas/cpl_mixvae.py:996-1444), written from its
description: the positions the five pruning masks cover, one masked train step in torch's ``weight_orig * mask`` semantics
on top of ``oracle/restatement.py`` (which is imported, not changed), and the assessment / decision in numpy.

* positions     :1124-1128  fcc.weight[k, :], fcc.bias[k], fc_mu.weight[:, L + k], fc_sigma.weight[:, L + k], fc6.weight[:, k]
* masked step   :1153-1161 (``prune.custom_from_mask``: forward on ``weight_orig * mask``, so the gradient of ``weight_orig``
                is the effective weight's times the mask), :1220 (``forward(mask=kept)``), Adam as the trajectory tests
* assessment    :1056-1107  per pair a confusion matrix of labels, column j divided by max(row sum j, column sum j) (0 where
                that is 0), its diagonal; the mean over pairs
* decision      :1108-1132  prune the kept category of smallest agreement while that is <= min_con and pr < max_prun_it
"""
import numpy as np
import torch

from oracle import restatement as R

PRUNED_TENSORS = ("fcc.weight", "fcc.bias", "fc_mu.weight", "fc_sigma.weight", "fc6.weight")


# --------------------------------------------------------------------------- positions
def keep_masks(h: R.Hyper, pruned, dtype=torch.float64):
    """{state_dict key: 0/1 tensor of the parameter's shape} for the five pruned tensors of every arm."""
    L, C, S = h.lowD_dim, h.n_categories, h.state_dim
    pruned = [int(k) for k in pruned]
    out = {}
    for a in range(h.n_arm):
        w = torch.ones(C, L, dtype=dtype); w[pruned, :] = 0
        b = torch.ones(C, dtype=dtype); b[pruned] = 0
        mu = torch.ones(S, L + C, dtype=dtype); mu[:, [L + k for k in pruned]] = 0
        f6 = torch.ones(L, C + S, dtype=dtype); f6[:, pruned] = 0
        out[f"fcc.{a}.weight"], out[f"fcc.{a}.bias"] = w, b
        out[f"fc_mu.{a}.weight"], out[f"fc_sigma.{a}.weight"], out[f"fc6.{a}.weight"] = mu, mu.clone(), f6
    return out


def pruned_flat_positions(per_arm, offset, A, L, C, S, pruned):
    """Sorted flat indices (int64) of the pruned positions in a buffer of the parameter layout: ``per_arm`` floats per arm,
    ``offset[t]`` of tensor t within an arm (mmvae_param_layout; 10 fcc.w[C,L], 11 fcc.b, 12 fc_mu.w[S,L+C],
    13 fc_sigma.w[S,L+C], 16 fc6.w[L,C+S], row-major)."""
    pos = []
    for a in range(A):
        base = a * int(per_arm)
        for k in pruned:
            k = int(k)
            pos += [base + int(offset[10]) + k * L + i for i in range(L)]
            pos.append(base + int(offset[11]) + k)
            pos += [base + int(offset[12]) + s * (L + C) + L + k for s in range(S)]
            pos += [base + int(offset[13]) + s * (L + C) + L + k for s in range(S)]
            pos += [base + int(offset[16]) + r * (C + S) + k for r in range(L)]
    pos = np.array(sorted(pos), dtype=np.int64)
    assert len(np.unique(pos)) == len(pos)
    return pos


# --------------------------------------------------------------------------- masked step
def effective(sd, keep):
    return {k: (v * keep[k].to(v.dtype) if k in keep else v) for k, v in sd.items()}


def masked_grads(sd, x, h: R.Hyper, noise, kept, keep):
    """forward(mask=kept) + loss on the effective parameters ``p * keep`` and the gradients of ``p`` (the effective weight's
    times ``keep``).  ``sd`` is left unchanged; returns (out, loss tuple, grads, the state dict with updated running stats)."""
    eff = effective({k: v.clone() for k, v in sd.items()}, keep)
    out, lt, gs = R.grads_autograd(eff, [x] * h.n_arm, h, noise, mask=[int(k) for k in kept])
    gs = {k: (g * keep[k].to(g.dtype) if k in keep else g) for k, g in gs.items()}
    return out, lt, gs, eff


def masked_adam_steps(sd, batches, h: R.Hyper, noises, kept, lr=1e-3):
    """k masked train steps with the Adam of the trajectory tests (R.adam_step) on ``weight_orig``; returns the per-step
    (loss tuple, grads) and the final EFFECTIVE state dict.  ``sd`` is not modified."""
    pruned = sorted(set(range(h.n_categories)) - {int(k) for k in kept})
    keep = keep_masks(h, pruned, dtype=next(iter(sd.values())).dtype)
    sd = {k: v.clone() for k, v in sd.items()}
    keys = R.param_keys(h)
    m = {k: torch.zeros_like(sd[k]) for k in keys}
    v = {k: torch.zeros_like(sd[k]) for k in keys}
    hist = []
    for t, (x, nz) in enumerate(zip(batches, noises), start=1):
        _, lt, gs, eff = masked_grads(sd, x, h, nz, kept, keep)
        for k in sd:
            if k not in keys:
                sd[k] = eff[k]                                   # running statistics
        for k in keys:
            sd[k], m[k], v[k] = R.adam_step(sd[k], gs[k], m[k], v[k], t, lr)
        hist.append((lt, gs))
    return hist, effective(sd, keep)


# --------------------------------------------------------------------------- assessment and decision
def start(bias):
    bias = np.asarray(bias)
    return np.where(bias != 0.0)[0], np.where(bias == 0.0)[0]


def agreement(labels, C):
    """labels: int [A, N].  float64 [C]: mean over arm pairs (a < b) of the diagonal of the normalised confusion matrix."""
    labels = np.asarray(labels).astype(np.int64)
    diags = []
    for a in range(labels.shape[0]):
        for b in range(a + 1, labels.shape[0]):
            cm = np.zeros((C, C))
            for i, j in zip(labels[a], labels[b]):
                cm[i, j] += 1
            num = np.array([max(cm[k, :].sum(), cm[:, k].sum()) for k in range(C)])
            cm = np.divide(cm, num, out=np.zeros_like(cm), where=num != 0)
            diags.append(np.diag(cm))
    return np.mean(diags, axis=0)


def decision(c_agreement, kept, min_con, pr, max_prun_it):
    """The category to prune, or None.  (A single remaining category is never pruned: the masked forward needs one.)"""
    kept = np.asarray(kept)
    if len(kept) <= 1:
        return None
    a = np.asarray(c_agreement)[kept]
    if np.min(a) <= min_con and pr < max_prun_it:
        return int(kept[np.argmin(a)])
    return None

"""The training objective under the ZINB likelihood and its gradients, restated in torch on the CPU (include/mmvae.h:
mmvae_zinb_train_step).  Built on ``oracle.restatement`` (the step's forward, the KL, entropy and coupling
terms, Adam) and ``tests/zinb_restatement.py`` (the term whose mean is zinb_loss); nothing under ``oracle/`` is changed.

The objective is the reference's ``loss()`` with the branch it left as ``assert False`` (mmidas/nn_model.py:547-549) taken
literally:

    total = max(A - 1, 1) sum_a (zinb_loss(x_rec_a, x_p_a, x_r_a, x_a) + beta KL_a) + loss_joint

``oracle.restatement.forward(..., keep=True)`` saves a differentiable ``d10`` per arm; the two gates ``sigmoid(fc11_p(d10))``,
``sigmoid(fc11_r(d10))`` are formed on it here, ``x_rec`` is the forward's own ``relu(fc11(d10))`` (so a ``relu_override`` of
site ``x_rec`` holds for it).  In float64 this is the truth the device is measured against, in float32 the reference whose
error sets the device's budget."""
import os
import sys

import torch
import torch.nn.functional as F

from oracle import restatement as R

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import zinb_restatement as ZR  # noqa: E402

EPS = ZR.EPS
HEAD_LAYERS = ("fc11_p", "fc11_r")
TERMS = ("zinb", "kl", "ent", "dist")


def init_heads(h: R.Hyper, seed: int, dtype=torch.float32):
    """``fc11_p`` / ``fc11_r`` of every arm at ``nn.Linear``'s default initialisation: {"fc11_p.<a>.weight": [D, H], ...}."""
    torch.manual_seed(seed)
    sd = {}
    for name in HEAD_LAYERS:
        for a in range(h.n_arm):
            lin = torch.nn.Linear(h.fc_dim, h.input_dim)
            sd[f"{name}.{a}.weight"] = lin.weight.detach().to(dtype).clone()
            sd[f"{name}.{a}.bias"] = lin.bias.detach().to(dtype).clone()
    return sd


def head_keys(h: R.Hyper):
    return [f"{name}.{a}.{kind}" for name in HEAD_LAYERS for a in range(h.n_arm) for kind in ("weight", "bias")]


def param_keys(h: R.Hyper):
    """The 28 tensors per arm in ``model.parameters()`` order, then the p and r heads."""
    return R.param_keys(h) + head_keys(h)


def zinb_losses(sd, out, saved, xs, h: R.Hyper, zeps=EPS):
    """[zinb_loss of arm a]: the mean over the B D elements of the term under the three heads on the forward's d10."""
    res = []
    for a in range(h.n_arm):
        d10 = saved[a]["d10"]
        x_p = torch.sigmoid(F.linear(d10, sd[f"fc11_p.{a}.weight"], sd[f"fc11_p.{a}.bias"]))
        x_r = torch.sigmoid(F.linear(d10, sd[f"fc11_r.{a}.weight"], sd[f"fc11_r.{a}.bias"]))
        res.append(ZR.terms(out[0][a], x_p, x_r, xs[a], zeps).mean())
    return res


def objective_terms(sd, xs, h: R.Hyper, noise, zeps=EPS, **fw):
    """One forward -> (out, saved, {"zinb": (A-1)' sum_a zinb_loss_a, "kl", "ent", "dist" as ``loss_terms`` carries them,
    "const"}, [zinb_loss_a]); the total is the sum of the five."""
    out, saved = R.forward(sd, xs, h, noise, keep=True, **fw)
    lt = R.loss_terms(out, xs, h)
    zl = zinb_losses(sd, out, saved, xs, h, zeps)
    terms = {"zinb": max(h.n_arm - 1, 1) * sum(zl), "kl": lt["kl"], "ent": lt["ent"], "dist": lt["dist"], "const": lt["const"]}
    return out, saved, terms, zl


def loss_tuple(out, xs, h: R.Hyper, terms, zl):
    """The reference's 9-tuple with the ZINB reconstruction: (total, [zinb_loss_a], loss_joint, c_entropy, c_distance, c_l2,
    [KL_a], [], [ll_a]); the joint, the means and ll (MSE-based, :542) are ``oracle.restatement.loss``'s."""
    mse = R.loss(out, xs, h)
    total = terms["zinb"] + terms["kl"] + terms["ent"] + terms["dist"] + terms["const"]
    return (total, torch.stack([z.detach() for z in zl]), mse[2], mse[3], mse[4], mse[5], mse[6], [], mse[8])


def _leaves(sd, h):
    keys = param_keys(h)
    leaves = {k: sd[k].detach().clone().requires_grad_(True) for k in keys}
    work = dict(sd)
    work.update(leaves)
    return keys, leaves, work


def grads_autograd(sd, xs, h: R.Hyper, noise, zeps=EPS, **fw):
    """forward + objective + ``autograd.grad``: (out, saved, loss tuple, {key: gradient}) for the 28 tensors per arm and the p
    and r heads; the running statistics of ``sd`` are updated as the forward updates them."""
    keys, leaves, work = _leaves(sd, h)
    out, saved, terms, zl = objective_terms(work, xs, h, noise, zeps, **fw)
    lt = loss_tuple(out, xs, h, terms, zl)
    gs = torch.autograd.grad(lt[0], [leaves[k] for k in keys])
    for k in sd:
        if k not in leaves:
            sd[k] = work[k]
    return out, saved, lt, dict(zip(keys, gs))


def term_grads(sd, xs, h: R.Hyper, noise, zeps=EPS, **fw):
    """{term: {key: gradient}} for TERMS (a tensor a term does not reach gets zeros); ``sd`` is left unchanged."""
    keys, leaves, work = _leaves(sd, h)
    _, _, terms, _ = objective_terms(work, xs, h, noise, zeps, update_running=False, **fw)
    res = {}
    for t in TERMS:
        gs = torch.autograd.grad(terms[t], [leaves[k] for k in keys], retain_graph=True, allow_unused=True)
        res[t] = {k: (torch.zeros_like(leaves[k]) if g is None else g) for k, g in zip(keys, gs)}
    return res


def objective_value(sd, xs, h: R.Hyper, noise, zeps=EPS, **fw):
    """The total alone, no gradient, ``sd`` unchanged: what the finite differences of the self-check evaluate."""
    with torch.no_grad():
        _, _, terms, _ = objective_terms(dict(sd), xs, h, noise, zeps, update_running=False, **fw)
    return float(sum(terms[t] for t in TERMS) + terms["const"])


def adam_losses(sd, x, h: R.Hyper, noises, lr=1e-3, zeps=EPS):
    """The float64 restatement of ``len(noises)`` training steps on one batch: every step a forward in training mode on its
    noise, the gradients by autograd, ``oracle.restatement.adam_step`` on every tensor; returns the total before each step."""
    sd = {k: (v.double().clone() if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    keys = param_keys(h)
    m = {k: torch.zeros_like(sd[k]) for k in keys}
    v = {k: torch.zeros_like(sd[k]) for k in keys}
    xs = [x.double()] * h.n_arm
    losses = []
    for t, nz in enumerate(noises, start=1):
        n64 = {k: [u.double() if u.is_floating_point() else u for u in vals] for k, vals in nz.items()}
        _, _, lt, gs = grads_autograd(sd, xs, h, n64, zeps)
        for k in keys:
            sd[k], m[k], v[k] = R.adam_step(sd[k], gs[k], m[k], v[k], t, lr)
            sd[k] = sd[k].detach()
        losses.append(float(lt[0].detach()))
    return losses


"""The gradient of the ZINB term with respect to the three heads, restated in torch on the CPU (DESIGN.md section 9m;
include/mmvae.h).  Two routes to the same numbers:

* ``analytic``: the table of the header, written out in the dtype of its inputs (float64: the truth's cross-check);
* ``autograd_*``: torch's autograd of ``tests/zinb_restatement.terms`` -- in float64 the truth the device is measured
  against, in float32 the reference's own arithmetic whose error sets the device's budget.

``magnitudes`` is the scale M the errors are measured on: per element of g the sum of the magnitudes of the selected
branch's addends times the chain factor; for dW and db the sum of those over the cells (times |d10| for dW)."""
import numpy as np
import torch
import torch.nn.functional as F

import zinb_restatement as ZR

EPS = ZR.EPS
HEADS = ("rec", "p", "r")


SHAPES = [(1, 1, 1), (63, 31, 7), (65, 33, 100), (257, 130, 128), (257, 31, 100), (1, 130, 7), (63, 1, 128), (65, 130, 1)]


def inputs(n, D, H):
    """(d10 [n, H], the six layer tensors, X [n, D]) float32: the inputs of DESIGN.md section 9k's table at one shape."""
    g = torch.Generator().manual_seed(1000 * n + 10 * D + H)
    d10 = torch.relu(torch.randn(n, H, generator=g))
    if not bool((d10 > 0).any()):
        d10[0, 0] = 0.75
    L = ZR.spread_layers(d10, D, g)
    X = ZR.counts_matrix(n, D, g)
    return d10, L, X


def pre_activations(d10, W, b, Wp, bp, Wr, br):
    return F.linear(d10, W, b), F.linear(d10, Wp, bp), F.linear(d10, Wr, br)


def _parts(a_rec, a_p, a_r, X, eps, subtract=False):
    k = X.exp() - 1.0
    r = torch.relu(a_rec) + eps
    sp, sr = torch.sigmoid(a_p), torch.sigmoid(a_r)
    # 1 - s without the cancelling subtraction
    cp, cr = torch.sigmoid(-a_p), torch.sigmoid(-a_r)
    p, q = (1 - eps) * (sp + eps), (1 - eps) * cp + eps * eps
    z, y = (1 - eps) * (sr + eps), (1 - eps) * cr + eps * eps
    if subtract:            # q and y as zinb_restatement.terms, and so its autograd, form them
        q, y, cp, cr = 1 - p, 1 - z, 1 - sp, 1 - sr
    return k, r, p, q, z, y, (a_rec > 0).to(X.dtype), (1 - eps) * sp * cp, (1 - eps) * sr * cr


def analytic(a_rec, a_p, a_r, X, eps=EPS, subtract=False):
    """(g_rec, g_p, g_r) = d term / d (a_rec, a_p, a_r): the header's table times the chain factors.  ``subtract``: with
    1 - p and 1 - z formed by subtraction, as ``zinb_restatement.terms`` forms them, in place of the kernels' way."""
    k, r, p, q, z, y, c_rec, c_p, c_r = _parts(a_rec, a_p, a_r, X, eps, subtract)
    lq = q.log()
    w = (r * lq).exp()
    u = z + y * w
    pos = X > 0
    gr = torch.where(pos, -torch.special.digamma(k + r) + torch.special.digamma(r) - lq, -(y * w * lq) / u)
    gp = torch.where(pos, -k / p + r / q, (y * r * w) / (q * u))
    gz = torch.where(pos, 1 / y, torch.expm1(r * lq) / u)
    return gr * c_rec, gp * c_p, gz * c_r


def magnitudes(a_rec, a_p, a_r, X, eps=EPS):
    """M of (g_rec, g_p, g_r) in float64."""
    a_rec, a_p, a_r, X = (t.double() for t in (a_rec, a_p, a_r, X))
    k, r, p, q, z, y, c_rec, c_p, c_r = _parts(a_rec, a_p, a_r, X, eps)
    lq = q.log()
    w = (r * lq).exp()
    u = z + y * w
    pos = X > 0
    Mr = torch.where(pos, torch.special.digamma(k + r).abs() + torch.special.digamma(r).abs() + lq.abs(), (y * w * lq / u).abs())
    Mp = torch.where(pos, k / p + r / q, (y * r * w / (q * u)).abs())
    Mz = torch.where(pos, (1 / y).abs(), (1 + w) / u)
    return Mr * c_rec, Mp * c_p, Mz * c_r


def autograd_pre(a_rec, a_p, a_r, X, eps=EPS):
    """d sum(terms) / d (a_rec, a_p, a_r) by autograd, in the dtype of the inputs."""
    a = [t.detach().clone().requires_grad_() for t in (a_rec, a_p, a_r)]
    ZR.terms(torch.relu(a[0]), torch.sigmoid(a[1]), torch.sigmoid(a[2]), X, eps).sum().backward()
    return tuple(t.grad for t in a)


def autograd_given(x_rec, x_p, x_r, X, eps=EPS):
    """d sum(terms) / d (x_rec, x_p, x_r), the heads given (no relu, no sigmoid)."""
    h = [t.detach().clone().requires_grad_() for t in (x_rec, x_p, x_r)]
    ZR.terms(h[0], h[1], h[2], X, eps).sum().backward()
    return tuple(t.grad for t in h)


def magnitudes_given(x_rec, x_p, x_r, X, eps=EPS):
    """M of the gradient with respect to given heads: chain factors 1, 1 - eps, 1 - eps."""
    x_rec, x_p, x_r, X = (t.double() for t in (x_rec, x_p, x_r, X))
    k = X.exp() - 1.0
    r = x_rec + eps
    p = (1 - eps) * (x_p + eps)
    z = (1 - eps) * (x_r + eps)
    q, y = 1 - p, 1 - z
    lq = q.log()
    w = (r * lq).exp()
    u = z + y * w
    pos = X > 0
    Mr = torch.where(pos, torch.special.digamma(k + r).abs() + torch.special.digamma(r).abs() + lq.abs(), (y * w * lq / u).abs())
    Mp = torch.where(pos, k / p + r / q, (y * r * w / (q * u)).abs())
    Mz = torch.where(pos, (1 / y).abs(), (1 + w) / u)
    return Mr, (1 - eps) * Mp, (1 - eps) * Mz


def autograd_heads(d10, L, X, eps=EPS, scale=1.0):
    """{"rec": (dW, db), "p": ..., "r": ...}: the gradient of scale * sum(terms) with respect to the three layers, by
    autograd of the restatement in the dtype of the inputs."""
    P = [t.detach().clone().requires_grad_() for t in L]
    (scale * ZR.terms(*ZR.heads(d10, *P), X, eps).sum()).backward()
    return {h: (P[2 * j].grad, P[2 * j + 1].grad) for j, h in enumerate(HEADS)}


def head_magnitudes(d10, L, X, eps=EPS, scale=1.0):
    """M of dW_j [D, H] and db_j [D] in float64."""
    d64, L64 = d10.double(), [t.double() for t in L]
    Mg = magnitudes(*pre_activations(d64, *L64), X.double(), eps)
    return {h: (scale * (Mg[j].T @ d64.abs()), scale * Mg[j].sum(0)) for j, h in enumerate(HEADS)}


# ---- the descent experiment -------------------------------------------------------------------------------------------------
def default_heads(D, H, seed):
    """Three ``nn.Linear(H, D)`` at their default initialisation -> [W, b, Wp, bp, Wr, br] float32."""
    torch.manual_seed(seed)
    out = []
    for _ in range(3):
        lin = torch.nn.Linear(H, D)
        out += [lin.weight.detach().clone(), lin.bias.detach().clone()]
    return out


def draw_counts(d10, rng, D):
    """X = log1p(counts) float32 [n, D]: counts drawn with numpy from known heads on ``d10`` [n, H] -- a Gamma-Poisson with
    shape r and odds p / (1 - p), zeroed with probability z."""
    n, H = d10.shape
    h = np.asarray(d10, dtype=np.float64)
    W = rng.normal(size=(3, D, H)) / np.sqrt(H)
    b = rng.normal(size=(3, D)) * 0.5
    r = np.maximum(h @ W[0].T + b[0] + 1.0, 0.0) + 0.05
    p = 1.0 / (1.0 + np.exp(-(h @ W[1].T + b[1] + 1.0)))
    z = 1.0 / (1.0 + np.exp(-(h @ W[2].T + b[2])))
    lam = rng.gamma(shape=r, scale=p / (1.0 - p))
    c = rng.poisson(np.minimum(lam, 1e4)) * (rng.random((n, D)) >= z)
    return torch.from_numpy(np.log1p(c.astype(np.float64))).float()


def descent_case(n=257, D=33, H=7, seed=11):
    """The inputs of the descent experiment: d10, the heads at ``nn.Linear``'s default initialisation, X."""
    g = torch.Generator().manual_seed(seed)
    d10 = torch.relu(torch.randn(n, H, generator=g))
    X = draw_counts(d10, np.random.default_rng(seed), D)
    return d10, default_heads(D, H, seed), X


def adam_losses(d10, L, X, steps=20, lr=1e-2, eps=EPS):
    """The float64 restatement of the fit: ``steps`` Adam steps on the mean term; the loss before each step."""
    P = [t.double().clone().requires_grad_() for t in L]
    opt = torch.optim.Adam(P, lr=lr)
    d64, X64 = d10.double(), X.double()
    losses = []
    for _ in range(steps):
        opt.zero_grad()
        loss = ZR.terms(*ZR.heads(d64, *P), X64, eps).mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return losses

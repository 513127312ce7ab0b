"""The gradient of the ZINB term with respect to the decoder below its heads, restated in torch on the CPU (DESIGN.md section
9n; include/mmvae.h: mmvae_zinb_d10_grad, mmvae_decoder_trunk_grads).  Built on tests/zinb_grad_restatement.py.

* ``gd10_analytic`` / ``trunk_backward``: the formulas of the header written out in the dtype of their inputs;
* ``gd10_autograd`` / ``decoder_autograd``: torch's autograd of the decoder ``relu(F.linear)`` x 5, the three heads and the
  term of ``zinb_restatement`` -- in float64 the truth, in float32 the reference whose error sets the device's budget;
* ``gd10_magnitudes`` / ``trunk_magnitudes``: the scale M the errors are measured on.  For gd10[i, h] the sum over the
  selected heads and the genes of M_g[i, d, j] |W_j[d, h]|; for the trunk the sum of the addends' magnitudes carried along
  the chain: M(dZ10) = |gd10| [d10 > 0], M(G_l-1) = M(dZ_l) |W_l|, M(dZ_l-1) = M(G_l-1) [d_l-1 > 0],
  M(dW_l) = M(dZ_l)^T |in_l|, M(db_l) = sum_i M(dZ_l)[i];
* ``gd10_emulated`` / ``trunk_emulated``: the kernels' own summation order in numpy.

A head that is not selected still shapes the likelihood (g of a selected head depends on all three pre-activations in the
zero branch); what the selection removes is that head's own path from the term to d10."""
import numpy as np
import torch
import torch.nn.functional as F

import zinb_grad_restatement as RG
import zinb_restatement as ZR

EPS = ZR.EPS
HEADS = RG.HEADS
TRUNK = ("fc6", "fc7", "fc8", "fc9", "fc10")
MASKS = [tuple(h for j, h in enumerate(HEADS) if m >> j & 1) for m in range(1, 8)]

# (N, C + S, L, H) of the trunk's error gate
TRUNK_SHAPES = [(1, 3, 2, 1), (63, 9, 5, 7), (65, 94, 10, 100), (257, 13, 10, 128)]


# ---- gd10 -------------------------------------------------------------------------------------------------------------------
def gd10_analytic(d10, L, X, heads=HEADS, scale=1.0, eps=EPS):
    """scale sum_{j in heads} g_j W_j in the dtype of the inputs."""
    g = RG.analytic(*RG.pre_activations(d10, *L), X, eps)
    return scale * sum(g[j] @ L[2 * j] for j, h in enumerate(HEADS) if h in heads)


def gd10_autograd(d10, L, X, heads=HEADS, scale=1.0, eps=EPS):
    """The same by autograd: an unselected head sees d10 detached."""
    x = d10.detach().clone().requires_grad_()
    a = [F.linear(x if h in heads else x.detach(), L[2 * j], L[2 * j + 1]) for j, h in enumerate(HEADS)]
    (scale * ZR.terms(torch.relu(a[0]), torch.sigmoid(a[1]), torch.sigmoid(a[2]), X, eps).sum()).backward()
    return x.grad


def gd10_magnitudes(d10, L, X, heads=HEADS, scale=1.0, eps=EPS):
    d64, L64 = d10.double(), [t.double() for t in L]
    Mg = RG.magnitudes(*RG.pre_activations(d64, *L64), X.double(), eps)
    return scale * sum(Mg[j] @ L64[2 * j].abs() for j, h in enumerate(HEADS) if h in heads)


def d10_segments(D, asked, n):
    """(segments used, gene tiles of one): mmvae_zinb_d10_grad's rule."""
    n_ct, n_gt = -(-n // 64), -(-D // 64)
    s = min(asked if asked > 0 else max(512 // n_ct, 1), n_gt)
    tps = -(-n_gt // s)
    return -(-n_gt // tps), tps


def gd10_emulated(d10, L, X, heads=HEADS, scale=1.0, segments=0, eps=EPS):
    """k_zg_d10's order in numpy: float32 pre-activations, g in float64 rounded once, then per segment one float32 chain over
    the genes in rising order, within a pair of genes the selected heads in the order rec, p, r (an instruction's two genes
    one after the other, each product added with one rounding); the segments added in float64, scaled, rounded once."""
    n, D = X.shape
    a = RG.pre_activations(d10, *L)
    g = [t.float().numpy() for t in RG.analytic(*(t.double() for t in a), X.double(), eps)]
    W = [L[2 * j].numpy() for j in range(3)]
    S, tps = d10_segments(D, segments, n)
    total = np.zeros((n, d10.shape[1]), dtype=np.float64)
    for s in range(S):
        acc = np.zeros((n, d10.shape[1]), dtype=np.float32)
        for k in range(s * tps * 64, min((s + 1) * tps * 64, D), 2):
            for j, h in enumerate(HEADS):
                if h in heads:
                    for d in (k, k + 1):
                        if d < D:
                            acc = (acc.astype(np.float64) + g[j][:, d, None].astype(np.float64) * W[j][None, d, :].astype(np.float64)
                                   ).astype(np.float32)
        total += acc.astype(np.float64)
    return torch.from_numpy((scale * total).astype(np.float32))


# ---- the trunk --------------------------------------------------------------------------------------------------------------
def default_trunk(Z, Lw, H, seed):
    """fc6 .. fc10 at ``nn.Linear``'s default initialisation -> [W6, b6, .. W10, b10] float32."""
    torch.manual_seed(seed)
    out = []
    for i, o in ((Z, Lw), (Lw, H), (H, H), (H, H), (H, H)):
        lin = torch.nn.Linear(i, o)
        out += [lin.weight.detach().clone(), lin.bias.detach().clone()]
    return out


def forward(zin, params):
    """[zin, d6, .. d10]: d_l = relu(fc_l(d_l-1)), in the dtype of the inputs."""
    acts = [zin]
    for l in range(5):
        acts.append(F.relu(F.linear(acts[-1], params[2 * l], params[2 * l + 1])))
    return acts


def trunk_inputs(n, Z, Lw, H):
    """(acts float32 as a float32 forward leaves them, params, gd10) at one shape of the gate.  The biases are shifted up so
    that about two thirds of every layer's units are alive; gd10 has both signs and a spread of magnitudes."""
    g = torch.Generator().manual_seed(7000 * n + 70 * Z + 7 * Lw + H)
    params = default_trunk(Z, Lw, H, 31 * n + H)
    for l in range(5):
        params[2 * l + 1] = params[2 * l + 1] + 0.1
    zin = torch.cat([torch.softmax(2 * torch.randn(n, max(Z - 2, 1), generator=g), 1), torch.randn(n, Z - max(Z - 2, 1), generator=g)], 1)
    acts = forward(zin, params)
    gd10 = torch.randn(n, H, generator=g) * torch.exp(2 * torch.randn(n, H, generator=g)) / n
    return acts, params, gd10


def trunk_backward(acts, params, gd10, rounded=False):
    """(the ten gradients dW6, db6 .. dW10, db10, gzin) from the given activations, in the dtype of the inputs.
    ``rounded``: every dZ_l rounded to float32 where the kernel stores it (for float64 inputs: the kernel's arithmetic)."""
    grads = [None] * 10
    dz = gd10 * (acts[5] > 0)
    for l in range(4, -1, -1):
        if rounded:
            dz = dz.float().to(gd10.dtype)
        grads[2 * l], grads[2 * l + 1] = dz.T @ acts[l], dz.sum(0)
        G = dz @ params[2 * l]
        dz = G * (acts[l] > 0) if l else G
    return grads, dz


def trunk_magnitudes(acts, params, gd10):
    acts, params = [t.double() for t in acts], [t.double().abs() for t in params]
    M = [None] * 10
    m = gd10.double().abs() * (acts[5] > 0)
    for l in range(4, -1, -1):
        M[2 * l], M[2 * l + 1] = m.T @ acts[l].abs(), m.sum(0)
        G = m @ params[2 * l]
        m = G * (acts[l] > 0) if l else G
    return M, m


def trunk_autograd(zin, params, gd10):
    """The same through autograd of the forward, in the dtype of the inputs: (ten gradients, gzin, acts)."""
    z = zin.detach().clone().requires_grad_()
    P = [t.detach().clone().requires_grad_() for t in params]
    acts = forward(z, P)
    acts[5].backward(gd10)
    return [p.grad for p in P], z.grad, [t.detach() for t in acts]


# ---- the whole decoder ------------------------------------------------------------------------------------------------------
def decoder_autograd(zin, params, L, X, scale=1.0, eps=EPS):
    """Autograd of scale x the sum of the terms through relu(F.linear) x 5 and the three heads, in the dtype of the inputs:
    {"trunk": ten gradients, "heads": six, "zin": gzin, "d10": gd10, "acts": the forward's activations}."""
    z = zin.detach().clone().requires_grad_()
    P = [t.detach().clone().requires_grad_() for t in params]
    Q = [t.detach().clone().requires_grad_() for t in L]
    acts = forward(z, P)
    acts[5].retain_grad()
    (scale * ZR.terms(*ZR.heads(acts[5], *Q), X, eps).sum()).backward()
    return {"trunk": [p.grad for p in P], "heads": [q.grad for q in Q], "zin": z.grad, "d10": acts[5].grad,
            "acts": [t.detach() for t in acts]}


# ---- the descent experiment -------------------------------------------------------------------------------------------------
def descent_case(n=60, Z=7, Lw=6, H=20, D=70, seed=13):
    """(zin, trunk params, heads, X): a decoder at ``nn.Linear``'s default initialisation and counts drawn from known heads on
    its own d10."""
    g = torch.Generator().manual_seed(seed)
    zin = torch.cat([F.one_hot(torch.randint(0, Z - 2, (n,), generator=g), Z - 2).float(), torch.randn(n, 2, generator=g)], 1)
    params = default_trunk(Z, Lw, H, seed)
    d10 = forward(zin, params)[5]
    X = RG.draw_counts(d10, np.random.default_rng(seed), D)
    return zin, params, RG.default_heads(D, H, seed + 1), X


def adam_losses(zin, params, L, X, steps=20, lr=1e-3, eps=EPS):
    """The float64 restatement of the whole-decoder fit: ``steps`` Adam steps on the mean term; the loss before each step."""
    P = [t.double().clone().requires_grad_() for t in list(params) + list(L)]
    opt = torch.optim.Adam(P, lr=lr)
    z64, X64 = zin.double(), X.double()
    losses = []
    for _ in range(steps):
        opt.zero_grad()
        loss = ZR.terms(*ZR.heads(forward(z64, P[:10])[5], *P[10:]), X64, eps).mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return losses

"""The augmenter's training step restated in torch (own code; float64 or float32, on any device).

One step of the reference's ``train_augmenter`` body in MSE mode as far as the augmenter is concerned
(mmidas/augmentation/train.py:61-116): optionally a statistics pass (a training-mode forward that only moves the BatchNorm
running statistics), the training-mode forward of ``Augmenter_smartseq`` (udagan.py:311-329) on a given dropout keep-mask,
``z0`` and ``eps``, and the gradient of ``weight * mean((x_aug - x)**2)`` by autograd.  ``relu_override`` (eleven boolean
tensors: the ReLU decisions of h1..h10 and of x_aug) replaces ``relu(y)`` by ``y * decision``, which is how a float64 truth is
evaluated on the device's own decisions.
"""
from __future__ import annotations

import torch

LINEARS = [f"fc{i}" for i in range(1, 12)] + ["fc_mu", "fc_sigma", "noise"]
BNS = [f"batch_fc{i}" for i in range(1, 11)] + ["batch_fc_mu", "bnz"]
PARAM_ORDER = (["noise.weight", "bnz.weight", "bnz.bias"] + [f"fc{i}.{t}" for i in range(1, 6) for t in ("weight", "bias")]
               + [f"{n}.{t}" for n in ("fc_mu", "fc_sigma") for t in ("weight", "bias")]
               + [f"fc{i}.{t}" for i in range(6, 12) for t in ("weight", "bias")])
ZERO_GRAD_BIASES = [f"fc{i}.bias" for i in range(1, 11)] + ["fc_mu.bias"]      # in front of a non-affine BatchNorm
BN_EPS, BN_MOM, BNZ_EPS, BNZ_MOM = 1e-10, 0.01, 1e-5, 0.1


def random_state_dict(NZ, Z, D, n_dim, seed):
    """nn.Linear-like uniform weights, non-trivial running statistics, bnz affine off its defaults."""
    g = torch.Generator().manual_seed(seed)
    n1, n5 = D // 5, n_dim // 5
    shapes = {"fc1": (n1, D), "fc2": (n1, n1), "fc3": (n_dim, n1), "fc4": (n_dim, n_dim), "fc5": (n5, n_dim + NZ),
              "fc_mu": (Z, n5), "fc_sigma": (Z, n5), "fc6": (n5, Z), "fc7": (n_dim, n5), "fc8": (n_dim, n_dim),
              "fc9": (n1, n_dim), "fc10": (n1, n1), "fc11": (D, n1), "noise": (NZ, NZ)}
    sd = {}
    for name, (o, i) in shapes.items():
        k = 1.0 / i ** 0.5
        sd[name + ".weight"] = (torch.rand(o, i, generator=g) * 2 - 1) * k
        if name != "noise":
            sd[name + ".bias"] = (torch.rand(o, generator=g) * 2 - 1) * k
    sd["bnz.weight"] = 0.5 + torch.rand(NZ, generator=g)
    sd["bnz.bias"] = 0.2 * torch.randn(NZ, generator=g)
    widths = [n1, n1, n_dim, n_dim, n5, n5, n_dim, n_dim, n1, n1, Z, NZ]
    for name, n in zip(BNS, widths):
        sd[name + ".running_mean"] = 0.1 * torch.randn(n, generator=g)
        sd[name + ".running_var"] = 0.5 + torch.rand(n, generator=g)
        sd[name + ".num_batches_tracked"] = torch.tensor(3)
    return sd


def synthetic_batch(B, D, seed):
    """log1p-count-like data: about half exact zeros."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, D, generator=g) * 4.0
    return x * (torch.rand(B, D, generator=g) > 0.5)


def draw_noise(B, D, NZ, Z, p_drop, seed, n_pass=1):
    g = torch.Generator().manual_seed(seed)
    mask = (torch.rand(n_pass, B, D, generator=g) >= p_drop).to(torch.uint8)
    return mask, torch.randn(n_pass, B, NZ, generator=g), torch.randn(n_pass, B, Z, generator=g)


MAG = "#M"      # run / upd also carry, under key + MAG, the sum of the magnitudes of the addends a running statistic is made of


def _bn(y, run, name, eps, mom, upd):
    B = y.shape[0]
    mean = y.mean(0)
    var = ((y - mean) ** 2).mean(0)
    if upd is not None:
        with torch.no_grad():
            km, kv = name + ".running_mean", name + ".running_var"
            upd[km] = (1 - mom) * run[km] + mom * mean
            upd[kv] = (1 - mom) * run[kv] + mom * var * B / (B - 1)
            upd[name + ".num_batches_tracked"] = run[name + ".num_batches_tracked"] + 1
            upd[km + MAG] = (1 - mom) * run.get(km + MAG, run[km].abs()) + mom * y.abs().mean(0)
            upd[kv + MAG] = (1 - mom) * run.get(kv + MAG, run[kv].abs()) + mom * ((y.abs() + mean.abs()) ** 2).mean(0) * B / (B - 1)
    return (y - mean) / torch.sqrt(var + eps)


def forward(P, run, x, mask, z0, eps, p_drop, scale=1.0, relu_override=None, upd=None, keep=None):
    """P: parameters (the step's dtype), run: running statistics.  Returns (s, x_aug); ``upd`` receives the updated running
    statistics, ``keep`` the normalised pre-activations ``pre`` (10), the post-ReLU ``h`` (10), the Linear outputs ``lin``."""
    pre, hs, lin, lin_in = [], [], {}, {}

    def L(name, v):
        lin_in[name] = v
        y = v @ P[name + ".weight"].T
        if name + ".bias" in P:
            y = y + P[name + ".bias"]
        if keep is not None and y.requires_grad:
            y.retain_grad()
        lin[name] = y
        return y

    def act(y, i):
        pre.append(y)
        h = torch.relu(y) if relu_override is None else y * relu_override[i].to(y.dtype)
        hs.append(h)
        return h

    def layer(i, v):
        return act(_bn(L(f"fc{i}", v), run, f"batch_fc{i}", BN_EPS, BN_MOM, upd), i - 1)

    zhat = _bn(L("noise", scale * z0), run, "bnz", BNZ_EPS, BNZ_MOM, upd)
    zb = zhat * P["bnz.weight"] + P["bnz.bias"]
    if keep is not None and zb.requires_grad:
        zb.retain_grad()
    z = torch.nn.functional.elu(zb)
    h = x * mask.to(x.dtype) / (1.0 - p_drop)
    for i in range(1, 5):
        h = layer(i, h)
    h = layer(5, torch.cat((h, z), dim=1))
    mu = _bn(L("fc_mu", h), run, "batch_fc_mu", BN_EPS, BN_MOM, upd)
    sigma = torch.sigmoid(L("fc_sigma", h))
    s = eps * sigma + mu
    h = s
    for i in range(6, 11):
        h = layer(i, h)
    y11 = L("fc11", h)
    x_aug = torch.relu(y11) if relu_override is None else y11 * relu_override[10].to(y11.dtype)
    if keep is not None:
        keep.update(pre=pre, h=hs, lin=lin, y11=y11, lin_in=lin_in, zhat=zhat, zb=zb, sigma=sigma)
    return s, x_aug


def step(sd, x, mask, z0, eps, p_drop, dtype=torch.float64, weight=0.25, scale=1.0, relu_override=None, stat=None, device="cpu"):
    """sd: a state_dict; mask / z0 / eps: the main forward's; stat: (mask, z0, eps) of the statistics pass or None.
    Returns a dict: s, x_aug, pre, h, grads {name: tensor}, dlin {Linear name: d loss / d its output}, running {name: new
    value} (after the statistics pass and the main forward; name + MAG: its magnitude sum), M {name: section 9m's per-element magnitude sums of "s", "x_aug" and every
    gradient, see _magnitudes}, mse, mismatch, recon_loss."""
    to = lambda t: t.detach().to(device=device, dtype=dtype)      # noqa: E731
    P = {k: to(v).requires_grad_(True) for k, v in sd.items() if k in PARAM_ORDER}
    run = {k: (v.detach().to(device) if k.endswith("num_batches_tracked") else to(v)) for k, v in sd.items() if k not in PARAM_ORDER}
    x = to(x)
    if stat is not None:
        upd = {}
        with torch.no_grad():
            forward(P, run, x, stat[0].to(device), to(stat[1]), to(stat[2]), p_drop, scale, None, upd)
        run = upd
    upd, keep = {}, {}
    s, x_aug = forward(P, run, x, mask.to(device), to(z0), to(eps), p_drop, scale, relu_override, upd, keep)
    mse = ((x_aug - x) ** 2).mean()
    (weight * mse).backward()
    mismatch = int(((x_aug > 1e-3) != (x > 1e-4)).sum())
    n = x.numel()
    mse = mse.detach()
    with torch.no_grad():
        M = _magnitudes(P, keep, to(eps), x, x_aug, 2.0 * weight / n)
    return {"s": s.detach(), "x_aug": x_aug.detach(), "pre": [t.detach() for t in keep["pre"]], "h": [t.detach() for t in keep["h"]],
            "y11": keep["y11"].detach(),
            "grads": {k: (p.grad if p.grad is not None else torch.zeros_like(p)) for k, p in P.items()},
            "dlin": {k: v.grad for k, v in keep["lin"].items() if v.grad is not None},
            "M": M, "running": upd, "mse": float(mse), "mismatch": mismatch, "recon_loss": (float(mse) + 100.0 * mismatch / n) / 2}


def _magnitudes(P, keep, eps, x, x_aug, coef):
    """Section 9m's M, per element of a compared tensor: the sum of the magnitudes of the addends of the sum that makes it.
      x_aug[b, d] = relu(sum_k h10 W11 + b11):        sum_k |h10| |W11| + |b11|
      s = eps sigma + (fc_mu(h5) - mean) rstd:       |eps| sigma + (sum_k |h5| |W| + |b| + |mean|) rstd
      dW[n, k] = sum_b dY[b, n] X[b, k],  db[n]:      sum_b M_dY M_X,  sum_b M_dY;   d gamma, d beta of bnz alike
    M_X is |X| for a given input (fc1's dropped-out x, the noise Linear's z0) and the bound above for a computed one: an
    activation h = relu((y - mean) rstd) carries (sum_k |h_prev| |W| + |b| + |mean|) rstd wherever it is not zero -- an h of 1e-6
    made of addends of magnitude 1 is known to 6e-8, not to 6e-14, in any float32 arithmetic.  M_dY = |dY|, except at fc11, whose dY = coef (x_aug - x) [x_aug > 0] is itself a difference of x and a computed value that
    carries the bound above: M_dY = coef (M_x_aug + |x|) [x_aug > 0] (an x_aug of 0.07 made of addends of magnitude 1.2 is known to
    6e-8 x 1.2, not 6e-8 x 0.07, in any float32 arithmetic).  Carrying the bound through all ten BatchNorm backward steps
    as well (M_dY = rstd (M_g + mean M_g + |y^| mean(M_g |y^|)), M_dX = M_dY |W|) was tried: it grows about tenfold a layer, so that
    float32's error over M falls below 2^-23 from fc9 down and the gate would say nothing there; the upstream gradient's own
    magnitude stands for its bound instead."""
    M, lin, lin_in, pre = {}, keep["lin"], keep["lin_in"], keep["pre"]

    def last_sum(name):          # of a Linear's output: sum_k |X| |W| + |b|
        m = lin_in[name].abs() @ P[name + ".weight"].abs().T
        return m + P[name + ".bias"].abs() if name + ".bias" in P else m

    def normalised(name, eps_bn):      # of a BatchNorm's output (y - mean) rstd
        y = lin[name]
        mean = y.mean(0)
        return (last_sum(name) + mean.abs()) / torch.sqrt(((y - mean) ** 2).mean(0) + eps_bn)

    M["x_aug"] = last_sum("fc11")
    M["s"] = eps.abs() * keep["sigma"] + normalised("fc_mu", BN_EPS)
    # the bound a computed Linear input carries into dW: h_i = relu(y^_i), fc6's s, fc5's cat(h4, elu(y^ gamma + beta))
    MX = {"fc1": lin_in["fc1"].abs(), "noise": lin_in["noise"].abs(), "fc6": M["s"]}
    for i in range(1, 11):
        Mh = normalised(f"fc{i}", BN_EPS) * (keep["h"][i - 1] != 0).to(x.dtype)
        for nxt in ((f"fc{i + 1}",) if i not in (4, 5) else ("fc_mu", "fc_sigma") if i == 5 else ()):
            MX[nxt] = Mh
        if i == 4:
            zb = keep["zb"]
            Mz = (normalised("noise", BNZ_EPS) * P["bnz.weight"].abs() + P["bnz.bias"].abs()) * torch.where(zb > 0, torch.ones_like(zb), torch.exp(zb))
            MX["fc5"] = torch.cat((Mh, Mz), dim=1)
    for name, y in lin.items():
        if y.grad is None:
            continue
        MdY = y.grad.abs() if name != "fc11" else coef * (M["x_aug"] + x.abs()) * (y.grad != 0).to(x.dtype)
        M[name + ".weight"] = MdY.T @ MX[name]
        if name + ".bias" in P:
            M[name + ".bias"] = MdY.sum(0)
    Mg = keep["zb"].grad.abs()
    M["bnz.weight"], M["bnz.bias"] = (Mg * normalised("noise", BNZ_EPS)).sum(0), Mg.sum(0)
    return {k: v.detach() for k, v in M.items()}


def decisions(h_list, x_aug):
    """The ReLU decisions of a run: eleven boolean tensors."""
    return [h > 0 for h in h_list] + [x_aug > 0]

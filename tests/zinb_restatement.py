"""The ZINB heads and loss term restated in torch on the CPU (mmidas/nn_model.py: decoder_zinb :289-295, zinb_loss :642-676),
in the dtype of their inputs: float64 is the truth the device is measured against, float32 is the reference's own arithmetic
whose error sets the device's budget (tests/test_gpu_zinb.py).  tests/test_zinb_cpu.py pins both to the live reference.

The operations and their order are the reference's, so the float32 results are the reference's bit for bit:
``F.linear`` for the three heads, ``(1 - p).pow(r)``, the [X > 0] mask as a float32 factor, the addends of the non-zero
branch subtracted one after the other."""
import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-6


def heads(d10, W, b, Wp, bp, Wr, br):
    """(x_rec, x_p, x_r) [N, D] from d10 [N, H] and the three layers' weight [D, H] and bias [D]."""
    return F.relu(F.linear(d10, W, b)), torch.sigmoid(F.linear(d10, Wp, bp)), torch.sigmoid(F.linear(d10, Wr, br))


def pre_activations(d10, Wp, bp, Wr, br):
    return F.linear(d10, Wp, bp), F.linear(d10, Wr, br)


def terms(rec_x, x_p, x_r, X, eps=EPS):
    """The per-element term whose mean is zinb_loss."""
    k = X.exp() - 1.0
    r = rec_x + eps
    p = (1 - eps) * (x_p + eps)
    z = (1 - eps) * (x_r + eps)
    m = (X > 0).to(torch.float32)
    zero = (m - 1) * (z + (1 - z) * (1 - p).pow(r)).log()
    nonzero = m * (-(k + r).lgamma() + r.lgamma() - k * p.log() - r * (1 - p).log() - (1 - z).log())
    return zero + nonzero


def loss(rec_x, x_p, x_r, X, eps=EPS):
    return terms(rec_x, x_p, x_r, X, eps).mean()


def magnitudes(rec_x, x_p, x_r, X, eps=EPS):
    """M: the sum of the magnitudes of the selected branch's addends, in float64 -- the scale a term's rounding errors live
    on (the addends cancel: lgamma(k + r) and k log p are each hundreds where the term is a few)."""
    rec_x, x_p, x_r, X = (t.double() for t in (rec_x, x_p, x_r, X))
    k = X.exp() - 1.0
    r = rec_x + eps
    p = (1 - eps) * (x_p + eps)
    z = (1 - eps) * (x_r + eps)
    zero = (z + (1 - z) * (1 - p).pow(r)).log().abs()
    nonzero = ((k + r).lgamma().abs() + r.lgamma().abs() + (k * p.log()).abs() + (r * (1 - p).log()).abs()
               + (1 - z).log().abs())
    return torch.where(X > 0, nonzero, zero)


def error_stat(value, truth, M):
    """|value - truth| / M per entry -> (maximum, 90th percentile) as floats; entries with M = 0 must be exact."""
    value, truth, M = (np.asarray(t, dtype=np.float64).ravel() for t in (value, truth, M))
    d = np.abs(value - truth)
    assert np.all(d[M == 0] == 0)
    q = d[M > 0] / M[M > 0]
    return (float(q.max()), float(np.quantile(q, 0.9))) if q.size else (0.0, 0.0)


def counts_matrix(n, D, g, zero_frac=0.7, max_count=1000):
    """X = log1p(counts) float32 [n, D]: counts <= max_count, about zero_frac of them zero; where there are at least two
    rows, row 0 is all zero and row 1 all positive."""
    c = torch.randint(1, max_count + 1, (n, D), generator=g).double()
    c = c * (torch.rand(n, D, generator=g) >= zero_frac)
    if n >= 2:
        c[0] = 0
        c[1] = torch.randint(1, max_count + 1, (D,), generator=g).double()
    return torch.log1p(c).float()


def spread_layers(d10, D, g, spread=8.0):
    """Three layers (W, b, Wp, bp, Wr, br) float32 for d10 [N, H]: fc11 of unit scale, fc11_p / fc11_r scaled so that their
    pre-activations on d10 reach +-spread and stay within it."""
    H = d10.shape[1]
    out = []
    for j in range(3):
        W = torch.randn(D, H, generator=g) / max(H, 1) ** 0.5
        b = 0.5 * torch.randn(D, generator=g)
        if j:
            a = F.linear(d10.double(), W.double(), b.double()).abs().max()
            s = float(spread * 0.98 / max(float(a), 1e-30))
            W, b = W * s, b * s
        out += [W.float(), b.float()]
    return out

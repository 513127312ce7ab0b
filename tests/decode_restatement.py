"""Restatement of the reference's decoder (mmidas/nn_model.py:277-287) and state_changes (:370-411) in plain torch, in the
dtype of the given state dict, for tests/test_decode_cpu.py (against the committed fixture) and tests/test_gpu_decode.py
(against the HIP engine).  Noise is explicit: u [A, n_samp, B] are the reference's torch.rand_like draws."""
import torch

_DEC = ("fc6", "fc7", "fc8", "fc9", "fc10")


def _lin(sd, name, a, x):
    return x @ sd[f"{name}.{a}.weight"].T + sd[f"{name}.{a}.bias"]


def decode_hidden(sd, a, c, s):
    """d6 .. d10 of arm a for rows [c | s]."""
    h = torch.cat((c, s), dim=1)
    out = []
    for name in _DEC:
        h = torch.relu(_lin(sd, name, a, h))
        out.append(h)
    return out


def decode(sd, a, c, s, fc11_round=None):
    """x_rec = relu(fc11(d10)); fc11_round: a function applied to d10, W11 and b11 first (the bf16 engine's rounding)."""
    d10 = decode_hidden(sd, a, c, s)[-1]
    w, b = sd[f"fc11.{a}.weight"], sd[f"fc11.{a}.bias"]
    if fc11_round is not None:
        d10, w, b = fc11_round(d10), fc11_round(w), fc11_round(b)
    return torch.relu(d10 @ w.T + b)


def encode_eval(sd, a, x, tau, eps):
    """Eval-mode encoder + latent block of arm a: (c, mu, v) with c the noise-free hard straight-through sample."""
    h = x
    for i, name in enumerate(("fc1", "fc2", "fc3", "fc4", "fc5")):
        h = torch.relu(_lin(sd, name, a, h))
        bn = f"batch_l{i + 1}.{a}"
        h = (h - sd[f"{bn}.running_mean"]) / torch.sqrt(sd[f"{bn}.running_var"] + eps)
    q = torch.softmax(_lin(sd, "fcc", a, h), dim=-1)
    q = torch.softmax(q / tau, dim=-1)
    hard = torch.zeros_like(q)
    hard.scatter_(1, q.argmax(dim=-1, keepdim=True), 1)
    c = (hard - q) + q
    y = torch.cat((h, c), dim=1)
    return c, _lin(sd, "fc_mu", a, y), torch.sigmoid(_lin(sd, "fc_sigma", a, y))


def state_changes(sd, x, d_s, u, tau=0.005, eps=1e-8, n_arm=2, fc11_round=None):
    """[A, n_samp, B, D] in sample order (no reordering)."""
    n_samp = u.shape[1]
    out = []
    for a in range(n_arm):
        c, mu, v = encode_eval(sd, a, x, tau, eps)
        rows = []
        for i in range(n_samp):
            s = mu.clone()
            s[:, d_s] = u[a, i].to(mu.dtype) * v[:, d_s].log().exp().sqrt() + mu[:, d_s]
            rows.append(decode(sd, a, c, s, fc11_round))
        out.append(torch.stack(rows))
    return torch.stack(out)


def bf16_round(t):
    return t.to(torch.bfloat16).to(t.dtype)

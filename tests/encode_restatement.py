"""Restatement of the reference's encoder (mmidas/nn_model.py:263-269), in eval mode and in training mode at a given dropout
keep-mask, of intermed (:271-275) and of the eval-mode latent block of forward (:330-351) in plain torch, in the dtype of the
given state dict, for tests/test_encode_cpu.py (against the committed fixture) and tests/test_gpu_encode.py (against the HIP
engine)."""
import torch

_ENC = ("fc1", "fc2", "fc3", "fc4", "fc5")


def _lin(sd, name, a, x):
    return x @ sd[f"{name}.{a}.weight"].T + sd[f"{name}.{a}.bias"]


def encoder(sd, a, x, eps=1e-8, training=False, keep=None, p=0.0, momentum=0.01):
    """(x_low, c_prob, bn) of arm a.  training: batch statistics, x multiplied by keep / (1 - p) when a keep-mask is given;
    bn: the BatchNorm buffers of batch_l1..5[a] afterwards (updated copies in training mode, sd's own otherwise)."""
    h = x
    if training and keep is not None:
        h = h * keep.to(h.dtype) / (1.0 - p)
    bn = {}
    for i, name in enumerate(_ENC):
        h = torch.relu(_lin(sd, name, a, h))
        key = f"batch_l{i + 1}.{a}"
        rm, rv, nbt = sd[f"{key}.running_mean"], sd[f"{key}.running_var"], sd[f"{key}.num_batches_tracked"]
        if training:
            mean, var = h.mean(0), h.var(0, unbiased=False)
            n = h.shape[0]
            rm = (1 - momentum) * rm + momentum * mean
            rv = (1 - momentum) * rv + momentum * var * n / (n - 1)
            nbt = nbt + 1
        else:
            mean, var = rm, rv
        bn[f"{key}.running_mean"], bn[f"{key}.running_var"], bn[f"{key}.num_batches_tracked"] = rm, rv, nbt
        h = (h - mean) / torch.sqrt(var + eps)
    return h, torch.softmax(_lin(sd, "fcc", a, h), dim=-1), bn


def intermed(sd, a, y):
    return _lin(sd, "fc_mu", a, y), torch.sigmoid(_lin(sd, "fc_sigma", a, y))


def latent_eval(sd, a, x, tau=0.005, eps=1e-8, mask=None):
    """forward(eval=True)'s latents of arm a: x_low, c_prob, c, c_smp, s_mean, s_logvar, labels.  mask: kept categories."""
    x_low, c_prob, _ = encoder(sd, a, x, eps)
    if mask is not None:
        c = torch.zeros_like(c_prob)
        c[:, mask] = torch.softmax(c_prob[:, mask] / tau, dim=-1)
    else:
        c = torch.softmax(c_prob / tau, dim=-1)
    labels = c.argmax(dim=-1)
    hard = torch.zeros_like(c)
    hard.scatter_(1, labels[:, None], 1)
    c_smp = (hard - c) + c
    mu, var = intermed(sd, a, torch.cat((x_low, c_smp), dim=1))
    return {"x_low": x_low, "c_prob": c_prob, "c": c, "c_smp": c_smp, "s_mean": mu, "s_logvar": (var + eps).log(),
            "labels": labels}

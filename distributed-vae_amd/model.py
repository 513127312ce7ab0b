"""``generate`` of mmidas/model.py:77-149 on the HIP engine.

Same name, keys, shapes and dtypes as the reference (float64 numpy arrays, as its ``np.zeros`` gives them); the forward,
the loss and the labels run on the device, every batch is written into its rows of [A, N, .] device buffers and the host
sees one copy at the end.
"""
from typing import Any, Mapping

import numpy as np
import torch

from . import _native as N
from . import dist as D
from ._utils import mk_masks


def _batch_size(dl) -> int:
    B = dl.batch_size
    if B is None:
        raise ValueError("the loader needs a batch size (rows i * B .. of the outputs belong to batch i)")
    return B


@torch.no_grad()
def fill_latents(dl, jobs, temp=1.0) -> torch.Tensor:
    """One pass over the batches ``(x, index)`` of ``dl``: for every job ``(model, kept, out, counts)`` the model's
    latent-only encode of batch i (``mixVAE_model.encode``, under the category mask ``kept``) lands in rows ``i * B ..`` of
    ``out``, a dict of [A, N, .] device arrays, and ``counts`` (or None) receives the between-arm confusion counts.  Several
    jobs read each batch once.  Returns the batches' indices, float64 [N] on the device.  The models must be in eval mode.
    ``generate(latent_only=True)``, ``evals2`` and ``cpl_mixVAE.encode_dataset`` are this loop."""
    B = _batch_size(dl)
    n_rows = len(dl.dataset)
    dev = next(jobs[0][0].parameters()).device
    inds = torch.zeros(n_rows, dtype=torch.float64, device=dev)
    for i, (x, i_x) in enumerate(dl):
        n_fst, n_lst = i * B, min((i + 1) * B, n_rows)
        x = x.to(dev)
        for f, kept, out, counts in jobs:
            f.encode(x.expand(f.n_arm, -1, -1), temp, mask=kept, out=out, row0=n_fst, counts=counts)
        inds[n_fst:n_lst] = torch.as_tensor(i_x).to(dev).to(torch.int64).to(torch.float64)
    return inds


@torch.no_grad()
def generate(f, dl, latent_only: bool = False) -> Mapping[str, Any]:
    """mmidas/model.py:77-149: the eval-mode forward (``temp=1.0``, ``mask=pruning_mask`` from ``f.fcc[0].bias``) and loss
    of every batch ``(x, index)`` of ``dl``, batch i at rows ``i * B ..``.  Returns ``x_recs`` [A,N,D], ``s_means``,
    ``s_logvars`` [A,N,S], ``cs``, ``c_smps`` [A,N,K], ``x_lows`` [A,N,L], ``inds_x`` [N], ``losses`` (a list of floats, one
    per batch), ``c_dists``, ``c_l2_dists`` (means over batches), ``loss_recs``, ``lls`` [A], ``inds_prune``,
    ``pruning_mask`` and ``preds`` [A,N] (argmax of c, plus one).

    The full form runs forward + loss as ``cpl_mixVAE.eval_model`` does.  ``latent_only=True`` runs the encoder and the
    latent block alone (``mixVAE_model.encode(out=, row0=)``: no decoder, no fc11, no loss) and leaves out ``x_recs``
    -- float64 [A,N,D] in the reference, gigabytes at a real data set's size, and unused by ``evals2`` -- and the loss
    keys ``losses``, ``c_dists``, ``c_l2_dists``, ``loss_recs`` and ``lls``.  ``f.training`` is restored on return (the
    reference leaves the model in eval mode)."""
    if D.is_dist():
        raise NotImplementedError("generate is not data-parallel: run it on one rank, outside the process group")
    A, K, Dm, L, S = f.n_arm, f.n_categories, f.input_dim, f.lowD_dim, f.state_dim
    n_rows = len(dl.dataset)
    B = _batch_size(dl)
    dev = next(f.parameters()).device
    pruning_mask, inds_prune = mk_masks(f.fcc[0].bias)
    f32 = dict(dtype=torch.float32, device=dev)
    out = {"x_low": torch.zeros(A, n_rows, L, **f32), "c": torch.zeros(A, n_rows, K, **f32),
           "c_smp": torch.zeros(A, n_rows, K, **f32), "s_mean": torch.zeros(A, n_rows, S, **f32),
           "s_logvar": torch.zeros(A, n_rows, S, **f32)}
    x_recs = None if latent_only else torch.zeros(A, n_rows, Dm, **f32)
    inds_x = torch.zeros(n_rows, dtype=torch.float64, device=dev)
    loss_vecs = []
    was_training = f.training
    f.eval()
    try:
        if latent_only:
            out["labels"] = torch.zeros(A, n_rows, dtype=torch.int32, device=dev)
            inds_x = fill_latents(dl, [(f, pruning_mask, out, None)], 1.0)
        else:
            for i, (x, i_x) in enumerate(dl):
                n_fst, n_lst = i * B, min((i + 1) * B, n_rows)
                xs = x.to(dev).expand(A, -1, -1)                           # xs = [x for _ in range(A)], model.py:107
                o = f(xs, 1.0, prior_c=0, eval=True, mask=pruning_mask)
                f.loss(o[0], o[1], o[2], xs, o[7], o[8], o[4], o[6], 0)
                loss_vecs.append(f._engine.loss_buf.clone())              # the 9-tuple's scalars, still on the device
                for dst, k in ((out["s_mean"], 7), (out["s_logvar"], 8), (out["c"], 4), (out["c_smp"], 6),
                               (out["x_low"], 3), (x_recs, 0)):
                    dst[:, n_fst:n_lst] = torch.stack(list(o[k]))
                inds_x[n_fst:n_lst] = torch.as_tensor(i_x).to(dev).to(torch.int64).to(torch.float64)
        labels = out["labels"] if latent_only else N.classify(out["c"])    # np.argmax: the first maximum
    finally:
        f.train(was_training)
    to64 = lambda t: t.double().cpu().numpy()
    res = {}
    if not latent_only:
        res["x_recs"] = to64(x_recs)
    res.update({"s_means": to64(out["s_mean"]), "s_logvars": to64(out["s_logvar"]), "cs": to64(out["c"]),
                "c_smps": to64(out["c_smp"]), "x_lows": to64(out["x_low"]), "inds_x": inds_x.cpu().numpy()})
    if not latent_only:
        lv = torch.stack(loss_vecs).double().cpu().numpy() if loss_vecs else np.zeros((0, 5 + 3 * A))
        res.update({"losses": [float(v) for v in lv[:, N.LOSS_TOTAL]],
                    "c_dists": np.mean(lv[:, N.LOSS_CDIST]),
                    "c_l2_dists": np.mean(lv[:, N.LOSS_CL2]),
                    "loss_recs": np.array([np.mean(lv[:, N.LOSS_REC0 + a]) for a in range(A)]),
                    "lls": np.array([np.mean(lv[:, N.LOSS_REC0 + 2 * A + a]) for a in range(A)])})
    res.update({"inds_prune": inds_prune, "pruning_mask": pruning_mask, "preds": to64(labels) + 1.0})
    return res

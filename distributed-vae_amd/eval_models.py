"""``summarize_inference`` of the reference (mmidas/eval_models.py): the per-checkpoint summary of a trained model -- losses,
labels, and for every arm pair the confusion counts and the consensus matrix cut to the kept categories.  The reference
fills each pair's matrix with a Python loop over the cells; here the labels go back to the device once per file and
``mmvae_confmat_accumulate`` / ``mmvae_consensus`` do the counting and the normalisation for all pairs at once."""
from __future__ import annotations

import pickle

import numpy as np
import torch

from . import _native as N
from . import dist as D


def pair_matrices(predicted_label: np.ndarray, Cc: int, device):
    """The confusion counts and ``counts / max(row sum, column sum)`` (along the last axis, 0 where that is 0) of every arm
    pair a < b of 1-based labels [A, N], in the reference's pair order: two float64 arrays [A (A - 1) / 2, C, C]."""
    A = predicted_label.shape[0]
    if A < 2:
        return np.zeros((0, Cc, Cc)), np.zeros((0, Cc, Cc))
    labels = torch.from_numpy(np.ascontiguousarray(predicted_label).astype(np.int64) - 1).to(device=device, dtype=torch.int32)
    counts = N.confmat_accumulate(labels, Cc)
    _, norm = N.consensus(counts, want_norm=True)
    host = torch.stack((counts.to(torch.float64), norm)).cpu().numpy()      # integer counts: exact in float64
    return host[0], host[1]


def summarize_inference(cpl, files, dl, saving_folder=""):
    """Inference summary of the checkpoints ``files`` (a list, or one path) on the loader ``dl``: ``cpl.load_model(file)`` and
    ``cpl.eval_model(dl)`` per file, and the reference's dictionary, key for key with its shapes and dtypes:

    ``recon_loss`` [A][file]; ``dc``, ``d_qc``, ``pred_label``, ``prune_indx``, ``sample_id``, ``num_pruned`` per file;
    ``consensus``, ``armA_vs_armB`` (float64 [kept, kept]), ``con_min``, ``con_mean`` per file and arm pair; ``nprune_indx``,
    ``state_mu``, ``state_var``, ``c_prob``, ``lowD_x`` of the last file; ``x_rec`` empty.  Saved as
    ``summary_performance_K_{C}_narm_{A}.p`` under ``saving_folder`` when that is given.

    Every label is taken to lie in 1..C, as ``eval_model``'s ``argmax + 1`` does: ``con_mean`` counts the cells outside the
    diagonal of the (0, 1) pair's confusion counts, and a label outside that range has no cell there.

    The reference's oddities are kept: ``con_mean`` is the agreement of arms 0 and 1 for every pair, ``num_pruned`` holds
    ``list(range(C))`` per file, and the pruned categories are cut only after the normalisation.  Departures: ``ref_prior``
    raises NotImplementedError (as ``eval_model``), an empty ``files`` raises ValueError (the reference dies on an unbound
    name), and the call is not data-parallel."""
    if D.is_dist():
        raise NotImplementedError("summarize_inference is not data-parallel: run it on one rank, outside the process group")
    if cpl.ref_prior:
        raise NotImplementedError("ref_prior is rejected by the reference loss (nn_model.py:578)")
    A, Cc = cpl.n_arm, cpl.n_categories
    files = [files] if not isinstance(files, list) else files
    if not files:
        raise ValueError("summarize_inference: no model file given")
    recon_loss = [[] for _ in range(A)]
    label_pred, dist_c, dist_qc, n_pruned, con_min, con_mean = [], [], [], [], [], []
    prune_indx, consensus, a_vs_b, sample_id = [], [], [], []
    for file in files:
        print(f"Model {file[file.rfind('/'):]}")
        cpl.load_model(file)
        evals = cpl.eval_model(dl)
        predicted_label = evals["predicted_label"]
        dist_c.append(evals["total_dist_z"])
        dist_qc.append(evals["total_dist_qz"])
        prune_indx.append(evals["prune_indx"])
        sample_id.append(evals["data_indx"])
        label_pred.append(predicted_label)
        for a in range(A):
            recon_loss[a].append(evals["total_loss_rec"][a])
        nprune_indx = np.where(np.isin(range(Cc), evals["prune_indx"]) == False)[0]   # noqa: E712
        counts, norm = pair_matrices(predicted_label, Cc, cpl.device)
        if A > 1:
            n_cells = predicted_label.shape[1]
            # the cells whose arms 0 and 1 differ: every cell is in the pair's counts once, the agreeing ones on the diagonal
            differ = np.int64(n_cells - int(np.trace(counts[0])))
        for pair in range(counts.shape[0]):
            _consensus = norm[pair][:, nprune_indx][nprune_indx]
            consensus.append(_consensus)
            con_min.append(np.min(np.diag(_consensus)))
            con_mean.append(1.0 - (differ / n_cells))
            a_vs_b.append(counts[pair][:, nprune_indx][nprune_indx])
        n_pruned.append(list(range(Cc)))
    summary = {
        "recon_loss": recon_loss,
        "dc": dist_c,
        "d_qc": dist_qc,
        "con_min": con_min,
        "con_mean": con_mean,
        "num_pruned": n_pruned,
        "pred_label": label_pred,
        "consensus": consensus,
        "armA_vs_armB": a_vs_b,
        "prune_indx": prune_indx,
        "nprune_indx": nprune_indx,
        "state_mu": evals["state_mu"],
        "state_var": evals["state_var"],
        "sample_id": sample_id,
        "c_prob": evals["z_prob"],
        "lowD_x": evals["x_low"],
        "x_rec": [],
    }
    if saving_folder:
        with open(saving_folder + "/summary_performance_K_" + str(Cc) + "_narm_" + str(A) + ".p", "wb") as fh:
            pickle.dump(summary, fh)
    return summary

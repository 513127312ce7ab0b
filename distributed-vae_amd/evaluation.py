"""The reference's top-level ``evaluation.py``: the numbers it reports about a trained model -- the adjusted mutual
information between every cell type and every cluster (``mutinfo``), its average over the cell types (``avg``) and the
between-arm agreement of the labels (``avg_consensus``).

The reference calls ``sklearn.metrics.adjusted_mutual_info_score`` once per (cell-type column, occupied cluster) on two
binary labelings of all cells.  Such a pair is three integers -- the ones of each labeling and the ones they share -- so here
one launch counts the contingency of every (arm, column, cluster) (``mmvae_mutinfo_counts``) and one launch evaluates
sklearn's formula on all of them in fp64 (``mmvae_ami_binary``)."""
from __future__ import annotations

import glob as _glob
from typing import Any, Dict, List

import numpy as np
import torch

from . import _native as N
from . import dist as D
from .cpl_mixvae import get_device
from .eval_models import summarize_inference


def _targets_on_device(targets, device):
    """(the 0/1 matrix as uint8 on ``device``, the reference's row count F_used)."""
    t = targets.detach().cpu().numpy() if isinstance(targets, torch.Tensor) else np.asarray(targets)
    if t.ndim != 2 or t.shape[1] < 1:
        raise ValueError(f"mutinfo: targets of shape {t.shape} are no [N, F] matrix")
    if not ((t == 0) | (t == 1)).all():
        raise ValueError("mutinfo: targets must be a 0/1 matrix")
    f_used = len(np.unique(np.argmax(t, axis=-1))) if t.shape[0] else 0
    return torch.from_numpy(np.ascontiguousarray(t.astype(np.uint8))).to(device), f_used


def _labels_on_device(z_prob, device):
    """argmax over the last axis (first maximum, as np.argmax) of [A, N, C] probabilities -> int32 [A, N] on ``device``.
    float32 data is classified on the device; other data (the reference's float64) on the host when rounding it to float32
    would change a value, so that no tie appears that the reference does not see."""
    if isinstance(z_prob, torch.Tensor):
        if z_prob.dtype == torch.float32:
            return N.classify(z_prob.to(device))
        z_prob = z_prob.detach().cpu().numpy()
    z = np.asarray(z_prob)
    z32 = z.astype(np.float32)
    if np.array_equal(z32.astype(z.dtype), z):
        return N.classify(torch.from_numpy(np.ascontiguousarray(z32)).to(device))
    return torch.from_numpy(np.argmax(z, axis=-1).astype(np.int32)).to(device)


def mutinfo_arms(z_prob, targets, device=None) -> List[np.ndarray]:
    """``mutinfo`` for every arm of ``z_prob`` [A, N, C] at once: one counts launch and one adjusted-MI launch for all arms;
    a list of A float64 arrays [F_used, K_occupied(arm)]."""
    if D.is_dist():
        raise NotImplementedError("mutinfo is not data-parallel: run it on one rank, outside the process group")
    device = get_device(device)
    if len(z_prob.shape) != 3:
        raise ValueError(f"mutinfo_arms: z_prob of shape {tuple(z_prob.shape)} is not [A, N, C]")
    A, n, Cc = (int(v) for v in z_prob.shape)
    tg, f_used = _targets_on_device(targets, device)
    if tg.shape[0] != n:
        raise ValueError(f"mutinfo: {tg.shape[0]} target rows for {n} cells")
    if n == 0:
        return [np.zeros((0, 0)) for _ in range(A)]
    labels = _labels_on_device(z_prob, device)
    counts, t_sum, p_sum = N.mutinfo_counts(labels, tg, Cc, f_used)
    ami = N.ami_binary(counts, t_sum, p_sum, n)
    ami, occupied = ami.cpu().numpy(), (p_sum > 0).cpu().numpy()
    return [ami[a][:, occupied[a]] for a in range(A)]


def mutinfo(probs, targets, device=None) -> np.ndarray:
    """evaluation.py::mutinfo: float64 [F_used, K_occupied], entry (f, k) = sklearn's ``adjusted_mutual_info_score`` of the
    binary labelings ``targets[:, f]`` and ``[argmax(probs) == k-th occupied category]`` (occupied categories ascending).

    Two quirks of the reference are kept: F_used is the number of distinct ``argmax(targets, -1)`` values and indexes the
    columns 0..F_used-1, so a class without cells shifts nothing and the last columns drop out.  ``targets`` must be a 0/1
    matrix (ValueError otherwise): the reference would hand any other value to sklearn as one more class of that column."""
    return mutinfo_arms(probs[None], targets, device)[0]


def avg(A) -> float:
    return np.mean(np.max(A, axis=-1)).item()


def avg_consensus(A, device=None) -> Dict[str, float]:
    """evaluation.py::avg_consensus of a label matrix [arms, N] (any values, any number of arms: equal is equal): ``all``
    the share of cells on which every arm agrees, ``pairwise`` the mean over the arm pairs i < j of the share on which the
    two agree (1.0 for one arm).  The agreeing cells are counted on the device (integer counts, so each share is the exact
    ratio the reference's ``np.mean`` of booleans gives) and accumulated in the reference's pair order."""
    if D.is_dist():
        raise NotImplementedError("avg_consensus is not data-parallel: run it on one rank, outside the process group")
    device = get_device(device)
    labels = (A.detach() if isinstance(A, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(A))).to(device)
    arms, n = labels.shape
    pairs = [(i, j) for i in range(arms) for j in range(i + 1, arms)]           # the reference's order: for i: for j > i
    counts = [(labels == labels[:1]).all(dim=0).sum()] + [(labels[i] == labels[j]).sum() for i, j in pairs]
    counts = torch.stack(counts).cpu().numpy()                                   # one copy
    res = {"all": np.float64(int(counts[0]) / n).item()}
    if arms == 1:
        res["pairwise"] = 1.0
        return res
    total = 0.0
    for k in counts[1:]:
        total += np.float64(k) / n
    res["pairwise"] = (total / len(pairs)).item()
    return res


def parse_epoch(s: str):
    """The epoch number of a checkpoint name ``..._epoch_<n>.<ext>``, or the name itself (sorting then fails across kinds,
    as in the reference)."""
    try:
        return int("".join(s.split(".")[:-1]).split("_epoch_")[-1])
    except Exception:
        return s


def evaluate(cpl, model_file: str, dl, targets) -> Dict[str, Any]:
    """What the reference's ``main`` computes once everything is loaded: ``summarize_inference`` of one checkpoint
    (``model_file``: a path, or a glob pattern of which the highest ``parse_epoch`` is taken), the average adjusted mutual
    information of every arm against ``targets`` and the consensus of the arms' labels:
    ``{'pairwise', 'all', 'mi' [A], 'avg_mi', 'arms'}``."""
    if D.is_dist():
        raise NotImplementedError("evaluate is not data-parallel: run it on one rank, outside the process group")
    if _glob.has_magic(model_file):
        found = _glob.glob(model_file)
        if not found:
            raise FileNotFoundError(f"evaluate: no checkpoint matches {model_file}")
        model_file = max(found, key=parse_epoch)
    preds = summarize_inference(cpl, model_file, dl)
    tg = targets.detach().cpu().numpy() if isinstance(targets, torch.Tensor) else np.asarray(targets)
    mis = [avg(m) for m in mutinfo_arms(preds["c_prob"], tg.astype(int), cpl.device)]
    consensus = avg_consensus(preds["pred_label"][0], cpl.device)
    return {"pairwise": consensus["pairwise"], "all": consensus["all"], "mi": mis, "avg_mi": np.mean(mis).item(),
            "arms": cpl.n_arm}

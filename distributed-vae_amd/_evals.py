"""Cross-run evaluation: ``evals2`` of mmidas/_evals.py:8-230 and the arithmetic of ``compute_consensus_statistics``
(mmidas/_utils.py:157-276) on the HIP engine.

The reference runs ``generate`` on both models, copies everything to the host and fills one confusion matrix and one
probability-distance matrix per arm pair with a Python loop over the cells.  Here both models ``encode`` every batch into
device buffers (no decoder, no ``x_recs``), one ``pair_stats`` launch fills all matrices from one pair table,
``pair_stats_finish`` normalises them, and the host receives the finished matrices and the probabilities in one copy.
"""
from typing import Any, List, Mapping, Tuple

import numpy as np
import torch

from . import _native as N
from . import dist as D
from ._utils import mk_masks, reassign
from .model import fill_latents


def pair_table(Aa: int, Ab: int, b0=None) -> Tuple[List[Tuple[int, int, int, int]], Tuple[int, int, int]]:
    """The arm pairs of ``evals2`` as rows ``(lab1, prob1, lab2, prob2)`` for ``pair_stats``, and the lengths of the three
    sections, in the reference's list order: cross (for a in run a, for b in run b, _evals.py:51-52), within run a
    (:51, :98) and within run b (:145-146).  Arms are numbered run a first, run b from ``b0`` (default ``Aa``; 0 when both
    runs are one model encoded once).  In the within-run loops the second labels are those of arm ``a + 1 + j`` but the
    second probabilities are ``qcas[j]`` / ``qcbs[j]``: j is the enumerate index of ``preds[a + 1:]`` (_evals.py:98, :106
    and :146, :154)."""
    b0 = Aa if b0 is None else b0
    cross = [(a, a, b0 + b, b0 + b) for a in range(Aa) for b in range(Ab)]
    in_a = [(a, a, a + 1 + j, j) for a in range(Aa) for j in range(Aa - a - 1)]
    in_b = [(b0 + a, b0 + a, b0 + a + 1 + j, b0 + j) for a in range(Ab) for j in range(Ab - a - 1)]
    return cross + in_a + in_b, (len(cross), len(in_a), len(in_b))


def _encode_runs(fa, fb, dl):
    """One pass over ``dl``: labels int32 [T, N] and c float32 [T, N, K] of run a's arms followed by run b's, on the device
    (T = Aa when ``fb is fa``: encoded once), and each run's ``mk_masks``."""
    same = fb is fa
    models = [fa] if same else [fa, fb]
    K = fa.n_categories
    T = sum(m.n_arm for m in models)
    n_rows = len(dl.dataset)
    dev = next(fa.parameters()).device
    labels = torch.zeros(T, n_rows, dtype=torch.int32, device=dev)
    cs = torch.zeros(T, n_rows, K, dtype=torch.float32, device=dev)
    masks = [mk_masks(m.fcc[0].bias) for m in models]
    was = [m.training for m in models]
    jobs, a0 = [], 0
    for m, (keep, _) in zip(models, masks):
        jobs.append((m, keep, {"c": cs[a0:a0 + m.n_arm], "labels": labels[a0:a0 + m.n_arm]}, None))
        a0 += m.n_arm
    try:
        for m in models:
            m.eval()
        fill_latents(dl, jobs, 1.0)
    finally:
        for m, w in zip(models, was):
            m.train(w)
    return labels, cs, masks


@torch.no_grad()
def evals2(fa, fb, dl, eps=1e-9) -> Mapping[str, Any]:
    """mmidas/_evals.py:8-230 for two ``mixVAE_model`` s on the device: the reference's dictionary key for key, every list
    in the reference's order, float64 numpy values.  With C = K = ``fa.n_categories``, labels = argmax of c under each run's
    own pruning mask (``generate``), pm the confusion counts of an arm pair, emp the per-matrix-cell sum of
    ``|qa[i1] - qb[i2]|`` and smp[j] = max(row sum j, column sum j) of pm:

    * ``consensus`` / ``consensus_a`` / ``consensus_b``: ``confmat_normalize(pm)`` of every cross pair (a of fa, b of fb) /
      pair a < b of fa / of fb, the FULL K x K matrices (:77, :125, :173), while ``pm*``, ``dist_l2*`` (= emp / smp[j]) and
      ``emp_l2*`` are cut to ``[inds_unpruned][:, inds_unpruned]`` (:78-80, :91-96).
    * ``pm`` holds every cross pair TWICE in a row (appended at :91 and again at :94); ``pm_a`` / ``pm_b`` once.
    * ``dist_log``, ``dist_log_a``, ``dist_log_b`` and ``emp_log_a`` are empty lists (their appends are commented out,
      :93, :141, :143, :189); ``emp_log`` holds one all-zero cut matrix per cross pair (:58, :96); the reference returns
      no ``emp_log_b``.
    * ``inds_unpruned`` comes from ``fa`` alone (``outs_a["inds_prune"]``, :20, :72) and cuts the ``_b`` lists too (:169).
    * ``consensus_min*`` is the minimum of the full diagonal, pruned categories (zeros) included (:86, :134, :182).
    * ``consensus_mean`` is ``confmat_mean(reassign(consensus))`` (:90); ``consensus_mean_a`` / ``consensus_mean_b`` are
      plain ``confmat_mean`` without ``reassign`` (:138, :186).
    * within a run, the pair (a, a + 1 + j) takes its second probability row from arm j, the enumerate index of
      ``preds[a + 1:]`` (``qcas[b]`` at :106, ``qcbs[b]`` at :154), not from arm a + 1 + j: mirrored, see ``pair_table``.
    * ``consensus_vec``: ``confmat_mean(confmat_normalize(...))`` of the pairs a < b of ``fa`` (:194-199).
    * ``cs_a`` / ``cs_b``: ``generate``'s ``cs`` [A, N, K] of each run.  ``eps`` is unused, as in the reference.

    Both models encode every batch of ``dl`` once (``fb is fa``: one model, once) into device buffers; labels and
    probabilities stay there until the finished matrices come back in one copy.  ``fa`` and ``fb`` must agree on
    ``n_categories`` and ``input_dim`` (ValueError); their arm counts may differ.  Not data-parallel."""
    if D.is_dist():
        raise NotImplementedError("evals2 is not data-parallel: run it on one rank, outside the process group")
    if fa.n_categories != fb.n_categories or fa.input_dim != fb.input_dim:
        raise ValueError(f"evals2: the runs differ in n_categories ({fa.n_categories}, {fb.n_categories}) or input_dim "
                         f"({fa.input_dim}, {fb.input_dim})")
    K, Aa, Ab = fa.n_categories, fa.n_arm, fb.n_arm
    same = fb is fa
    labels, cs, masks = _encode_runs(fa, fb, dl)
    pairs, (n_x, n_a, n_b) = pair_table(Aa, Ab, 0 if same else Aa)
    counts, acc = N.pair_stats(labels, cs, pairs, K)
    fin = N.pair_stats_finish(counts, acc)
    # the one copy: counts and probabilities widened to float64 on the device (exact) behind the finished matrices
    host = torch.cat((counts.to(torch.float64).reshape(-1), fin["packed"], cs.to(torch.float64).reshape(-1))).cpu().numpy()
    P, m = len(pairs), len(pairs) * K * K
    pm_all = host[0:m].reshape(P, K, K)
    cm_norm = host[m:2 * m].reshape(P, K, K)
    emp = host[2 * m:3 * m].reshape(P, K, K)
    dist = host[3 * m:4 * m].reshape(P, K, K)
    diag_mean, diag_min = host[4 * m:4 * m + P], host[4 * m + P:4 * m + 2 * P]
    cs64 = host[4 * m + 2 * P:].reshape(cs.shape)
    cs_a = cs64[:Aa].copy()
    cs_b = cs64[:Aa].copy() if same else cs64[Aa:].copy()

    inds_prune = masks[0][1]
    inds_unpruned = np.where(np.isin(range(K), inds_prune) == False)[0]   # noqa: E712  (_evals.py:72)
    cut = lambda mat: mat[inds_unpruned][:, inds_unpruned].copy()
    res = {k: [] for k in ("consensus", "consensus_min", "consensus_mean", "pm", "dist_l2", "dist_log", "emp_l2", "emp_log")}
    for p in range(n_x):
        res["consensus"].append(cm_norm[p].copy())
        res["consensus_min"].append(diag_min[p])
        res["consensus_mean"].append(np.mean(np.diag(reassign(cm_norm[p]))))
        res["pm"].append(cut(pm_all[p]))
        res["pm"].append(cut(pm_all[p]))
        res["dist_l2"].append(cut(dist[p]))
        res["emp_l2"].append(cut(emp[p]))
        res["emp_log"].append(cut(np.zeros((K, K))))
    side = {}
    for tag, p0, cnt in (("a", n_x, n_a), ("b", n_x + n_a, n_b)):
        rng = range(p0, p0 + cnt)
        side[tag] = {"consensus": [cm_norm[p].copy() for p in rng], "consensus_min": [diag_min[p] for p in rng],
                     "consensus_mean": [diag_mean[p] for p in rng], "pm": [cut(pm_all[p]) for p in rng],
                     "dist_l2": [cut(dist[p]) for p in rng], "emp_l2": [cut(emp[p]) for p in rng]}
    a, b = side["a"], side["b"]
    return {
        "consensus": res["consensus"],
        "consensus_vec": list(a["consensus_mean"]),       # the same pairs a < b of fa, the same arithmetic (:194-199)
        "consensus_min": res["consensus_min"],
        "consensus_mean": res["consensus_mean"],
        "pm": res["pm"],
        "consensus_a": a["consensus"],
        "consensus_min_a": a["consensus_min"],
        "consensus_mean_a": a["consensus_mean"],
        "pm_a": a["pm"],
        "consensus_b": b["consensus"],
        "consensus_min_b": b["consensus_min"],
        "consensus_mean_b": b["consensus_mean"],
        "pm_b": b["pm"],
        "inds_unpruned": inds_unpruned,
        "cs_a": cs_a,
        "cs_b": cs_b,
        "dist_l2": res["dist_l2"],
        "dist_log": [],
        "emp_l2": res["emp_l2"],
        "emp_log": res["emp_log"],
        "dist_l2_a": a["dist_l2"],
        "dist_log_a": [],
        "emp_l2_a": a["emp_l2"],
        "emp_log_a": [],
        "dist_l2_b": b["dist_l2"],
        "dist_log_b": [],
        "emp_l2_b": b["emp_l2"],
    }


def statistics_from_evals(cross: Mapping[Tuple[Any, Any], Mapping[str, Any]], within: Mapping[Any, Mapping[str, Any]],
                          A: int) -> Mapping[str, Any]:
    """The arithmetic of mmidas/_utils.py:146-276 on ``evals2`` results: ``cross[(ra, rb)]`` for every run pair in the
    reference's order, ``within[r] = evals2(f_r, f_r)``.  Per run pair, ``np.mean(np.diag(reassign(.)))`` of ``consensus[i]``
    and ``dist_l2[i]`` for every i = a * A + b (:162-180); per run, for the i with b > a (:195-214); their means and
    standard deviations, and the totals over all within-run / between-run values.  The ``log`` entries stay empty, so their
    totals are ``np.mean([])`` = NaN, as in the reference."""
    css, stds, means, l2s, stds_l2, means_l2, logs, stds_log, means_log = ({} for _ in range(9))

    def score(key, ev, keep):
        xs_c, xs_l = [], []
        i = 0
        for a in range(A):
            for b in range(A):
                if keep(a, b):
                    xs_c.append(np.mean(np.diag(reassign(ev["consensus"][i]))))
                    xs_l.append(np.mean(np.diag(reassign(ev["dist_l2"][i]))))
                    logs.setdefault(key, [])
                    stds_log.setdefault(key, [])
                    means_log.setdefault(key, [])
                i += 1
        css[key], l2s[key] = np.array(xs_c), np.array(xs_l)
        means[key] = np.mean(css[key])
        stds[key] = np.std(css[key].flatten())
        means_l2[key] = np.mean(l2s[key])
        stds_l2[key] = np.std(l2s[key].flatten())

    for key, ev in cross.items():
        score(key, ev, lambda a, b: True)
    for r, ev in within.items():
        score((r, r), ev, lambda a, b: b > a)
    wc, bc, wl, bl = [], [], [], []
    for ra, rb in css:
        if ra == rb:
            wc += css[(ra, rb)].tolist()
            wl += l2s[(ra, rb)].tolist()
        else:
            bc += css[(ra, rb)].tolist()
            bl += l2s[(ra, rb)].tolist()
    tot = lambda c, l: {"css/mean": np.mean(np.array(c)), "css/std": np.std(np.array(c)), "l2/mean": np.mean(np.array(l)),
                        "l2/std": np.std(np.array(l)), "log/mean": np.mean(np.array([])), "log/std": np.std(np.array([]))}
    return {"consensus": {"xs": css, "stds": stds, "means": means},
            "l2": {"xs": l2s, "stds": stds_l2, "means": means_l2},
            "log": {"xs": logs, "stds": stds_log, "means": means_log},
            "total": {"within_run": tot(wc, wl), "between_run": tot(bc, bl)}}


def consensus_statistics(vaes: Mapping[Any, Any], loader, A: int) -> Mapping[str, Any]:
    """``compute_consensus_statistics`` (mmidas/_utils.py:131-276) after its loading part: ``vaes`` maps run -> model (the
    reference builds it from hard-wired toml paths and ``load_vae``, :134-142), ``loader`` is the data to compare on and A the
    arm count of every run.  ``evals2`` for every run pair ra before rb (:157-160) and for every run against itself (:192-193),
    then ``statistics_from_evals``: the same nested result."""
    if D.is_dist():
        raise NotImplementedError("consensus_statistics is not data-parallel")
    runs = list(vaes)
    cross = {(ra, rb): evals2(vaes[ra], vaes[rb], loader) for j, ra in enumerate(runs) for rb in runs[j + 1:] if ra != rb}
    within = {r: evals2(vaes[r], vaes[r], loader) for r in runs}
    return statistics_from_evals(cross, within, A)

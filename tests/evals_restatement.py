"""A numpy restatement of the reference's cross-run evaluation, written from reading mmidas/_evals.py::evals2,
mmidas/model.py::generate (its label / probability part), mmidas/_utils.py::reassign and the arithmetic of
``compute_consensus_statistics``.  Pure fp64 numpy in the reference's order of operations, with plain loops over the cells:
tests/test_evals_cpu.py pins it to the reference's recorded results (tests/golden/evals2_a3.npz) bit for bit, and the GPU
tests compare the device against it.
"""
import itertools

import numpy as np


def preds_of(cs):
    """generate: ``preds[a] = np.argmax(c, axis=-1) + 1`` as float64 [A, N]; cs float64 [A, N, K]."""
    return (np.argmax(np.asarray(cs), axis=-1) + 1).astype(np.float64)


def inds_of(bias):
    """mk_masks: (pruning_mask, inds_prune) of a bias vector."""
    bias = np.asarray(bias)
    return np.where(bias != 0)[0], np.where(bias == 0)[0]


def reassign(x):
    """Columns of x permuted by a maximum-weight assignment: brute force over the permutations for K <= 7, scipy's solver
    beyond that (imported here, where available)."""
    x = np.asarray(x)
    K = x.shape[0]
    if K <= 7:
        rows = np.arange(K)
        best, arg = -np.inf, None
        for perm in itertools.permutations(range(K)):
            v = x[rows, list(perm)].sum()
            if v > best:
                best, arg = v, list(perm)
        return x[:, arg]
    from scipy.optimize import linear_sum_assignment
    return x[:, linear_sum_assignment(-x)[1]]


def confmat(l1, l2, K):
    m = np.zeros((K, K))
    np.add.at(m, (l1, l2), 1)
    return m


def normalize(cm):
    mx = np.maximum(np.sum(cm, axis=0), np.sum(cm, axis=1))
    return np.divide(cm, mx, out=np.zeros_like(cm), where=mx != 0)


def pair_matrices(pred1, pred2, q1, q2, K):
    """One arm pair: (pm, emp) filled cell by cell; labels are pred - 1, the distance is sqrt((qa[i1] - qb[i2])^2)."""
    pm, emp = np.zeros((K, K)), np.zeros((K, K))
    for c1, c2, qa, qb in zip(pred1, pred2, q1, q2):
        i1, i2 = int(c1) - 1, int(c2) - 1
        pm[i1, i2] += 1
        emp[i1, i2] += np.sqrt((qa[i1] - qb[i2]) ** 2)
    return pm, emp


def _smp(pm, K):
    return np.array([max(pm[c, :].sum(), pm[:, c].sum()) for c in range(K)])


def evals2(preds_a, preds_b, cs_a, cs_b, inds_prune, K, n_arm_a=None):
    """evals2 after its two ``generate`` calls: preds float64 [A, N] (1-based), cs float64 [A, N, K], inds_prune of run a."""
    preds_a, preds_b = np.asarray(preds_a), np.asarray(preds_b)
    A = len(preds_a) if n_arm_a is None else n_arm_a
    iu = np.where(np.isin(range(K), inds_prune) == False)[0]   # noqa: E712
    cut = lambda m: m[iu][:, iu]
    out = {k: [] for k in ("consensus", "consensus_vec", "consensus_min", "consensus_mean", "pm", "consensus_a",
                           "consensus_min_a", "consensus_mean_a", "pm_a", "consensus_b", "consensus_min_b",
                           "consensus_mean_b", "pm_b", "dist_l2", "dist_log", "emp_l2", "emp_log", "dist_l2_a", "dist_log_a",
                           "emp_l2_a", "emp_log_a", "dist_l2_b", "dist_log_b", "emp_l2_b")}

    def one(p1, p2, q1, q2):
        pm, emp = pair_matrices(p1, p2, q1, q2, K)
        smp = _smp(pm, K)
        cons = normalize(confmat(p1.astype(int) - 1, p2.astype(int) - 1, K))
        dist = np.divide(emp, smp, out=np.zeros_like(emp), where=smp != 0)[:, iu][iu]
        return pm, emp, cons, dist

    for a, pa in enumerate(preds_a):
        for b, pb in enumerate(preds_b):
            pm, emp, cons, dist = one(pa, pb, cs_a[a], cs_b[b])
            out["consensus"].append(cons)
            out["consensus_min"].append(np.min(np.diag(cons)))
            out["consensus_mean"].append(np.mean(np.diag(reassign(cons))))
            out["pm"].append(cut(pm))
            out["dist_l2"].append(dist)
            out["pm"].append(cut(pm))                       # the reference appends it a second time
            out["emp_l2"].append(cut(emp))
            out["emp_log"].append(cut(np.zeros((K, K))))
        for j, pb in enumerate(preds_a[a + 1:]):
            pm, emp, cons, dist = one(pa, pb, cs_a[a], cs_a[j])   # the probabilities of arm j, the enumerate index
            out["consensus_a"].append(cons)
            out["consensus_min_a"].append(np.min(np.diag(cons)))
            out["consensus_mean_a"].append(np.mean(np.diag(cons)))
            out["pm_a"].append(cut(pm))
            out["dist_l2_a"].append(dist)
            out["emp_l2_a"].append(cut(emp))
    for a, pa in enumerate(preds_b):
        for j, pb in enumerate(preds_b[a + 1:]):
            pm, emp, cons, dist = one(pa, pb, cs_b[a], cs_b[j])
            out["consensus_b"].append(cons)
            out["consensus_min_b"].append(np.min(np.diag(cons)))
            out["consensus_mean_b"].append(np.mean(np.diag(cons)))
            out["pm_b"].append(cut(pm))
            out["dist_l2_b"].append(dist)
            out["emp_l2_b"].append(cut(emp))
    for a in range(A):
        for b in range(a + 1, A):
            la, lb = preds_a[a].astype(int) - 1, preds_a[b].astype(int) - 1
            out["consensus_vec"].append(np.mean(np.diag(normalize(confmat(la, lb, K)))))
    out["inds_unpruned"] = iu
    out["cs_a"], out["cs_b"] = cs_a, cs_b
    return out


def pair_stats(labels, probs, pairs, K):
    """What mmvae_pair_stats + mmvae_pair_stats_finish compute, for a pair table over arms [T]: labels int [T, n] (0-based,
    entries outside [0, K) skipped), probs float32 [T, n, K].  Returns counts (int64), cm_norm, emp, dist_norm [P, K, K],
    diag_mean, diag_min [P] and smp [P, K]; the distance sums run over the cells in order, in fp64."""
    labels, probs = np.asarray(labels), np.asarray(probs, dtype=np.float64)
    P = len(pairs)
    counts = np.zeros((P, K, K), np.int64)
    emp = np.zeros((P, K, K))
    for p, (l1, p1, l2, p2) in enumerate(pairs):
        i1, i2 = labels[l1].astype(np.int64), labels[l2].astype(np.int64)
        ok = np.flatnonzero((i1 >= 0) & (i1 < K) & (i2 >= 0) & (i2 < K))
        i1, i2 = i1[ok], i2[ok]
        # np.add.at is unbuffered: repeated indices are added one after the other in cell order, as the reference's loop does
        np.add.at(counts[p], (i1, i2), 1)
        np.add.at(emp[p], (i1, i2), np.sqrt((probs[p1, ok, i1] - probs[p2, ok, i2]) ** 2))
    smp = np.maximum(counts.sum(axis=1), counts.sum(axis=2)).astype(np.float64)       # [P, K]: max(column sum, row sum)
    cm = counts.astype(np.float64)
    cm_norm, dist_norm = np.zeros_like(cm), np.zeros_like(cm)
    for p in range(P):
        np.divide(cm[p], smp[p], out=cm_norm[p], where=smp[p] != 0)
        np.divide(emp[p], smp[p], out=dist_norm[p], where=smp[p] != 0)
    diag_mean = np.array([np.mean(np.diag(cm_norm[p])) for p in range(P)])
    diag_min = np.array([np.min(np.diag(cm_norm[p])) for p in range(P)])
    return {"counts": counts, "cm_norm": cm_norm, "emp": emp, "dist_norm": dist_norm, "diag_mean": diag_mean,
            "diag_min": diag_min, "smp": smp}


def consensus_statistics(cross, within, A):
    """compute_consensus_statistics after its evals2 calls: cross[(ra, rb)] / within[r] are evals2 results."""
    css, stds, means, l2s, stds_l2, means_l2, logs, stds_log, means_log = ({} for _ in range(9))
    for (ra, rb), ev in cross.items():
        i = 0
        for a in range(A):
            for b in range(A):
                for d in (css, stds, means, l2s, stds_l2, means_l2, logs, stds_log, means_log):
                    d.setdefault((ra, rb), [])
                css[(ra, rb)].append(np.mean(np.diag(reassign(ev["consensus"][i]))))
                l2s[(ra, rb)].append(np.mean(np.diag(reassign(ev["dist_l2"][i]))))
                i += 1
        css[(ra, rb)], l2s[(ra, rb)] = np.array(css[(ra, rb)]), np.array(l2s[(ra, rb)])
        means[(ra, rb)], stds[(ra, rb)] = np.mean(css[(ra, rb)]), np.std(css[(ra, rb)].flatten())
        means_l2[(ra, rb)], stds_l2[(ra, rb)] = np.mean(l2s[(ra, rb)]), np.std(l2s[(ra, rb)].flatten())
    for r, ev in within.items():
        i = 0
        for a in range(A):
            for b in range(A):
                if b > a:
                    for d in (css, stds, means, l2s, stds_l2, means_l2, logs, stds_log, means_log):
                        d.setdefault((r, r), [])
                    css[(r, r)].append(np.mean(np.diag(reassign(ev["consensus"][i]))))
                    l2s[(r, r)].append(np.mean(np.diag(reassign(ev["dist_l2"][i]))))
                i += 1
        css[(r, r)], l2s[(r, r)] = np.array(css[(r, r)]), np.array(l2s[(r, r)])
        means[(r, r)], stds[(r, r)] = np.mean(css[(r, r)]), np.std(css[(r, r)].flatten())
        means_l2[(r, r)], stds_l2[(r, r)] = np.mean(l2s[(r, r)]), np.std(l2s[(r, r)].flatten())
    w_c, b_c, w_l, b_l, w_g, b_g = [], [], [], [], [], []
    for ra, rb in css:
        if ra == rb:
            w_c += css[(ra, rb)].tolist()
            w_l += l2s[(ra, rb)].tolist()
        else:
            b_c += css[(ra, rb)].tolist()
            b_l += l2s[(ra, rb)].tolist()
    tot = lambda c, l, g: {"css/mean": np.mean(np.array(c)), "css/std": np.std(np.array(c)), "l2/mean": np.mean(np.array(l)),
                           "l2/std": np.std(np.array(l)), "log/mean": np.mean(np.array(g)), "log/std": np.std(np.array(g))}
    return {"consensus": {"xs": css, "stds": stds, "means": means}, "l2": {"xs": l2s, "stds": stds_l2, "means": means_l2},
            "log": {"xs": logs, "stds": stds_log, "means": means_log},
            "total": {"within_run": tot(w_c, w_l, w_g), "between_run": tot(b_c, b_l, b_g)}}

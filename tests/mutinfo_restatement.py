"""numpy fp64 restatement of the reference's model scoring (mmidas/eval_models.py::summarize_inference and the top-level
evaluation.py: mutinfo, avg, avg_consensus), without sklearn: the contingency counts of mmvae_mutinfo_counts, sklearn's
adjusted_mutual_info_score of two binary labelings from the three integers (n11, t, p) and N, and the summary dictionary from
``eval_model`` dictionaries.  Checked against the reference's recorded results (tests/golden/mutinfo_kat.npz,
tests/golden/summary_a3.npz) and against the installed sklearn by tests/test_mutinfo_cpu.py."""
import math

import numpy as np

EPS = float(np.finfo(np.float64).eps)


def counts(labels, targets, F, C):
    """What mmvae_mutinfo_counts adds: labels int [A, n] (labels outside [0, C) are skipped), targets [n, >= F] with non-zero =
    set -> (counts [A, F, C], t_sum [F], p_sum [A, C]) int64."""
    labels = np.asarray(labels)
    T = np.asarray(targets)[:, :F] != 0
    A = labels.shape[0]
    cnt, p_sum = np.zeros((A, F, C), np.int64), np.zeros((A, C), np.int64)
    t_sum = T.sum(axis=0).astype(np.int64)
    for a in range(A):
        ok = (labels[a] >= 0) & (labels[a] < C)
        lab = labels[a][ok].astype(np.int64)
        p_sum[a] = np.bincount(lab, minlength=C)
        for f in range(F):
            cnt[a, f] = np.bincount(lab[T[ok, f]], minlength=C)
    return cnt, t_sum, p_sum


def ami_2x2(n11, t, p, N):
    """(adjusted_mutual_info_score(u, v), normalizer - EMI) of binary labelings u (t ones) and v (p ones) of N cells sharing
    n11 ones, in sklearn's operations (metrics/cluster/_supervised.py, _expected_mutual_info_fast.pyx;
    average_method="arithmetic"); the second value is None in the single-valued special cases."""
    n11, t, p, N = int(n11), int(t), int(p), int(N)
    one_u, one_v = t in (0, N), p in (0, N)
    if one_u and one_v:
        return 1.0, None
    if one_u or one_v:
        return 0.0, None
    a, b = [N - t, t], [N - p, p]
    n = [[N - t - p + n11, p - n11], [t - n11, n11]]
    log_n = math.log(N)
    terms = []
    for i in range(2):
        for j in range(2):
            v = n[i][j]
            if v:
                cnm = v / N
                terms.append(cnm * (math.log(v) - log_n) + cnm * (-math.log(a[i] * b[j]) + log_n + log_n))
    mi = 0.0
    for x in terms:                                   # np.sum of fewer than eight values: in order
        mi += 0.0 if abs(x) < EPS else x
    mi = max(mi, 0.0)
    emi = 0.0
    gl_n = math.lgamma(N + 1)
    for i in range(2):
        for j in range(2):
            ai, bj = a[i], b[j]
            log_a, log_b = math.log(ai), math.log(bj)
            g4 = math.lgamma(ai + 1) + math.lgamma(bj + 1) + math.lgamma(N - ai + 1) + math.lgamma(N - bj + 1)
            for nij in range(max(1, ai - N + bj), min(ai, bj) + 1):
                term2 = (log_n + math.log(nij)) - log_a - log_b
                gln = (g4 - (math.lgamma(nij + 1) + gl_n) - math.lgamma(ai - nij + 1) - math.lgamma(bj - nij + 1)
                       - math.lgamma(N - ai - bj + nij + 1))
                emi += (nij / N) * term2 * math.exp(gln)
    h = lambda k: -((k[0] / N) * (math.log(k[0]) - log_n) + (k[1] / N) * (math.log(k[1]) - log_n))
    den0 = (h(a) + h(b)) / 2.0 - emi
    den = min(den0, -EPS) if den0 < 0 else max(den0, EPS)
    num = mi - emi
    num = min(num, -EPS) if num < 0 else max(num, EPS)
    return num / den, den0


def ami_tables(cnt, t_sum, p_sum, N):
    """mmvae_ami_binary: [A, F, C] float64, NaN where p_sum == 0; and the |normalizer - EMI| of every table that has one."""
    A, F, C = cnt.shape
    out, dens = np.full((A, F, C), np.nan), []
    for a in range(A):
        for c in range(C):
            if p_sum[a, c] == 0:
                continue
            for f in range(F):
                out[a, f, c], d = ami_2x2(cnt[a, f, c], t_sum[f], p_sum[a, c], N)
                if d is not None:
                    dens.append(abs(d))
    return out, np.array(dens)


def f_used(targets):
    """The reference's row count: the number of distinct argmax values, used as the columns 0..F_used-1."""
    return len(np.unique(np.argmax(targets, axis=-1)))


def mutinfo_arms(z_prob, targets, with_dens=False):
    """evaluation.py::mutinfo for every arm of z_prob [A, N, C]: a list of [F_used, K_occupied(arm)] arrays."""
    z_prob, targets = np.asarray(z_prob), np.asarray(targets)
    labels = np.argmax(z_prob, axis=-1)
    F, N, C = f_used(targets), targets.shape[0], z_prob.shape[-1]
    cnt, t_sum, p_sum = counts(labels, targets, F, C)
    ami, dens = ami_tables(cnt, t_sum, p_sum, N)
    res = [ami[a][:, p_sum[a] > 0] for a in range(len(labels))]
    return (res, dens) if with_dens else res


def mutinfo(probs, targets):
    return mutinfo_arms(np.asarray(probs)[None], targets)[0]


def avg(mi):
    return np.mean(np.max(mi, axis=-1)).item()


def avg_consensus(labels):
    """evaluation.py::avg_consensus on a label matrix [A, N]."""
    labels = np.asarray(labels)
    A, N = labels.shape
    every = np.mean([np.sum(np.abs(np.diff(labels[:, i]))) == 0 for i in range(N)]).item()
    if A == 1:
        return {"all": every, "pairwise": 1.0}
    total, k = 0.0, 0
    for i in range(A):
        for j in range(i + 1, A):
            total += np.mean(labels[i] == labels[j])
            k += 1
    return {"all": every, "pairwise": (total / k).item()}


SUMMARY_KEYS = ["recon_loss", "dc", "d_qc", "con_min", "con_mean", "num_pruned", "pred_label", "consensus", "armA_vs_armB",
                "prune_indx", "nprune_indx", "state_mu", "state_var", "sample_id", "c_prob", "lowD_x", "x_rec"]


def summarize(evals_list, A, C):
    """summarize_inference's dictionary from the ``eval_model`` dictionaries of the files, in the reference's operations
    (mmidas/eval_models.py:41-119), oddities included: con_mean from arms 0 and 1 for every pair, num_pruned = range(C) per
    file, nprune_indx / state_mu / state_var / c_prob / lowD_x of the last file, x_rec empty."""
    test_loss = [[] for _ in range(A)]
    out = {k: [] for k in ("dc", "d_qc", "con_min", "con_mean", "num_pruned", "pred_label", "consensus", "armA_vs_armB",
                           "prune_indx", "sample_id")}
    nprune = None
    for ev in evals_list:
        pl = ev["predicted_label"]
        out["dc"].append(ev["total_dist_z"])
        out["d_qc"].append(ev["total_dist_qz"])
        out["prune_indx"].append(ev["prune_indx"])
        out["sample_id"].append(ev["data_indx"])
        out["pred_label"].append(pl)
        for a in range(A):
            test_loss[a].append(ev["total_loss_rec"][a])
        nprune = np.where(np.isin(range(C), ev["prune_indx"]) == False)[0]   # noqa: E712
        for a in range(A):
            for b in range(a + 1, A):
                m = np.zeros((C, C))
                np.add.at(m, (pl[a].astype(int) - 1, pl[b].astype(int) - 1), 1)
                smp = np.array([max(m[c, :].sum(), m[:, c].sum()) for c in range(C)])
                cons = np.divide(m, smp, out=np.zeros_like(m), where=smp != 0)[:, nprune][nprune]
                out["consensus"].append(cons)
                out["con_min"].append(np.min(np.diag(cons)))
                out["con_mean"].append(1.0 - (sum(np.abs(pl[0, :] - pl[1, :]) > 0.0) / pl.shape[1]))
                out["armA_vs_armB"].append(m[:, nprune][nprune])
        out["num_pruned"].append(list(range(C)))
    last = evals_list[-1]
    out.update({"recon_loss": test_loss, "nprune_indx": nprune, "state_mu": last["state_mu"], "state_var": last["state_var"],
                "c_prob": last["z_prob"], "lowD_x": last["x_low"], "x_rec": []})
    return {k: out[k] for k in SUMMARY_KEYS}


def flatten_summary(summary):
    """A summary dictionary as flat ``{key or key/index: array}``, the form tests/golden/summary_a3.npz stores: a list of
    arrays one entry each, anything else as one array."""
    assert list(summary) == SUMMARY_KEYS
    out = {}
    for k, v in summary.items():
        if isinstance(v, list) and v and isinstance(v[0], np.ndarray) and v[0].ndim:
            for i, m in enumerate(v):
                out[f"{k}/{i}"] = m
        else:
            out[k] = np.asarray(v)
    return out


def cut_arms(ev, arms):
    """An ``eval_model`` dictionary reduced to its first ``arms`` arms."""
    out = dict(ev)
    for k in ("state_mu", "state_var", "predicted_label", "z_prob", "x_low", "total_loss_rec"):
        out[k] = ev[k][:arms].copy()
    return out


def fixture_evals(G, arms):
    """The ``eval_model`` dictionaries of tests/golden/summary_a3.npz, cut to ``arms`` arms."""
    evs = []
    for i in range(2):
        ev = {k[len(f"ev{i}/"):]: G[k] for k in G.files if k.startswith(f"ev{i}/")}
        ev["total_dist_z"], ev["total_dist_qz"] = ev["total_dist_z"][()], ev["total_dist_qz"][()]
        evs.append(cut_arms(ev, arms))
    return evs


def assert_same_summary(got, want, exact=True):
    """Two flat summaries: the same keys, shapes, dtypes and (``exact``) bits."""
    assert sorted(got) == sorted(want), sorted(set(got) ^ set(want))
    for k in want:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (k, got[k].shape, want[k].shape, got[k].dtype)
        if exact:
            assert np.array_equal(got[k], want[k]), k

"""Build container only: run the REAL reference scoring code -- ``summarize_inference`` (mmidas/eval_models.py) and
``mutinfo`` / ``avg`` / ``avg_consensus`` (the top-level evaluation.py) -- and commit what it computed as the data-only
fixtures tests/golden/summary_a3.npz and tests/golden/mutinfo_kat.npz (tests/test_mutinfo_cpu.py, tests/test_gpu_mutinfo.py,
tests/test_gpu_summarize.py).

The functions are compiled in memory from the reference files where they lie (``ast``); ``trange`` is ``range``, the other
imports are not needed by the functions taken, ``adjusted_mutual_info_score`` is the installed sklearn's.  The print line of
eval_models.py holds an f-string that only Python >= 3.12 parses; it is neutralised in the text before parsing.  Nothing of
the reference is copied into the repository.

summary_a3.npz: two synthetic ``eval_model`` dictionaries (A = 3, C = 7, N = 150, S = 2, L = 4; labels with about 60 %
agreement between the arms; a different ``prune_indx`` per file; category KEPT_EMPTY kept by both files and taken by no cell)
  ev<i>/<key>          the dictionaries a stub ``cpl`` returns for file i
  a3/<key>[/<index>]   ``summarize_inference``'s result on them; list entries one array each
  a2/<key>[/<index>]   the same for a stub of two arms returning the first two arms of the dictionaries
mutinfo_kat.npz: per case k of CASES = (N, K, F)
  c<k>/probs, c<k>/targets, c<k>/mi   the logits (stored as float16: the reference saw these values as float64), the
                one-hot targets (stored as uint8; the reference saw int64) and the reference's mutinfo
  c<k>/e_ref    the worst |sklearn - exact| over the case's tables: exact = hypergeometric probabilities from Python integers
                (``Fraction``), summed with ``math.fsum``
  c<k>/min_den  the smallest |normalizer - EMI| over the case's tables (the tests' input condition wants >= 1e-3)
  hand/tables, hand/N, hand/ami, hand/e_ref, hand/min_den   tables (n11, t, p) chosen by hand at N = 5000, sklearn's value on
                labelings with these counts, and e_ref / min_den as above
  cons<A>/labels, cons<A>/all, cons<A>/pairwise   avg_consensus on label matrices of A = 1, 2, 3 arms
  avg<k>        avg(c<k>/mi)

    python -m tools.gen_golden_summary
"""
import ast
import math
import os
import re
import sys
from fractions import Fraction

import numpy as np

from oracle import ref_loader as RL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mutinfo_restatement as MR  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
A, C, N, S, L = 3, 7, 150, 2, 4
PRUNE = ([4], [2, 4])
KEPT_EMPTY = 5
CASES = ((64, 3, 3), (257, 5, 9), (300, 7, 6), (2000, 23, 17))
# (n11, t, p) at N = HAND_N: one cell set in either or both labelings; all but one; ranges longer than one pass of a wave
# (independent halves, identical halves); every single-valued special case (t in {0, N}, p = N)
HAND_N = 5000
HAND = ((0, 1, 1), (1, 1, 1), (1, 4999, 1), (2499, 4999, 2500), (1250, 2500, 2500), (2500, 2500, 2500), (0, 0, 2500),
        (2500, 5000, 2500), (0, 0, 5000), (5000, 5000, 5000), (1, 1, 5000))
_EVAL_MODELS = os.path.join(RL.REFERENCE_ROOT, "mmidas", "eval_models.py")
_EVALUATION = os.path.join(RL.REFERENCE_ROOT, "evaluation.py")


def _functions(path, names, ns, patch=None):
    with open(path, "r") as fh:
        text = fh.read()
    if patch:
        text = patch(text)
    tree = ast.parse(text, filename=path)
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert len(keep) == len(names), (path, names)
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, "exec"), ns)
    return ns


def load_reference():
    from sklearn.metrics.cluster import adjusted_mutual_info_score
    # print(f'Model {file[file.rfind('/'):]}'): quotes nested in an f-string, Python >= 3.12 only
    quiet = lambda text: re.sub(r"^(\s*)print\(f'Model .*$", r"\1pass", text, count=1, flags=re.M)
    ens = _functions(_EVAL_MODELS, ("summarize_inference",), {"np": np, "cpl_mixVAE": object, "DataLoader": object}, quiet)
    vns = _functions(_EVALUATION, ("mutinfo", "avg", "avg_consensus", "_avg_consensus", "_avg_consensus_all"),
                     {"np": np, "trange": range, "adjusted_mutual_info_score": adjusted_mutual_info_score})
    vns["adjusted_mutual_info_score"] = adjusted_mutual_info_score
    return ens["summarize_inference"], vns


class StubCpl:
    """What summarize_inference touches of a cpl_mixVAE: n_arm, n_categories, ref_prior, load_model, eval_model."""
    ref_prior = False

    def __init__(self, evals, arms):
        self.n_arm, self.n_categories, self.evals, self.i = arms, C, evals, -1

    def load_model(self, file):
        self.i += 1

    def eval_model(self, dl):
        return self.evals[self.i]


def _eval_dict(rng, prune):
    kept = [c for c in range(C) if c not in prune and c != KEPT_EMPTY]
    base = rng.choice(kept, N)
    labels = np.stack([np.where(rng.random(N) < 0.6, base, rng.choice(kept, N)) for _ in range(A)])
    z = rng.random((A, N, C)).astype(np.float32).astype(np.float64) * 0.5
    z[:, :, prune] = 0.0
    np.put_along_axis(z, labels[..., None], 1.0, axis=-1)
    assert np.array_equal(np.argmax(z, -1), labels)
    return {
        "state_mu": rng.standard_normal((A, N, S)), "state_var": rng.standard_normal((A, N, S)),
        "predicted_label": labels.astype(np.float64) + 1.0, "total_loss_rec": rng.random(A) + 1.0,
        "total_dist_z": np.float64(rng.random()), "total_dist_qz": np.float64(rng.random()),
        "data_indx": rng.permutation(N).astype(np.float64), "z_prob": z, "x_low": rng.standard_normal((A, N, L)),
        "prune_indx": np.array(prune, dtype=np.int64),
    }


def _store_summary(out, prefix, summary):
    for k, v in MR.flatten_summary(summary).items():
        out[f"{prefix}/{k}"] = v


def summary_fixture(summarize_inference):
    rng = np.random.default_rng(2024)
    evals = [_eval_dict(rng, p) for p in PRUNE]
    out = {"cfg": np.array([A, C, N, S, L, KEPT_EMPTY], np.int64)}
    for i, ev in enumerate(evals):
        for k, v in ev.items():
            out[f"ev{i}/{k}"] = np.asarray(v)
        lab = ev["predicted_label"]
        assert not (lab == KEPT_EMPTY + 1).any() and 0.4 < np.mean(lab[0] == lab[1]) < 0.8
    for arms in (3, 2):
        files = [f"run/model_{i}.pth" for i in range(len(evals))]
        _store_summary(out, f"a{arms}", summarize_inference(StubCpl([MR.cut_arms(ev, arms) for ev in evals], arms), files, None))
    path = os.path.join(GOLDEN, "summary_a3.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


def _emi_exact(a, b, n):
    terms = []
    for ai in a:
        for bj in b:
            whole = math.comb(n, bj)
            for k in range(max(1, ai + bj - n), min(ai, bj) + 1):
                pr = Fraction(math.comb(ai, k) * math.comb(n - ai, bj - k), whole)
                terms.append(k / n * math.log(n * k / (ai * bj)) * float(pr))
    return math.fsum(terms)


def ami_exact(n11, t, p, n):
    one_u, one_v = t in (0, n), p in (0, n)
    if one_u or one_v:
        return 1.0 if one_u and one_v else 0.0
    a, b, m = [n - t, t], [n - p, p], [[n - t - p + n11, p - n11], [t - n11, n11]]
    mi = math.fsum(m[i][j] / n * math.log(n * m[i][j] / (a[i] * b[j])) for i in range(2) for j in range(2) if m[i][j])
    h = lambda k: -math.fsum(x / n * math.log(x / n) for x in k)
    emi = _emi_exact(a, b, n)
    return (mi - emi) / (0.5 * (h(a) + h(b)) - emi)


def mutinfo_fixture(vns):
    rng = np.random.default_rng(7)
    out = {"cases": np.array(CASES, np.int64)}
    for k, ((n, K, F), corr) in enumerate(zip(CASES, (0.9, 0.0, 0.7, 0.5))):
        tl = rng.integers(0, F, n)
        if F == 9:
            tl[tl == 4] = 3                      # a class with no cells: F_used = 8, column 4 all zero, column 8 dropped
        targets = np.eye(F, dtype=np.int64)[tl]
        logits = rng.normal(size=(n, K))
        hit = rng.random(n) < corr
        logits[hit, tl[hit] % K] += 4
        probs = logits.astype(np.float16).astype(np.float64)
        mi = vns["mutinfo"](probs, targets)
        labels = np.argmax(probs, -1)
        f_used = MR.f_used(targets)
        cnt, t_sum, p_sum = MR.counts(labels[None], targets, f_used, K)
        occ = np.where(p_sum[0] > 0)[0]
        assert mi.shape == (f_used, len(occ))
        _, dens = MR.ami_tables(cnt, t_sum, p_sum, n)
        e_ref = max(abs(mi[f, j] - ami_exact(int(cnt[0, f, c]), int(t_sum[f]), int(p_sum[0, c]), n))
                    for f in range(f_used) for j, c in enumerate(occ))
        assert n >= 8 and dens.min() >= 1e-3, (n, dens.min())
        out.update({f"c{k}/probs": probs.astype(np.float16), f"c{k}/targets": targets.astype(np.uint8), f"c{k}/mi": mi, f"c{k}/e_ref": np.float64(e_ref),
                    f"c{k}/min_den": np.float64(dens.min()), f"avg{k}": np.float64(vns["avg"](mi))})
        print(f"case {k}: N {n} K {K} F {F} -> mi {mi.shape}, e_ref {e_ref:.2e}, min |den| {dens.min():.3f}")
    # tables by hand at N = HAND_N: (n11, t, p), sklearn on labelings built to have these counts
    ami_sk, vals, errs, dens = vns["adjusted_mutual_info_score"], [], [], []
    for n11, t, p in HAND:
        u, v = np.zeros(HAND_N, np.int64), np.zeros(HAND_N, np.int64)
        u[:t] = 1
        v[:n11] = 1
        v[t:t + p - n11] = 1
        assert u.sum() == t and v.sum() == p and (u & v).sum() == n11
        vals.append(ami_sk(u, v))
        errs.append(abs(vals[-1] - ami_exact(n11, t, p, HAND_N)))
        den = MR.ami_2x2(n11, t, p, HAND_N)[1]
        if den is not None:
            dens.append(abs(den))
    assert min(dens) >= 1e-3, min(dens)
    out.update({"hand/tables": np.array(HAND, np.int64), "hand/N": np.int64(HAND_N), "hand/ami": np.array(vals),
                "hand/e_ref": np.float64(max(errs)), "hand/min_den": np.float64(min(dens))})
    print(f"hand tables at N {HAND_N}: e_ref {max(errs):.2e}, min |den| {min(dens):.2e}", [f"{e:.1e}" for e in errs])
    for arms in (1, 2, 3):
        base = rng.integers(1, 8, 200)
        lab = np.stack([np.where(rng.random(200) < 0.6, base, rng.integers(1, 8, 200)) for _ in range(arms)]).astype(np.float64)
        res = vns["avg_consensus"](lab)
        out.update({f"cons{arms}/labels": lab, f"cons{arms}/all": np.float64(res["all"]),
                    f"cons{arms}/pairwise": np.float64(res["pairwise"])})
    path = os.path.join(GOLDEN, "mutinfo_kat.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


def main():
    summarize_inference, vns = load_reference()
    summary_fixture(summarize_inference)
    mutinfo_fixture(vns)


if __name__ == "__main__":
    main()

"""CPU: the host side of the model scoring (summarize_inference, mutinfo, avg, avg_consensus).  The numpy restatement
(tests/mutinfo_restatement.py) against the reference's own recorded results (tests/golden/mutinfo_kat.npz,
tests/golden/summary_a3.npz; tools/gen_golden_summary.py) and against the installed sklearn; the host-side contract of
mmvae_mutinfo_counts / mmvae_ami_binary: declared, exported, ABI version unchanged, every bad argument refused before any
device work; both new modules importable through the shim, without sklearn or scipy; and the input condition of every table
the GPU tests compare with a tolerance.

Bounds.  The restatement repeats sklearn's operations and differs from it only in the order of the expected-MI sum (and in
libm's lgamma against scipy's gammaln for the five precomputed terms): it is held to 8 x the case's recorded e_ref, the
reference's own distance from exact arithmetic.  Near a zero denominator sklearn's +-2^-52 clamps turn rounding noise into
+-1, so a tolerance comparison needs |normalizer - EMI| >= 1e-3 and N >= 8 of every table; none may be left out."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mutinfo_restatement as MR  # noqa: E402
import distributed_vae_amd  # noqa: F401,E402
from distributed_vae_amd import _native as N  # noqa: E402

K = np.load(os.path.join(ROOT, "tests", "golden", "mutinfo_kat.npz"))
S = np.load(os.path.join(ROOT, "tests", "golden", "summary_a3.npz"))
CASES = [tuple(int(v) for v in row) for row in K["cases"]]
NEW = ("mmvae_mutinfo_counts", "mmvae_debug_mutinfo_counts", "mmvae_ami_binary")
MIN_DEN, MIN_N = 1e-3, 8


def case(k):
    return K[f"c{k}/probs"].astype(np.float64), K[f"c{k}/targets"].astype(np.int64), K[f"c{k}/mi"], float(K[f"c{k}/e_ref"])


# ---- 1. the fixtures are what the generator promises, and the input condition -------------------------------------------
def test_fixture_is_what_the_generator_promises():
    assert CASES == [(64, 3, 3), (257, 5, 9), (300, 7, 6), (2000, 23, 17)]
    for k, (n, Kc, F) in enumerate(CASES):
        probs, targets, mi, e_ref = case(k)
        assert probs.shape == (n, Kc) and targets.shape == (n, F) and (targets.sum(1) == 1).all()
        assert mi.shape == (MR.f_used(targets), len(np.unique(np.argmax(probs, 1)))) and 0 < e_ref < 1e-12
    targets = case(1)[1]
    assert MR.f_used(targets) == 8 and not targets[:, 4].any() and targets[:, 8].any()   # the absent class shifts nothing
    A, Cc, n, _, _, kept_empty = [int(v) for v in S["cfg"]]
    assert (A, Cc, n) == (3, 7, 150)
    assert list(S["ev0/prune_indx"]) != list(S["ev1/prune_indx"])
    for i in range(2):
        lab = S[f"ev{i}/predicted_label"]
        assert kept_empty not in S[f"ev{i}/prune_indx"] and not (lab == kept_empty + 1).any()
        assert 0.4 < np.mean(lab[0] == lab[1]) < 0.8
    assert S["a3/consensus/0"].shape != S["a3/consensus/3"].shape                      # the files keep different categories


def test_input_condition_holds_for_every_table_compared_with_a_tolerance():
    """N >= 8 and |normalizer - EMI| >= 1e-3 for every table of the four cases and of the tables chosen by hand: the cap on
    tables left out is zero."""
    for k, (n, _, _) in enumerate(CASES):
        probs, targets, _, _ = case(k)
        _, dens = MR.mutinfo_arms(probs[None], targets, with_dens=True)
        assert n >= MIN_N and len(dens) and dens.min() >= MIN_DEN, (k, dens.min())
        assert abs(dens.min() - float(K[f"c{k}/min_den"])) < 1e-9
    n = int(K["hand/N"])
    dens = [MR.ami_2x2(*row, n)[1] for row in K["hand/tables"]]
    dens = [abs(d) for d in dens if d is not None]
    assert n >= MIN_N and len(dens) == 6 and min(dens) >= MIN_DEN, min(dens)


# ---- 2. the restatement is the reference's arithmetic -------------------------------------------------------------------
@pytest.mark.parametrize("k", range(4))
def test_restatement_mutinfo_equals_reference_fixture(k):
    probs, targets, mi, e_ref = case(k)
    got = MR.mutinfo(probs, targets)
    assert got.shape == mi.shape and got.dtype == np.float64
    err = float(np.abs(got - mi).max())
    print(f"case {k}: worst |restatement - sklearn| {err:.2e}, e_ref {e_ref:.2e}")
    assert err <= 8 * e_ref
    assert abs(MR.avg(got) - float(K[f"avg{k}"])) <= 8 * e_ref


def test_restatement_hand_tables_equal_reference_fixture():
    n, e_ref = int(K["hand/N"]), float(K["hand/e_ref"])
    got = np.array([MR.ami_2x2(*row, n)[0] for row in K["hand/tables"]])
    assert np.abs(got - K["hand/ami"]).max() <= 8 * e_ref
    assert list(K["hand/ami"][-5:]) == [0.0, 0.0, 1.0, 1.0, 0.0]                       # the single-valued special cases


@pytest.mark.parametrize("arms", [1, 2, 3])
def test_restatement_avg_consensus_equals_reference_fixture(arms):
    got = MR.avg_consensus(K[f"cons{arms}/labels"])
    assert got == {"all": float(K[f"cons{arms}/all"]), "pairwise": float(K[f"cons{arms}/pairwise"])}
    assert isinstance(got["all"], float) and isinstance(got["pairwise"], float)


@pytest.mark.parametrize("arms", [3, 2])
def test_restatement_summary_equals_reference_fixture_bit_for_bit(arms):
    Cc = int(S["cfg"][1])
    got = MR.flatten_summary(MR.summarize(MR.fixture_evals(S, arms), arms, Cc))
    want = {k[3:]: S[k] for k in S.files if k.startswith(f"a{arms}/")}
    MR.assert_same_summary(got, want)
    pairs = arms * (arms - 1) // 2
    assert want["con_mean"].shape == (2 * pairs,) and len(set(want["con_mean"][:pairs])) == 1   # arms 0 and 1 for every pair
    assert want["num_pruned"].shape == (2, Cc) and want["x_rec"].shape == (0,)
    assert list(want["nprune_indx"]) == [c for c in range(Cc) if c not in S["ev1/prune_indx"]]


def test_restatement_against_live_sklearn():
    ami = pytest.importorskip("sklearn.metrics").adjusted_mutual_info_score
    rng = np.random.default_rng(11)
    bound = 8 * max(float(K[f"c{k}/e_ref"]) for k in range(3))     # N <= 300: the recorded cases of that size
    for n in (8, 50, 300):
        for _ in range(6):
            u, v = (rng.random(n) < rng.uniform(0.1, 0.9)).astype(int), (rng.random(n) < rng.uniform(0.1, 0.9)).astype(int)
            if rng.random() < 0.5:
                v[: n // 2] = u[: n // 2]
            got, den = MR.ami_2x2(int((u & v).sum()), int(u.sum()), int(v.sum()), n)
            if den is None or abs(den) >= MIN_DEN:
                assert abs(got - ami(u, v)) <= bound, (n, got)
    for u, v, want in (([0] * 9, [0] * 9, 1.0), ([1] * 9, [0] * 9, 1.0), ([1] * 9, [0] * 8 + [1], 0.0)):
        u, v = np.array(u), np.array(v)
        assert ami(u, v) == want == MR.ami_2x2(int((u & v).sum()), int(u.sum()), int(v.sum()), 9)[0]


def test_restatement_counts():
    lab = np.array([[0, 1, 1, 5, -1, 2], [2, 2, 2, 2, 2, 2]])
    tg = np.array([[1, 0, 9], [1, 1, 9], [0, 1, 9], [1, 1, 9], [1, 0, 9], [0, 0, 9]])
    cnt, t, p = MR.counts(lab, tg, 2, 3)
    assert t.tolist() == [4, 3] and p.tolist() == [[1, 2, 1], [0, 0, 6]]
    assert cnt.tolist() == [[[1, 1, 0], [0, 2, 0]], [[0, 0, 4], [0, 0, 3]]]


# ---- 3. declared, exported, ABI unchanged; importable through the shim -----------------------------------------------------
def test_entry_points_declared_exported_and_abi_unchanged():
    hdr = open(os.path.join(ROOT, "include", "mmvae.h")).read()
    for fn in NEW:
        assert re.search(r"\bint " + fn + r"\(", hdr), fn
    assert re.search(r"\bsize_t mmvae_ami_binary_workspace_bytes\(", hdr)
    src = open(os.path.join(ROOT, "distributed-vae_amd", "csrc", "api.hip")).read()
    assert "int mmvae_abi_version(void) { return 5; }" in src
    lib = N.lib()
    assert lib.mmvae_abi_version() == 5 == N.ABI_VERSION
    for fn in NEW + ("mmvae_ami_binary_workspace_bytes",):
        assert hasattr(lib, fn), fn
    assert lib.mmvae_ami_binary_workspace_bytes(22365) == 2 * 22366 * 8
    assert lib.mmvae_ami_binary_workspace_bytes(0) == 0 == lib.mmvae_ami_binary_workspace_bytes((1 << 31) + 1)


def test_modules_import_through_the_shim_without_sklearn_or_scipy():
    from distributed_vae_amd import eval_models, evaluation
    assert callable(eval_models.summarize_inference)
    for fn in ("mutinfo", "mutinfo_arms", "avg", "avg_consensus", "parse_epoch", "evaluate"):
        assert callable(getattr(evaluation, fn)), fn
    for mod in (eval_models, evaluation):
        assert not re.search(r"^\s*(import|from)\s+(sklearn|scipy)", open(mod.__file__).read(), flags=re.M)
    assert evaluation.parse_epoch("run/model/cpl_mixVAE_model_epoch_500.pth") == 500
    assert evaluation.parse_epoch("run/model/cpl_mixVAE_model_before_pruning.pth") == "run/model/cpl_mixVAE_model_before_pruning.pth"
    assert evaluation.avg(np.array([[0.1, 0.5], [0.7, 0.2]])) == 0.6


def test_targets_outside_zero_one_and_empty_file_list_are_refused():
    from distributed_vae_amd import eval_models, evaluation
    with pytest.raises(ValueError):
        evaluation.mutinfo(np.zeros((4, 3)), np.array([[1, 0], [0, 2], [1, 0], [0, 1]]), device="cpu")

    class Cpl:
        n_arm, n_categories, ref_prior = 2, 4, False
    with pytest.raises(ValueError):
        eval_models.summarize_inference(Cpl(), [], None)
    Cpl.ref_prior = True
    with pytest.raises(NotImplementedError):
        eval_models.summarize_inference(Cpl(), ["x.pth"], None)


# ---- 4. refusals on the host ------------------------------------------------------------------------------------------------
PTR = 0x1000     # fake device pointers: every case must be refused (or succeed as a no-op) before anything dereferences them


def _counts(labels=PTR, A=3, n=10, Cc=7, targets=PTR, tbytes=1, ldt=9, F=9, counts=PTR, t_sum=PTR, p_sum=PTR, path=None):
    if path is None:
        return N.lib().mmvae_mutinfo_counts(labels, A, n, Cc, targets, tbytes, ldt, F, counts, t_sum, p_sum, None)
    return N.lib().mmvae_debug_mutinfo_counts(labels, A, n, Cc, targets, tbytes, ldt, F, counts, t_sum, p_sum, path, None)


COUNTS_CASES = [
    ("null_labels", -1), ("null_targets", -1), ("null_counts", -1), ("null_t_sum", -1), ("null_p_sum", -1), ("A0", -1),
    ("A9", -1), ("C0", -1), ("C_neg", -1), ("C129", -1), ("F0", -1), ("F4097", -1), ("n_neg", -1), ("n_past_2_31", -1),
    ("ldt_below_F", -1), ("tbytes2", -1), ("tbytes0", -1), ("n0", 0)]


@pytest.mark.parametrize("debug", [False, True])
@pytest.mark.parametrize("case,rc", COUNTS_CASES)
def test_mutinfo_counts_rejects_bad_arguments(case, rc, debug):
    kw = {"path": -1} if debug else {}
    if case.startswith("null_"): kw[case[5:]] = None
    elif case == "A0": kw["A"] = 0
    elif case == "A9": kw["A"] = 9
    elif case == "C0": kw["Cc"] = 0
    elif case == "C_neg": kw["Cc"] = -3
    elif case == "C129": kw["Cc"] = 129
    elif case == "F0": kw.update(F=0)
    elif case == "F4097": kw.update(F=4097, ldt=4097)
    elif case == "n_neg": kw["n"] = -1
    elif case == "n_past_2_31": kw["n"] = (1 << 31) + 1
    elif case == "ldt_below_F": kw["ldt"] = 8
    elif case == "tbytes2": kw["tbytes"] = 2
    elif case == "tbytes0": kw["tbytes"] = 0
    elif case == "n0": kw["n"] = 0
    assert _counts(**kw) == rc, N.lib().mmvae_last_error_string()
    if rc:
        assert N.lib().mmvae_last_error_string()


def test_debug_mutinfo_counts_rejects_bad_paths():
    assert _counts(path=2) == -1 and _counts(path=-2) == -1
    assert _counts(path=0, n=0) == 0 and _counts(path=1, n=0) == 0


def _ami(n11=PTR, t_sum=PTR, p_sum=PTR, A=3, F=9, Cc=7, n=100, ws=PTR, ws_bytes=2 * 101 * 8, ami=PTR):
    return N.lib().mmvae_ami_binary(n11, t_sum, p_sum, A, F, Cc, n, ws, ws_bytes, ami, None)


@pytest.mark.parametrize("case,rc", [
    ("null_n11", -1), ("null_t_sum", -1), ("null_p_sum", -1), ("null_ami", -1), ("A_neg", -1), ("A9", -1), ("C0", -1),
    ("C129", -1), ("F0", -1), ("F4097", -1), ("N0", -1), ("N_neg", -1), ("N_past_2_31", -1), ("ws_misaligned", -1),
    ("ws_small", -4), ("A0", 0), ("A0_no_ws", 0)])
def test_ami_binary_rejects_bad_arguments(case, rc):
    kw = {}
    if case.startswith("null_"): kw[case[5:]] = None
    elif case == "A_neg": kw["A"] = -1
    elif case == "A9": kw["A"] = 9
    elif case == "C0": kw["Cc"] = 0
    elif case == "C129": kw["Cc"] = 129
    elif case == "F0": kw["F"] = 0
    elif case == "F4097": kw["F"] = 4097
    elif case == "N0": kw["n"] = 0
    elif case == "N_neg": kw["n"] = -5
    elif case == "N_past_2_31": kw.update(n=(1 << 31) + 1, ws=None, ws_bytes=0)
    elif case == "ws_misaligned": kw["ws"] = PTR + 4
    elif case == "ws_small": kw["ws_bytes"] = 2 * 101 * 8 - 1
    elif case == "A0": kw["A"] = 0
    elif case == "A0_no_ws": kw.update(A=0, ws=None, ws_bytes=0)
    assert _ami(**kw) == rc, N.lib().mmvae_last_error_string()
    if rc:
        assert N.lib().mmvae_last_error_string()


def test_python_wrappers_have_no_cpu_fallback():
    import torch
    lab, tg = torch.zeros(2, 3, dtype=torch.int32), torch.zeros(3, 4, dtype=torch.uint8)
    with pytest.raises(N.NativeError):
        N.mutinfo_counts(lab, tg, 4)
    z = torch.zeros(2, 4, 4, dtype=torch.int64)
    with pytest.raises(N.NativeError):
        N.ami_binary(z, torch.zeros(4, dtype=torch.int64), torch.zeros(2, 4, dtype=torch.int64), 3)

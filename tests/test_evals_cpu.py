"""CPU: the cross-run evaluation's host side.  The numpy restatement (tests/evals_restatement.py) against the reference's own
recorded ``evals2`` results (tests/golden/evals2_a3.npz, tools/gen_golden_evals.py); the package's ``reassign`` against
brute force and scipy; the pair table against the reference's loop structure; and the host-side contract of
mmvae_pair_stats / mmvae_pair_stats_finish: declared, exported, ABI version unchanged, every bad argument refused before
any device work."""
import ctypes as C
import itertools
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import evals_restatement as ER  # noqa: E402
import distributed_vae_amd  # noqa: F401,E402
from distributed_vae_amd import _native as N  # noqa: E402
from distributed_vae_amd._evals import pair_table  # noqa: E402
from distributed_vae_amd._utils import mk_masks, reassign  # noqa: E402

G = np.load(os.path.join(ROOT, "tests", "golden", "evals2_a3.npz"))
A, NC, D, H, L, K, S, BATCH, PRUNED = [int(v) for v in G["cfg"]]
NEW = ("mmvae_pair_stats", "mmvae_pair_stats_finish")
KEYS = [k[3:] for k in G.files if k.startswith("ab/")]
# the reference's return statement, _evals.py:202-230
REF_KEYS = ["consensus", "consensus_vec", "consensus_min", "consensus_mean", "pm", "consensus_a", "consensus_min_a",
            "consensus_mean_a", "pm_a", "consensus_b", "consensus_min_b", "consensus_mean_b", "pm_b", "inds_unpruned", "cs_a",
            "cs_b", "dist_l2", "dist_log", "emp_l2", "emp_log", "dist_l2_a", "dist_log_a", "emp_l2_a", "emp_log_a", "dist_l2_b",
            "dist_log_b", "emp_l2_b"]


def _stacked(v):
    return np.asarray(v, dtype=np.float64) if not isinstance(v, np.ndarray) else v


# ---- 1. the restatement is the reference's arithmetic -------------------------------------------------------------------
def test_fixture_is_what_the_generator_promises():
    assert KEYS == REF_KEYS
    for tag in ("a", "b"):
        cs = np.sort(G[f"gen_{tag}/cs"], axis=-1)
        assert float((cs[..., -1] - cs[..., -2]).min()) > 1e-3                 # no fp32 engine can flip a label
        assert all(len(np.unique(p)) >= 2 for p in G[f"gen_{tag}/preds"])
        assert list(G[f"gen_{tag}/inds_prune"]) == [PRUNED]
        assert not G[f"gen_{tag}/cs"][:, :, PRUNED].any()
    assert G["ab/pm"].shape == (2 * A * A, K - 1, K - 1) and G["ab/consensus"].shape == (A * A, K, K)
    assert np.array_equal(G["ab/pm"][0::2], G["ab/pm"][1::2])                  # every cross pair twice
    for k in ("dist_log", "dist_log_a", "dist_log_b", "emp_log_a"):
        assert G[f"ab/{k}"].shape == (0,)
    assert not G["ab/emp_log"].any()


@pytest.mark.parametrize("case", ["ab", "aa"])
def test_restatement_equals_reference_fixture_bit_for_bit(case):
    ga, gb = "gen_a", ("gen_b" if case == "ab" else "gen_a")
    got = ER.evals2(G[f"{ga}/preds"], G[f"{gb}/preds"], G[f"{ga}/cs"], G[f"{gb}/cs"], G[f"{ga}/inds_prune"], K)
    assert np.array_equal(ER.preds_of(G[f"{ga}/cs"]), G[f"{ga}/preds"])
    assert sorted(got) == sorted(REF_KEYS)
    for k in REF_KEYS:
        want, have = G[f"{case}/{k}"], _stacked(got[k])
        assert have.shape == want.shape, k
        assert np.array_equal(have, want), k


def _lists(case):
    """A fixture result as evals2 returns it: lists of matrices."""
    return {k: list(G[f"{case}/{k}"]) for k in ("consensus", "dist_l2")}


def _same_tree(a, b, path=""):
    if isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b), path
        for k in a:
            _same_tree(a[k], b[k], f"{path}/{k}")
    else:
        x, y = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
        assert x.shape == y.shape and np.array_equal(x, y, equal_nan=True), path


@pytest.mark.filterwarnings("ignore:Mean of empty slice", "ignore:invalid value encountered", "ignore:Degrees of freedom")
def test_statistics_from_evals_equals_restatement_on_the_fixture():
    """The package's statistics (its own assignment solver) and the restatement's (brute force) on the reference's recorded
    evals2 results: the same nested dictionary, bit for bit, NaN for the empty ``log`` entries included."""
    from distributed_vae_amd._evals import statistics_from_evals
    cross, within = {("r0", "r1"): _lists("ab")}, {"r0": _lists("aa"), "r1": _lists("aa")}
    got, want = statistics_from_evals(cross, within, A), ER.consensus_statistics(cross, within, A)
    _same_tree(got, want)
    assert list(got) == ["consensus", "l2", "log", "total"] and list(got["consensus"]["xs"]) == [("r0", "r1"), ("r0", "r0"), ("r1", "r1")]
    assert got["consensus"]["xs"][("r0", "r1")].shape == (A * A,) and got["l2"]["xs"][("r0", "r0")].shape == (A * (A - 1) // 2,)
    assert np.isnan(got["total"]["between_run"]["log/mean"]) and got["log"]["xs"][("r0", "r1")] == []
    assert got["total"]["between_run"]["css/mean"] > 0


# ---- 2. reassign ------------------------------------------------------------------------------------------------------------
def _brute_value(x):
    rows = np.arange(x.shape[0])
    return max(x[rows, list(p)].sum() for p in itertools.permutations(range(x.shape[0])))


def _matrices(K_, rng):
    x = rng.random((K_, K_))
    yield "random", x
    yield "ties", np.round(x * 3) / 3                                     # four distinct values: many equal assignments
    z = x.copy()
    z[:, rng.integers(K_)] = 0.0
    if K_ > 2:
        z[rng.integers(K_), :] = 0.0
    yield "zero_column_and_row", z
    yield "zeros", np.zeros((K_, K_))
    yield "identity", np.eye(K_)
    yield "negative", x - 0.5
    n = ER.normalize(rng.integers(0, 5, (K_, K_)).astype(np.float64))
    yield "normalised_counts", n
    few = np.zeros((K_, K_))                                              # arms that use two or three of the K categories:
    few[np.ix_(rng.integers(0, K_, 2), rng.integers(0, K_, 3))] = rng.random((2, 3))   # all-zero rows and columns elsewhere
    yield "few_labels", few


@pytest.mark.parametrize("K_", [1, 2, 3, 4, 5, 6, 7])
def test_reassign_optimal_value_equals_brute_force(K_):
    rng = np.random.default_rng(100 + K_)
    for _ in range(3 if K_ == 7 else 8):
        for name, x in _matrices(K_, rng):
            r = reassign(x)
            assert r.shape == x.shape
            assert sorted(map(tuple, r.T.tolist())) == sorted(map(tuple, x.T.tolist())), name   # a permutation of the columns
            # equal exact values, each a sum of K entries of at most max|x| in its own order: K 2^-53 max|x| each way
            scale = np.abs(x).max()
            got, want = np.trace(r), _brute_value(x)
            assert abs(got - want) <= K_ * 2.0 ** -52 * scale, (name, got, want)
            assert abs(np.mean(np.diag(ER.reassign(x))) - np.mean(np.diag(r))) <= K_ * 2.0 ** -52 * scale, name


@pytest.mark.parametrize("K_", [7, 33, 92, 128])
def test_reassign_value_matches_scipy(K_):
    lsa = pytest.importorskip("scipy.optimize").linear_sum_assignment
    rng = np.random.default_rng(K_)
    for name, x in _matrices(K_, rng):
        want = np.mean(np.diag(x[:, lsa(-x)[1]]))
        got = np.mean(np.diag(reassign(x)))
        assert abs(got - want) <= K_ * 2.0 ** -52 * abs(want), (name, got, want)


def test_reassign_refuses_non_square_and_mk_masks():
    with pytest.raises(ValueError):
        reassign(np.zeros((3, 4)))
    import torch
    keep, drop = mk_masks(torch.tensor([0.5, 0.0, -1.0, 0.0]))
    assert keep.tolist() == [0, 2] and drop.tolist() == [1, 3] and keep.dtype == drop.dtype == np.int64


# ---- 3. the pair table ------------------------------------------------------------------------------------------------------
def _reference_loops(Aa, Ab):
    """The loop structure of _evals.py:51-191 on arm names: which prediction row and which probability row each zip takes."""
    preds_a, preds_b = [("a", i) for i in range(Aa)], [("b", i) for i in range(Ab)]
    qcas, qcbs = list(preds_a), list(preds_b)
    cross, in_a, in_b = [], [], []
    for a, pred_a in enumerate(preds_a):
        for b, pred_b in enumerate(preds_b):
            cross.append((pred_a, qcas[a], pred_b, qcbs[b]))
        for b, pred_b in enumerate(preds_a[a + 1:]):
            in_a.append((pred_a, qcas[a], pred_b, qcas[b]))
    for a, pred_a in enumerate(preds_b):
        for b, pred_b in enumerate(preds_b[a + 1:]):
            in_b.append((pred_a, qcbs[a], pred_b, qcbs[b]))
    return cross, in_a, in_b


@pytest.mark.parametrize("Aa,Ab", [(2, 2), (3, 3), (5, 5), (2, 3), (5, 2), (1, 3)])
def test_pair_table_is_in_reference_order(Aa, Ab):
    cross, in_a, in_b = _reference_loops(Aa, Ab)
    tab, sizes = pair_table(Aa, Ab)
    assert sizes == (len(cross), len(in_a), len(in_b)) == (Aa * Ab, Aa * (Aa - 1) // 2, Ab * (Ab - 1) // 2)
    arm = lambda t: t[1] if t[0] == "a" else Aa + t[1]
    assert [tuple(int(v) for v in row) for row in tab] == [tuple(arm(t) for t in row) for row in cross + in_a + in_b]
    if Aa >= 3:                       # the oddity itself: labels of arm 2, probabilities of arm 1, for the pair (1, 2)
        assert (1, 1, 2, 0) in tab and (0, 0, 2, 1) in tab
    if Aa == Ab:                      # one model encoded once: run b's arms are run a's
        same, _ = pair_table(Aa, Aa, 0)
        assert same == [tuple(v - Aa if v >= Aa else v for v in row) for row in tab]


# ---- 4. declared, exported, ABI unchanged ---------------------------------------------------------------------------------
def test_entry_points_declared_exported_and_abi_unchanged():
    hdr = open(os.path.join(ROOT, "include", "mmvae.h")).read()
    for fn in NEW:
        assert re.search(r"\bint " + fn + r"\(", hdr), fn
    src = open(os.path.join(ROOT, "distributed-vae_amd", "csrc", "api.hip")).read()
    assert "int mmvae_abi_version(void) { return 5; }" in src
    lib = N.lib()
    assert lib.mmvae_abi_version() == 5 == N.ABI_VERSION
    for fn in NEW:
        assert hasattr(lib, fn), fn


# ---- 5. refusals on the host ------------------------------------------------------------------------------------------------
PTR = 0x1000     # fake device pointers: every case must be refused (or succeed as a no-op) before anything dereferences them


def _pairs(rows):
    return np.ascontiguousarray(np.asarray(rows, dtype=np.int32).reshape(-1, 4))


def _stats(labels=PTR, probs=PTR, T=4, n=10, Cc=7, pairs=((0, 0, 2, 2),), n_pairs=None, counts=PTR, acc=PTR):
    tab = None if pairs is None else _pairs(pairs)
    tp = None if tab is None else tab.ctypes.data_as(C.c_void_p)
    return N.lib().mmvae_pair_stats(labels, probs, T, n, Cc, tp, (1 if tab is None else len(tab)) if n_pairs is None else n_pairs, counts, acc,
                                    None)


@pytest.mark.parametrize("case,rc", [
    ("null_labels", -1), ("null_probs", -1), ("null_pairs", -1), ("null_counts", -1), ("null_acc", -1), ("C0", -1),
    ("C_neg", -1), ("C129", -1), ("n_neg", -1), ("n_pairs_neg", -1), ("T0", -1), ("idx_lab1_T", -1), ("idx_prob1_neg", -1),
    ("idx_lab2_T", -1), ("idx_prob2_T", -1), ("idx_second_row", -1), ("n0", 0), ("n_pairs0", 0)])
def test_pair_stats_rejects_bad_arguments(case, rc):
    kw = {}
    if case.startswith("null_"): kw[case[5:]] = None
    elif case == "C0": kw["Cc"] = 0
    elif case == "C_neg": kw["Cc"] = -3
    elif case == "C129": kw["Cc"] = 129
    elif case == "n_neg": kw["n"] = -1
    elif case == "n_pairs_neg": kw["n_pairs"] = -1
    elif case == "T0": kw["T"] = 0
    elif case == "idx_lab1_T": kw["pairs"] = ((4, 0, 2, 2),)
    elif case == "idx_prob1_neg": kw["pairs"] = ((0, -1, 2, 2),)
    elif case == "idx_lab2_T": kw["pairs"] = ((0, 0, 4, 2),)
    elif case == "idx_prob2_T": kw["pairs"] = ((0, 0, 2, 7),)
    elif case == "idx_second_row": kw["pairs"] = ((0, 0, 2, 2), (1, 1, 3, 4))
    elif case == "n0": kw["n"] = 0
    elif case == "n_pairs0": kw["n_pairs"] = 0
    assert _stats(**kw) == rc, N.lib().mmvae_last_error_string()
    if rc:
        assert N.lib().mmvae_last_error_string()


def _finish(counts=PTR, acc=PTR, n_pairs=3, Cc=7, cm_norm=PTR, emp=PTR, dist_norm=PTR, diag_mean=PTR, diag_min=PTR):
    return N.lib().mmvae_pair_stats_finish(counts, acc, n_pairs, Cc, cm_norm, emp, dist_norm, diag_mean, diag_min, None)


@pytest.mark.parametrize("case,rc", [
    ("null_counts", -1), ("null_acc", -1), ("null_cm_norm", -1), ("null_emp", -1), ("null_dist_norm", -1),
    ("null_diag_mean", -1), ("null_diag_min", -1), ("C0", -1), ("C129", -1), ("n_pairs_neg", -1), ("n_pairs0", 0)])
def test_pair_stats_finish_rejects_bad_arguments(case, rc):
    kw = {}
    if case.startswith("null_"): kw[case[5:]] = None
    elif case == "C0": kw["Cc"] = 0
    elif case == "C129": kw["Cc"] = 129
    elif case == "n_pairs_neg": kw["n_pairs"] = -1
    elif case == "n_pairs0": kw["n_pairs"] = 0
    assert _finish(**kw) == rc, N.lib().mmvae_last_error_string()


def test_python_wrappers_have_no_cpu_fallback():
    import torch
    lab, pr = torch.zeros(2, 3, dtype=torch.int32), torch.zeros(2, 3, 4)
    with pytest.raises(N.NativeError):
        N.pair_stats(lab, pr, [(0, 0, 1, 1)], 4)
    with pytest.raises(N.NativeError):
        N.pair_stats_finish(torch.zeros(1, 4, 4, dtype=torch.int64), torch.zeros(1, 4, 4, 2, dtype=torch.int64))

"""GPU: the cross-run evaluation on the device.  mmvae_pair_stats / mmvae_pair_stats_finish against the numpy restatement
(tests/evals_restatement.py) on identical inputs, on both kernel paths; ``evals2``, ``generate`` and
``consensus_statistics`` end to end against the reference's recorded results (tests/golden/evals2_a3.npz).

Bounds.  Counts, cm_norm, diag_mean and diag_min are integer work followed by fp64 operations in numpy's order: bit-equal.
A distance sum of k terms: every term is truncated to a multiple of 2^-52 (at most 2^-52 lost each: k 2^-52), and the
restatement adds the same k non-negative doubles in cell order while the device's integer sum is exact (two orders of k
non-negative doubles differ by at most 2 k 2^-53 |sum|): |emp - ref| <= k 2^-52 + 2 k 2^-53 |ref|, and that over smp[j] for
dist_norm.  Against the fixture (fp64 reference, fp32 engine) c is held to tests/test_gpu_encode.py's REF_TOL, the labels are
equal (the fixture's top-2 margin is above 1e-3), so a distance term moves by at most 2 tol_c."""
import os
import sys

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader, TensorDataset

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import evals_restatement as ER  # noqa: E402
from gpu_util import DEV  # noqa: E402
from test_gpu_encode import REF_TOL  # noqa: E402
from distributed_vae_amd import _native as N  # noqa: E402
from distributed_vae_amd._evals import consensus_statistics, evals2, pair_table, statistics_from_evals  # noqa: E402
from distributed_vae_amd.model import generate  # noqa: E402
from distributed_vae_amd.nn_model import mixVAE_model  # noqa: E402

pytestmark = pytest.mark.gpu

# launch_pair_stats (csrc/consensus.hip): the per-workgroup LDS histogram takes 12 bytes per matrix cell and runs while
# C * C * 12 <= 160 KiB, i.e. up to C = 116 (161 472 B); from C = 117 the wave-combined global atomics run
LDS_MAX_C = 116
SHAPES = [(2, 2, 4, 50), (2, 2, 7, 1), (2, 3, 33, 1000), (3, 3, 92, 777), (2, 2, 92, 5000), (5, 5, 128, 5000),
          (2, 2, LDS_MAX_C, 2100), (2, 2, LDS_MAX_C + 1, 2100)]
LABELS = ["agree60", "identical", "out_of_range"]
PROBS = ["near_onehot", "uniform01"]


def _labels(kind, T, K, n, rng):
    base = rng.integers(0, K, n)
    if kind == "identical":                     # every cell of every pair on the diagonal: the worst contention
        lab = np.stack([base] * T)
    else:                                       # 60 % agreement, as tests/test_gpu_consensus.py
        lab = np.stack([np.where(rng.random(n) < 0.6, base, rng.integers(0, max(K - 2, 1), n)) for _ in range(T)])
    lab = lab.astype(np.int32)
    if kind == "out_of_range":
        lab[0, n // 2] = K
        if n > 1:
            lab[T - 1, 0] = -1
    return lab


def _probs(kind, T, K, n, rng):
    if kind == "uniform01":
        p = rng.random((T, n, K), dtype=np.float32)
        p[:, ::3, 0] = 0.0
        p[:, 1::3, K - 1] = 1.0
        return p
    z = torch.from_numpy(rng.standard_normal((T, n, K)).astype(np.float32))
    return torch.softmax(torch.softmax(z, -1) / 0.005, -1).numpy()     # near one-hot; zeros and denormals elsewhere


def _run(lab, pr, pairs, K, path="auto", counts=None, acc=None):
    return N.pair_stats(torch.from_numpy(lab).to(DEV), torch.from_numpy(pr).to(DEV), pairs, K, counts, acc, path=path)


def _check(fin, counts, ref, scale=1):
    k = ref["counts"].astype(np.float64) * scale
    want_emp = ref["emp"] * scale
    assert np.array_equal(counts.cpu().numpy(), ref["counts"] * scale)
    cm_norm = fin["cm_norm"].cpu().numpy()
    assert np.array_equal(cm_norm, ref["cm_norm"])
    assert np.array_equal(fin["diag_mean"].cpu().numpy(), ref["diag_mean"])
    assert np.array_equal(fin["diag_min"].cpu().numpy(), ref["diag_min"])
    bound = k * 2.0 ** -52 + 2 * k * 2.0 ** -53 * np.abs(want_emp)
    err = np.abs(fin["emp"].cpu().numpy() - want_emp)
    print(f"emp: worst err / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}, largest sum {want_emp.max():.3e}")
    assert (err <= bound).all()
    smp = ref["smp"][:, None, :] * scale
    errn = np.abs(fin["dist_norm"].cpu().numpy() - ref["dist_norm"])
    assert (errn <= np.where(smp != 0, bound / np.where(smp != 0, smp, 1.0), 0.0)).all()


@pytest.mark.parametrize("probs", PROBS)
@pytest.mark.parametrize("labels", LABELS)
@pytest.mark.parametrize("Aa,Ab,K,n", SHAPES)
def test_pair_stats_against_restatement(Aa, Ab, K, n, labels, probs):
    rng = np.random.default_rng(Aa * 100000 + Ab * 10000 + K * 10 + len(labels))
    T = Aa + Ab
    lab, pr = _labels(labels, T, K, n, rng), _probs(probs, T, K, n, rng)
    pairs, sizes = pair_table(Aa, Ab)
    assert len(pairs) == sum(sizes) == Aa * Ab + Aa * (Aa - 1) // 2 + Ab * (Ab - 1) // 2
    ref = ER.pair_stats(lab, pr, pairs, K)
    assert ref["counts"].sum() > 0 or n == 1
    counts, acc = _run(lab, pr, pairs, K)
    _check(N.pair_stats_finish(counts, acc), counts, ref)
    # a second call adds: counts and the fixed-point sums double exactly
    c1, a1 = counts.clone(), acc.clone()
    _run(lab, pr, pairs, K, counts=counts, acc=acc)
    assert torch.equal(counts, 2 * c1) and torch.equal(acc, 2 * a1)
    _check(N.pair_stats_finish(counts, acc), counts, ref, scale=2)
    # a second run from zero: identical bits
    c2, a2 = _run(lab, pr, pairs, K)
    assert torch.equal(c2, c1) and torch.equal(a2, a1)
    # the other kernel path adds up the same integers
    other = "wave" if K <= LDS_MAX_C else None
    if other:
        c3, a3 = _run(lab, pr, pairs, K, path=other)
        assert torch.equal(c3, c1)
        f1, f3 = N.pair_stats_finish(c1, a1), N.pair_stats_finish(c3, a3)
        assert torch.equal(f1["emp"], f3["emp"]) and torch.equal(f1["dist_norm"], f3["dist_norm"])
        c4, a4 = _run(lab, pr, pairs, K, path="lds")
        assert torch.equal(c4, c1) and torch.equal(a4, a1)
    else:
        with pytest.raises(NotImplementedError):
            _run(lab, pr, pairs, K, path="lds")
    # n = 0 leaves the accumulators untouched
    _run(lab[:, :0], pr[:, :0], pairs, K, counts=c2, acc=a2)
    assert torch.equal(c2, c1) and torch.equal(a2, a1)
    tab = np.ascontiguousarray(np.asarray(pairs, np.int32))                  # the C entry point itself at n = 0
    rc = N.lib().mmvae_pair_stats(c1.data_ptr(), c1.data_ptr(), T, 0, K, tab.ctypes.data, len(tab), c2.data_ptr(), a2.data_ptr(),
                                  None)
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(c2, c1) and torch.equal(a2, a1)


@pytest.mark.parametrize("path", ["lds", "wave"])
def test_pair_stats_table_longer_than_one_launch(path):
    """A launch carries 128 pairs (PS_MAX_PAIRS): a table of 135, the 45 pairs of A = 5 three times over, takes two, and the
    second writes from pair 128 on.  Every repeat must equal the first."""
    K, n = 9, 700
    rng = np.random.default_rng(11)
    lab, pr = _labels("agree60", 10, K, n, rng), _probs("uniform01", 10, K, n, rng)
    pairs, _ = pair_table(5, 5)
    counts, acc = _run(lab, pr, pairs * 3, K, path=path)
    assert counts.shape[0] == 135
    c1, a1 = _run(lab, pr, pairs, K, path=path)
    for r in range(3):
        assert torch.equal(counts[45 * r:45 * (r + 1)], c1) and torch.equal(acc[45 * r:45 * (r + 1)], a1), r
    ref = ER.pair_stats(lab, pr, pairs, K)
    ref3 = {k: np.concatenate([v] * 3) for k, v in ref.items()}
    _check(N.pair_stats_finish(counts, acc), counts, ref3)


def test_pair_stats_outside_the_window_reads_back_nan():
    """A term outside [0, 2) is no difference of probabilities: its matrix cell reads back NaN, the others are untouched."""
    K, n = 5, 300
    rng = np.random.default_rng(3)
    lab, pr = _labels("agree60", 2, K, n, rng), _probs("uniform01", 2, K, n, rng)
    pairs = [(0, 0, 1, 1)]
    ref = ER.pair_stats(lab, pr, pairs, K)
    i = 7
    i1, i2 = int(lab[0, i]), int(lab[1, i])
    pr[0, i, i1] = 3.5
    for path in ("lds", "wave"):
        counts, acc = _run(lab, pr, pairs, K, path=path)
        fin = N.pair_stats_finish(counts, acc)
        emp = fin["emp"].cpu().numpy()
        assert np.isnan(emp[0, i1, i2]) and np.isnan(fin["dist_norm"].cpu().numpy()[0, i1, i2])
        mask = np.ones((K, K), bool)
        mask[i1, i2] = False
        assert np.allclose(emp[0][mask], ref["emp"][0][mask], rtol=1e-12, atol=1e-12)
        assert np.array_equal(counts.cpu().numpy(), ref["counts"])


# ---- end to end against the reference fixture ------------------------------------------------------------------------------
G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "evals2_a3.npz"))
A, NC, D, H, L, K_, S, BATCH, PRUNED = [int(v) for v in G["cfg"]]
TOL_C = REF_TOL["fp32_mfma"]                      # the models below run the default engine
BIT_EQUAL = ["pm", "pm_a", "pm_b", "consensus", "consensus_a", "consensus_b", "consensus_min", "consensus_min_a",
             "consensus_min_b", "consensus_vec", "consensus_mean_a", "consensus_mean_b", "inds_unpruned", "emp_log"]
EMPTY = ["dist_log", "dist_log_a", "dist_log_b", "emp_log_a"]


def _sd(tag):
    sd = {k[5:]: torch.from_numpy(np.asarray(G[k])) for k in G.files if k.startswith(f"sd_{tag}/")}
    return {k: (v.float() if v.is_floating_point() else v) for k, v in sd.items()}


def _model(tag):
    m = mixVAE_model(input_dim=D, fc_dim=H, n_categories=K_, state_dim=S, lowD_dim=L, x_drop=0.5, s_drop=0.2, n_arm=A, lam=1,
                     lam_pc=1, tau=0.005, beta=1.0, hard=False, variational=True, device=DEV, eps=1e-8, momentum=0.01,
                     ref_prior=False, loss_mode="MSE")
    m.load_state_dict(_sd(tag))
    return m.to(DEV).eval()


def _loader():
    x = torch.from_numpy(G["x"]).float()
    return DataLoader(TensorDataset(x, torch.arange(NC, dtype=torch.float32)), batch_size=BATCH, shuffle=False)   # 64, 64, 22


@pytest.fixture(scope="module")
def runs():
    fa, fb = _model("a"), _model("b")
    dl = _loader()
    assert [len(b[0]) for b in dl] == [64, 64, 22]
    return {"fa": fa, "fb": fb, "dl": dl, "ab": evals2(fa, fb, dl), "aa": evals2(fa, fa, dl), "bb": evals2(fb, fb, dl)}


def _stack(v):
    return np.asarray(v, dtype=np.float64) if not isinstance(v, np.ndarray) else v


@pytest.mark.parametrize("case", ["ab", "aa"])
def test_evals2_against_reference_fixture(runs, case):
    ev = runs[case]
    want_keys = [k[3:] for k in G.files if k.startswith(f"{case}/")]
    assert list(ev) == want_keys                                           # key for key, in the reference's order
    for k in want_keys:
        assert _stack(ev[k]).shape == G[f"{case}/{k}"].shape, k
    for k in BIT_EQUAL:
        assert _stack(ev[k]).dtype == G[f"{case}/{k}"].dtype and np.array_equal(_stack(ev[k]), G[f"{case}/{k}"]), k
    for k in EMPTY:
        assert ev[k] == []
    for k in ("cs_a", "cs_b"):
        ref = G[f"{case}/{k}"]
        rel = float(np.abs(ev[k] - ref).max() / np.abs(ref).max())
        print(f"{case} {k}: {rel:.3e} (tolerance {TOL_C:.0e})")
        assert ev[k].dtype == np.float64 and rel < TOL_C
    tol_abs = TOL_C * max(float(np.abs(G[f"{case}/cs_a"]).max()), float(np.abs(G[f"{case}/cs_b"]).max()))
    for sfx, pm in (("", G[f"{case}/pm"][0::2]), ("_a", G[f"{case}/pm_a"]), ("_b", G[f"{case}/pm_b"])):
        bound = 2 * pm * tol_abs
        err = np.abs(_stack(ev["emp_l2" + sfx]) - G[f"{case}/emp_l2{sfx}"])
        assert (err <= bound).all(), (sfx, float(err.max()))
        smp = np.maximum(pm.sum(axis=1), pm.sum(axis=2))[:, None, :]
        errd = np.abs(_stack(ev["dist_l2" + sfx]) - G[f"{case}/dist_l2{sfx}"])
        assert (errd <= np.where(smp != 0, bound / np.where(smp != 0, smp, 1.0), 0.0)).all(), sfx
    got, want = np.array(ev["consensus_mean"]), G[f"{case}/consensus_mean"]
    assert (np.abs(got - want) <= K_ * 2.0 ** -52 * np.abs(want)).all()
    assert all(isinstance(v, np.float64) for v in ev["consensus_min"] + ev["consensus_mean"] + ev["consensus_vec"])
    assert runs["fa"].training is False


def test_evals2_restores_training_mode_and_refuses_mismatched_runs(runs):
    fa = runs["fa"]
    fa.train()
    try:
        evals2(fa, runs["fb"], runs["dl"])
        assert fa.training and not runs["fb"].training
    finally:
        fa.eval()
    other = mixVAE_model(input_dim=D, fc_dim=H, n_categories=K_ + 1, state_dim=S, lowD_dim=L, x_drop=0.5, s_drop=0.2, n_arm=2,
                         lam=1, lam_pc=1, tau=0.005, beta=1.0, hard=False, variational=True, device=DEV, eps=1e-8,
                         momentum=0.01, ref_prior=False, loss_mode="MSE").to(DEV).eval()
    with pytest.raises(ValueError):
        evals2(fa, other, runs["dl"])


def test_evals2_with_different_arm_counts(runs):
    """Aa = 3 against Ab = 2: the first two arms of run b as a model of its own."""
    sd = {k: v for k, v in _sd("b").items() if int(k.split(".")[1]) < 2}
    fb2 = mixVAE_model(input_dim=D, fc_dim=H, n_categories=K_, state_dim=S, lowD_dim=L, x_drop=0.5, s_drop=0.2, n_arm=2, lam=1,
                       lam_pc=1, tau=0.005, beta=1.0, hard=False, variational=True, device=DEV, eps=1e-8, momentum=0.01,
                       ref_prior=False, loss_mode="MSE")
    fb2.load_state_dict(sd)
    fb2 = fb2.to(DEV).eval()
    ev, full = evals2(runs["fa"], fb2, runs["dl"]), runs["ab"]
    assert len(ev["consensus"]) == 6 and len(ev["pm"]) == 12 and len(ev["consensus_a"]) == 3 and len(ev["consensus_b"]) == 1
    for a in range(A):
        for b in range(2):
            assert np.array_equal(ev["consensus"][a * 2 + b], full["consensus"][a * A + b])
            assert np.array_equal(ev["emp_l2"][a * 2 + b], full["emp_l2"][a * A + b])
    assert np.array_equal(ev["emp_l2_b"][0], full["emp_l2_b"][0]) and np.array_equal(ev["cs_b"], full["cs_b"][:2])


def test_generate_latent_only_equals_encode_dataset_and_full_key_set(runs):
    from distributed_vae_amd.cpl_mixvae import cpl_mixVAE
    t = cpl_mixVAE(saving_folder="", device=0, save_flag=False)
    t.init_model(n_categories=K_, state_dim=S, input_dim=D, fc_dim=H, lowD_dim=L, x_drop=0.5, s_drop=0.2, n_arm=A, temp=1.0,
                 tau=0.005)
    t.model.load_state_dict(_sd("a"))
    dl = runs["dl"]
    want = t.encode_dataset(dl)
    t.model.train()
    got = generate(t.model, dl, latent_only=True)
    assert t.model.training                                                   # restored
    names = {"s_means": "state_mu", "s_logvars": "state_var", "cs": "z_prob", "c_smps": "z_sample", "x_lows": "x_low",
             "inds_x": "data_indx", "preds": "predicted_label", "inds_prune": "prune_indx"}
    assert list(got) == ["s_means", "s_logvars", "cs", "c_smps", "x_lows", "inds_x", "inds_prune", "pruning_mask", "preds"]
    for k, kk in names.items():
        assert got[k].dtype == want[kk].dtype and np.array_equal(got[k], want[kk]), k
    assert got["pruning_mask"].tolist() == [k for k in range(K_) if k != PRUNED] and got["inds_prune"].tolist() == [PRUNED]
    assert np.array_equal(got["preds"], G["gen_a/preds"])
    full = generate(t.model.eval(), dl)
    shapes = {"x_recs": (A, NC, D), "s_means": (A, NC, S), "s_logvars": (A, NC, S), "cs": (A, NC, K_), "c_smps": (A, NC, K_),
              "x_lows": (A, NC, L), "inds_x": (NC,), "losses": None, "c_dists": (), "c_l2_dists": (), "loss_recs": (A,),
              "lls": (A,), "inds_prune": (1,), "pruning_mask": (K_ - 1,), "preds": (A, NC)}
    assert list(full) == list(shapes)                                       # mmidas/model.py:133-149
    for k, shp in shapes.items():
        if shp is None:
            assert isinstance(full[k], list) and len(full[k]) == 3 and all(isinstance(v, float) for v in full[k])
        else:
            assert np.asarray(full[k]).shape == shp and np.asarray(full[k]).dtype in (np.float64, np.int64), k
    for k in ("s_means", "s_logvars", "cs", "x_lows", "inds_x", "preds"):    # the same kernels as the latent-only form
        assert np.array_equal(full[k], got[k]), k
    assert np.isfinite(full["x_recs"]).all() and np.isfinite(full["losses"]).all() and full["x_recs"].any()


def _same_tree(a, b, path=""):
    if isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b), path
        for k in a:
            _same_tree(a[k], b[k], f"{path}/{k}")
    else:
        x, y = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
        assert x.shape == y.shape and np.array_equal(x, y, equal_nan=True), path


def test_consensus_statistics_equals_restatement_on_the_device_outputs(runs):
    got = consensus_statistics({0: runs["fa"], 1: runs["fb"]}, runs["dl"], A)
    cross, within = {(0, 1): runs["ab"]}, {0: runs["aa"], 1: runs["bb"]}
    want = ER.consensus_statistics(cross, within, A)
    _same_tree(got, want)
    _same_tree(statistics_from_evals(cross, within, A), want)
    assert list(got["consensus"]["xs"]) == [(0, 1), (0, 0), (1, 1)] and got["consensus"]["xs"][(0, 1)].shape == (A * A,)
    assert got["consensus"]["xs"][(0, 0)].shape == (A * (A - 1) // 2,)
    assert np.isnan(got["total"]["within_run"]["log/mean"]) and got["log"]["xs"][(0, 1)] == []
    assert np.isfinite(got["total"]["between_run"]["l2/mean"])

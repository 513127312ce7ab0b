"""CPU: the host side of the Gaussian classifiers (QDA_classifier, LDA_classifier, gaussian_cv_predict).  The numpy fp64
restatement (tests/gaussclf_restatement.py) against the reference's recorded returns and sklearn's recorded
``decision_function`` (tests/golden/gaussclf_kat.npz; tools/gen_golden_gaussclf.py); the host path of the package (folds,
models from moments) against the restatement, with the device's moments emulated in numpy; the preconditions the GPU tests
lean on; the host-side contract of mmvae_group_moments and mmvae_gauss_scores: declared, exported, ABI version unchanged, the
workspace sizes, every bad argument refused before any device work; the public functions' refusals.

Bounds.  Predictions, folds and accuracies are compared exactly.  Scores: the restatement against sklearn's recorded ones at
the case's e_ref (the same computation recorded it) plus the restatement's own summation bound for another BLAS
(``tolerance_sum``); the package's host path against the restatement at ``tolerance_cv``, the derived bound of the whole
path.  Near-ties: a GPU test may excuse a cell whose restated margin is within twice its gate, at most 1 % of the cells;
here every input is shown to excuse none."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gaussclf_inputs as GI  # noqa: E402
import gaussclf_restatement as GR  # noqa: E402
import distributed_vae_amd  # noqa: F401,E402
from distributed_vae_amd import _native as N  # noqa: E402
from distributed_vae_amd.utils import cluster_analysis as CA  # noqa: E402

G = np.load(os.path.join(ROOT, "tests", "golden", "gaussclf_kat.npz"))
CASES = [tuple(int(v) for v in row) for row in G["cases"]]
SETS = [(k, clf, str(key)) for k in range(len(CASES)) for clf in ("qda", "lda") for key in G[f"c{k}/keys"]]


# ---- 1. the fixture is what the generator promises -----------------------------------------------------------------------
def test_fixture_is_what_the_generator_promises():
    assert CASES == [(600, 2, 5, 0), (800, 10, 4, 3), (700, 12, 3, 11), (900, 10, 10, 1), (3000, 2, 10, 7), (1000, 12, 5, 2)]
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "gaussclf_kat.npz")) < 1024 * 1024
    assert all(G[k].dtype != object for k in G.files) and str(G["source"])
    assert np.allclose(G["c1/x"].astype(np.float64).sum(axis=1), 1.0, atol=1e-6) and (G["c1/x"] >= 0).all()      # the simplex
    assert G["c2/y/T"].dtype.kind == "U" and [str(v) for v in G["c3/keys"]] == ["T", "merged"]
    assert len(np.unique(G["c4/y/T"])) == 40
    for k, clf, key in SETS:
        n, d, kfold, _ = CASES[k]
        base = f"c{k}/{clf}/{key}"
        assert G[f"c{k}/x"].dtype == np.float32 and G[f"c{k}/x"].shape == (n, d)
        assert G[f"{base}/acc"].shape == (kfold,) and int(G[f"{base}/sizes"].sum()) == n
        assert G[f"{base}/pred"].shape == G[f"{base}/ref"].shape == (n,)
        assert G[f"{base}/dec"].shape == (len(G[f"{base}/rows"]), len(np.unique(G[f"c{k}/y/{key}"])))
        assert 0 <= float(G[f"{base}/e_ref"]) <= 1e-8 and float(G[f"{base}/min_margin"]) >= 1e-6


# ---- 2. the restatement is the reference's arithmetic -----------------------------------------------------------------------
@pytest.mark.parametrize("k", range(6))
def test_fold_split_is_sklearns(k):
    n, _, kfold, seed = CASES[k]
    fold = GR.fold_split(n, kfold, seed)
    assert np.array_equal(fold, CA.kfold_of(n, kfold, seed))
    key = str(G[f"c{k}/keys"][0])
    y, sizes = G[f"c{k}/y/{key}"], G[f"c{k}/qda/{key}/sizes"]
    assert np.array_equal(np.bincount(fold, minlength=kfold), sizes)
    assert sizes.max() - sizes.min() <= 1 and (np.diff(sizes) <= 0).all()                       # the first n % k one longer
    ref = np.split(G[f"c{k}/qda/{key}/ref"], np.cumsum(sizes)[:-1])
    for f in range(kfold):
        assert np.array_equal(y[fold == f], ref[f])                                             # ascending order of the index


@pytest.mark.parametrize("k,clf,key", SETS, ids=[f"c{k}-{clf}-{key}" for k, clf, key in SETS])
def test_restatement_equals_recorded_reference(k, clf, key):
    n, d, kfold, seed = CASES[k]
    x, y = G[f"c{k}/x"], G[f"c{k}/y/{key}"]
    base = f"c{k}/{clf}/{key}"
    acc, ref, pred = GR.classifier(x, {key: y}, kfold, seed, clf)
    assert list(acc) == [key] and len(acc[key]) == len(ref[key]) == len(pred[key]) == kfold
    assert np.array_equal(np.concatenate(pred[key]), G[f"{base}/pred"])                       # every cell, none left out
    assert np.array_equal(np.concatenate(ref[key]), G[f"{base}/ref"])
    assert np.array_equal(np.array(acc[key]), G[f"{base}/acc"]) and all(type(a) is float for a in acc[key])
    res = GR.cv_predict(x, y, kfold, seed, clf)
    rows = G[f"{base}/rows"]
    mine, theirs = res["scores"][rows], G[f"{base}/dec"]
    if clf == "lda":
        mine, theirs = mine - mine.max(axis=1, keepdims=True), theirs - theirs.max(axis=1, keepdims=True)
    own = GR.tolerance_sum(d, res["A"][rows], res["c0"][res["fold"][rows]])
    own = own + own.max(axis=1, keepdims=True) if clf == "lda" else own
    err = np.abs(mine - theirs)
    print(f"{base}: worst |restatement - sklearn| {err.max():.2e}, e_ref {float(G[f'{base}/e_ref']):.2e}")
    assert (err <= float(G[f"{base}/e_ref"]) + own).all()
    assert float((res["best"] - res["second"]).min()) == pytest.approx(float(G[f"{base}/min_margin"]), rel=1e-6)


# ---- 3. the package's host path, the device's moments emulated ---------------------------------------------------------------
def _host_path(x, y, kfold, seed, kind):
    """``_cv_on_device`` with numpy in the kernels' place: (scores [n, K] in the caller's order, classes, fold, pivot)."""
    n, d = x.shape
    classes, codes, fold = CA._cv_refusals(y, n, kfold, seed, kind)
    K = len(classes)
    group = codes * kfold + fold
    order = np.argsort(group, kind="stable")
    counts = np.bincount(group, minlength=K * kfold)
    offsets = np.concatenate([[0], np.cumsum(counts)])
    pivot = x.mean(axis=0, dtype=np.float32)
    s, M = GI.emulate_moments(x[order], offsets, pivot)
    mu, W, c0 = CA.models_from_moments(s.reshape(K, kfold, d), M.reshape(K, kfold, -1), counts.reshape(K, kfold).astype(np.float64),
                                       pivot, kind)
    sc = np.zeros((n, K))
    for f in range(kfold):
        rows = np.flatnonzero(fold == f)
        sc[rows] = GR.scores(x[rows], mu[f], W[f], c0[f])[0]
    return sc, classes, fold, pivot


@pytest.mark.parametrize("k,clf,key", SETS, ids=[f"c{k}-{clf}-{key}" for k, clf, key in SETS])
def test_models_from_moments_equal_the_restatement(k, clf, key):
    n, d, kfold, seed = CASES[k]
    x, y = G[f"c{k}/x"], G[f"c{k}/y/{key}"]
    sc, classes, fold, pivot = _host_path(x, y, kfold, seed, clf)
    res = GR.cv_predict(x, y, kfold, seed, clf)
    assert np.array_equal(classes, res["classes"]) and np.array_equal(fold, res["fold"])
    gate = GR.tolerance_cv(res, pivot.astype(np.float64), clf)
    err = np.abs(sc - res["scores"])
    print(f"c{k} {clf} {key}: worst |moments path - restatement| {err.max():.2e}, gate {gate.min():.2e} .. {gate.max():.2e}, "
          f"worst ratio {float((err / gate).max()):.2e}")
    assert (err <= gate).all()
    assert np.array_equal(np.argmax(sc, axis=1), res["pred"])
    # the precondition of the GPU test: no cell's margin within twice the gate
    assert not ((res["best"] - res["second"]) <= 2.0 * gate.max(axis=1)).any()


@pytest.mark.parametrize("K,F,d,n", [(4, 3, 3, 60), (5, 1, 4, 90), (6, 5, 17, 400)])
def test_fold_sums_are_formed_once_for_both_model_builders(K, F, d, n):
    """The one fold sum: ``fold_training_moments`` against the sum written out here (the groups g != f in increasing g from
    zeros; F = 1: the one group), and the two model builders that read it against each other.  Exact: no tolerance."""
    from distributed_vae_amd.utils import analysis_tree_helpers as TH
    rng = np.random.default_rng(3)
    codes = rng.integers(0, K - 1, size=n)                                     # the last class has no cell at all
    fold = rng.integers(0, F, size=n)
    x = rng.normal(size=(n, d)).astype(np.float32).astype(np.float64) + codes[:, None]     # float32-representable points
    pivot = x.mean(axis=0)
    iu = np.triu_indices(d)
    s, M, counts = np.zeros((K, F, d)), np.zeros((K, F, len(iu[0]))), np.zeros((K, F))
    for k in range(K):
        for f in range(F):
            t = x[(codes == k) & (fold == f)] - pivot
            s[k, f], M[k, f], counts[k, f] = t.sum(axis=0), (t.T @ t)[iu], len(t)
    assert not counts[K - 1].any() and counts.sum() == n
    folds = list(CA.fold_training_moments(s, M, counts))
    assert len(folds) == F
    for f, (cnt, offset, scatter) in enumerate(folds):
        c_tr, s_tr, M_tr = np.zeros(K), np.zeros((K, d)), np.zeros((K, len(iu[0])))
        for g in range(F):
            if g != f or F == 1:
                c_tr, s_tr, M_tr = c_tr + counts[:, g], s_tr + s[:, g], M_tr + M[:, g]
        full = np.zeros((K, d, d))
        full[:, iu[0], iu[1]] = M_tr
        full[:, iu[1], iu[0]] = M_tr
        Nk = np.maximum(c_tr, 1.0)
        assert np.array_equal(cnt, c_tr) and np.array_equal(offset, s_tr / Nk[:, None])
        assert np.array_equal(scatter, full - s_tr[:, :, None] * s_tr[:, None, :] / Nk[:, None, None])
    if F > 1:
        with np.errstate(all="ignore"):
            mu_leaf, _, c0_leaf, _ = TH.models_from_leaf_moments(s, M, counts, pivot, np.zeros(K), 6, 12, 1e-4)
            has_model = np.isfinite(c0_leaf)
            assert has_model.any() and not has_model[:, K - 1].any()
            for kind in ("qda", "lda"):
                mu = CA.models_from_moments(s, M, counts, pivot, kind)[0]
                assert np.array_equal(mu[has_model], mu_leaf[has_model])


# ---- 4. the preconditions the GPU tests lean on -----------------------------------------------------------------------------
def test_constants_of_the_inputs_are_those_of_the_source():
    assert (GI.ROW_TILE, GI.SEG) == (N.GAUSSCLF_ROW_TILE, N.GAUSSCLF_SEG_ROWS)


@pytest.mark.parametrize("name", sorted(GI.SCORE_CASES))
def test_score_inputs_excuse_no_cell(name):
    case = GI.score_input(name)
    n = len(case["pred"])
    excused = int((~GI.decided(case)).sum())
    print(f"{name}: {n} cells, smallest margin {float((case['best'] - case['second']).min()):.2e}, largest gate "
          f"{float(case['gate'].max()):.2e}, excused {excused}")
    assert excused == 0 <= 0.01 * n
    assert np.isfinite(case["best"]).all()
    if name == "absent":
        assert (case["scores"][case["model"] == 0, 1] == -np.inf).all() and (case["pred"][case["model"] == 0] != 1).all()
    if name == "lone_fold":
        assert int((case["model"] == 1).sum()) == 1


@pytest.mark.parametrize("name", sorted(GI.MOMENT_CASES))
def test_moment_bound_holds_for_the_emulated_sums(name):
    """The derived bound against numpy's own sums about the pivot (another summation order than the device's), near and far."""
    d = GI.MOMENT_CASES[name][1]
    for far in (False, True):
        m = GI.moment_input(name, far)
        x, off, pivot = m["x"], m["offsets"], m["pivot"].astype(np.float64)
        s, M = GI.emulate_moments(x, off, m["pivot"])
        full = GI.unpack(M, d)
        for g, (cnt, mean, scat) in enumerate(m["stats"]):
            if cnt == 0:
                assert not s[g].any() and not M[g].any()
                continue
            xg = x[off[g]:off[g + 1]].astype(np.float64)
            raw2 = ((xg - pivot) ** 2).mean(axis=0)
            tol_mean, tol_scat = GR.tolerance_moments(cnt, raw2, pivot, np.abs(xg).max(axis=0))
            assert (np.abs(pivot + s[g] / cnt - mean) <= tol_mean).all()
            assert (np.abs(full[g] - np.outer(s[g], s[g]) / cnt - scat) <= tol_scat).all()


# ---- 5. the C boundary ------------------------------------------------------------------------------------------------------
def test_entry_points_declared_exported_and_abi_unchanged():
    hdr = open(os.path.join(ROOT, "include", "mmvae.h")).read()
    for name in ("int mmvae_group_moments", "int mmvae_debug_group_moments", "size_t mmvae_group_moments_workspace_bytes",
                 "int mmvae_gauss_scores", "size_t mmvae_gauss_scores_workspace_bytes"):
        assert re.search(r"\b" + re.escape(name) + r"\(", hdr), name
        assert hasattr(N.lib(), name.split()[1])
    for word in ("kappa", "bit-identical", "CALLER'S", "lowest index on ties", "4 (N + 2) kappa u"):
        assert word in hdr, word
    src = open(os.path.join(ROOT, "distributed-vae_amd", "csrc", "api.hip")).read()
    assert "int mmvae_abi_version(void) { return 5; }" in src and N.lib().mmvae_abi_version() == 5 == N.ABI_VERSION
    assert '"gaussclf.hip"' in open(os.path.join(ROOT, "distributed-vae_amd", "build.py")).read()


def test_launch_constants_are_those_of_the_source():
    hpp = open(os.path.join(ROOT, "distributed-vae_amd", "csrc", "common.hpp")).read()

    def const(name):
        return int(re.search(r"constexpr int " + name + r" = (\d+);", hpp).group(1))
    assert const("GC_SEG_ROWS") == N.GAUSSCLF_SEG_ROWS == 256 and const("GC_ROW_CHUNK") == N.GAUSSCLF_ROW_CHUNK == 32
    assert const("GC_ROW_TILE") == N.GAUSSCLF_ROW_TILE == 64 and const("GC_COL_BLOCK") == N.GAUSSCLF_COL_BLOCK == 8
    assert const("GC_SCORE_WAVES") == N.GAUSSCLF_SCORE_WAVES == 16
    assert (const("GC_MAX_D"), const("GC_MAX_K"), const("GC_MAX_F")) == (N.GAUSSCLF_MAX_D, N.GAUSSCLF_MAX_K, N.GAUSSCLF_MAX_F)
    dc = re.search(r"GC_DC\[GC_N_DC\] = \{([^}]*)\}", hpp).group(1)
    assert tuple(int(v) for v in dc.split(",")) == N.GAUSSCLF_DC and const("GC_N_DC") == len(N.GAUSSCLF_DC)
    assert [N.gaussclf_dclass(d) for d in (1, 16, 17, 32, 33, 64, 65, 128)] == ["d16", "d16", "d32", "d32", "d64", "d64", "d128", "d128"]
    assert [N.GAUSSCLF_PATHS[f"d{v}"] for v in N.GAUSSCLF_DC] == [0, 1, 2, 3]
    # 256 threads of NPT sums hold all d (d + 3) / 2 sums of the instance's largest d
    for v, npt in zip(N.GAUSSCLF_DC, (1, 3, 9, 33)):
        assert 256 * (npt - 1) < v * (v + 3) // 2 <= 256 * npt


def _ws_moments(n, d, G):
    m = G + n // 256
    return 8 * (m * (d * (d + 3) // 2) + m + 1) + 4 * ((G + 2) // 2 * 2)


def test_workspace_bytes():
    ws = N.lib().mmvae_group_moments_workspace_bytes
    for n, d, Gn in ((1, 1, 1), (65, 2, 3), (22365, 10, 920), (22365, 92, 920), (1 << 31, 128, 1 << 20)):
        assert ws(n, d, Gn) == _ws_moments(n, d, Gn), (n, d, Gn)
    assert ws(22365, 92, 920) < 36 * 2 ** 20                               # the data set at d = 92, 10 folds: 35 MB
    for n, d, Gn in ((0, 2, 1), (-1, 2, 1), ((1 << 31) + 1, 2, 1), (10, 0, 1), (10, 129, 1), (10, 2, 0), (10, 2, (1 << 20) + 1)):
        assert ws(n, d, Gn) == 0, (n, d, Gn)
    assert N.lib().mmvae_gauss_scores_workspace_bytes(22365, 92, 10, 92) == 0


PTR = 0x1000     # fake device pointers: every case must be refused before anything dereferences them


def _moments(x=PTR, ld=10, n=100, d=10, offsets=PTR, G=7, pivot=PTR, ws=PTR, ws_bytes=None, s=PTR, M=PTR, dclass=-1):
    if ws_bytes is None:
        ws_bytes = 1 << 40
    return N.lib().mmvae_debug_group_moments(x, ld, n, d, offsets, G, pivot, ws, ws_bytes, s, M, dclass, None)


@pytest.mark.parametrize("case,rc", [
    ("null_x", -1), ("null_offsets", -1), ("null_pivot", -1), ("null_ws", -1), ("null_s", -1), ("null_M", -1), ("n0", -1),
    ("n_past_2_31", -1), ("d0", -1), ("G0", -1), ("ld_below_d", -1), ("ws_misaligned", -1), ("dclass_4", -1), ("dclass_m2", -1),
    ("d129", -2), ("G_past", -2), ("ws_small", -4), ("class_below_d", -2)])
def test_group_moments_rejects_bad_arguments(case, rc):
    kw = {}
    if case.startswith("null_"): kw[case[5:]] = None
    elif case == "n0": kw["n"] = 0
    elif case == "n_past_2_31": kw["n"] = (1 << 31) + 1
    elif case == "d0": kw["d"] = 0
    elif case == "G0": kw["G"] = 0
    elif case == "ld_below_d": kw["ld"] = 9
    elif case == "ws_misaligned": kw["ws"] = PTR + 4
    elif case == "dclass_4": kw["dclass"] = 4
    elif case == "dclass_m2": kw["dclass"] = -2
    elif case == "d129": kw.update(d=129, ld=129)
    elif case == "G_past": kw["G"] = (1 << 20) + 1
    elif case == "ws_small": kw["ws_bytes"] = _ws_moments(100, 10, 7) - 1
    elif case == "class_below_d": kw.update(d=17, ld=17, dclass=0)
    assert _moments(**kw) == rc, N.lib().mmvae_last_error_string()
    assert N.lib().mmvae_last_error_string()


def _scores(x=PTR, ld=10, n=100, d=10, model=PTR, F=3, K=7, mu=PTR, W=PTR, c0=PTR, perm=PTR, ws=None, label=PTR, best=PTR,
            second=PTR, scores=PTR):
    return N.lib().mmvae_gauss_scores(x, ld, n, d, model, F, K, mu, W, c0, perm, ws, 0, label, best, second, scores, None)


@pytest.mark.parametrize("case,rc", [
    ("null_x", -1), ("null_model", -1), ("null_mu", -1), ("null_W", -1), ("null_c0", -1), ("null_label", -1), ("null_best", -1),
    ("null_second", -1), ("n0", -1), ("n_past_2_31", -1), ("d0", -1), ("F0", -1), ("K0", -1), ("ld_below_d", -1),
    ("ws_misaligned", -1), ("d129", -2), ("K4097", -2), ("F65", -2)])
def test_gauss_scores_rejects_bad_arguments(case, rc):
    kw = {}
    if case.startswith("null_"): kw[case[5:]] = None
    elif case == "n0": kw["n"] = 0
    elif case == "n_past_2_31": kw["n"] = (1 << 31) + 1
    elif case == "d0": kw["d"] = 0
    elif case == "F0": kw["F"] = 0
    elif case == "K0": kw["K"] = 0
    elif case == "ld_below_d": kw["ld"] = 9
    elif case == "ws_misaligned": kw["ws"] = PTR + 4
    elif case == "d129": kw.update(d=129, ld=129)
    elif case == "K4097": kw["K"] = 4097
    elif case == "F65": kw["F"] = 65
    assert _scores(**kw) == rc, N.lib().mmvae_last_error_string()
    assert N.lib().mmvae_last_error_string()


def test_python_wrappers_have_no_cpu_fallback():
    import torch
    x, off = torch.zeros(5, 2), torch.tensor([0, 2, 5])
    with pytest.raises(N.NativeError):
        N.group_moments(x, off, torch.zeros(2))
    with pytest.raises(N.NativeError):
        N.gauss_scores(x, torch.zeros(5, dtype=torch.int32), torch.zeros(1, 2, 2, dtype=torch.float64),
                       torch.zeros(1, 2, 2, 2, dtype=torch.float64), torch.zeros(1, 2, dtype=torch.float64))


# ---- 6. the public functions' refusals: all before any device work (this machine has no device) -----------------------------
def test_refusals():
    x, codes = GI.points(60, 3, 3)
    for fn in (CA.QDA_classifier, CA.LDA_classifier):
        with pytest.raises(ValueError, match="greater than one"):
            fn(x, {"a": np.zeros(60, dtype=np.int64)}, 3, 0)
        with pytest.raises(ValueError, match="kfold"):
            fn(x, {"a": codes}, 1, 0)
        with pytest.raises(ValueError, match="kfold"):
            fn(x, {"a": codes}, 61, 0)
        with pytest.raises(ValueError, match="labels for"):
            fn(x, {"a": codes, "b": codes[:-1]}, 3, 0)                      # the second key: still before any device work
        bad = x.copy()
        bad[7, 1] = np.nan
        with pytest.raises(ValueError, match="NaN or infinity"):
            fn(bad, {"a": codes}, 3, 0)
    with pytest.raises(ValueError, match="kind"):
        CA.gaussian_cv_predict(x, codes, 3, 0, kind="rf")
    with pytest.raises(ValueError, match="not \\[n, d\\]"):
        CA.gaussian_cv_predict(x[:, 0], codes, 3, 0)
    with pytest.raises(NotImplementedError):
        CA.gaussian_cv_predict(np.zeros((60, 129), dtype=np.float32), codes, 3, 0)
    with pytest.raises(NotImplementedError):
        CA.gaussian_cv_predict(np.tile(x, (2, 1)), np.tile(codes, 2), 65, 0)


def test_singleton_class_raises_sklearns_error():
    x, codes = GI.points(60, 3, 3)
    fold = CA.kfold_of(60, 3, 0)
    other = int(np.flatnonzero(fold != fold[0])[0])
    y = codes.copy()
    y[[0, other]] = 7                                                         # class 7: two cells in two folds, so one
                                                                              # training cell in each of those folds
    with pytest.raises(ValueError, match="y has only 1 sample in class 7, covariance is ill defined."):
        CA.QDA_classifier(x, {"a": y}, 3, 0)
    with pytest.raises(ValueError, match="only 1 sample"):
        GR.cv_predict(x, y, 3, 0, "qda")


def test_process_group_is_refused(monkeypatch):
    x, codes = GI.points(60, 3, 3)
    monkeypatch.setattr(CA.D, "is_dist", lambda: True)
    for call in (lambda: CA.QDA_classifier(x, {"a": codes}, 3, 0), lambda: CA.LDA_classifier(x, {"a": codes}, 3, 0),
                 lambda: CA.gaussian_cv_predict(x, codes, 3, 0)):
        with pytest.raises(NotImplementedError, match="not data-parallel"):
            call()

"""CPU: the host side of the random forest (RF_classifier, forest_cv_predict, quantile_bins).  The numpy restatement of the
contract (tests/forest_restatement.py) checked against itself and against sklearn's recorded accuracies
(tests/golden/forest_kat.npz; tools/gen_golden_forest.py); the preconditions the GPU tests lean on -- each edge input of
tests/forest_inputs.py has the property it is named for --; the host-side contract of mmvae_forest_cv: declared, exported,
ABI version unchanged, the workspace rule, every bad argument refused before any device work; the public functions' refusals.

The gate against sklearn.  Both forests are random, so a fixed-seed forest can only be held to sklearn's distribution:
|mean fold accuracy of the restated forest (one seed, 100 trees) - sklearn's mean over 8 forest seeds| <= 4 sqrt(2) s, s the
standard deviation (the unbiased estimate, ddof = 1) over the 8 seeds of sklearn's fold-mean accuracy: the difference of two
independent draws has sqrt(2) the spread, and four of its standard deviations cap a test that is evaluated once.  Measured
(restated mean accuracy, sklearn's mean, distance, gate):
  c0  n 3000 d 10 K 40 spread 3.0   0.9963  0.9967  0.0004  0.0028
  c1  n 3000 d 10 K 40 spread 1.0   0.6310  0.6325  0.0015  0.0096
  c2  n 2000 d  2 K 20 spread 1.5   0.2940  0.2981  0.0041  0.0193
  c3  n 2760 d 10 K 92 spread 2.0   0.9330  0.9281  0.0049  0.0124
The four runs of the restated forest (1200 trees in numpy) take about a minute together."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import forest_inputs as FI  # noqa: E402
import forest_restatement as FR  # noqa: E402
import noise_restatement as NR  # noqa: E402
import distributed_vae_amd  # noqa: F401,E402
from distributed_vae_amd import _native as N  # noqa: E402
from distributed_vae_amd.utils import cluster_analysis as CA  # noqa: E402

G = np.load(os.path.join(ROOT, "tests", "golden", "forest_kat.npz"))
KAT = [tuple(int(v) for v in row) for row in G["cases"]]


# ---- 1. the restatement, against itself ------------------------------------------------------------------------------------
def test_philox_is_the_projects():
    rng = np.random.default_rng(0)
    ctr = rng.integers(0, 2 ** 32, size=(257, 4), dtype=np.uint64)
    for seed in (0, 1, 0xDEADBEEF12345678, 2 ** 64 - 1):
        assert np.array_equal(FR.philox(ctr, seed), NR.philox4x32_10(ctr, NR.key_of(seed)))
    # Random123's known answer for the all-ones counter and key
    assert [int(v) for v in FR.philox(np.full((1, 4), 0xFFFFFFFF), 2 ** 64 - 1)[0]] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]


@pytest.mark.parametrize("nf,g", [(1, 0), (2, 3), (7, 1), (64, 5), (1001, 2)])
def test_bootstrap_draws_training_rows(nf, g):
    rows = np.sort(np.random.default_rng(nf).choice(5 * nf, size=nf, replace=False))
    s = FR.bootstrap(rows, g, 11)
    assert s.shape == (nf,) and np.isin(s, rows).all()
    assert np.array_equal(s, FR.bootstrap(rows, g, 11)) and (nf < 64 or not np.array_equal(s, FR.bootstrap(rows, g + 1, 11)))
    if nf > 1000:
        assert 0.55 < len(np.unique(s)) / nf < 0.71            # 1 - 1 / e of the rows


@pytest.mark.parametrize("d", [1, 2, 3, 4, 5, 10, 128])
def test_feature_order_is_a_lazy_permutation(d):
    for node in (0, 1, 17):
        full = FR.feature_order(d, 2, node, 5)
        assert sorted(full) == list(range(d))
        for steps in (1, min(d, 4), min(d, 5)):
            assert FR.feature_order(d, 2, node, 5, steps) == full[:steps]
    firsts = {FR.feature_order(d, 2, node, 5, 1)[0] for node in range(200)}
    assert firsts <= set(range(d)) and (d == 1 or len(firsts) > 1)


def test_quantile_bins_properties():
    rng = np.random.default_rng(3)
    for n in (2, 63, 255, 256, 257, 1000):
        x = rng.normal(size=(n, 3)).astype(np.float32)
        x[:, 1] = np.round(x[:, 1] * 2.0) / 2.0                 # ties
        x[: n // 2, 2] = np.where(np.arange(n // 2) % 2 == 0, 0.0, -0.0)
        b = FR.quantile_bins(x)
        assert b.dtype == np.uint8 and b.shape == (n, 3)
        for j in range(3):
            order = np.argsort(x[:, j], kind="stable")
            assert (np.diff(b[order, j].astype(int)) >= 0).all()                       # monotone
            for v in np.unique(x[:, j]):
                assert len(np.unique(b[x[:, j] == v, j])) == 1                           # ties share a bin (-0.0 == 0.0)
            if n <= 256:
                assert len(np.unique(b[:, j])) == len(np.unique(x[:, j]))               # exact: a bin per distinct value
        assert b[:, 0].min() == 0 and int(b[:, 0].max()) == ((n - 1) * 256) // n
    with pytest.raises(ValueError, match="NaN or infinity"):
        FR.quantile_bins(np.array([[0.0], [np.inf]]))


EXACT = [k for k, v in FI.CASES.items() if v[0] <= 256 and v[5] != "clones"]


@pytest.mark.parametrize("name", EXACT)
def test_restated_trees_separate_their_own_sample(name):
    c = FI.case(name)
    res, stats = FI.restated(name)
    assert stats["impure"] == 0
    for f in range(c["F"]):
        tr = FR.train_rows(c["fold"], f)
        for t in range(c["T"]):
            g = f * c["T"] + t
            sample = FR.bootstrap(tr, g, c["seed"])
            nodes = res["trees"]["nodes"][g]
            assert np.array_equal(FR.predict_tree(nodes, c["bins"][sample]), c["codes"][sample])
            assert len(nodes) % 2 == 1 and nodes[0, 3] == len(tr)
            split = nodes[:, 0] >= 0
            assert (nodes[split, 3] == nodes[nodes[split, 2], 3] + nodes[nodes[split, 2] + 1, 3]).all()      # rows add up


# ---- 2. the preconditions the GPU tests lean on -----------------------------------------------------------------------------
def test_limits_of_the_inputs_are_those_of_the_source():
    assert (FI.MAX_K, FI.MAX_D) == (N.FOREST_MAX_K, N.FOREST_MAX_D)
    assert FI.CASES["Kmax"][2] == N.FOREST_MAX_K and FI.CASES["d128"][1] == N.FOREST_MAX_D
    assert {FI.CASES[k][0] for k in ("n63", "n64", "n65", "n256", "n257")} == {63, 64, 65, 256, 257}


@pytest.mark.parametrize("name", sorted(FI.CASES))
def test_each_edge_input_has_its_property(name):
    c = FI.case(name)
    res, stats = FI.restated(name)
    n, d, K, F, T, kind = FI.CASES[name]
    assert c["bins"].shape == (n, d) and c["codes"].max() == K - 1 and set(np.unique(c["fold"])) == set(range(F))
    assert len(res["trees"]["nodes"]) == F * T and res["votes"].sum() == n * T
    print(f"{name}: nodes a tree {res['trees']['count'].min()} .. {res['trees']['count'].max()}, {stats}")
    if name == "n256":
        assert all(len(np.unique(c["bins"][:, j])) == n for j in range(d))
    if name == "n257":
        assert any(len(np.unique(c["bins"][:, j])) < n for j in range(d))                # two values share a bin
    if name == "d1":
        assert c["mtry"] == 1 and stats["visited"] == 1
    if name == "d128":
        assert c["mtry"] == 11
    if kind == "const":
        assert (c["bins"][:, 1:] == c["bins"][0, 1:]).all() and stats["visited"] > c["mtry"]    # the "keep drawing" rule
    if kind == "clones":
        assert stats["impure"] > stats["tied"] > 0                                      # majority leaves and tied leaves
    if kind == "chain":
        assert stats["depth"] > FI.CHAIN_DEPTH
    if kind == "absent":
        assert not (c["codes"][c["fold"] != 0] == 3).any() and (c["codes"][c["fold"] == 0] == 3).sum() >= 5
        assert res["votes"][c["fold"] == 0, 3].sum() == 0 and res["votes"][c["fold"] != 0, 3].sum() > 0
    if kind == "plateau":
        between = 0
        for f in range(F):
            train, test = c["bins"][c["fold"] != f], c["bins"][c["fold"] == f]
            for j in range(d):
                occ = np.unique(train[:, j])
                assert np.diff(occ.astype(int)).max() > 8                               # wide gaps between occupied bins
                between += int((~np.isin(test[:, j], occ) & (test[:, j] > occ[0]) & (test[:, j] < occ[-1])).sum())
        assert between >= 8                                     # held-out rows in bins no training row has
    if kind == "lone":
        assert int((c["fold"] == 1).sum()) == 1
    if name == "T1":
        assert T == 1 and (res["best"] == 1).all() and (res["second"] == 0).all()


# ---- 3. the C boundary ------------------------------------------------------------------------------------------------------
def test_entry_points_declared_exported_and_abi_unchanged():
    hdr = open(os.path.join(ROOT, "include", "mmvae.h")).read()
    for name in ("int mmvae_forest_cv", "size_t mmvae_forest_workspace_bytes"):
        assert re.search(r"\b" + re.escape(name) + r"\(", hdr), name
        assert hasattr(N.lib(), name.split()[1])
    assert "mmvae_debug_forest" not in hdr                     # one path, no debug entry
    for word in ("(i, g, node, stream)", "lazy Fisher-Yates", "thr = (b_lo + b_hi) >> 1", "strictly larger score wins",
                 "lowest code on ties", "Departures from sklearn", "bit-identical"):
        assert word in hdr, word
    src = open(os.path.join(ROOT, "distributed-vae_amd", "csrc", "api.hip")).read()
    assert "int mmvae_abi_version(void) { return 5; }" in src and N.lib().mmvae_abi_version() == 5 == N.ABI_VERSION
    assert '"forest.hip"' in open(os.path.join(ROOT, "distributed-vae_amd", "build.py")).read()


def test_launch_constants_are_those_of_the_source():
    hpp = open(os.path.join(ROOT, "distributed-vae_amd", "csrc", "common.hpp")).read()

    def const(name):
        return re.search(r"constexpr (?:int|int64_t) " + name + r" = ([^;]+);", hpp).group(1)
    assert int(const("RF_BINS")) == N.FOREST_BINS == 256
    assert (int(const("RF_MAX_D")), int(const("RF_MAX_K")), int(const("RF_MAX_F")), int(const("RF_MAX_T"))) == \
           (N.FOREST_MAX_D, N.FOREST_MAX_K, N.FOREST_MAX_F, N.FOREST_MAX_T)
    assert const("RF_MAX_N") == "(int64_t)1 << 24" and N.FOREST_MAX_N == 1 << 24
    assert int(const("RF_TREE_BYTES_PER_ROW")) == N.FOREST_TREE_BYTES_PER_ROW == 2 * 16 + 16 + 2 * 4
    assert const("RF_CHUNK_BYTES") == "(int64_t)1 << 30" and N.FOREST_CHUNK_BYTES == 1 << 30
    # the fit kernel's LDS at the largest K: histogram, the four waves' partial sums, nL, and 2.2 KiB of static arrays
    assert N.FOREST_MAX_K * 256 * 4 + 4 * 256 * 20 + 256 * 4 + 2304 <= 160 * 1024


def _ws(n, F, K, T):
    c = N.forest_chunk(n, F, T)
    return (c * (56 * n + 4) + 4 * n * F + 4 * n * K + 4 * F + 15) // 16 * 16


def test_workspace_bytes():
    ws = N.lib().mmvae_forest_workspace_bytes
    for n, d, F, K, T in ((2, 1, 2, 2, 1), (65, 3, 2, 4, 4), (22365, 10, 10, 92, 100), (22365, 100, 10, 115, 100),
                          (1 << 24, 128, 64, 128, 4096)):
        assert ws(n, d, F, K, T) == _ws(n, F, K, T), (n, d, F, K, T)
    assert N.forest_chunk(22365, 10, 100) == 857 < 1000                    # the data set's forest is grown in two chunks
    assert ws(22365, 10, 10, 92, 100) < 2 * 2 ** 30 and ws(22365, 100, 10, 115, 100) < 2 * 2 ** 30
    assert N.forest_chunk(1 << 24, 64, 4096) == 1 and N.forest_chunk(65, 2, 4) == 8
    for n, d, F, K, T in ((1, 3, 2, 4, 4), ((1 << 24) + 1, 3, 2, 4, 4), (65, 0, 2, 4, 4), (65, 129, 2, 4, 4), (65, 3, 1, 4, 4),
                          (65, 3, 65, 4, 4), (65, 3, 2, 1, 4), (65, 3, 2, 129, 4), (65, 3, 2, 4, 0), (65, 3, 2, 4, 4097)):
        assert ws(n, d, F, K, T) == 0, (n, d, F, K, T)


PTR = 0x1000     # fake device pointers: every case must be refused before anything dereferences them


def _forest(bins=PTR, ld=10, n=100, d=10, codes=PTR, fold=PTR, K=7, F=3, T=5, mtry=3, seed=1, ws=PTR, ws_bytes=None, label=PTR,
            best=PTR, second=PTR, votes=PTR, tree_count=PTR, tree_nodes=PTR):
    if ws_bytes is None:
        ws_bytes = 1 << 40
    return N.lib().mmvae_forest_cv(bins, ld, n, d, codes, fold, K, F, T, mtry, seed, ws, ws_bytes, label, best, second, votes,
                                   tree_count, tree_nodes, None)


@pytest.mark.parametrize("case,rc", [
    ("null_bins", -1), ("null_codes", -1), ("null_fold", -1), ("null_ws", -1), ("null_label", -1), ("null_best", -1),
    ("null_second", -1), ("null_tree_count", -1), ("null_tree_nodes", -1), ("n1", -1), ("d0", -1), ("K1", -1), ("F1", -1), ("T0", -1),
    ("mtry0", -1), ("mtry_past_d", -1), ("ld_below_d", -1), ("ws_misaligned", -1), ("n_past", -2), ("d129", -2), ("K129", -2),
    ("F65", -2), ("T4097", -2), ("ws_small", -4)])
def test_forest_cv_rejects_bad_arguments(case, rc):
    kw = {}
    if case.startswith("null_"): kw[case[5:]] = None
    elif case == "n1": kw["n"] = 1
    elif case == "d0": kw["d"] = 0
    elif case == "K1": kw["K"] = 1
    elif case == "F1": kw["F"] = 1
    elif case == "T0": kw["T"] = 0
    elif case == "mtry0": kw["mtry"] = 0
    elif case == "mtry_past_d": kw["mtry"] = 11
    elif case == "ld_below_d": kw["ld"] = 9
    elif case == "ws_misaligned": kw["ws"] = PTR + 8
    elif case == "n_past": kw["n"] = (1 << 24) + 1
    elif case == "d129": kw.update(d=129, ld=129)
    elif case == "K129": kw["K"] = 129
    elif case == "F65": kw["F"] = 65
    elif case == "T4097": kw["T"] = 4097
    elif case == "ws_small": kw["ws_bytes"] = _ws(100, 3, 7, 5) - 1
    assert _forest(**kw) == rc, N.lib().mmvae_last_error_string()
    assert N.lib().mmvae_last_error_string()


def test_python_wrapper_has_no_cpu_fallback():
    import torch
    with pytest.raises(N.NativeError):
        N.forest_cv(torch.zeros(5, 2, dtype=torch.uint8), torch.zeros(5, dtype=torch.int32), torch.zeros(5, dtype=torch.int32),
                    2, 2, 1, 1, 0)


# ---- 4. the public functions' refusals: all before any device work (this machine has no device) -----------------------------
def test_refusals():
    x, codes = FI.points(60, 3, 3)
    calls = (lambda x, y, k: CA.RF_classifier(x, {"a": y}, k, 0), lambda x, y, k: CA.forest_cv_predict(x, y, k, 0))
    for fn in calls:
        with pytest.raises(ValueError, match="greater than one"):
            fn(x, np.zeros(60, dtype=np.int64), 3)
        with pytest.raises(ValueError, match="kfold"):
            fn(x, codes, 1)
        with pytest.raises(ValueError, match="kfold"):
            fn(x, codes, 61)
        with pytest.raises(ValueError, match="labels for"):
            fn(x, codes[:-1], 3)
        bad = x.copy()
        bad[7, 1] = np.nan
        with pytest.raises(ValueError, match="NaN or infinity"):
            fn(bad, codes, 3)
        with pytest.raises(ValueError, match="not \\[n, d\\]"):
            fn(x[:, 0], codes, 3)
        with pytest.raises(NotImplementedError, match="d = 129"):
            fn(np.zeros((60, 129), dtype=np.float32), codes, 3)
        with pytest.raises(NotImplementedError, match="129 classes"):
            fn(np.tile(x, (5, 1)), np.arange(300) % 129, 3)
        with pytest.raises(NotImplementedError, match="65 folds"):
            fn(np.tile(x, (2, 1)), np.tile(codes, 2), 65)
    with pytest.raises(ValueError, match="labels for"):
        CA.RF_classifier(x, {"a": codes, "b": codes[:-1]}, 3, 0)               # the second key: still before any device work
    with pytest.raises(ValueError, match="n_trees"):
        CA.forest_cv_predict(x, codes, 3, 0, n_trees=0)
    with pytest.raises(NotImplementedError, match="4097 trees"):
        CA.forest_cv_predict(x, codes, 3, 0, n_trees=4097)
    for bad_mf in (0, 4, "log2", 1.5):
        with pytest.raises(ValueError, match="max_features"):
            CA.forest_cv_predict(x, codes, 3, 0, max_features=bad_mf)
    with pytest.raises(ValueError, match="kind"):
        CA.gaussian_cv_predict(x, codes, 3, 0, kind="rf")                      # the forest is reached through its own names only


def test_process_group_is_refused(monkeypatch):
    x, codes = FI.points(60, 3, 3)
    monkeypatch.setattr(CA.D, "is_dist", lambda: True)
    for call in (lambda: CA.RF_classifier(x, {"a": codes}, 3, 0), lambda: CA.forest_cv_predict(x, codes, 3, 0)):
        with pytest.raises(NotImplementedError, match="not data-parallel"):
            call()


def test_default_mtry_and_folds_are_the_packages():
    for d in (1, 2, 3, 4, 8, 9, 10, 100, 128):
        x, codes = FI.points(40, d, 2)
        assert CA._forest_refusals(codes, 40, d, 2, 0, 5, "sqrt")[3] == FR.default_mtry(d) == max(1, int(np.sqrt(d)))
    assert np.array_equal(CA.kfold_of(101, 3, 7), FR.fold_split(101, 3, 7))


# ---- 5. against sklearn, from the recorded fixture --------------------------------------------------------------------------
def gate_of(k):
    """(sklearn's mean accuracy over its seeds, the gate 4 sqrt(2) s)."""
    m = G[f"c{k}/acc"].mean(axis=1)
    return float(m.mean()), 4.0 * np.sqrt(2.0) * float(m.std(ddof=1))


def test_fixture_is_what_the_generator_promises():
    assert KAT == [(3000, 10, 3, 0), (3000, 10, 3, 1), (2000, 2, 3, 2), (2760, 10, 3, 3)] and str(G["sklearn"]) == "1.7.2"
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "forest_kat.npz")) < 1024 * 1024
    assert all(G[k].dtype != object for k in G.files) and len(G["seeds"]) == 8
    for k, (n, d, kfold, _) in enumerate(KAT):
        assert G[f"c{k}/x"].dtype == np.float32 and G[f"c{k}/x"].shape == (n, d) and G[f"c{k}/acc"].shape == (8, kfold)
        assert gate_of(k)[1] > 0
    assert [len(np.unique(G[f"c{k}/y"])) for k in range(4)] == [40, 40, 20, 92]
    # what the midpoint rule is worth (recorded 0.6253 with thr = b_lo, 0.6310 with the midpoint; sklearn 0.6325, sd 0.0017)
    lo, mid = (float(v) for v in G["c1/thr_rule"])
    assert abs(mid - gate_of(1)[0]) < abs(lo - gate_of(1)[0]) and lo < G["c1/acc"].mean(axis=1).min() <= mid
    # what the quantisation alone costs sklearn: less than its own spread over seeds
    for k in range(4):
        assert abs(float(G[f"c{k}/raw_bins"][1] - G[f"c{k}/raw_bins"][0])) <= gate_of(k)[1]


@pytest.mark.parametrize("k", range(4))
def test_restated_forest_is_within_sklearns_spread(k):
    n, d, kfold, seed = KAT[k]
    x, y = G[f"c{k}/x"], G[f"c{k}/y"]
    acc, _, _ = FR.classifier(x, {"y": y}, kfold, seed)
    mine = float(np.mean(acc["y"]))
    theirs, gate = gate_of(k)
    print(f"c{k}: restated {mine:.4f}, sklearn {theirs:.4f}, distance {abs(mine - theirs):.4f}, gate {gate:.4f}")
    assert abs(mine - theirs) <= gate

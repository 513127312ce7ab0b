"""CPU: the host side of the silhouette scores (silhouette_samples, silhouette_score, get_SilhScore, cluster_compare).  The
fp64 difference-form restatement (tests/silhouette_restatement.py) against sklearn's recorded results
(tests/golden/silhouette_kat.npz; tools/gen_golden_silhouette.py), against the installed sklearn and on cases with known
answers; the host-side contract of mmvae_silhouette: declared, exported, ABI version unchanged, the workspace size, every bad
argument refused before any device work; the public module importable without sklearn, scipy or matplotlib, and its
ValueError rules.

Bounds.  The restatement and sklearn both work in fp64 on the same values; sklearn's Gram expansion loses a few ulps of the
squared norms to cancellation, which is what e_ref records.  Every case must have e_ref <= 1e-10; the restatement is compared
with the recorded values at e_ref itself (it is the same computation that recorded it) plus 1e-15 for another BLAS."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import silhouette_restatement as SR  # noqa: E402
import distributed_vae_amd  # noqa: F401,E402
from distributed_vae_amd import _native as N  # noqa: E402

G = np.load(os.path.join(ROOT, "tests", "golden", "silhouette_kat.npz"))
CASES = [tuple(int(v) for v in row) for row in G["cases"]]
SLACK = 1e-15


# ---- 1. the fixture is what the generator promises -----------------------------------------------------------------------
def test_fixture_is_what_the_generator_promises():
    assert CASES == [(3, 1, 2), (65, 1, 2), (257, 2, 7), (600, 10, 92), (400, 33, 130), (300, 128, 5)]
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "silhouette_kat.npz")) < 300 * 1024
    assert all(G[k].dtype != object for k in G.files)                       # arrays only
    assert str(G["source"])
    for k, (n, d, K) in enumerate(CASES):
        x, labels = G[f"c{k}/x"], G[f"c{k}/labels"]
        assert x.dtype == np.float32 and x.shape == (n, d) and np.isfinite(x).all() and np.abs(x).max() < 16
        assert labels.dtype == np.int64 and labels.shape == (n,) and sorted(np.unique(labels)) == list(range(K))
        assert G[f"c{k}/samples"].dtype == np.float64 and G[f"c{k}/samples"].shape == (n,)
        assert G[f"c{k}/mean_smp_sc"].dtype == np.float64 and G[f"c{k}/mean_smp_sc"].shape == (K,)
        for name in ("score", "sil_score", "e_ref"):
            assert G[f"c{k}/{name}"].dtype == np.float64 and G[f"c{k}/{name}"].shape == ()
        assert 0 <= float(G[f"c{k}/e_ref"]) <= 1e-10
        assert float(G[f"c{k}/score"]) == float(G[f"c{k}/sil_score"])      # the two calls the reference makes agree
    assert list(G["c0/labels"]) == [0, 0, 1]
    assert G["cc/data"].dtype == np.float32 and G["cc/data"].shape == (300, 40) and int(G["cc/num_pc"]) == 5
    names = [str(v) for v in G["cc/names"]]
    assert len(names) == 2 and G["cc/sil_score"].shape == (2,) and 0 <= float(G["cc/e_ref"]) <= 1e-10
    for i, name in enumerate(names):
        K = len(np.unique(G[f"cc/labels/{name}"]))
        assert G[f"cc/labels/{name}"].shape == (300,)
        assert G[f"cc/silh_smp_score/{i}"].shape == (K,) and G[f"cc/c_size/{i}"].shape == (K,)
        assert G[f"cc/c_size/{i}"].sum() == 300


# ---- 2. the restatement is sklearn's arithmetic -----------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(6))
def test_restatement_equals_recorded_sklearn(k):
    x, labels, e_ref = G[f"c{k}/x"].astype(np.float64), G[f"c{k}/labels"], float(G[f"c{k}/e_ref"])
    got = SR.silhouette_samples(x, labels)
    err = float(np.abs(got - G[f"c{k}/samples"]).max())
    print(f"case {k}: worst |restatement - sklearn| {err:.2e}, e_ref {e_ref:.2e}")
    assert got.dtype == np.float64 and err <= e_ref + SLACK
    means, score = SR.get_silh_score(x, labels)
    assert np.abs(means - G[f"c{k}/mean_smp_sc"]).max() <= e_ref + SLACK
    assert abs(score - float(G[f"c{k}/sil_score"])) <= e_ref + SLACK


def test_restatement_cluster_compare_equals_recorded_reference():
    z = SR.pca_project(G["cc/data"].astype(np.float64), int(G["cc/num_pc"]))
    e_ref = float(G["cc/e_ref"]) + 1e-12                                   # the projection: another SVD, same subspace
    for i, name in enumerate(str(v) for v in G["cc/names"]):
        labels = G[f"cc/labels/{name}"]
        s = SR.silhouette_samples(z, labels)
        means, sizes = SR.class_means(s, labels)
        assert abs(s.mean() - G["cc/sil_score"][i]) <= e_ref
        assert np.abs(means - G[f"cc/silh_smp_score/{i}"]).max() <= e_ref
        assert np.array_equal(sizes[np.argsort(means)], G[f"cc/c_size/{i}"])


def test_restatement_against_live_sklearn():
    metrics = pytest.importorskip("sklearn.metrics")
    rng = np.random.default_rng(5)
    for n, d, K in ((40, 3, 4), (200, 10, 17), (90, 64, 89)):
        x = rng.normal(size=(n, d)).astype(np.float32).astype(np.float64)
        labels = rng.permutation(np.arange(n) % K)
        assert np.abs(SR.silhouette_samples(x, labels) - metrics.silhouette_samples(x, labels)).max() <= 1e-10
        assert abs(SR.silhouette_score(x, labels) - metrics.silhouette_score(x, labels)) <= 1e-10


def test_restatement_hand_cases():
    # two points per cluster on a line: clusters {0, 1} and {4, 6}
    s = SR.silhouette_samples(np.array([[0.0], [1.0], [4.0], [6.0]]), [0, 0, 1, 1])
    a, b = np.array([1.0, 1.0, 2.0, 2.0]), np.array([5.0, 4.0, 3.5, 5.5])
    assert np.array_equal(s, (b - a) / b)
    # a singleton scores 0; its neighbours see it as the other cluster
    s = SR.silhouette_samples(np.array([[0.0], [2.0], [10.0]]), ["a", "a", "b"])
    assert s[2] == 0.0 and np.array_equal(s[:2], [(10 - 2) / 10, (8 - 2) / 8])
    # duplicates: a cluster of identical points has a = 0 < b, so 1; two clusters on one point have a = b = 0, so 0
    s = SR.silhouette_samples(np.array([[1.0, 1.0]] * 3 + [[4.0, 5.0]] * 2), [0, 0, 0, 1, 1])
    assert np.array_equal(s, np.ones(5))
    s = SR.silhouette_samples(np.array([[1.0, 1.0]] * 4 + [[4.0, 5.0]] * 2), [0, 0, 1, 1, 2, 2])
    assert np.array_equal(s, [0.0, 0.0, 0.0, 0.0, 1.0, 1.0])
    # unsorted string labels are encoded in np.unique order
    x = np.array([[0.0], [4.0], [1.0], [6.0]])
    assert np.array_equal(SR.silhouette_samples(x, ["u", "v", "u", "v"]), SR.silhouette_samples(x, [0, 1, 0, 1]))
    assert SR.tolerance(10) == 14 * 2.0 ** -23


# ---- 3. declared, exported, ABI unchanged; the workspace; the launch constants ---------------------------------------------
def _nseg(n, K):
    return K + n // N.SILHOUETTE_SEG_COLS


def _ws_bytes(n, K):
    return 8 * (_nseg(n, K) * n + _nseg(n, K) + 1) + 4 * ((K + 2) // 2 * 2)


def test_entry_points_declared_exported_and_abi_unchanged():
    hdr = open(os.path.join(ROOT, "include", "mmvae.h")).read()
    assert re.search(r"\bint mmvae_silhouette\(", hdr) and re.search(r"\bsize_t mmvae_silhouette_workspace_bytes\(", hdr)
    for word in ("S(i, k)", "f_{l_i} = 1", "max(a_i, b_i) = 0", "bit-identical", "CALLER'S", "mmvae_silhouette_workspace_bytes(n, K)"):
        assert word in hdr, word
    src = open(os.path.join(ROOT, "distributed-vae_amd", "csrc", "api.hip")).read()
    assert "int mmvae_abi_version(void) { return 5; }" in src
    lib = N.lib()
    assert lib.mmvae_abi_version() == 5 == N.ABI_VERSION
    assert hasattr(lib, "mmvae_silhouette") and hasattr(lib, "mmvae_silhouette_workspace_bytes")
    assert not hasattr(lib, "mmvae_debug_silhouette")                      # one launcher path: no debug entry
    build = open(os.path.join(ROOT, "distributed-vae_amd", "build.py")).read()
    assert '"silhouette.hip"' in build


def test_workspace_bytes():
    ws = N.lib().mmvae_silhouette_workspace_bytes
    for n, K in ((3, 2), (65, 2), (511, 7), (512, 7), (513, 512), (22365, 92), (100000, 99999)):
        assert ws(n, K) == _ws_bytes(n, K), (n, K)
    assert _nseg(22365, 92) == 135 and ws(22365, 92) < 25 * 2 ** 20      # the data set: 135 segments at most, 24 MB
    for n, K in ((2, 2), (0, 2), (-1, 2), ((1 << 31) + 1, 2), (10, 1), (10, 0), (10, -1), (10, 10)):
        assert ws(n, K) == 0, (n, K)
    assert ws(10, 9) == _ws_bytes(10, 9) and ws(1 << 31, 2) == _ws_bytes(1 << 31, 2)
    assert ws(1 << 31, (1 << 31) - 1) == 0                               # 2^62 doubles: no size_t holds the bytes


def test_launch_constants_are_those_of_the_source():
    """The module attributes the GPU tests size their shapes by are the constants the kernels were built with."""
    hpp = open(os.path.join(ROOT, "distributed-vae_amd", "csrc", "common.hpp")).read()

    def const(name):
        return int(re.search(r"constexpr int " + name + r" = (\d+);", hpp).group(1))
    assert const("SIL_SEG_COLS") == N.SILHOUETTE_SEG_COLS == 512
    assert const("SIL_ROW_TILE") == N.SILHOUETTE_ROW_TILE == 256
    assert const("SIL_LDS_FLOATS") == N.SILHOUETTE_LDS_FLOATS == 4096
    assert const("SIL_MAX_D") == N.SILHOUETTE_MAX_D == 128
    dv = re.search(r"SIL_DV\[SIL_N_DV\] = \{([^}]*)\}", hpp).group(1)
    assert tuple(int(v) for v in dv.split(",")) == N.SILHOUETTE_DV and const("SIL_N_DV") == len(N.SILHOUETTE_DV)
    # every table entry is built: the launchers instantiate through pd_dispatch, which spans all SIL_N_DV entries of SIL_DV
    csrc = os.path.join(ROOT, "distributed-vae_amd", "csrc")
    pd = open(os.path.join(csrc, "pairdist.hpp")).read()
    body = pd[pd.index("pd_dispatch("):]
    assert re.search(r"I\s*<\s*SIL_N_DV", body) and re.search(r"SIL_DV\[I\]", body) and re.search(r"pd_dispatch<I\s*\+\s*1>", body)
    for src, kernel in (("silhouette.hip", "k_sil_partial"), ("knn.hip", "k_knn_partial")):
        hip = open(os.path.join(csrc, src)).read()
        assert len(re.findall(r"pd_dispatch\(", hip)) == 1 and len(re.findall(kernel + "<", hip)) == 1   # no instance outside the table
    # the d dispatch at its switch points: the last d of one instance and the first of the next
    assert [N.silhouette_dv(d) for d in (1, 4, 5, 8, 9, 12, 13, 16, 17, 24, 25, 32, 33, 48, 49, 64, 65, 96, 97, 128)] == \
        [1, 1, 2, 2, 3, 3, 4, 4, 6, 6, 8, 8, 12, 12, 16, 16, 24, 24, 32, 32]
    assert all(4 * N.silhouette_dv(d) >= d for d in range(1, 129))


# ---- 4. refusals on the host ------------------------------------------------------------------------------------------------
PTR = 0x1000     # fake device pointers: every case must be refused before anything dereferences them


def _sil(x=PTR, ld=10, n=100, d=10, offsets=PTR, K=7, perm=PTR, ws=PTR, ws_bytes=None, s=PTR):
    if ws_bytes is None:
        ws_bytes = _ws_bytes(n, K) if 3 <= n <= 1 << 31 and 2 <= K <= n - 1 else 1 << 40
    return N.lib().mmvae_silhouette(x, ld, n, d, offsets, K, perm, ws, ws_bytes, s, None)


@pytest.mark.parametrize("case,rc", [
    ("null_x", -1), ("null_offsets", -1), ("null_ws", -1), ("null_s", -1), ("n2", -1), ("n0", -1), ("n_neg", -1),
    ("n_past_2_31", -1), ("K1", -1), ("K0", -1), ("K_neg", -1), ("K_n", -1), ("d0", -1), ("d_neg", -1), ("ld_below_d", -1),
    ("ws_misaligned", -1), ("d129", -2), ("ws_small", -4), ("ws_small_d129", -2), ("too_many_segments", -2)])
def test_silhouette_rejects_bad_arguments(case, rc):
    kw = {}
    if case.startswith("null_"): kw[case[5:]] = None
    elif case == "n2": kw.update(n=2, K=2)
    elif case == "n0": kw["n"] = 0
    elif case == "n_neg": kw["n"] = -5
    elif case == "n_past_2_31": kw["n"] = (1 << 31) + 1
    elif case == "K1": kw["K"] = 1
    elif case == "K0": kw["K"] = 0
    elif case == "K_neg": kw["K"] = -2
    elif case == "K_n": kw["K"] = 100
    elif case == "d0": kw["d"] = 0
    elif case == "d_neg": kw["d"] = -1
    elif case == "ld_below_d": kw["ld"] = 9
    elif case == "ws_misaligned": kw["ws"] = PTR + 4
    elif case == "d129": kw.update(d=129, ld=129)
    elif case == "ws_small": kw["ws_bytes"] = _ws_bytes(100, 7) - 1
    elif case == "ws_small_d129": kw.update(d=129, ld=129, ws_bytes=8)
    elif case == "too_many_segments": kw.update(n=1 << 31, K=1 << 23, ws_bytes=1 << 62)   # K + n / 512 above 2^23
    assert _sil(**kw) == rc, N.lib().mmvae_last_error_string()
    assert N.lib().mmvae_last_error_string()


def test_python_wrapper_has_no_cpu_fallback():
    import torch
    x, off = torch.zeros(5, 2), torch.tensor([0, 2, 5])
    with pytest.raises(N.NativeError):
        N.silhouette(x, off)
    with pytest.raises(N.NativeError):
        N.silhouette(x, off, perm=torch.arange(5))


# ---- 5. the public module ---------------------------------------------------------------------------------------------------
def test_public_module_imports_without_sklearn_scipy_or_matplotlib():
    code = ("import sys\n"
            "class Block:\n"
            "    def find_spec(self, name, path=None, target=None):\n"
            "        if name.split('.')[0] in ('sklearn', 'scipy', 'matplotlib', 'seaborn'):\n"
            "            raise ImportError(name + ' is blocked')\n"
            "sys.meta_path.insert(0, Block())\n"
            f"sys.path.insert(0, {ROOT!r})\n"
            "import distributed_vae_amd\n"
            "from distributed_vae_amd.utils import cluster_analysis as CA\n"
            "assert all(callable(getattr(CA, f)) for f in ('silhouette_samples', 'silhouette_score', 'get_SilhScore', 'cluster_compare'))\n"
            "assert CA._figure([('a', [0.1, 0.2])], 3) is None\n"
            "assert not any(m.split('.')[0] in ('sklearn', 'scipy', 'matplotlib', 'seaborn') for m in sys.modules)\n"
            "print('ok')\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr
    from distributed_vae_amd.utils import cluster_analysis as CA
    assert not re.search(r"^(import|from)\s+(sklearn|scipy|matplotlib|seaborn)", open(CA.__file__).read(), flags=re.M)


def test_value_error_rules():
    """Every refusal comes before any device work: these run without a GPU."""
    from distributed_vae_amd.utils import cluster_analysis as CA
    x = np.random.default_rng(0).normal(size=(6, 3))
    for fn in (CA.silhouette_samples, CA.silhouette_score, CA.get_SilhScore):
        with pytest.raises(ValueError, match="Number of labels is 1"):
            fn(x, [4] * 6)                                                # K = 1
        with pytest.raises(ValueError, match="Number of labels is 6"):
            fn(x, list("abcdef"))                                         # K = n
        with pytest.raises(ValueError):
            fn(x, [0, 1, 0, 1, 0])                                        # length mismatch
        bad = x.copy()
        bad[2, 1] = np.nan
        with pytest.raises(ValueError, match="NaN"):
            fn(bad, [0, 1, 0, 1, 0, 1])
        bad[2, 1] = np.inf
        with pytest.raises(ValueError):
            fn(bad, [0, 1, 0, 1, 0, 1])
    with pytest.raises(ValueError, match="num_pc"):
        CA.cluster_compare(x, {"a": [0, 1, 0, 1, 0, 1]})                  # num_pc = 0: a documented departure
    with pytest.raises(ValueError, match="num_pc"):
        CA.cluster_compare(x, {"a": [0, 1, 0, 1, 0, 1]}, num_pc=4)        # more components than the data has
    with pytest.raises(ValueError, match="Number of labels"):
        CA.cluster_compare(x, {"a": [0, 1, 0, 1, 0, 1], "b": [0] * 6}, num_pc=2)


def test_projection_is_the_exact_pca():
    from distributed_vae_amd.utils import cluster_analysis as CA
    data = G["cc/data"].astype(np.float64)
    z = CA._project(data, 5)
    assert z.dtype == np.float64 and z.shape == (300, 5)
    assert np.abs(np.abs(z) - np.abs(SR.pca_project(data, 5))).max() <= 1e-12
    # the variance along the components is the top of the spectrum, in descending order
    sv = np.linalg.svd(data - data.mean(0), compute_uv=False)
    assert np.allclose(np.sqrt((z ** 2).sum(0)), sv[:5], rtol=1e-12)

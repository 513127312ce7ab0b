"""CPU: the host side of the marker-gene analysis (utils/marker_analysis.py, cpl_mixVAE.category_markers).  The numpy
restatement (tests/ranksum_restatement.py) against scipy: U and the rank sums exactly, p within the GPU test's gate; the
module's float64 finish against the restatement; Benjamini-Hochberg against scipy; the host-side contract of mmvae_rank_sum:
declared, exported, ABI version unchanged, the workspace size, every bad argument refused before any device work; the public
module importable without scipy; the ordering of marker_genes; the refusals of category_markers, which come before the engine
is touched.

Bounds.  U and the rank sums are integers or halves below 2^53: equality.  p: scipy forms 2 * norm.sf(|z|), the restatement
erfc(|z| / sqrt 2); d ln p / dz ~ |z|, and z itself carries a few roundings, so the gate is (z^2 + 8) 2^-51 relative, the one
of tests/test_gpu_ranksum.py."""
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ranksum_restatement as RR  # noqa: E402
import distributed_vae_amd  # noqa: F401,E402
from distributed_vae_amd import _native as N  # noqa: E402
from distributed_vae_amd.utils import marker_analysis as MA  # noqa: E402

# (n, D, G, share of zeros)
CASES = [(64, 6, 3, 0.0), (97, 7, 5, 0.5), (333, 6, 12, 0.9), (1000, 5, 4, 0.7)]


def _case(k):
    n, D, G, zf = CASES[k]
    rng = np.random.default_rng(100 + k)
    x = RR.special_columns(RR.log1p_like(rng, n, D, zf), rng)
    codes = rng.integers(0, G, n)
    codes[codes == G - 1] = 0
    codes[n // 2] = G - 1                                                    # a one-cell group
    return x, codes, G


# ---- 1. the restatement is scipy's arithmetic -------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(CASES)))
def test_restatement_equals_scipy(k):
    stats = pytest.importorskip("scipy.stats")
    x, codes, G = _case(k)
    n, D = x.shape
    r2, tie, pos, tot, _ = RR.rank_sums(x, codes, G)
    n_g = np.bincount(codes, minlength=G)
    assert n_g[G - 1] == 1
    U, z = RR.z_score(r2, tie, n_g, n)
    p = RR.p_value(z)
    worst = 0.0
    for d in range(D):
        ranks = stats.rankdata(x[:, d])
        for g in range(G):
            m = codes == g
            assert r2[g, d] == 2.0 * ranks[m].sum()                          # halves below 2^53: exact
            res = stats.mannwhitneyu(x[m, d], x[~m, d], use_continuity=False, method="asymptotic")
            assert res.statistic == U[g, d]
            assert pos[g, d] == (x[m, d] > 0).sum()
            if len(np.unique(x[:, d])) == 1:
                assert z[g, d] == 0.0 and p[g, d] == 1.0 and np.isnan(res.pvalue)   # the stated choice where scipy gives NaN
                continue
            rel = abs(res.pvalue - p[g, d]) / p[g, d]
            worst = max(worst, rel / ((z[g, d] ** 2 + 8) * 2.0 ** -51))
    print(f"case {k}: worst |p - scipy| / p = {worst:.3f} of the gate")
    assert worst <= 1.0


def test_restatement_hand_case():
    x = np.array([[1.0], [2.0], [2.0], [3.0], [-0.0], [0.0]], dtype=np.float32)
    r2, tie, pos, tot, _ = RR.rank_sums(x, np.array([0, 0, 1, 1, 1, 0]), 2)
    # ranks: 3, 4.5, 4.5, 6, 1.5, 1.5
    assert r2[:, 0].tolist() == [2 * 9, 2 * 12] and tie[0] == 6 + 6 and pos[:, 0].tolist() == [2, 2]
    U, z = RR.z_score(r2, tie, [3, 3], 6)
    assert U[:, 0].tolist() == [3.0, 6.0] and z[0, 0] == -z[1, 0] < 0


# ---- 2. the module's float64 finish ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(CASES)))
def test_module_finish_equals_restatement(k):
    x, codes, G = _case(k)
    n = x.shape[0]
    r2, tie, _, _, _ = RR.rank_sums(x, codes, G)
    n_g = np.bincount(codes, minlength=G)
    U, z = RR.z_score(r2, tie, n_g, n)
    U2, z2, p2 = MA.z_and_p(r2, tie, n_g, n)
    assert np.array_equal(U, U2)
    assert (np.abs(z - z2) <= 16 * 2.0 ** -53 * np.abs(z)).all()
    p = RR.p_value(z)
    assert (np.abs(p - p2) <= (z ** 2 + 8) * 2.0 ** -51 * p).all()


def test_zero_variance_gives_z0_p1():
    r2 = np.array([[12, 20], [0, 0], [30, 22]], dtype=np.int64)
    U, z, p = MA.z_and_p(r2, np.array([6 ** 3 - 6, 0]), np.array([3, 0, 6]), 6)       # gene 0 all tied; empty and full groups
    assert not z[:, 0].any() and (p[:, 0] == 1).all() and not z[1:].any() and (p[1:] == 1).all()
    U, z, p = MA.z_and_p(np.array([[2]]), np.array([0]), np.array([1]), 1)           # one cell
    assert U[0, 0] == 0 and z[0, 0] == 0 and p[0, 0] == 1


def test_benjamini_hochberg_against_scipy():
    stats = pytest.importorskip("scipy.stats")
    rng = np.random.default_rng(3)
    p = np.concatenate([rng.random((4, 50)) ** 3, np.zeros((4, 2)), np.ones((4, 3))], axis=1)
    p[1, :10] = p[1, 10]                                                     # ties
    got = MA.benjamini_hochberg(p)
    for row, have in zip(p, got):
        assert np.allclose(have, stats.false_discovery_control(row), rtol=1e-14, atol=0)
        assert np.allclose(have, RR.benjamini_hochberg(row), rtol=1e-14, atol=0)
    assert (got >= p).all() and (got <= 1).all()


# ---- 3. declared, exported, ABI unchanged; the workspace ----------------------------------------------------------------------
def test_entry_points_declared_exported_and_abi_unchanged():
    hdr = open(os.path.join(ROOT, "include", "mmvae.h")).read()
    assert re.search(r"\bint mmvae_rank_sum\(", hdr) and re.search(r"\bsize_t mmvae_rank_sum_workspace_bytes\(", hdr)
    assert re.search(r"#define MMVAE_RANKSUM_MAX_N \(MMVAE_RANKSUM_KEY_LDS_BYTES / 4\)", hdr)
    assert re.search(r"#define MMVAE_RANKSUM_KEY_LDS_BYTES \(128 \* 1024\)", hdr)
    for word in ("lo + hi + 1", "t^3 - t", "bit-identical", "CALLER'S CONTRACT", "NaN IS NOT CHECKED FOR",
                 "mmvae_rank_sum_workspace_bytes(n, D, G)"):
        assert word in hdr, word
    src = open(os.path.join(ROOT, "distributed-vae_amd", "csrc", "api.hip")).read()
    assert "int mmvae_abi_version(void) { return 5; }" in src
    lib = MA._lib()
    assert lib.mmvae_abi_version() == 5 == N.ABI_VERSION
    assert hasattr(lib, "mmvae_rank_sum") and hasattr(lib, "mmvae_rank_sum_workspace_bytes")
    assert '"ranksum.hip"' in open(os.path.join(ROOT, "distributed-vae_amd", "build.py")).read()
    hpp = open(os.path.join(ROOT, "distributed-vae_amd", "csrc", "common.hpp")).read()
    assert "RS_MAX_N = MMVAE_RANKSUM_MAX_N" in hpp
    assert int(re.search(r"constexpr int RS_MAX_G = (\d+);", hpp).group(1)) == MA.MAX_GROUPS == 4096
    assert int(re.search(r"constexpr int RS_CHUNK = (\d+);", hpp).group(1)) == MA.CHUNK
    assert MA.MAX_CELLS == 128 * 1024 // 4 == 32768


def _ws_bytes(n, D):
    return (min(D, MA.CHUNK) * n * 4 + 7) // 8 * 8


def test_workspace_bytes():
    ws = MA._lib().mmvae_rank_sum_workspace_bytes
    for n, D, G in ((1, 1, 1), (3, 1, 2), (1025, 17, 4), (22365, 5032, 92), (32768, 3, 4096), (32768, 512, 1), (32768, 513, 1)):
        assert ws(n, D, G) == _ws_bytes(n, D), (n, D, G)
    assert ws(22365, 5032, 92) < 46 * 10 ** 6                                # the data set: 45.8 MB of staged genes
    for bad in ((0, 5, 1), (-1, 5, 1), (32769, 5, 1), (10, 0, 1), (10, -1, 1), (10, 5, 0), (10, 5, -1), (10, 5, 4097)):
        assert ws(*bad) == 0, bad


# ---- 4. refusals on the host ------------------------------------------------------------------------------------------------
PTR = 0x1000     # fake device pointers: every case must be refused before anything dereferences them


def _call(x=PTR, ld=40, n_total=100, D=40, rows=PTR, n=100, offsets=PTR, G=3, eps=0.0, ws=PTR, ws_bytes=None, r2=PTR, tie=PTR,
          pos=PTR, tot=PTR):
    if ws_bytes is None:
        ws_bytes = _ws_bytes(n, D) if n >= 1 and D >= 1 else 1 << 40
    return MA._lib().mmvae_rank_sum(x, ld, n_total, D, rows, n, offsets, G, eps, ws, ws_bytes, r2, tie, pos, tot, None)


BAD = [
    ("null_x", dict(x=None), -1), ("null_offsets", dict(offsets=None), -1), ("null_ws", dict(ws=None), -1),
    ("null_rank_sum2", dict(r2=None), -1), ("null_tie_term", dict(tie=None), -1), ("null_n_pos", dict(pos=None), -1),
    ("null_sum", dict(tot=None), -1),
    ("n0", dict(n=0), -1), ("n_neg", dict(n=-3), -1),
    ("n_32769", dict(n=32769, n_total=40000), -2), ("n_32769_ws_small", dict(n=32769, n_total=40000, ws_bytes=8), -2),
    ("n_2_40", dict(n=1 << 40, n_total=1 << 41, ws_bytes=1 << 50), -2),
    ("n_total0", dict(n_total=0), -1), ("no_rows_n_above_n_total", dict(rows=None, n=101), -1),
    ("D0", dict(D=0), -1), ("D_neg", dict(D=-1), -1), ("G0", dict(G=0), -1), ("G_neg", dict(G=-1), -1), ("G4097", dict(G=4097), -2),
    ("ld_below_D", dict(ld=39), -1), ("eps_nan", dict(eps=float("nan")), -1), ("ws_misaligned", dict(ws=PTR + 4), -1),
    ("ws_one_byte_short", dict(ws_bytes=_ws_bytes(100, 40) - 1), -4), ("ws_empty", dict(ws_bytes=0), -4),
]


@pytest.mark.parametrize("case,kw,rc", BAD, ids=[b[0] for b in BAD])
def test_rank_sum_rejects_bad_arguments(case, kw, rc):
    assert _call(**kw) == rc, N.lib().mmvae_last_error_string()
    assert N.lib().mmvae_last_error_string()


def test_python_layer_has_no_cpu_fallback():
    import torch
    with pytest.raises(N.NativeError):
        MA.rank_sums(torch.zeros(5, 3), None, torch.tensor([0, 5]))


# ---- 5. the public module ---------------------------------------------------------------------------------------------------
def test_public_module_imports_without_scipy_or_pandas():
    code = ("import sys\n"
            "class Block:\n"
            "    def find_spec(self, name, path=None, target=None):\n"
            "        if name.split('.')[0] in ('scipy', 'pandas', 'sklearn'):\n"
            "            raise ImportError(name + ' is blocked')\n"
            "sys.meta_path.insert(0, Block())\n"
            f"sys.path.insert(0, {ROOT!r})\n"
            "import distributed_vae_amd\n"
            "from distributed_vae_amd.utils import marker_analysis as MA\n"
            "from distributed_vae_amd.cpl_mixvae import cpl_mixVAE\n"
            "assert callable(MA.rank_sum_test) and callable(MA.marker_genes) and callable(cpl_mixVAE.category_markers)\n"
            "assert not any(m.split('.')[0] in ('scipy', 'pandas', 'sklearn') for m in sys.modules)\n"
            "print('ok')\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr
    src = open(MA.__file__).read()
    assert not re.search(r"^(import|from)\s+(scipy|pandas|sklearn)", src, flags=re.M)
    assert "torch.empty" not in src                       # every device buffer comes from _native._workspace


def test_refusals_of_rank_sum_test():
    """Every refusal comes before any device work: these run without a GPU."""
    rng = np.random.default_rng(0)
    x = rng.normal(size=(6, 3))
    with pytest.raises(ValueError, match="6 labels for 5 cells"):
        MA.rank_sum_test(x[:5], [0, 1, 0, 1, 0, 1])
    with pytest.raises(ValueError, match="1-D"):
        MA.rank_sum_test(x, np.zeros((6, 1)))
    with pytest.raises(ValueError, match="rows"):
        MA.rank_sum_test(x, [0, 1, 0], rows=[0, 1])
    with pytest.raises(ValueError, match="rows"):
        MA.rank_sum_test(x, [0, 1, 0], rows=np.arange(3.0))
    with pytest.raises(IndexError):
        MA.rank_sum_test(x, [0, 1, 0], rows=[0, 1, 6])
    with pytest.raises(ValueError, match="groups"):
        MA.rank_sum_test(x, [0, 1, 0, 1, 0, 1], groups=[0, 0])
    with pytest.raises(ValueError, match="eps"):
        MA.rank_sum_test(x, [0, 1, 0, 1, 0, 1], eps=float("nan"))
    with pytest.raises(NotImplementedError, match="32768"):
        MA.rank_sum_test(np.zeros((32769, 1), dtype=np.float32), np.zeros(32769, dtype=np.int64))
    with pytest.raises(NotImplementedError, match="4096"):
        MA.rank_sum_test(np.zeros((5000, 1), dtype=np.float32), np.arange(5000))
    broken = x.copy()
    broken[2, 1] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        MA.rank_sum_test(broken, [0, 1, 0, 1, 0, 1])
    with pytest.raises(ValueError, match="2-D"):
        MA.rank_sum_test(x[:, :1].reshape(6, 1, 1), [0, 1, 0, 1, 0, 1])


def test_marker_genes_ordering():
    z = np.array([[0.5, 3.0, 3.0, -1.0, 3.0, 0.5], [0.0, 0.0, 0.0, 0.0, 0.0, 0.0]])
    res = {"groups": np.array(["a", "b"]), "z": z, "frac": np.array([[1, .2, .9, 1, .5, 1], [0, 0, 0, 0, 0, 0.]])}
    for k in ("pval", "pval_adj", "logfc", "mean", "mean_rest", "frac_rest"):
        res[k] = z * 2
    top = MA.marker_genes(res, n_top=4, gene_names=list("ABCDEF"))
    assert [t["group"] for t in top] == ["a", "b"]
    assert top[0]["genes"].tolist() == [1, 2, 4, 0] and top[0]["names"].tolist() == list("BCEA")      # equal z: by index
    assert top[0]["z"].tolist() == [3.0, 3.0, 3.0, 0.5] and top[0]["logfc"].tolist() == [6.0, 6.0, 6.0, 1.0]
    assert top[1]["genes"].tolist() == [0, 1, 2, 3]
    few = MA.marker_genes(res, n_top=10, min_frac=0.5)
    assert few[0]["genes"].tolist() == [2, 4, 0, 5, 3] and few[0]["names"] is None and few[1]["genes"].tolist() == []
    with pytest.raises(ValueError):
        MA.marker_genes(res, n_top=0)
    with pytest.raises(ValueError):
        MA.marker_genes(res, gene_names=list("ABC"))


def test_category_markers_refusals_with_the_engine_stubbed(monkeypatch):
    from distributed_vae_amd import dist as DI
    from distributed_vae_amd.cpl_mixvae import cpl_mixVAE
    from distributed_vae_amd.utils.dataloader import DeviceLoader

    def engine(*a, **k):
        raise AssertionError("the engine was reached")
    t = object.__new__(cpl_mixVAE)
    t.n_arm, t.n_categories, t.ref_prior, t.device = 2, 5, False, "cpu"
    monkeypatch.setattr(t, "_encode_all", engine, raising=False)
    plain = types.SimpleNamespace(dataset=range(300), batch_size=64, drop_last=False, __iter__=engine)
    with pytest.raises(ValueError, match="arm = 2"):
        t.category_markers(plain, arm=2)
    with pytest.raises(ValueError, match="serves every row once"):
        t.category_markers(types.SimpleNamespace(dataset=range(300), batch_size=64, drop_last=True))
    sharded = object.__new__(DeviceLoader)
    sharded.world_size, sharded.drop_last, sharded.batch_size, sharded.dataset = 2, False, 64, range(300)
    with pytest.raises(ValueError, match="serves every row once"):
        t.category_markers(sharded)
    dropping = object.__new__(DeviceLoader)
    dropping.world_size, dropping.drop_last, dropping.batch_size, dropping.dataset = 1, True, 64, range(300)
    with pytest.raises(ValueError, match="serves every row once"):
        t.category_markers(dropping)
    with pytest.raises(NotImplementedError, match="cap of 32768 cells"):
        t.category_markers(types.SimpleNamespace(dataset=range(32769), batch_size=64, drop_last=False))
    t.ref_prior = True
    with pytest.raises(NotImplementedError, match="ref_prior"):
        t.category_markers(plain)
    t.ref_prior = False
    monkeypatch.setattr(DI, "is_dist", lambda: True)
    with pytest.raises(NotImplementedError, match="not data-parallel"):
        t.category_markers(plain)
    with pytest.raises(NotImplementedError, match="not data-parallel"):
        MA.rank_sum_test(np.zeros((4, 2)), [0, 1, 0, 1])

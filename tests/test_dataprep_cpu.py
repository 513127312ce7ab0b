"""CPU (no GPU): the data preparation (distributed_vae_amd.utils.tools).  The plain-numpy restatement
(tests/dataprep_restatement.py) against the reference's recorded returns (tests/golden/dataprep_kat.npz;
tools/gen_golden_dataprep.py); the gene order's contract on keys; the host-side contract of mmvae_cpm_dense, mmvae_cpm_csr and
mmvae_gene_stats: declared, exported, ABI version unchanged, the workspace rule, every bad argument refused before any device
work; the public module's refusals, which all come before any device work, its import without scipy and under a process
group."""
import importlib
import os
import re
import sys

import numpy as np
import pytest
import torch

import distributed_vae_amd  # noqa: F401
from distributed_vae_amd import _native as N
from distributed_vae_amd.utils import tools as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dataprep_restatement as DR  # noqa: E402

PATH = os.path.join(ROOT, "tests", "golden", "dataprep_kat.npz")
G = np.load(PATH)
U53, U24 = 2.0 ** -53, 2.0 ** -24


# ---- 1. the fixture ---------------------------------------------------------------------------------------------------------
def test_fixture_is_small_and_data_only():
    assert os.path.getsize(PATH) < 1024 * 1024
    assert all(G[k].dtype.kind in "iufbU" for k in G.files)
    counts = G["counts"]
    assert counts.dtype == np.int32 and counts.shape == (301, 1300)
    assert not counts[7].any() and np.count_nonzero(counts[11]) == 1 and {7, 11, 300} <= set(G["rows"].tolist())
    assert 0.15 < float((counts != 0).mean()) < 0.25
    assert not G["xf64"][5].any() and (G["xf64"] < 0).any()
    assert float(G["margin"]) >= 1e-6


# ---- 2. the restatement against the reference's recorded returns ---------------------------------------------------------------
def test_integer_counts_are_bit_equal_to_the_reference():
    counts, rows = G["counts"], G["rows"]
    assert np.array_equal(DR.normalize_cellxgene(counts, cells=rows), G["norm_i"])
    assert np.array_equal(DR.logcpm(counts, cells=rows), G["log_i"])
    assert not G["log_i"][list(rows).index(7)].any()                       # a zero row stays zero
    for dt in (np.int64, np.int16, np.uint8):                              # the width of the counts does not matter
        assert np.array_equal(DR.logcpm(counts.astype(dt), cells=rows), G["log_i"])
    # a selection is the selection of the whole result: the norm runs over all genes
    genes = np.random.default_rng(0).permutation(1300)[:57]
    assert np.array_equal(DR.logcpm(counts, cells=rows, genes=genes), G["log_i"][:, genes])


def _within(got, want, rel):
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got[~nan] == 0, want[~nan] == 0)
    err = np.abs(got[~nan].astype(np.float64) - want[~nan].astype(np.float64))
    assert (err <= rel * np.abs(want[~nan].astype(np.float64))).all(), float((err / np.maximum(np.abs(want[~nan]), 1e-300)).max())


def test_float64_input_is_within_the_summation_bound_of_the_reference():
    x = G["xf64"]
    Gn = x.shape[1]
    with np.errstate(invalid="ignore"):
        _within(DR.normalize_cellxgene(x), G["norm_f64"], (2 * Gn + 2) * U53)
        _within(DR.logcpm(x), G["log_f64"], (2 * Gn + 2) * U53)


def test_the_reference_float32_result_is_within_its_bound_of_the_fp64_restatement():
    x = G["xf64"].astype(np.float32)
    Gn = x.shape[1]
    with np.errstate(invalid="ignore"):
        _within(G["norm_f32"], DR.normalize_cellxgene(x), (Gn + 2) * U24)
        _within(G["log_f32"], DR.logcpm(x), (Gn + 2) * U24)


def test_csr_restatement_round_trip():
    indptr, indices, data, shape = DR.to_csr(G["counts"])
    assert indptr[8] == indptr[7] and indptr[12] - indptr[11] == 1 and indptr[-1] == indices.size == data.size
    dense = np.zeros(shape, dtype=np.int32)
    dense[np.repeat(np.arange(shape[0]), np.diff(indptr)), indices] = data
    assert np.array_equal(dense, G["counts"])


# ---- 3. reorder_genes: the kept set and the key sequence ------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,key", [(np.float32, "order32"), (np.float64, "order64")])
def test_reorder_genes_keeps_the_reference_set_and_key_sequence(dtype, key):
    x, ref = G["expr"].astype(dtype), G[key]
    n = x.shape[0]
    mine, k = DR.reorder_genes(x, float(G["eps"]))
    assert set(mine.tolist()) == set(ref.tolist()) and mine.size == ref.size == len(set(ref.tolist()))
    kk = DR.keys(k, n)
    assert np.array_equal(kk[mine], kk[ref])
    assert (np.diff(kk[mine]) <= 0).all()
    same = np.diff(kk[mine]) == 0
    assert (np.diff(mine)[same] > 0).all()                                 # equal keys by increasing gene index
    assert np.array_equal(T.order_from_counts(k, n, float(G["eps"])), mine)  # the public module's host half


def test_planted_columns():
    x32 = G["expr"]
    n = x32.shape[0]
    p = G["planted"]
    k32, k64 = DR.counts_above(x32, 0.1), DR.counts_above(x32.astype(np.float64), 0.1)
    assert k32[p].tolist() == [0, n, 0, 0, n, 1, n - 1]
    assert k64[p].tolist() == [0, n, n, 0, n, 1, n - 1]                    # float32(0.1) is above the double 0.1
    kept = set(G["order32"].tolist())
    assert not kept & set(p[:5].tolist())                                  # spread 0: dropped
    assert (p[5] in kept) == (np.sqrt(n - 1.0) / n > 0.1) and (p[6] in kept) == (p[5] in kept)
    st = DR.gene_stats(x32, 0.1)
    assert np.array_equal(st["n_above"], k32) and st["std"][p[0]] == 0 and st["kappa"][p[0]] == 1
    np.testing.assert_allclose(st["std"], x32.astype(np.float64).std(axis=0), rtol=1e-12, atol=1e-15)
    sel = np.arange(n)[::-3]
    assert np.array_equal(DR.counts_above(x32, 0.1, sel), DR.counts_above(x32[sel], 0.1))


# ---- 4. declared, exported, ABI unchanged; the workspace; the launch constants ---------------------------------------------
def test_entry_points_declared_exported_and_abi_unchanged():
    hdr = open(os.path.join(ROOT, "include", "mmvae.h")).read()
    for decl in (r"\bint mmvae_cpm_dense\(", r"\bint mmvae_debug_cpm_dense\(", r"\bint mmvae_cpm_csr\(", r"\bint mmvae_gene_stats\(",
                 r"\bint mmvae_debug_gene_stats\(", r"\bsize_t mmvae_gene_stats_workspace_bytes\("):
        assert re.search(decl, hdr), decl
    for word in ("over ALL G genes", "nothing contracted", "bit-identical", "CALLER'S", "INPUTS MUST BE FINITE",
                 "8 * 3 * ceil(n / 256) * D", "(n + 2) kappa 2^-53"):
        assert word in hdr, word
    src = open(os.path.join(ROOT, "distributed-vae_amd", "csrc", "api.hip")).read()
    assert "int mmvae_abi_version(void) { return 5; }" in src
    lib = N.lib()
    assert lib.mmvae_abi_version() == 5 == N.ABI_VERSION
    for name in ("mmvae_cpm_dense", "mmvae_debug_cpm_dense", "mmvae_cpm_csr", "mmvae_gene_stats", "mmvae_debug_gene_stats",
                 "mmvae_gene_stats_workspace_bytes"):
        assert hasattr(lib, name), name
    assert callable(N.cpm_dense) and callable(N.cpm_csr) and callable(N.gene_stats)
    build = open(os.path.join(ROOT, "distributed-vae_amd", "build.py")).read()
    assert '"dataprep.hip"' in build


def _ws_bytes(n, D):
    return 8 * 3 * ((n + N.GENESTATS_SEG_ROWS - 1) // N.GENESTATS_SEG_ROWS) * D


def test_workspace_bytes():
    ws = N.lib().mmvae_gene_stats_workspace_bytes
    for n, D in ((1, 1), (255, 5), (256, 5), (257, 5), (22365, 5032), (25481, 45768), (1 << 31, 5)):
        assert ws(n, D) == _ws_bytes(n, D), (n, D)
    assert ws(22365, 5032) < 11 * 2 ** 20                                  # the data set: 88 segments, 10.6 MB
    sizes = [ws(n, 7) for n in range(1, 1100)]
    assert all(b >= a for a, b in zip(sizes, sizes[1:]))
    for bad in ((0, 5), (-1, 5), ((1 << 31) + 1, 5), (10, 0), (10, -1), (1 << 31, 1 << 30)):
        assert ws(*bad) == 0, bad


def test_launch_constants_are_those_of_the_source():
    hpp = open(os.path.join(ROOT, "distributed-vae_amd", "csrc", "common.hpp")).read()

    def const(name):
        return eval(re.search(r"constexpr int " + name + r" = ([\d <]+);", hpp).group(1))
    assert const("CPM_THREADS") == N.CPM_THREADS == 256
    assert const("CPM_WINDOW") == N.CPM_WINDOW == 4096 and N.CPM_WINDOW % (4 * N.CPM_THREADS) == 0
    assert const("CPM_MAX_G") == N.CPM_MAX_G == T.MAX_GENES == 1 << 20
    assert const("GS_SEG_ROWS") == N.GENESTATS_SEG_ROWS == 256
    assert const("GS_TILE") == N.GENESTATS_TILE == 256
    assert N.CPM_PATHS == N.GENESTATS_PATHS == {"auto": -1, "narrow": 0, "wide": 1}
    assert N.CPM_VTYPES == {torch.int32: 0, torch.float32: 1, torch.float64: 2} and N.CPM_OTYPES == {torch.float32: 0, torch.float64: 1}


# ---- 5. refusals of the library on the host -------------------------------------------------------------------------------
PTR = 0x1000     # fake device pointers: every case must be refused before anything dereferences them


def _dense(x=PTR, vtype=0, ld=40, n_total=100, Gn=40, rows=PTR, n=100, genes=PTR, ng=7, scaler=1e6, mode=1, out=PTR, otype=0,
           norms=PTR, path=None):
    if path is None:
        return N.lib().mmvae_cpm_dense(x, vtype, ld, n_total, Gn, rows, n, genes, ng, scaler, mode, out, otype, norms, None)
    return N.lib().mmvae_debug_cpm_dense(x, vtype, ld, n_total, Gn, rows, n, genes, ng, scaler, mode, out, otype, norms, path, None)


def _csr(indptr=PTR, indices=PTR, data=PTR, vtype=0, nnz=50, n_total=100, Gn=40, rows=PTR, n=100, inv=PTR, ng=7, scaler=1e6,
         mode=1, out=PTR, otype=0, norms=PTR):
    return N.lib().mmvae_cpm_csr(indptr, indices, data, vtype, nnz, n_total, Gn, rows, n, inv, ng, scaler, mode, out, otype, norms,
                                 None)


def _stats(data=PTR, vtype=1, ld=40, n_total=100, D=40, rows=PTR, n=100, eps=0.1, ws=PTR, ws_bytes=None, k=PTR, mean=PTR, sd=PTR,
           path=None):
    if ws_bytes is None:
        ws_bytes = _ws_bytes(n, D) if 1 <= n <= 1 << 31 and D >= 1 else 1 << 40
    if path is None:
        return N.lib().mmvae_gene_stats(data, vtype, ld, n_total, D, rows, n, eps, ws, ws_bytes, k, mean, sd, None)
    return N.lib().mmvae_debug_gene_stats(data, vtype, ld, n_total, D, rows, n, eps, ws, ws_bytes, k, mean, sd, path, None)


COMMON = [
    ("null_out", dict(out=None), -1), ("null_norms", dict(norms=None), -1), ("vtype3", dict(vtype=3), -1),
    ("vtype_neg", dict(vtype=-1), -1), ("otype2", dict(otype=2), -1), ("mode2", dict(mode=2), -1), ("n0", dict(n=0), -1),
    ("n_2_31", dict(n=1 << 31), -1), ("n_total0", dict(n_total=0), -1), ("no_rows_n_above_n_total", dict(rows=None, n=101), -1),
    ("G0", dict(Gn=0), -1), ("ng0", dict(ng=0), -1), ("scaler_nan", dict(scaler=float("nan")), -1),
    ("scaler_inf", dict(scaler=float("inf")), -1),
]
BAD_DENSE = COMMON + [
    ("null_x", dict(x=None), -1), ("ld_below_G", dict(ld=39), -1), ("no_genes_ng_not_G", dict(genes=None), -1),
    ("x_misaligned", dict(x=PTR + 2), -1), ("x_misaligned_double", dict(x=PTR + 4, vtype=2), -1),
    ("G_above_cap", dict(Gn=(1 << 20) + 1, ld=(1 << 20) + 1), -2), ("ng_above_cap", dict(ng=(1 << 20) + 1), -2),
    ("debug_path_2", dict(path=2), -1), ("debug_path_neg2", dict(path=-2), -1),
    ("debug_wide_on_odd_ld", dict(path=1, ld=41), -2), ("debug_wide_on_offset_base", dict(path=1, x=PTR + 4), -2),
    ("debug_wide_on_odd_ld_double", dict(path=1, ld=41, vtype=2), -2),
]
BAD_CSR = COMMON + [
    ("null_indptr", dict(indptr=None), -1), ("null_inv", dict(inv=None), -1), ("nnz_neg", dict(nnz=-1), -1),
    ("null_indices", dict(indices=None), -1), ("null_data", dict(data=None), -1), ("ng_above_G", dict(ng=41), -1),
    ("G_above_cap", dict(Gn=(1 << 20) + 1), -2),
]
BAD_STATS = [
    ("null_data", dict(data=None), -1), ("null_ws", dict(ws=None), -1), ("null_k", dict(k=None), -1), ("null_mean", dict(mean=None), -1),
    ("null_sd", dict(sd=None), -1), ("vtype0", dict(vtype=0), -1), ("vtype3", dict(vtype=3), -1), ("n0", dict(n=0), -1),
    ("n_past_2_31", dict(n=(1 << 31) + 1), -1), ("n_total0", dict(n_total=0), -1),
    ("no_rows_n_above_n_total", dict(rows=None, n=101), -1), ("D0", dict(D=0), -1), ("ld_below_D", dict(ld=39), -1),
    ("eps_nan", dict(eps=float("nan")), -1), ("ws_misaligned", dict(ws=PTR + 4), -1), ("data_misaligned", dict(data=PTR + 2), -1),
    ("grid_too_large", dict(n=1 << 31, n_total=1 << 31, D=1 << 30, ld=1 << 30, ws_bytes=1 << 62), -2),
    ("ws_small", dict(ws_bytes=_ws_bytes(100, 40) - 1), -4), ("debug_path_2", dict(path=2), -1),
    ("debug_wide_on_odd_ld", dict(path=1, ld=41), -2), ("debug_wide_on_offset_base", dict(path=1, data=PTR + 4), -2),
]


@pytest.mark.parametrize("case,kw,rc", BAD_DENSE, ids=[b[0] for b in BAD_DENSE])
def test_cpm_dense_rejects_bad_arguments(case, kw, rc):
    assert _dense(**kw) == rc, N.lib().mmvae_last_error_string()
    assert N.lib().mmvae_last_error_string()


@pytest.mark.parametrize("case,kw,rc", BAD_CSR, ids=[b[0] for b in BAD_CSR])
def test_cpm_csr_rejects_bad_arguments(case, kw, rc):
    assert _csr(**kw) == rc, N.lib().mmvae_last_error_string()


@pytest.mark.parametrize("case,kw,rc", BAD_STATS, ids=[b[0] for b in BAD_STATS])
def test_gene_stats_rejects_bad_arguments(case, kw, rc):
    assert _stats(**kw) == rc, N.lib().mmvae_last_error_string()


def test_python_wrappers_have_no_cpu_fallback():
    with pytest.raises(N.NativeError):
        N.cpm_dense(torch.zeros(5, 3, dtype=torch.int32))
    with pytest.raises(N.NativeError):
        N.cpm_csr(torch.zeros(6, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), torch.zeros(0), (5, 3),
                  torch.zeros(3, dtype=torch.int32), 3)
    with pytest.raises(N.NativeError):
        N.gene_stats(torch.zeros(5, 3), 0.1)


# ---- 6. the public module's refusals: all on the host, before any device work -------------------------------------------------
class FakeCSR:
    """Any object with the four attributes is a CSR matrix: scipy is optional."""

    def __init__(self, indptr, indices, data, shape):
        self.indptr, self.indices, self.data, self.shape = np.asarray(indptr), np.asarray(indices), np.asarray(data), shape


X = np.arange(35, dtype=np.int32).reshape(5, 7) % 4
CALLS = [
    ("one_dimensional", lambda: T.logcpm(X[0]), ValueError, "not \\[cells, genes\\]"),
    ("three_dimensional", lambda: T.normalize_cellxgene(X[None]), ValueError, "not \\[cells, genes\\]"),
    ("no_rows", lambda: T.logcpm(X[:0]), ValueError, "no rows"),
    ("no_rows_tensor", lambda: T.logcpm(torch.zeros(0, 7)), ValueError, "no rows"),
    ("gene_duplicates", lambda: T.logcpm(X, genes=[1, 2, 1]), ValueError, "duplicates"),
    ("gene_out_of_range", lambda: T.logcpm(X, genes=[1, 7]), ValueError, "outside"),
    ("gene_negative", lambda: T.logcpm(X, genes=[-1]), ValueError, "outside"),
    ("gene_mask", lambda: T.logcpm(X, genes=np.ones(7, bool)), ValueError, "integer"),
    ("gene_empty", lambda: T.logcpm(X, genes=np.zeros(0, np.int64)), ValueError, "empty"),
    ("cell_out_of_range", lambda: T.logcpm(X, cells=[0, 5]), ValueError, "outside"),
    ("cell_mask_shape", lambda: T.logcpm(X, cells=np.ones(4, bool)), ValueError, "mask"),
    ("cell_mask_empty", lambda: T.logcpm(X, cells=np.zeros(5, bool)), ValueError, "empty"),
    ("out_kind", lambda: T.logcpm(X, out="cupy"), ValueError, "out ="),
    ("out_dtype", lambda: T.logcpm(X, dtype=torch.float16), ValueError, "dtype ="),
    ("scaler", lambda: T.logcpm(X, float("inf")), ValueError, "scaler"),
    ("int_range", lambda: T.logcpm(X.astype(np.int64) + 2 ** 31), ValueError, "int32 range"),
    ("uint_range", lambda: T.logcpm(X.astype(np.uint32) + np.uint32(2 ** 31)), ValueError, "int32 range"),
    ("complex", lambda: T.logcpm(X.astype(np.complex64)), TypeError, "counts or floats"),
    ("too_many_genes", lambda: T.logcpm(np.zeros((1, 2 ** 20 + 1), np.int8)), NotImplementedError, "genes above"),
    ("csr_duplicates", lambda: T.logcpm(FakeCSR([0, 2, 3], [1, 1, 0], [1, 2, 3], (2, 3))), ValueError, "sum_duplicates\\(\\)"),
    ("csr_unsorted", lambda: T.logcpm(([0, 2, 3], [2, 1, 0], [1, 2, 3], (2, 3))), ValueError, "sum_duplicates\\(\\)"),
    ("csr_column_range", lambda: T.logcpm(([0, 2, 3], [1, 3, 0], [1, 2, 3], (2, 3))), ValueError, "column index"),
    ("csr_indptr", lambda: T.logcpm(([0, 2, 1], [1, 2, 0], [1, 2, 3], (2, 3))), ValueError, "indptr"),
    ("csr_sizes", lambda: T.logcpm(([0, 2], [1, 2, 0], [1, 2, 3], (2, 3))), ValueError, "do not fit"),
    ("csr_no_rows", lambda: T.logcpm(([0], [], [], (0, 3))), ValueError, "no rows"),
    ("stats_sparse", lambda: T.gene_stats(FakeCSR([0, 1], [0], [1.0], (1, 3))), TypeError, "dense"),
    ("stats_one_dimensional", lambda: T.gene_stats(X[0].astype(np.float32)), ValueError, "not \\[cells, genes\\]"),
    ("stats_rows", lambda: T.gene_stats(X.astype(np.float32), rows=[5]), ValueError, "outside"),
    ("stats_eps", lambda: T.gene_stats(X.astype(np.float32), float("nan")), ValueError, "eps"),
    ("reorder_no_rows", lambda: T.reorder_genes(X[:0].astype(np.float32)), ValueError, "no rows"),
    ("reorder_rows_mask", lambda: T.reorder_genes(X.astype(np.float32), rows=np.ones(3, bool)), ValueError, "mask"),
]


@pytest.mark.parametrize("case,call,exc,match", CALLS, ids=[c[0] for c in CALLS])
def test_public_module_refuses_on_the_host(case, call, exc, match, monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("device work before the refusal")
    for name in ("cpm_dense", "cpm_csr", "gene_stats"):
        monkeypatch.setattr(N, name, no_device)
    monkeypatch.setattr(T._Matrix, "to", no_device)
    with pytest.raises(exc, match=match):
        call()


def test_signatures_mirror_the_reference():
    import inspect
    for fn, positional in ((T.normalize_cellxgene, ["x"]), (T.logcpm, ["x", "scaler"]), (T.reorder_genes, ["x", "chunksize", "eps"]),
                           (T.gene_stats, ["x", "eps"])):
        ps = inspect.signature(fn).parameters
        assert [k for k, p in ps.items() if p.kind == p.POSITIONAL_OR_KEYWORD] == positional
        assert all(p.kind == p.KEYWORD_ONLY for k, p in ps.items() if k not in positional)
    sig = inspect.signature(T.logcpm).parameters
    assert sig["scaler"].default == 1e6 and sig["out"].default == "numpy" and sig["dtype"].default is None
    sig = inspect.signature(T.reorder_genes).parameters
    assert sig["chunksize"].default == 1000 and sig["eps"].default == 1e-1
    for name in ("get_paths", "parse_toml", "download_file"):
        assert not hasattr(T, name) and name in T.__doc__


def test_process_group_is_refused(monkeypatch):
    monkeypatch.setattr(T.D, "is_dist", lambda: True)
    xf = X.astype(np.float32)
    for call in (lambda: T.logcpm(X), lambda: T.normalize_cellxgene(X), lambda: T.reorder_genes(xf), lambda: T.gene_stats(xf)):
        with pytest.raises(NotImplementedError, match="not data-parallel"):
            call()


def test_module_imports_and_takes_csr_without_scipy(monkeypatch):
    for name in [k for k in sys.modules if k == "scipy" or k.startswith("scipy.")]:
        monkeypatch.delitem(sys.modules, name)
    monkeypatch.setitem(sys.modules, "scipy", None)                       # `import scipy` now raises ImportError
    monkeypatch.setitem(sys.modules, "scipy.sparse", None)
    with pytest.raises(ImportError):
        import scipy  # noqa: F401
    mod = importlib.reload(T)
    try:
        assert "scipy" not in re.sub(r'""".*?"""', "", open(mod.__file__).read(), flags=re.S)
        m = mod._Matrix(FakeCSR(*DR.to_csr(G["counts"])), "logcpm")
        assert m.kind == "csr" and m.shape == (301, 1300) and m.data.dtype == torch.int32 and m.indices.dtype == torch.int32
        with pytest.raises(ValueError, match="sum_duplicates"):
            mod.logcpm(FakeCSR([0, 2], [0, 0], [1, 1], (1, 2)))
    finally:
        monkeypatch.undo()
        importlib.reload(T)


def test_scipy_csr_is_taken_where_scipy_is_present():
    sp = pytest.importorskip("scipy.sparse")
    m = T._Matrix(sp.csr_matrix(G["counts"]), "logcpm")
    indptr, indices, data, _ = DR.to_csr(G["counts"])
    assert np.array_equal(m.indptr.numpy(), indptr) and np.array_equal(m.indices.numpy(), indices) and np.array_equal(m.data.numpy(), data)
    with pytest.raises(TypeError, match="tocsr"):
        T._Matrix(sp.csc_matrix(G["counts"]), "logcpm")


def test_input_forms():
    """Integer widths are cast to int32, half types to float32, float32 and float64 stay; a strided host view is accepted."""
    for dt, want in ((np.int8, torch.int32), (np.uint8, torch.int32), (np.uint16, torch.int32), (np.int64, torch.int32),
                     (np.bool_, torch.int32), (np.float16, torch.float32), (np.float32, torch.float32), (np.float64, torch.float64)):
        assert T._Matrix(X.astype(dt), "logcpm").value_dtype == want, dt
    assert T._Matrix(torch.from_numpy(X).to(torch.bfloat16), "logcpm").value_dtype == torch.float32
    assert T._Matrix(X[:, ::-1], "logcpm").shape == (5, 7) and T._Matrix(X.tolist(), "logcpm").value_dtype == torch.int32
    assert T._out_dtype(None, torch.int32) == T._out_dtype(None, torch.float64) == torch.float64
    assert T._out_dtype(None, torch.float32) == T._out_dtype(np.float32, torch.int32) == T._out_dtype("float32", torch.int32) == torch.float32

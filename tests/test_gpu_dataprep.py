"""GPU: data preparation on the device.  mmvae_cpm_dense, mmvae_cpm_csr and mmvae_gene_stats through their wrappers, and the
public ``distributed_vae_amd.utils.tools``, against the plain-numpy restatement (tests/dataprep_restatement.py) on the same
inputs, at the smallest shapes where the kernels can go wrong: G across the 16-byte piece's tail and across one workgroup's
stride (256 pieces), n of one, two and more rows, CSR rows across the 256-entry round and the 4096-column window, gene_stats
across the 256-row segment and the 256-gene tile.

Gates.  Norms: integer input exact; float input within (G + 2) 2^-53 sum |x| of the fp64 restatement.
x / norm * scaler: bit-equal to the same three IEEE operations in numpy on the device's norm.  log1p to float32: within one
float32 ulp of float32(restatement), exact zeros bit-equal.  log1p to float64: the device library's log1p and numpy's are
both measured against log1p in np.longdouble on the same arguments; the gate is twice numpy's worst error plus 2 ulp
(the last test prints what the module measured)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dataprep_restatement as DR  # noqa: E402
from gpu_util import DEV  # noqa: E402
from distributed_vae_amd import _native as N  # noqa: E402
from distributed_vae_amd.utils import tools as T  # noqa: E402
from distributed_vae_amd.utils.dataloader import get_loaders  # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dataprep_kat.npz"))
U53 = 2.0 ** -53
VTYPES = {"int32": np.int32, "float32": np.float32, "float64": np.float64}
OTYPES = {"float32": torch.float32, "float64": torch.float64}
GS = (1, 3, 4, 5, 1023, 1024, 1025, 2051)
NS = (1, 2, 67)
SCALER = 1e6
SEG, TILE = N.GENESTATS_SEG_ROWS, N.GENESTATS_TILE
WORST = {"device": 0.0, "numpy": 0.0}       # log1p errors in fp64 ulps over everything this module ran (printed by the last test)


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _padded(x):
    """x on the device as the leading columns of a matrix whose row pitch is a whole number of 16 bytes: both load forms apply."""
    n, G = x.shape
    ld = (G + 3) // 4 * 4
    big = torch.zeros(n, ld, dtype=torch.from_numpy(x[:0]).dtype, device=DEV)
    big[:, :G] = _dev(x)
    v = big[:, :G]
    assert N.cpm_wide(v)
    return v


@functools.lru_cache(maxsize=None)
def matrix(kind, n, G, seed=0):
    """Non-negative counts (int32) or grid values (floats), about 20 % non-zero; with n >= 2 row 1 is zero; with n >= 4 row 2
    has one non-zero and row 3 no zero at all."""
    rng = np.random.default_rng(1000 * n + G + seed)
    x = rng.poisson(0.22, size=(n, G)) * rng.integers(1, 40, size=(n, G))
    if n >= 2:
        x[1] = 0
    if n >= 4:
        x[2] = 0
        x[2, rng.integers(G)] = 5
        x[3] = rng.integers(1, 9, size=G)
    x = x.astype(VTYPES[kind]) if kind == "int32" else (x / 8.0).astype(VTYPES[kind])
    return x


def selections(n, G, rng):
    """(genes, cells): none; a shuffled subset with a mask; the full set shuffled with non-monotone indices; one gene."""
    mask = rng.random(n) < 0.6
    mask[rng.integers(n)] = True
    return [(None, None),
            (rng.permutation(G)[:max(1, G // 3)], mask),
            (rng.permutation(G), rng.permutation(n)[:max(1, (2 * n) // 3)]),
            (np.array([G - 1]), None)]


def log_gate(arg, got):
    """The float64 log1p gate on the arguments ``arg``: (device worst, numpy worst, gate) in fp64 ulps."""
    nz = arg != 0
    if not nz.any():
        return 0.0, 0.0, 2.0
    a = arg[nz]
    truth = np.log1p(a.astype(np.longdouble))
    sp = np.spacing(np.abs(truth.astype(np.float64))).astype(np.longdouble)
    e_np = float((np.abs(np.log1p(a).astype(np.longdouble) - truth) / sp).max())
    e_dev = float((np.abs(got[nz].astype(np.longdouble) - truth) / sp).max())
    WORST["device"], WORST["numpy"] = max(WORST["device"], e_dev), max(WORST["numpy"], e_np)
    return e_dev, e_np, 2.0 * e_np + 2.0


def check_cpm(x, out, norms, genes, cells, log, odt, scaler):
    """One result of either kernel against the restatement."""
    r, g = DR.select(cells, x.shape[0]), DR.select(genes, x.shape[1])
    Gn = x.shape[1]
    out, norms = out.cpu().numpy(), norms.cpu().numpy()
    assert out.shape == (len(r), len(g)) and out.dtype == (np.float32 if odt == torch.float32 else np.float64)
    want, sums = DR.cpm(x, scaler, log, genes, cells)
    if x.dtype.kind == "i":
        assert np.array_equal(norms, sums)
    else:
        assert (np.abs(norms - sums) <= (Gn + 2) * U53 * sums).all(), float(np.abs(norms - sums).max())
    norm = np.where(norms == 0.0, 1.0, norms)
    arg = x[np.ix_(r, g)].astype(np.float64) / norm[:, None] * np.float64(scaler)      # the device's argument, to the bit
    assert np.array_equal(out == 0, arg == 0)                              # exact zeros, and only they
    if not log:
        assert np.array_equal(out, arg.astype(out.dtype))
        if x.dtype.kind == "i":
            assert np.array_equal(out, want.astype(out.dtype))             # integer norms are the restatement's own
        return
    ref = np.log1p(arg)
    if odt == torch.float32:
        ref32 = ref.astype(np.float32)
        assert (np.abs(out.astype(np.float64) - ref32.astype(np.float64)) <= np.spacing(ref32).astype(np.float64)).all()
    else:
        e_dev, e_np, gate = log_gate(arg, out)
        assert e_dev <= gate, (e_dev, e_np, gate, arg[np.unravel_index(np.argmax(np.abs(out - ref)), out.shape)])


def run_all_forms(x, genes, cells, log, odt, scaler=SCALER):
    """The narrow and the wide dense form and the CSR kernel on the same matrix and selection: each checked, all bit-equal."""
    xd = _padded(x)
    rows = None if cells is None else _dev(DR.select(cells, x.shape[0]))
    gl = None if genes is None else _dev(np.asarray(genes, dtype=np.int32))
    res = [N.cpm_dense(xd, rows, gl, scaler, log, odt, path=p) for p in ("narrow", "wide", "auto")]
    indptr, indices, data, shape = DR.to_csr(x)
    sel = DR.select(genes, x.shape[1])
    inv = np.full(x.shape[1], -1, dtype=np.int32)
    inv[sel] = np.arange(sel.size, dtype=np.int32)
    res.append(N.cpm_csr(_dev(indptr), _dev(indices), _dev(data), shape, _dev(inv), int(sel.size), rows, scaler, log, odt))
    check_cpm(x, res[0][0], res[0][1], genes, cells, log, odt, scaler)
    for o, nr in res[1:]:
        assert torch.equal(o, res[0][0]) and torch.equal(nr, res[0][1])
    return res[0]


# ---- 1. the two normalisation kernels ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(VTYPES))
@pytest.mark.parametrize("otype", list(OTYPES))
def test_cpm_every_shape_form_and_selection(kind, otype):
    rng = np.random.default_rng(5)
    for G in GS:
        for n in NS:
            x = matrix(kind, n, G)
            for genes, cells in selections(n, G, rng):
                run_all_forms(x, genes, cells, True, OTYPES[otype])
                if otype == "float64":
                    run_all_forms(x, genes, cells, False, OTYPES[otype])               # x / norm * scaler, pinned to the bit
                    run_all_forms(x, genes, cells, False, OTYPES[otype], scaler=1.0)   # normalize_cellxgene


@pytest.mark.parametrize("kind", list(VTYPES))
def test_misaligned_view_takes_the_narrow_form_with_the_same_bits(kind):
    x = matrix(kind, 67, 1025)
    big = torch.zeros(67, 1030, dtype=torch.from_numpy(x[:0]).dtype, device=DEV)
    big[:, 1:1026] = _dev(x)
    view = big[:, 1:1026]
    assert view.data_ptr() % 16 != 0 and not N.cpm_wide(view)
    with pytest.raises(NotImplementedError):
        N.cpm_dense(view, path="wide")
    with pytest.raises(ValueError):
        N.cpm_dense(view, path="lds")
    aligned = _padded(x)
    genes = _dev(np.random.default_rng(1).permutation(1025)[:300].astype(np.int32))
    for odt in OTYPES.values():
        a = N.cpm_dense(view, None, genes, SCALER, True, odt)
        b = N.cpm_dense(aligned, None, genes, SCALER, True, odt, path="wide")
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        check_cpm(x, a[0], a[1], genes.cpu().numpy(), None, True, odt, SCALER)


@pytest.mark.parametrize("kind", list(VTYPES))
def test_csr_rows_across_rounds_and_windows(kind):
    """Rows of more entries than one round of the workgroup (256) and matrices of more columns than one LDS window (4096):
    empty, full, sparse and last-column-only rows; genes dropped by the selection leave zeros."""
    rng = np.random.default_rng(9)
    for G in (N.CPM_WINDOW - 1, N.CPM_WINDOW, N.CPM_WINDOW + 1, 2 * N.CPM_WINDOW + 809):
        x = np.zeros((6, G), dtype=np.int64)
        x[1] = rng.integers(1, 9, size=G)                                  # every entry stored
        x[2] = rng.poisson(0.22, size=G) * rng.integers(1, 40, size=G)
        x[3, G - 1] = 7
        x[4, ::255] = 3
        x[5, N.CPM_WINDOW - 2:] = 2
        x = x.astype(VTYPES[kind]) if kind == "int32" else (x / 8.0).astype(VTYPES[kind])
        genes = rng.permutation(G)[:G // 5]
        for odt in OTYPES.values():
            out, _ = run_all_forms(x, genes, np.array([5, 0, 1, 3, 2, 4, 1]), True, odt)
            assert not out[1].any() and out[2].all()
        run_all_forms(x, None, None, False, torch.float64)


@pytest.mark.parametrize("kind", list(VTYPES))
def test_negative_values_count_by_magnitude(kind):
    x = np.array(matrix(kind, 67, 1025))
    x[::2] = -x[::2]
    out, norms = N.cpm_dense(_padded(x), None, None, 1.0, False, torch.float64)
    check_cpm(x, out, norms, None, None, False, torch.float64, 1.0)
    assert (norms.cpu().numpy() >= 0).all() and (out.cpu().numpy()[2] <= 0).all()


def test_two_runs_are_bit_identical():
    x = matrix("float32", 67, 2051)
    xd = _padded(x)
    indptr, indices, data, shape = (_dev(a) if isinstance(a, np.ndarray) else a for a in DR.to_csr(x))
    inv = _dev(np.arange(2051, dtype=np.int32))
    runs = [N.cpm_dense(xd, log=True, scaler=SCALER) for _ in range(2)] + \
           [N.cpm_csr(indptr, indices, data, shape, inv, 2051, log=True, scaler=SCALER) for _ in range(2)]
    for o, nr in runs[1:]:
        assert torch.equal(o, runs[0][0]) and torch.equal(nr, runs[0][1])
    e = _dev(GOLD["expr"])
    a, b = N.gene_stats(e, 0.1), N.gene_stats(e, 0.1)
    assert all(torch.equal(p, q) for p, q in zip(a, b))


# ---- 2. the per-gene statistics ----------------------------------------------------------------------------------------------
def stats_matrix(dtype, n, D, seed=0):
    """Values on a 1/64 grid with about half exact zeros, and eps = 0.1 with its neighbours in the dtype sprinkled in."""
    rng = np.random.default_rng(77 * n + D + seed)
    t = dtype(0.1)
    palette = np.array([t, np.nextafter(t, dtype(0)), np.nextafter(t, dtype(1)), dtype(np.float32(0.1)), dtype(0.09375), dtype(0.109375)],
                       dtype=dtype)
    x = (np.round(np.abs(rng.normal(size=(n, D))) * 128.0) / 64.0 + 2.0).astype(dtype)
    u = rng.random(size=(n, D))
    x = np.where(u < 0.5, dtype(0), np.where(u < 0.7, palette[rng.integers(len(palette), size=(n, D))], x)).astype(dtype)
    return x


def check_stats(x, got, rows=None):
    n = len(DR.select(rows, x.shape[0]))
    want = DR.gene_stats(x, 0.1, rows)
    k, mean, sd = (a.cpu().numpy() for a in got)
    assert np.array_equal(k, want["n_above"])
    # (n + 2) kappa 2^-53 of the spread, and the two roundings that the value's own representation carries on either side
    bound = (n + 2) * want["kappa"] * U53 * want["std"]
    assert (np.abs(mean - want["mean"]) <= bound + 2 * U53 * np.abs(want["mean"])).all()
    assert (np.abs(sd - want["std"]) <= bound + 2 * U53 * want["std"]).all()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_gene_stats_every_shape_and_form(dtype):
    rng = np.random.default_rng(3)
    for n in (1, SEG - 1, SEG, SEG + 1, 2 * SEG + 3):
        for D in (1, 3, TILE - 1, TILE, TILE + 1):
            x = stats_matrix(dtype, n, D)
            xd = _padded(x)
            res = [N.gene_stats(xd, 0.1, path=p) for p in ("narrow", "wide", "auto")]
            check_stats(x, res[0])
            for other in res[1:]:
                assert all(torch.equal(a, b) for a, b in zip(res[0], other))
            rows = rng.permutation(n)[:max(1, (2 * n) // 3)]
            got = N.gene_stats(xd, 0.1, _dev(rows))
            check_stats(x, got, rows)
            alone = N.gene_stats(_padded(np.ascontiguousarray(x[rows])), 0.1)          # a call on those rows alone: the same bits
            assert all(torch.equal(a, b) for a, b in zip(got, alone))


def test_gene_stats_misaligned_view():
    x = stats_matrix(np.float32, SEG + 1, TILE + 1)
    big = torch.zeros(x.shape[0], x.shape[1] + 6, device=DEV)
    big[:, 1:1 + x.shape[1]] = _dev(x)
    view = big[:, 1:1 + x.shape[1]]
    assert not N.cpm_wide(view)
    with pytest.raises(NotImplementedError):
        N.gene_stats(view, 0.1, path="wide")
    a, b = N.gene_stats(view, 0.1), N.gene_stats(_padded(x), 0.1, path="wide")
    assert all(torch.equal(p, q) for p, q in zip(a, b))


# ---- 3. the public module ---------------------------------------------------------------------------------------------------
def test_public_logcpm_and_normalize_on_the_recorded_counts():
    counts, rows = GOLD["counts"], GOLD["rows"]
    got = T.normalize_cellxgene(counts, cells=rows)
    assert got.dtype == np.float64 and np.array_equal(got, GOLD["norm_i"])             # the reference's own bits
    lg, norms = T.logcpm(counts, cells=rows, return_norms=True)
    assert np.array_equal(norms, DR.row_sums(counts[rows]))
    arg = counts[rows].astype(np.float64) / np.where(norms == 0, 1.0, norms)[:, None] * 1e6
    e_dev, e_np, gate = log_gate(arg, lg)
    assert e_dev <= gate and np.array_equal(lg == 0, GOLD["log_i"] == 0)
    assert (np.abs(lg - GOLD["log_i"]) <= (gate + e_np) * np.spacing(GOLD["log_i"])).all()
    # every input form gives the same bits: other integer widths, a device tensor, CSR as a tuple and as an object
    genes = np.random.default_rng(2).permutation(1300)[:211]
    mask = np.zeros(301, bool)
    mask[rows] = True
    base = T.logcpm(counts, genes=genes, cells=mask)
    assert np.array_equal(base, lg[:, genes])
    csr = DR.to_csr(counts)
    big = torch.zeros(301, 1304, dtype=torch.int32, device=DEV)
    big[:, 1:1301] = torch.from_numpy(counts).to(DEV)
    forms = [counts.astype(np.int64), counts.astype(np.uint16), torch.from_numpy(counts).to(DEV), big[:, 1:1301], csr,
             (csr[0], csr[1], csr[2].astype(np.int16), csr[3]), tuple(_dev(a) for a in csr[:3]) + (csr[3],),
             (csr[0], _dev(csr[1]), csr[2], csr[3])]
    try:
        import scipy.sparse as sp
        forms.append(sp.csr_matrix(counts))
    except ImportError:
        pass
    for f in forms:
        assert np.array_equal(T.logcpm(f, genes=genes, cells=mask), base)
    f32 = T.logcpm(counts, genes=genes, cells=mask, dtype=np.float32, out="torch")
    assert f32.dtype == torch.float32 and f32.is_contiguous() and f32.device.type == "cuda"
    ref32 = base.astype(np.float32)
    assert (np.abs(f32.cpu().numpy().astype(np.float64) - ref32) <= np.spacing(ref32)).all()


def test_public_float_input_dtypes_and_refusals():
    x64 = GOLD["xf64"]
    x64 = np.abs(x64)
    a = T.logcpm(x64)
    b = T.logcpm(x64.astype(np.float32))
    c = T.logcpm(x64.astype(np.float16).astype(np.float32))
    assert a.dtype == np.float64 and b.dtype == np.float32 and c.dtype == np.float32
    assert T.logcpm(torch.from_numpy(x64).to(torch.float16)).dtype == np.float32
    want = DR.logcpm(x64)
    assert (np.abs(a - want) <= (2 * 1300 + 8) * U53 * want).all()
    assert (np.abs(b.astype(np.float64) - want) <= 2.0 ** -23 * want).all()
    for bad in (np.nan, np.inf, -np.inf):
        y = x64.copy()
        y[3, 1299] = bad
        with pytest.raises(ValueError, match="NaN or infinity"):
            T.logcpm(y)
        with pytest.raises(ValueError, match="NaN or infinity"):
            T.normalize_cellxgene(DR.to_csr(y))
        assert np.isfinite(T.logcpm(y, cells=[0, 1, 2])).all()                     # only the selected rows are read
        with pytest.raises(ValueError, match="NaN or infinity"):
            T.gene_stats(y)


@pytest.mark.parametrize("dtype,key", [(np.float32, "order32"), (np.float64, "order64")])
def test_public_reorder_genes_and_gene_stats(dtype, key):
    x = GOLD["expr"].astype(dtype)
    n = x.shape[0]
    order, k = T.reorder_genes(x, return_counts=True)
    mine, k_want = DR.reorder_genes(x, 0.1)
    assert order.dtype == np.int64 and np.array_equal(order, mine) and np.array_equal(k, k_want)
    ref = GOLD[key]
    assert set(order.tolist()) == set(ref.tolist()) and np.array_equal(DR.keys(k, n)[order], DR.keys(k, n)[ref])
    p = GOLD["planted"]
    assert k[p].tolist() == ([0, n, 0, 0, n, 1, n - 1] if dtype == np.float32 else [0, n, n, 0, n, 1, n - 1])
    assert np.array_equal(T.reorder_genes(torch.from_numpy(x).to(DEV), 500, 0.1), order)
    st = T.gene_stats(x)
    assert set(st) == {"n_above", "mean", "std"} and np.array_equal(st["n_above"], k)
    check_stats(x, tuple(torch.from_numpy(st[q]) for q in ("n_above", "mean", "std")))
    sel = np.arange(n)[::-2]
    o2, k2 = T.reorder_genes(x, rows=sel, return_counts=True)
    m2, kw2 = DR.reorder_genes(x, 0.1, sel)
    assert np.array_equal(o2, m2) and np.array_equal(k2, kw2)
    ints = T.gene_stats(GOLD["counts"], 0.5)
    assert np.array_equal(ints["n_above"], (GOLD["counts"] > 0).sum(axis=0))


def test_logcpm_feeds_get_loaders_without_a_copy():
    counts = GOLD["counts"]
    rng = np.random.default_rng(4)
    genes, cells = rng.permutation(1300)[:96], rng.permutation(301)[:200]
    t = T.logcpm(counts, genes=genes, cells=cells, out="torch", dtype=torch.float32)
    tr, te, al = get_loaders(t, batch_size=32, seed=0)
    assert al.data.data_ptr() == t.data_ptr() == tr.data.data_ptr() == te.data.data_ptr()
    xb, idx = next(iter(al))
    assert torch.equal(xb, t[idx.long()]) and xb.shape == (32, 96)
    want = DR.logcpm(counts, genes=genes, cells=cells).astype(np.float32)
    assert (np.abs(t.cpu().numpy().astype(np.float64) - want) <= np.spacing(want)).all()


def test_zz_report_the_measured_log1p_errors():
    """Last in the file: what the float64 gate saw over the whole module (the figures of DESIGN.md section 9h)."""
    print(f"\nlog1p float64, worst error in ulps against np.longdouble: device {WORST['device']:.3f}, numpy {WORST['numpy']:.3f}, "
          f"gate {2 * WORST['numpy'] + 2:.3f}")
    assert WORST["device"] <= 2 * WORST["numpy"] + 2

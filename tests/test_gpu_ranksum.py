"""-m gpu: mmvae_rank_sum, utils.marker_analysis.rank_sum_test / marker_genes and cpl_mixVAE.category_markers against the numpy
restatement (tests/ranksum_restatement.py).

Gates.  rank_sum2, tie_term and n_pos are integers: equal, no element differing.  sum: the device adds exact fp64 terms, at
most n_g + 2 roundings against the longdouble sum: (n_g + 2) 2^-53 sum |x|.  z: U - mean is exact in fp64 (every term is a
multiple of 1/2 below 2^53), so only the variance, the square root and the division round: 16 2^-53 |z|.  p: d ln p / dz ~ |z|
and the two erfc implementations differ by a few 1e-13 at worst over z in [0, 38]: (z^2 + 8) 2^-51 relative where p > 1e-300.

Shapes: the smallest at which each mechanism can go wrong.  n = 1, 2 (fewer keys than the padded 128, one wave), 63, 64, 65
(the staging tile's 64 cells), 1024, 1025 (RS_BIG: a group of 1024 cells is one wave's, one of 1025 the whole workgroup's; 1025
keys pad to 2048 and 1024 threads) and 32768 (the cap: 128 KiB of keys, D = 3 there); D = 1, 15, 16, 17, 63, 64, 65 (the tile's
64 genes) and 513 (a second chunk of staged genes); G = 1, G = n, empty groups in the middle and at the end.  Every case with D > 6 carries an all-zero gene
(column 5), which includes 65 cells, groups above 1024 cells and the cap; the cap runs at D = 3 and again at D = 7, where it
also has the all-distinct gene (full-depth searches at 128 KiB of keys).

cpl_mixVAE.category_markers takes its groups from the model's own labels, which a planted gene would change; the planted-marker
run therefore substitutes the planted labels for the encoder's (everything after the encode is the real path), and a second run
with the model's labels is compared with rank_sum_test on encode_dataset's labels."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ranksum_restatement as RR  # noqa: E402
from gpu_util import DEV  # noqa: E402
from distributed_vae_amd.utils import marker_analysis as MA  # noqa: E402
from tests.alloc_guard import guarded  # noqa: E402

pytestmark = pytest.mark.gpu

# name: (n, D, number of labels, labels absent from the cells (empty groups), share of zeros)
SHAPES = {
    "n1": (1, 5, 1, (), 0.0),
    "n2": (2, 5, 2, (), 0.5),
    "n63_D15": (63, 15, 3, (), 0.6),
    "n64_D16_empty_middle_and_end": (64, 16, 6, (2, 5), 0.6),
    "n65_D17": (65, 17, 4, (), 0.9),
    "n65_D1": (65, 1, 2, (), 0.5),
    "n300_D63": (300, 63, 5, (), 0.7),
    "n300_D64": (300, 64, 1, (), 0.7),
    "n130_D65_every_cell_a_group": (130, 65, 130, (), 0.6),
    "n65_D513_two_chunks": (65, 513, 3, (), 0.7),
    "n1024_one_group": (1024, 7, 1, (), 0.7),
    "n1025_one_group": (1025, 7, 1, (), 0.7),
    "n1025_D16": (1025, 16, 7, (3,), 0.0),
    "n3000_big_and_small_groups": (3000, 7, 4, (), 0.8),
    "cap_n32768_D3": (32768, 3, 5, (1,), 0.7),
    "cap_n32768_D7": (32768, 7, 5, (1,), 0.7),         # with the all-distinct gene (column 4) and the all-zero gene at the cap
}
ZERO_GENE = 5          # planted wherever D > 6 (column D - 1 holds the infinities): every key the canonical zero key
ZERO_CASES = ["n65_D17", "n1025_D16", "n1025_one_group", "n3000_big_and_small_groups", "cap_n32768_D7"]


def _t(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)


@functools.lru_cache(maxsize=None)
def _case(name, zero_eps=False):
    """(x float32 [n, D], labels int64 [n], groups, eps, the restatement's results): computed once, never modified.  eps is a
    positive stored value, or with ``zero_eps`` exactly 0.0 (the same data), where 0 > eps must be false."""
    n, D, L, absent, zf = SHAPES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    x = RR.special_columns(RR.log1p_like(rng, n, D, zf), rng)
    x[:, 0] = -x[:, 0]                                                       # negative values (and their ties)
    if D > 6:
        x[:, ZERO_GENE] = 0.0                                                # an all-zero gene
    if n >= 63:
        x[rng.integers(0, n, 3), D - 1] = np.inf                             # +-inf rank above and below everything
        x[rng.integers(0, n, 3), D - 1] = -np.inf
    present = [g for g in range(L) if g not in absent]
    if L == n:
        labels = rng.permutation(n).astype(np.int64)
    else:
        weights = np.array([1.0 + 5.0 * (k == 0) for k in range(len(present))])        # one large group, small ones
        labels = np.asarray(present, dtype=np.int64)[rng.choice(len(present), size=n, p=weights / weights.sum())]
    stored = np.sort(x[(x > 0) & np.isfinite(x)])
    eps = float(stored[len(stored) // 2]) if len(stored) and not zero_eps else 0.0   # exactly a stored value
    r2, tie, pos, tot, tot_abs = RR.rank_sums(x, labels, L, eps)
    n_g = np.bincount(labels, minlength=L)
    U, z = RR.z_score(r2, tie, n_g, n)
    for a in (x, labels, r2, tie, pos, tot, tot_abs, U, z):
        a.setflags(write=False)
    return x, labels, np.arange(L), eps, dict(r2=r2, tie=tie, pos=pos, tot=tot, tot_abs=tot_abs, n_g=n_g, U=U, z=z, p=RR.p_value(z))


def _check(got, ref, n, what=""):
    assert got["rank_sum2"].dtype == np.int64 and got["tie_term"].dtype == np.int64
    assert np.array_equal(got["rank_sum2"], ref["r2"]), (what, int((got["rank_sum2"] != ref["r2"]).sum()))
    assert np.array_equal(got["tie_term"], ref["tie"]), (what, int((got["tie_term"] != ref["tie"]).sum()))
    assert np.array_equal(got["n"], ref["n_g"])
    n1 = ref["n_g"].astype(np.float64)[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        pos = got["frac"] * n1
    some = ref["n_g"] > 0
    assert np.array_equal(np.rint(pos[some]).astype(np.int64), ref["pos"][some]), what
    assert np.array_equal(got["U"], ref["U"])
    dz = np.abs(got["z"] - ref["z"])
    assert (dz <= 16 * 2.0 ** -53 * np.abs(ref["z"])).all(), (what, float(dz.max()))
    big = ref["p"] > 1e-300
    dp = np.abs(got["pval"] - ref["p"])[big]
    gate = ((ref["z"] ** 2 + 8) * 2.0 ** -51 * ref["p"])[big]
    print(f"{what}: worst |dz| / |z| {float((dz / np.maximum(np.abs(ref['z']), 1e-300)).max()):.2e}, "
          f"worst p error {float((dp / gate).max()) if dp.size else 0.0:.3f} of the gate")
    assert (dp <= gate).all(), what
    # the groups' sums, through the means: mean n_g is the device's sum up to one rounding each way
    fin = np.isfinite(np.asarray(ref["tot"], dtype=np.float64))
    with np.errstate(invalid="ignore"):                                     # (inf - inf in the column of infinities)
        err = np.abs((got["mean"] * n1).astype(np.longdouble) - ref["tot"])
    bound = (n1 + 4) * 2.0 ** -53 * np.asarray(ref["tot_abs"], dtype=np.float64)
    ok = fin & some[:, None]
    assert (err[ok] <= bound[ok]).all(), (what, float(err[ok].max()))
    if got["z"].shape[1] > 6:
        _check_zero_gene(got, n, what)


def _check_zero_gene(got, n, what):
    """The all-zero gene: one run of n ties, no cell above eps >= 0, sums of exactly 0, and the stated z = 0, p = 1."""
    d = ZERO_GENE
    some = got["n"] > 0
    assert got["tie_term"][d] == n ** 3 - n, what
    assert np.array_equal(got["rank_sum2"][:, d], got["n"] * (n + 1)), what  # every cell has the mid-rank (n + 1) / 2
    assert not got["z"][:, d].any() and (got["pval"][:, d] == 1.0).all() and (got["pval_adj"][:, d] == 1.0).all(), what
    assert not got["frac"][some, d].any() and not got["mean"][some, d].any(), what
    if n > got["n"].max():
        assert not got["frac_rest"][:, d].any() and not got["mean_rest"][:, d].any(), what


@pytest.mark.parametrize("name", list(SHAPES))
def test_device_against_restatement(name):
    x, labels, groups, eps, ref = _case(name)
    n, D = x.shape
    got = MA.rank_sum_test(_t(x), labels, groups=groups, eps=eps)
    _check(got, ref, n, name)
    # the raw outputs: n_pos and sum as the kernel wrote them
    order = np.argsort(labels, kind="stable")
    offsets = np.concatenate([[0], np.cumsum(ref["n_g"])]).astype(np.int64)
    r2, tie, pos, tot = (t.cpu().numpy() for t in MA.rank_sums(_t(x), _t(order.astype(np.int64)), _t(offsets), eps))
    assert np.array_equal(r2, ref["r2"]) and np.array_equal(tie, ref["tie"]) and np.array_equal(pos, ref["pos"])
    fin = np.isfinite(np.asarray(ref["tot"], dtype=np.float64))
    with np.errstate(invalid="ignore"):
        err = np.abs(tot.astype(np.longdouble) - ref["tot"])
    bound = (ref["n_g"][:, None] + 2) * 2.0 ** -53 * np.asarray(ref["tot_abs"], dtype=np.float64)
    assert (err[fin] <= bound[fin]).all(), (name, float(err[fin].max()))
    assert np.array_equal(tot[~fin], np.asarray(ref["tot"], dtype=np.float64)[~fin], equal_nan=True)   # +-inf and inf - inf
    # host arrays give the same bits as the device tensor
    host = MA.rank_sum_test(x, labels, groups=groups, eps=eps, device=DEV)
    for k in ("rank_sum2", "tie_term", "z", "pval", "pval_adj", "mean", "frac"):
        assert np.array_equal(host[k], got[k], equal_nan=True), (name, k)


@pytest.mark.parametrize("name", ZERO_CASES)
def test_all_zero_gene_and_eps_zero(name):
    """eps = 0.0 on data with an all-zero gene, at 65 cells, with groups above 1024 cells (one wave's and the whole
    workgroup's reduction) and at the cap: 0 > eps is false for every cell of the gene, and -0.0 > 0.0 is false too."""
    x, labels, groups, eps, ref = _case(name, True)
    n, D = x.shape
    assert eps == 0.0 and not x[:, ZERO_GENE].any() and (name in ("n65_D17", "n1025_D16") or ref["n_g"].max() > 1024)
    assert not ref["pos"][:, ZERO_GENE].any() and ref["pos"][:, 3].sum() == (x[:, 3] > 0).sum() < n   # (the -0.0 gene: zeros too)
    _check(MA.rank_sum_test(_t(x), labels, groups=groups, eps=0.0), ref, n, name + " eps 0")
    order = np.argsort(labels, kind="stable")
    offsets = np.concatenate([[0], np.cumsum(ref["n_g"])]).astype(np.int64)
    r2, tie, pos, tot = (t.cpu().numpy() for t in MA.rank_sums(_t(x), _t(order.astype(np.int64)), _t(offsets), 0.0))
    assert np.array_equal(r2, ref["r2"]) and np.array_equal(tie, ref["tie"]) and np.array_equal(pos, ref["pos"])
    assert not pos[:, ZERO_GENE].any() and not tot[:, ZERO_GENE].any() and tie[ZERO_GENE] == n ** 3 - n


def _bits(t):
    return t.contiguous().reshape(-1).view(torch.uint8)


@pytest.mark.parametrize("name", ["n65_D17", "n1025_D16", "cap_n32768_D7"])
def test_two_runs_equal_bits_and_the_allocation_contract(name, monkeypatch):
    """Plain, then under tests/alloc_guard.py with the fills 0xFF and 0x5A: the workspace and the four outputs all come from
    _native._workspace, so guarding _native guards them.  Guards intact; every output bit-equal to the plain run (an element
    the kernel left unwritten would hold the fill, which differs between the two fills and from the plain run)."""
    x, labels, _, eps, ref = _case(name)
    order = np.argsort(labels, kind="stable")
    offsets = _t(np.concatenate([[0], np.cumsum(ref["n_g"])]).astype(np.int64))
    xd, rows = _t(x), _t(order.astype(np.int64))
    plain = [t.clone() for t in MA.rank_sums(xd, rows, offsets, eps)]
    again = MA.rank_sums(xd, rows, offsets, eps)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(plain, again))
    for fill in (0xFF, 0x5A):
        with guarded(["_native"], fill, monkeypatch=monkeypatch) as g:
            got = MA.rank_sums(xd, rows, offsets, eps)
            g.check()
            assert len(g.allocs) == 5, g.sites()                           # four outputs and the staging workspace
            assert all(a.view.numel() * 8 == a.nbytes for a in g.allocs)
            for k, (a, b) in enumerate(zip(plain, got)):
                assert a.shape == b.shape and a.dtype == b.dtype
                assert torch.equal(_bits(a), _bits(b)), (name, hex(fill), k, int((_bits(a) != _bits(b)).sum()))


def test_gene_subset_strided_view_and_row_map():
    x, labels, groups, eps, ref = _case("n300_D63")
    n, D = x.shape
    full = MA.rank_sum_test(_t(x), labels, groups=groups, eps=eps)
    # a gene subset read through a row-strided view of the device matrix: those columns of the full call
    sub = MA.rank_sum_test(_t(x)[:, 5:42], labels, groups=groups, eps=eps)
    for k in ("rank_sum2", "U", "z", "pval", "mean", "mean_rest", "frac", "frac_rest", "logfc"):
        assert np.array_equal(sub[k], full[k][:, 5:42], equal_nan=True), k
    assert np.array_equal(sub["tie_term"], full["tie_term"][5:42])
    # a row map that permutes and subsets a larger matrix, itself a window of a wider one
    rng = np.random.default_rng(5)
    big = rng.normal(size=(n + 77, D + 9)).astype(np.float32)
    rows = rng.permutation(n + 77)[:n]
    big[rows, 4:4 + D] = x
    mapped = MA.rank_sum_test(_t(big)[:, 4:4 + D], labels, groups=groups, rows=rows, eps=eps)
    for k in ("rank_sum2", "tie_term", "z", "pval", "pval_adj", "mean", "frac", "logfc"):
        assert np.array_equal(mapped[k], full[k], equal_nan=True), k


def test_groups_subset_puts_the_other_cells_into_the_rest():
    x, labels, _, eps, ref = _case("n300_D63")
    got = MA.rank_sum_test(_t(x), labels, groups=[3, 0, 9], eps=eps)          # label 9: no cell
    assert got["groups"].tolist() == [3, 0, 9] and got["n"].tolist() == [int(ref["n_g"][3]), int(ref["n_g"][0]), 0]
    assert np.array_equal(got["rank_sum2"][:2], ref["r2"][[3, 0]]) and not got["rank_sum2"][2].any()
    assert np.array_equal(got["z"][:2], MA.z_and_p(ref["r2"][[3, 0]], ref["tie"], ref["n_g"][[3, 0]], 300)[1])
    assert not got["z"][2].any() and (got["pval"][2] == 1).all() and np.isnan(got["mean"][2]).all()


def _planted(n, D, K, seed):
    """log1p-like data in which gene 3 + 5 k is raised in the cells of category k; labels int64 [n]."""
    rng = np.random.default_rng(seed)
    x = RR.log1p_like(rng, n, D, 0.6)
    labels = rng.integers(0, K, n).astype(np.int64)
    for k in range(K):
        x[labels == k, 3 + 5 * k] += np.float32(2.0)
    return x, labels


def test_planted_markers_top_their_groups():
    x, labels = _planted(600, 64, 6, 1)
    res = MA.rank_sum_test(_t(x), labels)
    top = MA.marker_genes(res, n_top=3, gene_names=[f"g{d}" for d in range(64)])
    for k in range(6):
        assert top[k]["group"] == k and top[k]["genes"][0] == 3 + 5 * k and top[k]["names"][0] == f"g{3 + 5 * k}"
        assert top[k]["z"][0] > 8 and top[k]["pval_adj"][0] < 1e-10 and top[k]["logfc"][0] > 1.5
        assert (np.diff(top[k]["z"]) <= 0).all()


def test_category_markers_end_to_end(monkeypatch):
    from distributed_vae_amd.cpl_mixvae import cpl_mixVAE
    from distributed_vae_amd.utils.dataloader import DeviceLoader
    from torch.utils.data import DataLoader, TensorDataset
    Dm, Cc, A = 256, 6, 2
    t = cpl_mixVAE(saving_folder="", device=0, save_flag=False)
    t.init_model(n_categories=Cc, state_dim=2, input_dim=Dm, fc_dim=32, lowD_dim=6, x_drop=0.5, s_drop=0.2, n_arm=A, temp=1.0,
                 tau=0.005)
    host, planted = _planted(400, Dm, Cc, 2)
    index = torch.from_numpy(np.random.default_rng(2).permutation(400)[:300])
    rows = index.numpy()
    dl = DeviceLoader(_t(host), index, 64, False, False)
    enc = t.encode_dataset(dl)
    assert np.array_equal(enc["data_indx"].astype(np.int64), rows)
    plain = DataLoader(TensorDataset(torch.from_numpy(host[rows]), torch.arange(300, dtype=torch.float32)), batch_size=64)
    for arm in range(A):
        got = t.category_markers(dl, arm=arm, n_top=5)
        labels = enc["predicted_label"][arm].astype(np.int64) - 1
        want = MA.rank_sum_test(host[rows], labels, groups=np.arange(Cc), device=DEV)
        assert np.array_equal(got["categories"], np.arange(Cc)) and got["z"].shape == (Cc, Dm) and len(got["markers"]) == Cc
        for k in ("n", "rank_sum2", "tie_term", "U", "z", "pval", "pval_adj", "mean", "mean_rest", "frac", "frac_rest", "logfc"):
            assert np.array_equal(got[k], want[k], equal_nan=True), (arm, k)
        for c, m in enumerate(got["markers"]):
            assert m["genes"].shape == (5,) and np.array_equal(m["genes"], np.argsort(-got["z"][c], kind="stable")[:5])
        again = t.category_markers(plain, arm=arm, n_top=5)                 # a plain loader: the batches' concatenation
        for k in ("n", "rank_sum2", "tie_term", "z", "pval", "pval_adj", "mean", "logfc"):
            assert np.array_equal(again[k], got[k], equal_nan=True), (arm, k)
    with pytest.raises(ValueError):
        t.category_markers(dl, arm=A)
    # planted markers: the planted labels stand in for the encoder's
    real = t._encode_all

    def with_planted_labels(loader, counts=None):
        out, inds = real(loader, counts)
        out = dict(out)
        lab = torch.from_numpy(planted[inds.to(torch.int64).cpu().numpy()]).to(out["labels"].device, out["labels"].dtype)
        out["labels"] = lab.expand(A, -1).contiguous()
        return out, inds
    monkeypatch.setattr(t, "_encode_all", with_planted_labels)
    got = t.category_markers(dl, arm=0, n_top=3)
    for c in range(Cc):
        assert got["markers"][c]["genes"][0] == 3 + 5 * c and got["n"][c] == (planted[rows] == c).sum()

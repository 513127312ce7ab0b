"""-m gpu: mmvae_knn / mmvae_knn_votes, utils.neighbors and cpl_mixVAE.latent_neighbors / classify_neighbors against the numpy
float64 restatement (tests/knn_restatement.py).

Exact cases.  Integer coordinates in [-8, 8]: every squared distance is an integer below 2^24, exact in float32, so idx and
dist2 equal the restatement in EVERY element, ties (plentiful) by index.  Shapes: n = 1, 2 (fewer cells than k: the -1 / +inf
tails), 63, 64, 65 (the 64-query tile), 255, 256, 257 (the shortest segment the entry chooses, 256 columns) and 1000 (several
tiles and segments); d = 1, 3, 4, 5 (the float4 pieces), 10, 127, 128 (the cap: 32 pieces); k = 1, 2, 15, 63, 64 (below, at
and across the eight-slot chunks of the insertion; the cap).  Each under the three admission modes: none, self-exclusion,
five folds of which fold 0 holds all but k - 1 of the cells (its cells see k - 1 references: a tail).

Float cases.  gamma = (d + 3) 2^-23 relative on the squared distance (knn_restatement.gamma): every returned dist2 within
gamma of the float64 squared distance of the pair it names, rows non-decreasing, and on the unambiguous cells
(knn_restatement.unambiguous) the index set of the restatement; at most 2 % of a case's cells may be ambiguous (asserted)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_restatement as KR  # noqa: E402
from gpu_util import DEV  # noqa: E402
from distributed_vae_amd.utils import neighbors as NB  # noqa: E402
from tests.alloc_guard import guarded  # noqa: E402

pytestmark = pytest.mark.gpu

NS = (1, 2, 63, 64, 65, 255, 256, 257, 1000)
DS = (1, 3, 4, 5, 10, 127, 128)
KS = (1, 2, 15, 63, 64)
# every (n, d) pair, every k with every n and (over the n) with every d
LATTICE = [(n, d, KS[(i + j) % len(KS)]) for i, n in enumerate(NS) for j, d in enumerate(DS)]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _i32(a):
    return _t(np.asarray(a).astype(np.int32))


def _bits(t):
    return t.contiguous().reshape(-1).view(torch.uint8)


def _folds(n, k, seed):
    """Five folds; fold 0 holds all but k - 1 of the cells (all but one where n <= k), the others share the rest."""
    fold = np.zeros(n, dtype=np.int64)
    rest = np.random.default_rng(seed).permutation(n)[:min(k - 1, n - 1)]
    fold[rest] = 1 + np.arange(len(rest)) % 4
    return fold


def _device(q, r, k, qg=None, rg=None, **kw):
    idx, dist2 = NB.knn_device(_t(q), _t(r), k, None if qg is None else _i32(qg), None if rg is None else _i32(rg), **kw)
    return idx.cpu().numpy(), dist2.cpu().numpy()


def _assert_exact(got, want, what):
    idx, dist2 = got
    ref_idx, ref_d2, _ = want
    assert idx.dtype == np.int32 and dist2.dtype == np.float32 and idx.shape == ref_idx.shape
    assert np.array_equal(idx, ref_idx), (what, int((idx != ref_idx).sum()))
    assert np.array_equal(dist2, ref_d2.astype(np.float32)), what


@pytest.mark.parametrize("n,d,k", LATTICE, ids=[f"n{n}_d{d}_k{k}" for n, d, k in LATTICE])
def test_lattice_equals_the_restatement_in_every_element(n, d, k):
    x = KR.lattice(n, d, seed=n * 1000 + d)
    d2 = KR.sqdist(x, x)
    assert d2.max() < 2 ** 24
    own = np.arange(n)
    fold = _folds(n, k, seed=n + d)
    for what, g in (("none", None), ("self", own), ("folds", fold)):
        want = KR.neighbors(x, x, k, g, g, d2=d2)
        if what == "folds" and n > k + 1:
            assert (want[0][fold == 0, k - 1] == -1).all() and (want[0][fold == 0, :k - 1] >= 0).all()     # the tail is there
        if n < k or (what != "none" and n <= k):
            assert (want[0][:, -1] == -1).all() and np.isinf(want[1][:, -1]).all()
        _assert_exact(_device(x, x, k, g, g), want, (what, n, d, k))


@pytest.mark.parametrize("k", [1, 15, 64])
def test_all_points_identical_gives_the_smallest_admitted_indices(k):
    n = 300
    x = np.full((n, 5), 3.0, dtype=np.float32)
    idx, dist2 = _device(x, x, k)
    assert np.array_equal(idx, np.tile(np.arange(k), (n, 1))) and not dist2.any()
    idx, dist2 = _device(x, x, k, np.arange(n), np.arange(n))
    want = np.array([[j for j in range(k + 1) if j != i][:k] for i in range(n)])
    assert np.array_equal(idx, want) and not dist2.any()
    fold = np.arange(n) % 3
    idx, _ = _device(x, x, k, fold, fold)
    want = np.array([[j for j in range(2 * k + 2) if j % 3 != i % 3][:k] for i in range(n)])
    assert np.array_equal(idx, want)


@pytest.mark.parametrize("nq,nr", [(7, 1000), (1000, 7)])
def test_queries_against_another_set(nq, nr):
    rng = np.random.default_rng(nq)
    q, r = KR.lattice(nq, 10, seed=1), KR.lattice(nr, 10, seed=2)
    qg, rg = rng.integers(0, 3, nq), rng.integers(0, 3, nr)
    for k in (5, 15):
        _assert_exact(_device(q, r, k), KR.neighbors(q, r, k), (nq, nr, k))
        _assert_exact(_device(q, r, k, qg, rg), KR.neighbors(q, r, k, qg, rg), (nq, nr, k, "groups"))


def test_strided_rows_are_read_where_they_lie():
    wide_q, wide_r = KR.lattice(300, 23, seed=5), KR.lattice(411, 17, seed=6)
    q, r = wide_q[:, 4:14], wide_r[:, 7:17]
    tq, tr = _t(wide_q)[:, 4:14], _t(wide_r)[:, 7:17]
    assert tq.stride(0) == 23 and tr.stride(0) == 17 and not tq.is_contiguous()
    idx, dist2 = NB.knn_device(tq, tr, 15)
    _assert_exact((idx.cpu().numpy(), dist2.cpu().numpy()), KR.neighbors(q, r, 15), "strided")
    i2, d2 = NB.knn(tq, 15, ref=tr)                                       # the public call: device tensors in and out
    assert i2.is_cuda and torch.equal(i2, idx) and np.array_equal(d2.cpu().numpy(), np.sqrt(dist2.cpu().numpy()))


@functools.lru_cache(maxsize=None)
def _float_case(name):
    """(x, labels, k, the restatement's self-excluded neighbours), computed once and left unchanged."""
    x, labels, k = KR.mixture(name)
    own = np.arange(len(x))
    return x, labels, k, KR.neighbors(x, x, k, own, own)


@pytest.mark.parametrize("which", ["lattice", "float"])
def test_result_does_not_depend_on_the_partition(which):
    if which == "lattice":
        n, k = 1000, 15
        x = KR.lattice(n, 10, seed=77)
    else:
        x, _, k, _ = _float_case("n3000_d10_k15")
        x = x[:1000]
        n = 1000
    fold = np.arange(n) % 5
    xd, g = _t(x), _i32(fold)
    base_idx, base_d2 = NB.knn_device(xd, xd, k, g, g)
    for seg in (1, 7, 64, 257, n - 1, n, 0):
        idx, d2 = NB.knn_device(xd, xd, k, g, g, seg_cols=seg)
        assert torch.equal(idx, base_idx) and torch.equal(_bits(d2), _bits(base_d2)), (which, seg)
    rows = np.random.default_rng(3).permutation(n)[:137]                  # a subset of the queries: those rows, bit for bit
    idx, d2 = NB.knn_device(_t(x[rows]), xd, k, _i32(fold[rows]), g)
    sel = torch.from_numpy(rows).to(DEV)
    assert torch.equal(idx, base_idx[sel]) and torch.equal(_bits(d2), _bits(base_d2[sel]))
    idx, d2 = NB.knn_device(xd[400:401], xd, k, g[400:401], g, seg_cols=33)
    assert torch.equal(idx, base_idx[400:401]) and torch.equal(_bits(d2), _bits(base_d2[400:401]))


@pytest.mark.parametrize("name", sorted(KR.FLOAT_CASES))
def test_float_cases_within_the_gate(name):
    x, _, k, (ref_idx, ref_d2, nxt) = _float_case(name)
    n, d = x.shape
    own = np.arange(n)
    idx, dist2 = _device(x, x, k, own, own)
    assert (idx >= 0).all() and (idx < n).all() and (idx != own[:, None]).all()
    assert (np.diff(dist2, axis=1) >= 0).all()                            # every row non-decreasing
    x64 = x.astype(np.float64)
    true = ((x64[:, None, :] - x64[idx]) ** 2).sum(axis=2)                # the float64 squared distance of the pair named
    rel = np.abs(dist2.astype(np.float64) - true) / true
    sure = KR.unambiguous(ref_d2, nxt, d)
    print(f"{name}: worst |dist2 - float64| / float64 = {rel.max() / KR.gamma(d):.3f} of gamma; "
          f"{int((~sure).sum())} of {n} cells ambiguous")
    assert (true > 0).all() and rel.max() <= KR.gamma(d)
    assert (~sure).mean() <= 0.02
    assert np.array_equal(np.sort(idx[sure], axis=1), np.sort(ref_idx[sure], axis=1))
    i2, dist = NB.knn(x, k)                                               # the public call: numpy in and out, sqrt in float32
    assert isinstance(i2, np.ndarray) and np.array_equal(i2, idx) and dist.dtype == np.float32
    assert np.array_equal(dist, np.sqrt(dist2))


def test_votes_and_purity_equal_the_restatement():
    rng = np.random.default_rng(11)
    cases = []
    for n, d, k, K in ((2, 3, 5, 2), (40, 3, 64, 50), (300, 4, 15, 7), (1000, 10, 63, 4096), (257, 5, 1, 3), (500, 2, 8, 8)):
        x = KR.lattice(n, d, seed=n)
        labels = rng.integers(0, K, n)
        if n == 500:
            labels = np.arange(n) % 8                                     # k = 8 neighbours of (mostly) distinct labels: all-tie rows
        fold = _folds(n, k, seed=n)                                       # rows with -1 tails
        cases.append((x, labels, k, K, fold))
    for x, labels, k, K, fold in cases:
        n = len(x)
        for g in (np.arange(n), fold):
            idx, _ = NB.knn_device(_t(x), _t(x), k, _i32(g), _i32(g))
            pred, purity, top2 = NB.knn_votes_device(idx, _i32(labels), K, _i32(labels), top2=True)
            host = idx.cpu().numpy()
            want_pred, want_top2 = KR.votes(host, labels, K)
            want_purity = KR.purity(host, labels, labels)
            assert np.array_equal(pred.cpu().numpy(), want_pred), (n, k)
            assert np.array_equal(top2.cpu().numpy(), want_top2), (n, k)
            assert purity.dtype == torch.float64
            got_purity, nan = purity.cpu().numpy(), np.isnan(want_purity)
            assert np.array_equal(np.isnan(got_purity), nan), (n, k)      # NaN where the restatement's is; the rest bit for bit
            assert np.array_equal(got_purity[~nan].view(np.uint64), want_purity[~nan].view(np.uint64)), (n, k)
            only_pred, none, none2 = NB.knn_votes_device(idx, _i32(labels), K)
            assert none is None and none2 is None and torch.equal(only_pred, pred)
    assert (want_top2[:, 0] == want_top2[:, 1]).any() and (host < 0).any()
    # a row without a valid neighbour: pred -1, purity NaN
    idx = torch.full((3, 4), -1, dtype=torch.int32, device=DEV)
    idx[1, 0] = 2
    pred, purity, _ = NB.knn_votes_device(idx, _i32([0, 1, 1]), 2, _i32([1, 1, 1]))
    assert pred.tolist() == [-1, 1, -1] and np.array_equal(np.isnan(purity.cpu().numpy()), [True, False, True])
    assert float(purity[1]) == 1.0


def test_neighbor_purity_and_graph():
    x, labels, k, (ref_idx, ref_d2, nxt) = _float_case("n3000_d2_k5")
    res = NB.neighbor_purity(x, labels, k)
    idx, _ = NB.knn(x, k)
    want = KR.purity(idx, labels, labels)
    assert np.array_equal(res["cell"], want) and res["mean"] == float(np.mean(want))
    assert np.array_equal(res["classes"], np.unique(labels))
    assert np.array_equal(res["per_class"], [np.mean(want[labels == c]) for c in np.unique(labels)])
    assert 0.5 < res["mean"] <= 1.0
    indptr, indices, data = NB.knn_graph(x, k)
    assert np.array_equal(indptr, k * np.arange(len(x) + 1))
    assert np.array_equal(indices.reshape(-1, k), np.sort(idx, axis=1))
    _, dist = NB.knn(x, k)
    assert np.array_equal(np.sort(data.reshape(-1, k), axis=1), dist)
    _, _, ones = NB.knn_graph(x, k, mode="connectivity")
    assert ones.dtype == np.float32 and (ones == 1.0).all()


@pytest.mark.parametrize("name", ["n3000_d10_k15", "n3000_d2_k5"])
def test_cv_predict_and_classifier(name):
    x, labels, k, _ = _float_case(name)
    kfold, seed = 5, 3
    ref = KR.cv_predict(x, labels, kfold, seed, k)
    sure = ref["sure"]
    assert (~sure).mean() <= 0.02
    got = NB.knn_cv_predict(x, labels, kfold, seed, k=k)
    assert sorted(got) == ["best", "classes", "fold", "kth_distance", "pred", "purity", "second"]
    assert np.array_equal(got["fold"], ref["fold"]) and np.array_equal(got["classes"], ref["classes"])
    assert np.array_equal(got["pred"][sure], ref["pred"][sure])
    assert np.array_equal(got["purity"][sure], ref["purity"][sure])
    assert np.array_equal(got["best"][sure], ref["top2"][sure, 0]) and np.array_equal(got["second"][sure], ref["top2"][sure, 1])
    kth = np.sqrt(ref["dist2"][:, -1])
    assert got["kth_distance"].dtype == np.float32 and np.all(np.abs(got["kth_distance"] - kth) <= KR.gamma(x.shape[1]) * kth)
    names = np.array([f"type{v}" for v in labels])
    acc, ref_labels, pred_labels = NB.KNN_classifier(_t(x), {"codes": labels, "names": names}, kfold, seed, k=k)
    assert sorted(acc) == sorted(ref_labels) == sorted(pred_labels) == ["codes", "names"]
    by_name = NB.knn_cv_predict(x, names, kfold, seed, k=k)               # (a tie goes to the smallest label of ITS encoding)
    for key, y, res in (("codes", labels, got), ("names", names, by_name)):
        assert len(acc[key]) == len(ref_labels[key]) == len(pred_labels[key]) == kfold
        for f in range(kfold):
            test = np.flatnonzero(ref["fold"] == f)
            assert np.array_equal(ref_labels[key][f], y[test])
            assert np.array_equal(pred_labels[key][f], res["classes"][res["pred"][test]])
            assert isinstance(acc[key][f], float) and acc[key][f] == float(np.mean(pred_labels[key][f] == ref_labels[key][f]))
        assert np.mean(acc[key]) > 0.5


def test_two_runs_equal_bits_and_the_allocation_contract(monkeypatch):
    """Plain, then under tests/alloc_guard.py with the fills 0xFF and 0x5A: the workspace and every output come from
    _native._workspace, so guarding _native guards them.  Guards intact; every output bit-equal to the plain run (an element
    the kernels left unwritten would hold the fill, which differs between the two fills and from the plain run)."""
    x, labels, k, _ = _float_case("n3000_d10_k15")
    fold = np.arange(len(x)) % 5
    small = x[:37]                                                        # 37 cells, k = 64 > n: the tails are written too

    def run():
        i1, d1 = NB.knn(x, k, groups=fold)
        i2, d2 = NB.knn(small, 64)
        p = NB.neighbor_purity(x, labels, k)
        return [i1, d1, i2, d2, p["cell"], p["per_class"]]
    plain = run()
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(plain, run()))
    assert (plain[2][:, 36:] == -1).all() and np.isinf(plain[3][:, 36:]).all()
    for fill in (0xFF, 0x5A):
        with guarded(["_native"], fill, monkeypatch=monkeypatch) as g:
            got = run()
            g.check()
            # knn: idx, dist2 and the workspace, twice; neighbor_purity: those three, then pred and purity
            assert len(g.allocs) == 11, g.sites()
            for j, (a, b) in enumerate(zip(plain, got)):
                assert a.shape == b.shape and a.dtype == b.dtype
                assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (hex(fill), j)


def test_trainer_methods_equal_the_module_on_encode_dataset():
    from distributed_vae_amd.cpl_mixvae import cpl_mixVAE
    from distributed_vae_amd.utils.dataloader import DeviceLoader
    Dm, Cc, S, A, n = 64, 6, 2, 2, 512
    t = cpl_mixVAE(saving_folder="", device=0, save_flag=False)
    t.init_model(n_categories=Cc, state_dim=S, input_dim=Dm, fc_dim=32, lowD_dim=6, x_drop=0.5, s_drop=0.2, n_arm=A, temp=1.0,
                 tau=0.005)
    rng = np.random.default_rng(4)
    codes = rng.integers(0, 4, 600)
    data = _t(np.abs(3.0 * rng.standard_normal((4, Dm))[codes] + rng.standard_normal((600, Dm))).astype(np.float32))
    labels = np.array([f"type{v}" for v in codes])                        # one label per row of the data set
    index = torch.from_numpy(rng.permutation(600)[:n])
    dl = DeviceLoader(data, index, 64, False, False)
    enc = t.encode_dataset(dl)
    rows = enc["data_indx"].astype(np.int64)
    assert np.array_equal(rows, index.numpy())
    for on in ("x_low", "state_mu", "z_prob"):
        got = t.latent_neighbors(dl, k=15, arm=1, on=on)
        assert sorted(got) == ["data_indx", "distances", "indices"]
        idx, dist = NB.knn(enc[on][1], 15)
        assert got["indices"].shape == (n, 15) and np.array_equal(got["indices"], idx)
        assert np.array_equal(got["distances"].view(np.uint32), dist.view(np.uint32))
        assert np.array_equal(got["data_indx"].astype(np.int64), rows)
        res = t.classify_neighbors(dl, labels, k=7, kfold=3, seed=1, arm=1, on=on)
        assert sorted(res) == ["acc", "data_indx", "fold", "kth_distance", "margin", "pred_labels", "purity", "ref_labels"]
        want = NB.knn_cv_predict(enc[on][1], labels[rows], 3, 1, k=7)
        assert np.array_equal(res["fold"], want["fold"]) and np.array_equal(res["data_indx"].astype(np.int64), rows)
        assert np.array_equal(res["purity"], want["purity"]) and np.array_equal(res["kth_distance"], want["kth_distance"])
        assert np.array_equal(res["margin"], (want["best"] - want["second"]) / 7.0)
        for f in range(3):
            test = np.flatnonzero(want["fold"] == f)
            assert np.array_equal(res["pred_labels"][f], want["classes"][want["pred"][test]])
            assert np.array_equal(res["ref_labels"][f], labels[rows][test])
            assert res["acc"][f] == float(np.mean(res["pred_labels"][f] == res["ref_labels"][f]))
    with pytest.raises(ValueError):
        t.latent_neighbors(dl, arm=A)
    with pytest.raises(ValueError):
        t.classify_neighbors(dl, labels, on="recon")
    with pytest.raises(ValueError):
        t.latent_neighbors(DeviceLoader(data, index, 60, False, True))     # drop_last with a remainder

"""GPU: the random forest on the device.  mmvae_forest_cv through its wrapper, the public ``quantile_bins`` /
``forest_cv_predict`` / ``RF_classifier`` and ``cpl_mixVAE.classify_forest`` against the numpy restatement of the contract
(tests/forest_restatement.py), on the smallest shapes at which a launch can go wrong (tests/forest_inputs.py, whose properties
tests/test_forest_cpu.py checks), one mid-size case end to end, and sklearn's recorded accuracies
(tests/golden/forest_kat.npz).

Everything the forest computes is an integer or one of two correctly rounded fp64 operations, so every comparison with the
restatement is exact: node tables in every field (feature, threshold, left child, rows; the counts of nodes), labels, the two
vote counts, the votes matrix, and every accuracy to its last bit.  The one gate is the statistical one against sklearn,
|mean accuracy - sklearn's mean over 8 seeds| <= 4 sqrt(2) s (tests/test_forest_cpu.py states it and the measured distances);
the device forest equals the restated one, so that test only makes this file fail loudly on a change of the contract.

Measured on an MI355X: the 33 tests take 6.9 s, the slowest 1.6 s (``classify_forest``: eight encodes and forests), every
edge case 0.3 s or less; the device's accuracies on the four recorded cases are the restatement's, 0.9963, 0.6310, 0.2940 and
0.9330, at distances 0.0004, 0.0015, 0.0041 and 0.0049 from sklearn's means inside gates of 0.0028, 0.0096, 0.0193, 0.0124."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import forest_inputs as FI  # noqa: E402
import forest_restatement as FR  # noqa: E402
from gpu_util import DEV  # noqa: E402
from distributed_vae_amd import _native as N  # noqa: E402
from distributed_vae_amd.utils import cluster_analysis as CA  # noqa: E402

pytestmark = pytest.mark.gpu

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "forest_kat.npz"))
KAT = [tuple(int(v) for v in row) for row in G["cases"]]


def _t(a, dtype=None):
    return torch.from_numpy(np.array(a, dtype=dtype)).to(DEV)                    # a copy: the cached arrays are read-only


def _run(c, bins=None, codes=None, fold=None):
    """(label, best, second, votes, count, nodes) as numpy, from the case's inputs or the ones given."""
    b = _t(c["bins"]) if bins is None else bins
    label, best, second, votes, trees = N.forest_cv(b, _t(c["codes"] if codes is None else codes, np.int32),
                                                    _t(c["fold"] if fold is None else fold, np.int32), c["K"], c["F"], c["T"],
                                                    c["mtry"], c["seed"], return_votes=True, return_trees=True)
    return tuple(v.cpu().numpy() for v in (label, best, second, votes, trees["count"], trees["nodes"]))


def _assert_equals_restatement(got, res):
    label, best, second, votes, count, nodes = got
    want = res["trees"]
    assert count.dtype == np.int32 and np.array_equal(count, want["count"])
    for g, table in enumerate(want["nodes"]):
        assert np.array_equal(nodes[g, :len(table)], table), f"tree {g}"
    assert np.array_equal(votes, res["votes"]) and votes.dtype == np.int32
    assert np.array_equal(label, res["pred"]) and np.array_equal(best, res["best"]) and np.array_equal(second, res["second"])


# ---- 1. every edge case: the device's trees are the restatement's -----------------------------------------------------------
@pytest.mark.parametrize("name", sorted(FI.CASES))
def test_edge_case_equals_restatement(name):
    _assert_equals_restatement(_run(FI.case(name)), FI.restated(name)[0])


def test_row_strided_bins():
    c = FI.case("n65")
    n, d = c["bins"].shape
    wide = torch.full((n, d + 13), 255, dtype=torch.uint8, device=DEV)
    wide[:, 5:5 + d] = _t(c["bins"])
    before = wide.clone()
    _assert_equals_restatement(_run(c, bins=wide[:, 5:5 + d]), FI.restated("n65")[0])
    assert torch.equal(wide, before)


# ---- 2. the same bytes on every run; a fold's trees and a row's votes depend on nothing else -----------------------------------
def test_two_runs_give_the_same_bytes():
    for name in ("Kmax", "clones", "d128"):
        a, b = _run(FI.case(name)), _run(FI.case(name))
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)), name


def test_a_folds_trees_ignore_the_order_of_its_held_out_rows():
    """The held-out rows of fold 1 permuted among themselves: the trees of fold 1, which never see them, are the same bytes,
    and every row takes its votes with it."""
    c = FI.case("absent")                           # three folds
    label, best, second, votes, count, nodes = _run(c)
    mine = np.flatnonzero(c["fold"] == 1)
    src = np.arange(len(c["fold"]))
    src[mine] = np.random.default_rng(4).permutation(mine)
    assert (src != np.arange(len(src))).any()
    l2, b2, s2, v2, count2, nodes2 = _run(c, bins=_t(c["bins"][src]), codes=c["codes"][src])
    T = c["T"]
    assert count2[T:2 * T].tobytes() == count[T:2 * T].tobytes() and nodes2[T:2 * T].tobytes() == nodes[T:2 * T].tobytes()
    assert np.array_equal(l2[mine], label[src[mine]]) and np.array_equal(v2[mine], votes[src[mine]])
    assert np.array_equal(b2[mine], best[src[mine]]) and np.array_equal(s2[mine], second[src[mine]])


def test_a_rows_votes_do_not_depend_on_the_rows_beside_it():
    """A held-out row's bins handed to another held-out row of the same fold: that row now gets exactly the first one's votes,
    and no other row of that fold changes (the fold's trees never see either)."""
    c = FI.case("d2")
    label, best, second, votes, _, _ = _run(c)
    f0 = np.flatnonzero(c["fold"] == 0)
    a, b = int(f0[0]), int(f0[-1])
    bins = np.array(c["bins"])
    bins[b] = bins[a]
    l2, b2, s2, v2, _, _ = _run(c, bins=_t(bins))
    assert np.array_equal(v2[b], votes[a]) and l2[b] == label[a]
    others = f0[:-1]
    assert np.array_equal(v2[others], votes[others]) and np.array_equal(l2[others], label[others])


# ---- 3. the bins ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 255, 256, 257, 1000])
def test_quantile_bins_equal_the_hosts(n):
    rng = np.random.default_rng(n)
    x = rng.normal(size=(n, 4)).astype(np.float32)
    x[:, 1] = np.round(x[:, 1] * 2.0) / 2.0                     # ties
    x[: n // 2, 2] = np.where(np.arange(n // 2) % 2 == 0, 0.0, -0.0)
    x[:, 3] = 1.5                                               # one value
    want = FR.quantile_bins(x)
    got = CA.quantile_bins(x)
    assert got.dtype == torch.uint8 and got.device.type == "cuda" and np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(CA.quantile_bins(_t(x)).cpu().numpy(), want)                      # a device tensor
    assert np.array_equal(CA.quantile_bins(x.astype(np.float64)).cpu().numpy(), want)       # float64 of float32 values
    with pytest.raises(ValueError, match="NaN or infinity"):
        CA.quantile_bins(_t(np.where(np.arange(4 * n).reshape(n, 4) == 5, np.nan, x).astype(np.float32)))


# ---- 4. the public entries, end to end on one mid-size case --------------------------------------------------------------------
MID = dict(n=1500, d=10, K=12, kfold=3, seed=5, n_trees=20)


def _mid():
    x, codes = FI.points(MID["n"], MID["d"], MID["K"], seed=2, spread=1.5)
    return np.array(x), {"T": np.array([f"t{v:02d}" for v in codes]), "merged": np.array(codes) % 4}


def test_forest_cv_predict_equals_the_restatement():
    x, labels = _mid()
    want = FR.cv_predict(x, labels["T"], MID["kfold"], MID["seed"], n_trees=MID["n_trees"], want_trees=True)
    got = CA.forest_cv_predict(x, labels["T"], MID["kfold"], MID["seed"], n_trees=MID["n_trees"], return_votes=True,
                               return_trees=True)
    assert sorted(got) == ["best", "classes", "fold", "pred", "second", "trees", "votes"]
    assert got["pred"].dtype == np.int64 and got["classes"].dtype.kind == "U" and np.array_equal(got["classes"], want["classes"])
    assert np.array_equal(got["fold"], want["fold"])
    _assert_equals_restatement((got["pred"], got["best"], got["second"], got["votes"], got["trees"]["count"], got["trees"]["nodes"]),
                               want)
    assert 0.5 < float(np.mean(got["pred"] == np.unique(labels["T"], return_inverse=True)[1])) < 1.0
    # float64 input of float32 values, a device tensor used where it lies, and another forest seed
    wide = torch.full((MID["n"], MID["d"] + 3), 1e30, device=DEV)
    wide[:, 1:1 + MID["d"]] = _t(x)
    before = wide.clone()
    for other in (x.astype(np.float64), wide[:, 1:1 + MID["d"]]):
        again = CA.forest_cv_predict(other, labels["T"], MID["kfold"], MID["seed"], n_trees=MID["n_trees"], return_votes=True)
        assert np.array_equal(again["votes"], got["votes"]) and np.array_equal(again["pred"], got["pred"])
    assert torch.equal(wide, before)
    reseeded = CA.forest_cv_predict(x, labels["T"], MID["kfold"], MID["seed"], n_trees=MID["n_trees"], forest_seed=99, max_features=3,
                                    return_votes=True)
    want2 = FR.cv_predict(x, labels["T"], MID["kfold"], MID["seed"], n_trees=MID["n_trees"], mtry=3, forest_seed=99)
    assert np.array_equal(reseeded["fold"], got["fold"]) and not np.array_equal(reseeded["votes"], got["votes"])
    assert np.array_equal(reseeded["votes"], want2["votes"])


def test_rf_classifier_equals_the_restatement(monkeypatch):
    x, labels = _mid()
    monkeypatch.setattr(CA, "FOREST_TREES", MID["n_trees"])
    uploads, binnings = [], []
    upload, binning = CA._points_on_device, CA._bins_on_device
    monkeypatch.setattr(CA, "_points_on_device", lambda *a: uploads.append(1) or upload(*a))
    monkeypatch.setattr(CA, "_bins_on_device", lambda *a: binnings.append(1) or binning(*a))
    acc, ref, pred = CA.RF_classifier(x, labels, MID["kfold"], MID["seed"])
    assert len(uploads) == len(binnings) == 1                   # two label sets: uploaded and binned once
    want_acc, want_ref, want_pred = FR.classifier(x, labels, MID["kfold"], MID["seed"], n_trees=MID["n_trees"])
    assert list(acc) == list(ref) == list(pred) == list(labels)
    for key in labels:
        assert len(acc[key]) == len(ref[key]) == len(pred[key]) == MID["kfold"]
        assert all(type(a) is float for a in acc[key]) and acc[key] == want_acc[key]            # to the last bit
        for f in range(MID["kfold"]):
            assert pred[key][f].dtype == labels[key].dtype and np.array_equal(pred[key][f], want_pred[key][f])
            assert np.array_equal(ref[key][f], want_ref[key][f])
        print(f"RF_classifier {key}: accuracies {acc[key]}")
    dev_acc, _, dev_pred = CA.RF_classifier(_t(x), labels, MID["kfold"], MID["seed"])         # a float32 device tensor
    assert dev_acc == acc and all(np.array_equal(a, b) for a, b in zip(dev_pred["T"], pred["T"]))


# ---- 5. cpl_mixVAE.classify_forest ----------------------------------------------------------------------------------------------
def test_classify_forest_equals_forest_cv_predict(monkeypatch):
    from torch.utils.data import DataLoader, TensorDataset
    from distributed_vae_amd.cpl_mixvae import cpl_mixVAE
    from distributed_vae_amd.utils.dataloader import DeviceLoader
    from distributed_vae_amd.utils.pca import pca_project
    Dm, Cc, S, A, n, T = 40, 5, 2, 2, 300, 10
    t = cpl_mixVAE(saving_folder="", device=0, save_flag=False)
    t.init_model(n_categories=Cc, state_dim=S, input_dim=Dm, fc_dim=32, lowD_dim=6, x_drop=0.5, s_drop=0.2, n_arm=A, temp=1.0,
                 tau=0.005)
    x, codes = FI.points(400, Dm, 4, seed=9, spread=1.0)
    data = _t(np.abs(x))
    labels = np.array([f"type{v}" for v in codes])                                # one label per row of the data set
    index = torch.from_numpy(np.random.default_rng(2).permutation(400)[:n])
    resident = DeviceLoader(data, index, 64, False, False)
    plain = DataLoader(TensorDataset(data[index].cpu(), index.to(torch.float32)), batch_size=64, shuffle=False)
    enc = t.encode_dataset(resident)
    rows = enc["data_indx"].astype(np.int64)
    assert np.array_equal(rows, index.numpy())

    def same(got, want):
        assert sorted(got) == ["acc", "data_indx", "fold", "margin", "pred_labels", "ref_labels"]
        assert np.array_equal(got["fold"], want["fold"]) and np.array_equal(got["data_indx"].astype(np.int64), rows)
        assert got["margin"].dtype == np.float64 and np.array_equal(got["margin"], (want["best"] - want["second"]) / float(T))
        assert len(got["acc"]) == len(got["pred_labels"]) == len(got["ref_labels"]) == 3
        for f in range(3):
            test = np.flatnonzero(want["fold"] == f)
            assert np.array_equal(got["pred_labels"][f], want["classes"][want["pred"][test]])
            assert np.array_equal(got["ref_labels"][f], labels[rows][test])
            assert got["acc"][f] == float(np.mean(got["pred_labels"][f] == got["ref_labels"][f]))

    for on in ("x_low", "state_mu", "z_prob"):
        want = CA.forest_cv_predict(enc[on][1], labels[rows], 3, 1, n_trees=T)
        for dl in (resident, plain):
            same(t.classify_forest(dl, labels, kfold=3, seed=1, arm=1, on=on, n_trees=T), want)
    z = pca_project(data, 4, rows=index.to(DEV), out="device")
    want = CA.forest_cv_predict(z, labels[rows], 3, 1, n_trees=T)
    for dl in (resident, plain):
        same(t.classify_forest(dl, labels, kfold=3, seed=1, on="pcs", n_trees=T, num_pc=4), want)
    # the refusals of classify_latents
    with pytest.raises(ValueError, match="arm"):
        t.classify_forest(resident, labels, arm=A)
    with pytest.raises(ValueError, match="on ="):
        t.classify_forest(resident, labels, on="recon")
    with pytest.raises(ValueError, match="every row once"):
        t.classify_forest(DeviceLoader(data, index, 64, False, True), labels)    # drop_last with a remainder
    with pytest.raises(ValueError, match="kind"):
        t.classify_latents(resident, labels, kind="rf")                           # classify_latents keeps its two kinds
    monkeypatch.setattr(CA.D, "is_dist", lambda: True)
    with pytest.raises(NotImplementedError, match="not data-parallel"):
        t.classify_forest(resident, labels)


# ---- 6. against sklearn's recorded accuracies ----------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(4))
def test_device_forest_is_within_sklearns_spread(k):
    n, d, kfold, seed = KAT[k]
    x, y = G[f"c{k}/x"], G[f"c{k}/y"]
    acc, _, _ = CA.RF_classifier(x, {"y": y}, kfold, seed)
    m = G[f"c{k}/acc"].mean(axis=1)
    theirs, gate = float(m.mean()), 4.0 * np.sqrt(2.0) * float(m.std(ddof=1))
    mine = float(np.mean(acc["y"]))
    print(f"c{k}: device {mine:.4f}, sklearn {theirs:.4f}, distance {abs(mine - theirs):.4f}, gate {gate:.4f}")
    assert abs(mine - theirs) <= gate

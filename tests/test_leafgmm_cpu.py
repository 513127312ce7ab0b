"""The tree-based analysis without a GPU: tests/leafgmm_restatement.py against every return of the reference recorded in
tests/golden/leafgmm_kat.npz (tools/gen_golden_leafgmm.py), the package's tree helpers against the recorded merge sequences and
on edge trees, the model builder's branches, and every refusal of the new public functions that is decided before device work.

Probabilities: |restatement - reference| <= the case's recorded e_ref + 64 x 2^-53 (the recorded distance is the fixture's own
measurement on the build machine; the margin covers another numpy's exp and eigh).  Labels, counts and merge sequences: exact."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import leafgmm_restatement as LR  # noqa: E402
from distributed_vae_amd import _native as N  # noqa: E402
from distributed_vae_amd import dist as D  # noqa: E402
from distributed_vae_amd.utils import analysis_tree_helpers as TH  # noqa: E402

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "leafgmm_kat.npz"))
KINDS = [str(v) for v in G["kinds"]]
SETS = [(k, int(m)) for k in range(len(KINDS)) for m in G[f"c{k}/levels"]]


def _case(k):
    w = G[f"c{k}/weight"]
    return (G[f"c{k}/train_z"].astype(np.float64), G[f"c{k}/train_lbl"], G[f"c{k}/test_z"].astype(np.float64), G[f"c{k}/test_lbl"],
            G[f"c{k}/leaves"], w if len(w) else None)


def test_the_fixture_covers_what_it_should():
    assert KINDS == ["plain12", "weights10", "nested2", "simplex10", "wide2", "far10"]
    assert sorted({int(c[2]) for c in G["cases"]}) == [2, 10, 12] and {int(c[3]) for c in G["cases"]} >= {6, 40}
    acc = [float(G[f"c{k}/leaf_acc"]) for k in range(len(KINDS))]
    assert 2 * sum(0.5 < a < 0.99 for a in acc) >= len(acc)
    assert all(float(G[f"c{k}/min_margin"]) >= 1e-6 for k in range(len(KINDS)))
    far = KINDS.index("far10")
    for k, m in SETS:
        assert (len(G[f"c{k}/m{m}/nan_rows"]) > 0) == (k == far)
    for k in range(len(KINDS)):                                                    # a leaf without a model, a diagonal leaf
        cnt = np.array([(G[f"c{k}/train_lbl"] == leaf).sum() for leaf in G[f"c{k}/leaves"]])
        assert (cnt <= 6).any() and ((cnt >= 7) & (cnt <= 11)).any()
        assert int(G[f"c{k}/m0/counts"][0]) > 0 and int(G[f"c{k}/m0/counts"][2]) == 1
    nested = KINDS.index("nested2")
    assert "ghost" in G[f"c{nested}/m-1/dataset"] and "X34" in G[f"c{nested}/m-1/dataset"] and "L03" in G[f"c{nested}/m-1/dataset"]


@pytest.mark.parametrize("k,m", SETS, ids=[f"{KINDS[k]}-m{m}" for k, m in SETS])
def test_restatement_equals_the_recorded_reference(k, m):
    tr, ltr, te, lte, leaves, w = _case(k)
    base = f"c{k}/m{m}"
    res = LR.predict_leaf_gmm(tr, ltr, te, lte, 6, 12, G[f"{base}/dataset"], leaves, json.loads(str(G[f"{base}/desc"])), w)
    assert [res["n_excluded"], res["n_predicted"], res["n_removed"]] == list(G[f"{base}/counts"])
    assert np.array_equal(res["true"], G[f"{base}/true"])
    ok = ~np.isnan(G[f"{base}/prob"])
    assert np.array_equal(np.flatnonzero(~ok), G[f"{base}/nan_rows"])
    assert np.array_equal(res["pred"][ok], G[f"{base}/pred"][ok])
    err = np.abs(res["prob"][ok] - G[f"{base}/prob"][ok])
    assert (err <= float(G[f"c{k}/e_ref"]) + 64 * LR.U).all(), err.max()
    if (~ok).any():                            # where the reference is 0 / 0 the log-domain posterior is finite, and recorded
        assert np.isfinite(res["prob"]).all()
        assert np.array_equal(res["pred"][~ok], G[f"{base}/far_pred"])
        assert np.allclose(res["prob"][~ok], G[f"{base}/far_prob"], rtol=1e-9, atol=0)


def test_restated_custom_qda_equals_the_recorded_reference():
    true, pred, _ = LR.custom_qda(G["qda/train_z"].astype(np.float64), G["qda/train_lbl"], G["qda/test_z"].astype(np.float64),
                                  G["qda/test_lbl"])
    assert np.array_equal(pred, G["qda/pred"]) and np.array_equal(true, G["qda/true"])
    cnt = np.array([(G["qda/train_lbl"] == c).sum() for c in np.unique(G["qda/train_lbl"])])
    assert ((cnt >= 7) & (cnt <= 11)).any() and (cnt > 6).all()


# ---- the tree helpers -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(KINDS)), ids=KINDS)
def test_tree_helpers_equal_the_recorded_reference(k):
    child, parent, y = G[f"c{k}/tree/child"], G[f"c{k}/tree/parent"], G[f"c{k}/tree/y"]
    leaves = G[f"c{k}/leaves"]
    changes = json.loads(str(G[f"c{k}/changes"]))
    y_before = y.copy()
    for mod in (TH, LR):
        assert json.loads(json.dumps(mod.get_merge_sequence(child, parent, y))) == changes
        assert np.array_equal(y, y_before)                                          # the caller's heights are left alone
    assert any(len(c[0]) == 3 for c in changes) and changes[-1][1] == "n1" and changes[-1][2] == 1
    for node, want in json.loads(str(G[f"c{k}/descendants"])).items():
        assert TH.get_descendants(child, parent, y, node) == want == LR.get_descendants(child, parent, y, node)
    for node, want in json.loads(str(G[f"c{k}/leafonly"])).items():
        assert sorted(TH.get_descendants(child, parent, y, node, leafonly=True)) == want
    for leaf, want in json.loads(str(G[f"c{k}/ancestors"])).items():
        assert [str(a) for a in TH.get_ancestors(leaf, child, parent)] == want
    for m in G[f"c{k}/levels"]:
        if m < 0:
            continue
        before = leaves.copy()
        got = TH.do_merges(leaves, changes, int(m))
        assert np.array_equal(got, G[f"c{k}/merged/{m}"]) and np.array_equal(leaves, before)
        assert np.array_equal(TH.labels_at(leaves, changes, int(m)), np.unique(G[f"c{k}/merged/{m}"]))
        assert np.array_equal(TH.labels_at(leaves, changes, int(m)), G[f"c{k}/m{m}/dataset"])
        assert TH.descendants_at(changes, int(m)) == json.loads(str(G[f"c{k}/m{m}/desc"]))


def test_edge_trees():
    # a single merge
    child, parent, y = np.array(["a", "b", "n1"]), np.array(["n1", "n1", ""]), np.array([0.0, 0.0, 0.5])
    assert TH.get_merge_sequence(child, parent, y) == [[["a", "b"], "n1", 1]]
    assert TH.get_ancestors("a", child, parent) == ["n1"] and TH.get_ancestors("n1", child, parent) == []
    # a node with three children under a root with two
    child = np.array(["a", "b", "c", "d", "n2", "n1"])
    parent = np.array(["n2", "n2", "n2", "n1", "n1", ""])
    y = np.array([np.nan, np.nan, np.nan, np.nan, 0.2, 0.7])                         # NaN heights mark leaves as zeros do
    ch = TH.get_merge_sequence(child, parent, y)
    assert ch == [[["a", "b", "c"], "n2", 3], [["d", "n2"], "n1", 1]]
    assert TH.get_descendants(child, parent, y, "n1") == ["d", "n2", "a", "b", "c"]
    assert sorted(TH.get_descendants(child, parent, y, "n1", leafonly=True)) == ["a", "b", "c", "d"]
    assert TH.get_ancestors("b", child, parent) == ["n2", "n1"]
    assert list(TH.do_merges(np.array(["a", "d", "c"]), ch, 1)) == ["n2", "d", "n2"]
    assert list(TH.labels_at(["a", "b", "c", "d"], ch, 0)) == ["a", "b", "c", "d"]
    assert list(TH.labels_at(["a", "b", "c", "d"], ch, 1)) == ["d", "n2"] and list(TH.labels_at(["a", "b", "c", "d"], ch, 2)) == ["n1"]
    assert TH.descendants_at(ch, 1) == {"n2": ["a", "b", "c"]} and TH.descendants_at(ch, 2) == {"n1": ["d", "n2", "a", "b", "c"]}
    # equal heights: the first row of the two merges first
    child = np.array(["a", "b", "c", "d", "n3", "n2", "n1"])
    parent = np.array(["n3", "n3", "n2", "n2", "n1", "n1", ""])
    y = np.array([0.0, 0.0, 0.0, 0.0, 0.3, 0.3, 0.9])
    assert [c[1] for c in TH.get_merge_sequence(child, parent, y)] == ["n3", "n2", "n1"]
    # a parent's name longer than the labels' width is kept whole, and more merges than there are print a note
    wide = TH.do_merges(np.array(["a", "b"]), [[["a", "b"], "node_17", 1]], 5)
    assert list(wide) == ["node_17", "node_17"]
    with pytest.raises(ValueError):
        TH.get_ancestors("zz", child, parent)


def test_parse_dend(tmp_path):
    pd = pytest.importorskip("pandas")
    k = KINDS.index("nested2")
    child, parent, y = G[f"c{k}/tree/child"], G[f"c{k}/tree/parent"], G[f"c{k}/tree/y"]
    leaf = np.isin(child, G[f"c{k}/leaves"])
    rng = np.random.default_rng(1)
    order = rng.permutation(len(child))                                              # the file's rows in any order
    x = np.arange(len(child), dtype=np.float64)                                      # ties in y are broken by x: keep the order
    frame = pd.DataFrame({"x": x, "y": y, "leaf": np.where(leaf, True, np.nan), "label": child,
                          "parent": np.where(parent == "", np.nan, parent.astype(object)), "col": "#000000"}).iloc[order]
    path = tmp_path / "dend.csv"
    frame.to_csv(path, index=False)
    changes, desc, treeobj, leaves, ch, pa = TH.parse_dend(str(path))
    assert json.loads(json.dumps(changes)) == json.loads(str(G[f"c{k}/changes"]))
    assert sorted(leaves) == sorted(G[f"c{k}/leaves"]) and list(treeobj.columns) == ["x", "y", "leaf", "label", "parent", "col"]
    want = json.loads(str(G[f"c{k}/descendants"]))
    assert all(desc[node] == want[node] for node in want) and all(desc[str(l)] == [] for l in leaves)
    assert np.isnan(treeobj["y"].values[treeobj["leaf"].values]).all()


# ---- the model builder ------------------------------------------------------------------------------------------------------
def _moments(x, codes, L, pivot):
    d = x.shape[1]
    iu = np.triu_indices(d)
    s, M, cnt = np.zeros((L, 1, d)), np.zeros((L, 1, len(iu[0]))), np.zeros((L, 1))
    for k in range(L):
        t = x[codes == k] - pivot
        s[k, 0], M[k, 0], cnt[k, 0] = t.sum(axis=0), (t.T @ t)[iu], len(t)
    return s, M, cnt


def test_model_builder_branches_at_the_thresholds():
    rng = np.random.default_rng(5)
    sizes = [6, 7, 11, 12, 40]
    d = 3
    codes = np.repeat(np.arange(len(sizes)), sizes)
    x = np.round(rng.normal(size=(len(codes), d)) * 4096) / 4096 + codes[:, None]
    leaves = np.array(["a", "b", "c", "d", "e"])
    pivot = x.mean(axis=0)
    w = np.array([1.0, 2.0, 0.5, 0.0, 3.0])
    with np.errstate(divide="ignore"):
        mu, W, c0, train = TH.models_from_leaf_moments(*_moments(x, codes, 5, pivot), pivot, np.log(w), 6, 12, 1e-4)
    ref = LR.leaf_models(x, leaves[codes], leaves, 6, 12, 1e-4, w)
    assert list(train[0]) == sizes
    assert np.isneginf(c0[0, 0]) and np.isneginf(c0[0, 3]) and np.isfinite(c0[0, [1, 2, 4]]).all()      # 6: no model; weight 0
    assert np.allclose(c0[0, [1, 2, 4]], ref["c0"][[1, 2, 4]], rtol=1e-12) and np.allclose(mu[0, 1:], ref["mu"][1:], atol=1e-13)
    for k in (1, 2):                                                                 # 7 and 11 cells: the diagonal alone
        P = W[0, k] @ W[0, k].T
        assert np.count_nonzero(P - np.diag(np.diag(P))) == 0
    with np.errstate(divide="ignore"):
        mu, W, c0, _ = TH.models_from_leaf_moments(*_moments(x, codes, 5, pivot), pivot, np.zeros(5), 6, 12, 1e-4)
    P = W[0, 3] @ W[0, 3].T                                                          # 12 cells: the full covariance
    assert np.count_nonzero(P - np.diag(np.diag(P))) > 0
    t = x[codes == 3] - x[codes == 3].mean(axis=0)
    assert np.allclose(np.linalg.inv(P), t.T @ t / 11.0 + 1e-4 * np.eye(d), rtol=1e-9)
    # folds: the model of fold f is fitted to the other folds' cells
    fold = np.arange(len(codes)) % 3
    iu = np.triu_indices(d)
    s, M, cnt = np.zeros((5, 3, d)), np.zeros((5, 3, 6)), np.zeros((5, 3))
    for k in range(5):
        for f in range(3):
            t = x[(codes == k) & (fold == f)] - pivot
            s[k, f], M[k, f], cnt[k, f] = t.sum(axis=0), (t.T @ t)[iu], len(t)
    mu, W, c0, train = TH.models_from_leaf_moments(s, M, cnt, pivot, np.zeros(5), 6, 12, 1e-4)
    for f in range(3):
        ref = LR.leaf_models(x[fold != f], leaves[codes[fold != f]], leaves, 6, 12, 1e-4)
        assert list(train[f]) == list(ref["counts"]) and np.array_equal(np.isneginf(c0[f]), np.isneginf(ref["c0"]))
        have = np.isfinite(ref["c0"])
        assert np.allclose(c0[f][have], ref["c0"][have], rtol=1e-11) and np.allclose(mu[f][have], ref["mu"][have], atol=1e-12)
    # a singular covariance names the label
    flat = x.copy()
    flat[:, 2] = 1.0
    with pytest.raises(ValueError, match="custom_QDA: the covariance of label 'b' is singular"):
        TH.models_from_leaf_moments(*_moments(flat, codes, 5, pivot), pivot, np.zeros(5), 6, 12, 0.0, "custom_QDA", leaves)


def test_merge_tables():
    ls, st, lf = N.merge_tables([[[0], [1, 2], []], [[0, 1, 2]]])
    assert ls.dtype == st.dtype == lf.dtype == np.int32
    assert list(ls) == [0, 3, 4] and list(st) == [0, 1, 3, 3, 6] and list(lf) == [0, 1, 2, 0, 1, 2]


# ---- refusals decided before any device work ----------------------------------------------------------------------------
def _inputs(n=40, d=3, L=4):
    rng = np.random.default_rng(0)
    leaves = np.array([f"t{i}" for i in range(L)])
    lbl = leaves[np.arange(n) % L]
    return rng.normal(size=(n, d)).astype(np.float32), lbl, rng.normal(size=(10, d)).astype(np.float32), lbl[:10], leaves


def test_predict_leaf_gmm_refusals():
    tr, ltr, te, lte, leaves = _inputs()
    kw = dict(unique_dataset_lbl=leaves.tolist(), unique_leaf_lbl=leaves.tolist())
    with pytest.raises(NotImplementedError, match="d = 129"):
        TH.predict_leaf_gmm(np.zeros((40, 129), np.float32), ltr, np.zeros((10, 129), np.float32), lte, **kw)
    with pytest.raises(NotImplementedError, match="d = 0"):
        TH.predict_leaf_gmm(np.zeros((40, 0), np.float32), ltr, np.zeros((10, 0), np.float32), lte, **kw)
    with pytest.raises(NotImplementedError, match="leaves"):
        TH.predict_leaf_gmm(tr, ltr, te, lte, unique_dataset_lbl=["a"], unique_leaf_lbl=np.arange(4097))
    with pytest.raises(NotImplementedError, match="labels"):
        TH.predict_leaf_gmm(tr, ltr, te, lte, unique_dataset_lbl=[f"x{i}" for i in range(4097)], unique_leaf_lbl=leaves,
                            descendant_dict={"x0": ["t0"]})
    with pytest.raises(ValueError, match="columns"):
        TH.predict_leaf_gmm(tr, ltr, te[:, :2], lte, **kw)
    with pytest.raises(ValueError, match="true_train_lbl"):
        TH.predict_leaf_gmm(tr, ltr[:-1], te, lte, **kw)
    with pytest.raises(ValueError, match="true_test_lbl"):
        TH.predict_leaf_gmm(tr, ltr, te, lte[:-1], **kw)
    with pytest.raises(ValueError, match="not \\[n, d\\]"):
        TH.predict_leaf_gmm(tr[0], ltr, te, lte, **kw)
    with pytest.raises(ValueError, match="unique_leaf_lbl is empty"):
        TH.predict_leaf_gmm(tr, ltr, te, lte, unique_dataset_lbl=leaves.tolist())
    with pytest.raises(ValueError, match="unique_dataset_lbl should not be empty if descendant_dict is provided"):
        TH.predict_leaf_gmm(tr, ltr, te, lte, unique_leaf_lbl=leaves, descendant_dict={"n1": ["t0", "t1"]})
    with pytest.raises(ValueError, match="unique_dataset_lbl should not be empty"):
        TH.predict_leaf_gmm(tr, ltr, te, lte, unique_leaf_lbl=leaves)
    with pytest.raises(ValueError, match="is no leaf"):                               # where the reference stops in pdb
        TH.predict_leaf_gmm(tr, ltr, te, lte, unique_dataset_lbl=["t0", "n9"], unique_leaf_lbl=leaves)
    for bad in ([1.0, -1.0, 1.0, 1.0], [1.0, np.nan, 1.0, 1.0], [1.0, np.inf, 1.0, 1.0], [1.0, 1.0]):
        with pytest.raises(ValueError, match="weights"):
            TH.predict_leaf_gmm(tr, ltr, te, lte, label_weight=bad, **kw)
    with pytest.raises(ValueError, match="n_per_class_thr"):
        TH.predict_leaf_gmm(tr, ltr, te, lte, n_per_class_thr=0, **kw)
    nan = tr.copy()
    nan[3, 1] = np.nan
    with pytest.raises(ValueError, match="NaN or infinity"):
        TH.predict_leaf_gmm(nan, ltr, te, lte, **kw)


def test_the_other_public_functions_refuse_before_device_work(monkeypatch):
    tr, ltr, te, lte, leaves = _inputs()
    changes = [[["t0", "t1"], "n3", 5], [["t2", "t3"], "n2", 3], [["n3", "n2"], "n1", 1]]
    with pytest.raises(ValueError, match="true_test_lbl is needed"):
        TH.custom_QDA(tr, ltr, te, None)
    with pytest.raises(NotImplementedError, match="d = 200"):
        TH.custom_QDA(np.zeros((40, 200), np.float32), ltr, np.zeros((10, 200), np.float32), lte)
    with pytest.raises(ValueError, match="true_test_lbl"):
        TH.custom_QDA(tr, ltr, te, lte[:3])
    with pytest.raises(ValueError, match="levels"):
        TH.merge_sweep(tr, ltr, te, lte, changes, leaves, levels=[0, 4])
    with pytest.raises(ValueError, match="levels"):
        TH.merge_sweep(tr, ltr, te, lte, changes, leaves, levels=[])
    with pytest.raises(ValueError, match="true_test_lbl is needed"):
        TH.merge_sweep(tr, ltr, te, None, changes, leaves)
    with pytest.raises(TypeError, match="unexpected"):
        TH.merge_sweep(tr, ltr, te, lte, changes, leaves, reg=0.0)
    with pytest.raises(ValueError, match="weights"):
        TH.merge_sweep(tr, ltr, te, lte, changes, leaves, label_weight=[1.0, 2.0])
    with pytest.raises(NotImplementedError, match="d = 129"):
        TH.merge_sweep(np.zeros((40, 129), np.float32), ltr, np.zeros((10, 129), np.float32), lte, changes, leaves)
    with pytest.raises(ValueError, match="fold"):
        TH.leaf_gaussians(tr, ltr, leaves, fold=np.zeros(39, dtype=np.int64))
    with pytest.raises(ValueError, match="fold"):
        TH.leaf_gaussians(tr, ltr, leaves, fold=np.full(40, 0.5))
    with pytest.raises(NotImplementedError, match="folds"):
        TH.leaf_gaussians(tr, ltr, leaves, fold=np.arange(40) * 2)
    with pytest.raises(ValueError, match="weights"):
        TH.leaf_gaussians(tr, ltr, leaves, label_weight=[-1.0, 1.0, 1.0, 1.0])
    x = torch.from_numpy(tr)                                                         # refused before the tensor is touched
    for kfold in (1, 41, 2.5):
        with pytest.raises(ValueError, match="kfold"):
            TH.classify_tree_points(x, ltr, changes, leaves, kfold, 0)
    with pytest.raises(NotImplementedError, match="folds"):
        TH.classify_tree_points(torch.zeros(100, 3), np.arange(100) % 4, changes, leaves, 65, 0)
    with pytest.raises(ValueError, match="labels"):
        TH.classify_tree_points(x, ltr[:-1], changes, leaves, 5, 0)
    with pytest.raises(ValueError, match="levels"):
        TH.classify_tree_points(x, ltr, changes, leaves, 5, 0, levels=[7])
    for bad in ((np.zeros((2, 2), np.float32), [0, 1, 2], [0, 1], [0]), (np.zeros((2, 2)), [0, 1], [0, 1], [0])):
        with pytest.raises((TypeError, N.NativeError)):                              # a host tensor, a wrong dtype
            N.leaf_merge(torch.from_numpy(bad[0]), *bad[1:])
    monkeypatch.setattr(D, "is_dist", lambda: True)
    for call in (lambda: TH.predict_leaf_gmm(tr, ltr, te, lte, unique_dataset_lbl=leaves, unique_leaf_lbl=leaves),
                 lambda: TH.custom_QDA(tr, ltr, te, lte), lambda: TH.merge_sweep(tr, ltr, te, lte, changes, leaves),
                 lambda: TH.leaf_gaussians(tr, ltr, leaves)):
        with pytest.raises(NotImplementedError, match="not data-parallel"):
            call()

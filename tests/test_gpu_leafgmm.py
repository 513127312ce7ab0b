"""``mmvae_leaf_merge`` (csrc/leafmerge.hip) and, on it, ``predict_leaf_gmm`` / ``custom_QDA`` / ``merge_sweep`` /
``cpl_mixVAE.classify_tree`` against the numpy fp64 restatement (tests/leafgmm_restatement.py) and the reference's returns
recorded in tests/golden/leafgmm_kat.npz.

Bounds (derived in include/mmvae.h and DESIGN.md section 9j, not tuned; u = 2^-53).
  Posteriors on the same scores: ``tolerance_posteriors``, (2 L + 12) u p + 2^-1070 -- both sides form s - max alike, so the exp
  (1 ulp a side), the L-term sum and the division are all that differ.
  Given the device's own posteriors read back, every merged sum, ``prob``, ``second`` and ``label`` are numpy's sequential sums
  and ``np.argmax``, BIT FOR BIT.
  The whole path on the fixture (device moments, host eigh, device scores, device merge) against the restatement:
  ``tolerance_scores`` (the first-order bound of the Gaussian classifiers, section 9f) carried through the softmax
  (``tolerance_path``) and the sums (``tolerance_merged``); against the recorded reference the case's e_ref is added.
  Predicted labels, counts and ``n_excluded_cells``: exact.

Bit-equality claims tested here: level t of a multi-level call and the one-level call; two runs; a cell alone and the same cell
in a batch; a padded matrix (ldp > L) and its padding left alone; every level of ``merge_sweep`` and ``predict_leaf_gmm`` for
that level.

Measured on an MI355X, worst error over gate: posteriors on synthetic scores 0.117; the whole path on the fixture 1.5e-3
(absolute 1.3e-12 at 40 leaves); ``classify_tree`` 4.0e-4 to 4.6e-4; against the reference's recorded probabilities at most 1.7e-12
absolute.  No cell was excused anywhere."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gaussclf_inputs as GI  # noqa: E402
import leafgmm_restatement as LR  # noqa: E402
from gpu_util import DEV  # noqa: E402
from distributed_vae_amd import _native as N  # noqa: E402
from distributed_vae_amd.utils import analysis_tree_helpers as TH  # noqa: E402
from distributed_vae_amd.utils.cluster_analysis import kfold_of  # noqa: E402

pytestmark = pytest.mark.gpu

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "leafgmm_kat.npz"))
KINDS = [str(v) for v in G["kinds"]]
SETS = [(k, int(m)) for k in range(len(KINDS)) for m in G[f"c{k}/levels"]]
NS, LS = (1, 63, 64, 65, 130), (1, 2, 63, 64, 65, 257)


def _bits(a, b):
    a, b = (v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v) for v in (a, b))
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- leaf_merge alone -----------------------------------------------------------------------------------------------------
def make_scores(n, L, seed):
    """Score rows [n, L]: plain rows of spread 30, -inf columns, and by row index (where there are that many rows) 0: all
    -inf; 1: a spread above 745 (every e but the largest underflows to exact 0 or a denormal); 2, 3: rows near +1e5 and
    -1e5 (the maximum has to come off first); 4: one finite score among -inf."""
    rng = np.random.default_rng(seed)
    s = rng.normal(size=(n, L)) * 30.0
    if L > 2:
        s[:, rng.choice(L, size=max(1, L // 8), replace=False)] = -np.inf
    if n > 1:
        s[1] = -750.0 - rng.uniform(0, 400, size=L)
        s[1, L // 2] = 3.0
        if L > 1:
            s[1, 0] = 3.0 - 720.0                                   # e = exp(-720): a denormal
    if n > 3:
        s[2] = 1e5 + rng.normal(size=L) * 3.0
        s[3] = -1e5 + rng.normal(size=L) * 3.0
    if n > 4:
        s[4] = -np.inf
        s[4, L - 1] = -12.5
    s[0] = -np.inf                                                  # (n = 1: the only row is the degenerate one)
    return s


def make_levels(L, T):
    """T = 1: one level with an empty list, a list of all leaves, two overlapping lists and some single leaves.  T = 3: that,
    a level with one label, and a level of L labels of one leaf each in descending order (more than 64 labels at L = 65, 257)."""
    first = [[], list(range(L)), list(range(0, L // 2 + 1)), list(range(L // 3, L))] + [[l] for l in range(0, L, max(1, L // 5))]
    return [first] if T == 1 else [first, [list(range(L))], [[l] for l in range(L - 1, -1, -1)]]


def run_merge(s, levels, pad=3, second=True, merged=True):
    n, L = s.shape
    buf = torch.full((n, L + pad), 7.25, dtype=torch.float64, device=DEV)
    buf[:, :L] = torch.from_numpy(s).to(DEV)
    p = buf[:, :L]
    label, prob, sec, mg = N.leaf_merge(p, *N.merge_tables(levels), return_second=second, return_merged=merged)
    assert bool((buf[:, L:] == 7.25).all())                         # the padding of a row is left alone
    return p.cpu().numpy(), label.cpu().numpy(), prob.cpu().numpy(), None if sec is None else sec.cpu().numpy(), \
        None if mg is None else mg.cpu().numpy()


WORST = {"posterior": 0.0}


@pytest.mark.parametrize("L", LS)
def test_leaf_merge_on_synthetic_scores(L):
    for n in NS:
        s = make_scores(n, L, 100 * L + n)
        want = LR.posteriors(s)
        for T in (1, 3):
            levels = make_levels(L, T)
            p, label, prob, second, merged = run_merge(s, levels)
            # the posteriors against the restatement, within the derived gate
            assert np.array_equal(np.isnan(p), np.isnan(want)) and np.isnan(p[0]).all()
            ok = ~np.isnan(want)
            gate = LR.tolerance_posteriors(want, L)
            err = np.abs(p - want)
            assert (err[ok] <= gate[ok]).all(), (n, L, float((err[ok] / gate[ok]).max(initial=0.0)))
            WORST["posterior"] = max(WORST["posterior"], float((err[ok] / gate[ok]).max(initial=0.0)))
            if n > 1:
                assert p[1, L // 2] == 1.0 or L == 1                # the spread above 745: the others are 0 or denormal
                assert (p[1][np.arange(L) != L // 2] < 2.0 ** -1022).all()
            # given the device's posteriors: numpy's sequential sums and arg-max, bit for bit
            assert label.dtype == np.int32 and label.shape == prob.shape == second.shape == (T, n)
            for t, lists in enumerate(levels):
                P, lab, pr, sec = LR.merge(p, lists)
                assert np.array_equal(label[t], lab), (n, L, t)
                assert _bits(np.nan_to_num(prob[t], nan=-1.0), np.nan_to_num(pr, nan=-1.0))
                assert np.array_equal(np.isnan(prob[t]), np.isnan(pr))
                assert np.array_equal(second[t], sec, equal_nan=True)
                if t == 0:
                    assert merged.shape == P.shape and np.array_equal(np.isnan(merged), np.isnan(P))
                    assert _bits(np.nan_to_num(merged, nan=-1.0), np.nan_to_num(P, nan=-1.0))
                    assert (merged[:, 0] == 0.0).all()              # the empty list: exactly 0, also in a NaN row
                if len(lists) == 1:
                    assert (second[t] == 0.0).all() and (label[t] == 0).all()
            assert label[0, 0] == 1 and np.isnan(prob[0, 0])          # all -inf: np.argmax takes the first NaN, past the empty list
            # level t of the multi-level call is the one-level call; a second run gives the same bits
            if T == 3:
                again = run_merge(s, levels)
                assert all(_bits(a, b) for a, b in zip(again, (p, label, prob, second, merged)))
                for t, lists in enumerate(levels):
                    p1, l1, pr1, s1, _ = run_merge(s, [lists], merged=False)
                    assert _bits(p1, p) and _bits(l1[0], label[t]) and _bits(pr1[0], prob[t]) and _bits(s1[0], second[t])
                # a cell alone is the cell in the batch
                for r in sorted({0, min(1, n - 1), n // 2, n - 1}):
                    pa, la, pra, sa, ma = run_merge(s[r:r + 1], levels, pad=0)
                    assert _bits(pa[0], p[r]) and _bits(la[:, 0], label[:, r]) and _bits(pra[:, 0], prob[:, r])
                    assert _bits(sa[:, 0], second[:, r]) and _bits(ma[0], merged[r])
    print(f"L = {L}: worst posterior error / gate {WORST['posterior']:.3f}")


def test_leaf_merge_without_the_optional_outputs_and_on_ties():
    s = np.array([[0.0, 0.0, -1.0], [-1.0, 0.0, 0.0], [0.0, 0.0, 0.0]])         # equal scores give equal posteriors, to the bit
    levels = [[[0], [1], [2]], [[2], [1], [0]], [[0, 1], [1, 0]]]
    p, label, prob, second, merged = run_merge(s, levels, second=False, merged=False)
    assert second is None and merged is None
    assert p[0, 0] == p[0, 1] > p[0, 2] and p[1, 1] == p[1, 2] > p[1, 0] and p[2, 0] == p[2, 1] == p[2, 2]
    assert label.tolist() == [[0, 1, 0], [1, 0, 0], [0, 0, 0]]      # ties: the lowest index, as np.argmax
    _, _, prob2, second2, _ = run_merge(s, levels)
    assert _bits(prob, prob2) and _bits(second2, prob2)             # the runner-up of a tie is its equal


# ---- refusals of the C entry, before any launch ------------------------------------------------------------------------------
def test_leaf_merge_refusals():
    n, L, T, K = 8, 5, 2, 3
    p = torch.zeros(n, L, dtype=torch.float64, device=DEV)
    ls = torch.tensor([0, 3, 6], dtype=torch.int32, device=DEV)
    st = torch.tensor([0, 1, 2, 3, 4, 5, 6], dtype=torch.int32, device=DEV)
    lf = torch.tensor([0, 1, 2, 3, 4, 0], dtype=torch.int32, device=DEV)
    label = torch.full((T, n), -5, dtype=torch.int32, device=DEV)
    prob = torch.full((T, n), -5.0, dtype=torch.float64, device=DEV)
    merged = torch.zeros(n, K, dtype=torch.float64, device=DEV)
    good = dict(p=p.data_ptr(), ldp=L, n=n, L=L, ls=ls.data_ptr(), T=T, st=st.data_ptr(), K_total=6, K_max=K, lf=lf.data_ptr(),
                nnz=6, ws=None, ws_bytes=0, label=label.data_ptr(), prob=prob.data_ptr(), second=None, merged=merged.data_ptr(), K0=K)

    def call(**change):
        a = dict(good, **change)
        return N.lib().mmvae_leaf_merge(a["p"], a["ldp"], a["n"], a["L"], a["ls"], a["T"], a["st"], a["K_total"], a["K_max"], a["lf"],
                                        a["nnz"], a["ws"], a["ws_bytes"], a["label"], a["prob"], a["second"], a["merged"], a["K0"],
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream))

    BAD, UNS = -1, -2                                               # MMVAE_E_BADARG, MMVAE_E_UNSUPPORTED (include/mmvae.h)
    for change in (dict(p=None), dict(ls=None), dict(st=None), dict(lf=None), dict(label=None), dict(prob=None), dict(n=0),
                   dict(n=2 ** 31 + 1), dict(L=0), dict(T=0), dict(K_max=0), dict(K_total=0), dict(K_total=T * K + 1), dict(nnz=-1),
                   dict(K0=0), dict(K0=K + 1), dict(ldp=L - 1), dict(p=p.data_ptr() + 4), dict(prob=prob.data_ptr() + 4),
                   dict(second=prob.data_ptr() + 4), dict(merged=merged.data_ptr() + 4), dict(label=label.data_ptr() + 2),
                   dict(ls=ls.data_ptr() + 2), dict(st=st.data_ptr() + 1), dict(lf=lf.data_ptr() + 3), dict(ws=12)):
        assert call(**change) == BAD, change
        assert N.lib().mmvae_last_error_string().decode().startswith("leaf_merge:")
    for change in (dict(L=4097, ldp=4097), dict(K_max=4097), dict(T=4097, K_total=6), dict(nnz=2 ** 31)):
        assert call(**change) == UNS, change
    # n = 2^31 is still a count: such a call gets past the argument checks to the limits, n = 2^31 + 1 (above) does not
    assert call(n=2 ** 31, L=4097, ldp=4097) == UNS and call(n=2 ** 31 + 1, L=4097, ldp=4097) == BAD
    assert call(K0=0, merged=None) == 0                             # K0 is not read without merged
    torch.cuda.synchronize()
    assert int(N.lib().mmvae_leaf_merge_workspace_bytes(n, L, T)) == 0
    with pytest.raises(ValueError):
        N.leaf_merge(p, [0, 1], [0, 1], [L])                        # the wrapper reads the tables: a leaf that is no column
    with pytest.raises(ValueError):
        N.leaf_merge(p, [0, 0, 1], [0, 1], [0])                     # a level without a label
    with pytest.raises(ValueError):
        N.leaf_merge(p, [0, 1], [0, 2], [0])                        # start past the leaf entries
    with pytest.raises(TypeError):
        N.leaf_merge(p.t(), [0, 1], [0, 1], [0])                    # written in place: no copy can stand in


# ---- the fixture's cases ------------------------------------------------------------------------------------------------------
def _case(k):
    w = G[f"c{k}/weight"]
    return G[f"c{k}/train_z"], G[f"c{k}/train_lbl"], G[f"c{k}/test_z"], G[f"c{k}/test_lbl"], G[f"c{k}/leaves"], w.tolist()


_RESTATED = {}


def _restated(k, m):
    """The restatement of level m of case k and the derived gate of every merged sum, computed once."""
    if (k, m) not in _RESTATED:
        tr, ltr, te, lte, leaves, w = _case(k)
        base = f"c{k}/m{m}"
        res = LR.predict_leaf_gmm(tr.astype(np.float64), ltr, te.astype(np.float64), lte, 6, 12, G[f"{base}/dataset"], leaves,
                                  json.loads(str(G[f"{base}/desc"])), w if len(w) else None)
        pivot = torch.from_numpy(tr).to(DEV).mean(dim=0).cpu().numpy().astype(np.float64)
        delta = LR.tolerance_scores(res, pivot, tr.shape[1], np.abs(tr).max(axis=0))
        gate = LR.tolerance_merged(LR.tolerance_path(res["post"], delta), res["lists"])[res["keep"]]
        _RESTATED[(k, m)] = (res, gate)
    return _RESTATED[(k, m)]


@pytest.mark.parametrize("k,m", SETS, ids=[f"{KINDS[k]}-m{m}" for k, m in SETS])
def test_fixture_predict_leaf_gmm_equals_the_recorded_reference(k, m):
    tr, ltr, te, lte, leaves, w = _case(k)
    base = f"c{k}/m{m}"
    dataset, desc = G[f"{base}/dataset"], json.loads(str(G[f"{base}/desc"]))
    before = lte.copy()
    true, pred, n_exc, n_pred, n_rem, prob = TH.predict_leaf_gmm(tr, ltr, te, lte, 6, 12, dataset.tolist(), leaves.tolist(), desc, w)
    assert np.array_equal(lte, before)                              # the caller's labels are left alone
    assert [int(n_exc), int(n_pred), int(n_rem)] == list(G[f"{base}/counts"]) and int(n_exc) > 0
    assert np.array_equal(true, G[f"{base}/true"])
    res, gate = _restated(k, m)
    ok = ~np.isnan(G[f"{base}/prob"])
    assert np.array_equal(pred[ok], G[f"{base}/pred"][ok]) and np.array_equal(pred, res["pred"])          # every kept cell
    rows = np.arange(len(pred))
    g = gate[rows, np.argmax(res["merged"], axis=1)]
    err = np.abs(prob - res["prob"])
    print(f"{base}: worst |device - restatement| {err.max():.2e}, worst error / gate {float((err / g).max()):.2e}")
    assert np.isfinite(prob).all() and (err <= g).all()
    err_ref = np.abs(prob[ok] - G[f"{base}/prob"][ok])
    print(f"{base}: worst |device - reference| {err_ref.max():.2e}, e_ref {float(G[f'c{k}/e_ref']):.2e}")
    assert (err_ref <= g[ok] + float(G[f"c{k}/e_ref"])).all()
    if KINDS[k] == "far10":                    # where the reference is 0 / 0 = NaN (and labels the cell with column 0)
        assert len(G[f"{base}/nan_rows"]) > 0 and np.array_equal(np.flatnonzero(~ok), G[f"{base}/nan_rows"])
        assert np.array_equal(pred[~ok], G[f"{base}/far_pred"])
    else:
        assert ok.all()
    # without test labels nothing is dropped and None comes back
    t2, p2, e2, _, _, pr2 = TH.predict_leaf_gmm(tr, ltr, te, None, 6, 12, dataset.tolist(), leaves.tolist(), desc, w)
    assert t2 is None and int(e2) == 0 and len(p2) == len(te) and _bits(pr2[res["keep"]], prob) and np.array_equal(p2[res["keep"]], pred)


@pytest.mark.parametrize("k", range(len(KINDS)), ids=KINDS)
def test_every_level_of_merge_sweep_is_predict_leaf_gmm(k):
    tr, ltr, te, lte, leaves, w = _case(k)
    changes = json.loads(str(G[f"c{k}/changes"]))
    levels = [int(m) for m in G[f"c{k}/levels"] if m >= 0]
    kw = dict(label_weight=w) if len(w) else {}
    sweep = TH.merge_sweep(tr, ltr, te, lte, changes, leaves, levels=levels, **kw)
    assert sorted(sweep) == ["acc", "keep", "levels", "n_classes", "n_excluded_cells", "pred", "prob", "true"]
    assert list(sweep["levels"]) == levels and sweep["n_excluded_cells"] == int(G[f"c{k}/m0/counts"][0])
    for t, m in enumerate(levels):
        dataset = TH.labels_at(leaves, changes, m)
        true, pred, n_exc, _, _, prob = TH.predict_leaf_gmm(tr, ltr, te, lte, 6, 12, dataset, leaves, TH.descendants_at(changes, m), w)
        assert np.array_equal(dataset, G[f"c{k}/m{m}/dataset"]) and sweep["n_classes"][t] == len(dataset)
        assert np.array_equal(sweep["pred"][t], pred) and np.array_equal(sweep["true"][t], true) and _bits(sweep["prob"][t], prob)
        assert sweep["acc"][t] == np.mean(pred == true)
        ok = ~np.isnan(G[f"c{k}/m{m}/prob"])
        assert np.array_equal(sweep["pred"][t][ok], G[f"c{k}/m{m}/pred"][ok]) and np.array_equal(sweep["true"][t], G[f"c{k}/m{m}/true"])
    if k == 0:                                                      # the default: every level that leaves two labels or more
        full = TH.merge_sweep(tr, ltr, te, lte, changes, leaves)
        assert list(full["levels"]) == [m for m in range(len(changes) + 1) if len(TH.labels_at(leaves, changes, m)) >= 2]
        assert full["n_classes"][0] == len(leaves) and full["n_classes"][-1] >= 2 and (np.diff(full["n_classes"]) < 0).all()
        for t, m in enumerate(levels):
            assert _bits(full["prob"][list(full["levels"]).index(m)], sweep["prob"][t])


def test_fixture_custom_qda_equals_the_recorded_reference():
    lte = G["qda/test_lbl"]
    true, pred = TH.custom_QDA(G["qda/train_z"], G["qda/train_lbl"], G["qda/test_z"], lte.tolist())
    assert np.array_equal(pred, G["qda/pred"]) and np.array_equal(true, G["qda/true"])
    # a class with too few training cells: never predicted, and its test cells read 'excluded' in both returns
    tr, ltr = G["qda/train_z"], G["qda/train_lbl"]
    drop = np.flatnonzero(ltr == "Q0")[5:]
    keep = np.setdiff1d(np.arange(len(ltr)), drop)
    true2, pred2 = TH.custom_QDA(tr[keep], ltr[keep], G["qda/test_z"], lte)
    mt, mp, _ = LR.custom_qda(tr[keep].astype(np.float64), ltr[keep], G["qda/test_z"].astype(np.float64), lte)
    assert np.array_equal(true2, mt.astype(true2.dtype)) and np.array_equal(pred2, mp.astype(pred2.dtype))
    assert (true2[lte == "Q0"] == "excluded").all() and (pred2[lte == "Q0"] == "excluded").all() and not (pred2 == "Q0").any()
    flat = tr.copy()
    flat[:, 1] = 0.5
    with pytest.raises(ValueError, match="is singular"):
        TH.custom_QDA(flat, ltr, G["qda/test_z"], lte)


# ---- the trainer entry ----------------------------------------------------------------------------------------------------
def test_classify_tree_equals_the_restatement_on_the_latents():
    from distributed_vae_amd.cpl_mixvae import cpl_mixVAE
    from distributed_vae_amd.utils.dataloader import DeviceLoader
    Dm, Cc, S, A, n, kfold = 40, 5, 2, 2, 300, 3
    t = cpl_mixVAE(saving_folder="", device=0, save_flag=False)
    t.init_model(n_categories=Cc, state_dim=S, input_dim=Dm, fc_dim=32, lowD_dim=6, x_drop=0.5, s_drop=0.2, n_arm=A, temp=1.0,
                 tau=0.005)
    x, codes = GI.points(400, Dm, 4, seed=9, spread=1.0)
    data = torch.from_numpy(np.abs(x)).to(DEV)
    labels = np.array([f"type{v}" for v in codes])
    leaves = np.unique(labels)
    changes = [[["type0", "type1"], "n3", 5], [["type2", "type3"], "n2", 3], [["n3", "n2"], "n1", 1]]
    index = torch.from_numpy(np.random.default_rng(2).permutation(400)[:n])
    dl = DeviceLoader(data, index, 64, False, False)
    got = t.classify_tree(dl, labels, changes, leaves, kfold=kfold, seed=1, arm=1, on="x_low")
    assert sorted(got) == ["acc", "data_indx", "fold", "keep", "levels", "n_classes", "pred", "prob"]
    rows = got["data_indx"].astype(np.int64)
    assert np.array_equal(rows, index.numpy()) and np.array_equal(got["fold"], kfold_of(n, kfold, 1))
    assert list(got["levels"]) == [0, 1, 2] and list(got["n_classes"]) == [4, 3, 2] and got["keep"].all()
    z = t.encode_dataset(dl)["x_low"][1]
    z = (z.cpu().numpy() if isinstance(z, torch.Tensor) else np.asarray(z)).astype(np.float64)
    y = labels[rows]
    pred = np.empty((3, n), dtype=got["pred"].dtype)
    prob, gate = np.zeros((3, n)), np.zeros((3, n))
    for f in range(kfold):
        test, train = got["fold"] == f, got["fold"] != f
        m = LR.leaf_models(z[train], y[train], leaves)
        sc, mag = LR.scores(z[test], m)
        post = LR.posteriors(sc)
        delta = LR.tolerance_scores({"models": m, "scores": sc, "A": mag}, z.mean(axis=0), z.shape[1], np.abs(z).max(axis=0))
        for lv in range(3):
            at = LR.do_merges(leaves, changes, lv)
            labs = np.unique(at)
            lists = [[int(i) for i in np.flatnonzero(at == name)] for name in labs]
            _, lab, pr, _ = LR.merge(post, lists)
            pred[lv, test], prob[lv, test] = labs[lab], pr
            gate[lv, test] = LR.tolerance_merged(LR.tolerance_path(post, delta), lists)[np.arange(len(lab)), lab]
    assert np.array_equal(got["pred"], pred)                        # labels exact
    err = np.abs(got["prob"] - prob)
    print(f"classify_tree: worst |device - restatement| {err.max():.2e}, worst error / gate {float((err / gate).max()):.2e}")
    assert (err <= gate).all()
    for lv in range(3):
        hit = pred[lv] == LR.do_merges(y, changes, lv)
        for f in range(kfold):
            assert got["acc"][f, lv] == np.mean(hit[got["fold"] == f])
    sub = t.classify_tree(dl, labels, changes, leaves, kfold=kfold, seed=1, arm=1, levels=[2, 0])
    assert _bits(sub["prob"][0], got["prob"][2]) and _bits(sub["prob"][1], got["prob"][0])
    with pytest.raises(ValueError):
        t.classify_tree(dl, labels, changes, leaves, arm=A)
    with pytest.raises(ValueError):
        t.classify_tree(dl, labels, changes, leaves, on="recon")
    with pytest.raises(ValueError):
        t.classify_tree(DeviceLoader(data, index, 64, False, True), labels, changes, leaves)   # drop_last with a remainder
    with pytest.raises(ValueError):
        t.classify_tree(dl, labels, changes, leaves, kfold=1)

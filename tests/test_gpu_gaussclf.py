"""GPU: the Gaussian classifiers on the device.  mmvae_group_moments and mmvae_gauss_scores through their wrappers, the public
``QDA_classifier`` / ``LDA_classifier`` / ``gaussian_cv_predict`` and ``cpl_mixVAE.classify_latents`` against the numpy fp64
restatement (tests/gaussclf_restatement.py) and the reference's recorded returns (tests/golden/gaussclf_kat.npz), on the
fixture's cases and on the smallest shapes at which a launch can go wrong (tests/gaussclf_inputs.py).

Bounds (derived in DESIGN.md section 9f and include/mmvae.h, not tuned; u = 2^-53).
  Moments: against the two-pass mean and scatter of every group, ``tolerance_moments``: 5 (N + 2) u N sqrt(m_i m_j) for the
  scatter (four units the device's raw-moment form, one the two-pass reference's own rounding), m the mean square about
  the pivot = kappa var, so the bound grows with the pivot's distance as kappa does.
  Scores, the kernel handed the restatement's own mu, W and c0: ``tolerance_sum``, (3 d + 4) u (A + |c0|) -- summation
  order alone.  Labels are compared on the cells whose restated margin exceeds twice the row's largest gate; the CPU tests
  show that this is every cell of every input here (the cap on excused cells is 1 %; none is excused).
  The whole path (device moments, host eigh, device scores) against the restatement (two-pass covariance): ``tolerance_cv``;
  against sklearn's recorded decision_function the case's e_ref is added.  Predictions, folds and accuracies: exact.

Bit-equality claims tested here: the four instances of the segment kernel; a group of a grouped call and a call on its rows
alone; a padded or unaligned matrix and its contiguous copy; three runs; a cell's scores under a permutation of the cells
and a relabelling of the classes; float64 host input of float32 values and the device tensor.

Measured on an MI355X, worst error over gate: moments 0.047 (pivot at the mean) and 0.032 (100 standard deviations away);
scores on the same model 0.27 (K37; absolute 1.8e-12); the whole path on the fixture 4.6e-3 (absolute 4.5e-9 on QDA scores of
magnitude 1e5, 7.1e-13 on LDA scores); against sklearn's recorded scores 1.9e-9 (QDA) and 7.0e-13 (LDA).  No cell was
excused anywhere."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gaussclf_inputs as GI  # noqa: E402
import gaussclf_restatement as GR  # noqa: E402
from gpu_util import DEV  # noqa: E402
from distributed_vae_amd import _native as N  # noqa: E402
from distributed_vae_amd.utils import cluster_analysis as CA  # noqa: E402

pytestmark = pytest.mark.gpu

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gaussclf_kat.npz"))
CASES = [tuple(int(v) for v in row) for row in G["cases"]]
SETS = [(k, clf, str(key)) for k in range(len(CASES)) for clf in ("qda", "lda") for key in G[f"c{k}/keys"]]


def _t(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)          # a copy: the cached arrays are read-only


def _bits(a, b):
    a, b = (v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v) for v in (a, b))
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_the_named_switch_points():
    assert (N.GAUSSCLF_SEG_ROWS, N.GAUSSCLF_ROW_TILE, N.GAUSSCLF_COL_BLOCK) == (256, 64, 8) and N.GAUSSCLF_DC == (16, 32, 64, 128)
    assert N.GAUSSCLF_SCORE_WAVES == 16 and {GI.SCORE_CASES[k][2] for k in ("K2", "K16", "K17", "K37")} == {2, 16, 17, 37}


# ---- the fixture's cases ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(6))
def test_fixture_classifiers_equal_the_recorded_reference(k):
    n, d, kfold, seed = CASES[k]
    x = G[f"c{k}/x"]
    labels = {str(key): G[f"c{k}/y/{key}"] for key in G[f"c{k}/keys"]}
    for clf, fn in (("qda", CA.QDA_classifier), ("lda", CA.LDA_classifier)):
        acc, ref, pred = fn(x, labels, kfold, seed)
        assert list(acc) == list(ref) == list(pred) == list(labels)
        for key in labels:
            base = f"c{k}/{clf}/{key}"
            assert len(acc[key]) == len(ref[key]) == len(pred[key]) == kfold
            assert [len(p) for p in pred[key]] == list(G[f"{base}/sizes"])
            got = np.concatenate(pred[key])
            assert got.dtype == G[f"{base}/pred"].dtype and np.array_equal(got, G[f"{base}/pred"])     # every cell
            assert np.array_equal(np.concatenate(ref[key]), G[f"{base}/ref"])
            assert all(type(a) is float for a in acc[key]) and np.array_equal(np.array(acc[key]), G[f"{base}/acc"])


@pytest.mark.parametrize("k,clf,key", SETS, ids=[f"c{k}-{clf}-{key}" for k, clf, key in SETS])
def test_fixture_scores_within_the_derived_gate(k, clf, key):
    n, d, kfold, seed = CASES[k]
    x, y = G[f"c{k}/x"], G[f"c{k}/y/{key}"]
    base = f"c{k}/{clf}/{key}"
    res = GR.cv_predict(x, y, kfold, seed, clf)
    got = CA.gaussian_cv_predict(x, y, kfold, seed, kind=clf, return_scores=True)
    assert np.array_equal(got["classes"], res["classes"]) and np.array_equal(got["fold"], res["fold"])
    assert got["pred"].dtype == np.int64 and np.array_equal(got["pred"], res["pred"])
    pivot = torch.from_numpy(x).to(DEV).mean(dim=0).cpu().numpy().astype(np.float64)
    gate = GR.tolerance_cv(res, pivot, clf)
    err = np.abs(got["scores"] - res["scores"])
    print(f"{base}: worst |device - restatement| {err.max():.2e}, gate {gate.min():.2e} .. {gate.max():.2e}, worst error / gate "
          f"{float((err / gate).max()):.2e}")
    assert (err <= gate).all()
    assert (np.abs(got["best"] - res["best"]) <= gate.max(axis=1)).all()
    assert (np.abs(got["second"] - res["second"]) <= gate.max(axis=1)).all()
    assert _bits(got["best"], got["scores"].max(axis=1)) and _bits(got["best"], got["scores"][np.arange(n), got["pred"]])
    rows = G[f"{base}/rows"]
    mine, theirs, g = got["scores"][rows], G[f"{base}/dec"], gate[rows]
    if clf == "lda":                              # sklearn's scores: up to a term that is the same for every class of a cell
        mine, theirs = mine - mine.max(axis=1, keepdims=True), theirs - theirs.max(axis=1, keepdims=True)
        g = g + g.max(axis=1, keepdims=True)
    err_sk = np.abs(mine - theirs)
    print(f"{base}: worst |device - sklearn| {err_sk.max():.2e}, e_ref {float(G[f'{base}/e_ref']):.2e}")
    assert (err_sk <= g + float(G[f"{base}/e_ref"])).all()


# ---- the moments kernel -------------------------------------------------------------------------------------------------------
def _check_moments(name, far, s, M, what):
    m = GI.moment_input(name, far)
    d = GI.MOMENT_CASES[name][1]
    x, off, pivot = m["x"], m["offsets"], m["pivot"].astype(np.float64)
    s, M = s.cpu().numpy(), M.cpu().numpy()
    assert s.dtype == M.dtype == np.float64 and s.shape == (len(off) - 1, d) and M.shape == (len(off) - 1, d * (d + 1) // 2)
    full = GI.unpack(M, d)
    worst = 0.0
    for g, (cnt, mean, scat) in enumerate(m["stats"]):
        if cnt == 0:
            assert not s[g].any() and not M[g].any(), what                # an empty group: zeros
            continue
        xg = x[off[g]:off[g + 1]].astype(np.float64)
        tol_mean, tol_scat = GR.tolerance_moments(cnt, ((xg - pivot) ** 2).mean(axis=0), pivot, np.abs(xg).max(axis=0))
        e_mean, e_scat = np.abs(pivot + s[g] / cnt - mean), np.abs(full[g] - np.outer(s[g], s[g]) / cnt - scat)
        worst = max(worst, float((e_mean / tol_mean).max()), float((e_scat / tol_scat).max()))
        assert (e_mean <= tol_mean).all() and (e_scat <= tol_scat).all(), (what, g)
    print(f"{what}: worst error / bound {worst:.2e}")
    return worst


@pytest.mark.parametrize("name", sorted(GI.MOMENT_CASES))
def test_moments_against_the_two_pass_restatement(name):
    d = GI.MOMENT_CASES[name][1]
    for far in (False, True):                     # the pivot at the data's mean, and 100 standard deviations away
        m = GI.moment_input(name, far)
        s, M = N.group_moments(_t(m["x"]), _t(m["offsets"]), _t(m["pivot"]))
        _check_moments(name, far, s, M, f"{name} far={far}")
        for path in N.GAUSSCLF_PATHS:             # every instance that holds d: the same bits
            if path != "auto" and d <= int(path[1:]):
                s2, M2 = N.group_moments(_t(m["x"]), _t(m["offsets"]), _t(m["pivot"]), path=path)
                assert _bits(s, s2) and _bits(M, M2), path
    if d > N.GAUSSCLF_DC[0]:
        with pytest.raises(NotImplementedError):
            N.group_moments(_t(m["x"]), _t(m["offsets"]), _t(m["pivot"]), path="d16")
    with pytest.raises(ValueError):
        N.group_moments(_t(m["x"]), _t(m["offsets"]), _t(m["pivot"]), path="wide")


def test_moments_one_group_and_a_group_alone():
    """G = 1, and every group of a grouped call against a call on its rows alone: the same bits."""
    m = GI.moment_input("segments")
    x, off, pivot = m["x"], m["offsets"], _t(m["pivot"])
    s, M = N.group_moments(_t(x), _t(off), pivot)
    for g in range(len(off) - 1):
        if off[g + 1] > off[g]:
            s1, M1 = N.group_moments(_t(x[off[g]:off[g + 1]]), _t(np.array([0, off[g + 1] - off[g]], dtype=np.int64)), pivot)
            assert _bits(s1[0], s[g]) and _bits(M1[0], M[g]), g
    runs = [N.group_moments(_t(x), _t(off), pivot) for _ in range(2)]
    assert all(_bits(r[0], s) and _bits(r[1], M) for r in runs)                                  # three runs


@pytest.mark.parametrize("name", ["d2", "d17"])
def test_moments_read_only_the_window(name):
    """ld > d with 1e30 beside the window and a base that is not 16-byte aligned: the bits of the contiguous copy."""
    m = GI.moment_input(name)
    x, d = m["x"], GI.MOMENT_CASES[name][1]
    n, ld = x.shape[0], d + 3
    flat = torch.full((n * ld + 1,), 1e30, device=DEV)
    odd = flat[1:].view(n, ld)[:, :d]
    odd.copy_(_t(x))
    assert odd.stride() == (ld, 1) and odd.data_ptr() % 16 != 0
    s, M = N.group_moments(_t(x), _t(m["offsets"]), _t(m["pivot"]))
    s2, M2 = N.group_moments(odd, _t(m["offsets"]), _t(m["pivot"]))
    assert _bits(s, s2) and _bits(M, M2)


def test_moments_bound_scales_with_kappa():
    """A pivot 100 standard deviations away: kappa about 1e4, the bound 1e4 times as large, and the error inside it."""
    near, far = GI.moment_input("d2"), GI.moment_input("d2", True)
    x = near["x"].astype(np.float64)
    k_near = 1 + ((x.mean(0) - near["pivot"]) ** 2 / x.var(0)).max()
    k_far = 1 + ((x.mean(0) - far["pivot"]) ** 2 / x.var(0)).min()
    assert k_near < 1.01 and 5e3 < k_far < 2e4
    s, M = N.group_moments(_t(far["x"]), _t(far["offsets"]), _t(far["pivot"]))
    assert _check_moments("d2", True, s, M, "kappa 1e4") <= 1.0


# ---- the scores kernel --------------------------------------------------------------------------------------------------------
def _run_scores(case, perm=None, scores=True):
    x, model = case["x"], case["model"]
    order = np.argsort(model, kind="stable") if perm is None else perm
    out = N.gauss_scores(_t(x[order]), _t(model[order]), _t(case["mu"]), _t(case["W"]), _t(case["c0"]), _t(order.astype(np.int64)),
                         return_scores=scores)
    return [None if o is None else o.cpu().numpy() for o in out]


@pytest.mark.parametrize("name", sorted(GI.SCORE_CASES))
def test_scores_against_the_restatement_on_the_same_model(name):
    case = GI.score_input(name)
    label, best, second, sc = _run_scores(case)
    n, K = case["scores"].shape
    assert label.dtype == np.int32 and best.dtype == second.dtype == sc.dtype == np.float64 and sc.shape == (n, K)
    want = case["scores"]
    assert np.array_equal(np.isneginf(sc), np.isneginf(want)) and not np.isnan(sc).any()       # -inf exactly where absent
    fin = np.isfinite(want)
    err = np.abs(sc[fin] - want[fin])
    gate = case["gate"][fin]
    print(f"{name}: worst |device - restatement| {err.max():.2e}, gate {gate.min():.2e} .. {gate.max():.2e}, worst error / gate "
          f"{float((err / gate).max()):.2e}")
    assert (err <= gate).all()
    must = GI.decided(case)
    assert must.all()                                                           # no cell is excused (cap: 1 %)
    assert np.array_equal(label[must], case["pred"][must])
    assert _bits(best, sc.max(axis=1)) and _bits(best, sc[np.arange(n), label])
    assert _bits(second, np.sort(sc, axis=1)[:, -2])
    # without the score matrix, and without the permutation: the same bits
    l2, b2, s2, none = _run_scores(case, scores=False)
    assert none is None and _bits(l2, label) and _bits(b2, best) and _bits(s2, second)
    order = np.argsort(case["model"], kind="stable")
    l3, b3, _, _ = N.gauss_scores(_t(case["x"][order]), _t(case["model"][order]), _t(case["mu"]), _t(case["W"]), _t(case["c0"]))
    assert _bits(l3, label[order]) and _bits(b3, best[order])


def test_scores_exact_tie_gives_the_lowest_index():
    """Classes 0 and 2 are given the same model: their scores are the same bits, and the label is never 2."""
    case = dict(GI.score_input("n200_F3"))
    mu, W, c0 = (np.array(case[k]) for k in ("mu", "W", "c0"))
    mu[:, 2], W[:, 2], c0[:, 2] = mu[:, 0], W[:, 0], c0[:, 0]
    case.update(mu=mu, W=W, c0=c0)
    label, best, second, sc = _run_scores(case)
    assert _bits(sc[:, 0], sc[:, 2]) and (label != 2).all() and np.array_equal(label, np.argmax(sc, axis=1))
    tied = label == 0
    assert tied.any() and _bits(best[tied], second[tied])


def test_scores_do_not_depend_on_the_order_of_cells_or_classes():
    """Three runs, unsorted cells (every tile walks several models), and relabelled classes: each cell the same bits."""
    case = GI.score_input("n200_F3")
    label, best, second, sc = _run_scores(case)
    for _ in range(2):
        again = _run_scores(case)
        assert all(_bits(a, b) for a, b in zip(again, (label, best, second, sc)))
    shuffled = np.random.default_rng(5).permutation(len(label))
    l2, b2, s2, sc2 = _run_scores(case, perm=shuffled)
    assert _bits(l2, label) and _bits(b2, best) and _bits(s2, second) and _bits(sc2, sc)
    relabel = np.array([3, 0, 4, 1, 2])                                          # new class j is old class relabel[j]
    moved = dict(case)
    moved.update(mu=case["mu"][:, relabel], W=case["W"][:, relabel], c0=case["c0"][:, relabel])
    l3, b3, s3, sc3 = _run_scores(moved)
    assert _bits(sc3, sc[:, relabel]) and _bits(b3, best) and _bits(s3, second) and np.array_equal(relabel[l3], label)


# ---- the public entries ---------------------------------------------------------------------------------------------------------
def test_device_tensor_in_place_and_float64_host_input():
    k = 0
    n, d, kfold, seed = CASES[k]
    x, y = G[f"c{k}/x"], G[f"c{k}/y/T"]
    host = CA.gaussian_cv_predict(x.astype(np.float64), y, kfold, seed, return_scores=True)     # float64 of float32 values
    wide = torch.full((n, d + 5), 1e30, device=DEV)
    wide[:, 2:2 + d] = _t(x)
    window = wide[:, 2:2 + d]                                                     # a column window, used where it lies
    before = wide.clone()
    dev = CA.gaussian_cv_predict(window, y, kfold, seed, return_scores=True)
    assert torch.equal(wide, before)
    for name in ("pred", "fold", "best", "second", "scores"):
        assert _bits(dev[name], host[name]), name
    strings = np.array([f"t{v:03d}" for v in y])                                 # names that sort as the numbers do
    named = CA.gaussian_cv_predict(x, strings, kfold, seed, kind="lda")
    plain = CA.gaussian_cv_predict(x, y, kfold, seed, kind="lda")
    assert named["classes"].dtype.kind == "U" and _bits(named["best"], plain["best"])
    a1, r1, p1 = CA.LDA_classifier(_t(x), {"s": strings}, kfold, seed)
    assert p1["s"][0].dtype.kind == "U" and np.array_equal(np.concatenate(r1["s"]), strings[np.argsort(plain["fold"], kind="stable")])


def test_singleton_class_and_small_class_departure():
    """A class with one training cell raises sklearn's error; a class with at most d training cells (where sklearn's own
    prediction hangs on an arbitrary null-space vector) follows the restatement: all d eigen-directions."""
    x, codes = (np.array(a) for a in GI.points(240, 12, 4, seed=3))
    fold = CA.kfold_of(240, 4, 0)
    other = int(np.flatnonzero(fold != fold[0])[0])
    y = codes.copy()
    y[[0, other]] = 9
    with pytest.raises(ValueError, match="y has only 1 sample in class 9"):
        CA.gaussian_cv_predict(x, y, 4, 0)
    y = codes.copy()
    y[np.flatnonzero(codes == 3)[10:]] = 0                                       # class 3: ten cells, d = 12
    res = GR.cv_predict(x, y, 4, 0, "qda")
    assert 2 <= res["counts"][:, 3].min() and res["counts"][:, 3].max() <= 12
    got = CA.gaussian_cv_predict(x, y, 4, 0, return_scores=True)
    pivot = torch.from_numpy(np.array(x)).to(DEV).mean(dim=0).cpu().numpy().astype(np.float64)
    gate = GR.tolerance_cv(res, pivot, "qda")
    err = np.abs(got["scores"] - res["scores"])
    print(f"small class: worst |device - restatement| {err.max():.2e}, worst error / gate {float((err / gate).max()):.2e}")
    assert (err <= gate).all()
    sure = (res["best"] - res["second"]) > 2.0 * gate.max(axis=1)
    assert sure.mean() >= 0.99 and np.array_equal(got["pred"][sure], res["pred"][sure])


def test_classify_latents_equals_gaussian_cv_predict_on_encode_dataset():
    from distributed_vae_amd.cpl_mixvae import cpl_mixVAE
    from distributed_vae_amd.utils.dataloader import DeviceLoader
    Dm, Cc, S, A, n = 40, 5, 2, 2, 300
    t = cpl_mixVAE(saving_folder="", device=0, save_flag=False)
    t.init_model(n_categories=Cc, state_dim=S, input_dim=Dm, fc_dim=32, lowD_dim=6, x_drop=0.5, s_drop=0.2, n_arm=A, temp=1.0,
                 tau=0.005)
    x, codes = GI.points(400, Dm, 4, seed=9, spread=1.0)
    data = _t(np.abs(x))
    labels = np.array([f"type{v}" for v in codes])                                # one label per row of the data set
    index = torch.from_numpy(np.random.default_rng(2).permutation(400)[:n])
    dl = DeviceLoader(data, index, 64, False, False)
    enc = t.encode_dataset(dl)
    rows = enc["data_indx"].astype(np.int64)
    assert np.array_equal(rows, index.numpy())
    for on, kind in (("x_low", "qda"), ("state_mu", "qda"), ("z_prob", "lda")):
        got = t.classify_latents(dl, labels, kfold=3, seed=1, arm=1, on=on, kind=kind)
        assert sorted(got) == ["acc", "data_indx", "fold", "margin", "pred_labels", "ref_labels"]
        want = CA.gaussian_cv_predict(enc[on][1], labels[rows], 3, 1, kind=kind)
        assert np.array_equal(got["fold"], want["fold"]) and _bits(got["margin"], want["best"] - want["second"])
        assert len(got["acc"]) == len(got["pred_labels"]) == len(got["ref_labels"]) == 3
        for f in range(3):
            test = np.flatnonzero(want["fold"] == f)
            assert np.array_equal(got["pred_labels"][f], want["classes"][want["pred"][test]])
            assert np.array_equal(got["ref_labels"][f], labels[rows][test])
            assert got["acc"][f] == float(np.mean(got["pred_labels"][f] == got["ref_labels"][f]))
    with pytest.raises(ValueError):
        t.classify_latents(dl, labels, arm=A)
    with pytest.raises(ValueError):
        t.classify_latents(dl, labels, on="recon")
    with pytest.raises(ValueError):
        t.classify_latents(DeviceLoader(data, index, 64, False, True), labels)   # drop_last with a remainder

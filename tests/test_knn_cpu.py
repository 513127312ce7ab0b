"""CPU: the host side of the k-nearest-neighbour analysis (utils/neighbors.py, cpl_mixVAE.latent_neighbors /
classify_neighbors).  The numpy restatement (tests/knn_restatement.py) against sklearn on float64 copies of the GPU test's
float cases: on the unambiguous cells (knn_restatement.unambiguous: the k-th and (k+1)-th squared distances further apart
than twice the fp32 gate, far more than sklearn's float64 Gram form moves them) equal neighbour sets and equal cross-validated
predictions.  The host-side contract of mmvae_knn / mmvae_knn_votes: declared, exported, ABI version unchanged, the workspace
size at the caps, every bad argument refused before any device work.  The refusals of the public functions, which come
before any device is touched, and knn_graph's CSR assembly."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import knn_restatement as KR  # noqa: E402
import distributed_vae_amd  # noqa: F401,E402
from distributed_vae_amd import _native as N  # noqa: E402
from distributed_vae_amd.utils import neighbors as NB  # noqa: E402


# ---- 1. the restatement is sklearn's answer -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(KR.FLOAT_CASES))
def test_restatement_neighbours_equal_sklearn(name):
    nn = pytest.importorskip("sklearn.neighbors")
    x32, _, k = KR.mixture(name)
    x = x32.astype(np.float64)
    idx, dist2, nxt = KR.neighbors(x, x, k, np.arange(len(x)), np.arange(len(x)))
    sure = KR.unambiguous(dist2, nxt, x.shape[1])
    print(f"{name}: {int((~sure).sum())} of {len(x)} cells ambiguous")
    assert (~sure).mean() <= 0.02
    assert (np.diff(dist2, axis=1) >= 0).all() and (idx != np.arange(len(x))[:, None]).all()
    dist, ind = nn.NearestNeighbors(n_neighbors=k, algorithm="brute").fit(x).kneighbors()         # (X = None: without itself)
    assert np.array_equal(np.sort(ind[sure], axis=1), np.sort(idx[sure], axis=1))
    assert np.allclose(dist[sure] ** 2, dist2[sure], rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("name", ["n3000_d10_k15", "n3000_d2_k5"])
def test_restatement_cv_predictions_equal_sklearn(name):
    nn = pytest.importorskip("sklearn.neighbors")
    ms = pytest.importorskip("sklearn.model_selection")
    x32, labels, k = KR.mixture(name)
    x = x32.astype(np.float64)
    kfold, seed = 5, 3
    res = KR.cv_predict(x, labels, kfold, seed, k)
    assert (~res["sure"]).mean() <= 0.02
    pred = np.full(len(x), -1, dtype=np.int64)
    for f, (train, test) in enumerate(ms.KFold(kfold, shuffle=True, random_state=seed).split(x)):
        assert np.array_equal(np.flatnonzero(res["fold"] == f), test)
        pred[test] = nn.KNeighborsClassifier(n_neighbors=k, algorithm="brute").fit(x[train], labels[train]).predict(x[test])
    got = res["classes"][res["pred"]]
    assert np.array_equal(got[res["sure"]], pred[res["sure"]])
    assert np.mean(got == labels) > 0.5


def test_restatement_hand_cases():
    r = np.array([[0.0], [1.0], [1.0], [3.0], [-1.0]])
    idx, d2, nxt = KR.neighbors(r, r, 2)
    assert idx.tolist() == [[0, 1], [1, 2], [1, 2], [3, 1], [4, 0]]                     # ties by index; a cell is its own first
    idx, d2, nxt = KR.neighbors(r, r, 3, np.arange(5), np.arange(5))
    assert idx.tolist() == [[1, 2, 4], [2, 0, 3], [1, 0, 3], [1, 2, 0], [0, 1, 2]] and d2[0].tolist() == [1, 1, 1]
    assert nxt.tolist() == [9, 4, 4, 16, 16]
    idx, d2, nxt = KR.neighbors(r, r, 3, [0, 0, 0, 1, 1], [0, 0, 0, 1, 1])             # two folds
    assert idx.tolist() == [[4, 3, -1], [3, 4, -1], [3, 4, -1], [1, 2, 0], [0, 1, 2]] and np.isinf(d2[:3, 2]).all()
    assert np.isinf(nxt).all() and KR.unambiguous(d2, nxt, 1).all()
    pred, top2 = KR.votes(np.array([[0, 1, 2], [3, 4, -1], [-1, -1, -1], [4, 4, 0]]), np.array([2, 1, 1, 3, 0]), 4)
    assert pred.tolist() == [1, 0, -1, 0] and top2.tolist() == [[2, 1], [1, 1], [0, 0], [2, 1]]  # the smallest label on ties
    p = KR.purity(np.array([[0, 1, 2], [3, 4, -1], [-1, -1, -1]]), np.array([2, 1, 1, 3, 0]), np.array([1, 0, 0]))
    assert p[0] == 2 / 3 and p[1] == 0.5 and np.isnan(p[2])


# ---- 2. the C entries on the host ---------------------------------------------------------------------------------------------
def test_entries_declared_exported_and_abi_unchanged():
    header = open(os.path.join(ROOT, "include", "mmvae.h")).read()
    L = NB._lib()
    for name in ("mmvae_knn_workspace_bytes", "mmvae_knn", "mmvae_debug_knn", "mmvae_knn_votes"):
        assert re.search(r"\b%s\(" % name, header), name
        assert hasattr(L, name), name
    assert L.mmvae_abi_version() == N.ABI_VERSION == 5
    assert '"knn.hip"' in open(os.path.join(ROOT, "distributed-vae_amd", "build.py")).read()
    assert "mmvae_knn" not in open(os.path.join(ROOT, "distributed-vae_amd", "_native.py")).read()   # bound in neighbors._lib()
    src = open(NB.__file__).read()
    assert "torch.empty" not in src and "new_empty" not in src        # every device buffer comes from _native._workspace
    assert not re.search(r"^(import|from)\s+(scipy|pandas|sklearn)", src, flags=re.M)
    for name in ("knn", "knn_graph", "neighbor_purity", "knn_cv_predict", "KNN_classifier"):
        assert f"``{name}``" in NB.__doc__ and callable(getattr(NB, name))


def test_workspace_bytes_at_the_caps_and_monotone_in_k():
    two_gib = 2 << 30
    for nq, nr, d in ((1 << 20, 1 << 20, 128), (1 << 20, 1, 1), (1, 1 << 20, 128), (256, 1 << 20, 128), (22365, 22365, 10),
                      (131072, 131072, 10), (1000, 1000, 10), (65536, 1 << 20, 2)):
        last = 0
        for k in range(1, NB.MAX_K + 1):
            b = NB.workspace_bytes(nq, nr, d, k)
            assert 8 <= b <= two_gib and b % 8 == 0, (nq, nr, d, k, b)
            assert b >= last, (nq, nr, d, k, b, last)                  # (the segment count does not depend on k)
            last = b
    assert NB.workspace_bytes(22365, 22365, 10, 15) < 64 * 10 ** 6
    for bad in ((0, 5, 3, 2), (5, 0, 3, 2), ((1 << 20) + 1, 5, 3, 2), (5, (1 << 20) + 1, 3, 2), (5, 5, 0, 2), (5, 5, 129, 2),
                (5, 5, 3, 0), (5, 5, 3, 65), (-1, 5, 3, 2)):
        assert NB.workspace_bytes(*bad) == 0, bad


PTR = 0x1000     # fake device pointers: every case must be refused before anything dereferences them


def _knn(q=PTR, ldq=10, nq=100, r=PTR, ldr=10, nr=100, d=10, k=15, qg=None, rg=None, ws=PTR, ws_bytes=1 << 32, idx=PTR, dist2=PTR,
         seg_cols=None, phases=0):
    L = NB._lib()
    if seg_cols is None:
        return L.mmvae_knn(q, ldq, nq, r, ldr, nr, d, k, qg, rg, ws, ws_bytes, idx, dist2, None)
    return L.mmvae_debug_knn(q, ldq, nq, r, ldr, nr, d, k, qg, rg, ws, ws_bytes, idx, dist2, seg_cols, phases, None)


BAD_KNN = [
    ("null_q", dict(q=None), -1), ("null_r", dict(r=None), -1), ("null_ws", dict(ws=None), -1), ("null_idx", dict(idx=None), -1),
    ("null_dist2", dict(dist2=None), -1), ("qgroup_alone", dict(qg=PTR), -1), ("rgroup_alone", dict(rg=PTR), -1),
    ("k0", dict(k=0), -1), ("k_neg", dict(k=-1), -1), ("k65", dict(k=65), -2), ("d0", dict(d=0, ldq=0, ldr=0), -1),
    ("d129", dict(d=129, ldq=129, ldr=129), -2), ("nq0", dict(nq=0), -1), ("nr0", dict(nr=0), -1),
    ("nq_above", dict(nq=(1 << 20) + 1), -2), ("nr_above", dict(nr=(1 << 20) + 1), -2), ("ldq_below_d", dict(ldq=9), -1),
    ("ldr_below_d", dict(ldr=9), -1), ("ws_misaligned", dict(ws=PTR + 4), -1), ("seg_cols_neg", dict(seg_cols=-1), -1),
    ("phases_3", dict(seg_cols=0, phases=3), -1), ("ws_short", dict(seg_cols=10, ws_bytes=8 * 10 * 100 * 15 - 1), -4),
    ("ws_empty", dict(ws_bytes=0), -4), ("segments_above_2GiB", dict(nq=1 << 20, nr=1 << 20, k=64, seg_cols=1 << 17), -2),
]


@pytest.mark.parametrize("case,kw,rc", BAD_KNN, ids=[b[0] for b in BAD_KNN])
def test_knn_rejects_bad_arguments(case, kw, rc):
    assert _knn(**kw) == rc, N.lib().mmvae_last_error_string()
    assert N.lib().mmvae_last_error_string()


def _votes(idx=PTR, nq=100, k=15, rlabel=PTR, nr=100, n_classes=7, qlabel=PTR, pred=PTR, purity=PTR, top2=PTR):
    return NB._lib().mmvae_knn_votes(idx, nq, k, rlabel, nr, n_classes, qlabel, pred, purity, top2, None)


BAD_VOTES = [
    ("null_idx", dict(idx=None), -1), ("null_rlabel", dict(rlabel=None), -1), ("null_pred", dict(pred=None), -1),
    ("purity_without_qlabel", dict(qlabel=None), -1), ("k0", dict(k=0), -1), ("k65", dict(k=65), -2), ("classes0", dict(n_classes=0), -1),
    ("classes4097", dict(n_classes=4097), -2), ("nq0", dict(nq=0), -1), ("nr0", dict(nr=0), -1), ("nq_above", dict(nq=(1 << 20) + 1), -2),
]


@pytest.mark.parametrize("case,kw,rc", BAD_VOTES, ids=[b[0] for b in BAD_VOTES])
def test_knn_votes_rejects_bad_arguments(case, kw, rc):
    assert _votes(**kw) == rc, N.lib().mmvae_last_error_string()
    assert N.lib().mmvae_last_error_string()


# ---- 3. the refusals of the public functions ----------------------------------------------------------------------------------
def test_refusals_come_before_any_device_work(monkeypatch):
    """These run without a GPU: nothing below may reach an upload."""
    import torch
    x = np.random.default_rng(0).normal(size=(40, 3))
    y = np.arange(40) % 3
    with pytest.raises(ValueError, match="k = 0 below 1"):
        NB.knn(x, 0)
    with pytest.raises(NotImplementedError, match="k = 65 above 64"):
        NB.knn(x, 65)
    with pytest.raises(ValueError, match="d = 0 below 1"):
        NB.knn(np.zeros((5, 0)), 2)
    with pytest.raises(NotImplementedError, match="d = 129 above 128"):
        NB.knn(np.zeros((5, 129)), 2)
    big = np.lib.stride_tricks.as_strided(np.zeros(1, dtype=np.float32), shape=((1 << 20) + 1, 2), strides=(0, 0))
    with pytest.raises(NotImplementedError, match="n = 1048577 above 1048576"):
        NB.knn(big, 2)
    with pytest.raises(NotImplementedError, match="above 1048576"):
        NB.knn(x, 2, ref=np.lib.stride_tricks.as_strided(np.zeros(1, dtype=np.float32), shape=((1 << 20) + 1, 3), strides=(0, 0)))
    with pytest.raises(ValueError, match="one group array without the other"):
        NB.knn(x, 2, ref=x, groups=np.arange(40))
    with pytest.raises(ValueError, match="one group array without the other"):
        NB.knn(x, 2, ref=x, ref_groups=np.arange(40))
    with pytest.raises(ValueError, match="one group array without the other"):
        NB.knn(x, 2, ref_groups=np.arange(40))
    with pytest.raises(ValueError, match="one group array without the other"):
        NB.knn_device(torch.zeros(4, 2), torch.zeros(4, 2), 2, qgroup=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="groups must be 40 integers"):
        NB.knn(x, 2, groups=np.arange(39))
    with pytest.raises(ValueError, match="exclude_self needs ref=None"):
        NB.knn(x, 2, ref=x, exclude_self=True)
    with pytest.raises(ValueError, match="3 coordinates and ref 4"):
        NB.knn(x, 2, ref=np.zeros((5, 4)))
    with pytest.raises(ValueError, match=r"not \[n, d\]"):
        NB.knn(np.zeros(5), 2)
    broken = x.copy()
    broken[7, 1] = np.nan
    for call in (lambda: NB.knn(broken, 2), lambda: NB.knn(x, 2, ref=broken), lambda: NB.knn_graph(broken, 2),
                 lambda: NB.neighbor_purity(broken, y, 2), lambda: NB.knn_cv_predict(broken, y, 4, 0, k=5),
                 lambda: NB.KNN_classifier(broken, {"a": y}, 4, 0, k=5)):
        with pytest.raises(ValueError, match="holds NaN"):
            call()
    with pytest.raises(ValueError, match="mode"):
        NB.knn_graph(x, 2, mode="umap")
    # a fold that leaves fewer than k training cells, where sklearn raises: 40 cells in 2 folds leave 20
    with pytest.raises(ValueError, match="Expected n_neighbors <= n_samples_fit, but n_neighbors = 21, n_samples_fit = 20"):
        NB.knn_cv_predict(x, y, 2, 0, k=21)
    with pytest.raises(ValueError, match="n_samples_fit = 20"):
        NB.KNN_classifier(x, {"a": y, "b": y}, 2, 0, k=21)
    with pytest.raises(ValueError, match="39 labels for 40 samples"):
        NB.knn_cv_predict(x, y[:39], 4, 0)
    with pytest.raises(ValueError, match="kfold = 1 outside"):
        NB.knn_cv_predict(x, y, 1, 0)
    with pytest.raises(ValueError, match="39 labels for 40 samples"):
        NB.neighbor_purity(x, y[:39], 3)
    with pytest.raises(NotImplementedError, match="classes above 4096"):
        NB.neighbor_purity(np.zeros((5000, 2)), np.arange(5000), 3)
    with pytest.raises(N.NativeError):                                   # no CPU fallback
        NB.knn_device(torch.zeros(5, 3), torch.zeros(5, 3), 2)
    from distributed_vae_amd import dist as DI
    monkeypatch.setattr(DI, "is_dist", lambda: True)
    for call in (lambda: NB.knn(x, 2), lambda: NB.knn_graph(x, 2), lambda: NB.neighbor_purity(x, y, 2),
                 lambda: NB.knn_cv_predict(x, y, 4, 0), lambda: NB.KNN_classifier(x, {"a": y}, 4, 0)):
        with pytest.raises(NotImplementedError, match="not data-parallel"):
            call()


def test_trainer_methods_refuse_before_the_engine(monkeypatch):
    import types
    from distributed_vae_amd import dist as DI
    from distributed_vae_amd.cpl_mixvae import cpl_mixVAE

    def engine(*a, **k):
        raise AssertionError("the engine was reached")
    t = object.__new__(cpl_mixVAE)
    t.n_arm, t.n_categories, t.ref_prior, t.device = 2, 5, False, "cpu"
    monkeypatch.setattr(t, "_encode_all", engine, raising=False)
    plain = types.SimpleNamespace(dataset=range(300), batch_size=64, drop_last=False, __iter__=engine)
    with pytest.raises(ValueError, match="arm = 2"):
        t.latent_neighbors(plain, arm=2)
    with pytest.raises(ValueError, match="on = 'recon'"):
        t.classify_neighbors(plain, np.zeros(300), on="recon")
    monkeypatch.setattr(DI, "is_dist", lambda: True)
    with pytest.raises(NotImplementedError, match="latent_neighbors is not data-parallel"):
        t.latent_neighbors(plain)
    with pytest.raises(NotImplementedError, match="classify_neighbors is not data-parallel"):
        t.classify_neighbors(plain, np.zeros(300))


# ---- 4. the CSR assembly ------------------------------------------------------------------------------------------------------
def test_csr_assembly_on_a_hand_made_index_array():
    idx = np.array([[2, 0, 3], [3, -1, -1], [1, 0, -1], [-1, -1, -1], [4, 2, 1]], dtype=np.int32)
    dist = np.array([[0.5, 1.5, 2.5], [1.0, np.inf, np.inf], [2.0, 3.0, np.inf], [np.inf] * 3, [0.0, 0.25, 4.0]], dtype=np.float32)
    indptr, indices, data = NB.csr_from_neighbors(idx, dist, 5)
    assert indptr.dtype == np.int64 and indices.dtype == np.int32 and data.dtype == np.float32
    assert indptr.tolist() == [0, 3, 4, 6, 6, 9]
    assert indices.tolist() == [0, 2, 3, 3, 0, 1, 1, 2, 4]                   # every row's columns ascend
    assert data.tolist() == [1.5, 0.5, 2.5, 1.0, 3.0, 2.0, 4.0, 0.25, 0.0]
    indptr, indices, ones = NB.csr_from_neighbors(idx, None, 5)
    assert indices.tolist() == [0, 2, 3, 3, 0, 1, 1, 2, 4] and ones.tolist() == [1.0] * 9
    with pytest.raises(IndexError):
        NB.csr_from_neighbors(idx, None, 4)
    with pytest.raises(ValueError):
        NB.csr_from_neighbors(idx, dist[:, :2], 5)
    sparse = pytest.importorskip("scipy.sparse")
    indptr, indices, data = NB.csr_from_neighbors(idx, dist, 5)
    m = NB.to_scipy(indptr, indices, data, 5)
    assert sparse.issparse(m) and m.has_canonical_format and m.shape == (5, 5) and m[4, 2] == 0.25 and m.nnz == 9

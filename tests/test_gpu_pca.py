"""GPU: principal components on the device.  mmvae_gram (the fp64 MFMA), mmvae_symm_mul and mmvae_pca_project through their
wrappers, then ``pca_fit`` / ``pca_transform`` / ``cluster_compare(pca="device")`` / ``cpl_mixVAE.classify_pcs`` against the
numpy restatement (tests/pca_restatement.py) and sklearn's recorded results (tests/golden/pca_cases.npz).

Integer inputs come first: x[r, j] = (3 r + 5 j + r j) mod 7 - 3 with pivot 0 makes every sum an integer that fp64 holds
exactly, so G, s, C Q and (x - mean) V must equal int64 arithmetic bit for bit -- a wrong f64 MFMA lane map (the f32 map
puts three of four results in the wrong row), a wrong tile edge, a wrong segment cut or a lost row cannot hide in a
tolerance.  The shapes sit on both sides of the MFMA tile (16), the workgroup tile (64), the staged chunk (32 rows), every
multiple of the segment length up to three segments, and the 16-row / 64-coordinate blocks of the row kernel.

Bounds (derived in include/mmvae.h, not tuned; u = 2^-53), against np.longdouble on the same doubles t:
  G: (n + 2) u sum_r |t_ri t_rj|;   covariance: 4 (n + 2) kappa u sqrt(var_i var_j) n / (n - 1);
  symm_mul: (D + 1) u sum_j |C_ij Q_jc|;   project: (D + 2) u sum_j |t_j V_jc|.
End to end the gates of tests/test_pca_cpu.py: subspace 2 residual / gap + 4 e_ref, eigenvalues 16 D u lambda_1.

Measured on an MI355X, worst error over gate: G 0.036 (pivot at the mean) and 0.0043 (pivot 0), covariance 0.0090 and 0.0010,
symm_mul 0.070, project 0.030; subspace 0.46 (1.1e-9 against 2.4e-9, the wide input; through eigh 2e-15 .. 1e-14), eigenvalues
0.008, sklearn's recorded components 0.19 and transform 0.18; cluster_compare(pca="device") 1.4e-8 from the recorded returns
against a gate of 1.1e-6; classify_pcs: every prediction equal, smallest margin 4.3e3.  No integer entry off."""
import functools
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pca_restatement as PR  # noqa: E402
import silhouette_restatement as SR  # noqa: E402
from gpu_util import DEV  # noqa: E402
from distributed_vae_amd import _native as N  # noqa: E402
from distributed_vae_amd.utils import cluster_analysis as CA  # noqa: E402
from distributed_vae_amd.utils import pca as P  # noqa: E402

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "pca_cases.npz"))
SIL = np.load(os.path.join(HERE, "golden", "silhouette_kat.npz"))
S = N.GRAM_SEG_ROWS
GRAM_D = (1, 15, 16, 17, 63, 64, 65, 130)


def _t(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)


def _bits(a, b):
    a, b = (v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v) for v in (a, b))
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _exact(got, want_int):
    """A float64 device result against int64 arithmetic: equal, entry for entry."""
    got = got.cpu().numpy()
    return got.dtype == np.float64 and got.shape == want_int.shape and np.array_equal(got, want_int.astype(np.float64))


def test_the_named_switch_points():
    assert (N.GRAM_TILE, N.GRAM_KC, S, N.GRAM_MAX_SEGS, N.PCA_MAX_BLOCK) == (64, 32, 256, 3, 64)
    assert [N.gram_segments(n, 17)[0] for n in (S, S + 1, 2 * S, 2 * S + 1, 3 * S, 3 * S + 1)] == [1, 2, 2, 3, 3, 3]
    assert N.gram_segments(3 * S + 1, 17)[1] == S + 32                        # past three segments they grow by whole chunks


# ---- integer inputs: every sum exact ----------------------------------------------------------------------------------------
def _gram_exact(n, D):
    x = PR.integer_matrix(n, D)
    xi = x.astype(np.int64)
    s, Gm = N.gram(_t(x), torch.zeros(D, device=DEV))
    assert _exact(s, xi.sum(axis=0)), ("s", n, D)
    assert _exact(Gm, xi.T @ xi), ("G", n, D)


@pytest.mark.parametrize("D", GRAM_D)
def test_gram_of_integers_is_exact(D):
    for n in (2, 3, 4, 5, 63, 257):
        _gram_exact(n, D)


@pytest.mark.parametrize("D", (17, 65))
def test_gram_of_integers_is_exact_at_the_segment_edges(D):
    for m in (1, 2, 3):
        for n in (m * S - 1, m * S, m * S + 1):
            _gram_exact(n, D)
    _gram_exact(3 * S + 33, D)                                               # segments of S + 32 and a short last one


def test_gram_covariance_of_integers():
    """cov = 1 on integers: (G - s s^T / n) / (n - 1) formed from exact G and s, so only the finishing arithmetic rounds."""
    n, D = 2 * S + 1, 65
    x = PR.integer_matrix(n, D)
    xi = x.astype(np.int64)
    s, C = N.gram(_t(x), torch.zeros(D, device=DEV), cov=True)
    sf = xi.sum(axis=0).astype(np.float64)
    want = ((xi.T @ xi).astype(np.float64) - np.outer(sf, sf) / n) / (n - 1)
    assert _exact(s, xi.sum(axis=0)) and _bits(C, np.triu(want) + np.triu(want, 1).T)


@pytest.mark.parametrize("D", GRAM_D)
def test_symm_mul_of_integers_is_exact(D):
    Cm = PR.integer_matrix(D, D).astype(np.float64)                          # asymmetric: the kernel reads every entry
    assert D == 1 or not np.array_equal(Cm, Cm.T)
    for b in (1, 8, 9, 32, 64):
        Q = PR.integer_matrix(D, b, shift=2).astype(np.float64)
        Y = N.symm_mul(_t(Cm), _t(Q))
        assert _exact(Y, Cm.astype(np.int64) @ Q.astype(np.int64)), (D, b)


@pytest.mark.parametrize("D", (1, 17, 256, 257, 1030))
def test_project_of_integers_is_exact(D):
    mean = (np.arange(D) % 3 - 1).astype(np.float64)
    for k in (1, 2, 10, 64):
        V = PR.integer_matrix(D, k, shift=4).astype(np.float64)
        for n in (2, 63, 64, 65, 1000):
            x = PR.integer_matrix(n, D, shift=1)
            Z = N.pca_project(_t(x), _t(mean), _t(V))
            assert _exact(Z, (x.astype(np.int64) - mean.astype(np.int64)) @ V.astype(np.int64)), (D, k, n)


def test_rows_past_two_to_the_31_elements():
    """The last rows of a matrix of 2.2e9 floats through a row map: the element offsets do not fit 32 bits."""
    n_total, D = 2_200_000, 1000
    big = torch.empty(n_total, D, device=DEV)
    x = PR.integer_matrix(5, D)
    big[n_total - 5:] = _t(x)
    rows = torch.arange(n_total - 5, n_total, device=DEV)
    xi = x.astype(np.int64)
    s, Gm = N.gram(big, torch.zeros(D, device=DEV), rows)
    assert _exact(s, xi.sum(axis=0)) and _exact(Gm, xi.T @ xi)
    V = PR.integer_matrix(D, 3, shift=4).astype(np.float64)
    Z = N.pca_project(big, torch.zeros(D, dtype=torch.float64, device=DEV), _t(V), rows)
    assert _exact(Z, xi @ V.astype(np.int64))


# ---- the rounding input -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _counts():
    """log1p of sparse counts, float32 [4096, 96]: non-negative, a third zeros, as the expression matrix is."""
    rng = np.random.default_rng(96)
    x = np.log1p(rng.gamma(0.6, 40.0, size=(4096, 96)) * (rng.random((4096, 96)) < 0.67)).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _counts_exact(near):
    x = _counts()
    pivot = x.mean(axis=0, dtype=np.float32) if near else np.zeros(x.shape[1], dtype=np.float32)
    t = PR.t_of(x, pivot)
    s, Gm, A = PR.gram_exact(t)
    cov, var, kappa = PR.covariance_exact(t)
    return pivot, s, Gm, A, cov, var, kappa


# ---- addressing: the same bits as the call on the gathered, aligned copy ------------------------------------------------------
def test_gram_and_project_read_the_matrix_where_it_lies():
    x = _counts()[:700, :70]
    n_total, D = x.shape
    pivot = _t(x.mean(axis=0, dtype=np.float32))
    rows = np.random.default_rng(3).permutation(n_total)[:601]
    mean = _t(x.astype(np.float64).mean(axis=0))
    V = _t(np.linalg.qr(np.random.default_rng(4).normal(size=(D, 7)))[0])
    gathered = _t(np.ascontiguousarray(x[rows]))
    roomy = torch.full((len(rows), D + 2), 1e30, device=DEV)                                             # ld = 72: 16-byte loads,
    roomy[:, :D] = gathered                                                                              # the last quad cut by D
    wide = torch.full((n_total, D + 10), 1e30, device=DEV)                                               # ld > D
    wide[:, :D] = _t(x)
    flat = torch.full((n_total * (D + 3) + 1,), 1e30, device=DEV)                                        # a base off by one float
    odd = flat[1:].view(n_total, D + 3)[:, :D]
    odd.copy_(_t(x))
    assert not N.gram_wide(gathered) and N.gram_wide(roomy) and N.gram_wide(wide) and D % 4 == 2
    assert odd.data_ptr() % 16 != 0 and not N.gram_wide(odd)
    for cov in (False, True):
        want = N.gram(gathered, pivot, cov=cov)
        assert all(_bits(a, b) for a, b in zip(N.gram(_t(x), pivot, _t(rows), cov=cov), want))          # a shuffled subset
        assert all(_bits(a, b) for a, b in zip(N.gram(wide[:, :D], pivot, _t(rows), cov=cov), want))
        assert all(_bits(a, b) for a, b in zip(N.gram(odd, pivot, _t(rows), cov=cov), want))
        for path in ("narrow", "wide"):                                                                    # the load forms
            assert all(_bits(a, b) for a, b in zip(N.gram(roomy[:, :D], pivot, cov=cov, path=path), want))
            assert all(_bits(a, b) for a, b in zip(N.gram(wide[:, :D], pivot, _t(rows), cov=cov, path=path), want))
        with pytest.raises(NotImplementedError):
            N.gram(odd, pivot, _t(rows), path="wide")
    with pytest.raises(ValueError):
        N.gram(_t(x), pivot, path="d16")
    want = N.pca_project(_t(np.ascontiguousarray(x[rows])), mean, V)
    assert _bits(N.pca_project(_t(x), mean, V, _t(rows)), want)
    assert _bits(N.pca_project(wide[:, :D], mean, V, _t(rows)), want) and _bits(N.pca_project(odd, mean, V, _t(rows)), want)
    Cm = N.gram(_t(x), pivot, cov=True)[1]
    Q = _t(np.random.default_rng(5).normal(size=(D, 9)))
    padded = torch.full((D, D + 5), 1e300, dtype=torch.float64, device=DEV)
    padded[:, :D] = Cm
    assert _bits(N.symm_mul(padded[:, :D], Q), N.symm_mul(Cm, Q))


# ---- rounding: against np.longdouble on the same doubles ------------------------------------------------------------------------
@pytest.mark.parametrize("near", (True, False), ids=("pivot_at_the_mean", "pivot_0"))
def test_gram_and_covariance_within_the_derived_bounds(near):
    x = _counts()
    n, D = x.shape
    pivot, s, Gm, A, cov, var, kappa = _counts_exact(near)
    assert N.gram_segments(n, D)[0] == 3
    s_d, G_d = N.gram(_t(x), _t(pivot))
    s_c, C_d = N.gram(_t(x), _t(pivot), cov=True)
    G_h, C_h = G_d.cpu().numpy(), C_d.cpu().numpy()
    assert np.array_equal(G_h, G_h.T) and np.array_equal(C_h, C_h.T) and _bits(s_d, s_c)               # exact symmetry
    again = N.gram(_t(x), _t(pivot)), N.gram(_t(x), _t(pivot), cov=True)
    assert _bits(again[0][1], G_d) and _bits(again[0][0], s_d) and _bits(again[1][1], C_d)             # two runs: the same bits
    e_s = np.abs((s_d.cpu().numpy() - s).astype(np.float64))
    assert (e_s <= (n + 2) * PR.U * np.abs(PR.t_of(x, pivot)).sum(axis=0)).all()
    e_G, gate_G = np.abs((G_h - Gm).astype(np.float64)), PR.gram_gate(n, A)
    e_C, gate_C = np.abs((C_h - cov).astype(np.float64)), PR.covariance_gate(n, var, kappa)
    print(f"near={near}: kappa {kappa.min():.2f} .. {kappa.max():.2f}; G worst error / gate {float((e_G / gate_G).max()):.2e}; "
          f"covariance worst error / gate {float((e_C / gate_C).max()):.2e}")
    assert (e_G <= gate_G).all()
    assert (e_C <= gate_C).all()


def test_symm_mul_and_project_within_the_derived_bounds():
    x = _counts()
    n, D = x.shape
    pivot = _counts_exact(True)[0]
    C_d = N.gram(_t(x), _t(pivot), cov=True)[1]
    rng = np.random.default_rng(11)
    Q = rng.normal(size=(D, 20))
    Y = N.symm_mul(C_d, _t(Q))
    want, A = PR.mul_exact(C_d.cpu().numpy(), Q)
    e, gate = np.abs((Y.cpu().numpy() - want).astype(np.float64)), PR.symm_mul_gate(D, A)
    print(f"symm_mul: worst error / gate {float((e / gate).max()):.2e}")
    assert (e <= gate).all() and _bits(N.symm_mul(C_d, _t(Q)), Y)
    mean = x.astype(np.float64).mean(axis=0)
    V = np.linalg.qr(rng.normal(size=(D, 10)))[0]
    Z = N.pca_project(_t(x), _t(mean), _t(V))
    t = x.astype(np.float64) - mean                                           # the doubles the kernel forms: one rounding each
    want, A = PR.mul_exact(t, V)
    e, gate = np.abs((Z.cpu().numpy() - want).astype(np.float64)), PR.project_gate(D, A)
    print(f"project: worst error / gate {float((e / gate).max()):.2e}")
    assert (e <= gate).all() and _bits(N.pca_project(_t(x), _t(mean), _t(V)), Z)
    for r in (0, 15, 16, 4095):                                               # a row alone, as a matrix of one and through a map
        assert _bits(N.pca_project(_t(x[r:r + 1]), _t(mean), _t(V))[0], Z[r])
        assert _bits(N.pca_project(_t(x), _t(mean), _t(V), torch.tensor([r], device=DEV))[0], Z[r])


# ---- end to end ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(PR.CASES))
def test_pca_fit_within_the_gates(name):
    n, D, k = PR.CASES[name]
    X = G[f"{name}/x"]
    _, ref, lam = PR.eigh_route(X, k)
    e = PR.reference_errors(X, k)
    x64 = X.astype(np.float64)
    norms = np.sqrt(((x64 - x64.mean(axis=0)) ** 2).sum(axis=1))
    for solver in ("subspace", "eigh"):
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            fit = P.pca_fit(X, k, solver=solver)
        if name == "flat" and solver == "subspace":
            assert fit.solver_used == "eigh" and not fit.converged and fit.iterations == 300
            assert any(issubclass(w.category, RuntimeWarning) and "has not converged" in str(w.message) for w in caught)
        else:
            assert fit.solver_used == solver and fit.converged and fit.iterations <= 300 and not caught
        dist, gate = PR.subspace_distance(fit.components, ref), PR.subspace_gate(fit, e["subspace"])
        verr, vgate = float(np.abs(fit.explained_variance - lam[:k]).max()), PR.value_gate(D, lam[0])
        dk = PR.davis_kahan(fit)
        cerr = np.abs(fit.components - G[f"{name}/components"])
        z = P.pca_transform(fit, X)
        zerr, zgate = np.abs(z - G[f"{name}/transform"]), (dk * norms)[:, None] + 4 * e["transform"]
        print(f"{name} {solver}: {fit.iterations} iterations; subspace {dist:.2e} gate {gate:.2e}; eigenvalues {verr:.2e} gate "
              f"{vgate:.2e}; components vs sklearn / gate {float(cerr.max() / (dk + 4 * e['components'])):.2e}; transform vs sklearn "
              f"/ gate {float((zerr / zgate).max()):.2e}")
        assert dist <= gate
        assert verr <= vgate
        assert (cerr <= dk + 4 * e["components"]).all()
        assert (np.abs(fit.explained_variance - G[f"{name}/explained_variance"]) <= fit.residual + vgate + 4 * e["values"]).all()
        assert (np.abs(fit.explained_variance_ratio - G[f"{name}/explained_variance_ratio"])
                <= (fit.residual + vgate) / fit.total_variance + 4 * e["ratio"]).all()
        assert z.dtype == np.float64 and (zerr <= zgate).all()
        at = np.argmax(np.abs(fit.components), axis=1)
        assert (fit.components[np.arange(k), at] > 0).all()                   # the sign convention
        assert np.abs(fit.mean - G[f"{name}/mean"]).max() <= 8 * PR.U * np.abs(X).max()
        again = P.pca_fit(_t(X), k, solver=solver) if not caught else fit     # the device tensor where it lies: the same bits
        assert _bits(again.components, fit.components) and _bits(again.explained_variance, fit.explained_variance)
        zd = P.pca_transform(fit, _t(X), out="device")
        assert zd.dtype == torch.float32 and zd.device.type == "cuda" and _bits(zd, z.astype(np.float32))


def test_pca_project_rows_and_all_components():
    X = G["n<D/x"]
    rows = np.random.default_rng(8).permutation(20)[:15]
    z = P.pca_project(_t(X), 3, rows=rows)
    fit = P.pca_fit(np.ascontiguousarray(X[rows]), 3)
    assert _bits(z, P.pca_transform(fit, np.ascontiguousarray(X[rows])))
    full = P.pca_fit(X[:, :12], 12)                                           # k = D
    assert full.converged and np.isnan(full.gap)
    lam = PR.eigh_route(X[:, :12], 12)[2]
    assert np.abs(full.explained_variance - lam).max() <= PR.value_gate(12, lam[0])


def test_cluster_compare_on_the_device_projection_meets_the_recorded_returns():
    names = [str(v) for v in SIL["cc/names"]]
    labels = {name: SIL[f"cc/labels/{name}"] for name in names}
    num_pc, e_ref = int(SIL["cc/num_pc"]), float(SIL["cc/e_ref"])
    gate = SR.tolerance(num_pc) + e_ref                                       # the gate of the host projection
    for data in (SIL["cc/data"], _t(SIL["cc/data"])):
        fig, smp, sil, c_size = CA.cluster_compare(data, labels, num_pc=num_pc, pca="device")
        if fig is not None:
            import matplotlib.pyplot as plt
            plt.close(fig)
        for i in range(2):
            err = max(float(np.abs(smp[i] - SIL[f"cc/silh_smp_score/{i}"]).max()), abs(float(sil[i]) - float(SIL["cc/sil_score"][i])))
            print(f"cluster_compare(pca='device') {names[i]}: worst |device - recorded| {err:.2e}, gate {gate:.2e}")
            assert err <= gate
            assert np.array_equal(c_size[i], SIL[f"cc/c_size/{i}"])


def test_classify_pcs_equals_the_classifier_on_host_projected_points(monkeypatch):
    from distributed_vae_amd.cpl_mixvae import cpl_mixVAE
    from distributed_vae_amd.utils.dataloader import DeviceLoader
    Dm, n_total, n, num_pc = 40, 400, 300, 4
    rng = np.random.default_rng(13)
    codes = rng.permutation(np.arange(n_total) % 3)
    centres = 12.0 * rng.normal(size=(3, Dm))
    x = (centres[codes] + rng.normal(size=(n_total, Dm))).astype(np.float32)
    labels = np.array([f"blob{v}" for v in codes])
    t = cpl_mixVAE(saving_folder="", device=0, save_flag=False)
    t.init_model(n_categories=5, state_dim=2, input_dim=Dm, fc_dim=32, lowD_dim=6, x_drop=0.5, s_drop=0.2, n_arm=2, temp=1.0,
                 tau=0.005)
    data = _t(x)
    index = torch.from_numpy(rng.permutation(n_total)[:n])
    for shuffle in (False, True):
        dl = DeviceLoader(data, index, 64, shuffle, False, seed=5)
        got = t.classify_pcs(dl, labels, num_pc=num_pc, kfold=3, seed=1, kind="qda")
        assert sorted(got) == ["acc", "data_indx", "fold", "margin", "pred_labels", "ref_labels"]
        rows = got["data_indx"].astype(np.int64)
        assert sorted(rows) == sorted(index.numpy()) and (shuffle or np.array_equal(rows, index.numpy()))
        xs = x[rows]
        mean, comps, lam = PR.eigh_route(xs, num_pc)
        z = PR.transform(xs, mean, comps)
        want = CA.gaussian_cv_predict(z.astype(np.float32), labels[rows], 3, 1, kind="qda")
        # precondition: every margin orders above what the projection can move a score by.  A point moves by at most delta
        # (the subspace gate times the longest row, and one float32 rounding); |W|_2 <= reg^(-1/2) = 10, so
        # q = |W^T (x - mu)|^2 moves by at most 2 |W| sqrt(q) delta and the score by half that
        fit = P.pca_fit(data, num_pc, rows=torch.from_numpy(rows))
        e = PR.reference_errors(xs, num_pc)
        delta = PR.subspace_gate(fit, e["subspace"]) * np.sqrt(((xs.astype(np.float64) - mean) ** 2).sum(axis=1)).max() \
            + 2.0 ** -23 * np.abs(z).max()
        moved = 10.0 * np.sqrt(2.0 * np.abs(want["second"]).max() + 20.0) * delta
        margin = want["best"] - want["second"]
        print(f"classify_pcs shuffle={shuffle}: smallest margin {margin.min():.2e}, a score moves by at most {moved:.2e}")
        assert margin.min() >= 1e3 * moved
        assert np.array_equal(got["fold"], want["fold"])
        assert len(got["acc"]) == len(got["pred_labels"]) == len(got["ref_labels"]) == 3
        n_seen = 0
        for f in range(3):
            test = np.flatnonzero(want["fold"] == f)
            assert np.array_equal(got["pred_labels"][f], want["classes"][want["pred"][test]])      # every cell, none left out
            assert np.array_equal(got["ref_labels"][f], labels[rows][test])
            assert got["acc"][f] == float(np.mean(got["pred_labels"][f] == got["ref_labels"][f]))
            n_seen += len(test)
        assert n_seen == n and np.abs(got["margin"] - margin).max() <= 1e3 * moved
    # the refusals
    with pytest.raises(ValueError, match="every row once"):
        t.classify_pcs(DeviceLoader(data, index, 64, False, True), labels)     # drop_last with a remainder
    with pytest.raises(ValueError, match="kind"):
        t.classify_pcs(DeviceLoader(data, index, 64, False, False), labels, kind="rf")
    monkeypatch.setattr(P.D, "is_dist", lambda: True)
    with pytest.raises(NotImplementedError, match="not data-parallel"):
        t.classify_pcs(DeviceLoader(data, index, 64, False, False), labels)
    with pytest.raises(NotImplementedError, match="not data-parallel"):
        P.pca_fit(data, 2)

"""CPU: the host side of the device PCA (utils/pca.py; csrc/pca.hip).  The host-side contract of mmvae_gram, mmvae_symm_mul
and mmvae_pca_project: declared, exported, ABI version unchanged, the workspace sizes and the segment rule, every bad argument
refused before any device work.  The subspace driver with a numpy multiply in the device's place on the five designed inputs
(tests/pca_restatement.py; recorded with sklearn's results in tests/golden/pca_cases.npz by tools/gen_golden_pca.py), the
sign convention, k = D, a constant column, determinism, the public functions' refusals, and the recorded ``cluster_compare``
returns reproduced through this projection.

Gates (u = 2^-53).  Subspace: |V V^T - V_ref V_ref^T|_2 <= 2 residual / gap + 4 e_ref -- Davis-Kahan with the fit's own
residual and Ritz gap (doubled because the gap is an estimate), plus four times the distance e_ref between numpy's eigh route
and numpy's SVD route on the same input (two independent fp64 computations and the Gram's rounding).  Eigenvalues: within
16 D u lambda_1 of eigh's.  Against the recorded sklearn results the same two terms, entrywise: 2 residual / gap times the
norm of the row being projected (1 for a component) plus 4 e_ref of that quantity; for a variance the first term is the
residual itself (every Ritz value lies within its residual of an eigenvalue) plus the eigenvalue gate.

Measured here (numpy multiply): subspace distance 2.1e-10 .. 1.1e-9 against gates 5.1e-10 .. 5.7e-9 on the four converging
inputs (8, 79, 17, 8 iterations); the flat input does not converge in 300 iterations and comes back through eigh at 9.3e-13
against 1.0e-11; eigenvalues at most 5e-3 of their gate."""
import os
import re
import sys
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pca_restatement as PR  # noqa: E402
import silhouette_restatement as SR  # noqa: E402
import distributed_vae_amd  # noqa: F401,E402
from distributed_vae_amd import _native as N  # noqa: E402
from distributed_vae_amd.utils import cluster_analysis as CA  # noqa: E402
from distributed_vae_amd.utils import pca as P  # noqa: E402

G = np.load(os.path.join(ROOT, "tests", "golden", "pca_cases.npz"))
SIL = np.load(os.path.join(ROOT, "tests", "golden", "silhouette_kat.npz"))


def host_fit(X, k, **kw):
    """``pca_fit`` with numpy in the kernels' place: the pivot is the fp32 column means, the moments are about it."""
    X = np.asarray(X, dtype=np.float32)
    pivot = X.mean(axis=0, dtype=np.float32)
    s, _, C = PR.moments_about(X, pivot)
    mean = pivot.astype(np.float64) + s / X.shape[0]
    return P.fit_from_covariance(lambda Q: C @ Q, lambda: C, mean, float(np.trace(C)), k, **kw)


def quiet_fit(X, k, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return host_fit(X, k, **kw)


# ---- 1. the fixture is what the generator promises -----------------------------------------------------------------------
def test_fixture_is_what_the_generator_promises():
    assert sorted(str(v) for v in G["names"]) == sorted(PR.CASES) and str(G["sklearn"]) and str(G["source"])
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "pca_cases.npz")) < 1024 * 1024
    assert all(G[f].dtype != object for f in G.files)
    for name, (n, D, k) in PR.CASES.items():
        x = G[f"{name}/x"]
        assert x.dtype == np.float32 and x.shape == (n, D)
        assert G[f"{name}/components"].shape == (k, D) and G[f"{name}/transform"].shape == (n, k)
        assert G[f"{name}/explained_variance"].shape == G[f"{name}/explained_variance_ratio"].shape == (k,)
        # the designed spectrum, up to the 2^-12 grid of the recorded input
        r = min(n - 1, D)
        lam = PR.eigh_route(x, k)[2]
        assert np.abs(lam[:r] - PR.spectrum(name, r)).max() <= 1e-4 * lam[0]
        assert np.array_equal(PR.sign_flip(G[f"{name}/components"]), G[f"{name}/components"])       # sklearn's own convention


# ---- 2. the subspace driver on the designed inputs -----------------------------------------------------------------------
@pytest.mark.parametrize("name", PR.CONVERGING)
def test_subspace_iteration_converges_within_the_gate(name):
    n, D, k = PR.CASES[name]
    X = G[f"{name}/x"]
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                          # no fallback, no warning
        fit = host_fit(X, k)
    assert fit.converged and fit.solver_used == "subspace" and 1 <= fit.iterations <= 300
    _, ref, lam = PR.eigh_route(X, k)
    e = PR.reference_errors(X, k)
    dist, gate = PR.subspace_distance(fit.components, ref), PR.subspace_gate(fit, e["subspace"])
    verr, vgate = float(np.abs(fit.explained_variance - lam[:k]).max()), PR.value_gate(D, lam[0])
    print(f"{name}: {fit.iterations} iterations, residual {fit.residual:.2e}, gap {fit.gap:.2e}; subspace {dist:.2e} gate {gate:.2e} "
          f"(e_ref {e['subspace']:.2e}); eigenvalues {verr:.2e} gate {vgate:.2e}")
    assert dist <= gate
    assert verr <= vgate
    # the Ritz gap overestimates the true one (theta_(k+1) <= lambda_(k+1)), by less than the factor 2 the gate allows for it
    true_gap = lam[k - 1] - lam[k]
    assert true_gap * (1 - 1e-9) <= fit.gap <= 2.0 * true_gap and fit.residual <= 1e-10 * lam[0] * np.sqrt(k)
    assert fit.total_variance == pytest.approx(lam.sum(), rel=1e-12)
    assert np.abs(fit.explained_variance_ratio - lam[:k] / lam.sum()).max() <= vgate / lam.sum() + 4 * e["ratio"]
    assert np.abs(fit.components @ fit.components.T - np.eye(k)).max() <= 64 * D * PR.U
    assert np.abs(fit.mean - X.astype(np.float64).mean(axis=0)).max() <= 8 * PR.U * np.abs(X).max()


def test_flat_spectrum_falls_back_to_eigh_with_a_warning():
    n, D, k = PR.CASES["flat"]
    X = G["flat/x"]
    with pytest.warns(RuntimeWarning, match="has not converged"):
        fit = host_fit(X, k)
    assert fit.solver_used == "eigh" and not fit.converged and fit.iterations == 300
    _, ref, lam = PR.eigh_route(X, k)
    e = PR.reference_errors(X, k)
    dist, gate = PR.subspace_distance(fit.components, ref), PR.subspace_gate(fit, e["subspace"])
    print(f"flat: subspace {dist:.2e} gate {gate:.2e} (e_ref {e['subspace']:.2e})")
    assert dist <= gate
    assert np.abs(fit.explained_variance - lam[:k]).max() <= PR.value_gate(D, lam[0])
    direct = host_fit(X, k, solver="eigh")
    assert direct.solver_used == "eigh" and direct.converged and direct.iterations == 0
    assert direct.components.tobytes() == fit.components.tobytes()              # the same route, the same bits


@pytest.mark.parametrize("name", sorted(PR.CASES))
def test_fit_equals_recorded_sklearn(name):
    n, D, k = PR.CASES[name]
    X = G[f"{name}/x"]
    e = PR.reference_errors(X, k)
    x64 = X.astype(np.float64)
    for solver in ("subspace", "eigh"):
        fit = quiet_fit(X, k, solver=solver)
        dk = PR.davis_kahan(fit)
        lam1 = float(G[f"{name}/explained_variance"][0])
        worst = {}
        err = np.abs(fit.components - G[f"{name}/components"])
        worst["components"] = float(err.max() / (dk + 4 * e["components"]))
        assert (err <= dk + 4 * e["components"]).all()
        err = np.abs(fit.explained_variance - G[f"{name}/explained_variance"])
        vgate = fit.residual + PR.value_gate(D, lam1) + 4 * e["values"]
        worst["variance"] = float(err.max() / vgate)
        assert (err <= vgate).all()
        err = np.abs(fit.explained_variance_ratio - G[f"{name}/explained_variance_ratio"])
        assert (err <= vgate / fit.total_variance + 4 * e["ratio"]).all()
        z = PR.transform(x64, fit.mean, fit.components)
        rows = np.sqrt(((x64 - fit.mean) ** 2).sum(axis=1))
        err = np.abs(z - G[f"{name}/transform"])
        zgate = (dk * rows)[:, None] + 4 * e["transform"]
        worst["transform"] = float((err / zgate).max())
        assert (err <= zgate).all()
        assert np.abs(fit.mean - G[f"{name}/mean"]).max() <= 8 * PR.U * np.abs(X).max()
        print(f"{name} {solver}: worst error / gate {worst}")


# ---- 3. conventions and corner cases -----------------------------------------------------------------------------------------
def test_sign_convention():
    c = np.array([[0.1, -0.9, 0.3], [0.5, 0.5, -0.5], [-0.7, 0.7, 0.0], [0.0, 0.0, 0.0]])
    f = P.sign_flip(c)
    assert np.array_equal(f[0], -c[0]) and np.array_equal(f[1], c[1])           # a tie: the lowest index decides
    assert np.array_equal(f[2], -c[2]) and np.array_equal(f[3], c[3])
    assert np.array_equal(f, PR.sign_flip(c))
    for name in ("gap", "wide"):
        fit = host_fit(G[f"{name}/x"], PR.CASES[name][2])
        at = np.argmax(np.abs(fit.components), axis=1)
        assert (fit.components[np.arange(len(at)), at] > 0).all()


def test_all_components_and_a_constant_column():
    X = np.array(G["n<D/x"][:, :12])
    X[:, 7] = 2.5                                                               # a constant column: a zero row of the covariance
    fit = host_fit(X, 12)                                                       # k = D: the block is the whole space
    assert fit.converged and fit.solver_used == "subspace" and np.isnan(fit.gap) and fit.iterations <= 2
    _, ref, lam = PR.eigh_route(X, 12)
    assert np.abs(fit.explained_variance - lam).max() <= PR.value_gate(12, lam[0])
    assert fit.explained_variance[-1] <= PR.value_gate(12, lam[0]) and fit.mean[7] == 2.5
    assert abs(fit.explained_variance_ratio.sum() - 1.0) <= 64 * PR.U
    assert np.abs(fit.components @ fit.components.T - np.eye(12)).max() <= 64 * 12 * PR.U
    few = host_fit(X, 3)
    assert few.converged and np.abs(few.components[:, 7]).max() <= 1e-10        # no weight on the constant column
    e = PR.reference_errors(X, 3)
    assert PR.subspace_distance(few.components, ref[:3]) <= PR.subspace_gate(few, e["subspace"])


def test_two_fits_give_the_same_bits_and_the_seed_matters():
    X = G["gap/x"]
    a, b = host_fit(X, 5), host_fit(X, 5)
    for f in ("mean", "components", "explained_variance", "explained_variance_ratio"):
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes()
    assert (a.residual, a.gap, a.iterations) == (b.residual, b.gap, b.iterations)
    c = host_fit(X, 5, seed=1)
    assert c.components.tobytes() != a.components.tobytes()
    assert PR.subspace_distance(c.components, a.components) <= PR.davis_kahan(a) + PR.davis_kahan(c)


def test_driver_arguments():
    C = np.diag(np.arange(6, 0, -1.0))
    out = P.subspace_iteration(lambda Q: C @ Q, 6, 6, 6)
    assert out["converged"] and np.isnan(out["gap"]) and np.allclose(out["theta"], np.arange(6, 0, -1.0))
    out = P.subspace_iteration(lambda Q: C @ Q, 6, 2, 6)
    assert out["converged"] and out["gap"] == pytest.approx(1.0) and out["iterations"] == 1
    out = P.subspace_iteration(lambda Q: C @ Q, 6, 2, 3, max_iter=1)
    assert out["iterations"] == 1 and not out["converged"] and out["V"].shape == (6, 2)
    with pytest.raises(ValueError):
        P.subspace_iteration(lambda Q: C @ Q, 6, 3, 2)
    with pytest.raises(ValueError, match="solver"):
        P.fit_from_covariance(lambda Q: C @ Q, lambda: C, np.zeros(6), 21.0, 2, solver="randomized")
    with pytest.raises(NotImplementedError):
        P.fit_from_covariance(lambda Q: Q, lambda: None, np.zeros(200), 1.0, 40)       # a block of 80


# ---- 4. the recorded cluster_compare returns through this projection ---------------------------------------------------------
def test_recorded_cluster_compare_is_reproduced_through_the_subspace_projection():
    data, num_pc = SIL["cc/data"], int(SIL["cc/num_pc"])
    fit = host_fit(data, num_pc)
    assert fit.converged
    x64 = data.astype(np.float64)
    z = PR.transform(x64, fit.mean, fit.components)
    # a point moves by at most delta, so a distance by 2 delta, a and b by 2 delta, and s = 1 - a / b (or b / a - 1) by at
    # most 4 delta / max(a, b); the smallest max(a, b) is at least the smallest mean distance of a cell to another cluster
    e = PR.reference_errors(data, num_pc)
    delta = PR.davis_kahan(fit) * np.sqrt(((x64 - fit.mean) ** 2).sum(axis=1)).max() + 4 * e["transform"]
    for i, name in enumerate(str(v) for v in SIL["cc/names"]):
        labels = SIL[f"cc/labels/{name}"]
        _, codes = SR.encode(labels)
        K = int(codes.max()) + 1
        other = SR.cluster_sums(z, codes, K) / np.bincount(codes, minlength=K)
        other[np.arange(len(codes)), codes] = np.inf
        gate = float(SIL["cc/e_ref"]) + 1e-12 + 4 * delta / other.min()
        s = SR.silhouette_samples(z, labels)
        means, sizes = SR.class_means(s, labels)
        print(f"cc {name}: score off by {abs(s.mean() - SIL['cc/sil_score'][i]):.2e}, gate {gate:.2e}")
        assert abs(s.mean() - SIL["cc/sil_score"][i]) <= gate
        assert np.abs(means - SIL[f"cc/silh_smp_score/{i}"]).max() <= gate
        assert np.array_equal(sizes[np.argsort(means)], SIL[f"cc/c_size/{i}"])


# ---- 5. the C boundary ------------------------------------------------------------------------------------------------------
def test_entry_points_declared_exported_and_abi_unchanged():
    hdr = open(os.path.join(ROOT, "include", "mmvae.h")).read()
    for name in ("int mmvae_gram", "int mmvae_debug_gram", "size_t mmvae_gram_workspace_bytes", "int mmvae_gram_segments",
                 "int mmvae_symm_mul", "size_t mmvae_symm_mul_workspace_bytes", "int mmvae_pca_project",
                 "size_t mmvae_pca_project_workspace_bytes"):
        assert re.search(r"\b" + re.escape(name) + r"\(", hdr), name
        assert hasattr(N.lib(), name.split()[1])
    for word in ("v_mfma_f64_16x16x4_f64", "(n + 2) u sum_r |t_ri t_rj|", "(D + 1) u sum_j |C_ij Q_jc|", "(D + 2) u sum_j |t_j V_jc|",
                 "bit-identical", "CALLER'S", "segment order"):
        assert word in hdr, word
    src = open(os.path.join(ROOT, "distributed-vae_amd", "csrc", "api.hip")).read()
    assert "int mmvae_abi_version(void) { return 5; }" in src and N.lib().mmvae_abi_version() == 5 == N.ABI_VERSION
    assert '"pca.hip"' in open(os.path.join(ROOT, "distributed-vae_amd", "build.py")).read()
    kernel = open(os.path.join(ROOT, "distributed-vae_amd", "csrc", "pca.hip")).read()
    assert "__builtin_amdgcn_mfma_f64_16x16x4f64" in kernel and "asm" not in kernel and "atomic" not in kernel.lower().replace("no atomics", "")


def test_launch_constants_are_those_of_the_source():
    hpp = open(os.path.join(ROOT, "distributed-vae_amd", "csrc", "common.hpp")).read()

    def const(name):
        return int(re.search(r"constexpr int " + name + r" = (\d+);", hpp).group(1))
    assert const("GRAM_TILE") == N.GRAM_TILE == 64 and const("GRAM_KC") == N.GRAM_KC == 32
    assert const("GRAM_SEG_ROWS") == N.GRAM_SEG_ROWS == 256 and const("GRAM_MAX_SEGS") == N.GRAM_MAX_SEGS == 3
    assert const("GRAM_FILL_TILES") == N.GRAM_FILL_TILES == 256 and const("GRAM_MAX_D") == N.GRAM_MAX_D == 32768
    assert const("RM_CHUNK") == N.PCA_MAX_BLOCK == P.MAX_COMPONENTS == 64
    assert N.GRAM_SEG_ROWS % N.GRAM_KC == 0 and const("GRAM_PITCH") >= N.GRAM_TILE


def _segments(n, D):
    """The rule of csrc/pca.hip, restated."""
    T = -(-D // 64)
    if T * (T + 1) // 2 >= 256 or n <= 256:
        return 1, n
    rows = 256 if n <= 3 * 256 else -(-(-(-n // 3)) // 32) * 32
    return -(-n // rows), rows


def test_segments_and_workspace_bytes():
    S = N.GRAM_SEG_ROWS
    shapes = [(2, 1), (S, 1), (S + 1, 17), (2 * S, 64), (2 * S + 1, 65), (3 * S, 130), (3 * S + 1, 130), (4096, 96), (22365, 10),
              (22365, 1408), (22365, 1409), (22365, 5032), (1 << 31, 1), (1 << 31, 32768)]
    for n, D in shapes:
        nseg, rows = N.gram_segments(n, D)
        assert (nseg, rows) == _segments(n, D), (n, D)
        assert 1 <= nseg <= N.GRAM_MAX_SEGS and (nseg - 1) * rows < n <= nseg * rows
        ws = N.lib().mmvae_gram_workspace_bytes(n, D)
        assert ws == 8 * ((nseg - 1) * D * D + nseg * D), (n, D)
        assert ws <= 2 * 8 * D * D + 3 * 8 * D                                  # twice G plus the tables, at any shape
    assert [N.gram_segments(n, 96)[0] for n in (S - 1, S, S + 1, 2 * S, 2 * S + 1, 3 * S, 3 * S + 1)] == [1, 1, 2, 2, 3, 3, 3]
    assert N.gram_segments(22365, 5032) == (1, 22365) and N.gram_segments(22365, 10) == (3, 7456)
    for n, D in ((1, 4), (0, 4), (-1, 4), ((1 << 31) + 1, 4), (10, 0), (10, -1), (10, 32769)):
        assert N.lib().mmvae_gram_workspace_bytes(n, D) == 0 and N.gram_segments(n, D) == (0, 0), (n, D)
    assert N.lib().mmvae_symm_mul_workspace_bytes(5032, 20) == 0 and N.lib().mmvae_pca_project_workspace_bytes(22365, 5032, 10) == 0


PTR = 0x1000     # fake device pointers: every case must be refused before anything dereferences them


def _gram(data=PTR, ld=10, n_total=100, rows=PTR, n=100, D=10, pivot=PTR, ws=PTR, ws_bytes=1 << 40, s=PTR, G_=PTR, cov=1, path=-1):
    return N.lib().mmvae_debug_gram(data, ld, n_total, rows, n, D, pivot, ws, ws_bytes, s, G_, cov, path, None)


@pytest.mark.parametrize("case,rc", [
    ("null_data", -1), ("null_pivot", -1), ("null_ws", -1), ("null_s", -1), ("null_G_", -1), ("n1", -1), ("n0", -1),
    ("n_past_2_31", -1), ("n_total0", -1), ("no_rows_n_above_total", -1), ("D0", -1), ("ld_below_D", -1), ("ws_misaligned", -1),
    ("cov2", -1), ("path2", -1), ("path_m2", -1), ("D32769", -2), ("wide_on_odd_ld", -2), ("ws_small", -4)])
def test_gram_rejects_bad_arguments(case, rc):
    kw = {}
    if case.startswith("null_"): kw[case[5:]] = None
    elif case == "n1": kw["n"] = 1
    elif case == "n0": kw["n"] = 0
    elif case == "n_past_2_31": kw["n"] = (1 << 31) + 1
    elif case == "n_total0": kw["n_total"] = 0
    elif case == "no_rows_n_above_total": kw.update(rows=None, n=101)
    elif case == "D0": kw["D"] = 0
    elif case == "ld_below_D": kw["ld"] = 9
    elif case == "ws_misaligned": kw["ws"] = PTR + 4
    elif case == "cov2": kw["cov"] = 2
    elif case == "path2": kw["path"] = 2
    elif case == "path_m2": kw["path"] = -2
    elif case == "D32769": kw.update(D=32769, ld=32769)
    elif case == "wide_on_odd_ld": kw.update(path=1, ld=10)
    elif case == "ws_small": kw.update(n=600, n_total=600, ws_bytes=8 * (2 * 100 + 3 * 10) - 1)
    assert _gram(**kw) == rc, N.lib().mmvae_last_error_string()
    assert N.lib().mmvae_last_error_string()


def _symm(C=PTR, ldc=10, D=10, Q=PTR, b=4, Y=PTR):
    return N.lib().mmvae_symm_mul(C, ldc, D, Q, b, Y, None)


@pytest.mark.parametrize("case,rc", [("null_C", -1), ("null_Q", -1), ("null_Y", -1), ("D0", -1), ("b0", -1), ("ldc_below_D", -1),
                                     ("b65", -2), ("D32769", -2)])
def test_symm_mul_rejects_bad_arguments(case, rc):
    kw = {}
    if case.startswith("null_"): kw[case[5:]] = None
    elif case == "D0": kw["D"] = 0
    elif case == "b0": kw["b"] = 0
    elif case == "ldc_below_D": kw["ldc"] = 9
    elif case == "b65": kw["b"] = 65
    elif case == "D32769": kw.update(D=32769, ldc=32769)
    assert _symm(**kw) == rc, N.lib().mmvae_last_error_string()
    assert N.lib().mmvae_last_error_string()


def _project(data=PTR, ld=10, n_total=100, rows=PTR, n=100, D=10, mean=PTR, V=PTR, k=4, Z=PTR):
    return N.lib().mmvae_pca_project(data, ld, n_total, rows, n, D, mean, V, k, Z, None)


@pytest.mark.parametrize("case,rc", [("null_data", -1), ("null_mean", -1), ("null_V", -1), ("null_Z", -1), ("n0", -1),
                                     ("n_past_2_31", -1), ("n_total0", -1), ("no_rows_n_above_total", -1), ("D0", -1), ("k0", -1),
                                     ("ld_below_D", -1), ("k65", -2)])
def test_pca_project_rejects_bad_arguments(case, rc):
    kw = {}
    if case.startswith("null_"): kw[case[5:]] = None
    elif case == "n0": kw["n"] = 0
    elif case == "n_past_2_31": kw["n"] = (1 << 31) + 1
    elif case == "n_total0": kw["n_total"] = 0
    elif case == "no_rows_n_above_total": kw.update(rows=None, n=101)
    elif case == "D0": kw["D"] = 0
    elif case == "k0": kw["k"] = 0
    elif case == "ld_below_D": kw["ld"] = 9
    elif case == "k65": kw["k"] = 65
    assert _project(**kw) == rc, N.lib().mmvae_last_error_string()
    assert N.lib().mmvae_last_error_string()


def test_python_wrappers_have_no_cpu_fallback():
    import torch
    x = torch.zeros(5, 3)
    with pytest.raises(N.NativeError):
        N.gram(x, torch.zeros(3))
    with pytest.raises(N.NativeError):
        N.symm_mul(torch.zeros(3, 3, dtype=torch.float64), torch.zeros(3, 2, dtype=torch.float64))
    with pytest.raises(N.NativeError):
        N.pca_project(x, torch.zeros(3, dtype=torch.float64), torch.zeros(3, 2, dtype=torch.float64))


# ---- 6. the public functions' refusals: all before any device work (this machine has no device) -----------------------------
def test_refusals():
    x = np.array(G["n<D/x"][:, :6])
    labels = {"a": np.arange(20) % 3}
    with pytest.raises(ValueError, match="n_components"):
        P.pca_fit(x, 0)
    with pytest.raises(ValueError, match="n_components"):
        P.pca_fit(x, 7)
    with pytest.raises(ValueError, match="solver"):
        P.pca_fit(x, 2, solver="randomized")
    with pytest.raises(ValueError, match="not \\[n, D\\]"):
        P.pca_fit(x[:, 0], 1)
    with pytest.raises(ValueError, match="at least two"):
        P.pca_fit(x[:1], 1)
    with pytest.raises(ValueError, match="at least two"):
        P.pca_fit(x, 1, rows=[3])
    with pytest.raises(NotImplementedError):
        P.pca_fit(np.zeros((4, 100), dtype=np.float32), 40)                     # a block of 80 vectors
    bad = x.copy()
    bad[3, 2] = np.nan
    for call in (lambda: P.pca_fit(bad, 2), lambda: P.pca_project(bad, 2), lambda: CA.cluster_compare(bad, labels, 2, pca="device")):
        with pytest.raises(ValueError, match="NaN or infinity"):
            call()
    with pytest.raises(ValueError, match="out"):
        P.pca_project(x, 2, out="torch")
    with pytest.raises(ValueError, match="pca"):
        CA.cluster_compare(x, labels, 2, pca="sklearn")
    with pytest.raises(ValueError, match="num_pc"):
        CA.cluster_compare(x, labels, 7, pca="device")
    with pytest.raises(ValueError, match="num_pc"):
        CA.cluster_compare(x, labels, 0, pca="device")
    with pytest.raises(ValueError, match="Number of labels"):
        CA.cluster_compare(x, {"a": labels["a"], "b": np.zeros(20)}, 2, pca="device")


def test_process_group_is_refused(monkeypatch):
    x = np.array(G["n<D/x"][:, :6])
    fit = host_fit(x, 2)
    monkeypatch.setattr(P.D, "is_dist", lambda: True)
    for call in (lambda: P.pca_fit(x, 2), lambda: P.pca_transform(fit, x), lambda: P.pca_project(x, 2),
                 lambda: CA.cluster_compare(x, {"a": np.arange(20) % 3}, 2, pca="device")):
        with pytest.raises(NotImplementedError, match="not data-parallel"):
            call()


def test_cluster_compare_keeps_its_default():
    import inspect
    sig = inspect.signature(CA.cluster_compare)
    assert list(sig.parameters) == ["data", "labels", "num_pc", "saving_path", "pca"] and sig.parameters["pca"].default == "host"
    assert "plumbing, not a hot path" not in (CA.__doc__ + CA.cluster_compare.__doc__)

"""GPU: the silhouette samples on the device.  mmvae_silhouette and the public ``silhouette_samples`` / ``get_SilhScore`` /
``cluster_compare`` against the fp64 difference-form restatement (tests/silhouette_restatement.py) and against sklearn's
recorded results (tests/golden/silhouette_kat.npz), on the fixture's cases and on the smallest shapes at which the launch can
go wrong: n around a wave and around the 256-row tile, clusters of exactly one segment and one column more, cluster
boundaries on and off the boundaries of an LDS pass, K = 2 and K = n - 1, d on both sides of every switch of the d dispatch.

Bounds (derived, not tuned; u = 2^-24).  An fp32 difference-form distance is off by at most (d / 2 + 2) u relatively: the
subtraction, the d-term sum of non-negative squares and a square root good to 1 ulp.  The fp64 sums add nothing visible, a and
b inherit the bound, the minimum of perturbed values is within it of the true minimum, and s = 1 - a / b or b / a - 1 with the
ratio at most 1, so |ds| <= (d + 4) u.  The gate is twice that, (d + 4) 2^-23, per sample and with none left out, against the
restatement on the same float32 values; against recorded sklearn the case's e_ref is added.  Means of samples (the score, the
per-class means) have the same gate.  Degenerate values are compared exactly.

Measured on an MI355X, worst |device - restatement|: 1e-8 .. 8e-8 over every shape here (d = 1 .. 128) against gates of
6e-7 .. 1.6e-5; an emulation of the fp32 distances on the CPU gave 1e-8 .. 3e-8."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import silhouette_restatement as SR  # noqa: E402
from gpu_util import DEV  # noqa: E402
from distributed_vae_amd import _native as N  # noqa: E402
from distributed_vae_amd.utils import cluster_analysis as CA  # noqa: E402

pytestmark = pytest.mark.gpu

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "silhouette_kat.npz"))
T, ROWS = N.SILHOUETTE_SEG_COLS, N.SILHOUETTE_ROW_TILE


def _pass_cols(d):
    """Columns one LDS pass of the row kernel stages at dimension d."""
    return N.SILHOUETTE_LDS_FLOATS // (4 * N.silhouette_dv(d))


@functools.lru_cache(maxsize=None)
def _blobs(sizes, d, seed=0):
    """float32 blobs, one per cluster of ``sizes`` cells, in shuffled order; (x, labels, the restatement's samples)."""
    rng = np.random.default_rng(1000 * d + len(sizes) + seed)
    labels = rng.permutation(np.repeat(np.arange(len(sizes)), sizes))
    x = (rng.normal(size=(len(sizes), d))[labels] * 1.5 + rng.normal(size=(len(labels), d)) * 0.7).astype(np.float32)
    want = SR.silhouette_samples(x, labels)
    want.setflags(write=False)
    return x, labels, want


def _device(x, labels):
    """mmvae_silhouette through the wrapper, the sorting done here: float64 [n] on the host, in the caller's order."""
    _, codes = SR.encode(labels)
    order = np.argsort(codes, kind="stable")
    offsets = np.concatenate([[0], np.cumsum(np.bincount(codes))]).astype(np.int64)
    perm = torch.from_numpy(order).to(DEV)
    xs = torch.from_numpy(np.ascontiguousarray(x[order])).to(DEV)
    return N.silhouette(xs, torch.from_numpy(offsets).to(DEV), perm).cpu().numpy()


def _check(got, want, d, what, extra=0.0):
    err = float(np.abs(got - want).max())
    gate = SR.tolerance(d) + extra
    print(f"{what}: worst |device - reference| {err:.2e}, gate {gate:.2e}")
    assert got.dtype == np.float64 and got.shape == want.shape and np.isfinite(got).all()
    assert (np.abs(got - want) <= gate).all(), (what, err, gate)


def test_the_named_switch_points():
    assert (T, ROWS) == (512, 256) and _pass_cols(10) == 341 and _pass_cols(128) == 32 and _pass_cols(2) == 1024


# ---- the fixture's cases ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(6))
def test_fixture_cases_against_restatement_and_recorded_sklearn(k):
    x, labels, e_ref = G[f"c{k}/x"], G[f"c{k}/labels"], float(G[f"c{k}/e_ref"])
    d = x.shape[1]
    want = SR.silhouette_samples(x, labels)
    for name, got in (("kernel", _device(x, labels)), ("silhouette_samples", CA.silhouette_samples(x, labels))):
        _check(got, want, d, f"case {k} {name} vs restatement")
        _check(got, G[f"c{k}/samples"], d, f"case {k} {name} vs sklearn", e_ref)
    score = CA.silhouette_score(x, labels)
    assert isinstance(score, float) and abs(score - float(G[f"c{k}/score"])) <= SR.tolerance(d) + e_ref


@pytest.mark.parametrize("k", range(6))
def test_get_silhscore_against_the_recorded_returns(k):
    x, labels, e_ref = G[f"c{k}/x"], G[f"c{k}/labels"], float(G[f"c{k}/e_ref"])
    means, score = CA.get_SilhScore(x.astype(np.float64), labels)          # float64 of float32 values: rounding changes nothing
    _check(means, G[f"c{k}/mean_smp_sc"], x.shape[1], f"case {k} per-class means", e_ref)
    _check(np.asarray(score), G[f"c{k}/sil_score"], x.shape[1], f"case {k} score", e_ref)


def test_cluster_compare_against_the_recorded_returns():
    names = [str(v) for v in G["cc/names"]]
    labels = {name: G[f"cc/labels/{name}"] for name in names}
    num_pc, e_ref = int(G["cc/num_pc"]), float(G["cc/e_ref"])
    fig, smp, sil, c_size = CA.cluster_compare(G["cc/data"], labels, num_pc=num_pc)
    assert len(smp) == len(sil) == len(c_size) == 2
    try:
        import matplotlib.figure
        assert isinstance(fig, matplotlib.figure.Figure) and len(fig.axes[0].lines) == 2
        import matplotlib.pyplot as plt
        plt.close(fig)
    except ImportError:
        assert fig is None
    for i in range(2):
        _check(smp[i], G[f"cc/silh_smp_score/{i}"], num_pc, f"cluster_compare means {names[i]}", e_ref)
        _check(np.asarray(sil[i]), G["cc/sil_score"][i], num_pc, f"cluster_compare score {names[i]}", e_ref)
        assert np.array_equal(c_size[i], G[f"cc/c_size/{i}"])


# ---- the smallest shapes at which the launch can go wrong -------------------------------------------------------------------
EDGE = [
    ((32, 31), 3), ((32, 32), 3), ((33, 32), 3),                            # n = 63, 64, 65: a wave
    ((100, 90, 65), 3), ((100, 90, 66), 3), ((100, 90, 67), 3),             # n = 255, 256, 257: the row tile
    ((T, 9), 10), ((T + 1, 9), 10), ((T - 1, 9), 10),                       # a cluster of one segment, of two, and one short
    ((2 * T, 5, 2 * T + 1), 2),                                             # two and three segments; more than one row tile
    ((341, 342, 340, 1), 10),                                               # d = 10 stages 341 columns a pass: on, past, short
    ((32, 33, 64, 1, 31), 128),                                             # d = 128 stages 32 columns a pass
    ((35, 35), 1), ((2, 97), 7),                                            # K = 2
    ((2,) + (1,) * 68, 4),                                                  # K = n - 1: every cluster but one a singleton
    ((1,) * 40 + (3,), 33),
]


@pytest.mark.parametrize("sizes,d", EDGE, ids=[f"n{sum(s)}_K{len(s)}_d{d}" for s, d in EDGE])
def test_edge_shapes_against_restatement(sizes, d):
    x, labels, want = _blobs(sizes, d)
    got = _device(x, labels)
    _check(got, want, d, f"sizes {sizes[:5]} d {d}")
    singles = np.isin(labels, [k for k, f in enumerate(sizes) if f == 1])
    assert (got[singles] == 0.0).all() and (want[singles] == 0.0).all()


SWITCH_D = (1, 4, 5, 8, 9, 12, 13, 16, 17, 24, 25, 32, 33, 48, 49, 64, 65, 96, 97, 128)


@pytest.mark.parametrize("d", SWITCH_D)
def test_both_sides_of_every_switch_of_the_d_dispatch(d):
    x, labels, want = _blobs((40, 33, 24), d, seed=1)
    got = _device(x, labels)
    _check(got, want, d, f"d {d} (instance {N.silhouette_dv(d)})")
    if N.silhouette_dv(d) < N.SILHOUETTE_DV[-1]:                            # the widest instance has no next one
        # zero coordinates up to the next instance: fma(0, 0, acc) = acc, so another instance gives the same bits
        wide = np.concatenate([x, np.zeros((len(x), 4 * N.silhouette_dv(d) + 1 - d), np.float32)], axis=1)
        assert N.silhouette_dv(wide.shape[1]) > N.silhouette_dv(d)
        assert np.array_equal(_device(wide, labels), got)


def test_strided_rows_and_identity_permutation():
    """ld > d: a column window of a wider matrix is read in place; perm = None writes in sorted order."""
    sizes, d = (70, 3, 60), 10
    x, labels, want = _blobs(sizes, d)
    order = np.argsort(labels, kind="stable")
    offsets = torch.tensor([0, 70, 73, 133], device=DEV)
    wide = torch.full((133, 24), 1e30, device=DEV)                          # what lies beside the window must not be read
    wide[:, 5:5 + d] = torch.from_numpy(x[order]).to(DEV)
    view = wide[:, 5:5 + d]
    assert view.stride() == (24, 1)
    got = N.silhouette(view, offsets)
    _check(got.cpu().numpy(), want[order], d, "strided view")
    assert torch.equal(got, N.silhouette(view.contiguous(), offsets))
    out = torch.empty(133, dtype=torch.float64, device=DEV)
    assert N.silhouette(view, offsets, out=out) is out and torch.equal(out, got)
    with pytest.raises(ValueError):
        N.silhouette(view, offsets, path="lds")


def test_unsorted_string_labels():
    x, labels, want = _blobs((20, 31, 14), 5)
    names = np.array(["zeta", "alpha", "mid"])[labels]
    got = CA.silhouette_samples(x, names)
    _check(got, SR.silhouette_samples(x, names), 5, "string labels")
    # the classes are only names: the same partition under other labels gives the same bits
    assert np.array_equal(got, CA.silhouette_samples(x, labels))


def test_device_tensor_in_place_equals_host_float64():
    x, labels, _ = _blobs((100, 90, 67), 3)
    t = torch.from_numpy(x).to(DEV)
    before = t.clone()
    got = CA.silhouette_samples(t, labels)
    assert torch.equal(t, before)
    assert np.array_equal(got, CA.silhouette_samples(x.astype(np.float64), labels))
    assert np.array_equal(got, CA.silhouette_samples(torch.from_numpy(x), list(labels)))
    with pytest.raises(ValueError):
        CA.silhouette_samples(torch.full_like(t, float("nan")), labels)


# ---- degenerate values: exact ---------------------------------------------------------------------------------------------------
def test_degenerate_values_are_exact():
    rng = np.random.default_rng(3)
    d = 10
    x = rng.normal(size=(90, d)).astype(np.float32)
    labels = np.repeat([0, 1, 2, 3, 4], [30, 20, 20, 19, 1])
    x[labels == 1] = x[30]                                                  # a cluster of identical points: a = 0 < b
    x[labels == 2] = x[50]
    x[labels == 3] = x[50]                                                  # two clusters on one point: a = b = 0
    shuffle = rng.permutation(90)
    x, labels = x[shuffle], labels[shuffle]
    got = CA.silhouette_samples(x, labels)
    assert (got[labels == 1] == 1.0).all()
    assert (got[labels == 2] == 0.0).all() and (got[labels == 3] == 0.0).all()
    assert (got[labels == 4] == 0.0).all()                                  # a singleton
    _check(got, SR.silhouette_samples(x, labels), d, "degenerate")
    # two points per cluster on a line, known answers (a square root of 1 ulp need not be exact on a perfect square: the gate)
    _check(CA.silhouette_samples(np.array([[0.0], [1.0], [4.0], [6.0]]), [0, 0, 1, 1]),
           (np.array([5.0, 4.0, 3.5, 5.5]) - [1, 1, 2, 2]) / [5.0, 4.0, 3.5, 5.5], 1, "line")


# ---- determinism ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes,d", [((T + 1, 9, 300), 10), ((32, 33, 64, 1, 31), 128)])
def test_two_runs_give_the_same_bits(sizes, d):
    x, labels, _ = _blobs(sizes, d)
    order = np.argsort(labels, kind="stable")
    offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)).to(DEV)
    xs, perm = torch.from_numpy(x[order]).to(DEV), torch.from_numpy(order).to(DEV)
    runs = [N.silhouette(xs, offsets, perm) for _ in range(3)]
    assert runs[0].dtype == torch.float64
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])


def test_a_row_does_not_depend_on_the_rows_beside_it():
    """The same cells scored alone in their tile and among others: take a cluster's rows from a run on all cells and from a
    run in which another cluster's cells come first in the sorted order (so the rows sit in other lanes and tiles)."""
    x, labels, _ = _blobs((100, 90, 67), 3)
    got = CA.silhouette_samples(x, labels)
    relabel = np.array([2, 0, 1])[labels]                                   # the same partition, the clusters in another order
    again = CA.silhouette_samples(x, relabel)
    # a, the sums within the own cluster, and b's candidates are added in the same column order within each cluster: same bits
    assert np.array_equal(got, again)


def test_the_cap_on_n_is_refused_by_argument():
    rc = N.lib().mmvae_silhouette(0x1000, 4, (1 << 31) + 1, 4, 0x1000, 5, None, 0x1000, 1 << 40, 0x1000, None)
    assert rc == -1 and b"n outside" in N.lib().mmvae_last_error_string()

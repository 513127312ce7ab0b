"""GPU: the mutual-information evaluation on the device.  mmvae_mutinfo_counts against the numpy restatement
(tests/mutinfo_restatement.py) on both kernel paths, bit for bit; mmvae_ami_binary and the public ``mutinfo`` /
``mutinfo_arms`` / ``avg_consensus`` against the reference's recorded results (tests/golden/mutinfo_kat.npz).

Bounds.  Counts are integer atomics: bit-equal.  The adjusted MI is held, absolutely and per entry, to 16 x the case's
recorded e_ref -- the reference's own distance from exact arithmetic (hypergeometric probabilities from Python integers):
the device's error is of the same kind, nine log-gammas of magnitude lgamma(N + 1) cancelling in every exponent, with the
device's lgamma / log / exp and a different summation order in place of libm's and the serial loop.  Every table compared so
has N >= 8 and |normalizer - EMI| >= 1e-3 (tests/test_mutinfo_cpu.py asserts it; none is left out).

Measured on an MI355X, worst |device - sklearn| (the same in table and per-term mode): 1.0e-15 = 0.82 e_ref (N = 64),
4.0e-15 = 0.83 e_ref (257), 4.1e-15 = 1.40 e_ref (300), 1.4e-14 = 0.77 e_ref (2000), 1.2e-14 = 1.01 e_ref (by hand, N = 5000)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mutinfo_restatement as MR  # noqa: E402
from gpu_util import DEV  # noqa: E402
from distributed_vae_amd import _native as N  # noqa: E402
from distributed_vae_amd import evaluation as EV  # noqa: E402

pytestmark = pytest.mark.gpu

K = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mutinfo_kat.npz"))
GATE = 16
# launch_mi_counts (csrc/mutinfo.hip): a workgroup's LDS histograms hold F * C + C + F 32-bit counts and run while that is at
# most 16384 words (64 KiB): at C = 128, F = 126 is the last shape in LDS (16 382 words), F = 127 the first on global atomics
LDS_MAX_WORDS = N.MUTINFO_LDS_MAX_WORDS
# (A, F, C, n)
SHAPES = [(1, 1, 1, 1), (2, 3, 4, 50), (3, 9, 7, 257), (2, 17, 92, 2000), (3, 130, 128, 5000), (2, 126, 128, 1500),
          (2, 127, 128, 1500)]


def _fits(F, Cc):
    return F * Cc + Cc + F <= LDS_MAX_WORDS


def test_the_named_switch_point():
    assert LDS_MAX_WORDS == 16384 and _fits(126, 128) and not _fits(127, 128) and not _fits(130, 128) and _fits(115, 92)


@functools.lru_cache(maxsize=None)
def _inputs(A, F, Cc, n):
    rng = np.random.default_rng(1000 * F + n)
    base = rng.integers(0, Cc, n)
    lab = np.stack([np.where(rng.random(n) < 0.6, base, rng.integers(0, max(Cc - 2, 1), n)) for _ in range(A)]).astype(np.int32)
    tg = (rng.random((n, F)) < min(0.5, 3.0 / F)).astype(np.uint8)
    if F >= 9:
        tg[:, 2] = 0                                  # a cell type without cells
        tg[:, 5] = 1                                  # and one that every cell has
    return lab, tg, MR.counts(lab, tg, F, Cc)


def _run(lab, tg, Cc, F=None, path="auto", out=None):
    return N.mutinfo_counts(torch.from_numpy(lab).to(DEV), torch.from_numpy(tg).to(DEV), Cc, F, out, path)


def _same(got, want):
    for g, w, name in zip(got, want, ("counts", "t_sum", "p_sum")):
        assert g.dtype == torch.int64 and np.array_equal(g.cpu().numpy(), w), name


@pytest.mark.parametrize("path", ["auto", "lds", "global"])
@pytest.mark.parametrize("A,F,Cc,n", SHAPES)
def test_counts_equal_restatement_on_every_path(A, F, Cc, n, path):
    lab, tg, want = _inputs(A, F, Cc, n)
    if path == "lds" and not _fits(F, Cc):
        with pytest.raises(NotImplementedError):
            _run(lab, tg, Cc, path=path)
        return
    _same(_run(lab, tg, Cc, path=path), want)
    assert int(want[2].sum()) == A * n


@pytest.mark.parametrize("path", ["lds", "global"])
def test_counts_of_int32_targets_and_of_a_wider_matrix(path):
    A, F, Cc, n = 3, 9, 7, 257
    lab, tg, want = _inputs(A, F, Cc, n)
    _same(_run(lab, tg.astype(np.int32) * 7, Cc, path=path), want)          # non-zero = set
    wide = np.concatenate([tg, np.ones((n, 4), np.uint8)], axis=1)          # ldt = 13 > F = 9: the last columns are not read
    _same(_run(lab, wide, Cc, F=F, path=path), want)
    view = torch.from_numpy(wide).to(DEV)[:, :F]                            # a strided view: rows 13 apart
    _same(N.mutinfo_counts(torch.from_numpy(lab).to(DEV), view, Cc, path=path), want)


@pytest.mark.parametrize("path", ["lds", "global"])
def test_out_of_range_labels_are_skipped_and_two_batches_equal_one(path):
    A, F, Cc, n = 2, 17, 92, 2000
    lab, tg, _ = _inputs(A, F, Cc, n)
    lab = lab.copy()
    lab[0, ::7], lab[1, 3::11], lab[1, 0] = Cc, -1, 1 << 30
    want = MR.counts(lab, tg, F, Cc)
    assert int(want[2].sum()) < A * n and np.array_equal(want[1], tg.sum(0))     # t_sum counts every cell, whatever its labels
    _same(_run(lab, tg, Cc, path=path), want)
    cut = 1100                                                              # a chunk boundary (1024) inside the first batch
    out = _run(lab[:, :cut].copy(), tg[:cut], Cc, path=path)
    out = _run(lab[:, cut:].copy(), tg[cut:], Cc, path=path, out=out)
    _same(out, want)


# ---- the adjusted mutual information ---------------------------------------------------------------------------------------
def _ami(tables, n, table):
    """mmvae_ami_binary on a list of (n11, t, p): table k sits at [0, k, k] of an [1, T, T] problem."""
    T = len(tables)
    cnt, ts, ps = np.zeros((1, T, T), np.int64), np.zeros(T, np.int64), np.zeros((1, T), np.int64)
    for k, (n11, t, p) in enumerate(tables):
        cnt[0, k, k], ts[k], ps[0, k] = n11, t, p
    out = N.ami_binary(*(torch.from_numpy(v).to(DEV) for v in (cnt, ts, ps)), n, table=table)
    return out.cpu().numpy()[0][np.arange(T), np.arange(T)]


@pytest.mark.parametrize("table", [True, False], ids=["table", "per_term"])
def test_ami_of_tables_chosen_by_hand(table):
    """N = 5000: one cell set in either or both labelings, all but one, ranges longer than one pass of a wave (t = p = 2500,
    independent and identical), every single-valued special case; a column without cells and counts that are no table: NaN."""
    n, e_ref = int(K["hand/N"]), float(K["hand/e_ref"])
    tables = [tuple(int(v) for v in row) for row in K["hand/tables"]]
    got = _ami(tables + [(0, 10, 0), (5, 3, 10), (0, 3000, 3000), (-1, 5, 5)], n, table)
    err = np.abs(got[:len(tables)] - K["hand/ami"])
    print(f"hand tables ({'table' if table else 'per term'}): worst |device - sklearn| {err.max():.2e} = {err.max() / e_ref:.2f} e_ref")
    assert (err <= GATE * e_ref).all(), err
    assert list(got[len(tables) - 5:len(tables)]) == [0.0, 0.0, 1.0, 1.0, 0.0]      # the special cases: exactly
    assert np.isnan(got[len(tables):]).all()
    assert got[5] > 1 - GATE * e_ref and abs(got[4]) < 1e-3                           # identical halves: 1; independent: ~0


@pytest.mark.parametrize("table", [True, False], ids=["table", "per_term"])
@pytest.mark.parametrize("k", range(4))
def test_ami_of_the_fixture_cases(k, table):
    probs, targets = K[f"c{k}/probs"].astype(np.float64), K[f"c{k}/targets"]
    want, e_ref = K[f"c{k}/mi"], float(K[f"c{k}/e_ref"])
    n, Kc = probs.shape
    F = MR.f_used(targets)
    lab = np.argmax(probs, -1).astype(np.int32)[None]
    cnt, ts, ps = _run(lab, targets, Kc, F=F)
    runs = [N.ami_binary(cnt, ts, ps, n, table=table) for _ in range(2)]
    assert torch.equal(runs[0].view(torch.int64), runs[1].view(torch.int64))          # two runs: the same bits
    got = runs[0].cpu().numpy()[0]
    occ = ps.cpu().numpy()[0] > 0
    assert np.isnan(got[:, ~occ]).all() and not np.isnan(got[:, occ]).any()
    err = np.abs(got[:, occ] - want)
    print(f"case {k} N {n} ({'table' if table else 'per term'}): worst |device - sklearn| {err.max():.2e} = "
          f"{err.max() / e_ref:.2f} e_ref")
    assert (err <= GATE * e_ref).all()


# ---- the public functions -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(4))
def test_mutinfo_and_mutinfo_arms_against_the_fixture(k):
    probs, targets = K[f"c{k}/probs"].astype(np.float64), K[f"c{k}/targets"].astype(np.int64)
    want, e_ref = K[f"c{k}/mi"], float(K[f"c{k}/e_ref"])
    got = EV.mutinfo(probs, targets)
    assert got.shape == want.shape and got.dtype == np.float64
    assert (np.abs(got - want) <= GATE * e_ref).all()
    assert abs(EV.avg(got) - float(K[f"avg{k}"])) <= GATE * e_ref
    # a second arm with the categories rolled by one: the same tables under other names
    Kc = probs.shape[1]
    arms = EV.mutinfo_arms(torch.from_numpy(np.stack([probs, np.roll(probs, 1, axis=1)])).float(), torch.from_numpy(targets))
    assert len(arms) == 2 and np.array_equal(arms[0], got)
    occ = np.unique(np.argmax(probs, -1))
    rolled = np.sort((occ + 1) % Kc)
    cols = [int(np.where(occ == (c - 1) % Kc)[0][0]) for c in rolled]
    assert np.array_equal(arms[1], got[:, cols])
    with pytest.raises(ValueError):
        EV.mutinfo(probs, targets * 2)


@pytest.mark.parametrize("arms", [1, 2, 3])
def test_avg_consensus_equals_the_fixture(arms):
    got = EV.avg_consensus(K[f"cons{arms}/labels"])
    assert got == {"all": float(K[f"cons{arms}/all"]), "pairwise": float(K[f"cons{arms}/pairwise"])}
    assert got == EV.avg_consensus(torch.from_numpy(K[f"cons{arms}/labels"]) * 10.0 - 3.0)   # any values: equal is equal

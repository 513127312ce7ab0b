"""GPU: the state-gene correlation on the device.  mmvae_state_corr, the public ``corr_analysis`` and
``cpl_mixVAE.state_gene_corr`` against the two-pass fp64 restatement (tests/statecorr_restatement.py) and against the
reference's recorded returns (tests/golden/statecorr_kat.npz), on the fixture's cases and on the smallest shapes at which the
launch can go wrong: D around the four-gene lane and the 256-gene tile, row pitches and bases that forbid the 16-byte loads,
n around the 256-row segment, one and many segments, every split of S into passes, groups that are empty, at and past the
`> 4` rule and longer than a segment.

Bound (derived in DESIGN.md section 9e, not tuned; u = 2^-53).  The five sums are fp64 sums of c exact terms: each is off by
at most c u times the sum of the terms' magnitudes.  That puts var_x, var_s and the covariance within (3 c + 3) u kappa of
their scale, kappa = max(1 + mean^2 / var) over the mask, and r, with the division, the square root and the product, within
(6 c + 6) kappa u + 4 u <= 8 (c + 1) kappa u.  The gate is exactly that, per entry and with none left out, against the
restatement on the same float32 values; against the recorded reference the case's e_ref64 (float64 call) or e_ref32 (float32
call) is added.  Zeros (c <= 4) and NaNs (a constant input) are compared exactly, and so are the counts.

Bit-equality claims tested here: the narrow and the 16-byte loads; S states in one call and in S one-state calls; G = 1 and
the ungrouped call; a group of a grouped call and a call on that group's rows alone (a segment starts where its group
starts, so the order of every sum is the same); a row map and the gathered copy; two runs.

Measured on an MI355X, worst |device - restatement| over the finite entries: 7e-16 .. 3.7e-15 on every shape here, against
gates of 1.6e-13 and more on the entries that are not 0 by rule; a numpy emulation of the raw-moment sums gave at most 1 % of
the gate on the fixture's cases."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import statecorr_restatement as SR  # noqa: E402
from gpu_util import DEV  # noqa: E402
from distributed_vae_amd import _native as N  # noqa: E402
from distributed_vae_amd.utils import tree_based_analysis as TA  # noqa: E402

pytestmark = pytest.mark.gpu

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "statecorr_kat.npz"))
SEG, TILE = N.STATECORR_SEG_ROWS, N.STATECORR_TILE


@functools.lru_cache(maxsize=None)
def _data(n, D, S, seed=0):
    """(state float32 [n, S], cell float32 [n, D]): about 75 % exact zeros, some negatives, expression that follows the
    states, states offset from zero."""
    rng = np.random.default_rng(7919 * n + 31 * D + S + seed)
    state = (rng.normal(size=(n, S)) * 0.8 + rng.uniform(-3.0, 3.0, size=S)).astype(np.float32)
    which = np.arange(D) % S
    level = np.abs(rng.normal(size=(n, D))) * 2.0 + 1.0 + rng.normal(size=D) * 0.6 * (state[:, which] - state.mean(0)[which])
    u = rng.random(size=(n, D))
    cell = np.where(u < 0.25, np.maximum(level, 1e-3), np.where(u < 0.31, -np.abs(rng.normal(size=(n, D))), 0.0))
    state.setflags(write=False)
    cell = cell.astype(np.float32)
    cell.setflags(write=False)
    return state, cell


@functools.lru_cache(maxsize=None)
def _want(n, D, S, seed=0):
    state, cell = _data(n, D, S, seed)
    out = SR.state_corr(state, cell)
    for a in out:
        a.setflags(write=False)
    return out


def _t(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)          # a copy: the cached arrays are read-only


def _device(state, cell, rows=None, offsets=None, path="auto"):
    """mmvae_state_corr through the wrapper on host arrays (already ordered by group): (r, count) on the host."""
    r, c = N.state_corr(_t(cell), _t(state), _t(rows), _t(offsets), path=path)
    return r.cpu().numpy(), c.cpu().numpy()


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def _check(got, cnt, want, want_cnt, kappa, what, extra=0.0, absolute=False):
    """Counts, zeros and NaNs exact; every finite entry within the derived gate (+ ``extra``)."""
    assert got.dtype == np.float64 and got.shape == want.shape
    if cnt is not None:
        assert cnt.dtype == np.int64 and np.array_equal(cnt, want_cnt), what
    few = np.broadcast_to((want_cnt <= 4)[:, None, :], want.shape)
    assert (got[few] == 0).all(), what
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got == 0, want == 0), what
    fin = np.isfinite(want)
    gate = SR.tolerance(want_cnt, kappa) + extra
    a, b = (np.abs(got), np.abs(want)) if absolute else (got, want)
    err = np.abs(a - b)
    worst = float(err[fin].max()) if fin.any() else 0.0
    print(f"{what}: worst |device - reference| {worst:.2e}, smallest gate {float(gate[fin].min()) if fin.any() else 0:.2e}, "
          f"largest {float(gate[fin].max()) if fin.any() else 0:.2e}")
    assert (err[fin] <= gate[fin]).all(), (what, worst)
    return float(gate[fin].max()) if fin.any() else 0.0


def test_the_named_switch_points():
    assert (SEG, TILE) == (256, 256)


# ---- the fixture's cases ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(6))
def test_fixture_cases_against_restatement_and_recorded_reference(k):
    state, cell = G[f"c{k}/state"], G[f"c{k}/cell"]
    e32, e64 = float(G[f"c{k}/e_ref32"]), float(G[f"c{k}/e_ref64"])
    S = state.shape[1]
    want, want_cnt, kappa = SR.state_corr(state, cell)
    got, cnt = _device(state, cell)
    _check(got, cnt, want, want_cnt, kappa, f"case {k} kernel vs restatement")
    assert np.array_equal(np.isnan(got[0]), G[f"c{k}/nan"]) and np.array_equal(got[0] == 0, G[f"c{k}/zero"])
    _check(got, cnt, G[f"c{k}/abs64"][None], want_cnt, kappa, f"case {k} kernel vs reference float64", e64, absolute=True)
    _check(got, cnt, G[f"c{k}/abs32"][None], want_cnt, kappa, f"case {k} kernel vs reference float32", e32, absolute=True)
    # the public function: the reference's two returns
    all_corr, all_gene, r, counts = TA.corr_analysis(state, cell, return_r=True)
    assert _same_bits(r, got) and np.array_equal(counts, cnt)
    plain = TA.corr_analysis(state, cell)
    assert len(plain) == 2 and len(all_corr) == len(all_gene) == S
    fin = np.isfinite(want)
    gate = float(SR.tolerance(want_cnt, kappa)[fin].max())                  # sorting is 1-Lipschitz in the maximum norm
    for s in range(S):
        assert all_corr[s].dtype == np.float64 and _same_bits(all_corr[s], np.sort(np.abs(got[0, s])))
        assert _same_bits(plain[0][s], all_corr[s]) and np.array_equal(plain[1][s], all_gene[s])
        assert np.array_equal(all_gene[s], np.argsort(np.abs(got[0, s])))
        for name, e_ref in (("corr64", e64), ("corr32", e32)):
            ref = G[f"c{k}/{name}"][s]
            assert np.array_equal(np.isnan(all_corr[s]), np.isnan(ref))
            both = np.isfinite(ref)
            assert (np.abs(all_corr[s] - ref)[both] <= gate + e_ref).all(), (k, s, name)
        for name, e_ref in (("abs64", e64), ("abs32", e32)):
            theirs = G[f"c{k}/{name}"][s][all_gene[s]]                      # the reference's |r| in the device's order
            n_fin = int(np.isfinite(theirs).sum())
            assert np.isfinite(theirs[:n_fin]).all() and np.isnan(theirs[n_fin:]).all()       # NaN last
            assert (np.diff(theirs[:n_fin]) >= -2 * (gate + e_ref)).all(), (k, s, name)


# ---- the smallest shapes at which the launch can go wrong -------------------------------------------------------------------
EDGE = [(300, 1, 2), (300, 5, 2), (300, TILE - 1, 2), (300, TILE + 1, 2),                    # D: a lane's four genes, the tile
        (SEG - 1, 37, 2), (SEG, 37, 2), (SEG + 1, 37, 2),                                     # n around one segment
        (1500, 600, 2)]                                                                       # many segments, three tiles


@pytest.mark.parametrize("n,D,S", EDGE, ids=[f"n{n}_D{D}_S{S}" for n, D, S in EDGE])
def test_edge_shapes_against_restatement(n, D, S):
    state, cell = _data(n, D, S)
    want, want_cnt, kappa = _want(n, D, S)
    got, cnt = _device(state, cell)
    _check(got, cnt, want, want_cnt, kappa, f"n {n} D {D} S {S}")


@pytest.mark.parametrize("D", [5, TILE + 1, 600])
def test_narrow_loads_give_the_bits_of_the_wide_loads(D):
    """ld > D with ld % 4 != 0 and a base offset by one float take the narrow loads; a padded, aligned copy the 16-byte ones."""
    n, S = 300, 2
    state, cell = _data(n, D, S)
    want, want_cnt, kappa = _want(n, D, S)
    ld = D + 3 if (D + 3) % 4 else D + 5
    flat = torch.full((n * ld + 1,), 1e30, device=DEV)                      # what lies beside the window must not be read
    odd = flat[1:].view(n, ld)[:, :D]
    odd.copy_(_t(cell))
    assert odd.stride() == (ld, 1) and ld % 4 != 0 and odd.data_ptr() % 16 != 0 and not N.state_corr_wide(odd)
    ldp = (D + 3) // 4 * 4 + 4
    padded = torch.full((n, ldp), 1e30, device=DEV)[:, :D]
    padded.copy_(_t(cell))
    assert N.state_corr_wide(padded)
    st = _t(state)
    r_odd, c_odd = N.state_corr(odd, st)
    r_pad, c_pad = N.state_corr(padded, st)
    assert torch.equal(c_odd, c_pad) and _same_bits(r_odd.cpu().numpy(), r_pad.cpu().numpy())
    _check(r_odd.cpu().numpy(), c_odd.cpu().numpy(), want, want_cnt, kappa, f"narrow loads D {D}")
    for path in ("wide", "narrow"):
        r_p, c_p = N.state_corr(padded, st, path=path)
        assert torch.equal(c_p, c_pad) and _same_bits(r_p.cpu().numpy(), r_pad.cpu().numpy()), path
    r_n, _ = N.state_corr(odd, st, path="narrow")
    assert _same_bits(r_n.cpu().numpy(), r_pad.cpu().numpy())
    with pytest.raises(NotImplementedError):
        N.state_corr(odd, st, path="wide")
    with pytest.raises(ValueError):
        N.state_corr(odd, st, path="lds")


@pytest.mark.parametrize("S", [1, 2, 3, 5, 9])
def test_states_in_one_call_equal_one_state_calls(S):
    """S = 3 is a pass of two states and one of one, 5 is four and one, 9 four, four and one: the same bits as S calls."""
    n, D = 700, 70
    state, cell = _data(n, D, S)
    want, want_cnt, kappa = _want(n, D, S)
    data, st = _t(cell), _t(state)
    r, c = N.state_corr(data, st)
    _check(r.cpu().numpy(), c.cpu().numpy(), want, want_cnt, kappa, f"S {S}")
    for s in range(S):
        r1, c1 = N.state_corr(data, st[:, s:s + 1])                         # a strided state: lds = S
        assert torch.equal(c1, c) and _same_bits(r1[:, 0].cpu().numpy(), r[:, s].cpu().numpy()), s


def test_the_state_limit():
    state, cell = _data(300, 5, 2)
    wide_state = torch.zeros(300, N.STATECORR_MAX_S + 1, device=DEV)
    with pytest.raises(NotImplementedError):
        N.state_corr(_t(cell), wide_state)
    full = torch.from_numpy(np.tile(state, (1, N.STATECORR_MAX_S // 2))).to(DEV)
    r, _ = N.state_corr(_t(cell), full)
    got, _ = _device(state, cell)
    assert _same_bits(r[0, :2].cpu().numpy(), got[0]) and _same_bits(r[0, -2:].cpu().numpy(), got[0])


# ---- groups -----------------------------------------------------------------------------------------------------------------
def test_one_group_equals_the_ungrouped_call():
    state, cell = _data(SEG + 1, 37, 2)
    plain = _device(state, cell)
    grouped = _device(state, cell, offsets=np.array([0, SEG + 1], dtype=np.int64))
    assert _same_bits(plain[0], grouped[0]) and np.array_equal(plain[1], grouped[1])


def test_groups_empty_small_and_longer_than_a_segment():
    """Groups of 100, 0, 4, 5, SEG + 44 and 0 cells: an empty group gives zeros, four cells zeros by the `> 4` rule, five cells
    the first values; every group equals, bit for bit, a call on its rows alone, and the restatement within the gate."""
    sizes = np.array([100, 0, 4, 5, SEG + 44, 0])
    n, D, S = int(sizes.sum()), 37, 2
    state, cell = (a.copy() for a in _data(n, D, S, seed=1))
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    cell[offsets[2]:offsets[4], 0] = 1.0 + np.arange(9, dtype=np.float32)   # gene 0 is expressed by every cell of the small groups
    codes = np.repeat(np.arange(len(sizes)), sizes)
    want, want_cnt, kappa = SR.state_corr(state, cell, codes, len(sizes))
    got, cnt = _device(state, cell, offsets=offsets)
    assert got.shape == (6, S, D) and cnt.shape == (6, D)
    _check(got, cnt, want, want_cnt, kappa, "grouped")
    assert not got[1].any() and not cnt[1].any() and not got[5].any() and not cnt[5].any() and not got[2].any()
    assert cnt[2, 0] == 4 and cnt[3, 0] == 5 and np.isfinite(got[3, :, 0]).all() and got[3, :, 0].all()
    for g, f in enumerate(sizes):
        if f:
            alone = _device(state[offsets[g]:offsets[g + 1]], cell[offsets[g]:offsets[g + 1]])
            assert _same_bits(alone[0][0], got[g]) and np.array_equal(alone[1][0], cnt[g]), g
    # the public function: labels of any dtype in any order
    rng = np.random.default_rng(3)
    shuffle = rng.permutation(n)
    names = np.array(["c100", "x", "c4", "c5", "long", "y"])[codes][shuffle]
    corr, gene, r, counts = TA.corr_analysis(state[shuffle], cell[shuffle], groups=names, return_r=True)
    classes = list(np.unique(names))
    assert classes == ["c100", "c4", "c5", "long"] and r.shape == (4, S, D) and len(corr) == len(gene) == 4
    w, wc, kp = SR.state_corr(state[shuffle], cell[shuffle], SR.encode(names)[1], 4)
    _check(r, counts, w, wc, kp, "corr_analysis(groups=)")
    for g in range(4):
        for s in range(S):
            assert _same_bits(corr[g][s], np.sort(np.abs(r[g, s]))) and np.array_equal(gene[g][s], np.argsort(np.abs(r[g, s])))


def test_row_map_equals_the_gathered_copy():
    n_total, D, S = 900, TILE + 1, 2
    state_all, cell = _data(n_total, D, S)
    rng = np.random.default_rng(11)
    rows = rng.permutation(n_total)[:SEG + 77].astype(np.int64)
    state = state_all[rows]
    mapped = _device(state, cell, rows=rows)
    gathered = _device(state, cell[rows])
    assert _same_bits(mapped[0], gathered[0]) and np.array_equal(mapped[1], gathered[1])
    want, want_cnt, kappa = SR.state_corr(state, cell[rows])
    _check(mapped[0], mapped[1], want, want_cnt, kappa, "row map")
    corr, gene, r, counts = TA.corr_analysis(state, cell, rows=rows, return_r=True)
    assert _same_bits(r, mapped[0]) and np.array_equal(counts, mapped[1])
    # with groups: the row map is sorted with the cells
    codes = rng.integers(0, 3, size=len(rows))
    _, _, r_g, c_g = TA.corr_analysis(state, cell, groups=codes, rows=rows, return_r=True)
    _, _, r_h, c_h = TA.corr_analysis(state, cell[rows], groups=codes, return_r=True)
    assert _same_bits(r_g, r_h) and np.array_equal(c_g, c_h)


# ---- determinism ----------------------------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bits():
    state, cell = _data(1500, 600, 2)
    offsets = _t(np.array([0, 7, 700, 700, 1500], dtype=np.int64))
    data, st = _t(cell), _t(state)
    runs = [N.state_corr(data, st, None, offsets) for _ in range(3)]
    assert runs[0][0].dtype == torch.float64 and runs[0][1].dtype == torch.int64
    for r, c in runs[1:]:
        assert _same_bits(r.cpu().numpy(), runs[0][0].cpu().numpy()) and torch.equal(c, runs[0][1])


# ---- the public entries ---------------------------------------------------------------------------------------------------------
def test_host_arrays_and_device_tensors_agree():
    state, cell = _data(300, TILE + 1, 2)
    host = TA.corr_analysis(state.astype(np.float64), cell.astype(np.float64), return_r=True)   # float64 of float32 values
    ts, tc = _t(state), _t(cell)
    before = tc.clone()
    dev = TA.corr_analysis(ts, tc, return_r=True)
    assert torch.equal(tc, before)
    mixed = TA.corr_analysis(torch.from_numpy(state.copy()), tc, return_r=True)
    for other in (dev, mixed):
        assert _same_bits(other[2], host[2]) and np.array_equal(other[3], host[3])
        for s in range(2):
            assert _same_bits(other[0][s], host[0][s]) and np.array_equal(other[1][s], host[1][s])
    window = torch.full((300, TILE + 8), 1e30, device=DEV)                  # a column window of a wider matrix, used in place
    window[:, 3:3 + TILE + 1] = tc
    strided = TA.corr_analysis(ts, window[:, 3:3 + TILE + 1], return_r=True)
    assert _same_bits(strided[2], host[2])


def test_state_gene_corr_equals_corr_analysis_on_encode_dataset():
    from distributed_vae_amd.cpl_mixvae import cpl_mixVAE
    from distributed_vae_amd.utils.dataloader import DeviceLoader
    Dm, Cc, S, A = 256, 6, 2, 2
    t = cpl_mixVAE(saving_folder="", device=0, save_flag=False)
    t.init_model(n_categories=Cc, state_dim=S, input_dim=Dm, fc_dim=32, lowD_dim=6, x_drop=0.5, s_drop=0.2, n_arm=A, temp=1.0,
                 tau=0.005)
    _, cell = _data(400, Dm, S, seed=5)
    host = np.abs(cell) * (cell != 0)                                       # counts-like: non-negative, 70 % zeros
    data = _t(host)
    index = torch.from_numpy(np.random.default_rng(2).permutation(400)[:300])
    dl = DeviceLoader(data, index, 64, False, False)
    enc = t.encode_dataset(dl)
    rows = enc["data_indx"].astype(np.int64)
    assert np.array_equal(rows, index.numpy())
    for arm in range(A):
        got = t.state_gene_corr(dl, arm=arm)
        assert sorted(got) == ["categories", "corr", "n"] and np.array_equal(got["categories"], np.arange(Cc))
        assert got["corr"].shape == (Cc, S, Dm) and got["corr"].dtype == np.float64
        assert got["n"].shape == (Cc, Dm) and got["n"].dtype == np.int64
        labels = enc["predicted_label"][arm].astype(np.int64) - 1
        _, _, r, counts = TA.corr_analysis(enc["state_mu"][arm], host[rows], groups=labels, return_r=True)
        present = np.unique(labels)
        assert _same_bits(got["corr"][present], r) and np.array_equal(got["n"][present], counts)
        absent = np.setdiff1d(np.arange(Cc), present)
        assert not got["corr"][absent].any() and not got["n"][absent].any()  # a category with no cell: a row of zeros
        everything = t.state_gene_corr(dl, arm=arm, by_category=False)
        _, _, r_all, c_all = TA.corr_analysis(enc["state_mu"][arm], host[rows], return_r=True)
        assert list(everything["categories"]) == [-1] and _same_bits(everything["corr"], r_all)
        assert np.array_equal(everything["n"], c_all)
    # a plain loader: the batches' concatenation on the device
    from torch.utils.data import DataLoader, TensorDataset
    plain = DataLoader(TensorDataset(torch.from_numpy(host[rows]), torch.arange(300, dtype=torch.float32)), batch_size=64)
    again = t.state_gene_corr(plain, arm=0)
    first = t.state_gene_corr(dl, arm=0)
    assert _same_bits(again["corr"], first["corr"]) and np.array_equal(again["n"], first["n"])
    with pytest.raises(ValueError):
        t.state_gene_corr(dl, arm=A)

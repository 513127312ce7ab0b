"""-m gpu: mmvae_rank_sum_blocked and the ``block_cells`` keyword of utils.marker_analysis / cpl_mixVAE.category_markers.

Up to the one-call path's 32768 cells the blocked path must give mmvae_rank_sum's BITS in all four outputs (the fp64 sums
through their int64 view), whatever the block is.  Beyond, it is compared with the numpy restatement
(tests/ranksum_restatement.py): the integers equal; sum within (n_g + 2) 2^-53 sum |x| of the longdouble sum (the device adds
exact fp64 terms, at most n_g + 2 roundings), the bound of tests/test_gpu_ranksum.py.  That the blocked identity itself gives
those integers on every case here is checked without a GPU in tests/test_ranksum_blocked_cpu.py.

Shapes (tests/ranksum_blocked_restatement.py): with blocks of 128 cells n = 1, 127, 128, 129 (a last block of one cell), 256,
257, 300; every cell its own group; empty groups and a group across a block edge; D = 1, 65, 513 (the staging tile's 64 genes
and a second gene chunk); 1024 and 1025 cells in one group (RS_BIG, and 512 against 1024 reducing threads) with blocks of 128
and 1024; 3000 cells with one large and small groups; 32768 cells with blocks of 8192 and the default.  Beyond the cap of the
one-call path: 32769 and 65537 cells (a last block of one cell after full default blocks), 40000 cells with the default block
and blocks of 4096, and 1048576 cells, the cap, where the all-tied gene's tie term n^3 - n is a hair under 2^60."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ranksum_blocked_restatement as RB  # noqa: E402
import ranksum_restatement as RR  # noqa: E402
from gpu_util import DEV  # noqa: E402
from distributed_vae_amd.utils import marker_analysis as MA  # noqa: E402
from tests.alloc_guard import guarded  # noqa: E402

pytestmark = pytest.mark.gpu


def _t(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)


def _bits(t):
    return t.contiguous().reshape(-1).view(torch.int64).cpu().numpy()


@functools.lru_cache(maxsize=None)
def _device_case(name):
    """(x on the device, the group-sorted row map, the offsets, eps): made once."""
    x, labels, L, eps = RB.make_case(name)
    order, offsets = RB.group_order(labels, L)
    return _t(x), _t(order), _t(offsets), eps


def _block_arg(n, block):
    """The ``block_cells`` that reaches the blocked path: an int; the default block as the int 32768 where "auto" would take
    the one-call path."""
    return block if block else (RB.DEFAULT_BLOCK if n <= MA.MAX_CELLS else "auto")


def _blocked(name, block):
    xd, rows, offsets, eps = _device_case(name)
    return [_bits(t) for t in MA.rank_sums(xd, rows, offsets, eps, block_cells=_block_arg(xd.shape[0], block))]


BITWISE = [(name, block) for name, case in RB.BITWISE.items() for block in case[5]]


@pytest.mark.parametrize("name,block", BITWISE, ids=[f"{n}-block{b}" for n, b in BITWISE])
def test_bitwise_against_the_one_call_path(name, block):
    xd, rows, offsets, eps = _device_case(name)
    n = xd.shape[0]
    one = [_bits(t) for t in MA.rank_sums(xd, rows, offsets, eps)]
    got = [_bits(t) for t in MA.rank_sums(xd, rows, offsets, eps, block_cells=_block_arg(n, block))]
    for k, (a, b) in enumerate(zip(one, got)):                               # rank_sum2, tie_term, n_pos, sum (as int64 bits)
        assert a.shape == b.shape and np.array_equal(a, b), (name, block, k, int((a != b).sum()))
    assert np.array_equal(one[0], [_bits(t) for t in MA.rank_sums(xd, rows, offsets, eps, block_cells="auto")][0])


def test_row_map_and_strided_view():
    """The case's matrix scattered over the rows of a larger one, itself a column window of a wider one: the same bits."""
    name = "n300_empty_middle_and_end_group_across_a_block_edge"
    x, labels, L, eps = RB.make_case(name)
    n, D = x.shape
    order, offsets = RB.group_order(labels, L)
    xd, rows, offs, _ = _device_case(name)
    want = [_bits(t) for t in MA.rank_sums(xd, rows, offs, eps)]
    rng = np.random.default_rng(5)
    big = rng.normal(size=(n + 77, D + 9)).astype(np.float32)
    where = rng.permutation(n + 77)[:n]
    big[where, 4:4 + D] = x
    view = _t(big)[:, 4:4 + D]
    assert view.stride(0) == D + 9
    got = [_bits(t) for t in MA.rank_sums(view, _t(where[order].astype(np.int64)), offs, eps, block_cells=128)]
    assert all(np.array_equal(a, b) for a, b in zip(want, got))
    # a row-strided view and no row map: the cells already in group order
    sorted_x = np.ascontiguousarray(x[order])
    wide = np.zeros((n, D + 3), dtype=np.float32)
    wide[:, :D] = sorted_x
    got = [_bits(t) for t in MA.rank_sums(_t(wide)[:, :D], None, offs, eps, block_cells=128)]
    assert all(np.array_equal(a, b) for a, b in zip(want, got))


@functools.lru_cache(maxsize=None)
def _reference(name):
    x, labels, L, eps = RB.make_case(name)
    r2, tie, pos, tot, tot_abs = RR.rank_sums(x, labels, L, eps)
    return r2, tie, pos, tot, tot_abs, np.bincount(labels, minlength=L)


BEYOND = [(name, block) for name, case in RB.BEYOND.items() for block in case[5]]


@pytest.mark.parametrize("name,block", BEYOND, ids=[f"{n}-block{b}" for n, b in BEYOND])
def test_beyond_the_old_cap_against_the_restatement(name, block):
    xd, rows, offsets, eps = _device_case(name)
    n, D = xd.shape
    assert n > MA.MAX_CELLS
    r2_ref, tie_ref, pos_ref, tot_ref, tot_abs, n_g = _reference(name)
    r2, tie, pos, tot = (t.cpu().numpy() for t in MA.rank_sums(xd, rows, offsets, eps, block_cells=_block_arg(n, block)))
    assert r2.dtype == np.int64 and tie.dtype == np.int64 and pos.dtype == np.int64 and tot.dtype == np.float64
    assert np.array_equal(r2, r2_ref), (name, int((r2 != r2_ref).sum()))
    assert np.array_equal(tie, tie_ref), (name, tie.tolist(), tie_ref.tolist())
    assert np.array_equal(pos, pos_ref)
    # the all-tied gene (every value 0.75): one run of n ties, every cell at the mid-rank (n + 1) / 2
    assert int(tie[RB.TIED_GENE]) == n ** 3 - n and np.array_equal(r2[:, RB.TIED_GENE], n_g * (n + 1))
    fin = np.isfinite(np.asarray(tot_ref, dtype=np.float64))
    with np.errstate(invalid="ignore"):
        err = np.abs(tot.astype(np.longdouble) - tot_ref)
    bound = (n_g[:, None] + 2) * 2.0 ** -53 * np.asarray(tot_abs, dtype=np.float64)
    print(f"{name} block {block}: worst sum error {float((err[fin] / np.maximum(bound[fin], 1e-300)).max()):.3f} of the bound")
    assert (err[fin] <= bound[fin]).all(), (name, float(err[fin].max()))
    assert np.array_equal(tot[~fin], np.asarray(tot_ref, dtype=np.float64)[~fin], equal_nan=True)


def test_public_layer_auto_at_40000_cells():
    """rank_sum_test(block_cells="auto") through the gates of tests/test_gpu_ranksum.py: U equal, z within 16 2^-53 |z|, p
    within (z^2 + 8) 2^-51 p where p > 1e-300, and the all-zero gene's closed forms."""
    name = "n40000_D7"
    x, labels, L, eps = RB.make_case(name)
    n, D = x.shape
    r2_ref, tie_ref, pos_ref, tot_ref, tot_abs, n_g = _reference(name)
    U_ref, z_ref = RR.z_score(r2_ref, tie_ref, n_g, n)
    p_ref = RR.p_value(z_ref)
    got = MA.rank_sum_test(_device_case(name)[0], labels, groups=np.arange(L), eps=eps, block_cells="auto")
    assert np.array_equal(got["rank_sum2"], r2_ref) and np.array_equal(got["tie_term"], tie_ref) and np.array_equal(got["n"], n_g)
    assert np.array_equal(got["U"], U_ref)
    dz = np.abs(got["z"] - z_ref)
    assert (dz <= 16 * 2.0 ** -53 * np.abs(z_ref)).all(), float(dz.max())
    big = p_ref > 1e-300
    dp = np.abs(got["pval"] - p_ref)[big]
    gate = ((z_ref ** 2 + 8) * 2.0 ** -51 * p_ref)[big]
    print(f"worst p error {float((dp / gate).max()):.3f} of the gate")
    assert (dp <= gate).all()
    d, some = RB.ZERO_GENE, n_g > 0
    assert got["tie_term"][d] == n ** 3 - n and np.array_equal(got["rank_sum2"][:, d], n_g * (n + 1))
    assert not got["z"][:, d].any() and (got["pval"][:, d] == 1.0).all() and (got["pval_adj"][:, d] == 1.0).all()
    assert not got["frac"][some, d].any() and not got["mean"][some, d].any()
    assert not got["frac_rest"][:, d].any() and not got["mean_rest"][:, d].any()
    with pytest.raises(NotImplementedError, match="32768"):                  # without the keyword: refused as before
        MA.rank_sum_test(_device_case(name)[0], labels, groups=np.arange(L), eps=eps)


def test_two_runs_equal_bits():
    for name, block in (("n3000_big_and_small_groups", 128), ("n40000_D7", 4096)):
        a, b = _blocked(name, block), _blocked(name, block)
        assert all(np.array_equal(u, v) for u, v in zip(a, b)), name


@pytest.mark.parametrize("name,block", [("n300_empty_middle_and_end_group_across_a_block_edge", 128), ("n40000_D7", 4096)])
def test_both_forms_of_the_rank_kernel_give_the_same_bits(name, block):
    """mmvae_debug_rank_sum_blocked (the timing tool's entry): form 0, every block's keys copied to LDS, which is the entry's
    own choice, and form 1, the blocks searched where they lie."""
    from distributed_vae_amd import _native as N
    xd, rows, offsets, eps = _device_case(name)
    n, Dm = (int(v) for v in xd.shape)
    G = int(offsets.numel()) - 1
    L = MA._lib()
    want = _blocked(name, block)
    ws_bytes = int(L.mmvae_rank_sum_blocked_workspace_bytes(n, Dm, G, block))
    for form in (0, 1):
        ws = N._workspace(ws_bytes, DEV)
        r2, pos, tot = (MA._buffer((G, Dm), dt, DEV) for dt in (torch.int64, torch.int64, torch.float64))
        tie = MA._buffer((Dm,), torch.int64, DEV)
        N.check(L.mmvae_debug_rank_sum_blocked(N._ptr(xd), int(xd.stride(0)), n, Dm, N._ptr(rows), n, N._ptr(offsets), G, float(eps),
                                               block, N._ptr(ws), ws_bytes, N._ptr(r2), N._ptr(tie), N._ptr(pos), N._ptr(tot), form, 0,
                                               N._stream(DEV)), "mmvae_debug_rank_sum_blocked")
        assert all(np.array_equal(a, _bits(b)) for a, b in zip(want, (r2, tie, pos, tot))), (name, form)


def test_the_allocation_contract(monkeypatch):
    """Plain, then under tests/alloc_guard.py with the fills 0xFF and 0x5A: guards intact, every output bit-equal to the plain
    run (an element left unwritten, or a workspace element read before it is written, would carry the fill into them)."""
    name = RB.GUARDED[0]
    xd, rows, offsets, eps = _device_case(name)
    assert tuple(xd.shape) == (300, 65)
    plain = [t.clone() for t in MA.rank_sums(xd, rows, offsets, eps, block_cells=128)]
    one = MA.rank_sums(xd, rows, offsets, eps)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(plain, one))
    for fill in (0xFF, 0x5A):
        with guarded(["_native"], fill, monkeypatch=monkeypatch) as g:
            got = MA.rank_sums(xd, rows, offsets, eps, block_cells=128)
            g.check()
            assert len(g.allocs) == 5, g.sites()                           # four outputs and the workspace
            assert all(a.view.numel() * 8 == a.nbytes for a in g.allocs)
            for k, (a, b) in enumerate(zip(plain, got)):
                assert a.shape == b.shape and a.dtype == b.dtype
                assert np.array_equal(_bits(a), _bits(b)), (hex(fill), k, int((_bits(a) != _bits(b)).sum()))


def test_category_markers_auto_at_33000_cells():
    from distributed_vae_amd.cpl_mixvae import cpl_mixVAE
    from distributed_vae_amd.utils.dataloader import DeviceLoader
    n, Dm, Cc, A = 33000, 64, 6, 2
    t = cpl_mixVAE(saving_folder="", device=0, save_flag=False)
    t.init_model(n_categories=Cc, state_dim=2, input_dim=Dm, fc_dim=32, lowD_dim=6, x_drop=0.5, s_drop=0.2, n_arm=A, temp=1.0,
                 tau=0.005)
    rng = np.random.default_rng(7)
    host = RR.log1p_like(rng, n, Dm, 0.6)
    dl = DeviceLoader(_t(host), torch.arange(n), 4096, False, False)
    with pytest.raises(NotImplementedError, match="cap of 32768 cells"):
        t.category_markers(dl)
    enc = t.encode_dataset(dl)
    rows = enc["data_indx"].astype(np.int64)
    arm = 1
    got = t.category_markers(dl, arm=arm, n_top=5, block_cells="auto")
    labels = enc["predicted_label"][arm].astype(np.int64) - 1
    want = MA.rank_sum_test(_t(host), labels, groups=np.arange(Cc), rows=rows, block_cells="auto")
    assert got["n"].sum() == n and np.array_equal(got["categories"], np.arange(Cc)) and len(got["markers"]) == Cc
    for k in ("n", "rank_sum2", "tie_term", "U", "z", "pval", "pval_adj", "mean", "mean_rest", "frac", "frac_rest", "logfc"):
        assert np.array_equal(got[k], want[k], equal_nan=True), k
    # and those integers are the restatement's
    r2, tie, _, _, _ = RR.rank_sums(host[rows], labels, Cc)
    assert np.array_equal(got["rank_sum2"], r2) and np.array_equal(got["tie_term"], tie)

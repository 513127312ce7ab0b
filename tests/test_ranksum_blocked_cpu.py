"""CPU: the host side of the blocked rank sums (mmvae_rank_sum_blocked; utils/marker_analysis.py's ``block_cells``).  Declared,
exported, ABI version unchanged; the workspace formula; every bad argument refused before any device work (fake pointers);
the Python refusals with the engine stubbed; and the blocked identity restated in numpy
(tests/ranksum_blocked_restatement.py) against the one-sort restatement (tests/ranksum_restatement.py) on EVERY case of
tests/test_gpu_ranksum_blocked.py: integers, so equality."""
import os
import re
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ranksum_blocked_restatement as RB  # noqa: E402
import ranksum_restatement as RR  # noqa: E402
import distributed_vae_amd  # noqa: F401,E402
from distributed_vae_amd import _native as N  # noqa: E402
from distributed_vae_amd.utils import marker_analysis as MA  # noqa: E402

CAP = 1 << 20


# ---- 1. declared, exported, ABI unchanged -----------------------------------------------------------------------------------
def test_entry_points_declared_exported_and_abi_unchanged():
    hdr = open(os.path.join(ROOT, "include", "mmvae.h")).read()
    assert re.search(r"\bint mmvae_rank_sum_blocked\(", hdr) and re.search(r"\bsize_t mmvae_rank_sum_blocked_workspace_bytes\(", hdr)
    assert re.search(r"#define MMVAE_RANKSUM_BLOCKED_MAX_N \(1 << 20\)", hdr)
    for word in ("lo + hi + 1", "n^3 - n < 2^60", "bit-identical", "CALLER'S CONTRACT", "NaN IS NOT CHECKED FOR",
                 "mmvae_rank_sum_blocked_workspace_bytes(n, D, G, block)"):
        assert word in hdr[hdr.index("rank sums past 32768 cells"):], word
    src = open(os.path.join(ROOT, "distributed-vae_amd", "csrc", "api.hip")).read()
    assert "int mmvae_abi_version(void) { return 5; }" in src
    lib = MA._lib()
    assert lib.mmvae_abi_version() == 5 == N.ABI_VERSION
    assert hasattr(lib, "mmvae_rank_sum_blocked") and hasattr(lib, "mmvae_rank_sum_blocked_workspace_bytes")
    hpp = open(os.path.join(ROOT, "distributed-vae_amd", "csrc", "common.hpp")).read()
    assert "RSB_MAX_N = MMVAE_RANKSUM_BLOCKED_MAX_N" in hpp and "n^3 - n < 2^60" in hpp
    assert int(re.search(r"constexpr int RSB_MIN_BLOCK = (\d+);", hpp).group(1)) == MA.MIN_BLOCK == 128
    assert MA.MAX_CELLS_BLOCKED == CAP == 1048576 and MA.MAX_CELLS == RB.DEFAULT_BLOCK == 32768
    # the signatures are declared beside the one-call entries', not in _native.py (whose entries need a row in alloc_cases.py)
    assert "rank_sum_blocked" not in open(os.path.join(ROOT, "distributed-vae_amd", "_native.py")).read()


# ---- 2. the workspace -------------------------------------------------------------------------------------------------------
def _ws_bytes(n, D):
    """gc genes at a time: three 4-byte [gc][n] arrays and one int64 per tile of 4096 cells; gc shrinks to keep it in 4 GiB."""
    gene = 12 * n + 8 * -(-n // 4096)
    gc = min(D, MA.CHUNK, (1 << 32) // gene)
    return (gc * gene + 7) // 8 * 8


def test_workspace_bytes():
    ws = MA._lib().mmvae_rank_sum_blocked_workspace_bytes
    for n, D, G, block in ((1, 1, 1, 0), (3, 1, 2, 128), (129, 513, 3, 128), (4097, 5, 3, 4096), (22365, 5032, 92, 0),
                           (22365, 5032, 92, 8192), (131072, 5032, 92, 0), (CAP, 3, 3, 0), (CAP, 512, 92, 0),
                           (CAP, 5032, 4096, 0), (CAP, 5032, 4096, 32768)):
        assert ws(n, D, G, block) == _ws_bytes(n, D), (n, D, G, block)
    assert ws(3, 1, 2, 128) == 3 * 12 + 8 + 4                                # 44 bytes, rounded up to whole 8
    assert ws(CAP, 5032, 4096, 0) == 341 * (12 * CAP + 8 * 256) <= 1 << 32   # the gene chunk shrinks: 341 genes, not 512
    assert ws(131072, 5032, 92, 0) == 512 * (12 * 131072 + 8 * 32)
    for bad in ((0, 5, 1, 0), (-1, 5, 1, 0), (CAP + 1, 5, 1, 0), (10, 0, 1, 0), (10, -1, 1, 0), (10, 5, 0, 0), (10, 5, -1, 0),
                (10, 5, 4097, 0), (10, 5, 1, 64), (10, 5, 1, 100), (10, 5, 1, 65536), (10, 5, 1, -128), (10, 5, 1, 1)):
        assert ws(*bad) == 0, bad


# ---- 3. refusals of the entry, before any device work -----------------------------------------------------------------------
PTR = 0x1000     # fake device pointers: every case must be refused before anything dereferences them


def _call(x=PTR, ld=40, n_total=100, D=40, rows=PTR, n=100, offsets=PTR, G=3, eps=0.0, block=0, ws=PTR, ws_bytes=None, r2=PTR,
          tie=PTR, pos=PTR, tot=PTR):
    if ws_bytes is None:
        ws_bytes = _ws_bytes(n, D) if n >= 1 and D >= 1 else 1 << 40
    return MA._lib().mmvae_rank_sum_blocked(x, ld, n_total, D, rows, n, offsets, G, eps, block, ws, ws_bytes, r2, tie, pos, tot, None)


BAD = [
    ("null_x", dict(x=None), -1), ("null_offsets", dict(offsets=None), -1), ("null_ws", dict(ws=None), -1),
    ("null_rank_sum2", dict(r2=None), -1), ("null_tie_term", dict(tie=None), -1), ("null_n_pos", dict(pos=None), -1),
    ("null_sum", dict(tot=None), -1),
    ("n0", dict(n=0), -1), ("n_neg", dict(n=-3), -1),
    ("n_cap_plus_1", dict(n=CAP + 1, n_total=CAP + 5), -2), ("n_cap_plus_1_ws_small", dict(n=CAP + 1, n_total=CAP + 5, ws_bytes=8), -2),
    ("n_2_40", dict(n=1 << 40, n_total=1 << 41, ws_bytes=1 << 50), -2),
    ("n_total0", dict(n_total=0), -1), ("no_rows_n_above_n_total", dict(rows=None, n=101), -1),
    ("D0", dict(D=0), -1), ("D_neg", dict(D=-1), -1), ("G0", dict(G=0), -1), ("G_neg", dict(G=-1), -1), ("G4097", dict(G=4097), -2),
    ("ld_below_D", dict(ld=39), -1), ("eps_nan", dict(eps=float("nan")), -1),
    ("block_64", dict(block=64), -1), ("block_100", dict(block=100), -1), ("block_65536", dict(block=65536), -1),
    ("block_neg", dict(block=-128), -1), ("block_1", dict(block=1), -1),
    ("ws_misaligned", dict(ws=PTR + 4), -1),
    ("ws_one_byte_short", dict(ws_bytes=_ws_bytes(100, 40) - 1), -4), ("ws_empty", dict(ws_bytes=0), -4),
    ("ws_one_byte_short_above_the_old_cap", dict(n=32769, n_total=40000, ws_bytes=_ws_bytes(32769, 40) - 1), -4),
]


@pytest.mark.parametrize("case,kw,rc", BAD, ids=[b[0] for b in BAD])
def test_rank_sum_blocked_rejects_bad_arguments(case, kw, rc):
    assert _call(**kw) == rc, N.lib().mmvae_last_error_string()
    assert N.lib().mmvae_last_error_string()


def test_debug_entry_rejects_a_bad_form_or_phase():
    L = MA._lib()

    def call(form, phases, block=0):
        return L.mmvae_debug_rank_sum_blocked(PTR, 40, 100, 40, PTR, 100, PTR, 3, 0.0, block, PTR, 0, PTR, PTR, PTR, PTR, form, phases,
                                              None)
    for form, phases in ((-2, 0), (2, 0), (0, -1), (0, 4)):
        assert call(form, phases) == -1 and b"form" in N.lib().mmvae_last_error_string()
    for form, phases in ((-1, 0), (0, 0), (1, 0), (1, 3)):                   # these pass on to the workspace check: 0 bytes given
        assert call(form, phases) == -4
    assert call(0, 0, block=100) == -1


def test_the_one_call_entry_still_refuses_32769():
    L = MA._lib()
    assert L.mmvae_rank_sum_workspace_bytes(32769, 5, 1) == 0
    assert L.mmvae_rank_sum(PTR, 40, 40000, 40, PTR, 32769, PTR, 3, 0.0, PTR, 1 << 40, PTR, PTR, PTR, PTR, None) == -2


# ---- 4. the Python refusals, the engine stubbed -----------------------------------------------------------------------------
def test_python_refusals_come_before_the_engine(monkeypatch):
    import torch

    def engine(*a, **k):
        raise AssertionError("the engine was reached")
    monkeypatch.setattr(MA, "_float32_device", engine)
    monkeypatch.setattr(MA, "_lib", engine)
    monkeypatch.setattr(N, "_workspace", engine)
    small = np.zeros((300, 1), dtype=np.float32)
    for bad in (64, 100, 65536, 0, -128, 127, 3.5, "blocks", True):
        with pytest.raises(ValueError, match="block_cells"):
            MA.rank_sum_test(small, np.zeros(300, dtype=np.int64), block_cells=bad)
    big = types.SimpleNamespace(shape=(CAP + 1, 1))                          # (the cap is refused before x is looked at)
    for block in ("auto", 4096):
        with pytest.raises(NotImplementedError, match="1048576"):
            MA.rank_sum_test(big, np.zeros(CAP + 1, dtype=np.int64), block_cells=block)
    # block_cells=None: today's refusal, with a hint at the keyword
    with pytest.raises(NotImplementedError, match="32768") as e:
        MA.rank_sum_test(np.zeros((32769, 1), dtype=np.float32), np.zeros(32769, dtype=np.int64))
    assert "block_cells" in str(e.value)
    # rank_sums: refused after the tensors' checks, which need a device tensor; _block_of is what it calls
    assert MA._block_of(None, 32768, "rank_sum") is None and MA._block_of("auto", 32768, "rank_sum") is None
    assert MA._block_of("auto", 32769, "rank_sum") == 0 and MA._block_of(128, 5, "rank_sum") == 128
    assert MA._block_of(np.int64(32768), CAP, "rank_sum") == 32768
    with pytest.raises(NotImplementedError, match="32768"):
        MA._block_of(None, 32769, "rank_sum")
    with pytest.raises(NotImplementedError, match="1048576"):
        MA._block_of(128, CAP + 1, "rank_sum")
    with pytest.raises(N.NativeError):                                       # no CPU fall-back
        MA.rank_sums(torch.zeros(5, 3), None, torch.tensor([0, 5]), block_cells=128)


def test_category_markers_refusals_with_the_engine_stubbed(monkeypatch):
    from distributed_vae_amd.cpl_mixvae import cpl_mixVAE

    def engine(*a, **k):
        raise AssertionError("the engine was reached")
    t = object.__new__(cpl_mixVAE)
    t.n_arm, t.n_categories, t.ref_prior, t.device = 2, 5, False, "cpu"
    monkeypatch.setattr(t, "_encode_all", engine, raising=False)

    def loader(n):
        return types.SimpleNamespace(dataset=range(n), batch_size=64, drop_last=False, __iter__=engine)
    with pytest.raises(NotImplementedError, match="cap of 32768 cells"):
        t.category_markers(loader(32769))
    for block in ("auto", 1024):
        with pytest.raises(NotImplementedError, match="1048576"):
            t.category_markers(loader(CAP + 1), block_cells=block)
    with pytest.raises(ValueError, match="block_cells"):
        t.category_markers(loader(300), block_cells=100)
    from distributed_vae_amd import cpl_mixvae
    monkeypatch.setattr(cpl_mixvae, "_Replay", engine)
    with pytest.raises(AssertionError, match="the engine was reached"):      # 33000 cells pass the gates with "auto"
        t.category_markers(loader(33000), block_cells="auto")


def test_markers_tool_takes_block_cells():
    src = open(os.path.join(ROOT, "tools", "markers.py")).read()
    assert '"--block-cells"' in src and src.count("block_cells=args.block_cells") == 2


# ---- 5. the blocked identity gives the one-sort restatement's integers, on every case of the GPU test -------------------------
@pytest.mark.parametrize("name", list(RB.CASES))
def test_blocked_restatement_equals_the_restatement(name):
    x, labels, L, eps = RB.make_case(name)
    n, D = x.shape
    assert (n, D) == RB.CASES[name][:2]
    r2, tie, _, _, _ = RR.rank_sums(x, labels, L, eps)
    for block in RB.CASES[name][5]:
        r2_b, tie_b = RB.blocked_rank_sums(x, labels, L, block)
        assert np.array_equal(r2_b, r2) and np.array_equal(tie_b, tie), (name, block)
        assert -(-n // RB.block_len(block)) >= 1
    if D > 6:
        n_g = np.bincount(labels, minlength=L)
        assert tie[RB.ZERO_GENE] == n ** 3 - n and np.array_equal(r2[:, RB.ZERO_GENE], n_g * (n + 1))


def test_the_cases_hold_what_they_are_named_for():
    for name, (n, D, L, absent, zf, blocks) in RB.CASES.items():
        assert all(b == 0 or (128 <= b <= 32768 and b & (b - 1) == 0) for b in blocks), name
        assert (name in RB.BEYOND) == (n > 32768), name
    assert [RB.CASES[k][0] % 128 for k in ("n129_last_block_of_one_cell", "n257")] == [1, 1]
    assert RB.BEYOND["n32769_D3"][0] % 32768 == 1 and RB.BEYOND["n65537_D3"][0] % 32768 == 1
    x, labels, L, _ = RB.make_case("n300_empty_middle_and_end_group_across_a_block_edge")
    order, offsets = RB.group_order(labels, L)
    sizes = np.diff(offsets)
    assert sizes[2] == 0 and sizes[5] == 0 and (sizes[[0, 1, 3, 4]] > 0).all()
    assert any(offsets[g] < 128 < offsets[g + 1] for g in range(L))          # a group with cells on both sides of cell 128
    x, labels, L, _ = RB.make_case("n3000_big_and_small_groups")
    sizes = np.bincount(labels, minlength=L)
    assert sizes.max() > 1024 and sizes.min() <= 1024
    n = 1 << 20
    assert n ** 3 - n < 2 ** 60 and 2 * n + 1 < 2 ** 22 and n * (2 * n + 1) < 2 ** 42

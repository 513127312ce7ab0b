"""The blocked rank-sum identity restated in numpy, and the shapes on which mmvae_rank_sum_blocked is tested.

The n cells of a gene, in the call's group-sorted order, are cut into blocks of L cells (the last one shorter); every block is
sorted on its own; for a cell with value v
    lo = sum over the blocks of searchsorted(block, v, "left"),   hi = sum over the blocks of searchsorted(block, v, "right"),
twice the mid-rank is lo + hi + 1 and the cell adds t^2 - 1, t = hi - lo, to the tie term.  These must be the integers of
tests/ranksum_restatement.py (one sort of the whole column, run lengths for the tie term): tests/test_ranksum_blocked_cpu.py
checks that on every case below, which is what tests/test_gpu_ranksum_blocked.py asks of the device.

A column's distinct values are searched once each (``np.unique``) and the counts spread back to the cells: the same sums."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ranksum_restatement as RR  # noqa: E402

DEFAULT_BLOCK = 32768
ZERO_GENE = 5          # planted wherever D > 6, as in tests/test_gpu_ranksum.py
TIED_GENE = 1          # special_columns: every value 0.75

# name: (n, D, number of labels, labels absent from the cells, share of zeros, the block arguments (0: the default))
# the cases at or below the one-call path's 32768 cells: compared bit for bit with mmvae_rank_sum
BITWISE = {
    "n1": (1, 7, 1, (), 0.0, (128,)),
    "n127": (127, 7, 3, (), 0.6, (128,)),
    "n128": (128, 7, 3, (), 0.6, (128,)),
    "n129_last_block_of_one_cell": (129, 7, 3, (), 0.6, (128,)),
    "n256": (256, 7, 3, (), 0.6, (128,)),
    "n257": (257, 7, 3, (), 0.6, (128,)),
    "n300": (300, 7, 3, (), 0.7, (128,)),
    "n130_every_cell_a_group": (130, 7, 130, (), 0.6, (128,)),
    "n300_empty_middle_and_end_group_across_a_block_edge": (300, 7, 6, (2, 5), 0.6, (128,)),
    "n129_D1": (129, 1, 2, (), 0.5, (128,)),
    "n129_D65": (129, 65, 3, (), 0.7, (128,)),
    "n129_D513_two_chunks": (129, 513, 3, (), 0.7, (128,)),
    "n1024_one_group": (1024, 7, 1, (), 0.7, (128, 1024)),
    "n1025_one_group": (1025, 7, 1, (), 0.7, (128, 1024)),
    "n3000_big_and_small_groups": (3000, 7, 4, (), 0.8, (128, 1024, 0)),
    "n32768_D7": (32768, 7, 5, (1,), 0.7, (8192, 0)),
}
# beyond it: compared with the numpy restatement
BEYOND = {
    "n32769_D3": (32769, 3, 4, (), 0.7, (0,)),                      # 32768 + 1: a last block of one cell
    "n65537_D3": (65537, 3, 4, (), 0.7, (0,)),
    "n40000_D7": (40000, 7, 5, (1,), 0.7, (0, 4096)),
    "n1048576_D3": (1 << 20, 3, 3, (), 0.7, (0,)),                  # the cap: 32 blocks, the all-tied gene's n^3 - n a hair under 2^60
}
CASES = {**BITWISE, **BEYOND}
GUARDED = ("n300_D65_guarded", (300, 65, 5, (), 0.7, (128,)))       # the allocation-contract case
CASES[GUARDED[0]] = GUARDED[1]


def block_len(block):
    return DEFAULT_BLOCK if block == 0 else block


@functools.lru_cache(maxsize=None)
def make_case(name):
    """(x float32 [n, D], labels int64 [n], number of labels, eps): the data of tests/test_gpu_ranksum.py -- log1p_like,
    special_columns, a negated column, an all-zero gene where D > 6, +-inf planted in the last column from 63 cells up; one
    large group and small ones; eps a stored positive value.  Computed once, never modified."""
    n, D, L, absent, zf, _ = CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    x = RR.special_columns(RR.log1p_like(rng, n, D, zf), rng)
    x[:, 0] = -x[:, 0]
    if D > 6:
        x[:, ZERO_GENE] = 0.0
    if n >= 63:
        x[rng.integers(0, n, 3), D - 1] = np.inf
        x[rng.integers(0, n, 3), D - 1] = -np.inf
    present = [g for g in range(L) if g not in absent]
    if L == n:
        labels = rng.permutation(n).astype(np.int64)
    else:
        weights = np.array([1.0 + 5.0 * (k == 0) for k in range(len(present))])
        labels = np.asarray(present, dtype=np.int64)[rng.choice(len(present), size=n, p=weights / weights.sum())]
    stored = np.sort(x[(x > 0) & np.isfinite(x)])
    eps = float(stored[len(stored) // 2]) if len(stored) else 0.0
    x.setflags(write=False)
    labels.setflags(write=False)
    return x, labels, L, eps


def group_order(labels, n_groups):
    """(order int64 [n], offsets int64 [G + 1]): the cells sorted by group (stable), as rank_sum_test sorts them."""
    order = np.argsort(labels, kind="stable").astype(np.int64)
    offsets = np.concatenate([[0], np.cumsum(np.bincount(labels, minlength=n_groups))]).astype(np.int64)
    return order, offsets


def blocked_rank_sums(x, codes, n_groups, block):
    """(rank_sum2 int64 [G, D], tie_term int64 [D]) by the blocked identity with blocks of ``block_len(block)`` cells of the
    group-sorted order."""
    x = np.asarray(x)
    n, D = x.shape
    L = block_len(block)
    order, offsets = group_order(np.asarray(codes), n_groups)
    r2 = np.zeros((n_groups, D), dtype=np.int64)
    tie = np.zeros(D, dtype=np.int64)
    for d in range(D):
        col = x[order, d]
        values, inverse = np.unique(col, return_inverse=True)
        lo = np.zeros(len(values), dtype=np.int64)
        hi = np.zeros(len(values), dtype=np.int64)
        for b0 in range(0, n, L):
            blk = np.sort(col[b0:b0 + L])
            lo += np.searchsorted(blk, values, side="left")
            hi += np.searchsorted(blk, values, side="right")
        lo, hi = lo[inverse.reshape(-1)], hi[inverse.reshape(-1)]
        t = hi - lo
        tie[d] = int((t * t - 1).sum())
        twice = np.concatenate([[0], np.cumsum(lo + hi + 1)])
        r2[:, d] = twice[offsets[1:]] - twice[offsets[:-1]]
    return r2, tie

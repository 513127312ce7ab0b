"""The edge inputs of the random-forest tests, shared by tests/test_forest_cpu.py (which checks on the CPU that each has the
property it is named for) and tests/test_gpu_forest.py.  Everything is cached and read-only; the restated forest of a case is
computed once."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import forest_restatement as FR  # noqa: E402
from gaussclf_inputs import points  # noqa: E402

MAX_K, MAX_D = 128, 128         # FOREST_MAX_K, FOREST_MAX_D (tests/test_forest_cpu.py pins them to the source)
CHAIN_DEPTH = 20                # the chain's trees are deeper than this (a balanced tree of its 100 training rows: 7)

# name: (n, d, K, F, T, kind)
CASES = {
    "n63": (63, 3, 4, 2, 4, "plain"), "n64": (64, 3, 4, 2, 4, "plain"), "n65": (65, 3, 4, 2, 4, "plain"),
    "n256": (256, 3, 4, 2, 4, "plain"), "n257": (257, 3, 4, 2, 4, "plain"),        # bins exact, then shared
    "K2": (130, 5, 2, 2, 4, "plain"),
    "Kmax": (4 * MAX_K, 4, MAX_K, 2, 3, "plain"),
    "d1": (150, 1, 3, 2, 4, "plain"), "d2": (150, 2, 3, 3, 4, "plain"), "d128": (200, MAX_D, 5, 2, 3, "plain"),
    "const_first": (120, 6, 3, 2, 6, "const"),      # d - 1 constant columns: most nodes draw a constant column first
    "clones": (96, 2, 3, 2, 8, "clones"),           # groups of identical rows with different labels: impure leaves
    "chain": (200, 1, 2, 2, 3, "chain"),            # sorted distinct values, alternating labels: deep trees
    "absent": (120, 3, 4, 3, 4, "absent"),          # class 3 only in fold 0's test set
    "plateau": (300, 2, 3, 2, 6, "plateau"),        # few distinct values far apart, and lone values between them
    "T1": (100, 3, 3, 3, 1, "plain"),
    "lone_fold": (90, 2, 3, 2, 5, "lone"),          # F = 2 with a fold of one cell
}


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def case(name):
    """dict: x float32 [n, d], bins uint8 [n, d], codes int64 [n], fold int64 [n], K, F, T, mtry, seed."""
    n, d, K, F, T, kind = CASES[name]
    rng = np.random.default_rng(7919 * n + 31 * d + K)
    x, codes = points(n, d, K, seed=len(name), spread=1.5)
    x, codes = np.array(x), np.array(codes)
    fold = rng.permutation(np.arange(n) % F)
    if kind == "const":
        x[:, 1:] = np.float32(0.25)
    elif kind == "clones":                          # 12 points, 8 copies each; labels 5 : 3 in even groups, 4 : 4 in odd ones
        group = np.arange(n) // 8
        x = x[group * 8]
        within = np.arange(n) % 8
        codes = np.where(group % 2 == 0, np.where(within < 5, 0, 1), np.where(within < 4, 1, 2))
        fold = within % F
    elif kind == "chain":
        x = np.arange(n, dtype=np.float32).reshape(n, 1) * np.float32(0.5)
        codes = np.arange(n) % 2
        fold = (np.arange(n) // 2) % F
    elif kind == "absent":
        codes = np.where(fold == 0, codes, codes % 3)
        codes[np.flatnonzero(fold == 0)[:5]] = 3
    elif kind == "plateau":
        x = (np.floor(x * 0.7) * 8.0).astype(np.float32)                  # a few levels, 8 apart
        lone = rng.choice(n, size=24, replace=False)
        x[lone] += rng.uniform(1.0, 7.0, size=(24, d)).astype(np.float32)  # values of their own, between the levels
    elif kind == "lone":
        fold = np.zeros(n, dtype=np.int64)
        fold[n // 2] = 1
    return {"x": _frozen(x), "bins": _frozen(FR.quantile_bins(x)), "codes": _frozen(codes.astype(np.int64)),
            "fold": _frozen(fold.astype(np.int64)), "K": K, "F": F, "T": T, "mtry": FR.default_mtry(d), "seed": 1000 + len(name)}


@functools.lru_cache(maxsize=None)
def restated(name):
    """(the restated forest of the case (``forest_cv``), the statistics of its trees (``grow``'s stats))."""
    c = case(name)
    stats = {}
    res = FR.forest_cv(c["bins"], c["codes"], c["fold"], c["K"], c["F"], c["T"], c["mtry"], c["seed"], stats=stats)
    for v in (res["pred"], res["best"], res["second"], res["votes"], res["trees"]["count"], *res["trees"]["nodes"]):
        v.setflags(write=False)
    return res, stats

"""The edge inputs of the Gaussian-classifier tests, shared by tests/test_gaussclf_cpu.py (which checks on the CPU the
preconditions the GPU tests lean on) and tests/test_gpu_gaussclf.py.  Everything is cached and read-only."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gaussclf_restatement as GR  # noqa: E402

ROW_TILE, SEG = 64, 256         # GAUSSCLF_ROW_TILE, GAUSSCLF_SEG_ROWS (tests/test_gaussclf_cpu.py pins them to the source)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


@functools.lru_cache(maxsize=None)
def points(n, d, K, seed=0, spread=3.0):
    """(x float32 [n, d], codes int64 [n]): K Gaussian classes with their own scales, every class present."""
    rng = np.random.default_rng(104729 * n + 131 * d + 7 * K + seed)
    codes = rng.permutation(np.arange(n) % K)
    means = rng.normal(size=(K, d)) * spread
    scale = rng.uniform(0.5, 1.5, size=(K, d))
    x = (means[codes] + rng.normal(size=(n, d)) * scale[codes]).astype(np.float32)
    return _frozen(x, codes)


# name: (n, d, K, F, options)
SCORE_CASES = {
    "n63": (ROW_TILE - 1, 3, 4, 1, {}),
    "n64": (ROW_TILE, 3, 4, 1, {}),
    "n65": (ROW_TILE + 1, 3, 4, 1, {}),
    "n200_F3": (200, 10, 5, 3, {}),                         # tiles that straddle two folds
    "lone_fold": (150, 2, 3, 2, {"lone": True}),            # F = 2 with a fold of one cell
    "K2": (130, 12, 2, 2, {}),
    "K16": (150, 2, 16, 1, {}),                             # one class a wave
    "K17": (200, 3, 17, 2, {}),                             # two classes a wave, the last waves without a class
    "K37": (300, 2, 37, 1, {}),                             # three classes a wave, the last wave one
    "absent": (190, 5, 4, 2, {"absent": True}),             # class 1 absent from model 0: c0 = -inf, mu and W NaN
    "rank": (140, 9, 3, 2, {"rank": 4}),                    # W with five zero columns
    "d1": (129, 1, 3, 2, {}),
    "d8": (100, 8, 3, 1, {}),                               # one whole column block, no tail
    "d128": (200, 128, 2, 2, {}),
}


@functools.lru_cache(maxsize=None)
def score_input(name):
    """dict: x float32 [n, d], model int32 [n], mu [F, K, d], W [F, K, d, d], c0 [F, K] and the restatement's scores [n, K],
    pred, best, second and summation gate [n, K] for them.  Model f is a QDA model of a subset of the cells."""
    n, d, K, F, opt = SCORE_CASES[name]
    x, codes = points(n, d, K, seed=len(name))
    rng = np.random.default_rng(n + d)
    if opt.get("lone"):
        fold = np.zeros(n, dtype=np.int64)
        fold[n // 2] = 1
    else:
        fold = rng.permutation(np.arange(n) % F)
    mu, W, c0 = np.zeros((F, K, d)), np.zeros((F, K, d, d)), np.zeros((F, K))
    for f in range(F):                                      # model f: fitted to the cells whose index is not f mod F + 1
        mu[f], W[f], c0[f], _ = GR.qda_from_stats(*GR.fold_stats(x, codes, K, np.arange(n) % (F + 1), f))
    if opt.get("rank"):
        W[..., opt["rank"]:] = 0.0
    if opt.get("absent"):
        c0[0, 1], mu[0, 1], W[0, 1] = -np.inf, np.nan, np.nan
    sc, gate = np.zeros((n, K)), np.zeros((n, K))
    for f in range(F):
        rows = np.flatnonzero(fold == f)
        with np.errstate(invalid="ignore"):
            s, A = GR.scores(x[rows], mu[f], W[f], c0[f])
        sc[rows] = s
        gate[rows] = np.where(np.isfinite(s), GR.tolerance_sum(d, np.where(np.isfinite(s), A, 0.0), c0[f][None]), 0.0)
    pred, best, second = GR.best_two(sc)
    return {k: _frozen(v) for k, v in dict(x=x, model=fold.astype(np.int32), mu=mu, W=W, c0=c0, scores=sc, gate=gate, pred=pred,
                                           best=best, second=second).items()}


def decided(case):
    """The cells whose restated margin exceeds twice the largest gate of their row: the device must give their label."""
    return (case["best"] - case["second"]) > 2.0 * case["gate"].max(axis=1)


# name: (group sizes, d)
MOMENT_CASES = {
    "n63": ((63,), 3), "n64": ((64,), 3), "n65": ((65,), 3),
    "segments": ((SEG, SEG + 1, SEG - 1, 1, 0, 2 * SEG + 5, 0), 10),
    "d1": ((70, 0, 5), 1), "d2": ((300, 33), 2), "d128": ((40, 140), 128),
    "d16": ((90, 1), 16), "d17": ((90, 1), 17), "d32": ((90, 1), 32), "d33": ((90, 1), 33), "d64": ((90, 1), 64),
    "d65": ((90, 1), 65),
}


@functools.lru_cache(maxsize=None)
def moment_input(name, far=False):
    """dict: x float32 [n, d] ordered by group, offsets int64 [G + 1], pivot float32 [d] (the data's mean, or with ``far`` a
    point 100 standard deviations away: kappa about 1e4) and per group the two-pass count, mean and scatter."""
    sizes, d = MOMENT_CASES[name]
    n = int(np.sum(sizes))
    x, _ = points(n, d, 3, seed=17)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    pivot = x.astype(np.float64).mean(axis=0)
    if far:
        pivot = pivot + 100.0 * x.astype(np.float64).std(axis=0)
    pivot = pivot.astype(np.float32)
    stats = [GR.two_pass(x[offsets[g]:offsets[g + 1]]) for g in range(len(sizes))]
    return {"x": x, "offsets": _frozen(offsets), "pivot": _frozen(pivot), "stats": stats}


def unpack(M, d):
    """The packed upper triangles [G, d (d + 1) / 2] as full symmetric matrices [G, d, d]."""
    iu = np.triu_indices(d)
    full = np.zeros((M.shape[0], d, d))
    full[:, iu[0], iu[1]] = M
    full[:, iu[1], iu[0]] = M
    return full


def emulate_moments(x, offsets, pivot):
    """numpy fp64 (s [G, d], M packed [G, d (d + 1) / 2]) about ``pivot``: the definition, in numpy's summation order."""
    d = x.shape[1]
    iu = np.triu_indices(d)
    t = x.astype(np.float64) - pivot.astype(np.float64)
    G = len(offsets) - 1
    s, M = np.zeros((G, d)), np.zeros((G, len(iu[0])))
    for g in range(G):
        tg = t[offsets[g]:offsets[g + 1]]
        s[g] = tg.sum(axis=0)
        M[g] = (tg.T @ tg)[iu]
    return s, M

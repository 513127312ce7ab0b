"""Bit identity of the device analysis routines across builds: silhouette, state-gene correlation, the Gaussian classifiers'
group moments and scores, the Gram matrix, the PCA projection, data preparation, the rank sums and k nearest neighbours
(csrc/silhouette.hip, statecorr.hip, gaussclf.hip, pca.hip, dataprep.hip, ranksum.hip, knn.hip, the segment table,
csrc/segments.hip, and the distance, csrc/pairdist.hpp, that some of them share).

Every case calls the wrappers of distributed_vae_amd._native (the rank sums and k-NN: those of utils.marker_analysis and
utils.neighbors) on inputs drawn from a seeded numpy.random.Generator(PCG64) and
takes the SHA-256 of the raw bytes of every output tensor.  The kernels use no atomics and add in a fixed order, so equal
digests are the gate of a change that must not alter what they compute.

    MMVAE_LIB=<the parent commit's libmmvae_hip.so> python tools/analysis_bits.py --write --parent <its hash>

writes tests/golden/analysis_bits.npz (digests, shapes and the parent's hash only) with the library of the commit a change
must stay bit-identical to; tests/test_gpu_analysis_bits.py recomputes the digests with the tree's library and compares.
Without --write the tool prints each case's verdict.

The cases are the smallest shapes at which the shared pieces can go wrong:
  * silhouette: clusters of 1, 511, 512, 513, 0 and 1025 cells -- a singleton, both sides of SIL_SEG_COLS, an empty cluster
    and one of three segments -- at d = 3 and 5 (one and two float4 pieces a point), with and without the permutation, on
    strided rows; d = 50 (sixteen pieces); and 300 clusters of 1-3 cells, where every thread of the table kernel owns two
    groups;
  * state_corr: groups of 0, 1, 255, 256, 257 and 513 cells, D = 5 (a lane's quad reaches past D) and 257 (a second tile of
    one gene), S = 3 (a 2-state and a 1-state pass), with and without a row map, without offsets, narrow (a pitch that is
    no multiple of 4) and wide loads; and G = 300;
  * group_moments: groups of 0, 1, 31, 32, 33, 256 and 257 cells (both sides of GC_ROW_CHUNK and GC_SEG_ROWS), d = 3 and 17 on
    every instance that admits them; and G = 300;
  * gauss_scores, gram (n = 257, D = 65, sums and covariance), pca_project, cpm_dense and cpm_csr (int32 and float32, with and
    without log1p, a gene subset) and gene_stats: one case each on a shuffled row map with repeats, narrow on a pitch that
    is no multiple of 4 and wide on an aligned copy;
  * rank sums (rank_sum2, tie_term, n_pos and sum at eps = 0.0 and 0.1), on values rounded to one decimal with three zeros in
    ten, so that ties are the rule, read through a shuffled row map with repeats from a strided view: the one-call path and
    the blocked one with blocks of 128 and 32768 cells, on 65 cells in groups of 0, 64 and 1 (128 padded keys, a workgroup of
    one wave), on 130 cells and 513 genes (a second gene chunk, a ninth gene tile of the staging copy), on groups of 1, 1024,
    0, 1025 and 65 cells (both sides of RS_BIG) and on 300 groups of 1-3 cells (every wave walks several); the blocked path
    alone on 4097 cells in blocks of 128 and 4096 (two tiles of k_rsb_rank, a last block of one cell);
  * knn (idx and dist2), 130 queries (a partial third tile) against 700 references, on such values too, so that equal
    distances are common: d = 3, 5 and 50 (1, 2 and 16 float4 pieces; 16 is the path without the four-wide unroll) by k = 1,
    15 and 64 (15 is no multiple of the insert's chunk of 8), each without groups and with fold groups of 5, with the entry's
    own segmentation, with seg_cols = 256 (three segments and the merge -- which the entry also chooses at this size) and
    with seg_cols = 1024 (one segment: two staging passes at d = 3, no merge); once on strided rows; and knn_votes on a k = 15
    result with 7 classes, qlabel and top2.
"""
import argparse
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "analysis_bits.npz")
PARENT_KEY = "__parent__"

SIL_SIZES = (1, 511, 512, 513, 0, 1025)
SC_SIZES = (0, 1, 255, 256, 257, 513)
GC_SIZES = (0, 1, 31, 32, 33, 256, 257)


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _digest(t: torch.Tensor):
    a = t.detach().contiguous().cpu().numpy()
    return hashlib.sha256(a.tobytes()).digest(), tuple(a.shape)


def _offsets(sizes, dev):
    return torch.as_tensor(np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64))]), dtype=torch.int64).to(dev)


def _pitched(a: np.ndarray, ld: int, dev) -> torch.Tensor:
    """``a`` [n, D] on the device as the leading columns of a matrix of row pitch ``ld``."""
    base = torch.zeros(a.shape[0], ld, dtype=torch.as_tensor(a[:0]).dtype, device=dev)
    base[:, :a.shape[1]] = torch.as_tensor(a).to(dev)
    return base[:, :a.shape[1]]


def _narrow_ld(D):
    return D + 2 if (D + 2) % 4 else D + 3


def _wide_ld(D):
    return (D + 3) // 4 * 4 + 4


def _small_groups(rng, G):
    return rng.integers(1, 4, size=G)


# ---- the cases: name -> function(N, dev) -> {output name: tensor} ------------------------------------------------------------
def _sil(sizes, d, perm, ld, seed):
    def run(N, dev):
        rng = _rng(seed)
        n = int(np.sum(sizes))
        x = rng.standard_normal((n, d)).astype(np.float32)
        xs = _pitched(x, ld, dev) if ld else torch.as_tensor(x).to(dev)
        p = torch.as_tensor(rng.permutation(n).astype(np.int64)).to(dev) if perm else None
        return {"s": N.silhouette(xs, _offsets(sizes, dev), p)}
    return run


def _sc(sizes, D, S, rows, offsets, path, seed):
    def run(N, dev):
        rng = _rng(seed)
        n = int(np.sum(sizes))
        n_total = n + 37 if rows else n
        data = rng.standard_normal((n_total, D)).astype(np.float32)
        data[data < -0.3] = 0.0                                       # a mask that differs gene by gene
        state = rng.standard_normal((n, S)).astype(np.float32)
        x = _pitched(data, _wide_ld(D) if path == "wide" else _narrow_ld(D), dev)
        assert N.state_corr_wide(x) == (path == "wide")
        r = torch.as_tensor(rng.integers(0, n_total, size=n).astype(np.int64)).to(dev) if rows else None
        off = _offsets(sizes, dev) if offsets else None
        out_r, count = N.state_corr(x, torch.as_tensor(state).to(dev), r, off, path=path)
        return {"r": out_r, "count": count}
    return run


def _gm(sizes, d, path, seed):
    def run(N, dev):
        rng = _rng(seed)
        n = int(np.sum(sizes))
        x = (rng.standard_normal((n, d)) + 2.0).astype(np.float32)
        pivot = torch.as_tensor(x[0].copy()).to(dev)
        s, M = N.group_moments(_pitched(x, d + 1, dev), _offsets(sizes, dev), pivot, path=path)
        return {"s": s, "M": M}
    return run


def _gauss_scores(N, dev):
    rng = _rng(40)
    n, d, F, K = 203, 5, 2, 3
    x = rng.standard_normal((n, d)).astype(np.float32)
    model = np.sort(rng.integers(0, F, size=n)).astype(np.int32)
    mu = rng.standard_normal((F, K, d))
    W = rng.standard_normal((F, K, d, d))
    c0 = rng.standard_normal((F, K))
    c0[1, 2] = -np.inf                                                # a class a fold never saw
    perm = torch.as_tensor(rng.permutation(n).astype(np.int64)).to(dev)
    label, best, second, scores = N.gauss_scores(_pitched(x, d + 2, dev), torch.as_tensor(model).to(dev),
                                                 torch.as_tensor(mu).to(dev), torch.as_tensor(W).to(dev),
                                                 torch.as_tensor(c0).to(dev), perm, return_scores=True)
    return {"label": label, "best": best, "second": second, "scores": scores}


def _row_map(rng, n_total, n, dev):
    """A shuffled map with repeats: n draws from n_total rows."""
    return torch.as_tensor(rng.integers(0, n_total, size=n).astype(np.int64)).to(dev)


def _gram(N, dev):
    rng = _rng(50)
    n_total, n, D = 300, 257, 65
    data = rng.standard_normal((n_total, D)).astype(np.float32)
    rows = _row_map(rng, n_total, n, dev)
    pivot = torch.as_tensor(data[3].copy()).to(dev)
    out = {}
    for path, ld in (("narrow", _narrow_ld(D)), ("wide", _wide_ld(D))):
        x = _pitched(data, ld, dev)
        assert N.gram_wide(x) == (path == "wide")
        for cov in (False, True):
            s, G = N.gram(x, pivot, rows, cov=cov, path=path)
            out[f"{path}/cov{int(cov)}/s"], out[f"{path}/cov{int(cov)}/G"] = s, G
    return out


def _pca_project(N, dev):
    rng = _rng(60)
    n_total, n, D, k = 300, 257, 65, 3
    data = rng.standard_normal((n_total, D)).astype(np.float32)
    rows = _row_map(rng, n_total, n, dev)
    mean = torch.as_tensor(rng.standard_normal(D)).to(dev)
    V = torch.as_tensor(rng.standard_normal((D, k))).to(dev)
    return {"Z": N.pca_project(_pitched(data, _narrow_ld(D), dev), mean, V, rows)}


def _counts(rng, n_total, G, dtype):
    c = rng.poisson(0.7, size=(n_total, G)).astype(dtype)
    if dtype == np.float32:
        c *= rng.random((n_total, G), dtype=np.float32)
    c[5] = 0                                                          # a zero row: its norm is 1
    return c


def _cpm_dense(N, dev):
    rng = _rng(70)
    n_total, n, G = 90, 70, 1031
    genes = torch.as_tensor(np.sort(rng.choice(G, size=301, replace=False)).astype(np.int32)).to(dev)
    rows = _row_map(rng, n_total, n, dev)
    out = {}
    for dtype in (np.int32, np.float32):
        c = _counts(rng, n_total, G, dtype)
        for path, ld in (("narrow", _narrow_ld(G)), ("wide", _wide_ld(G))):
            x = _pitched(c, ld, dev)
            assert N.cpm_wide(x) == (path == "wide")
            for log in (False, True):
                o, norms = N.cpm_dense(x, rows, genes, scaler=1e4, log=log, path=path)
                key = f"{np.dtype(dtype).name}/{path}/log{int(log)}"
                out[key + "/out"], out[key + "/norms"] = o, norms
    return out


def _cpm_csr(N, dev):
    rng = _rng(80)
    n_total, n, G, ng = 90, 70, 1031, 301
    sel = np.sort(rng.choice(G, size=ng, replace=False))
    inv = np.full(G, -1, dtype=np.int32)
    inv[sel] = np.arange(ng, dtype=np.int32)
    rows = _row_map(rng, n_total, n, dev)
    out = {}
    for dtype in (np.int32, np.float32):
        c = _counts(rng, n_total, G, dtype)
        nz = c != 0
        indptr = np.concatenate([[0], np.cumsum(nz.sum(axis=1))]).astype(np.int64)
        indices = np.nonzero(nz)[1].astype(np.int32)
        vals = c[nz]
        for log in (False, True):
            o, norms = N.cpm_csr(torch.as_tensor(indptr).to(dev), torch.as_tensor(indices).to(dev), torch.as_tensor(vals).to(dev),
                                 (n_total, G), torch.as_tensor(inv).to(dev), ng, rows, scaler=1e4, log=log)
            key = f"{np.dtype(dtype).name}/log{int(log)}"
            out[key + "/out"], out[key + "/norms"] = o, norms
    return out


def _gene_stats(N, dev):
    rng = _rng(90)
    n_total, n, D = 700, 513, 261
    data = rng.standard_normal((n_total, D)).astype(np.float32)
    rows = _row_map(rng, n_total, n, dev)
    out = {}
    for path, ld in (("narrow", _narrow_ld(D)), ("wide", _wide_ld(D))):
        x = _pitched(data, ld, dev)
        assert N.cpm_wide(x) == (path == "wide")
        out[f"{path}/n_above"], out[f"{path}/mean"], out[f"{path}/std"] = N.gene_stats(x, 0.1, rows, path=path)
    return out


def _quantised(rng, shape):
    """Values on a grid of tenths, three in ten exactly zero: ties in value and in distance are common."""
    a = np.round(rng.standard_normal(shape), 1).astype(np.float32)
    a[rng.random(shape) < 0.3] = 0.0
    return a


def _rs(sizes, D, block, seed):
    def run(N, dev):
        from distributed_vae_amd.utils import marker_analysis as MA
        rng = _rng(seed)
        n = int(np.sum(sizes))
        n_total = n + 37
        x = _pitched(_quantised(rng, (n_total, D)), _narrow_ld(D), dev)
        rows = _row_map(rng, n_total, n, dev)
        out = {}
        for eps in (0.0, 0.1):
            res = MA.rank_sums(x, rows, _offsets(sizes, dev), eps, block_cells=block)
            for key, t in zip(_RS_OUT, res):
                out[f"eps{eps}/{key}"] = t
        return out
    return run


def _knn_inputs(d, seed, dev, strided=False):
    rng = _rng(seed)
    nq, nr = 130, 700
    q, r = _quantised(rng, (nq, d)), _quantised(rng, (nr, d))
    qg = torch.as_tensor(rng.integers(0, 5, size=nq).astype(np.int32)).to(dev)
    rg = torch.as_tensor(rng.integers(0, 5, size=nr).astype(np.int32)).to(dev)
    if strided:
        return _pitched(q, d + 2, dev), _pitched(r, d + 3, dev), qg, rg
    return torch.as_tensor(q).to(dev), torch.as_tensor(r).to(dev), qg, rg


def _knn(d, k, strided, seed):
    def run(N, dev):
        from distributed_vae_amd.utils import neighbors as NB
        q, r, qg, rg = _knn_inputs(d, seed, dev, strided)
        out = {}
        for gname, groups in (("plain", (None, None)), ("fold", (qg, rg))):
            for sname, seg in _KNN_SEGS[:1] if strided else _KNN_SEGS:
                out[f"{gname}/{sname}/idx"], out[f"{gname}/{sname}/dist2"] = NB.knn_device(q, r, k, *groups, seg_cols=seg)
        return out
    return run


def _knn_votes(N, dev):
    from distributed_vae_amd.utils import neighbors as NB
    q, r, _, _ = _knn_inputs(3, 103, dev)
    rng = _rng(199)
    rlabel = torch.as_tensor(rng.integers(0, 7, size=int(r.shape[0])).astype(np.int32)).to(dev)
    qlabel = torch.as_tensor(rng.integers(0, 7, size=int(q.shape[0])).astype(np.int32)).to(dev)
    idx, _ = NB.knn_device(q, r, 15)
    pred, purity, top2 = NB.knn_votes_device(idx, rlabel, 7, qlabel, top2=True)
    return {"pred": pred, "purity": purity, "top2": top2}


_RS_OUT = ("rank_sum2", "tie_term", "n_pos", "sum")
_RS_SHAPES = {"n65": ((0, 64, 1), 3), "n130_D513": ((65, 65), 513), "big_small": ((1, 1024, 0, 1025, 65), 17),
              "g300": (tuple(int(v) for v in _small_groups(_rng(4), 300)), 5)}
_KNN_SEGS = (("own", None), ("seg256", 256), ("seg1024", 1024))

CASES = {}
for _d in (3, 5):
    CASES[f"sil_d{_d}"] = _sil(SIL_SIZES, _d, False, 0, 10 + _d)
    CASES[f"sil_d{_d}_perm"] = _sil(SIL_SIZES, _d, True, 0, 10 + _d)
    CASES[f"sil_d{_d}_perm_strided"] = _sil(SIL_SIZES, _d, True, _d + 2, 10 + _d)
CASES["sil_d50"] = _sil(SIL_SIZES, 50, False, 0, 60)
CASES["sil_k300"] = _sil(tuple(int(v) for v in _small_groups(_rng(1), 300)), 3, True, 0, 19)
for _D in (5, 257):
    CASES[f"sc_D{_D}_narrow_rows"] = _sc(SC_SIZES, _D, 3, True, True, "narrow", 20 + _D)
    CASES[f"sc_D{_D}_wide_rows"] = _sc(SC_SIZES, _D, 3, True, True, "wide", 20 + _D)
    CASES[f"sc_D{_D}_narrow"] = _sc(SC_SIZES, _D, 3, False, True, "narrow", 20 + _D)
    CASES[f"sc_D{_D}_wide_one_group"] = _sc(SC_SIZES, _D, 3, False, False, "wide", 20 + _D)
CASES["sc_g300"] = _sc(tuple(int(v) for v in _small_groups(_rng(2), 300)), 5, 3, True, True, "narrow", 29)
for _d, _paths in ((3, ("auto", "d16", "d32", "d64", "d128")), (17, ("auto", "d32", "d64", "d128"))):
    for _p in _paths:
        CASES[f"gm_d{_d}_{_p}"] = _gm(GC_SIZES, _d, _p, 30 + _d)
CASES["gm_g300"] = _gm(tuple(int(v) for v in _small_groups(_rng(3), 300)), 3, "auto", 39)
CASES["gauss_scores"] = _gauss_scores
CASES["gram"] = _gram
CASES["pca_project"] = _pca_project
CASES["cpm_dense"] = _cpm_dense
CASES["cpm_csr"] = _cpm_csr
CASES["gene_stats"] = _gene_stats
for _i, (_name, (_sizes, _D)) in enumerate(_RS_SHAPES.items()):
    for _b in (None, 128, 32768):
        CASES[f"rs_{_name}_{'one_call' if _b is None else 'b%d' % _b}"] = _rs(_sizes, _D, _b, 110 + _i)
for _b in (128, 4096):
    CASES[f"rs_n4097_b{_b}"] = _rs((1025, 3000, 72), 5, _b, 119)
for _d in (3, 5, 50):
    for _k in (1, 15, 64):
        CASES[f"knn_d{_d}_k{_k}"] = _knn(_d, _k, False, 100 + _d)
CASES["knn_d5_k15_strided"] = _knn(5, 15, True, 105)
CASES["knnvotes"] = _knn_votes

_PATHS2 = ("narrow", "wide")
_KEYS = {
    "sil": ("s",), "sc": ("r", "count"), "gm": ("s", "M"), "gauss_scores": ("label", "best", "second", "scores"),
    "gram": tuple(f"{p}/cov{c}/{a}" for p in _PATHS2 for c in (0, 1) for a in ("s", "G")),
    "pca_project": ("Z",),
    "cpm_dense": tuple(f"{t}/{p}/log{g}/{a}" for t in ("int32", "float32") for p in _PATHS2 for g in (0, 1) for a in ("out", "norms")),
    "cpm_csr": tuple(f"{t}/log{g}/{a}" for t in ("int32", "float32") for g in (0, 1) for a in ("out", "norms")),
    "gene_stats": tuple(f"{p}/{a}" for p in _PATHS2 for a in ("n_above", "mean", "std")),
    "rs": tuple(f"eps{e}/{a}" for e in (0.0, 0.1) for a in _RS_OUT),
    "knn": tuple(f"{g}/{s}/{a}" for g in ("plain", "fold") for s, _ in _KNN_SEGS for a in ("idx", "dist2")),
    "knn_d5_k15_strided": tuple(f"{g}/own/{a}" for g in ("plain", "fold") for a in ("idx", "dist2")),
    "knnvotes": ("pred", "purity", "top2"),
}


def expected_keys(name):
    return set(_KEYS[name] if name in _KEYS else _KEYS[name.split("_")[0]])


def run_case(name, device="cuda:0"):
    """{output name: (sha256 digest (bytes), shape)} of one case with the library that is loaded."""
    import distributed_vae_amd  # noqa: F401
    from distributed_vae_amd import _native as N
    out = CASES[name](N, torch.device(device))
    torch.cuda.synchronize()
    return {k: _digest(t) for k, t in out.items()}


def load_golden(path=GOLDEN):
    """({case: {output: (digest, shape)}}, the hash of the commit whose library wrote them)"""
    z = np.load(path)
    gold = {}
    for k in z.files:
        if k == PARENT_KEY or k.endswith("|shape"):
            continue
        case, arr = k.split("|")
        gold.setdefault(case, {})[arr] = (z[k].tobytes(), tuple(int(v) for v in z[k + "|shape"]))
    return gold, str(z[PARENT_KEY])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--write", action="store_true", help="write tests/golden/analysis_bits.npz from the loaded library")
    ap.add_argument("--parent", default="", help="with --write: the hash of the commit the loaded library was built from")
    ap.add_argument("--out", default=GOLDEN)
    args = ap.parse_args()
    from distributed_vae_amd import _native as N
    print("library:", N.LIB_PATH)
    got = {name: run_case(name) for name in CASES}
    if args.write:
        assert args.parent, "--write needs --parent"
        again = {name: run_case(name) for name in CASES}          # a digest that differs run to run is no reference
        assert again == got, [n for n in CASES if again[n] != got[n]]
        flat = {PARENT_KEY: np.asarray(args.parent)}
        for case, arrs in got.items():
            assert set(arrs) == expected_keys(case), case
            for arr, (dg, shape) in arrs.items():
                flat[f"{case}|{arr}"] = np.frombuffer(dg, dtype=np.uint8)
                flat[f"{case}|{arr}|shape"] = np.asarray(shape, dtype=np.int64)
        np.savez(args.out, **flat)
        print(f"wrote {args.out}: {len(got)} cases, {sum(len(v) for v in got.values())} digests, parent {args.parent}")
        return 0
    gold, parent = load_golden(args.out)
    print("golden written at", parent)
    bad = 0
    for case in CASES:
        diff = sorted(k for k in set(gold[case]) | set(got[case]) if gold[case].get(k) != got[case].get(k))
        bad += bool(diff)
        print(f"{case}: {'identical' if not diff else 'DIFFERS in ' + ', '.join(diff)}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

"""Build container only (sklearn and the reference are present there): record what the reference's ``normalize_cellxgene``,
``logcpm`` and ``reorder_genes`` compute, as the data-only fixture tests/golden/dataprep_kat.npz
(tests/test_dataprep_cpu.py, tests/test_gpu_dataprep.py).

The three functions are the reference's own (mmidas/utils/tools.py): the module is imported where that works; where one of
its imports is missing (``toml``, ``requests``) the three functions are compiled in memory from the file where it lies
(``ast``) with the installed ``sklearn.preprocessing.normalize``; ``source`` records which.  Nothing of the reference is
copied into the repository.

  counts            int32 [301, 1300]  Poisson counts, about 20 % non-zero, row 7 all zero, row 11 one non-zero
  rows              int64 [R]          the rows whose reference results are recorded (the two above among them)
  norm_i, log_i     float64 [R, 1300]  normalize_cellxgene(counts)[rows], logcpm(counts)[rows]
  xf64              float64 [24, 1300] counts on a 1/8 grid with some negative entries, a zero row
  norm_f64, log_f64 float64 [24, 1300] the reference's returns on xf64
  norm_f32, log_f32 float32 [24, 1300] its returns on xf64.astype(float32) (sklearn then sums in float32)
  expr              float32 [301, 1300] expression on a 1/64 grid, about 75 % zeros, with the planted columns ``planted``
                    (gene index of: all zero; all above eps; every cell float32(0.1); its lower float32 neighbour; its upper
                    neighbour; exactly one cell above eps; all but one)
  order32, order64  int64  the reference's reorder_genes(expr) and reorder_genes(expr.astype(float64))
  margin            float64  the least |closed-form std - eps| over the genes, both dtypes (asserted >= 1e-6: nearer, the
                    reference's np.std and the closed form may legitimately keep different sets)

    python -m tools.gen_golden_dataprep
"""
import ast
import contextlib
import importlib.util
import io
import os
import sys

import numpy as np

from oracle import ref_loader as RL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dataprep_restatement as DR  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
_FILE = os.path.join(RL.REFERENCE_ROOT, "mmidas", "utils", "tools.py")
NAMES = ("normalize_cellxgene", "logcpm", "reorder_genes")
N_CELLS, N_GENES, EPS = 301, 1300, 1e-1


def load_reference():
    import sklearn
    from sklearn.preprocessing import normalize
    try:
        spec = importlib.util.spec_from_file_location("_ref_tools", _FILE)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return {k: getattr(mod, k) for k in NAMES}, f"module imported; sklearn {sklearn.__version__}, numpy {np.__version__}"
    except ImportError as e:
        with open(_FILE, "r") as fh:
            tree = ast.parse(fh.read(), filename=_FILE)
        keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in NAMES]
        assert len(keep) == len(NAMES)
        ns = {"np": np, "normalize": normalize, "Any": object}
        exec(compile(ast.Module(body=keep, type_ignores=[]), _FILE, "exec"), ns)
        return ({k: ns[k] for k in NAMES},
                f"functions compiled from the reference file ({e}); sklearn {sklearn.__version__}, numpy {np.__version__}")


def quiet(fn, *a):
    with contextlib.redirect_stdout(io.StringIO()):              # reorder_genes prints
        return fn(*a)


def make_expr(rng):
    n, D = N_CELLS, N_GENES
    level = np.round(np.abs(rng.normal(size=(n, D))) * 2.0 * 64.0 + 8.0) / 64.0       # >= 0.125 > eps
    low = np.round(rng.random(size=(n, D)) * 6.0) / 64.0                              # <= 0.094 < eps: expressed, not counted
    u = rng.random(size=(n, D))
    frac = rng.random(size=D) * 0.6                                                   # a gene's share of cells above eps
    expr = np.where(u < frac, level, np.where(u < frac + 0.05, low, 0.0)).astype(np.float32)
    t = np.float32(EPS)
    planted = np.arange(7, dtype=np.int64) * 3 + 2
    expr[:, planted[0]] = 0.0
    expr[:, planted[1]] = level[:, planted[1]]
    expr[:, planted[2]] = t                                                            # not above float32(eps); above eps in float64
    expr[:, planted[3]] = np.nextafter(t, np.float32(0))
    expr[:, planted[4]] = np.nextafter(t, np.float32(1))
    expr[:, planted[5]] = 0.0
    expr[rng.integers(n), planted[5]] = 1.5                                            # k = 1
    expr[:, planted[6]] = level[:, planted[6]]
    expr[rng.integers(n), planted[6]] = 0.0                                            # k = n - 1
    return expr, planted


def main():
    ref, source = load_reference()
    rng = np.random.default_rng(20259)
    counts = rng.poisson(0.22, size=(N_CELLS, N_GENES)).astype(np.int32)
    counts[7] = 0
    counts[11] = 0
    counts[11, 123] = 3
    rows = np.unique(np.concatenate([[7, 11, N_CELLS - 1], np.arange(0, N_CELLS, 9)])).astype(np.int64)
    norm_i = np.asarray(ref["normalize_cellxgene"](counts))
    log_i = np.asarray(ref["logcpm"](counts))
    assert norm_i.dtype == np.float64 and log_i.dtype == np.float64
    # the restatement reproduces both to the bit on integer counts (every row, not only the recorded ones)
    assert np.array_equal(DR.normalize_cellxgene(counts), norm_i) and np.array_equal(DR.logcpm(counts), log_i)

    xf64 = (rng.poisson(0.4, size=(24, N_GENES)) * rng.integers(1, 64, size=(24, N_GENES))) / 8.0
    xf64 = np.where(rng.random(size=xf64.shape) < 0.02, -xf64, xf64)
    xf64[5] = 0.0
    xf32 = xf64.astype(np.float32)
    assert np.array_equal(xf32.astype(np.float64), xf64)
    norm_f64, log_f64 = np.asarray(ref["normalize_cellxgene"](xf64)), np.asarray(ref["logcpm"](xf64))
    norm_f32, log_f32 = np.asarray(ref["normalize_cellxgene"](xf32)), np.asarray(ref["logcpm"](xf32))
    assert norm_f64.dtype == np.float64 and norm_f32.dtype == np.float32 and log_f32.dtype == np.float32

    expr, planted = make_expr(rng)
    order32 = np.asarray(quiet(ref["reorder_genes"], expr), dtype=np.int64)
    order64 = np.asarray(quiet(ref["reorder_genes"], expr.astype(np.float64)), dtype=np.int64)
    margin = np.inf
    for x, order in ((expr, order32), (expr.astype(np.float64), order64)):
        mine, k = DR.reorder_genes(x, EPS)
        std = np.sqrt(DR.keys(k, N_CELLS).astype(np.float64)) / N_CELLS
        margin = min(margin, float(np.abs(std - EPS).min()))
        assert set(mine.tolist()) == set(order.tolist())
        assert np.array_equal(DR.keys(k, N_CELLS)[mine], DR.keys(k, N_CELLS)[order])
        print(f"reorder_genes {x.dtype}: {order.size} of {N_GENES} kept, same order {bool(np.array_equal(mine, order))}")
    assert margin >= 1e-6, margin
    out = {"source": np.array(source), "counts": counts, "rows": rows, "norm_i": norm_i[rows], "log_i": log_i[rows], "xf64": xf64,
           "norm_f64": norm_f64, "log_f64": log_f64, "norm_f32": norm_f32, "log_f32": log_f32, "expr": expr, "planted": planted,
           "order32": order32, "order64": order64, "margin": np.float64(margin), "eps": np.float64(EPS)}
    print(source)
    print(f"counts: {float((counts != 0).mean()):.3f} non-zero; margin {margin:.3e}")
    path = os.path.join(GOLDEN, "dataprep_kat.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

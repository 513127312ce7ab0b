"""Build container only (scipy and the reference are present there): record what the reference's ``corr_analysis`` computes,
as the data-only fixture tests/golden/statecorr_kat.npz (tests/test_statecorr_cpu.py, tests/test_gpu_statecorr.py).

``corr_analysis`` is the reference's own function (mmidas/utils/tree_based_analysis.py): the module is imported where that
works; where one of its imports is missing the function is compiled in memory from the file where it lies (``ast``) with the
installed ``scipy.stats``; ``source`` records which.  Nothing of the reference is copied into the repository.

per case k of CASES = (n, D, S): expression with about 75 % exact zeros and some negative entries, states offset from zero by
a few standard deviations (so that kappa = 1 + mean^2 / var stays moderate), everything on a 2^-12 grid (so that the file
compresses), and planted columns where D allows them (``c<k>/planted``: gene index or -1 for all-zero, exactly 4 positive
cells, exactly 5, equal positive values, state 0 constant over the gene's mask)
  c<k>/state     float32 [n, S]
  c<k>/cell      float32 [n, D]
  c<k>/corr32, c<k>/gene32   the reference's two returns called with the float32 arrays (scipy then computes in float32,
                 which is the reference's behaviour on such inputs), stacked [S, D]
  c<k>/corr64, c<k>/gene64   its two returns called with their float64 copies
  c<k>/abs32, c<k>/abs64     the same |r| put back in gene order, [S, D]
  c<k>/nan, c<k>/zero        bool [S, D]: where the float64 call's |r| is NaN, and where it is exactly 0
  c<k>/e_ref32, c<k>/e_ref64   max | |reference| - |tests/statecorr_restatement.py| | over the finite entries

    python -m tools.gen_golden_statecorr
"""
import ast
import importlib.util
import os
import sys
import warnings

import numpy as np

from oracle import ref_loader as RL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import statecorr_restatement as SR  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = ((5, 1, 1), (6, 3, 1), (64, 9, 2), (300, 260, 2), (1100, 70, 3), (700, 40, 5))
_FILE = os.path.join(RL.REFERENCE_ROOT, "mmidas", "utils", "tree_based_analysis.py")
GRID = 4096.0


def load_reference():
    import scipy
    import scipy.stats as stats
    try:
        spec = importlib.util.spec_from_file_location("_ref_tree_based_analysis", _FILE)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod.corr_analysis, f"module imported; scipy {scipy.__version__}"
    except ImportError as e:
        with open(_FILE, "r") as fh:
            tree = ast.parse(fh.read(), filename=_FILE)
        keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "corr_analysis"]
        assert len(keep) == 1
        ns = {"np": np, "stats": stats}
        exec(compile(ast.Module(body=keep, type_ignores=[]), _FILE, "exec"), ns)
        return ns["corr_analysis"], f"function compiled from the reference file ({e}); scipy {scipy.__version__}"


def grid(a):
    return (np.round(np.asarray(a) * GRID) / GRID).astype(np.float32)


def make_case(rng, n, D, S):
    """(state, cell, planted)."""
    state = rng.normal(size=(n, S)) * 0.8 + rng.uniform(-3.0, 3.0, size=S)
    slope = rng.normal(size=D) * 0.6
    level = np.abs(rng.normal(size=(n, D))) * 2.0 + 1.0 + slope * (state[:, np.arange(D) % S] - state.mean(0)[np.arange(D) % S])
    u = rng.random(size=(n, D))
    cell = np.where(u < 0.25, np.maximum(level, 1.0 / GRID), np.where(u < 0.31, -np.abs(rng.normal(size=(n, D))), 0.0))
    if n <= 8:                                                  # the two tiny cases: every cell expresses gene 0
        cell[:, 0] = np.maximum(level[:, 0], 1.0 / GRID)
    state, cell = grid(state), grid(cell)
    planted = -np.ones(5, dtype=np.int64)

    def positives(g, k, value=None):
        col = np.minimum(cell[:, g], 0.0)                       # nothing positive ...
        col[rng.choice(n, k, replace=False)] = 1.0              # ... but k cells
        pos = col > 0
        vals = grid(np.abs(rng.normal(size=n)) + 0.5) if value is None else np.full(n, value, np.float32)
        cell[:, g] = np.where(pos, vals, col)

    if D >= 3 and n >= 6:
        planted[0] = 0
        cell[:, 0] = np.minimum(cell[:, 0], 0.0) if n > 8 else 0.0      # all-zero (or negative) gene
        planted[1], planted[2] = 1, 2
        positives(1, 4)
        positives(2, 5)
    if D >= 9:
        planted[3] = 3
        positives(3, min(n // 3, 40), value=1.75)               # equal positive values
        planted[4] = 4
        positives(4, min(n // 3, 33))
        state[cell[:, 4] > 0, 0] = state[0, 0]                  # state 0 constant over gene 4's mask
    return state, cell, planted


def stacked(ret):
    corr, gene = ret
    return np.stack([np.asarray(c, dtype=np.float64) for c in corr]), np.stack([np.asarray(g, dtype=np.int64) for g in gene])


def in_gene_order(corr, gene):
    out = np.empty_like(corr)
    for s in range(corr.shape[0]):
        out[s, gene[s]] = corr[s]
    return out


def main():
    ref, source = load_reference()
    rng = np.random.default_rng(20251)
    out = {"cases": np.array(CASES, dtype=np.int64), "source": np.array(source)}
    for k, (n, D, S) in enumerate(CASES):
        state, cell, planted = make_case(rng, n, D, S)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                     # scipy warns of every constant input
            corr32, gene32 = stacked(ref(state, cell))
            corr64, gene64 = stacked(ref(state.astype(np.float64), cell.astype(np.float64)))
        abs32, abs64 = in_gene_order(corr32, gene32), in_gene_order(corr64, gene64)
        r, cnt, kap = SR.state_corr(state, cell)
        want = np.abs(r[0])
        assert np.array_equal(np.isnan(want), np.isnan(abs64)) and np.array_equal(want == 0, abs64 == 0)
        fin = np.isfinite(want)
        e32 = float(np.abs(abs32 - want)[fin & np.isfinite(abs32)].max())
        e64 = float(np.abs(abs64 - want)[fin].max())
        out.update({f"c{k}/state": state, f"c{k}/cell": cell, f"c{k}/planted": planted, f"c{k}/corr32": corr32,
                    f"c{k}/gene32": gene32, f"c{k}/corr64": corr64, f"c{k}/gene64": gene64, f"c{k}/abs32": abs32,
                    f"c{k}/abs64": abs64, f"c{k}/nan": np.isnan(abs64), f"c{k}/zero": abs64 == 0,
                    f"c{k}/e_ref32": np.float64(e32), f"c{k}/e_ref64": np.float64(e64)})
        print(f"case {k} {(n, D, S)}: zeros {float((cell == 0).mean()):.2f}, negatives {float((cell < 0).mean()):.2f}, "
              f"NaN {int(np.isnan(abs64).sum())}, exact 0 {int((abs64 == 0).sum())}, kappa max {float(kap[np.isfinite(kap)].max()):.1f}, "
              f"e_ref32 {e32:.2e}, e_ref64 {e64:.2e}")
    print(source)
    path = os.path.join(GOLDEN, "statecorr_kat.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

"""Build container only (sklearn and the reference are present there): record what the reference's clusterability code
computes, as the data-only fixture tests/golden/silhouette_kat.npz (tests/test_silhouette_cpu.py, tests/test_gpu_silhouette.py).

``get_SilhScore`` and ``cluster_compare`` are the reference's own functions (mmidas/utils/cluster_analysis.py): the module is
imported where that works; where one of its imports is missing (seaborn, say) the two functions are compiled in memory from
the file where it lies (``ast``) with the installed sklearn's ``silhouette_samples`` / ``silhouette_score`` / ``PCA``;
``source`` records which.  ``PCA`` is given ``svd_solver="full"`` (sklearn's own choice at the recorded size).  Nothing of
the reference is copied into the repository.

per case k of CASES = (n, d, K): Gaussian blobs of O(1) scale on a 2^-12 grid (so that the file compresses), every label taken
  c<k>/x        float32 [n, d]
  c<k>/labels   int64 [n]
  c<k>/samples, c<k>/score   sklearn's silhouette_samples / silhouette_score on the float64 copy of x
  c<k>/mean_smp_sc, c<k>/sil_score   get_SilhScore's two returns on the same
  c<k>/e_ref    max |sklearn - tests/silhouette_restatement.py| over the samples
cc/data float32 [300, 40], cc/num_pc, cc/labels/<name>, and cluster_compare's returns cc/silh_smp_score/<i>, cc/sil_score,
cc/c_size/<i>; cc/e_ref as above on the projected points (the restatement's projection against sklearn's).

    python -m tools.gen_golden_silhouette
"""
import ast
import functools
import importlib.util
import os
import sys

import numpy as np

from oracle import ref_loader as RL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import silhouette_restatement as SR  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = ((3, 1, 2), (65, 1, 2), (257, 2, 7), (600, 10, 92), (400, 33, 130), (300, 128, 5))
CC = (300, 40, 5, (("few", 4), ("many", 23)))        # n, D, num_pc, (name, K) of the label sets
_FILE = os.path.join(RL.REFERENCE_ROOT, "mmidas", "utils", "cluster_analysis.py")
NAMES = ("get_SilhScore", "cluster_compare")


def load_reference():
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    from sklearn.decomposition import PCA
    from sklearn.metrics import silhouette_samples, silhouette_score
    full = functools.partial(PCA, svd_solver="full")
    try:
        spec = importlib.util.spec_from_file_location("_ref_cluster_analysis", _FILE)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        mod.PCA = full
        return {n: getattr(mod, n) for n in NAMES}, "module imported"
    except ImportError as e:
        with open(_FILE, "r") as fh:
            tree = ast.parse(fh.read(), filename=_FILE)
        keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in NAMES]
        assert len(keep) == len(NAMES)
        ns = {"np": np, "plt": plt, "PCA": full, "silhouette_samples": silhouette_samples, "silhouette_score": silhouette_score}
        exec(compile(ast.Module(body=keep, type_ignores=[]), _FILE, "exec"), ns)
        return ns, f"functions compiled from the reference file ({e})"


def blobs(rng, n, d, K, first=None):
    labels = np.array(first) if first is not None else rng.permutation(np.arange(n) % K)
    centres = rng.normal(size=(K, d)) * 1.5
    x = centres[labels] + rng.normal(size=(n, d)) * 0.6
    return (np.round(x * 4096) / 4096).astype(np.float32), labels.astype(np.int64)


def main():
    from sklearn.metrics import silhouette_samples, silhouette_score
    ref, source = load_reference()
    rng = np.random.default_rng(20250)
    out = {"cases": np.array(CASES, dtype=np.int64), "source": np.array(source)}
    for k, (n, d, K) in enumerate(CASES):
        x, labels = blobs(rng, n, d, K, first=[0, 0, 1] if n == 3 else None)
        assert len(np.unique(labels)) == K
        x64 = x.astype(np.float64)
        smp = silhouette_samples(x64, labels)
        mean_smp_sc, sil = ref["get_SilhScore"](x64, labels)
        e_ref = float(np.abs(smp - SR.silhouette_samples(x64, labels)).max())
        out.update({f"c{k}/x": x, f"c{k}/labels": labels, f"c{k}/samples": smp,
                    f"c{k}/score": np.float64(silhouette_score(x64, labels)), f"c{k}/mean_smp_sc": mean_smp_sc,
                    f"c{k}/sil_score": np.float64(sil), f"c{k}/e_ref": np.float64(e_ref)})
        print(f"case {k} {(n, d, K)}: score {float(sil):+.6f}, e_ref {e_ref:.2e}")
    n, D, num_pc, sets = CC
    data, _ = blobs(rng, n, D, 6)
    labels = {name: rng.permutation(np.arange(n) % K).astype(np.int64) for name, K in sets}
    # correlate the label sets with the geometry, so that the scores are not all near zero
    z = SR.pca_project(data.astype(np.float64), num_pc)
    labels["few"] = np.digitize(z[:, 0], np.quantile(z[:, 0], [0.25, 0.5, 0.75])).astype(np.int64)
    fig, smp_sc, sil, c_size = ref["cluster_compare"](data.astype(np.float64), labels, num_pc=num_pc)
    e_cc = max(float(np.abs(SR.silhouette_samples(z, labels[name]).mean() - sil[i])) for i, (name, _) in enumerate(sets))
    out.update({"cc/data": data, "cc/num_pc": np.int64(num_pc), "cc/names": np.array([name for name, _ in sets]),
                "cc/sil_score": np.array(sil, dtype=np.float64), "cc/e_ref": np.float64(e_cc)})
    for i, (name, _) in enumerate(sets):
        out.update({f"cc/labels/{name}": labels[name], f"cc/silh_smp_score/{i}": smp_sc[i], f"cc/c_size/{i}": c_size[i]})
    print(f"cluster_compare: scores {sil}, e_ref {e_cc:.2e}; {source}")
    path = os.path.join(GOLDEN, "silhouette_kat.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

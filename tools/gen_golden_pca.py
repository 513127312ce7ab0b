"""Build container only (sklearn is present there): record what sklearn's ``PCA(n_components, svd_solver="full")`` -- the
solver the reference's ``cluster_compare`` gets at these sizes -- computes on the designed inputs of
tests/pca_restatement.py, as the data-only fixture tests/golden/pca_cases.npz (tests/test_pca_cpu.py, tests/test_gpu_pca.py).

per case <name> of pca_restatement.CASES (n, D, k), the input X = U diag(sqrt(lambda (n - 1))) W^T + offsets put on a 2^-12
grid (so that the file compresses; the spectrum moves by 1e-7) and held as float32:
  <name>/x                          float32 [n, D]
  <name>/components                 float64 [k, D]   PCA.components_ on the float64 copy of x
  <name>/explained_variance, <name>/explained_variance_ratio   float64 [k]
  <name>/mean                       float64 [D]
  <name>/transform                  float64 [n, k]   PCA.transform of the same
names, the sklearn version, and ``source`` (how the file was made).

    python -m tools.gen_golden_pca
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pca_restatement as PR  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "pca_cases.npz")


def main():
    import sklearn
    from sklearn.decomposition import PCA
    out = {"names": np.array(sorted(PR.CASES)), "sklearn": np.array(sklearn.__version__),
           "source": np.array('sklearn.decomposition.PCA(n_components=k, svd_solver="full") on tests/pca_restatement.design')}
    for name, (n, D, k) in PR.CASES.items():
        x = (np.round(PR.design(name).astype(np.float64) * 4096.0) / 4096.0).astype(np.float32)
        assert x.shape == (n, D)
        p = PCA(n_components=k, svd_solver="full")
        z = p.fit_transform(x.astype(np.float64))
        out[f"{name}/x"] = x
        out[f"{name}/components"] = p.components_
        out[f"{name}/explained_variance"] = p.explained_variance_
        out[f"{name}/explained_variance_ratio"] = p.explained_variance_ratio_
        out[f"{name}/mean"] = p.mean_
        out[f"{name}/transform"] = z
        lam = PR.eigh_route(x, k)[2]
        print(f"{name}: lambda_1..k+1 {np.array2string(lam[:k + 1], precision=4)}, e_ref {PR.reference_errors(x, k)}")
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    assert size < 1024 * 1024, size
    print(f"{OUT}: {size} bytes")


if __name__ == "__main__":
    main()

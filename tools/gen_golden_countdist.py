"""Build machine only: run the REAL reference's ``mmidas/utils/distributions.py`` (loaded by path, where the checkout lies) and
commit what it computed as the data-only fixture tests/golden/countdist_kat.npz (tests/test_countdist_cpu.py,
tests/test_gpu_countdist.py).  Arrays only; nothing of the reference's text is copied.

Per likelihood case ``<c>`` (``cases`` lists the names; inputs from tests/countdist_inputs.regimes, which covers theta below 1,
at 1 and large, mu = 0 .. 1e3 and mu = theta = 1e9, logits at +-30 and about 0, x = 0, eps and large; c0 has theta as a matrix,
c1 as a vector [D]):
  <c>/x, mu, theta, pi, mu2, theta2     the float32 inputs
  <c>/<fn>/f32, <c>/<fn>/f64            the reference's return on the float32 inputs and on the same inputs as float64, fn in
                                        nb (log_nb_positive), zinb (log_zinb_positive), mix (log_mixture_nb with theta_2),
                                        mix1 (log_mixture_nb with theta_2 = None)
Per sampler setting ``<s>`` of tests/countdist_inputs.SETTINGS (``settings`` lists the names):
  <s>/values, <s>/counts                the histogram of 2^16 draws of the reference's ``sample`` (NegativeBinomial, or
                                        ZeroInflatedNegativeBinomial where the setting has a zero-inflation probability) in
                                        float32, the reference's dtype, after torch.manual_seed(SEED + its position)

    python -m tools.gen_golden_countdist [path of the reference checkout; default: oracle.ref_loader.REFERENCE_ROOT]
"""
import importlib.util
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import countdist_inputs as CI  # noqa: E402
from oracle import ref_loader as RL  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
CASES = {"c0": (23, 31, 11, False), "c1": (17, 29, 12, True)}      # n, D, seed, theta as a vector
SEED = 1234


def load_reference(root):
    path = os.path.join(root, "mmidas", "utils", "distributions.py")
    sys.dont_write_bytecode = True
    spec = importlib.util.spec_from_file_location("ref_distributions", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ref = load_reference(sys.argv[1] if len(sys.argv) > 1 else RL.REFERENCE_ROOT)
    out = {"cases": np.array(sorted(CASES)), "settings": np.array([s[0] for s in CI.SETTINGS])}
    for name, (n, D, seed, vec) in sorted(CASES.items()):
        r = CI.regimes(n, D, seed, theta_vector=vec)
        for k, v in r.items():
            out[f"{name}/{k}"] = v
        for tag, dtype in (("f32", torch.float32), ("f64", torch.float64)):
            t = {k: torch.from_numpy(v).to(dtype) for k, v in r.items()}
            res = {"nb": ref.log_nb_positive(t["x"], t["mu"], t["theta"]),
                   "zinb": ref.log_zinb_positive(t["x"], t["mu"], t["theta"], t["pi"]),
                   "mix": ref.log_mixture_nb(t["x"], t["mu"], t["mu2"], t["theta"], t["theta2"], t["pi"]),
                   "mix1": ref.log_mixture_nb(t["x"], t["mu"], t["mu2"], t["theta"], None, t["pi"])}
            for fn, v in res.items():
                assert v.dtype == dtype and tuple(v.shape) == (n, D) and bool(torch.isfinite(v).all()), (name, fn, tag)
                out[f"{name}/{fn}/{tag}"] = v.numpy()
    for i, (name, mu, theta, z) in enumerate(CI.SETTINGS):
        torch.manual_seed(SEED + i)
        m, th = torch.full((CI.N_DRAWS,), mu), torch.full((CI.N_DRAWS,), theta)
        if z is None:
            d = ref.NegativeBinomial(mu=m, theta=th)
        else:
            d = ref.ZeroInflatedNegativeBinomial(mu=m, theta=th, zi_logits=torch.logit(torch.full((CI.N_DRAWS,), z)))
        draws = d.sample()
        assert draws.dtype == torch.float32 and draws.shape == (CI.N_DRAWS,)
        v, c = np.unique(draws.numpy().astype(np.int64), return_counts=True)
        out[f"{name}/values"], out[f"{name}/counts"] = v.astype(np.int32), c.astype(np.int32)
    path = os.path.join(GOLDEN, "countdist_kat.npz")
    np.savez_compressed(path, **out)
    print({k: np.asarray(v).shape for k, v in out.items()})
    print(os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

"""Build container only: run the REAL reference ``evals2`` (mmidas/_evals.py) on two small reference models and commit
what it computed as the data-only fixture tests/golden/evals2_a3.npz (tests/test_evals_cpu.py, tests/test_gpu_evals.py).

``generate`` (mmidas/model.py, without its ``@unstable`` decorator), ``evals2`` and the helpers of mmidas/_utils.py they
call are compiled in memory from the reference files where they lie; stub ``mmidas``, ``mmidas.model`` and
``mmidas._utils`` modules let ``evals2``'s inner imports resolve.  Nothing of the reference is copied into the repository.

Two models (A = 3, D = 64, H = 16, L = 4, C = 7, S = 2) from different seeds, parameters x 1.5, BatchNorm running
statistics randomised, category PRUNED's fcc bias zeroed in every arm; N = 150 cells in batches of 64 (64, 64, 22); fp64.
  sd_a/<key>, sd_b/<key>   the two state dicts
  x                        the cells [N, D]
  gen_a/*, gen_b/*         generate's preds, cs, inds_prune, pruning_mask of each model
  ab/<key>                 every key of evals2(fa, fb, dl); lists as stacked arrays (empty lists: shape (0,))
  aa/<key>                 every key of evals2(fa, fa, dl)
The seeds are searched until every cell's top-2 margin of c exceeds 1e-3 in every arm of both models (an fp32 engine then
cannot flip a label) and at least two labels occur per arm.

    python -m tools.gen_golden_evals
"""
import ast
import os
import sys
import types

import numpy as np
import torch
from torch.utils.data import DataLoader, TensorDataset

from oracle import ref_loader as RL

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
A, D, H, L, C, S = 3, 64, 16, 4, 7, 2
N, BATCH, PRUNED = 150, 64, 4
MARGIN = 1e-3
_MODEL = os.path.join(RL.REFERENCE_ROOT, "mmidas", "model.py")
_EVALS = os.path.join(RL.REFERENCE_ROOT, "mmidas", "_evals.py")
_UTILS = os.path.join(RL.REFERENCE_ROOT, "mmidas", "_utils.py")
_UTIL_FUNCS = ("to_np", "mk_masks", "reassign", "classify", "compute_confmat", "confmat_normalize", "confmat_mean")


def _functions(path, names, ns):
    with open(path, "r") as fh:
        tree = ast.parse(fh.read(), filename=path)
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert len(keep) == len(names), (path, names)
    for fn in keep:
        fn.decorator_list = []                      # generate / mk_masks: @unstable only warns
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, "exec"), ns)
    return ns


def load_reference_evals():
    """(generate, evals2) of the reference, compiled in memory and wired to each other through stub modules."""
    from typing import Any, Mapping

    from scipy.optimize import linear_sum_assignment
    from torch import nn
    from tqdm import tqdm
    uns = _functions(_UTILS, _UTIL_FUNCS, {"np": np, "th": torch, "linear_sum_assignment": linear_sum_assignment})
    mns = _functions(_MODEL, ("generate",), {"np": np, "th": torch, "nn": nn, "DataLoader": DataLoader, "tqdm": tqdm,
                                             "Mapping": Mapping, "Any": Any, "mk_masks": uns["mk_masks"],
                                             "to_np": uns["to_np"]})
    pkg, m_model, m_utils = types.ModuleType("mmidas"), types.ModuleType("mmidas.model"), types.ModuleType("mmidas._utils")
    m_model.generate = mns["generate"]
    for k in _UTIL_FUNCS:
        setattr(m_utils, k, uns[k])
    pkg.model, pkg._utils = m_model, m_utils
    sys.modules.update({"mmidas": pkg, "mmidas.model": m_model, "mmidas._utils": m_utils})
    ens = _functions(_EVALS, ("evals2",), {"np": np, "nn": nn, "DataLoader": DataLoader, "tqdm": tqdm, "Mapping": Mapping,
                                           "Any": Any})
    return mns["generate"], ens["evals2"]


def _model(ref, seed):
    torch.manual_seed(seed)
    m = ref.mixVAE_model(input_dim=D, fc_dim=H, n_categories=C, state_dim=S, lowD_dim=L, x_drop=0.5, s_drop=0.2, n_arm=A,
                         lam=1, lam_pc=1, tau=0.005, beta=1.0, hard=False, variational=True, device="cpu", eps=1e-8,
                         momentum=0.01, ref_prior=False, loss_mode="MSE")
    g = torch.Generator().manual_seed(seed + 1000)
    with torch.no_grad():
        for name, buf in m.named_buffers():
            if name.endswith("running_mean"):
                buf.copy_(0.3 * torch.randn(buf.shape, generator=g, dtype=torch.float64))
            elif name.endswith("running_var"):
                buf.copy_(0.5 + torch.rand(buf.shape, generator=g, dtype=torch.float64))
        for p in m.parameters():
            p.mul_(1.5)
        for a in range(A):
            m.fcc[a].bias[PRUNED] = 0.0
    return m.eval()


def _ok(gen):
    top = np.sort(gen["cs"], axis=-1)
    margin = float((top[..., -1] - top[..., -2]).min())
    labels = [len(np.unique(p)) for p in gen["preds"]]
    return margin > MARGIN and min(labels) >= 2, margin, labels


def _store(out, prefix, ev):
    for k, v in ev.items():
        arr = np.asarray(v, dtype=np.float64) if not isinstance(v, np.ndarray) else v
        out[f"{prefix}/{k}"] = arr


def main():
    ref = RL.load_reference_nn_model()
    generate, evals2 = load_reference_evals()
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        g = torch.Generator().manual_seed(31)
        x = torch.relu(torch.randn(N, D, generator=g, dtype=torch.float64)) * 2
        dl = DataLoader(TensorDataset(x, torch.arange(N, dtype=torch.float64)), batch_size=BATCH, shuffle=False)
        models, gens, seed = [], [], 5
        while len(models) < 2:
            m = _model(ref, seed)
            gen = generate(m, dl)
            ok, margin, labels = _ok(gen)
            print(f"seed {seed}: margin {margin:.3e}, labels per arm {labels} -> {'kept' if ok else 'skipped'}")
            if ok:
                models.append(m)
                gens.append(gen)
            seed += 1
            assert seed < 200, "no seed with a safe label margin"
        for m, gen in zip(models, gens):          # the asserted properties of what is stored
            ok, margin, labels = _ok(gen)
            assert ok and margin > MARGIN and min(labels) >= 2
        fa, fb = models
        out = {"x": x.numpy(), "cfg": np.array([A, N, D, H, L, C, S, BATCH, PRUNED], np.int64)}
        for tag, m, gen in (("a", fa, gens[0]), ("b", fb, gens[1])):
            for k, v in m.state_dict().items():
                out[f"sd_{tag}/{k}"] = v.detach().cpu().numpy().copy()
            for k in ("preds", "cs", "inds_prune", "pruning_mask"):
                out[f"gen_{tag}/{k}"] = np.asarray(gen[k])
        _store(out, "ab", evals2(fa, fb, dl))
        _store(out, "aa", evals2(fa, fa, dl))
    finally:
        torch.set_default_dtype(old)
    path = os.path.join(GOLDEN, "evals2_a3.npz")
    np.savez_compressed(path, **out)
    print({k: v.shape for k, v in out.items() if "sd_" not in k}, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

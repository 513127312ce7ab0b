"""Bit identity of the ZINB entries on d10 across builds: zinb_nll, zinb_head_grads, zinb_d10_grad, zinb_step_grads,
zinb_terms_grad and zinb_sample (csrc/zinb.hip, zinb_grad.hip, countdist.hip and what they share, csrc/zb_tile.hpp and
zinb_core.hpp).

Every case calls the wrappers of distributed_vae_amd._native on inputs drawn from a seeded numpy.random.Generator(PCG64) and
takes the SHA-256 of the raw bytes of every output tensor.  The kernels use no atomics and add in a fixed order, so equal
digests are the gate of a change that must not alter what they compute.

    MMVAE_LIB=<the parent commit's libmmvae_hip.so> python tools/zinb_grad_digest.py --out parent.json
    python tools/zinb_grad_digest.py --out head.json
    python tools/zinb_grad_digest.py --compare parent.json head.json --out profiles/zinb_grad_refactor_bits.json

One process a library; the last form needs no GPU, writes both sets of digests to one file and fails unless they are equal.

The shapes (N, D, H) are the edge cases, not the workload: one element; less than a tile with H = 1; one cell, gene and
column past a tile, H odd; five cell tiles and three gene tiles at H = 100 (two workgroups a CU) and at H = 128 (the largest,
one a CU).  Head masks 7, 6 and 1; segments 0 (the library's rule), 2 and 5."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = ((1, 1, 1), (63, 31, 1), (65, 33, 7), (257, 130, 100), (257, 130, 128))
MASKS = {7: ("rec", "p", "r"), 6: ("p", "r"), 1: ("rec",)}
SEGMENTS = (0, 2, 5)


def _inputs(n, D, H, dev):
    import torch
    rng = np.random.Generator(np.random.PCG64(1000 * n + 10 * D + H))
    f = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    d10 = f(rng.standard_normal((n, H)))
    layers = []
    for _ in range(3):
        layers += [f(0.3 * rng.standard_normal((D, H))), f(0.3 * rng.standard_normal(D))]
    X = f(np.log1p(rng.poisson(0.8, size=(n, D))))           # about half of the elements take the X = 0 branch
    given = [f(rng.gamma(2.0, 1.0, size=(n, D))), f(rng.uniform(0.02, 0.98, size=(n, D))), f(rng.uniform(0.02, 0.98, size=(n, D)))]
    return d10, layers, X, given


def digests(device="cuda:0"):
    """{case: sha256 hex} of every output of every case with the library that is loaded."""
    import torch

    import distributed_vae_amd  # noqa: F401
    from distributed_vae_amd import _native as N
    dev, out = torch.device(device), {}

    def put(case, **tensors):
        torch.cuda.synchronize()
        for k, t in tensors.items():
            out[f"{case}/{k}"] = hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()

    for n, D, H in SHAPES:
        d10, L, X, given = _inputs(n, D, H, dev)
        shape = f"N{n}_D{D}_H{H}"
        cell, gene = N.zinb_nll(d10, *L, X)
        put(f"{shape}/nll", cell=cell, gene=gene)
        g_rec, g_p, g_r = N.zinb_terms_grad(*given, X, scale=0.25)
        put(f"{shape}/terms_grad", g_rec=g_rec, g_p=g_p, g_r=g_r)
        put(f"{shape}/sample", x=N.zinb_sample(d10, *L, seed=7, offset=3))
        for mask, heads in MASKS.items():
            for seg in SEGMENTS:
                case = f"{shape}/mask{mask}_seg{seg}"
                grads, cell, gene = N.zinb_head_grads(d10, *L, X, heads=heads, segments=seg)
                flat = {f"{h}_{k}": t for h, pair in grads.items() for k, t in zip(("dW", "db"), pair)}
                put(case + "/head_grads", cell=cell, gene=gene, **flat)
                put(case + "/d10_grad", gd10=N.zinb_d10_grad(d10, *L, X, heads=heads, segments=seg))
                grads, cell, gene, gd10 = N.zinb_step_grads(d10, *L, X, heads=heads, segments=seg)
                flat = {f"{h}_{k}": t for h, pair in grads.items() for k, t in zip(("dW", "db"), pair)}
                put(case + "/step_grads", cell=cell, gene=gene, gd10=gd10, **flat)
    return {"library": N.LIB_PATH, "device": torch.cuda.get_device_name(0), "sha256": out}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", required=True)
    ap.add_argument("--compare", nargs=2, metavar=("PARENT", "HEAD"), help="two files this tool wrote: no GPU is used")
    a = ap.parse_args()
    if a.compare:
        parent, head = (json.load(open(p)) for p in a.compare)
        differ = sorted(k for k in set(parent["sha256"]) | set(head["sha256"]) if parent["sha256"].get(k) != head["sha256"].get(k))
        res = {"what": __doc__.split("\n\n")[0].replace("\n", " "), "digests": len(head["sha256"]), "equal": not differ, "differ": differ,
               "parent": parent, "head": head}
    else:
        res = digests()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    if a.compare:
        print(f"{res['digests']} digests: " + ("all equal" if res["equal"] else "DIFFER in " + ", ".join(differ)))
        return 0 if res["equal"] else 1
    print(f"wrote {a.out}: {len(res['sha256'])} digests with {res['library']}")
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""Bit identity of the tile-engine GEMMs (k_x3_gemm, k_x3_small, k_bf16_gemm; csrc/gemm_bf16.hip) across builds.

Every case runs one fused train step (do_adam=False) with fixed seeds and takes the SHA-256 of the raw bytes of what depends
on these kernels: the loss vector, the flat gradient (dW1, [dW11 | db11] and the small-layer gradients are their products),
the BatchNorm running statistics, and the workspace arrays R1 (behind fc1) and DZ1 (dW1's operand).  The split-K slabs
themselves have no workspace id (mmvae_ws_offset), so they are covered through their reductions: R1 and the gradient.

    MMVAE_LIB=<the parent commit's libmmvae_hip.so> python tools/gemm_bits.py --write

writes tests/golden/gemm_bits.npz (digests and shapes only) with the library of the commit a change must stay bit-identical
to; tests/test_gpu_gemm_bits.py recomputes the digests with the tree's library and compares.  Without --write the tool
prints the digests' verdicts and every case's split factors.

The cases are the smallest shapes at which these kernels can go wrong (H = 100, L = 10, C = 92, S = 2 everywhere):
  * tiles along cells (fc1): B = 50 one tile, the block's second group idle; 130 two tiles, the second ragged; 300 three,
    so the last block's second group is idle;
  * tiles along genes (dW1, dW11): D = 96 and 100 one tile, 256 two full ones, 260 three (the last four genes wide);
  * K tails: D = 100 ends inside a 32-wide K tile of fc1, D = 96 is exactly three K tiles; B = 50, 97, 130 end the K-minor
    tiles of dW1, dW11 and the small products at k counts that are no multiples of 2 or 4;
  * keep mask: x_drop = 0.5 (in-kernel Philox noise; one case with explicit noise) against x_drop = 0, a null mask pointer;
  * row map: fused_train_step_rows on a fixed permutation of a resident matrix of 2 B rows (the IDX instantiations; the library
    offers the row map only under input dropout, so these cases all carry the mask);
  * arms: A = 1, 2, 3 (A = 3: k_x3_small has an odd number of (product, arm) units, one idle group);
  * K splits: the layout splits K at these shapes already -- fc1 min(16, ceil(D / 32)) ways, dW1, dW11 and the small products
    up to ceil(B / 32) ways.  EVERY case asserts that fc1, dW1, dW11 and k_x3_small each run on more than one K split; the
    widest are B = 300, D = 256 (fc1 8, dW1 / dW11 / small 10 ways) and B = 130, D = 260 (fc1 9, the others 5 ways); the tool
    prints the factors of every case;
  * "bf16": the one-plane engine (k_bf16_gemm), which shares the piece helpers and the epilogue: on the batch, through the row
    map on the fp32 matrix (fp32 pieces through the map) and through the row map on the matrix's bf16 copy.
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
GOLDEN = os.path.join(ROOT, "tests", "golden", "gemm_bits.npz")

H, L, C, S = 100, 10, 92, 2

# name: engine, A, B, D, x_drop, noise, rows
#   engine "x3": gemm_dtype fp32 (fp32x3 engine);  "bf16": gemm_dtype bf16
#   noise  "philox": drawn in the kernels from a fixed seed;  "explicit": arrays handed in
#   rows   False: fused_train_step on the batch;  True: fused_train_step_rows on a permutation of a 2 B-row matrix (the bf16
#          engine: on its bf16 copy);  "fp32": the bf16 engine through the row map on the fp32 matrix itself
CASES = {
    "x3_b50_d96_a2_drop":      ("x3", 2, 50, 96, 0.5, "philox", False),
    "x3_b130_d100_a1":         ("x3", 1, 130, 100, 0.0, "philox", False),
    "x3_b300_d256_a2_drop":    ("x3", 2, 300, 256, 0.5, "philox", False),
    "x3_b97_d260_a3":          ("x3", 3, 97, 260, 0.0, "philox", False),
    "x3_b130_d260_a3_drop_x":  ("x3", 3, 130, 260, 0.5, "explicit", False),
    "x3_b50_d100_a2":          ("x3", 2, 50, 100, 0.0, "philox", False),
    "x3_b97_d256_a1_drop":     ("x3", 1, 97, 256, 0.5, "philox", False),
    "x3_rows_b97_d100_a2":     ("x3", 2, 97, 100, 0.5, "philox", True),
    "x3_rows_b130_d260_a1":    ("x3", 1, 130, 260, 0.5, "philox", True),
    "bf16_b97_d100_a2_drop":   ("bf16", 2, 97, 100, 0.5, "philox", False),
    "bf16_rows_b130_d96_a2":   ("bf16", 2, 130, 96, 0.5, "philox", True),
    "bf16_rows32_b97_d100_a2": ("bf16", 2, 97, 100, 0.5, "philox", "fp32"),
}
KEYS = ("loss", "grad", "bn_running", "R1", "DZ1")
SPLIT_NAMES = ("fc1", "fc11", "dw1", "small", "gd10", "dw11")


def expected_keys(name):
    return set(KEYS)


def _digest(t: torch.Tensor):
    a = t.detach().contiguous().cpu().numpy()
    return hashlib.sha256(a.tobytes()).digest(), tuple(a.shape)


def run_case(name, device="cuda:0", splits_out=None):
    """{array name: (sha256 digest (bytes), shape)} of one case with the library that is loaded."""
    import distributed_vae_amd  # noqa: F401
    from distributed_vae_amd import _native as N
    from distributed_vae_amd.nn_model import mixVAE_model
    from oracle import restatement as R

    engine, A, B, D, x_drop, noise_kind, rows = CASES[name]
    h = R.Hyper(input_dim=D, fc_dim=H, n_categories=C, state_dim=S, lowD_dim=L, x_drop=x_drop, s_drop=0.0, n_arm=A, hard=False)
    sd = R.init_state_dict(h, 546)
    m = mixVAE_model(input_dim=D, fc_dim=H, n_categories=C, state_dim=S, lowD_dim=L, x_drop=x_drop, s_drop=0.0, n_arm=A,
                     lam=h.lam, lam_pc=1, tau=h.tau, beta=h.beta, hard=False, variational=True, device=device, eps=h.eps,
                     momentum=h.momentum, ref_prior=False, loss_mode="MSE")
    m.load_state_dict(sd)
    m = m.to(device)
    m.gemm_dtype = "fp32" if engine == "x3" else "bf16"
    data16 = None
    if rows:
        data = R.synthetic_batch(2 * B, D, seed=21).to(device)
        idx = torch.randperm(2 * B, generator=torch.Generator("cpu").manual_seed(5))[:B].to(device)
        if engine == "bf16" and rows != "fp32":
            data16 = N.to_bf16(data)
    else:
        x = R.synthetic_batch(B, D).to(device)
    plan = N.debug_plan(N.Dims(A, B, D, H, L, C, S), m._hyper(1.0, False), m._exec, "STEP_ROWS" if rows else "STEP",
                        has_x16=data16 is not None)
    assert plan["big"] == ("GEMM_X3" if engine == "x3" else "GEMM_BF16"), (name, plan["big"])
    assert plan["small_x3"] and bool(plan["rowmap"]) == bool(rows), (name, plan)     # (k_x3_small serves both engines)
    if noise_kind == "explicit":
        nz = R.draw_noise(h, B, seed=3)
        dev_nz = {}
        for k, v in nz.items():
            dev_nz[k] = None
            if v:
                t = torch.stack([torch.as_tensor(a) for a in v])
                dev_nz[k] = (t.to(torch.uint8) if "mask" in k else t.to(torch.float32)).contiguous().to(device)
        m.set_explicit_noise(dev_nz)
    else:
        m._noise_seed, m._noise_offset = 0x5EED0123456789, 6
    m.train()
    if rows:
        buf = m.fused_train_step_rows(data, idx, 1.0, None, do_adam=False, data16=data16)
    else:
        buf = m.fused_train_step(x.expand(A, -1, -1), 1.0, None, do_adam=False)
    torch.cuda.synchronize()
    eng = m._ensure(B)
    sp = dict(zip(SPLIT_NAMES, eng.splits()))
    assert min(sp["fc1"], sp["dw1"], sp["dw11"], sp["small"]) > 1, (name, sp)     # every kernel on more than one K split
    if splits_out is not None:
        splits_out[name] = sp
    out = {"loss": _digest(buf), "grad": _digest(m.flat_grad()), "bn_running": _digest(m._bn_flat)}
    out["R1"] = _digest(eng.ws_view("r1", H))
    out["DZ1"] = _digest(eng.ws_view("dz1", H))
    return out


def load_golden(path=GOLDEN):
    """{case: {array: (digest, shape)}}"""
    z = np.load(path)
    gold = {}
    for k in z.files:
        if k.endswith("/shape"):
            continue
        case, arr = k.split("/")
        gold.setdefault(case, {})[arr] = (z[k].tobytes(), tuple(int(v) for v in z[k + "/shape"]))
    return gold


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--write", action="store_true", help="write tests/golden/gemm_bits.npz from the loaded library")
    ap.add_argument("--out", default=GOLDEN)
    args = ap.parse_args()
    from distributed_vae_amd import _native as N
    print("library:", N.LIB_PATH)
    splits = {}
    got = {name: run_case(name, splits_out=splits) for name in CASES}
    for name, sp in splits.items():
        print(f"{name}: splits {sp}")
    if args.write:
        again = {name: run_case(name) for name in CASES}          # a digest that differs run to run is no reference
        assert again == got, [n for n in CASES if again[n] != got[n]]
        flat = {}
        for case, arrs in got.items():
            assert set(arrs) == expected_keys(case), case
            for arr, (dg, shape) in arrs.items():
                flat[f"{case}/{arr}"] = np.frombuffer(dg, dtype=np.uint8)
                flat[f"{case}/{arr}/shape"] = np.asarray(shape, dtype=np.int64)
        np.savez(args.out, **flat)
        print(f"wrote {args.out}: {len(got)} cases, {sum(len(v) for v in got.values())} digests")
        return 0
    gold = load_golden(args.out)
    bad = 0
    for case in CASES:
        diff = sorted(k for k in set(gold[case]) | set(got[case]) if gold[case].get(k) != got[case].get(k))
        bad += bool(diff)
        print(f"{case}: {'identical' if not diff else 'DIFFERS in ' + ', '.join(diff)}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

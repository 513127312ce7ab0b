"""Bit identity of the chain kernels (k_chain_fwd, k_chain_fwd_couple, k_chain_bwd; csrc/chain.hip) across builds.

Every case runs one call with fixed seeds and takes the SHA-256 of the raw bytes of what the chain kernels write and of
what depends on it: the loss vector, the flat gradients, the BatchNorm running statistics, and the workspace arrays
R2..R5, D6..D10 (forward), G1..G4, DZ2..DZ5, DZ1 and the gd10-dependent G5 (backward); a decode call gives D6..D10 and the
reconstruction.

    MMVAE_LIB=<the parent commit's libmmvae_hip.so> python tools/chain_bits.py --write

writes tests/golden/chain_bits.npz (digests and shapes only) with the library of the commit a change must stay
bit-identical to; tests/test_gpu_chain_bits.py recomputes the digests with the tree's library and compares.  Without
--write the tool prints the digests of the loaded library and compares them with the file.

The cases are the smallest shapes at which these kernels can go wrong (D = 96, L = 10, C = 92, S = 2 everywhere): B = 50 is
one ragged 64-row block, 97 one full and one ragged, 130 two full and a 2-row block; H = 100 leaves K and N tails of 4 in
the 32-wide tiles, H = 128 and H = 96 none; A = 1, 2, 3, 5 (the coupling role of the decoder launch exists from two arms up
and is instantiated per arm count).  "x3" is the default engine: k_chain_*<true> up to H = 124 (make_plan: chain_planes),
so its no-tail width is H = 96, and at H = 128 it runs k_chain_*<false>; "f32" is the fp32 matrix-instruction engine and
"cf" the default engine with the chains' own GEMMs held on the fp32 matrix instruction (both k_chain_*<false>).
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
GOLDEN = os.path.join(ROOT, "tests", "golden", "chain_bits.npz")

D, L, C, S = 96, 10, 92, 2
TUNE_CHAIN_FP32 = 21        # csrc/tune.h MMVAE_TUNE_CHAIN_FP32

# name: form, A, B, H, kind, noise, mask
#   form   "x3": gemm_dtype fp32 (fp32x3 engine);  "f32": gemm_dtype fp32_mfma;  "cf": fp32x3 engine, chains on fp32
#   kind   "step": one fused train step;  "eval": forward(eval=True) of a model in eval mode;  "decode": mixVAE_model.decoder
#   noise  "philox": drawn in the kernels from a fixed seed;  "explicit": arrays handed in
#   mask   None, or the kept categories (a pruned step)
MASK = list(range(0, 92, 3)) + [91]
CASES = {
    "x3_b50_h100_a2_step":     ("x3", 2, 50, 100, "step", "philox", None),
    "x3_b97_h100_a1_step":     ("x3", 1, 97, 100, "step", "philox", None),
    "x3_b130_h100_a3_step_x":  ("x3", 3, 130, 100, "step", "explicit", None),
    "x3_b97_h128_a5_step":     ("x3", 5, 97, 128, "step", "philox", None),
    "x3_b130_h128_a2_step":    ("x3", 2, 130, 128, "step", "philox", None),
    "x3_b50_h100_a5_step":     ("x3", 5, 50, 100, "step", "philox", None),
    "x3_b97_h100_a2_mask":     ("x3", 2, 97, 100, "step", "philox", MASK),
    "x3_b130_h100_a2_eval":    ("x3", 2, 130, 100, "eval", "philox", None),
    "x3_b50_h96_a3_eval":      ("x3", 3, 50, 96, "eval", "philox", None),
    "x3_b130_h96_a2_step":     ("x3", 2, 130, 96, "step", "philox", None),
    "x3_b97_h100_a2_decode":   ("x3", 2, 97, 100, "decode", "philox", None),
    "x3_b130_h96_a1_decode":   ("x3", 1, 130, 96, "decode", "philox", None),
    "f32_b50_h100_a2_step":    ("f32", 2, 50, 100, "step", "philox", None),
    "f32_b130_h128_a3_step_x": ("f32", 3, 130, 128, "step", "explicit", None),
    "f32_b97_h100_a5_step":    ("f32", 5, 97, 100, "step", "philox", None),
    "f32_b97_h128_a1_mask":    ("f32", 1, 97, 128, "step", "philox", MASK),
    "f32_b97_h100_a2_eval":    ("f32", 2, 97, 100, "eval", "philox", None),
    "f32_b130_h100_a2_decode": ("f32", 2, 130, 100, "decode", "philox", None),
    "cf_b97_h100_a2_step":     ("cf", 2, 97, 100, "step", "philox", None),
    "cf_b130_h128_a3_step":    ("cf", 3, 130, 128, "step", "philox", None),
    "cf_b50_h100_a2_eval":     ("cf", 2, 50, 100, "eval", "philox", None),
}
# (key, workspace region, width: "H" or "L")
FWD_ENC = (("R2", "r2", "H"), ("R3", "r3", "H"), ("R4", "r4", "H"), ("R5", "r5", "L"))
FWD_DEC = (("D6", "d6", "L"), ("D7", "d7", "H"), ("D8", "d8", "H"), ("D9", "d9", "H"), ("D10", "d10", "H"))
BWD = (("G1", "g1", "H"), ("G2", "g2", "H"), ("G3", "g3", "H"), ("G4", "g4", "H"), ("G5", "g5", "L"),
       ("DZ1", "dz1", "H"), ("DZ2", "dz2", "H"), ("DZ3", "dz3", "H"), ("DZ4", "dz4", "H"), ("DZ5", "dz5", "L"))


def expected_keys(name):
    kind = CASES[name][4]
    if kind == "decode":
        return {"x_rec"} | {k for k, _, _ in FWD_DEC}
    if kind == "eval":
        return {"bn_running"} | {k for k, _, _ in FWD_ENC}
    return {"loss", "grad", "bn_running"} | {k for k, _, _ in FWD_ENC + FWD_DEC + BWD}


def _digest(t: torch.Tensor):
    a = t.detach().contiguous().cpu().numpy()
    return hashlib.sha256(a.tobytes()).digest(), tuple(a.shape)


def run_case(name, device="cuda:0"):
    """{array name: (sha256 digest (bytes), shape)} of one case with the library that is loaded."""
    import distributed_vae_amd  # noqa: F401
    from distributed_vae_amd import _native as N
    from distributed_vae_amd.nn_model import mixVAE_model
    from oracle import restatement as R

    form, A, B, H, kind, noise_kind, mask = CASES[name]
    h = R.Hyper(input_dim=D, fc_dim=H, n_categories=C, state_dim=S, lowD_dim=L, x_drop=0.0, s_drop=0.0, n_arm=A, hard=False)
    sd = R.init_state_dict(h, 546)
    x = R.synthetic_batch(B, D).to(device)
    m = mixVAE_model(input_dim=D, fc_dim=H, n_categories=C, state_dim=S, lowD_dim=L, x_drop=0.0, s_drop=0.0, n_arm=A,
                     lam=h.lam, lam_pc=1, tau=h.tau, beta=h.beta, hard=False, variational=True, device=device, eps=h.eps,
                     momentum=h.momentum, ref_prior=False, loss_mode="MSE")
    m.load_state_dict(sd)
    m = m.to(device)
    m.gemm_dtype = "fp32_mfma" if form == "f32" else "fp32"
    if form == "cf":
        ex = N.exec_from_env(N.gemm_mode(m.gemm_dtype))
        ex.tune[TUNE_CHAIN_FP32] = 1
        m._exec = ex
    hy = m._hyper(1.0, False)
    plan = N.debug_plan(N.Dims(A, B, D, H, L, C, S), hy, m._exec, "STEP")
    assert bool(plan["chain_planes"]) == (form == "x3" and H <= 124), (name, plan["chain_planes"])
    width = {"H": H, "L": L}
    out = {}
    if kind == "decode":
        m.eval()
        g = torch.Generator("cpu").manual_seed(11)
        c = torch.softmax(4.0 * torch.randn(B, C, generator=g), dim=1).to(device)
        s = torch.randn(B, S, generator=g).to(device)
        arm = A - 1
        out["x_rec"] = _digest(m.decoder(c, s, arm))
        torch.cuda.synchronize()
        eng = m._dec_engine(1, B)
        for key, ws_name, w in FWD_DEC:
            out[key] = _digest(eng.ws_view(ws_name, width[w]))
        return out
    if noise_kind == "explicit":
        nz = R.draw_noise(h, B, seed=3, training=kind != "eval", eval_flag=kind != "step")
        dev_nz = {}
        for k, v in nz.items():
            dev_nz[k] = None
            if v:
                t = torch.stack([torch.as_tensor(a) for a in v])
                dev_nz[k] = (t.to(torch.uint8) if "mask" in k else t.to(torch.float32)).contiguous().to(device)
        m.set_explicit_noise(dev_nz)
    else:
        m._noise_seed, m._noise_offset = 0x5EED0123456789, 6
    xs = x.expand(A, -1, -1)
    if kind == "step":
        m.train()
        buf = m.fused_train_step(xs, 1.0, None, do_adam=False, mask=mask)
        torch.cuda.synchronize()
        out["loss"] = _digest(buf)
        out["grad"] = _digest(m.flat_grad())
    else:
        m.eval()
        with torch.no_grad():
            m(xs, 1.0, eval=True)
        torch.cuda.synchronize()
    out["bn_running"] = _digest(m._bn_flat)
    eng = m._ensure(B)
    for key, ws_name, w in FWD_ENC + (FWD_DEC + BWD if kind == "step" else ()):
        out[key] = _digest(eng.ws_view(ws_name, width[w]))
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
    ap.add_argument("--write", action="store_true", help="write tests/golden/chain_bits.npz from the loaded library")
    ap.add_argument("--out", default=GOLDEN)
    args = ap.parse_args()
    from distributed_vae_amd import _native as N
    print("library:", N.LIB_PATH)
    got = {name: run_case(name) for name in CASES}
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

"""Bit identity of the latent kernels (k_lat_fwd[_h], k_lat_bwd[_h]) across builds.

Every case runs one call with fixed seeds and takes the SHA-256 of the raw bytes of what the latent kernels write and of
what depends on it: the loss vector, the flat gradients, the BatchNorm running statistics, and the workspace arrays
XLOW, CPROB, CC, YSOFT, CSMP, MU, LV, SS (forward) and GMS, GZC, G5 (backward).

    MMVAE_LIB=<the parent commit's libmmvae_hip.so> python tools/latent_bits.py --write

writes tests/golden/latent_bits.npz (digests and shapes only) with the library of the commit a change must stay
bit-identical to; tests/test_gpu_latent_bits.py recomputes the digests with the tree's library and compares.  Without
--write the tool prints the digests of the loaded library and compares them with the file.

The cases are the smallest shapes at which these kernels can go wrong (D = 96, H = 100, L = 10, S = 2 everywhere):
B = 50 and 97 leave the last workgroup ragged for the 8-cell (backward) and 48-cell (forward) blocks; C = 92 is three
columns per lane with a tail in the half-wave form, C = 32 / 33 / 64 the lane-count edges; C = 97 / 100 / 128 are the wave
form (make_plan: lat_half iff C <= 96, L <= 32, 2 S <= 32; a shape has one form, so the wave form has cases of its own).
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
GOLDEN = os.path.join(ROOT, "tests", "golden", "latent_bits.npz")

D, H, L, S = 96, 100, 10, 2

# name: A, B, C, s_drop, hard, kind, noise, mask
#   kind   "step": one fused train step;  "eval": one eval-mode forward;  "evalflag": forward(eval=True) of a model in
#          training mode, loss and backward (the backward kernel's eval_flag branch)
#   noise  "philox": drawn in the kernels from a fixed seed;  "explicit": arrays handed in
#   mask   None, or the kept categories
CASES = {
    # half-wave form
    "h_b50_c92_a2_soft":      (2, 50, 92, 0.0, False, "step", "philox", None),
    "h_b97_c92_a2_hard_sd":   (2, 97, 92, 0.25, True, "step", "philox", None),
    "h_b50_c32_a1_soft_sd":   (1, 50, 32, 0.25, False, "step", "philox", None),
    "h_b97_c33_a3_hard":      (3, 97, 33, 0.0, True, "step", "philox", None),
    "h_b50_c64_a5_soft_sd":   (5, 50, 64, 0.25, False, "step", "philox", None),
    "h_b97_c92_a5_hard":      (5, 97, 92, 0.0, True, "step", "philox", None),
    "h_b97_c92_a3_soft_sd_x": (3, 97, 92, 0.25, False, "step", "explicit", None),
    "h_b50_c33_a2_hard_x":    (2, 50, 33, 0.0, True, "step", "explicit", None),
    "h_b97_c92_a2_mask":      (2, 97, 92, 0.25, False, "step", "philox", list(range(0, 92, 3)) + [91]),
    "h_b50_c33_a2_eval":      (2, 50, 33, 0.0, False, "eval", "philox", None),
    "h_b97_c92_a2_evalflag":  (2, 97, 92, 0.0, False, "evalflag", "explicit", None),
    # wave form
    "w_b50_c97_a2_soft_sd":   (2, 50, 97, 0.25, False, "step", "philox", None),
    "w_b97_c128_a3_hard":     (3, 97, 128, 0.0, True, "step", "philox", None),
    "w_b50_c100_a1_soft_x":   (1, 50, 100, 0.0, False, "step", "explicit", None),
    "w_b97_c97_a5_soft":      (5, 97, 97, 0.0, False, "step", "philox", None),
    "w_b50_c100_a2_mask":     (2, 50, 100, 0.0, True, "step", "philox", list(range(1, 100, 2))),
    "w_b97_c97_a2_eval":      (2, 97, 97, 0.0, False, "eval", "philox", None),
}
FWD = (("XLOW", "x_low", "L"), ("CPROB", "c_prob", "C"), ("CC", "c", "C"), ("YSOFT", "y_soft", "C"), ("CSMP", "c_smp", "C"),
       ("MU", "s_mean", "S"), ("LV", "s_logvar", "S"), ("SS", "s_smp", "S"))


def _digest(t: torch.Tensor):
    a = t.detach().contiguous().cpu().numpy()
    return hashlib.sha256(a.tobytes()).digest(), tuple(a.shape)


def _gms(eng, A, B, C):
    """GMS has no workspace id: make_layout (csrc/api.hip) places it between GZIN and GZC, every region rounded up to 64
    floats."""
    from distributed_vae_amd import _native as N
    import ctypes

    def off(name):
        return int(N.lib().mmvae_ws_offset(ctypes.byref(eng.dims), eng._x(), N.WS_IDS[name]))
    up = lambda n: (n + 63) // 64 * 64
    o = off("gzin") + up(A * B * (C + S))
    assert o + up(A * B * 2 * S) == off("gzc"), "workspace layout: GMS is no longer between GZIN and GZC"
    return eng.ws[o: o + A * B * 2 * S].view(A, B, 2 * S)


def run_case(name, device="cuda:0"):
    """{array name: (sha256 digest (bytes), shape)} of one case with the library that is loaded."""
    import distributed_vae_amd  # noqa: F401
    from distributed_vae_amd import _native as N
    from distributed_vae_amd.nn_model import mixVAE_model
    from oracle import restatement as R

    A, B, C, s_drop, hard, kind, noise_kind, mask = CASES[name]
    h = R.Hyper(input_dim=D, fc_dim=H, n_categories=C, state_dim=S, lowD_dim=L, x_drop=0.0, s_drop=s_drop, n_arm=A, hard=hard)
    sd = R.init_state_dict(h, 546)
    x = R.synthetic_batch(B, D).to(device)
    m = mixVAE_model(input_dim=D, fc_dim=H, n_categories=C, state_dim=S, lowD_dim=L, x_drop=0.0, s_drop=s_drop, n_arm=A,
                     lam=h.lam, lam_pc=1, tau=h.tau, beta=h.beta, hard=hard, variational=True, device=device, eps=h.eps,
                     momentum=h.momentum, ref_prior=False, loss_mode="MSE")
    m.load_state_dict(sd)
    m = m.to(device)
    half = N.debug_plan(N.Dims(A, B, D, H, L, C, S), m._hyper(1.0, False), None, "STEP")["lat_half"]
    assert half == name.startswith("h_"), (name, half)
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
    out = {}
    if kind == "step":
        m.train()
        buf = m.fused_train_step(xs, 1.0, None, do_adam=False, mask=mask)
        torch.cuda.synchronize()
        out["loss"] = _digest(buf)
        out["grad"] = _digest(m.flat_grad())
    elif kind == "evalflag":
        m.train()
        o = m(xs, 1.0, eval=True)
        lt = m.loss(o[0], [], [], xs, o[7], o[8], o[4], o[6], 0.0)
        m.zero_grad()
        lt[0].backward()
        torch.cuda.synchronize()
        out["loss"] = _digest(lt[0].detach())
        out["grad"] = _digest(m.flat_grad())
    else:
        m.eval()
        with torch.no_grad():
            m(xs, 1.0, eval=True, mask=mask)
        torch.cuda.synchronize()
    out["bn_running"] = _digest(m._bn_flat)
    eng = m._ensure(B)
    width = {"L": L, "C": C, "S": S}
    for key, ws_name, w in FWD:
        out[key] = _digest(eng.ws_view(ws_name, width[w]))
    if kind != "eval":
        out["GMS"] = _digest(_gms(eng, A, B, C))
        out["GZC"] = _digest(eng.ws_view("gzc", C))
        out["G5"] = _digest(eng.ws_view("g5", L))
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
    ap.add_argument("--write", action="store_true", help="write tests/golden/latent_bits.npz from the loaded library")
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

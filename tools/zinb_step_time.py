"""Timing of training under the ZINB objective on synthetic inputs of tools/zinb_decoder_time.py's kind.

  * the single pass over g against the two launches it replaces, one arm at N = 5000, D = 5032, H = 100, in one process,
    warm, HIP-event medians: ``mmvae_zinb_step_grads`` against ``mmvae_zinb_head_grads`` + ``mmvae_zinb_d10_grad`` (each at
    the library's own segment rule, which is what a step composed of them would call), every buffer allocated beforehand;
  * the whole step, ``mixVAE_model.zinb_train_step`` with Adam, at A = 2, B = 5000, D = 5032, H = 100 (C = 92, S = 2, L = 10,
    in-kernel Philox noise), beside ``fused_train_step`` of an MSE model of the same shape on the same batch;
  * torch autograd of the same objective (tests/zinb_step_restatement.py, float32) on the same GPU and inputs: time and the
    peak allocation above the inputs.  A baseline, not library code.

    python tools/zinb_step_time.py [--repeats R] [--out profiles/zinb_step_time.json]"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import distributed_vae_amd  # noqa: F401,E402
from distributed_vae_amd import _native as N  # noqa: E402
from distributed_vae_amd.cpl_mixvae import FusedAdam  # noqa: E402
from distributed_vae_amd.nn_model import mk_vae  # noqa: E402
import zinb_restatement as ZR  # noqa: E402
import zinb_step_restatement as S  # noqa: E402
from oracle import restatement as R  # noqa: E402
from zinb_decoder_time import _inputs  # noqa: E402
from zinb_fit_time import _median_ms, _with_peak  # noqa: E402

A, NB, D, H, CC, SS, LD, SEED = 2, 5000, 5032, 100, 92, 2, 10, 0
DEV = "cuda:0"


def launches(out, repeats):
    acts, _, L, X = _inputs(NB)
    d10 = acts[5].contiguous()
    lib, p, st = N.lib(), N._ptr, N._stream(DEV)
    f32 = dict(dtype=torch.float32, device=DEV)
    g = [torch.empty(D, H, **f32) if k % 2 == 0 else torch.empty(D, **f32) for k in range(6)]
    g2 = [torch.empty_like(t) for t in g]
    cell, gene = torch.empty(NB, dtype=torch.float64, device=DEV), torch.empty(D, dtype=torch.float64, device=DEV)
    cell2, gene2 = torch.empty_like(cell), torch.empty_like(gene)
    gd, gd2 = torch.empty(NB, H, **f32), torch.empty(NB, H, **f32)
    nb = {k: int(getattr(lib, f"mmvae_zinb_{k}_workspace_bytes")(NB, D, H, 0)) for k in ("head_grads", "d10_grad", "step_grads")}
    ws = {k: N._workspace(v, DEV) for k, v in nb.items()}
    sc = 1.0 / (float(NB) * float(D))
    common = (p(d10), H, NB, H, D, *(p(t) for t in L), p(X), D, 1e-6, sc, 7, 0)

    def heads():
        N.check(lib.mmvae_zinb_head_grads(*common, p(ws["head_grads"]), nb["head_grads"], *(p(t) for t in g), p(cell), p(gene), st), "head_grads")

    def d10g():
        N.check(lib.mmvae_zinb_d10_grad(*common, p(ws["d10_grad"]), nb["d10_grad"], p(gd), H, st), "d10_grad")

    def both():
        heads()
        d10g()

    def single():
        N.check(lib.mmvae_zinb_step_grads(*common, p(ws["step_grads"]), nb["step_grads"], *(p(t) for t in g2), p(cell2), p(gene2), p(gd2), H, st),
                "step_grads")

    r = {"workspace_bytes": nb, "d10_segments_two_launch": N.zinb_d10_grad_segments(NB, D, 0), "gene_tiles": -(-D // 64)}
    # A / B / A / B: the two forms alternate, so a drift of the clocks shows as a difference between the two rounds
    for rnd in (1, 2):
        r[f"two_launches_round{rnd}_ms"] = _median_ms(both, repeats)
        r[f"single_pass_round{rnd}_ms"] = _median_ms(single, repeats)
    r["head_grads_ms"], r["d10_grad_ms"] = _median_ms(heads, repeats), _median_ms(d10g, repeats)
    two = min(r["two_launches_round1_ms"], r["two_launches_round2_ms"])
    one = min(r["single_pass_round1_ms"], r["single_pass_round2_ms"])
    r["single_pass_over_two_launches"] = one / two
    both()
    single()
    torch.cuda.synchronize()
    r["heads_and_sums_bit_identical"] = bool(all(torch.equal(a, b) for a, b in zip(g + [cell, gene], g2 + [cell2, gene2])))
    r["gd10_largest_difference_over_largest_entry"] = float((gd - gd2).abs().max() / gd.abs().max())   # (6 segments against 79)
    out["launches_one_arm"] = r


def _model(mode):
    torch.manual_seed(SEED)
    m = mk_vae(CC, SS, D, DEV, fc_dim=H, latent_dim=LD, A=A, mode=mode).to(DEV)
    m.train()
    m.gemm_dtype = "fp32x3"
    return m


def whole_step(out, repeats):
    x = ZR.counts_matrix(NB, D, torch.Generator().manual_seed(SEED + 1)).to(DEV)
    xs = x.expand(A, -1, -1)
    r = {}
    m = _model("ZINB")
    r["zinb_train_step_ms"] = _median_ms(lambda: m.zinb_train_step(xs, 1.0), repeats)
    r["loss_vector_after"] = [float(v) for v in m.zinb_train_step(xs, 1.0).tolist()]
    mse = _model("MSE")
    opt = FusedAdam(mse, lr=1e-3)
    r["mse_fused_train_step_ms"] = _median_ms(lambda: mse.fused_train_step(xs, 1.0, opt, do_adam=True), repeats)
    # torch autograd of the same objective, float32, on the GPU
    h = R.Hyper(input_dim=D, fc_dim=H, n_categories=CC, state_dim=SS, lowD_dim=LD, x_drop=0.5, s_drop=0.2, n_arm=A, tau=0.005)
    sd = {k: v.to(DEV) for k, v in R.init_state_dict(h, SEED).items()}
    sd.update({k: v.to(DEV) for k, v in S.init_heads(h, SEED + 1).items()})
    noise = {k: [t.to(DEV) for t in v] for k, v in R.draw_noise(h, NB, seed=SEED + 2).items()}
    r["torch_autograd_float32_same_objective"] = _with_peak(lambda: S.grads_autograd(dict(sd), [x] * A, h, noise)[3], max(3, repeats // 3))
    r["ratio_torch_over_device"] = r["torch_autograd_float32_same_objective"]["ms"] / r["zinb_train_step_ms"]
    out["whole_step_two_arms"] = r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "zinb_step_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("zinb_step_time needs a GPU")
    out = {"shape": {"A": A, "B": NB, "D": D, "H": H, "C": CC, "S": SS, "L": LD}, "repeats": a.repeats,
           "device": torch.cuda.get_device_name(0)}
    launches(out, a.repeats)
    whole_step(out, a.repeats)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()

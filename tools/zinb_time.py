"""Timing of ZINB inference at the SmartSeq size: N = 22 365 cells, D = 5032 genes, H = 100, A = 2 arms, on synthetic inputs of
the tests' kind (d10 = relu of a normal draw, the gates' pre-activations spread to +-8, X = log1p(counts), counts <= 1000,
about 70 % zeros).

  * HIP-event medians of ``mmvae_zinb_heads``, ``mmvae_zinb_nll`` and ``mmvae_zinb_terms`` (sums only, and with the terms
    written) for one arm; for the fused kernel the multiply-adds of its three products (6 N D H flop) over its time against
    the 155 TF/s the fp32 matrix instruction reaches on this part -- a whole-call rate, not the product phase's share;
  * ``cpl_mixVAE.score_zinb`` end to end from a resident matrix (``DeviceLoader``, batches of --batch cells), wall clock, and
    beside it the eval forwards of the same batches alone, as ``zinb_nll`` runs them (what the scoring pays for the forward,
    the unused mean-head reconstruction included);
  * two baselines, neither of them code of the library: the reference's arithmetic in torch float32 on this host's CPU (the
    three ``F.linear`` heads, then the loss term and its two sums; one run, wall clock), and the same arithmetic composed from
    torch ops on the GPU, which materialises the three N x D heads (HIP events; its peak allocation is recorded);
  * the memory the fused path avoids: three N x D float32 matrices, against its own workspace.

    python tools/zinb_time.py [--repeats R] [--only kernels|score|nll] [--out profiles/zinb_time.json]

``--only nll`` runs mmvae_zinb_nll a few times and nothing else (the window a counter or kernel-trace run wants)."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import distributed_vae_amd  # noqa: F401,E402
from distributed_vae_amd import _native as N  # noqa: E402
from tests import zinb_restatement as ZR  # noqa: E402

NC, D, H, A, SEED = 22365, 5032, 100, 2, 0
MFMA_F32_FLOPS = 155e12
DEV = "cuda:0"


def _median_ms(fn, repeats):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        t.append(e0.elapsed_time(e1))
    t.sort()
    return t[len(t) // 2]


def _wall_ms(fn, repeats):
    fn()
    t = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    t.sort()
    return t[len(t) // 2]


def _inputs(n):
    g = torch.Generator().manual_seed(SEED)
    d10 = torch.relu(torch.randn(n, H, generator=g))
    # the layers' scale from a sample of the cells (the whole product in fp64 on the host would take a minute)
    L = ZR.spread_layers(d10[:512], D, g)
    for j in (2, 4):                      # the sample's +-8 may be exceeded a little by the other cells: pull in by 0.8
        L[j], L[j + 1] = L[j] * 0.8, L[j + 1] * 0.8
    X = ZR.counts_matrix(n, D, g)
    return d10, L, X


def _torch_nll(d10, L, X):
    t = ZR.terms(*ZR.heads(d10, *L), X)
    return t.sum(1), t.sum(0)


def kernels(out, repeats, n):
    d10, L, X = _inputs(n)
    # ---- the host baseline first (nothing else running): the reference's arithmetic in torch float32 on the CPU
    t0 = time.perf_counter()
    cpu_cell, _ = _torch_nll(d10, L, X)
    out["baseline_torch_cpu"] = {"ms": (time.perf_counter() - t0) * 1e3, "threads": torch.get_num_threads(), "runs": 1}
    d10g, Lg, Xg = d10.to(DEV), [t.to(DEV) for t in L], X.to(DEV)
    k = {}
    k["zinb_heads_ms"] = _median_ms(lambda: N.zinb_heads(d10g, *Lg[2:]), repeats)
    k["zinb_nll_ms"] = _median_ms(lambda: N.zinb_nll(d10g, *Lg, Xg), repeats)
    flop = 6.0 * n * D * H
    k["zinb_nll_product_flop"] = flop
    k["zinb_nll_product_flop_per_s_whole_call"] = flop / (k["zinb_nll_ms"] * 1e-3)
    k["zinb_nll_share_of_fp32_mfma_rate_whole_call"] = k["zinb_nll_product_flop_per_s_whole_call"] / MFMA_F32_FLOPS
    k["zinb_nll_elements_per_s"] = n * D / (k["zinb_nll_ms"] * 1e-3)
    heads = [h.contiguous() for h in ZR.heads(d10g, *Lg)]
    k["zinb_terms_sums_only_ms"] = _median_ms(lambda: N.zinb_terms(*heads, Xg), repeats)
    k["zinb_terms_with_terms_written_ms"] = _median_ms(lambda: N.zinb_terms(*heads, Xg, return_terms=True), repeats)
    out["kernels_one_arm"] = k
    # ---- the same arithmetic composed from torch ops on the GPU
    del heads
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ms = _median_ms(lambda: _torch_nll(d10g, Lg, Xg), max(3, repeats // 3))
    out["baseline_torch_gpu"] = {"ms": ms, "peak_bytes_above_inputs": int(torch.cuda.max_memory_allocated() - base)}
    out["memory"] = {"three_heads_bytes_not_written": 3 * 4 * n * D,
                     "zinb_nll_workspace_bytes": int(N.lib().mmvae_zinb_nll_workspace_bytes(n, D))}
    # the two device paths and the host agree (a check of the tool, not a gate)
    cell, _ = N.zinb_nll(d10g, *Lg, Xg)
    tc, _ = _torch_nll(d10g, Lg, Xg)
    scale = float(cpu_cell.abs().max())
    out["agreement"] = {"device_vs_torch_gpu_rel": float((cell - tc.double()).abs().max()) / scale,
                        "device_vs_torch_cpu_rel": float((cell.cpu() - cpu_cell.double()).abs().max()) / scale}


def score(out, repeats, n, batch):
    from distributed_vae_amd.cpl_mixvae import cpl_mixVAE
    from distributed_vae_amd.utils.dataloader import DeviceLoader
    torch.manual_seed(SEED)
    t = cpl_mixVAE(saving_folder="", device=0, save_flag=False)
    t.init_model(n_categories=92, state_dim=2, input_dim=D, fc_dim=H, lowD_dim=10, n_arm=A, temp=1.0, tau=0.005, mode="ZINB")
    data = ZR.counts_matrix(n, D, torch.Generator().manual_seed(SEED + 1)).to(DEV)
    dl = DeviceLoader(data, torch.arange(n), batch, False, False)
    s = {"batch": batch, "batches": len(dl)}
    s["score_zinb_end_to_end_ms"] = _wall_ms(lambda: t.score_zinb(dl), repeats)
    m = t.model.eval()

    def forwards():                      # what zinb_nll runs in front of the fused kernel: the eval forward without the heads
        for x, _ in dl:
            m._forward(x.expand(A, -1, -1), 1.0, True, None, False)
    s["eval_forwards_alone_ms"] = _wall_ms(forwards, repeats)
    r = t.score_zinb(dl)
    s["mean"] = [float(v) for v in r["mean"]]
    out["score_zinb"] = s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--only", choices=["kernels", "score", "nll"], default=None)
    ap.add_argument("--cells", type=int, default=NC)
    ap.add_argument("--batch", type=int, default=5000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "zinb_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("zinb_time needs a GPU")
    if a.only == "nll":
        d10, L, X = _inputs(a.cells)
        d10g, Lg, Xg = d10.to(DEV), [t.to(DEV) for t in L], X.to(DEV)
        for _ in range(3):
            N.zinb_nll(d10g, *Lg, Xg)
        torch.cuda.synchronize()
        return
    out = {"shape": {"N": a.cells, "D": D, "H": H, "A": A}, "repeats": a.repeats, "device": torch.cuda.get_device_name(0)}
    if a.only in (None, "kernels"):
        kernels(out, a.repeats, a.cells)
    if a.only in (None, "score"):
        score(out, max(3, a.repeats // 3), a.cells, a.batch)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()

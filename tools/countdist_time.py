"""Timing of the count distributions at the SmartSeq size: N = 22 365 cells, D = 5032 genes, H = 100, one arm, on synthetic
inputs (x = counts <= 1000 with about 70 % zeros, mu log-normal about 2, theta [D] log-normal about 1, logits normal with
deviation 2; for the fused sampler d10 and layers of tools/zinb_time.py's kind).

  * HIP-event medians of ``mmvae_count_logp`` for each kind, with the terms written and with the sums only;
    of ``mmvae_count_sample`` (NB and ZINB) and of ``mmvae_zinb_sample``; wall clock of ``cpl_mixVAE.sample_counts`` over a
    resident matrix (``DeviceLoader``, batches of --batch cells, one arm; it hands the counts to the host);
  * beside each, the same arithmetic composed from torch ops on the same GPU in float32 -- the reference's formulas for the
    likelihoods, torch's ``Gamma`` and ``poisson`` for the samplers -- with the peak allocation above the inputs;
  * the mean number of Philox calls per element, counted by tests/countdist_restatement.py on the first rows of the same
    inputs.

    python tools/countdist_time.py [--repeats R] [--only logp|sample] [--out profiles/countdist_time.json]

``--only`` runs one group a few times and writes nothing (the window a counter or kernel-trace run wants)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import distributed_vae_amd  # noqa: F401,E402
from distributed_vae_amd import _native as N  # noqa: E402
import countdist_restatement as CR  # noqa: E402
import zinb_restatement as ZR  # noqa: E402

NC, D, H, SEED = 22365, 5032, 100, 0
DEV = "cuda:0"
EPS = 1e-8


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


def _with_peak(fn, repeats):
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ms = _median_ms(fn, repeats)
    return {"ms": ms, "peak_bytes_above_inputs": int(torch.cuda.max_memory_allocated() - base)}


def _inputs(n):
    g = torch.Generator().manual_seed(SEED)
    x = torch.round(torch.expm1(ZR.counts_matrix(n, D, g)))
    r = {"x": x, "mu": torch.exp(0.7 + torch.randn(n, D, generator=g)), "theta": torch.exp(torch.randn(D, generator=g)),
         "pi": 2.0 * torch.randn(n, D, generator=g), "mu2": torch.exp(1.5 + torch.randn(n, D, generator=g)),
         "theta2": torch.exp(torch.randn(D, generator=g))}
    return {k: v.float() for k, v in r.items()}


# the reference's arithmetic, float32 torch ops (its order of operations; its softplus)
def _t_nb(x, mu, th):
    ltm = torch.log(th + mu + EPS)
    return th * (torch.log(th + EPS) - ltm) + x * (torch.log(mu + EPS) - ltm) + torch.lgamma(x + th) - torch.lgamma(th) - torch.lgamma(x + 1)


def _t_zinb(x, mu, th, pi):
    sp = F.softplus(-pi)
    ltm = torch.log(th + mu + EPS)
    ptl = -pi + th * (torch.log(th + EPS) - ltm)
    zero = (x < EPS).float() * (F.softplus(ptl) - sp)
    pos = (x > EPS).float() * (-sp + ptl + x * (torch.log(mu + EPS) - ltm) + torch.lgamma(x + th) - torch.lgamma(th) - torch.lgamma(x + 1))
    return zero + pos


def _t_mix(x, mu1, mu2, th1, th2, pi):
    lse = torch.logsumexp(torch.stack((_t_nb(x, mu1, th1), _t_nb(x, mu2, th2) - pi)), dim=0)
    return lse - F.softplus(-pi)


def _t_sample(mu, th, zp=None):
    w = torch.distributions.Gamma(concentration=th.expand_as(mu), rate=th / mu).sample()
    k = torch.poisson(torch.clamp(w, max=1e8))
    if zp is not None:
        k[torch.rand_like(k) <= zp] = 0.0
    return k


def logp(out, repeats, n, only=False):
    d = {k: v.to(DEV) for k, v in _inputs(n).items()}
    calls = {"nb": dict(x=d["x"], mu=d["mu"], theta=d["theta"]),
             "zinb": dict(x=d["x"], mu=d["mu"], theta=d["theta"], pi=d["pi"]),
             "mixture": dict(x=d["x"], mu=d["mu"], theta=d["theta"], pi=d["pi"], mu2=d["mu2"], theta2=d["theta2"])}
    torch_fn = {"nb": lambda: _t_nb(d["x"], d["mu"], d["theta"]), "zinb": lambda: _t_zinb(d["x"], d["mu"], d["theta"], d["pi"]),
                "mixture": lambda: _t_mix(d["x"], d["mu"], d["mu2"], d["theta"], d["theta2"], d["pi"])}
    res = {}
    for kind, kw in calls.items():
        if only:
            for _ in range(3):
                N.count_logp(kind, return_terms=False, return_sums=True, **kw)
            continue
        r = {"terms_written": _with_peak(lambda: N.count_logp(kind, return_terms=True, return_sums=False, **kw), repeats),
             "sums_only": _with_peak(lambda: N.count_logp(kind, return_terms=False, return_sums=True, **kw), repeats),
             "torch_ops_float32": _with_peak(torch_fn[kind], max(3, repeats // 3))}
        r["elements_per_s_sums_only"] = n * D / (r["sums_only"]["ms"] * 1e-3)
        # a check of the tool, not a gate: the two agree to float32's error on the mean term
        dev = N.count_logp(kind, **kw)[0].double().mean()
        r["mean_term_device"], r["mean_term_torch_float32"] = float(dev), float(torch_fn[kind]().double().mean())
        res[kind] = r
    torch.cuda.synchronize()
    if not only:
        out["count_logp"] = res


def sample(out, repeats, n, batch, only=False):
    d = {k: v.to(DEV) for k, v in _inputs(n).items()}
    zp = torch.sigmoid(d["pi"])
    g = torch.Generator().manual_seed(SEED + 2)
    d10 = torch.relu(torch.randn(n, H, generator=g))
    L = ZR.spread_layers(d10[:512], D, g)
    for j in (2, 4):
        L[j], L[j + 1] = L[j] * 0.8, L[j + 1] * 0.8
    d10g, Lg = d10.to(DEV), [t.to(DEV) for t in L]
    if only:
        for _ in range(3):
            N.count_sample(d["mu"], d["theta"], zp, "probs", seed=1)
            N.zinb_sample(d10g, *Lg, seed=1)
        torch.cuda.synchronize()
        return
    s = {"count_sample_nb": _with_peak(lambda: N.count_sample(d["mu"], d["theta"], seed=1), repeats),
         "count_sample_zinb": _with_peak(lambda: N.count_sample(d["mu"], d["theta"], zp, "probs", seed=1), repeats),
         "zinb_sample_fused": _with_peak(lambda: N.zinb_sample(d10g, *Lg, seed=1), repeats),
         "torch_gamma_poisson_nb": _with_peak(lambda: _t_sample(d["mu"], d["theta"]), max(3, repeats // 3)),
         "torch_gamma_poisson_zinb": _with_peak(lambda: _t_sample(d["mu"], d["theta"], zp), max(3, repeats // 3))}
    # heads written, then drawn from: what the fused form avoids
    heads = lambda: N.count_sample(torch.relu(F.linear(d10g, Lg[0], Lg[1])), *N.zinb_heads(d10g, *Lg[2:]), heads_eps=1e-6, seed=1)   # noqa: E731
    s["heads_written_then_count_sample"] = _with_peak(heads, repeats)
    got = N.count_sample(d["mu"], d["theta"], zp, "probs", seed=1)
    s["mean_count_device"], s["mean_count_torch"] = float(got.double().mean()), float(_t_sample(d["mu"], d["theta"], zp).double().mean())
    s["mean_count_exact"] = float(((1 - zp.double()) * d["mu"].double()).mean())
    rows = 48
    r = CR.sample(d["mu"][:rows].cpu().numpy(), d["theta"].cpu().numpy(), zp[:rows].cpu().numpy(), "probs", seed=1)
    s["philox_calls_per_element_zinb"] = float(r["calls"].mean())
    s["philox_calls_per_element_nb"] = float(r["calls"].mean()) - 1.0
    s["philox_calls_counted_on_rows"] = rows
    assert np.array_equal(got[:rows].cpu().numpy()[r["margin"] >= 1e-9], r["draw"].astype(np.float32)[r["margin"] >= 1e-9])
    out["samplers_one_arm"] = s
    del d, zp, d10g, Lg, got
    torch.cuda.empty_cache()
    from distributed_vae_amd.cpl_mixvae import cpl_mixVAE
    from distributed_vae_amd.utils.dataloader import DeviceLoader
    torch.manual_seed(SEED)
    t = cpl_mixVAE(saving_folder="", device=0, save_flag=False)
    t.init_model(n_categories=92, state_dim=2, input_dim=D, fc_dim=H, lowD_dim=10, n_arm=2, temp=1.0, tau=0.005, mode="ZINB")
    data = ZR.counts_matrix(n, D, torch.Generator().manual_seed(SEED + 1)).to(DEV)
    dl = DeviceLoader(data, torch.arange(n), batch, False, False)
    t.sample_counts(dl, seed=1, arm=0)
    w = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        c = t.sample_counts(dl, seed=1, arm=0)
        w.append((time.perf_counter() - t0) * 1e3)
    m = t.model.eval()

    def on_device():
        for i, (x, _) in enumerate(dl):
            m.zinb_sample_batch(x.expand(2, -1, -1), 1, 1.0, cell0=i * batch, arms=[0])
    on_device()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    on_device()
    torch.cuda.synchronize()
    out["sample_counts"] = {"batch": batch, "batches": len(dl), "arm": 0, "end_to_end_wall_ms_median_of_3": sorted(w)[1],
                            "forwards_and_draws_on_the_device_wall_ms": (time.perf_counter() - t0) * 1e3,
                            "bytes_handed_to_the_host": int(c["counts"].nbytes), "mean_count": float(c["counts"].mean())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--only", choices=["logp", "sample"], default=None)
    ap.add_argument("--cells", type=int, default=NC)
    ap.add_argument("--batch", type=int, default=5000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "countdist_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("countdist_time needs a GPU")
    out = {"shape": {"N": a.cells, "D": D, "H": H}, "repeats": a.repeats, "device": torch.cuda.get_device_name(0)}
    if a.only == "logp":
        return logp(out, a.repeats, a.cells, only=True)
    if a.only == "sample":
        return sample(out, a.repeats, a.cells, a.batch, only=True)
    logp(out, a.repeats, a.cells)
    sample(out, a.repeats, a.cells, a.batch)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()

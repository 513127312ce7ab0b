"""GPU: the gradients of the ZINB term with respect to the decoder's three heads -- mmvae_zinb_head_grads,
mmvae_zinb_terms_grad (csrc/zinb_grad.hip) -- and what is built on them: nn_model.zinb_loss_grad,
mixVAE_model.zinb_head_grads, cpl_mixVAE.fit_zinb_heads; against tests/zinb_grad_restatement.py (pinned on the CPU by
tests/test_zinb_grad_cpu.py).  Nothing here reads the reference.

Error rule (DESIGN.md section 9m, section 9k's own): the statistic is |value - truth| / M, its maximum and 90th percentile.
Truth: float64 autograd of the restatement on the same float32 d10, weights and X.  Reference: float32 autograd of the same
restatement on the CPU in the same run.  The device must stay within max(3 x reference, 2^-23) in both figures, for the
elementwise gradients of zinb_terms_grad and for dW_j, db_j of every head; 2^-23 is the two float32 roundings of one product
(g, then the result).  M of an element of g is the sum of the magnitudes of the selected branch's addends times the chain
factor; of dW[d, h] the sum over the cells of M_g[i, d] |d10[i, h]|, of db[d] the sum of M_g[i, d].  Shapes: the eight of
section 9k's table, and N = 257 with the segment count forced to 1, 2 and 5.  Both figures are printed per case (pytest -s)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import zinb_grad_restatement as RG  # noqa: E402
import zinb_restatement as ZR  # noqa: E402
from gpu_util import DEV  # noqa: E402
from distributed_vae_amd import _native as N  # noqa: E402
from distributed_vae_amd import nn_model as NM  # noqa: E402

pytestmark = pytest.mark.gpu

MARGIN = 3.0
FLOOR = 2.0 ** -23
NAMES = {"rec": "fc11", "p": "fc11_p", "r": "fc11_r"}


def pitched(t, pad=3):
    """``t`` [n, w] on the device as rows of a wider matrix: row pitch w + pad, the pad filled with NaN."""
    buf = torch.full((t.shape[0], t.shape[1] + pad), float("nan"), dtype=t.dtype, device=DEV)
    buf[:, :t.shape[1]] = t.to(DEV)
    return buf[:, :t.shape[1]]


@functools.lru_cache(maxsize=None)
def case(n, D, H):
    """One shape's inputs and everything the CPU computes from them, once."""
    d10, L, X = RG.inputs(n, D, H)
    sc = 1.0 / (n * D)
    L64 = [t.double() for t in L]
    h32 = ZR.heads(d10, *L)
    c = {"d10": d10, "L": L, "X": X, "scale": sc, "h32": h32,
         "truth": RG.autograd_heads(d10.double(), L64, X.double(), scale=sc), "ref": RG.autograd_heads(d10, L, X, scale=sc),
         "M": RG.head_magnitudes(d10, L, X, scale=sc),
         # given heads: the truth is the float64 gradient at the SAME float32 heads
         "g_truth": RG.autograd_given(*(t.double() for t in h32), X.double()), "g_ref": RG.autograd_given(*h32, X),
         "g_M": RG.magnitudes_given(*h32, X)}
    for h in RG.HEADS:
        assert all(bool(torch.isfinite(t).all()) for t in c["truth"][h] + c["ref"][h])
    return c


def within(name, dev, cpu):
    print(f"    {name:<10} device max {dev[0]:.3e} p90 {dev[1]:.3e} | reference float32 max {cpu[0]:.3e} p90 {cpu[1]:.3e}")
    return dev[0] <= max(MARGIN * cpu[0], FLOOR) and dev[1] <= max(MARGIN * cpu[1], FLOOR)


def head_grads(c, **kw):
    return N.zinb_head_grads(pitched(c["d10"]), *(t.to(DEV) for t in c["L"]), pitched(c["X"]), **kw)


# ---- 1. the error gate ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,D,H,segments", [s + (0,) for s in RG.SHAPES] + [(257, 130, 128, 1), (257, 130, 128, 2), (257, 130, 128, 5),
                                                                           (257, 31, 100, 2), (257, 31, 100, 5)])
def test_head_grads_error_gate(n, D, H, segments):
    c = case(n, D, H)
    used = N.zinb_head_grads_segments(n, D, segments)
    print(f"\n  N = {n}, D = {D}, H = {H}, segments asked {segments}, used {used}")
    assert used == (min(segments, -(-n // 64)) if segments else -(-n // 64))      # at these sizes the rule is a segment per cell tile
    g, cell, gene = head_grads(c, segments=segments)
    ok = True
    for h in RG.HEADS:
        dW, db = g[h]
        assert dW.shape == (D, H) and db.shape == (D,) and dW.dtype == db.dtype == torch.float32
        for k, (nm, got) in enumerate((("dW", dW), ("db", db))):
            truth, ref, M = c["truth"][h][k], c["ref"][h][k], c["M"][h][k]
            ok &= within(f"{nm} {h}", ZR.error_stat(got.cpu(), truth, M), ZR.error_stat(ref, truth, M))
    assert ok
    # the sums beside the gradients are mmvae_zinb_nll's, bit for bit
    cell2, gene2 = N.zinb_nll(pitched(c["d10"]), *(t.to(DEV) for t in c["L"]), pitched(c["X"]))
    assert torch.equal(cell, cell2) and torch.equal(gene, gene2)


@pytest.mark.parametrize("n,D,H", RG.SHAPES)
def test_terms_grad_error_gate(n, D, H):
    c = case(n, D, H)
    print(f"\n  N = {n}, D = {D}, H = {H}")
    got = N.zinb_terms_grad(*(pitched(h) for h in c["h32"]), pitched(c["X"]))
    ok = True
    for j, h in enumerate(RG.HEADS):
        assert got[j].shape == (n, D) and got[j].dtype == torch.float32
        truth, ref, M = c["g_truth"][j], c["g_ref"][j], c["g_M"][j]
        ok &= within(f"g {h}", ZR.error_stat(got[j].cpu(), truth, M), ZR.error_stat(ref, truth, M))
    assert ok
    # zinb_loss_grad: the same kernel scaled by 1 / numel; a 3-D input is flattened over its leading dimensions
    lg = NM.zinb_loss_grad(*(h.to(DEV) for h in c["h32"]), c["X"].to(DEV))
    want = N.zinb_terms_grad(*(h.to(DEV) for h in c["h32"]), c["X"].to(DEV), scale=1.0 / (n * D))
    lg3 = NM.zinb_loss_grad(*(h.to(DEV)[None] for h in c["h32"]), c["X"].to(DEV)[None])
    for a, b, b3 in zip(lg, want, lg3):
        assert a.shape == (n, D) and torch.equal(a, b) and b3.shape == (1, n, D) and torch.equal(b3[0], a)


# ---- 2. lane maps -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,D,H", [(65, 33, 7), (63, 31, 1), (257, 130, 100)])
def test_lane_maps_exact_products(n, D, H):
    """Operands on which every product and sum of both matrix runs is exact.  d10 holds small integers; fc11 is W = 0, b = -1
    (a dead relu everywhere: dW_rec = 0, r = eps) and both gates are W = 0, b = 0; eps = 0.  Then p = q = z = y = 1/2 and
    r = 0, so for X > 0 d term / d z = 1 / y = 2 times the slope 1/4, and for X <= 0 it is expm1(0) / u = 0:
    g_r = [X > 0] / 2 exactly, a random 0 / 1 pattern.  dW_r = g_r^T d10 and db_r are sums of halves of small integers."""
    g = torch.Generator().manual_seed(n + D + H)
    d10 = torch.randint(0, 4, (n, H), generator=g).float()
    X = ZR.counts_matrix(n, D, g)
    zW, zb = torch.zeros(D, H), torch.zeros(D)
    out, _, _ = N.zinb_head_grads(pitched(d10), zW.to(DEV), (zb - 1).to(DEV), zW.to(DEV), zb.to(DEV), zW.to(DEV), zb.to(DEV), pitched(X),
                                  eps=0.0, scale=1.0, segments=2 if n > 128 else 0)
    pat = 0.5 * (X > 0).double()
    assert torch.equal(out["r"][0].cpu().double(), pat.T @ d10.double())
    assert torch.equal(out["r"][1].cpu().double(), pat.sum(0))
    assert not bool(out["rec"][0].any()) and not bool(out["rec"][1].any())
    assert 0.1 < float(pat.mean()) < 0.4


@pytest.mark.parametrize("n,D,H", [(65, 33, 7), (63, 31, 1), (257, 130, 100)])
def test_lane_maps_exact_products_p_head(n, D, H):
    """The p head on a pattern of its own, exact too.  X = 0 everywhere (the zero branch), eps = 0, fc11_p is W = 0, b = 0
    (p = q = 1/2, slope 1/4) and fc11_r is W = 0, b = -200, so that z = 1.4e-87 and y = 1 in fp64.  fc11 has small integer
    weights in its first four columns and an integer bias: r = relu(a_rec) is an integer up to 14, exact in any order.  Then
    w = q^r >= 2^-14 swallows z (u = w), q u = w / 2 and y r w = r w exactly up to one fp64 rounding, and
    d term / d p = y r w / (q u) = 2 r within an fp64 ulp: g_p = r / 2 exactly once rounded to float32, an asymmetric
    pattern of halves of integers.  dW_p = g_p^T d10 and db_p are exact sums, far from the r head's pattern [X > 0] / 2 and
    from g_rec = log 2 [a_rec > 0], so a swap of two heads' images, or of their outputs, cannot pass."""
    g = torch.Generator().manual_seed(2 * n + D + H)
    d10 = torch.randint(0, 4, (n, H), generator=g).float()
    W = torch.zeros(D, H)
    W[:, :4] = torch.randint(-1, 2, (D, min(H, 4)), generator=g).float()
    b = torch.randint(-2, 3, (D,), generator=g).float()
    zW, zb = torch.zeros(D, H), torch.zeros(D)
    X = torch.zeros(n, D)
    out, _, _ = N.zinb_head_grads(pitched(d10), W.to(DEV), b.to(DEV), zW.to(DEV), zb.to(DEV), zW.to(DEV), (zb - 200).to(DEV), pitched(X),
                                  eps=0.0, scale=1.0, segments=2 if n > 128 else 0)
    r = torch.relu(d10.double() @ W.double().T + b.double())
    assert float(r.max()) <= 14 and float(r.max()) >= 2 and len(r.unique()) >= 3
    assert torch.equal(out["p"][0].cpu().double(), (r / 2).T @ d10.double())
    assert torch.equal(out["p"][1].cpu().double(), (r / 2).sum(0))
    # the other two heads are not this pattern: fc11's is log 2 where the relu is alive, fc11_r's vanishes with its slope
    want_rec = float(np.log(2.0)) * (r > 0).double()
    assert torch.allclose(out["rec"][1].cpu().double(), want_rec.sum(0), rtol=1e-6, atol=0)
    assert float(out["r"][0].abs().max()) < 1e-80 and float(out["r"][1].abs().max()) < 1e-80


def test_terms_grad_outside_the_heads_domain():
    """Given heads are not checked (include/mmvae.h): where X > 0 and x_rec + eps is not positive, psi's argument is outside
    its domain and g_rec is NaN -- at once, whatever the size of the argument, and without touching another element (the
    pole at exactly 0 is in tests/test_zinb_grad_cpu.py).  The other elements equal those of a call on well-formed heads bit for bit."""
    c = case(63, 31, 7)
    X = c["X"].clone()
    X[1] = np.log1p(3.0)                                         # row 1: every X > 0
    good = [h.clone() for h in c["h32"]]
    bad = [h.clone() for h in good]
    odd = [-1e-3, -0.5, -3.0, -1e9, -3e38, float("-inf"), float("nan"), float("inf")]
    bad[0][1, :len(odd)] = torch.tensor(odd)
    bad[0][0, :len(odd)] = torch.tensor(odd)                     # row 0: X = 0, the zero branch, where psi is not asked
    ref = N.zinb_terms_grad(*(pitched(h) for h in good), pitched(X))
    got = N.zinb_terms_grad(*(pitched(h) for h in bad), pitched(X))
    torch.cuda.synchronize()
    g_rec = got[0].cpu()
    assert bool(torch.isnan(g_rec[1, :7]).all())
    assert not bool(torch.isfinite(g_rec[1, 7]))                 # +inf: psi(inf) - psi(inf)
    keep = torch.ones(63, 31, dtype=torch.bool)
    keep[:2, :len(odd)] = False
    for a, b in zip(got, ref):
        assert torch.equal(a.cpu()[keep], b.cpu()[keep])


@pytest.mark.parametrize("n,D,H", [(65, 33, 7), (63, 31, 1), (257, 130, 100), (257, 130, 128)])
def test_lane_maps_one_cell_per_column(n, D, H):
    """Every head, with g of full precision: column h of d10 is non-zero in one cell only, i(h), where it is a power of two.
    Then dW_j[d, h] = fl32(g_j[i(h), d]) d10[i(h), h] with no sum to round, and with weights in multiples of 1/16 and biases of
    1/64 the pre-activations are exact in any order, so the restatement evaluates g at the kernel's own pre-activations.
    The kernel rounds its fp64 g once (0.5 ulp); its exp, log and psi may differ from torch's in their last bits: 1 ulp."""
    g = torch.Generator().manual_seed(3 * n + D + H)
    d10 = torch.zeros(n, H)
    cells = [(7 * h + 3) % n for h in range(H)]
    for h, i in enumerate(cells):
        d10[i, h] = 2.0 ** (h % 3 - 1)
    L = []
    for j in range(3):
        L += [torch.randint(-5, 6, (D, H), generator=g).float() / 16, torch.randint(-40, 41, (D,), generator=g).float() / 64]
    L[1] = L[1].abs() + 0.25                                    # fc11 alive in the cells without a column
    X = ZR.counts_matrix(n, D, g)
    a = RG.pre_activations(d10.double(), *(t.double() for t in L))
    assert all(torch.equal(t, s.double()) for t, s in zip(a, RG.pre_activations(d10, *L)))
    want = [t.float() for t in RG.analytic(*a, X.double())]
    out, _, _ = N.zinb_head_grads(pitched(d10), *(t.to(DEV) for t in L), pitched(X), scale=1.0, segments=2 if n > 128 else 0)
    for j, h in enumerate(RG.HEADS):
        w = torch.stack([want[j][i] * d10[i, hh] for hh, i in enumerate(cells)], dim=1)            # [D, H], exact products
        ulp = torch.from_numpy(np.spacing(w.abs().numpy())).double()
        err = (out[h][0].cpu().double() - w.double()).abs()
        assert bool((err <= ulp).all()), (h, float((err / ulp).max()))
        assert float(w.abs().max()) > 0


# ---- 3. determinism, the head mask -----------------------------------------------------------------------------------------
def test_runs_are_bit_identical_and_a_gene_stands_alone():
    c = case(257, 130, 128)
    d10, X, L = pitched(c["d10"]), pitched(c["X"]), [t.to(DEV) for t in c["L"]]
    first, cell, gene = N.zinb_head_grads(d10, *L, X, scale=c["scale"], segments=5)
    again, cell2, gene2 = N.zinb_head_grads(d10, *L, X, scale=c["scale"], segments=5)
    assert torch.equal(cell, cell2) and torch.equal(gene, gene2)
    for h in RG.HEADS:
        assert torch.equal(first[h][0], again[h][0]) and torch.equal(first[h][1], again[h][1])
    among65, _, _ = N.zinb_head_grads(d10, *(t[:65] for t in L), X[:, :65], scale=c["scale"], segments=5)
    for d in (0, 37, 64):        # (gene 64 alone sits in row 0 of its tile, among 65 and 130 in row 0 of the second tile)
        alone, _, _ = N.zinb_head_grads(d10, *(t[d:d + 1] for t in L), X[:, d:d + 1], scale=c["scale"], segments=5)
        for h in RG.HEADS:
            for k in (0, 1):
                assert torch.equal(alone[h][k][0], among65[h][k][d]) and torch.equal(alone[h][k][0], first[h][k][d]), (d, h, k)
    t1, t2 = (N.zinb_terms_grad(*(pitched(h) for h in c["h32"]), X) for _ in range(2))
    assert all(torch.equal(p, q) for p, q in zip(t1, t2))


def test_head_mask_leaves_the_other_heads_alone():
    c = case(257, 31, 100)
    d10, X, L = pitched(c["d10"]), pitched(c["X"]), [t.to(DEV) for t in c["L"]]
    D, H = 31, 100
    full, cell, _ = N.zinb_head_grads(d10, *L, X)
    poison = (torch.full((D, H), float("nan"), device=DEV), torch.full((D,), float("nan"), device=DEV))
    bits = [t.clone().view(torch.int32) for t in poison]
    out = {"rec": poison, "p": (torch.empty(D, H, device=DEV), torch.empty(D, device=DEV)),
           "r": (torch.empty(D, H, device=DEV), torch.empty(D, device=DEV))}
    got, cell2, _ = N.zinb_head_grads(d10, *L, X, heads=("p", "r"), out=out)
    assert sorted(got) == ["p", "r"] and torch.equal(cell, cell2)
    assert all(torch.equal(t.view(torch.int32), b) for t, b in zip(poison, bits))            # no fc11 output is written
    for h in ("p", "r"):
        assert got[h][0] is out[h][0] and torch.equal(got[h][0], full[h][0]) and torch.equal(got[h][1], full[h][1])
    only, _, _ = N.zinb_head_grads(d10, *L, X, heads=("rec",))
    assert sorted(only) == ["rec"] and torch.equal(only["rec"][0], full["rec"][0]) and torch.equal(only["rec"][1], full["rec"][1])


# ---- 4. descent on the kernel itself ----------------------------------------------------------------------------------------
def test_descent_on_the_restatements_inputs():
    """The inputs of tests/test_zinb_grad_cpu.py::test_descent_restatement_is_monotone: 20 steps of mmvae_zinb_head_grads and
    mmvae_adam_step at lr = 1e-2 from nn.Linear's default initialisation, one full batch.  Every step's loss is below the one
    before, and the losses follow the float64 restatement's."""
    d10, L, X = RG.descent_case()
    n, D, H = 257, 33, 7
    want = RG.adam_losses(d10, L, X, steps=20, lr=1e-2)
    assert np.all(np.diff(want) < 0)
    sizes = [t.numel() for t in L]
    buf = torch.cat([t.reshape(-1) for t in L]).to(DEV)
    grad, m1, m2 = torch.zeros_like(buf), torch.zeros_like(buf), torch.zeros_like(buf)
    views = lambda t: [v.view(s.shape) for v, s in zip(t.split(sizes), L)]
    P, Gv = views(buf), views(grad)
    out = {h: (Gv[2 * j], Gv[2 * j + 1]) for j, h in enumerate(RG.HEADS)}
    d10d, Xd = d10.to(DEV), X.to(DEV)
    losses = []
    for step in range(1, 21):
        _, cell, _ = N.zinb_head_grads(d10d, *P, Xd, out=out)
        losses.append(float(cell.sum()) / (n * D))
        N.adam_step(buf, grad, m1, m2, step, 1e-2)
    print(f"\n  loss {losses[0]:.6f} -> {losses[-1]:.6f}; restatement {want[0]:.6f} -> {want[-1]:.6f}")
    assert np.all(np.diff(losses) < 0), losses
    assert np.allclose(losses, want, rtol=1e-4, atol=0)


# ---- 5. fit_zinb_heads ------------------------------------------------------------------------------------------------------
A_, DM, HF, CC, SS, N_ALL, N_CELLS, BATCH = 2, 70, 20, 5, 2, 80, 60, 21


def trainer(seed=4, mode="ZINB"):
    from distributed_vae_amd.cpl_mixvae import cpl_mixVAE
    torch.manual_seed(seed)
    t = cpl_mixVAE(saving_folder="", device=0, save_flag=False)
    t.init_model(n_categories=CC, state_dim=SS, input_dim=DM, fc_dim=HF, lowD_dim=6, x_drop=0.5, s_drop=0.2, n_arm=A_, temp=1.0,
                 tau=0.005, mode=mode)
    return t


@functools.lru_cache(maxsize=None)
def cells():
    data = ZR.counts_matrix(N_ALL, DM, torch.Generator().manual_seed(8)).to(DEV)
    index = torch.from_numpy(np.random.default_rng(2).permutation(N_ALL)[:N_CELLS])
    u = torch.rand(A_, N_CELLS, SS, generator=torch.Generator().manual_seed(9)).to(DEV)
    return data, index, u


def loader(lo=0, hi=N_CELLS, batch=BATCH):
    from distributed_vae_amd.utils.dataloader import DeviceLoader
    data, index, _ = cells()
    return DeviceLoader(data, index[lo:hi], batch, False, False)


def noise(epochs=1, lo=0, hi=N_CELLS, batch=BATCH):
    u = cells()[2]
    return [{"u_state": u[:, i:min(i + batch, hi)].contiguous()} for _ in range(epochs) for i in range(lo, hi, batch)]


def head_bits(m):
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_fit_steps_are_torch_adam_on_the_device_gradient(wd):
    """Three steps, one batch each: before a step the model's own zinb_head_grads for that batch, torch.optim.Adam on the CPU
    applied to that gradient; after fit_zinb_heads' step the parameters agree within 2e-6, the tolerance of
    test_adam_kernel_matches_torch."""
    t = trainer()
    m = t.model
    data, index, _ = cells()
    ref = {}
    for a in range(A_):
        for h, name in NAMES.items():
            lin = getattr(m, name)[a]
            ref[(a, h, 0)], ref[(a, h, 1)] = (p.detach().cpu().clone().requires_grad_() for p in (lin.weight, lin.bias))
    opt = torch.optim.Adam(list(ref.values()), lr=1e-3, weight_decay=wd)
    state = None
    for b in range(3):
        lo, hi = b * BATCH, min((b + 1) * BATCH, N_CELLS)
        x = data[index[lo:hi].to(DEV)]
        m.eval()
        m.set_explicit_noise(noise(1, lo, hi))
        g = m.zinb_head_grads(x.expand(A_, -1, -1), t.temp)
        m.train()
        for a in range(A_):
            assert sorted(g[a]) == ["fc11", "fc11_p", "fc11_r", "loss"] and g[a]["loss"].dtype == torch.float64 and g[a]["loss"].dim() == 0
            for h, name in NAMES.items():
                ref[(a, h, 0)].grad, ref[(a, h, 1)].grad = g[a][name][0].cpu().clone(), g[a][name][1].cpu().clone()
        opt.step()
        m.set_explicit_noise(noise(1, lo, hi))
        res = t.fit_zinb_heads(loader(lo, hi), 1, lr=1e-3, weight_decay=wd, state=state)
        state = res["state"]
        assert state["step"] == b + 1 and m.training
        assert res["train_loss"].shape == (1, A_) and res["val_loss"] is None
        assert np.allclose(res["train_loss"][0], [float(g[a]["loss"]) for a in range(A_)], rtol=1e-12)
        worst = 0.0
        for a in range(A_):
            for h, name in NAMES.items():
                lin = getattr(m, name)[a]
                worst = max(worst, float((lin.weight.detach().cpu() - ref[(a, h, 0)].detach()).abs().max()),
                            float((lin.bias.detach().cpu() - ref[(a, h, 1)].detach()).abs().max()))
        print(f"\n  step {b + 1}, weight_decay {wd}: largest difference from torch's Adam {worst:.3e}")
        assert worst < 2e-6
    m.set_explicit_noise(None)


@pytest.mark.parametrize("heads", [("p", "r"), ("rec",), ("rec", "p", "r")])
def test_fit_leaves_everything_else_alone(heads):
    t = trainer()
    m = t.model
    m.flat_parameters()
    before, flat, bn = head_bits(m), m.flat_parameters().clone(), m._bn_flat.clone()
    m.set_explicit_noise((noise(1) + noise(1, batch=64)) * 2)            # an epoch's three batches, then score_zinb's one
    res = t.fit_zinb_heads(loader(), 2, lr=1e-2, heads=heads, test_loader=loader(batch=64))
    m.set_explicit_noise(None)
    assert m.training                                                   # the mode is restored
    assert res["train_loss"].shape == res["val_loss"].shape == (2, A_) and res["state"]["step"] == 6
    assert np.all(np.isfinite(res["train_loss"])) and np.all(np.isfinite(res["val_loss"]))
    after = head_bits(m)
    chosen = tuple(NAMES[h] + "." for h in heads)
    for k in before:
        if k.startswith(chosen):
            assert not torch.equal(before[k], after[k]), k
        else:
            assert torch.equal(before[k], after[k]), k
    assert torch.equal(bn, m._bn_flat)
    if "rec" not in heads:
        assert torch.equal(flat, m.flat_parameters())
    # val_loss is score_zinb of the fitted model
    m.set_explicit_noise(noise(1, batch=64))
    assert np.array_equal(res["val_loss"][1], t.score_zinb(loader(batch=64))["mean"])
    m.set_explicit_noise(None)
    m.eval()
    t.fit_zinb_heads(loader(0, BATCH), 0)
    assert not m.training                                               # eval stays eval
    m.set_explicit_noise([])                                            # an exhausted schedule: the forward raises
    m.train()
    with pytest.raises(RuntimeError, match="exhausted"):
        t.fit_zinb_heads(loader(0, BATCH), 1)
    assert m.training                                                   # restored after an exception too
    m.set_explicit_noise(None)


def test_fit_descends_on_counts_drawn_from_known_heads():
    """Counts drawn with numpy from known heads on the model's own d10 (Gamma-Poisson, zero inflation), X = log1p; the heads at
    nn.Linear's default initialisation, one full batch, lr = 1e-2, 20 steps: every step's loss is below the one before.  The
    float64 restatement of the same fit on the device's d10 of that X is checked first."""
    from distributed_vae_amd.utils.dataloader import DeviceLoader
    t = trainer(seed=6)
    m = t.model.eval()
    data, index, u = cells()
    x0 = data[index.to(DEV)]
    m.set_explicit_noise({"u_state": u})
    m(x0.expand(A_, -1, -1), t.temp, eval=True)
    d10 = m._engine.ws_view("d10", HF)[0].cpu()
    X = RG.draw_counts(d10, np.random.default_rng(5), DM)
    assert 0.3 < float((X == 0).double().mean()) < 0.95
    m(X.to(DEV).expand(A_, -1, -1), t.temp, eval=True)
    d10x = m._engine.ws_view("d10", HF).cpu()
    for a in range(A_):
        want = RG.adam_losses(d10x[a], [p.cpu() for p in m._zinb_layers(a)], X, steps=20, lr=1e-2)
        assert np.all(np.diff(want) < -1e-5), want
    m.train()
    res = t.fit_zinb_heads(DeviceLoader(X.to(DEV), torch.arange(N_CELLS), N_CELLS, False, False), 20, lr=1e-2)
    m.set_explicit_noise(None)
    loss = res["train_loss"]
    print(f"\n  loss per arm {loss[0]} -> {loss[-1]}")
    assert loss.shape == (20, A_) and np.all(np.diff(loss, axis=0) < 0), loss


def test_fit_resumes_bit_for_bit_and_round_trips():
    t4, t22 = trainer(), trainer()
    t22.model.load_state_dict(head_bits(t4.model))
    t4.model.set_explicit_noise(noise(4))
    r4 = t4.fit_zinb_heads(loader(), 4, lr=1e-2)
    t22.model.set_explicit_noise(noise(4))
    r2 = t22.fit_zinb_heads(loader(), 2, lr=1e-2)
    r22 = t22.fit_zinb_heads(loader(), 2, lr=1e-2, state=r2["state"])
    assert r2["state"]["step"] == 6 and r22["state"]["step"] == r4["state"]["step"] == 12
    assert np.array_equal(np.concatenate([r2["train_loss"], r22["train_loss"]]), r4["train_loss"])
    for k in ("exp_avg", "exp_avg_sq"):
        assert torch.equal(r22["state"][k], r4["state"][k])
    sd4, sd22 = head_bits(t4.model), head_bits(t22.model)
    assert all(torch.equal(sd4[k], sd22[k]) for k in sd4)
    with pytest.raises(ValueError, match="state"):
        t22.fit_zinb_heads(loader(), 1, heads=("p",), state=r2["state"])
    # a state_dict saved after the fit, loaded into a fresh ZINB model, scores the same bits
    fresh = trainer(seed=99)
    assert not torch.equal(fresh.model.fc11_p[0].weight, t4.model.fc11_p[0].weight)
    fresh.model.load_state_dict({k: v.cpu() for k, v in sd4.items()})
    scores = []
    for t in (t4, fresh):
        t.model.set_explicit_noise(noise(1))
        scores.append(t.score_zinb(loader()))
        t.model.set_explicit_noise(None)
    assert np.array_equal(scores[0]["cell"], scores[1]["cell"]) and np.array_equal(scores[0]["gene"], scores[1]["gene"])


def test_fit_refusals(monkeypatch):
    from distributed_vae_amd import dist as DD
    t = trainer()
    with pytest.raises(ValueError, match="heads"):
        t.fit_zinb_heads(loader(), 1, heads=("rec", "pi"))
    with pytest.raises(RuntimeError, match="loss_mode='ZINB'"):
        trainer(mode="MSE").fit_zinb_heads(loader(), 1)
    with pytest.raises(RuntimeError, match="eval"):
        t.model.train().zinb_head_grads(torch.zeros(A_, 4, DM, device=DEV))
    monkeypatch.setattr(DD, "is_dist", lambda: True)
    with pytest.raises(NotImplementedError, match="not data-parallel"):
        t.fit_zinb_heads(loader(), 1)


def test_the_pinned_refusals_still_hold():
    """What stays refused beside the new names: zinb_loss has no backward, the fused step does not train a ZINB model."""
    t = trainer()
    h = torch.rand(4, DM, device=DEV)
    with pytest.raises(NotImplementedError, match="no backward"):
        NM.zinb_loss(h.clone().requires_grad_(), h, h, h)
    with pytest.raises(NotImplementedError, match="training under loss_mode='ZINB' is not built"):
        t.model.fused_train_step(h.expand(A_, -1, -1), 1.0, None, do_adam=False)
    with pytest.raises(NotImplementedError, match="training under loss_mode='ZINB' is not built"):
        t._step(h.expand(A_, -1, -1))

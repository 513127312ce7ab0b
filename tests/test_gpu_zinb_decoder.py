"""GPU: the gradient of the ZINB term below the heads -- mmvae_zinb_d10_grad (csrc/zinb_grad.hip), mmvae_decoder_trunk_grads
(csrc/zinb_trunk.hip) -- and what is built on them: mixVAE_model.zinb_decoder_grads, cpl_mixVAE.fit_zinb_decoder; against
tests/zinb_decoder_restatement.py (pinned on the CPU by tests/test_zinb_decoder_cpu.py).  Nothing here reads the reference.

Error rule (DESIGN.md sections 9k, 9m, 9n): the statistic is |value - truth| / M, its maximum and 90th percentile.  Truth:
float64 on the same float32 inputs (autograd of the restatement for gd10; the backward's formulas at the given activations
for the trunk, which tests/test_zinb_decoder_cpu.py holds to float64 autograd).  Reference: float32 autograd on the CPU in
the same run.  The device must stay within max(3 x reference, 2^-23) in both figures.  Both are printed per case (pytest -s)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import zinb_decoder_restatement as RD  # noqa: E402
import zinb_grad_restatement as RG  # noqa: E402
import zinb_restatement as ZR  # noqa: E402
from gpu_util import DEV  # noqa: E402
from distributed_vae_amd import _native as N  # noqa: E402
from distributed_vae_amd import nn_model as NM  # noqa: E402

pytestmark = pytest.mark.gpu

MARGIN = 3.0
FLOOR = 2.0 ** -23
NAMES = {"rec": "fc11", "p": "fc11_p", "r": "fc11_r"}
BIG = (65, 257, 100)              # five gene tiles: the shape whose segments are forced


def pitched(t, pad=3):
    """``t`` [n, w] on the device as rows of a wider matrix: row pitch w + pad, the pad filled with NaN."""
    buf = torch.full((t.shape[0], t.shape[1] + pad), float("nan"), dtype=t.dtype, device=DEV)
    buf[:, :t.shape[1]] = t.to(DEV)
    return buf[:, :t.shape[1]]


def within(name, dev, cpu):
    print(f"    {name:<10} device max {dev[0]:.3e} p90 {dev[1]:.3e} | reference float32 max {cpu[0]:.3e} p90 {cpu[1]:.3e}")
    return dev[0] <= max(MARGIN * cpu[0], FLOOR) and dev[1] <= max(MARGIN * cpu[1], FLOOR)


@functools.lru_cache(maxsize=None)
def case(n, D, H, heads=RD.HEADS):
    """One shape's inputs and everything the CPU computes from them, once."""
    d10, L, X = RG.inputs(n, D, H)
    sc = 1.0 / (n * D)
    return {"d10": d10, "L": L, "X": X, "scale": sc,
            "truth": RD.gd10_autograd(d10.double(), [t.double() for t in L], X.double(), heads, sc),
            "ref": RD.gd10_autograd(d10, L, X, heads, sc), "M": RD.gd10_magnitudes(d10, L, X, heads, sc)}


def d10_grad(c, **kw):
    return N.zinb_d10_grad(pitched(c["d10"]), *(t.to(DEV) for t in c["L"]), pitched(c["X"]), **kw)


# ---- 1. the error gate ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,D,H,segments", [s + (0,) for s in RG.SHAPES] + [BIG + (s,) for s in (0, 1, 2, 5)])
def test_gd10_error_gate(n, D, H, segments):
    c = case(n, D, H)
    used = N.zinb_d10_grad_segments(n, D, segments)
    print(f"\n  N = {n}, D = {D}, H = {H}, segments asked {segments}, used {used}")
    assert used == (min(segments, -(-D // 64)) if segments else -(-D // 64))       # at these sizes the rule is a segment per gene tile
    got = d10_grad(c, segments=segments, out=pitched(torch.zeros(n, H)))
    assert got.shape == (n, H) and got.dtype == torch.float32
    assert within("gd10", ZR.error_stat(got.cpu(), c["truth"], c["M"]), ZR.error_stat(c["ref"], c["truth"], c["M"]))


@pytest.mark.parametrize("heads", RD.MASKS)
def test_gd10_error_gate_every_head_mask(heads):
    c = case(*BIG, heads=heads)
    print(f"\n  N, D, H = {BIG}, heads {heads}")
    got = d10_grad(c, heads=heads, segments=2)
    assert within("gd10", ZR.error_stat(got.cpu(), c["truth"], c["M"]), ZR.error_stat(c["ref"], c["truth"], c["M"]))


@functools.lru_cache(maxsize=None)
def trunk_case(n, Z, Lw, H):
    acts, params, gd10 = RD.trunk_inputs(n, Z, Lw, H)
    truth, truth_z = RD.trunk_backward([t.double() for t in acts], [t.double() for t in params], gd10.double())
    ref, ref_z, racts = RD.trunk_autograd(acts[0], params, gd10)
    assert all(torch.equal(a, b) for a, b in zip(acts, racts))
    M, Mz = RD.trunk_magnitudes(acts, params, gd10)
    return {"acts": acts, "params": params, "gd10": gd10, "truth": truth + [truth_z], "ref": ref + [ref_z], "M": M + [Mz]}


def trunk_grads(c, **kw):
    g, gz = N.decoder_trunk_grads([pitched(a) for a in c["acts"]], [p.to(DEV) for p in c["params"]], pitched(c["gd10"]), **kw)
    return g + [gz]


@pytest.mark.parametrize("n,Z,Lw,H,segments", [s + (0,) for s in RD.TRUNK_SHAPES] + [(257, 13, 10, 128, 2), (257, 13, 10, 128, 5)])
def test_trunk_grads_error_gate(n, Z, Lw, H, segments):
    c = trunk_case(n, Z, Lw, H)
    print(f"\n  N = {n}, C + S = {Z}, L = {Lw}, H = {H}, segments asked {segments}, used {N.decoder_trunk_grads_segments(n, segments)}")
    got = trunk_grads(c, segments=segments)
    names = [f"{RD.TRUNK[k // 2]}.{'b' if k % 2 else 'W'}" for k in range(10)] + ["gzin"]
    ok = True
    for k, nm in enumerate(names):
        assert got[k].shape == c["truth"][k].shape and got[k].dtype == torch.float32
        ok &= within(nm, ZR.error_stat(got[k].cpu(), c["truth"][k], c["M"][k]), ZR.error_stat(c["ref"][k], c["truth"][k], c["M"][k]))
    assert ok
    # gzin is optional, and the ten gradients do not depend on it; out= receives them
    flat = torch.zeros(sum(t.numel() for t in c["params"]), device=DEV)
    views = [v.view(p.shape) for v, p in zip(flat.split([t.numel() for t in c["params"]]), c["params"])]
    g2, none = N.decoder_trunk_grads([a.to(DEV) for a in c["acts"]], [p.to(DEV) for p in c["params"]], c["gd10"].to(DEV),
                                     segments=segments, out=views, want_gzin=False)
    assert none is None and all(a is b for a, b in zip(g2, views)) and all(torch.equal(a, b) for a, b in zip(g2, got[:10]))


# ---- 2. lane maps, exact ----------------------------------------------------------------------------------------------------
LANE_SHAPES = [(65, 33, 7), (63, 31, 1), (257, 130, 100), (257, 130, 128)]


def _noise_layer(D, H, g):
    return torch.randn(D, H, generator=g)


@pytest.mark.parametrize("n,D,H", LANE_SHAPES)
def test_lane_maps_exact_products_r_head(n, D, H):
    """d10 = 0: every pre-activation is its bias whatever W holds; eps = 0.  fc11's bias is -1 (a dead relu: r = 0), both gates'
    biases are 0 (p = q = z = y = 1/2, slope 1/4): for X > 0 d term / d z = 1 / y = 2, for X <= 0 it is expm1(0) / u = 0, so
    g_r = [X > 0] / 2 exactly, and with small-integer Wr every product and sum of the second matrix run is exact:
    gd10[i, h] = sum_d [X[i, d] > 0] / 2 Wr[d, h]."""
    g = torch.Generator().manual_seed(n + D + H)
    X = ZR.counts_matrix(n, D, g)
    Wr = torch.randint(-3, 4, (D, H), generator=g).float()
    zb = torch.zeros(D)
    got = N.zinb_d10_grad(pitched(torch.zeros(n, H)), _noise_layer(D, H, g).to(DEV), (zb - 1).to(DEV), _noise_layer(D, H, g).to(DEV),
                          zb.to(DEV), Wr.to(DEV), zb.to(DEV), pitched(X), eps=0.0, scale=1.0, heads=("r",), segments=2 if D > 64 else 0)
    pat = 0.5 * (X > 0).double()
    assert torch.equal(got.cpu().double(), pat @ Wr.double())
    assert 0.1 < float(pat.mean()) < 0.4 and bool(got.any())


@pytest.mark.parametrize("n,D,H", LANE_SHAPES)
def test_lane_maps_exact_products_p_head(n, D, H):
    """d10 = 0, eps = 0, X = 0 everywhere (the zero branch), b_p = 0 (p = q = 1/2, slope 1/4), b_r = -200 (z = 1.4e-87, y = 1 in
    fp64) and a small integer b_rec: r = relu(b_rec), w = q^r swallows z, d term / d p = y r w / (q u) = 2 r within an fp64 ulp,
    g_p = r / 2 exactly once rounded: gd10[i, h] = sum_d relu(b_rec[d]) / 2 Wp[d, h] with small-integer Wp, an exact sum."""
    g = torch.Generator().manual_seed(2 * n + D + H)
    b = torch.randint(-2, 7, (D,), generator=g).float()
    Wp = torch.randint(-3, 4, (D, H), generator=g).float()
    zb = torch.zeros(D)
    got = N.zinb_d10_grad(pitched(torch.zeros(n, H)), _noise_layer(D, H, g).to(DEV), b.to(DEV), Wp.to(DEV), zb.to(DEV),
                          _noise_layer(D, H, g).to(DEV), (zb - 200).to(DEV), pitched(torch.zeros(n, D)), eps=0.0, scale=1.0, heads=("p",),
                          segments=2 if D > 64 else 0)
    want = (torch.relu(b.double()) / 2) @ Wp.double()
    assert torch.equal(got.cpu().double(), want.expand(n, H)) and len(torch.relu(b).unique()) >= 3


@pytest.mark.parametrize("n,D,H", LANE_SHAPES)
def test_lane_maps_one_weight_per_column(n, D, H):
    """Every head, with g of full precision: d10 = 0 and eps = 0 as above, random biases and X, and the selected head's W has one
    non-zero entry per column h, a power of two at gene d(h): gd10[i, h] = fl32(g_j[i, d(h)]) W_j[d(h), h] with no sum to round.
    The kernel rounds its fp64 g once (0.5 ulp); its exp, log and psi may differ from torch's in their last bits: 1 ulp."""
    g = torch.Generator().manual_seed(3 * n + D + H)
    genes = [(7 * h + 3) % D for h in range(H)]
    L = []
    for j in range(3):
        L += [_noise_layer(D, H, g), torch.randint(-40, 41, (D,), generator=g).float() / 64]
    L[1] = L[1].abs() + 0.25                                    # fc11 alive
    X = ZR.counts_matrix(n, D, g)
    a = [L[2 * j + 1].double().expand(n, D) for j in range(3)]
    want = [t.float() for t in RG.analytic(*a, X.double(), eps=0.0)]
    for j, h in enumerate(RG.HEADS):
        Lj = list(L)
        Lj[2 * j] = torch.zeros(D, H)
        for hh, d in enumerate(genes):
            Lj[2 * j][d, hh] = 2.0 ** (hh % 3 - 1)
        got = N.zinb_d10_grad(pitched(torch.zeros(n, H)), *(t.to(DEV) for t in Lj), pitched(X), eps=0.0, scale=1.0, heads=(h,),
                              segments=2 if D > 64 else 0)
        w = torch.stack([want[j][:, d] * Lj[2 * j][d, hh] for hh, d in enumerate(genes)], dim=1)          # [n, H], exact products
        ulp = torch.from_numpy(np.spacing(w.abs().numpy())).double()
        err = (got.cpu().double() - w.double()).abs()
        assert bool((err <= ulp).all()), (h, float((err / ulp).max()))
        assert float(w.abs().max()) > 0


# ---- 3. determinism, independence, the head mask ----------------------------------------------------------------------------
def test_runs_are_bit_identical_and_a_cell_stands_alone():
    c = case(257, 130, 128)
    d10, X, L = pitched(c["d10"]), pitched(c["X"]), [t.to(DEV) for t in c["L"]]
    first = N.zinb_d10_grad(d10, *L, X, scale=c["scale"], segments=2)
    again = N.zinb_d10_grad(d10, *L, X, scale=c["scale"], segments=2)
    assert torch.equal(first, again)
    among65 = N.zinb_d10_grad(d10[:65], *L, X[:65], scale=c["scale"], segments=2)
    for i in (0, 37, 64):       # (cell 64 alone sits in row 0 of its tile, among 65 and 257 in row 0 of the second tile)
        alone = N.zinb_d10_grad(d10[i:i + 1], *L, X[i:i + 1], scale=c["scale"], segments=2)
        assert torch.equal(alone[0], among65[i]) and torch.equal(alone[0], first[i]), i
    tc = trunk_case(257, 13, 10, 128)
    t1, t2 = trunk_grads(tc, segments=5), trunk_grads(tc, segments=5)
    assert all(torch.equal(p, q) for p, q in zip(t1, t2))


def test_an_unselected_head_has_no_path_of_its_own():
    """An unselected head's weights enter the pre-activations only.  Where X > 0 the selected branch of the table makes g_rec and
    g_p functions of (a_rec, a_p) alone and g_r a function of a_r alone, so on a matrix of positive X an unselected head may be
    NaN throughout without a bit of the result moving; in the zero branch every g depends on all three pre-activations, and
    no such statement holds (nor does autograd make it)."""
    c = case(65, 130, 100)
    d10, L = pitched(c["d10"]), [t.to(DEV) for t in c["L"]]
    X = pitched(c["X"].clamp_min(float(np.log1p(1.0))))
    nan = [torch.full_like(t, float("nan")) for t in L]
    for heads, poisoned in ((("rec", "p"), L[:4] + nan[4:]), (("r",), nan[:4] + L[4:]), (("rec",), L[:4] + nan[4:])):
        clean = N.zinb_d10_grad(d10, *L, X, heads=heads, segments=2)
        got = N.zinb_d10_grad(d10, *poisoned, X, heads=heads, segments=2)
        assert bool(torch.isfinite(clean).all()) and bool(clean.any()) and torch.equal(clean, got), heads


# ---- 4. zinb_decoder_grads and fit_zinb_decoder -----------------------------------------------------------------------------
A_, DM, HF, CC, SS, LD, N_ALL, N_CELLS, BATCH = 2, 70, 20, 5, 2, 6, 80, 60, 21
DESCENT = dict(steps=20, lr=2e-3)


def trainer(seed=4, mode="ZINB"):
    from distributed_vae_amd.cpl_mixvae import cpl_mixVAE
    torch.manual_seed(seed)
    t = cpl_mixVAE(saving_folder="", device=0, save_flag=False)
    t.init_model(n_categories=CC, state_dim=SS, input_dim=DM, fc_dim=HF, lowD_dim=LD, x_drop=0.5, s_drop=0.2, n_arm=A_, temp=1.0,
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


def bits(m):
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def decoder_names(heads=RD.HEADS):
    return tuple(nm + "." for nm in RD.TRUNK) + tuple(NAMES[h] + "." for h in heads)


def test_decoder_grads_are_the_restatements():
    """mixVAE_model.zinb_decoder_grads on a batch against float64 autograd of the whole decoder from the device's own zin: the
    three launches compose to the gradient of the mean term (loose bound: the device's activations are float32; the gates above
    are the precision tests)."""
    t = trainer()
    m = t.model.eval()
    data, index, u = cells()
    x = data[index.to(DEV)]
    m.set_explicit_noise({"u_state": u})
    res = m.zinb_decoder_grads(x.expand(A_, -1, -1), t.temp)
    zin = m._engine.ws_view("zin", CC + SS).cpu()
    m.set_explicit_noise(None)
    for a in range(A_):
        assert sorted(res[a]) == sorted(["loss", "d10", "c", "s", "fc11", "fc11_p", "fc11_r"] + list(RD.TRUNK))
        params = [p.detach().cpu() for nm in RD.TRUNK for p in (getattr(m, nm)[a].weight, getattr(m, nm)[a].bias)]
        L = [p.cpu() for p in m._zinb_layers(a)]
        full = RD.decoder_autograd(zin[a].double(), [p.double() for p in params], [p.double() for p in L], x.cpu().double(), 1.0 / x.numel())
        assert res[a]["c"].shape == (N_CELLS, CC) and res[a]["s"].shape == (N_CELLS, SS) and res[a]["d10"].shape == (N_CELLS, HF)
        pairs = [(res[a][nm][k], full["trunk"][2 * i + k]) for i, nm in enumerate(RD.TRUNK) for k in (0, 1)]
        pairs += [(res[a][NAMES[h]][k], full["heads"][2 * j + k]) for j, h in enumerate(RD.HEADS) for k in (0, 1)]
        pairs += [(res[a]["d10"], full["d10"]), (torch.cat([res[a]["c"], res[a]["s"]], 1), full["zin"])]
        for got, want in pairs:
            assert got.shape == want.shape
            assert float((got.cpu().double() - want).abs().max()) <= 1e-4 * float(want.abs().max()) + 1e-12
    # heads=: the unselected heads are left out of the result and of gd10
    m.set_explicit_noise({"u_state": u})
    only = m.zinb_decoder_grads(x.expand(A_, -1, -1), t.temp, heads=("p",))
    m.set_explicit_noise(None)
    assert "fc11" not in only[0] and "fc11_r" not in only[0] and not torch.equal(only[0]["d10"], res[0]["d10"])
    assert torch.equal(only[0]["fc11_p"][0], res[0]["fc11_p"][0])


@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_fit_steps_are_torch_adam_on_the_device_gradient(wd):
    """Three steps, one batch each: before a step the model's own zinb_decoder_grads for that batch, torch.optim.Adam on the CPU
    applied to that gradient; after fit_zinb_decoder's step trunk and heads agree within 2e-6 (section 9m's tolerance)."""
    t = trainer()
    m = t.model
    data, index, _ = cells()
    layers = list(RD.TRUNK) + list(NAMES.values())
    ref = {}
    for a in range(A_):
        for name in layers:
            lin = getattr(m, name)[a]
            ref[(a, name, 0)], ref[(a, name, 1)] = (p.detach().cpu().clone().requires_grad_() for p in (lin.weight, lin.bias))
    opt = torch.optim.Adam(list(ref.values()), lr=1e-3, weight_decay=wd)
    state = None
    for b in range(3):
        lo, hi = b * BATCH, min((b + 1) * BATCH, N_CELLS)
        x = data[index[lo:hi].to(DEV)]
        m.eval()
        m.set_explicit_noise(noise(1, lo, hi))
        g = m.zinb_decoder_grads(x.expand(A_, -1, -1), t.temp)
        m.train()
        for a in range(A_):
            for name in layers:
                ref[(a, name, 0)].grad, ref[(a, name, 1)].grad = g[a][name][0].cpu().clone(), g[a][name][1].cpu().clone()
        opt.step()
        m.set_explicit_noise(noise(1, lo, hi))
        res = t.fit_zinb_decoder(loader(lo, hi), 1, lr=1e-3, weight_decay=wd, state=state)
        state = res["state"]
        assert state["step"] == b + 1 and m.training
        assert res["train_loss"].shape == (1, A_) and res["val_loss"] is None
        assert np.allclose(res["train_loss"][0], [float(g[a]["loss"]) for a in range(A_)], rtol=1e-12)
        worst = 0.0
        for a in range(A_):
            for name in layers:
                lin = getattr(m, name)[a]
                worst = max(worst, float((lin.weight.detach().cpu() - ref[(a, name, 0)].detach()).abs().max()),
                            float((lin.bias.detach().cpu() - ref[(a, name, 1)].detach()).abs().max()))
        print(f"\n  step {b + 1}, weight_decay {wd}: largest difference from torch's Adam {worst:.3e}")
        assert worst < 2e-6
    m.set_explicit_noise(None)


@pytest.mark.parametrize("heads", [("p", "r"), ("rec", "p", "r")])
def test_fit_leaves_everything_else_alone(heads):
    t = trainer()
    m = t.model
    flat = m.flat_parameters()
    lay = m._layout
    before, flat0, bn = bits(m), flat.clone(), m._bn_flat.clone()
    m.set_explicit_noise((noise(1) + noise(1, batch=64)) * 2)            # an epoch's three batches, then score_zinb's one
    res = t.fit_zinb_decoder(loader(), 2, lr=1e-2, heads=heads, test_loader=loader(batch=64), weight_decay=0.01)
    m.set_explicit_noise(None)
    assert m.training and flat.data_ptr() == m.flat_parameters().data_ptr()
    assert res["train_loss"].shape == res["val_loss"].shape == (2, A_) and res["state"]["step"] == 6
    assert np.all(np.isfinite(res["train_loss"])) and np.all(np.isfinite(res["val_loss"]))
    after = bits(m)
    chosen = decoder_names(heads)
    for k in before:
        if k.startswith(chosen):
            assert not torch.equal(before[k], after[k]), k
        else:                                                           # encoder, latent block, BatchNorm, unselected heads
            assert torch.equal(before[k], after[k]), k
    assert torch.equal(bn, m._bn_flat)
    # the flat buffer: nothing outside the decoder's tensors moved, the padding between them included
    touched = torch.zeros_like(flat, dtype=torch.bool)
    for a in range(A_):
        for tn in list(range(16, 26)) + ([26, 27] if "rec" in heads else []):
            o = a * int(lay.per_arm) + int(lay.offset[tn])
            touched[o: o + m._param_of(tn, a).numel()] = True
    assert torch.equal(flat0[~touched], m.flat_parameters()[~touched]) and int((~touched).sum()) > 0
    # val_loss is score_zinb of the fitted model
    m.set_explicit_noise(noise(1, batch=64))
    assert np.array_equal(res["val_loss"][1], t.score_zinb(loader(batch=64))["mean"])
    m.set_explicit_noise([])                                            # an exhausted schedule: the forward raises
    with pytest.raises(RuntimeError, match="exhausted"):
        t.fit_zinb_decoder(loader(0, BATCH), 1)
    assert m.training                                                   # restored after an exception too
    m.set_explicit_noise(None)
    m.eval()
    t.fit_zinb_decoder(loader(0, BATCH), 0)
    assert not m.training                                               # eval stays eval


def test_fit_descends_as_the_restatement_does():
    """Counts drawn with numpy from known heads on the model's own d10, X = log1p; one full batch, 20 steps at lr = 2e-3 on the
    whole decoder.  The float64 restatement of the same fit from the device's zin of that X falls at every step (asserted
    first); the device's losses do too, and follow it."""
    from distributed_vae_amd.utils.dataloader import DeviceLoader
    t = trainer(seed=6)
    m = t.model.eval()
    data, index, u = cells()
    m.set_explicit_noise({"u_state": u})
    m(data[index.to(DEV)].expand(A_, -1, -1), t.temp, eval=True)
    X = RG.draw_counts(m._engine.ws_view("d10", HF)[0].cpu(), np.random.default_rng(5), DM)
    assert 0.3 < float((X == 0).double().mean()) < 0.95
    m(X.to(DEV).expand(A_, -1, -1), t.temp, eval=True)
    zin = m._engine.ws_view("zin", CC + SS).cpu()
    want = []
    for a in range(A_):
        params = [p.detach().cpu() for nm in RD.TRUNK for p in (getattr(m, nm)[a].weight, getattr(m, nm)[a].bias)]
        want.append(RD.adam_losses(zin[a], params, [p.cpu() for p in m._zinb_layers(a)], X, **DESCENT))
        assert np.all(np.diff(want[-1]) < -1e-6), want[-1]
    m.train()
    res = t.fit_zinb_decoder(DeviceLoader(X.to(DEV), torch.arange(N_CELLS), N_CELLS, False, False), DESCENT["steps"], lr=DESCENT["lr"])
    m.set_explicit_noise(None)
    loss = res["train_loss"]
    print(f"\n  loss per arm {loss[0]} -> {loss[-1]}; restatement {[w[0] for w in want]} -> {[w[-1] for w in want]}")
    assert loss.shape == (20, A_) and np.all(np.diff(loss, axis=0) < 0), loss
    assert np.allclose(loss, np.array(want).T, rtol=1e-4, atol=0)


def test_fit_resumes_bit_for_bit_round_trips_and_leaves_no_stale_trunk():
    t4, t22 = trainer(), trainer()
    t22.model.load_state_dict(bits(t4.model))
    t4.model.set_explicit_noise(noise(4))
    r4 = t4.fit_zinb_decoder(loader(), 4, lr=1e-2)
    t22.model.set_explicit_noise(noise(4))
    r2 = t22.fit_zinb_decoder(loader(), 2, lr=1e-2)
    r22 = t22.fit_zinb_decoder(loader(), 2, lr=1e-2, state=r2["state"])
    assert r2["state"]["step"] == 6 and r22["state"]["step"] == r4["state"]["step"] == 12
    assert np.array_equal(np.concatenate([r2["train_loss"], r22["train_loss"]]), r4["train_loss"])
    for k in ("exp_avg", "exp_avg_sq"):
        assert torch.equal(r22["state"][k], r4["state"][k])
    sd4, sd22 = bits(t4.model), bits(t22.model)
    assert all(torch.equal(sd4[k], sd22[k]) for k in sd4)
    with pytest.raises(ValueError, match="state"):
        t22.fit_zinb_decoder(loader(), 1, heads=("p",), state=r2["state"])
    with pytest.raises(ValueError, match="state"):                       # a heads-only state is not a decoder state
        t22.fit_zinb_decoder(loader(), 1, state=t22.fit_zinb_heads(loader(), 0)["state"])
    # a state_dict saved after the fit, loaded into a fresh ZINB model, gives the same bits: no stale trunk anywhere
    fresh = trainer(seed=99)
    assert not torch.equal(fresh.model.fc8[0].weight, t4.model.fc8[0].weight)
    fresh.model.load_state_dict({k: v.cpu() for k, v in sd4.items()})
    data, index, u = cells()
    x = data[index.to(DEV)].expand(A_, -1, -1)
    nll = []
    for t in (t4, fresh):
        t.model.eval()
        t.model.set_explicit_noise({"u_state": u})
        nll.append(t.model.zinb_nll(x, t.temp))
        t.model.set_explicit_noise(noise(1))
        nll.append(t.score_zinb(loader()))
        t.model.set_explicit_noise(None)
    assert torch.equal(nll[0]["cell"], nll[2]["cell"]) and torch.equal(nll[0]["gene"], nll[2]["gene"])
    assert np.array_equal(nll[1]["cell"], nll[3]["cell"]) and np.array_equal(nll[1]["gene"], nll[3]["gene"])


def test_each_batch_meets_the_trunk_of_the_step_before():
    """One epoch of three batches equals three calls of one batch each, bit for bit: between two calls the model's parameters
    are all there is, so the forward of batch k + 1 inside one call read the trunk of step k."""
    t1, t3 = trainer(), trainer()
    t3.model.load_state_dict(bits(t1.model))
    t1.model.set_explicit_noise(noise(1))
    r1 = t1.fit_zinb_decoder(loader(), 1, lr=1e-2)
    state, losses = None, []
    for b in range(3):
        lo, hi = b * BATCH, min((b + 1) * BATCH, N_CELLS)
        t3.model.set_explicit_noise(noise(1, lo, hi))
        r = t3.fit_zinb_decoder(loader(lo, hi), 1, lr=1e-2, state=state)
        state = r["state"]
        losses.append(r["train_loss"][0])
    sd1, sd3 = bits(t1.model), bits(t3.model)
    assert all(torch.equal(sd1[k], sd3[k]) for k in sd1)
    sizes = np.array([min((b + 1) * BATCH, N_CELLS) - b * BATCH for b in range(3)], dtype=np.float64)
    assert np.allclose(r1["train_loss"][0], (np.array(losses) * sizes[:, None]).sum(0) / N_CELLS, rtol=1e-12)
    # and the trunk did move between the batches: the second batch's loss differs from the unfitted model's
    t0 = trainer()
    t0.model.load_state_dict(bits(trainer().model))
    t0.model.eval()
    data, index, _ = cells()
    t0.model.set_explicit_noise(noise(1, BATCH, 2 * BATCH))
    g0 = t0.model.zinb_decoder_grads(data[index[BATCH:2 * BATCH].to(DEV)].expand(A_, -1, -1), t0.temp)
    t0.model.set_explicit_noise(None)
    assert all(float(g0[a]["loss"]) != losses[1][a] for a in range(A_))


@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_a_pruned_categorys_column_of_fc6_stays_zero(wd):
    t = trainer()
    m = t.model
    kept = np.array([0, 1, 3, 4])
    m.prune_apply(kept)                                                  # as prune leaves it: fcc bias 0, fc6's column 0
    assert all(float(m.fcc[a].bias.detach()[2]) == 0.0 and not bool(m.fc6[a].weight.detach()[:, 2].any()) for a in range(A_))
    m.set_explicit_noise(noise(2))
    t.fit_zinb_decoder(loader(), 2, lr=1e-2, weight_decay=wd)
    m.set_explicit_noise(None)
    for a in range(A_):
        col = m.fc6[a].weight.detach()[:, 2]
        assert torch.equal(col.view(torch.int32), torch.zeros_like(col).view(torch.int32))          # +0.0, every bit
        assert bool(m.fc6[a].weight.detach()[:, 1].any())


def test_fit_refusals(monkeypatch):
    from distributed_vae_amd import dist as DD
    t = trainer()
    with pytest.raises(ValueError, match="heads"):
        t.fit_zinb_decoder(loader(), 1, heads=("rec", "pi"))
    with pytest.raises(RuntimeError, match="loss_mode='ZINB'"):
        trainer(mode="MSE").fit_zinb_decoder(loader(), 1)
    with pytest.raises(RuntimeError, match="eval"):
        t.model.train().zinb_decoder_grads(torch.zeros(A_, 4, DM, device=DEV))
    monkeypatch.setattr(DD, "is_dist", lambda: True)
    with pytest.raises(NotImplementedError, match="not data-parallel"):
        t.fit_zinb_decoder(loader(), 1)


def test_the_pinned_refusals_still_hold():
    """What stays refused beside the new names: zinb_loss has no backward, the training entry points do not train a ZINB model."""
    t = trainer()
    h = torch.rand(4, DM, device=DEV)
    with pytest.raises(NotImplementedError, match="no backward"):
        NM.zinb_loss(h.clone().requires_grad_(), h, h, h)
    with pytest.raises(NotImplementedError, match="training under loss_mode='ZINB' is not built"):
        t.model.fused_train_step(h.expand(A_, -1, -1), 1.0, None, do_adam=False)
    with pytest.raises(NotImplementedError, match="training under loss_mode='ZINB' is not built"):
        t._step(h.expand(A_, -1, -1))

"""CPU: the gradient of the ZINB term below the heads -- the restatement's formulas against float64
autograd, a numpy emulation of the kernels' summation order against the device's own error gate, the two C entry points'
host side (workspace, segments, every refusal) through ctypes, the Python surface without a device, and the float64
restatement of the whole-decoder descent experiment.

The statistic is |value - truth| / M (tests/zinb_decoder_restatement.py); where M = 0 the value must be an exact 0."""
import ctypes as C
import inspect
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import zinb_decoder_restatement as RD  # noqa: E402
import zinb_grad_restatement as RG  # noqa: E402
import zinb_restatement as ZR  # noqa: E402
from distributed_vae_amd import _native as N  # noqa: E402
from distributed_vae_amd.nn_model import mk_vae  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12
MARGIN, FLOOR = 3.0, 2.0 ** -23
D10_SHAPES = RG.SHAPES + [(65, 257, 100)]


def _worst(value, truth, M):
    value, truth, M = (np.asarray(t, dtype=np.float64).ravel() for t in (value, truth, M))
    d = np.abs(value - truth)
    assert np.all(np.isfinite(value)) and np.all(d[M == 0] == 0)
    return float((d[M > 0] / M[M > 0]).max()) if (M > 0).any() else 0.0


def _within(name, dev, ref):
    print(f"    {name:<10} emulation max {dev[0]:.3e} p90 {dev[1]:.3e} | reference float32 max {ref[0]:.3e} p90 {ref[1]:.3e}")
    return dev[0] <= max(MARGIN * ref[0], FLOOR) and dev[1] <= max(MARGIN * ref[1], FLOOR)


# ---- 1. the formulas against float64 autograd -------------------------------------------------------------------------------
@pytest.mark.parametrize("n,D,H", D10_SHAPES)
def test_gd10_formula_equals_float64_autograd(n, D, H):
    d10, L, X = RG.inputs(n, D, H)
    d64, L64, X64 = d10.double(), [t.double() for t in L], X.double()
    for heads in (RD.MASKS if (n, D, H) == (65, 33, 100) else [RD.HEADS, ("p",)]):
        e = _worst(RD.gd10_analytic(d64, L64, X64, heads), RD.gd10_autograd(d64, L64, X64, heads), RD.gd10_magnitudes(d10, L, X, heads))
        print(f"  ({n}, {D}, {H}) {heads}: {e:.3e}")
        assert e <= TOL, heads


@pytest.mark.parametrize("n,Z,Lw,H", RD.TRUNK_SHAPES)
def test_trunk_formulas_equal_float64_autograd(n, Z, Lw, H):
    acts32, params, gd10 = RD.trunk_inputs(n, Z, Lw, H)
    want, want_z, acts = RD.trunk_autograd(acts32[0].double(), [t.double() for t in params], gd10.double())
    got, got_z = RD.trunk_backward(acts, [t.double() for t in params], gd10.double())
    M, Mz = RD.trunk_magnitudes(acts, params, gd10)
    for k in range(10):
        assert _worst(got[k], want[k], M[k]) <= TOL, k
    assert _worst(got_z, want_z, Mz) <= TOL
    alive = [float((a > 0).double().mean()) for a in acts[1:]]
    assert n < 60 or all(0.2 < f < 0.95 for f in alive), alive


def test_whole_decoder_autograd_is_the_three_pieces():
    """Autograd through trunk, heads and term at once equals the head gradients of section 9m, gd10 and the trunk's backward
    from that gd10: the decomposition mixVAE_model.zinb_decoder_grads relies on."""
    zin, params, L, X = RD.descent_case()
    sc = 1.0 / X.numel()
    full = RD.decoder_autograd(zin.double(), [t.double() for t in params], [t.double() for t in L], X.double(), sc)
    acts, d10 = full["acts"], full["acts"][5]
    L64 = [t.double() for t in L]
    assert _worst(RD.gd10_analytic(d10, L64, X.double(), scale=sc), full["d10"], RD.gd10_magnitudes(d10, L, X, scale=sc)) <= TOL
    got, gz = RD.trunk_backward(acts, [t.double() for t in params], full["d10"])
    M, Mz = RD.trunk_magnitudes(acts, params, full["d10"])
    for k in range(10):
        assert _worst(got[k], full["trunk"][k], M[k]) <= TOL, k
    assert _worst(gz, full["zin"], Mz) <= TOL
    hg = RG.autograd_heads(d10, L64, X.double(), scale=sc)
    for j, h in enumerate(RG.HEADS):
        assert torch.allclose(hg[h][0], full["heads"][2 * j], rtol=1e-12, atol=1e-300)


# ---- 2. the kernels' summation order, held to the device's gate on the CPU --------------------------------------------------
@pytest.mark.parametrize("n,D,H,segments", [s + (0,) for s in D10_SHAPES] + [(65, 257, 100, 1), (65, 257, 100, 2), (65, 257, 100, 5)])
def test_gd10_emulation_holds_the_gate(n, D, H, segments):
    d10, L, X = RG.inputs(n, D, H)
    sc = 1.0 / (n * D)
    truth = RD.gd10_autograd(d10.double(), [t.double() for t in L], X.double(), scale=sc)
    ref = RD.gd10_autograd(d10, L, X, scale=sc)
    M = RD.gd10_magnitudes(d10, L, X, scale=sc)
    print(f"\n  N = {n}, D = {D}, H = {H}, segments {segments}")
    assert _within("gd10", ZR.error_stat(RD.gd10_emulated(d10, L, X, scale=sc, segments=segments), truth, M), ZR.error_stat(ref, truth, M))


@pytest.mark.parametrize("n,Z,Lw,H", RD.TRUNK_SHAPES)
def test_trunk_emulation_holds_the_gate(n, Z, Lw, H):
    """The kernel's arithmetic (exact products, float64 sums, every dZ rounded to float32 where it is stored) against the
    float64 truth at the same float32 activations, beside float32 autograd's own error."""
    acts, params, gd10 = RD.trunk_inputs(n, Z, Lw, H)
    a64, p64 = [t.double() for t in acts], [t.double() for t in params]
    truth, truth_z = RD.trunk_backward(a64, p64, gd10.double())
    ref, ref_z, racts = RD.trunk_autograd(acts[0], params, gd10)
    assert all(torch.equal(a, b) for a, b in zip(acts, racts))          # float32 autograd meets the same activations
    emu, emu_z = RD.trunk_backward(a64, p64, gd10.double(), rounded=True)
    M, Mz = RD.trunk_magnitudes(acts, params, gd10)
    print(f"\n  N = {n}, Z = {Z}, L = {Lw}, H = {H}")
    ok = True
    for k in range(10):
        ok &= _within(f"{RD.TRUNK[k // 2]}.{'b' if k % 2 else 'W'}", ZR.error_stat(emu[k].float(), truth[k], M[k]), ZR.error_stat(ref[k], truth[k], M[k]))
    ok &= _within("gzin", ZR.error_stat(emu_z.float(), truth_z, Mz), ZR.error_stat(ref_z, truth_z, Mz))
    assert ok


# ---- 3. the C boundary ------------------------------------------------------------------------------------------------------
PTR = 0x1000     # fake device pointers: every case must be refused before anything dereferences them
BAD, UNSUPPORTED, WORKSPACE = -1, -2, -4


def test_entry_points_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "mmvae.h")).read()
    for name in ("mmvae_zinb_d10_grad", "mmvae_zinb_d10_grad_workspace_bytes", "mmvae_zinb_d10_grad_segments",
                 "mmvae_decoder_trunk_grads", "mmvae_decoder_trunk_grads_workspace_bytes", "mmvae_decoder_trunk_grads_segments"):
        assert name + "(" in hdr and hasattr(N.lib(), name), name
    assert hdr.index("int mmvae_zinb_d10_grad(") > hdr.index("int mmvae_zinb_head_grads(")
    assert N.lib().mmvae_abi_version() == N.ABI_VERSION                  # entry points are only added
    assert '"zinb_trunk.hip"' in open(os.path.join(ROOT, "distributed-vae_amd", "build.py")).read()


def test_d10_workspace_bytes_and_segments():
    ws, seg = N.lib().mmvae_zinb_d10_grad_workspace_bytes, N.lib().mmvae_zinb_d10_grad_segments
    for n, D, H, asked, S in ((1, 1, 1, 0, 1), (65, 257, 100, 0, 5), (65, 257, 100, 1, 1), (65, 257, 100, 2, 2), (65, 257, 100, 5, 5),
                              (65, 257, 100, 4, 3), (65, 257, 100, 99, 5), (257, 130, 128, 0, 3), (5000, 5032, 100, 0, 6),
                              (22365, 5032, 100, 0, 1)):
        assert seg(n, D, asked) == S == RD.d10_segments(D, asked, n)[0], (n, D, asked)
        assert ws(n, D, H, asked) == 8 * ((S * n * H + 1) // 2), (n, D, H, asked)
    # never like N x D: 6 segments of N x H floats for 5 000 cells
    assert ws(5000, 5032, 100, 0) == 4 * 6 * 5000 * 100
    assert ws(0, 5, 5, 0) == 0 and ws(5, 0, 5, 0) == 0 and ws(5, 5, 0, 0) == 0 and ws(5, 5, 129, 0) == 0 and ws(5, 5, 5, -1) == 0
    assert ws(1 << 31, 1 << 20, 5, 0) == 0


def _d10_grad(**kw):
    a = dict(d10=PTR, ldh=100, N=64, H=100, D=70, W=PTR, b=PTR, Wp=PTR, bp=PTR, Wr=PTR, br=PTR, X=PTR, ldx=70, eps=1e-6, scale=1.0,
             mask=7, segments=0, ws=PTR, ws_bytes=1 << 40, gd10=PTR, ldg=100)
    a.update(kw)
    return N.lib().mmvae_zinb_d10_grad(a["d10"], a["ldh"], a["N"], a["H"], a["D"], a["W"], a["b"], a["Wp"], a["bp"], a["Wr"], a["br"],
                                       a["X"], a["ldx"], a["eps"], a["scale"], a["mask"], a["segments"], a["ws"], a["ws_bytes"],
                                       a["gd10"], a["ldg"], None)


@pytest.mark.parametrize("kw,rc", [
    (dict(d10=None), BAD), (dict(W=None), BAD), (dict(b=None), BAD), (dict(Wp=None), BAD), (dict(bp=None), BAD), (dict(Wr=None), BAD),
    (dict(br=None), BAD), (dict(X=None), BAD), (dict(ws=None), BAD), (dict(gd10=None), BAD), (dict(mask=0), BAD), (dict(mask=8), BAD),
    (dict(N=0), BAD), (dict(D=0), BAD), (dict(H=0), BAD), (dict(ldh=99), BAD), (dict(ldx=69), BAD), (dict(ldg=99), BAD),
    (dict(eps=-1e-6), BAD), (dict(eps=1.0), BAD), (dict(scale=float("inf")), BAD), (dict(scale=float("nan")), BAD),
    (dict(segments=-1), BAD), (dict(ws=PTR + 4), BAD), (dict(H=129, ldh=129, ldg=129), UNSUPPORTED),
    (dict(N=1 << 31, D=1 << 20, ldx=1 << 20), UNSUPPORTED), (dict(ws_bytes=4 * 2 * 64 * 100 - 1), WORKSPACE)])
def test_zinb_d10_grad_rejects_bad_arguments(kw, rc):
    assert _d10_grad(**kw) == rc
    assert "zinb_d10_grad" in N.lib().mmvae_last_error_string().decode()


def test_trunk_workspace_bytes_and_segments():
    ws, seg = N.lib().mmvae_decoder_trunk_grads_workspace_bytes, N.lib().mmvae_decoder_trunk_grads_segments
    for n, asked, S in ((1, 0, 1), (257, 0, 1), (257, 2, 2), (257, 5, 5), (257, 4, 3), (257, 99, 9), (513, 0, 2), (5000, 0, 10),
                        (22365, 0, 32), (1 << 20, 0, 32)):
        assert seg(n, asked) == S, (n, asked)
    Z, Lw, H = 94, 10, 100
    P = Lw * (Z + 1) + H * (Lw + 1) + 3 * H * (H + 1)
    assert ws(5000, Z, Lw, H, 0) == 4 * 5000 * (Lw + 4 * H) + 8 * 10 * P
    assert ws(63, 9, 5, 7, 0) == 8 * ((63 * 33 + 1) // 2) + 8 * (5 * 10 + 7 * 6 + 3 * 7 * 8)
    assert ws(0, 3, 2, 1, 0) == 0 and ws(5, 0, 2, 1, 0) == 0 and ws(5, 3, 0, 1, 0) == 0 and ws(5, 3, 2, 0, 0) == 0
    assert ws(5, 3, 2, 129, 0) == 0 and ws(5, 3, 129, 2, 0) == 0 and ws(5, 3, 2, 1, -1) == 0 and ws(5, 3, 2, 1, 1025) == 0


def _trunk(**kw):
    a = dict(N=64, Z=9, L=5, H=7, act=[PTR] * 6, ld=[9, 5, 7, 7, 7, 7], params=[PTR] * 10, gd10=PTR, ldg=7, segments=0, ws=PTR,
             ws_bytes=1 << 40, grads=[PTR] * 10, gzin=PTR, ldgz=9)
    a.update(kw)
    arr = lambda v, n: None if v is None else (C.c_void_p * n)(*v)
    ld = None if a["ld"] is None else (C.c_int64 * 6)(*a["ld"])
    return N.lib().mmvae_decoder_trunk_grads(a["N"], a["Z"], a["L"], a["H"], arr(a["act"], 6), ld, arr(a["params"], 10), a["gd10"],
                                             a["ldg"], a["segments"], a["ws"], a["ws_bytes"], arr(a["grads"], 10), a["gzin"],
                                             a["ldgz"], None)


def _one_null(n, k):
    return [None if i == k else PTR for i in range(n)]


@pytest.mark.parametrize("kw,rc", [
    (dict(act=None), BAD), (dict(ld=None), BAD), (dict(params=None), BAD), (dict(grads=None), BAD), (dict(gd10=None), BAD),
    (dict(ws=None), BAD), (dict(act=_one_null(6, 0)), BAD), (dict(act=_one_null(6, 5)), BAD), (dict(params=_one_null(10, 3)), BAD),
    (dict(grads=_one_null(10, 9)), BAD), (dict(N=0), BAD), (dict(Z=0), BAD), (dict(L=0), BAD), (dict(H=0), BAD),
    (dict(segments=-1), BAD), (dict(segments=1025), BAD), (dict(ld=[8, 5, 7, 7, 7, 7]), BAD), (dict(ld=[9, 4, 7, 7, 7, 7]), BAD),
    (dict(ld=[9, 5, 7, 7, 7, 6]), BAD), (dict(ldg=6), BAD), (dict(ldgz=8), BAD), (dict(ws=PTR + 4), BAD),
    (dict(H=129, ld=[9, 5, 129, 129, 129, 129], ldg=129), UNSUPPORTED), (dict(L=129, ld=[9, 129, 7, 7, 7, 7]), UNSUPPORTED),
    (dict(ws_bytes=8 * ((64 * 33 + 1) // 2) + 8 * (5 * 10 + 7 * 6 + 3 * 7 * 8) - 1), WORKSPACE)])
def test_decoder_trunk_grads_rejects_bad_arguments(kw, rc):
    assert _trunk(**kw) == rc
    assert "decoder_trunk_grads" in N.lib().mmvae_last_error_string().decode()


def test_gzin_may_be_null():
    assert _trunk(gzin=None, ldgz=0, ws_bytes=8) == WORKSPACE                # past the pointer and pitch checks
    assert "workspace" in N.lib().mmvae_last_error_string().decode()


# ---- 4. the Python surface without a device ---------------------------------------------------------------------------------
def test_signatures():
    from distributed_vae_amd.cpl_mixvae import cpl_mixVAE
    from distributed_vae_amd.nn_model import mixVAE_model
    p = inspect.signature(cpl_mixVAE.fit_zinb_decoder).parameters
    assert list(p) == list(inspect.signature(cpl_mixVAE.fit_zinb_heads).parameters)
    assert (p["lr"].default, p["heads"].default, p["betas"].default, p["eps"].default, p["weight_decay"].default) == (
        1e-3, ("rec", "p", "r"), (0.9, 0.999), 1e-8, 0.0) and p["state"].default is None and p["test_loader"].default is None
    p = inspect.signature(mixVAE_model.zinb_decoder_grads).parameters
    assert list(p) == ["self", "x", "temp", "mask", "heads"] and p["heads"].default == ("rec", "p", "r")
    assert p["temp"].default == 1.0 and p["mask"].default is None
    p = inspect.signature(N.zinb_d10_grad).parameters
    assert list(p)[:8] == ["d10", "W", "b", "Wp", "bp", "Wr", "br", "X"] and {"heads", "segments", "scale", "out"} <= set(p)
    assert p["segments"].default == 0 and p["scale"].default is None and p["out"].default is None
    assert callable(N.decoder_trunk_grads) and N.TRUNK_LAYERS == RD.TRUNK


def test_refusals_without_a_device(monkeypatch):
    from distributed_vae_amd import dist as DD
    from distributed_vae_amd.cpl_mixvae import cpl_mixVAE
    mse, z = mk_vae(7, 2, 64, "cpu", fc_dim=16, latent_dim=5, mode="MSE").eval(), mk_vae(7, 2, 64, "cpu", fc_dim=16, latent_dim=5,
                                                                                      mode="ZINB")
    x = torch.zeros(2, 3, 64)
    with pytest.raises(RuntimeError, match="loss_mode='ZINB'"):
        mse.zinb_decoder_grads(x)
    with pytest.raises(RuntimeError, match="eval"):
        z.zinb_decoder_grads(x)                                   # training mode
    z.eval()
    with pytest.raises(ValueError, match="heads"):
        z.zinb_decoder_grads(x, heads=("rec", "pi"))
    with pytest.raises(N.NativeError):
        z.zinb_decoder_grads(x)                                   # as far as the device check
    t = torch.zeros(3, 5)
    with pytest.raises(N.NativeError):
        N.zinb_d10_grad(torch.zeros(3, 4), *[torch.zeros(5, 4), torch.zeros(5)] * 3, t)
    with pytest.raises(ValueError, match="heads"):
        N.zinb_d10_grad(torch.zeros(3, 4), *[torch.zeros(5, 4), torch.zeros(5)] * 3, t, heads=())
    acts, params, gd10 = RD.trunk_inputs(3, 4, 2, 5)
    with pytest.raises(N.NativeError):
        N.decoder_trunk_grads(acts, params, gd10)
    with pytest.raises(ValueError, match="six activations"):
        N.decoder_trunk_grads(acts[:5], params, gd10)
    # the trainer's refusals come before any loader or device is touched
    tr = cpl_mixVAE(saving_folder="", device="cpu", save_flag=False)
    tr.init_model(n_categories=5, state_dim=2, input_dim=24, fc_dim=6, lowD_dim=3, n_arm=2)
    with pytest.raises(RuntimeError, match="loss_mode='ZINB'"):
        tr.fit_zinb_decoder(None, 1)
    tz = cpl_mixVAE(saving_folder="", device="cpu", save_flag=False)
    tz.init_model(n_categories=5, state_dim=2, input_dim=24, fc_dim=6, lowD_dim=3, n_arm=2, mode="ZINB")
    with pytest.raises(ValueError, match="heads"):
        tz.fit_zinb_decoder(None, 1, heads=("rec", "gate"))
    for kw in (dict(n_epoch=-1), dict(n_epoch=1, lr=-1e-3), dict(n_epoch=1, lr=float("nan")), dict(n_epoch=1, weight_decay=-0.1),
               dict(n_epoch=1, eps=-1e-8), dict(n_epoch=1, betas=(0.9, 1.0)), dict(n_epoch=1, betas=(-0.1, 0.9)), dict(n_epoch=1, betas=(0.9,))):
        with pytest.raises(ValueError, match="fit_zinb_decoder"):
            tz.fit_zinb_decoder(None, **kw)
    monkeypatch.setattr(DD, "is_dist", lambda: True)
    with pytest.raises(NotImplementedError, match="not data-parallel"):
        tz.fit_zinb_decoder(None, 1)


# ---- 5. the descent experiment's restatement --------------------------------------------------------------------------------
DESCENT = dict(steps=20, lr=2e-3)


def test_descent_restatement_is_monotone():
    """The float64 restatement of a whole-decoder fit: 20 Adam steps at lr = 2e-3 on trunk and heads from nn.Linear's default
    initialisation, one full batch; every step's loss is below the one before, by far more than float32 can blur."""
    zin, params, L, X = RD.descent_case()
    zeros = float((X == 0).double().mean())
    losses = RD.adam_losses(zin, params, L, X, **DESCENT)
    steps = -np.diff(losses)
    print(f"  zeros {zeros:.2f}; loss {losses[0]:.4f} -> {losses[-1]:.4f}; smallest step {steps.min():.3e}")
    assert 0.3 < zeros < 0.95 and np.all(steps > 1e-5) and np.all(np.isfinite(losses))

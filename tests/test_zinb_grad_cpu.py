"""CPU: the gradient of the ZINB term with respect to the heads -- the restatement's analytic table
against float64 autograd, the kernels' element code (psi included) through its host-only debug entries against the
restatement, the C entry points' refusals through ctypes, the Python surface without a device, and the descent experiment's
float64 restatement on the inputs tests/test_gpu_zinb_fit.py uses.

The statistic is |value - truth| / M, M the sum of the magnitudes of the selected branch's addends times the chain factor
(tests/zinb_grad_restatement.magnitudes); where M = 0 (a dead relu) the value must be an exact 0.  The bound 1e-12 keeps the
fp64 arithmetic four orders of magnitude under the 2^-24 rounding of the float32 outputs."""
import inspect
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import zinb_grad_restatement as RG  # noqa: E402
import zinb_restatement as ZR  # noqa: E402
from distributed_vae_amd import _native as N  # noqa: E402
from distributed_vae_amd import nn_model as NM  # noqa: E402
from distributed_vae_amd.nn_model import mk_vae  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12


def _worst(value, truth, M):
    value, truth, M = (np.asarray(t, dtype=np.float64).ravel() for t in (value, truth, M))
    d = np.abs(value - truth)
    assert np.all(np.isfinite(value)) and np.all(d[M == 0] == 0)
    return float((d[M > 0] / M[M > 0]).max()) if (M > 0).any() else 0.0


# ---- 1. the table against autograd ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,D,H", RG.SHAPES)
def test_analytic_table_equals_float64_autograd(n, D, H):
    d10, L, X = RG.inputs(n, D, H)
    a = RG.pre_activations(d10.double(), *(t.double() for t in L))
    got = RG.analytic(*a, X.double())
    same = RG.analytic(*a, X.double(), subtract=True)
    want = RG.autograd_pre(*a, X.double())
    M = RG.magnitudes(*a, X)
    for name, g, g_sub, w, m in zip(RG.HEADS, got, same, want, M):
        # autograd differentiates 1 - p as the restatement's terms form it, by a subtraction that at a gate of +8 leaves
        # 3.4e-4 carrying the 1.1e-16 of p: 3e-13 of the result.  The table with the same subtraction agrees with autograd to
        # a few 1e-15; the table as the kernels evaluate it (1 - s from exp(-|a|)) differs from autograd by that 3e-13,
        # which is autograd's error, not the table's.
        e, e_sub = _worst(g, w, m), _worst(g_sub, w, m)
        print(f"  ({n}, {D}, {H}) {name}: {e:.3e} (1 - p subtracted, as autograd has it: {e_sub:.3e})")
        assert e <= TOL and e_sub <= 1e-14, name
    # the layers' gradients are those products
    hg = RG.autograd_heads(d10.double(), [t.double() for t in L], X.double())
    hM = RG.head_magnitudes(d10, L, X)
    for j, h in enumerate(RG.HEADS):
        assert _worst(got[j].T @ d10.double(), hg[h][0], hM[h][0]) <= TOL
        assert _worst(got[j].sum(0), hg[h][1], hM[h][1]) <= TOL
    # given heads: no relu in front of rec_x
    h32 = ZR.heads(d10, *L)
    gg = RG.autograd_given(*(t.double() for t in h32), X.double())
    assert all(bool(torch.isfinite(t).all()) for t in gg)


# ---- 2. the C++ element code on the host ------------------------------------------------------------------------------------
def test_host_digamma():
    """psi against torch.special.digamma in float64, on the scale of psi's own addends: log of the shifted argument plus
    the recurrence's reciprocals.  Arguments from 1e-6 to 2e3, dense around the switch to the series at 10."""
    x = np.concatenate([np.logspace(-6, np.log10(2e3), 400), np.linspace(8.5, 11.5, 301), [9.999999999, 10.0, 10.000000001, 1.0, 0.5,
                        1.4616321449683623]])
    got = N.debug_digamma_host(x)
    want = torch.special.digamma(torch.from_numpy(x)).numpy()
    n = np.maximum(np.ceil(10.0 - x), 0)
    scale = np.abs(np.log(x + n)) + np.array([sum(1.0 / (xi + i) for i in range(int(ni))) for xi, ni in zip(x, n)])
    e = np.abs(got - want) / scale
    print(f"  digamma: worst {e.max():.3e} of the addends' scale at x = {x[e.argmax()]:.6g}")
    assert e.max() <= TOL
    # outside psi's domain here: the pole, then NaN for anything not positive, and no long walk up the recurrence (a
    # million such arguments return at once)
    odd = N.debug_digamma_host(np.array([0.0, -0.0, -0.5, -3.0, -1e9, -1e300, -np.inf, np.nan, np.inf, 5e-324]))
    assert odd[0] == odd[1] == -np.inf and np.all(np.isnan(odd[2:8])) and odd[8] == np.inf and odd[9] == -np.inf
    assert np.all(np.isnan(N.debug_digamma_host(np.full(1 << 20, -1e18))))
    assert N.ZINB_PSI_SERIES == 10.0 and "constexpr double ZB_PSI_SERIES = 10.0;" in open(
        os.path.join(ROOT, "distributed-vae_amd", "csrc", "zinb_core.hpp")).read()


def _grid():
    """Pre-activations and X that cover: a dead relu (r = eps), r up to 1e3, k = 0 (the zero branch) and k up to 1e3, gates
    at +-8 and between, k + r on both sides of the series' switch at 10."""
    a_rec = [-3.0, 0.0, 1e-3, 0.3, 0.5, 1.0, 4.0, 9.5, 37.0, 1e3]
    k = [0.0, 1.0, 2.0, 5.0, 9.0, 9.5, 10.0, 31.0, 1e3]
    gate = [-8.0, -2.5, 0.0, 0.7, 8.0]
    g = np.array(np.meshgrid(a_rec, k, gate, gate, indexing="ij"), dtype=np.float64).reshape(4, -1)
    return (np.log1p(g[1]).astype(np.float32), g[0].astype(np.float32), g[2].astype(np.float32), g[3].astype(np.float32))


def test_host_element_function_equals_the_restatement():
    X, a_rec, a_p, a_r = _grid()
    kr = np.expm1(X.astype(np.float64)) + np.maximum(a_rec, 0)
    assert ((kr < 10) & (X > 0)).any() and ((kr > 10) & (X > 0)).any() and (a_rec <= 0).any()
    g, term = N.debug_zinb_grad_host(X, a_rec, a_p, a_r)
    t64 = [torch.from_numpy(t).double() for t in (a_rec, a_p, a_r, X)]
    want = RG.analytic(*t64)
    M = RG.magnitudes(*t64)
    for j, name in enumerate(RG.HEADS):
        e = _worst(g[j], want[j], M[j])
        print(f"  host g_{name}: worst {e:.3e} of M")
        assert e <= TOL, name
    assert bool((g[0][a_rec <= 0] == 0).all())
    # the term beside it is zinb_nll's
    h = (torch.relu(t64[0]), torch.sigmoid(t64[1]), torch.sigmoid(t64[2]))
    assert _worst(term, ZR.terms(*h, t64[3]), ZR.magnitudes(*h, t64[3]) + 1) <= TOL


def test_host_element_function_on_the_table_shapes():
    for n, D, H in RG.SHAPES:
        d10, L, X = RG.inputs(n, D, H)
        a = RG.pre_activations(d10, *L)                     # float32 pre-activations, as the kernel's epilogue meets them
        g, _ = N.debug_zinb_grad_host(X.numpy(), *(t.numpy() for t in a))
        want = RG.analytic(*(t.double() for t in a), X.double())
        M = RG.magnitudes(*a, X)
        for j in range(3):
            assert _worst(g[j], want[j], M[j]) <= TOL, (n, D, H, j)


# ---- 3. the C boundary ------------------------------------------------------------------------------------------------------
PTR = 0x1000     # fake device pointers: every case must be refused before anything dereferences them
BAD, UNSUPPORTED, WORKSPACE = -1, -2, -4


def test_entry_points_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "mmvae.h")).read()
    for name in ("mmvae_zinb_head_grads", "mmvae_zinb_head_grads_workspace_bytes", "mmvae_zinb_head_grads_segments",
                 "mmvae_zinb_terms_grad", "mmvae_debug_zinb_grad_host", "mmvae_debug_digamma_host"):
        assert name + "(" in hdr and hasattr(N.lib(), name), name
    assert N.lib().mmvae_abi_version() == 5 == N.ABI_VERSION            # entry points are only added
    assert '"zinb_grad.hip"' in open(os.path.join(ROOT, "distributed-vae_amd", "build.py")).read()


def test_workspace_bytes_and_segments():
    ws, seg, nll = (N.lib().mmvae_zinb_head_grads_workspace_bytes, N.lib().mmvae_zinb_head_grads_segments,
                    N.lib().mmvae_zinb_nll_workspace_bytes)
    for n, D, H, asked, S in ((1, 1, 1, 0, 1), (257, 130, 128, 0, 5), (257, 130, 128, 2, 2), (257, 130, 128, 5, 5),
                              (257, 130, 128, 4, 3), (257, 31, 100, 99, 5), (5000, 5032, 100, 0, 6), (22365, 5032, 100, 0, 6)):
        assert seg(n, D, asked) == S, (n, D, asked)
        floats = S * 3 * D * (H + 1)
        assert ws(n, D, H, asked) == nll(n, D) + 8 * ((floats + 1) // 2), (n, D, H, asked)
    # never like N x D: beyond mmvae_zinb_nll's workspace the partials of 6 segments, 37 MB, for 5 000 cells as for 22 365
    part = [ws(n, 5032, 100, 0) - nll(n, 5032) for n in (5000, 22365, 1 << 20)]
    assert part[0] == part[1] == part[2] == 4 * 6 * 3 * 5032 * 101
    assert ws(0, 5, 5, 0) == 0 and ws(5, 0, 5, 0) == 0 and ws(5, 5, 0, 0) == 0 and ws(5, 5, 129, 0) == 0 and ws(5, 5, 5, -1) == 0
    assert ws(1 << 31, 1 << 20, 5, 0) == 0


def _head_grads(**kw):
    a = dict(d10=PTR, ldh=100, N=64, H=100, D=70, W=PTR, b=PTR, Wp=PTR, bp=PTR, Wr=PTR, br=PTR, X=PTR, ldx=70, eps=1e-6, scale=1.0,
             mask=7, segments=0, ws=PTR, ws_bytes=1 << 40, dW=PTR, db=PTR, dWp=PTR, dbp=PTR, dWr=PTR, dbr=PTR, cell=PTR, gene=PTR)
    a.update(kw)
    return N.lib().mmvae_zinb_head_grads(a["d10"], a["ldh"], a["N"], a["H"], a["D"], a["W"], a["b"], a["Wp"], a["bp"], a["Wr"],
                                         a["br"], a["X"], a["ldx"], a["eps"], a["scale"], a["mask"], a["segments"], a["ws"],
                                         a["ws_bytes"], a["dW"], a["db"], a["dWp"], a["dbp"], a["dWr"], a["dbr"], a["cell"],
                                         a["gene"], None)


@pytest.mark.parametrize("kw,rc", [
    (dict(d10=None), BAD), (dict(W=None), BAD), (dict(b=None), BAD), (dict(Wp=None), BAD), (dict(bp=None), BAD), (dict(Wr=None), BAD),
    (dict(br=None), BAD), (dict(X=None), BAD), (dict(ws=None), BAD), (dict(cell=None), BAD), (dict(gene=None), BAD),
    (dict(dW=None), BAD), (dict(dbp=None), BAD), (dict(dWr=None), BAD), (dict(mask=0), BAD), (dict(mask=8), BAD),
    (dict(mask=6, dWp=None), BAD), (dict(N=0), BAD), (dict(D=0), BAD), (dict(H=0), BAD), (dict(ldh=99), BAD), (dict(ldx=69), BAD),
    (dict(eps=-1e-6), BAD), (dict(eps=1.0), BAD), (dict(scale=float("inf")), BAD), (dict(scale=float("nan")), BAD),
    (dict(segments=-1), BAD), (dict(ws=PTR + 4), BAD), (dict(H=129, ldh=129), UNSUPPORTED),
    (dict(N=1 << 31, D=1 << 20, ldx=1 << 20), UNSUPPORTED),
    (dict(ws_bytes=8 * (3 * 64 + 2 * 70) + 4 * 3 * 70 * 101 - 1), WORKSPACE)])
def test_zinb_head_grads_rejects_bad_arguments(kw, rc):
    assert _head_grads(**kw) == rc
    assert "zinb_head_grads" in N.lib().mmvae_last_error_string().decode()


def _step_grads(**kw):
    a = dict(d10=PTR, ldh=100, N=64, H=100, D=70, W=PTR, b=PTR, Wp=PTR, bp=PTR, Wr=PTR, br=PTR, X=PTR, ldx=70, eps=1e-6, scale=1.0,
             mask=7, segments=0, ws=PTR, ws_bytes=1 << 40, dW=PTR, db=PTR, dWp=PTR, dbp=PTR, dWr=PTR, dbr=PTR, cell=PTR, gene=PTR,
             gd10=PTR, ldg=100)
    a.update(kw)
    return N.lib().mmvae_zinb_step_grads(a["d10"], a["ldh"], a["N"], a["H"], a["D"], a["W"], a["b"], a["Wp"], a["bp"], a["Wr"],
                                         a["br"], a["X"], a["ldx"], a["eps"], a["scale"], a["mask"], a["segments"], a["ws"],
                                         a["ws_bytes"], a["dW"], a["db"], a["dWp"], a["dbp"], a["dWr"], a["dbr"], a["cell"],
                                         a["gene"], a["gd10"], a["ldg"], None)


# the union of the tables of mmvae_zinb_head_grads (above) and mmvae_zinb_d10_grad (test_zinb_decoder_cpu.py), gd10 = None and a
# short ldg; the workspace is the head gradients' (one cell segment) and then gd10's at a segment a gene tile (two)
STEP_WS = 8 * (3 * 64 + 2 * 70) + 4 * 3 * 70 * 101 + 4 * 2 * 64 * 100


@pytest.mark.parametrize("kw,rc", [
    (dict(d10=None), BAD), (dict(W=None), BAD), (dict(b=None), BAD), (dict(Wp=None), BAD), (dict(bp=None), BAD), (dict(Wr=None), BAD),
    (dict(br=None), BAD), (dict(X=None), BAD), (dict(ws=None), BAD), (dict(cell=None), BAD), (dict(gene=None), BAD),
    (dict(gd10=None), BAD), (dict(dW=None), BAD), (dict(dbp=None), BAD), (dict(dWr=None), BAD), (dict(mask=0), BAD),
    (dict(mask=8), BAD), (dict(mask=6, dWp=None), BAD), (dict(N=0), BAD), (dict(D=0), BAD), (dict(H=0), BAD), (dict(ldh=99), BAD),
    (dict(ldx=69), BAD), (dict(ldg=99), BAD), (dict(eps=-1e-6), BAD), (dict(eps=1.0), BAD), (dict(scale=float("inf")), BAD),
    (dict(scale=float("nan")), BAD), (dict(segments=-1), BAD), (dict(ws=PTR + 4), BAD),
    (dict(H=129, ldh=129), BAD),                       # doubly bad: the short ldg is met before H above 128
    (dict(H=129, ldh=129, ldg=129), UNSUPPORTED), (dict(N=1 << 31, D=1 << 20, ldx=1 << 20), UNSUPPORTED),
    (dict(ws_bytes=8 * (3 * 64 + 2 * 70) + 4 * 3 * 70 * 101 - 1), WORKSPACE), (dict(ws_bytes=4 * 2 * 64 * 100 - 1), WORKSPACE),
    (dict(ws_bytes=STEP_WS - 1), WORKSPACE)])
def test_zinb_step_grads_rejects_bad_arguments(kw, rc):
    assert _step_grads(**kw) == rc
    assert "zinb_step_grads" in N.lib().mmvae_last_error_string().decode()


def test_an_unselected_heads_outputs_may_be_null():
    assert _head_grads(mask=6, dW=None, db=None, ws_bytes=8) == WORKSPACE          # past the pointer checks
    assert "workspace" in N.lib().mmvae_last_error_string().decode()


def _terms_grad(**kw):
    a = dict(x_rec=PTR, ld_rec=70, x_p=PTR, ld_p=70, x_r=PTR, ld_r=70, X=PTR, ldx=70, N=64, D=70, eps=1e-6, scale=1.0, g_rec=PTR,
             g_p=PTR, g_r=PTR, ld_g=70)
    a.update(kw)
    return N.lib().mmvae_zinb_terms_grad(a["x_rec"], a["ld_rec"], a["x_p"], a["ld_p"], a["x_r"], a["ld_r"], a["X"], a["ldx"], a["N"],
                                         a["D"], a["eps"], a["scale"], a["g_rec"], a["g_p"], a["g_r"], a["ld_g"], None)


@pytest.mark.parametrize("kw,rc", [
    (dict(x_rec=None), BAD), (dict(x_p=None), BAD), (dict(x_r=None), BAD), (dict(X=None), BAD), (dict(g_rec=None), BAD),
    (dict(g_p=None), BAD), (dict(g_r=None), BAD), (dict(N=0), BAD), (dict(D=0), BAD), (dict(ld_rec=69), BAD), (dict(ld_p=69), BAD),
    (dict(ld_r=69), BAD), (dict(ldx=69), BAD), (dict(ld_g=69), BAD), (dict(eps=2.0), BAD), (dict(scale=float("nan")), BAD),
    (dict(N=1 << 31, D=1 << 20, ld_rec=1 << 20, ld_p=1 << 20, ld_r=1 << 20, ldx=1 << 20, ld_g=1 << 20), UNSUPPORTED)])
def test_zinb_terms_grad_rejects_bad_arguments(kw, rc):
    assert _terms_grad(**kw) == rc
    assert "zinb_terms_grad" in N.lib().mmvae_last_error_string().decode()


# ---- 4. the Python surface without a device ---------------------------------------------------------------------------------
def test_signatures():
    from distributed_vae_amd.cpl_mixvae import cpl_mixVAE
    from distributed_vae_amd.nn_model import mixVAE_model
    p = inspect.signature(cpl_mixVAE.fit_zinb_heads).parameters
    assert list(p) == ["self", "train_loader", "n_epoch", "lr", "heads", "test_loader", "betas", "eps", "weight_decay", "state"]
    assert (p["lr"].default, p["heads"].default, p["betas"].default, p["eps"].default, p["weight_decay"].default) == (
        1e-3, ("rec", "p", "r"), (0.9, 0.999), 1e-8, 0.0) and p["state"].default is None and p["test_loader"].default is None
    p = inspect.signature(mixVAE_model.zinb_head_grads).parameters
    assert list(p) == ["self", "x", "temp", "mask", "heads"] and p["heads"].default == ("rec", "p", "r")
    assert p["temp"].default == 1.0 and p["mask"].default is None
    p = inspect.signature(NM.zinb_loss_grad).parameters
    assert list(p) == ["rec_x", "x_p", "x_r", "X", "eps"] and p["eps"].default == 1e-6
    assert callable(N.zinb_head_grads) and callable(N.zinb_terms_grad)


def test_head_masks():
    assert N.zinb_head_mask(("rec", "p", "r")) == 7 and N.zinb_head_mask(("p", "r")) == 6 and N.zinb_head_mask("rec") == 1
    assert N.zinb_head_mask(["r", "r"]) == 4
    for bad in (("rec", "q"), (), ("fc11",)):
        with pytest.raises(ValueError, match="heads"):
            N.zinb_head_mask(bad)


def test_refusals_without_a_device(monkeypatch):
    from distributed_vae_amd import dist as DD
    from distributed_vae_amd.cpl_mixvae import cpl_mixVAE
    mse, z = mk_vae(7, 2, 64, "cpu", fc_dim=16, latent_dim=5, mode="MSE").eval(), mk_vae(7, 2, 64, "cpu", fc_dim=16, latent_dim=5,
                                                                                      mode="ZINB")
    x = torch.zeros(2, 3, 64)
    with pytest.raises(RuntimeError, match="loss_mode='ZINB'"):
        mse.zinb_head_grads(x)
    with pytest.raises(RuntimeError, match="eval"):
        z.zinb_head_grads(x)                                      # training mode
    z.eval()
    with pytest.raises(ValueError, match="heads"):
        z.zinb_head_grads(x, heads=("rec", "pi"))
    with pytest.raises(N.NativeError):
        z.zinb_head_grads(x)                                      # as far as the device check
    t = torch.zeros(3, 5)
    with pytest.raises(N.NativeError):
        NM.zinb_loss_grad(t, t, t, t)
    with pytest.raises(ValueError):
        NM.zinb_loss_grad(t, t[:2], t, t)
    with pytest.raises(N.NativeError):
        N.zinb_terms_grad(t, t, t, t)
    with pytest.raises(N.NativeError):
        N.zinb_head_grads(torch.zeros(3, 4), *[torch.zeros(5, 4), torch.zeros(5)] * 3, t)
    # zinb_loss keeps its refusal: the gradient lives under a new name
    with pytest.raises(NotImplementedError, match="no backward"):
        NM.zinb_loss(t.clone().requires_grad_(), t, t, t)
    # the trainer's refusals come before any loader or device is touched
    tr = cpl_mixVAE(saving_folder="", device="cpu", save_flag=False)
    tr.init_model(n_categories=5, state_dim=2, input_dim=24, fc_dim=6, lowD_dim=3, n_arm=2)
    with pytest.raises(RuntimeError, match="loss_mode='ZINB'"):
        tr.fit_zinb_heads(None, 1)
    tz = cpl_mixVAE(saving_folder="", device="cpu", save_flag=False)
    tz.init_model(n_categories=5, state_dim=2, input_dim=24, fc_dim=6, lowD_dim=3, n_arm=2, mode="ZINB")
    with pytest.raises(ValueError, match="heads"):
        tz.fit_zinb_heads(None, 1, heads=("rec", "gate"))
    for kw in (dict(n_epoch=-1), dict(n_epoch=1, lr=-1e-3), dict(n_epoch=1, lr=float("nan")), dict(n_epoch=1, weight_decay=-0.1),
               dict(n_epoch=1, eps=-1e-8), dict(n_epoch=1, betas=(0.9, 1.0)), dict(n_epoch=1, betas=(-0.1, 0.9)), dict(n_epoch=1, betas=(0.9,))):
        with pytest.raises(ValueError, match="fit_zinb_heads"):
            tz.fit_zinb_heads(None, **kw)
    monkeypatch.setattr(DD, "is_dist", lambda: True)
    with pytest.raises(NotImplementedError, match="not data-parallel"):
        tz.fit_zinb_heads(None, 1)


# ---- 5. the descent experiment's restatement --------------------------------------------------------------------------------
def test_descent_restatement_is_monotone():
    """The float64 restatement of the fit on exactly the inputs of tests/test_gpu_zinb_fit.py's descent test: 20 Adam steps at
    lr = 1e-2 from nn.Linear's default initialisation, one full batch; every step's loss is below the one before, by far more
    than float32 can blur."""
    d10, L, X = RG.descent_case()
    assert d10.shape == (257, 7) and X.shape == (257, 33)
    zeros = float((X == 0).double().mean())
    losses = RG.adam_losses(d10, L, X, steps=20, lr=1e-2)
    steps = -np.diff(losses)
    print(f"  zeros {zeros:.2f}; loss {losses[0]:.4f} -> {losses[-1]:.4f}; smallest step {steps.min():.3e}")
    assert 0.4 < zeros < 0.9 and np.all(steps > 1e-4) and np.all(np.isfinite(losses))

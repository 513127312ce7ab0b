"""GPU: mixVAE_model.decoder and state_changes on the HIP engine (mmvae_decode / mmvae_state_changes) against the
restatement of tests/decode_restatement.py and the reference's own outputs (tests/golden/decode_a2.npz).

Gates (those of the full-size fp32 suite): the decoder's hidden activations d6 .. d10, read from the decode workspace, within
1e-5 of their scale of the fp64 restatement evaluated on the device's ReLU decisions (a decision may differ only where the
fp64 pre-activation is within 1e-4 of the layer's scale of zero); x_rec within 1e-5 of its scale of fc11 evaluated in fp64
on the device's d10 -- on the bf16 engine on the bf16-rounded fc11 operands (d10, W11, b11), which is what that engine
multiplies."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_restatement as DR  # noqa: E402
from gpu_util import DEV  # noqa: E402
from distributed_vae_amd.nn_model import mixVAE_model  # noqa: E402

pytestmark = pytest.mark.gpu

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decode_a2.npz"))
ENGINES = ["fp32_mfma", "bf16", "fp32x3"]
TOL, MARGIN = 1e-5, 1e-4
# the traversal end to end (encoder, latent block, decoder against fp64): the encoder's BatchNorm divisions and the tau = 0.005
# softmax in front of the straight-through sample carry the fp32 rounding of the encoder into mu and c; the bf16 engine's fc1
# takes rounded operands (its configuration's 5e-2 gate)
TRAV_TOL = {"fp32_mfma": 1e-4, "fp32x3": 1e-4, "bf16": 5e-2}


def _model(A, D, H, L, Cc, S, sd=None, seed=0):
    torch.manual_seed(seed)
    m = mixVAE_model(input_dim=D, fc_dim=H, n_categories=Cc, state_dim=S, lowD_dim=L, x_drop=0.5, s_drop=0.2, n_arm=A, lam=1,
                     lam_pc=1, tau=0.005, beta=1.0, hard=False, variational=True, device=DEV, eps=1e-8, momentum=0.01,
                     ref_prior=False, loss_mode="MSE")
    if sd is not None:
        m.load_state_dict(sd)
    else:
        g = torch.Generator().manual_seed(seed + 1)
        with torch.no_grad():
            for name, buf in m.named_buffers():
                if name.endswith("running_mean"):
                    buf.copy_(0.3 * torch.randn(buf.shape, generator=g))
                elif name.endswith("running_var"):
                    buf.copy_(0.5 + torch.rand(buf.shape, generator=g))
            for p in m.parameters():
                p.mul_(1.5)
    return m.to(DEV).eval()


def _fixture_model():
    sd = {k[3:]: torch.from_numpy(np.asarray(G[k])) for k in G.files if k.startswith("sd/")}
    sd = {k: (v.float() if v.is_floating_point() else v) for k, v in sd.items()}
    A, _, D, H, L, Cc, S = [int(v) for v in G["cfg"]]
    return _model(A, D, H, L, Cc, S, sd)


def _sd64(m):
    return {k: v.detach().double().cpu() for k, v in m.state_dict().items() if v.is_floating_point()}


def _dec_engine(m, A, n, n_samp=None):
    return next(e for k, e in m._dec_engines.items() if k[0] == A and k[1] == n and k[2] == n_samp)


def _check_decode(m, arm, c, s, x_rec, eng, row0=0, engine="fp32x3"):
    """x_rec [N, D] of arm `arm` from rows (c, s); eng: the DecodeEngine whose workspace arm row0 .. holds d6 .. d10."""
    sd = _sd64(m)
    n = c.shape[0]
    h = torch.cat((c, s), dim=1).double().cpu()
    dev = {}
    widths = {"d6": m.lowD_dim, "d7": m.fc_dim, "d8": m.fc_dim, "d9": m.fc_dim, "d10": m.fc_dim}
    for i, (site, name) in enumerate(zip(widths, ("fc6", "fc7", "fc8", "fc9", "fc10"))):
        dv = eng.ws_view(site, widths[site])[row0].double().cpu()
        dev[site] = dv
        z = h @ sd[f"{name}.{arm}.weight"].T + sd[f"{name}.{arm}.bias"]
        scale = float(z.abs().max()) + 1e-30
        near = z.abs() <= MARGIN * scale
        far = ((dv > 0) != (z > 0)) & ~near
        assert not bool(far.any()), (site, int(far.sum()))
        h = torch.where(near, torch.where(dv > 0, z, torch.zeros_like(z)), torch.relu(z))   # the device's decision near zero
        err = float((dv - h).abs().max()) / (float(h.abs().max()) + 1e-30)
        assert err < TOL, (site, err)
    d10, w, b = dev["d10"], sd[f"fc11.{arm}.weight"], sd[f"fc11.{arm}.bias"]
    if engine == "bf16":
        d10, w, b = DR.bf16_round(d10.float()).double(), DR.bf16_round(w.float()).double(), DR.bf16_round(b.float()).double()
    want = torch.relu(d10 @ w.T + b)
    got = x_rec.double().cpu()
    assert got.shape == (n, m.input_dim)
    err = float((got - want).abs().max()) / (float(want.abs().max()) + 1e-30)
    assert err < TOL, err
    assert float(want.abs().max()) > 0


def _codes(A, n, Cc, S, seed):
    g = torch.Generator().manual_seed(seed)
    c = torch.softmax(3 * torch.randn(A, n, Cc, generator=g), -1)
    s = torch.randn(A, n, S, generator=g)
    return c.to(DEV), s.to(DEV)


@pytest.mark.parametrize("engine", ENGINES)
def test_decoder_fixture_size(engine):
    m = _fixture_model()
    m.gemm_dtype = engine
    c = torch.from_numpy(G["dec/c"]).float().to(DEV)
    s = torch.from_numpy(G["dec/s"]).float().to(DEV)
    for a in range(m.n_arm):
        x = m.decoder(c[a], s[a], a)
        torch.cuda.synchronize()
        assert x.device.type == "cuda" and x.shape == (c.shape[1], m.input_dim)
        _check_decode(m, a, c[a], s[a], x, _dec_engine(m, 1, c.shape[1]), engine=engine)
        if engine != "bf16":   # and the reference's own fp64 output
            ref = torch.from_numpy(G["f64/dec/out"][a])
            assert float((x.double().cpu() - ref).abs().max()) < 1e-5 * float(ref.abs().max())


@pytest.mark.parametrize("engine", ENGINES)
def test_decoder_full_size(engine):
    A, D, H, L, Cc, S, n = 2, 5000, 100, 10, 92, 2, 5000
    m = _model(A, D, H, L, Cc, S, seed=3)
    m.gemm_dtype = engine
    c, s = _codes(A, n, Cc, S, 4)
    for a in range(A):
        x = m.decoder(c[a], s[a], a)
        torch.cuda.synchronize()
        _check_decode(m, a, c[a], s[a], x, _dec_engine(m, 1, n), engine=engine)


@pytest.mark.parametrize("engine", ENGINES)
def test_decoder_of_forward_codes_reproduces_forward(engine):
    A, D, H, L, Cc, S, B = 2, 5000, 100, 10, 92, 2, 5000
    m = _model(A, D, H, L, Cc, S, seed=5)
    m.gemm_dtype = engine
    g = torch.Generator().manual_seed(6)
    x = (torch.relu(torch.randn(B, D, generator=g)) * 2).to(DEV)
    with torch.no_grad():
        out = m(x.expand(A, -1, -1), 1.0, eval=True)
    for a in range(A):
        xr = m.decoder(out[6][a], out[5][a], a)
        torch.cuda.synchronize()
        if engine == "fp32_mfma":
            # the same d10 (the same chain kernel on the same ZIN) and the same fc11 accumulation code
            assert torch.equal(xr, out[0][a])
        else:
            # forward(eval) writes x_rec with the fp32 matrix-instruction kernel (fp32x3) or k_bf16_fc11 (bias in fp32)
            err = float((xr - out[0][a]).abs().max()) / float(out[0][a].abs().max())
            assert err < (TOL if engine == "fp32x3" else 2e-2), err


@pytest.mark.parametrize("n", [1, 63, 129, 40000])
@pytest.mark.parametrize("engine", ENGINES)
def test_decoder_ragged_and_beyond_training_cap(engine, n):
    m = _fixture_model()
    m.gemm_dtype = engine
    c, s = _codes(m.n_arm, n, m.n_categories, m.state_dim, n)
    x = m.decoder(c[1], s[1], 1)
    torch.cuda.synchronize()
    _check_decode(m, 1, c[1], s[1], x, _dec_engine(m, 1, n), engine=engine)


def test_decoder_refuses_state_dropout_and_cpu_tensors():
    m = _fixture_model()
    c = torch.from_numpy(G["dec/c"]).float()
    s = torch.from_numpy(G["dec/s"]).float()
    from distributed_vae_amd._native import NativeError
    with pytest.raises(NativeError):
        m.decoder(c[0], s[0], 0)
    m.train()
    with pytest.raises(NotImplementedError):
        m.decoder(c[0].to(DEV), s[0].to(DEV), 0)
    m.s_dp.p = 0.0   # training mode without state dropout decodes as eval mode does
    x_train = m.decoder(c[0].to(DEV), s[0].to(DEV), 0)
    m.eval()
    assert torch.equal(x_train, m.decoder(c[0].to(DEV), s[0].to(DEV), 0))
    m.train()
    with pytest.raises(RuntimeError):
        m.state_changes(torch.from_numpy(G["sc/x"]).float().to(DEV), 0, 1.0)


@pytest.mark.parametrize("engine", ENGINES)
def test_state_changes_matches_reference_fixture(engine):
    m = _fixture_model()
    m.gemm_dtype = engine
    x = torch.from_numpy(G["sc/x"]).float().to(DEV)
    u = torch.from_numpy(G["sc/u"]).float()                      # [A, n_samp, 1]
    d_s, perm = int(G["sc/d_s"]), torch.from_numpy(G["sc/perm"])
    m.set_explicit_state_noise(u.to(DEV))
    recon, srt = m.state_changes(x, d_s, 1.0, n_samp=100)
    m.set_explicit_state_noise(None)
    assert recon.device.type == "cpu" and recon.dtype == torch.float32 and tuple(recon.shape) == (2, 100, 64)
    assert srt.dtype == torch.float32 and tuple(srt.shape) == (2, 100) and not bool(srt.any())
    # sample order on both sides: undo each side's reordering (the same permutation)
    got = torch.empty_like(recon)
    got[:, perm] = recon
    want = torch.empty(2, 100, 64, dtype=torch.float64)
    want[:, perm] = torch.from_numpy(G["f64/sc/recon"])
    tol = TRAV_TOL[engine]
    assert float((got.double() - want).abs().max()) < tol * float(want.abs().max())
    # the restatement on the same draws
    rs = DR.state_changes(_sd64(m), x.double().cpu(), d_s, u.double())[:, :, 0, :]
    assert float((got.double() - rs).abs().max()) < tol * float(rs.abs().max())


def test_state_changes_batch_of_cells_and_philox():
    m = _fixture_model()
    g = torch.Generator().manual_seed(8)
    x3 = (torch.relu(torch.randn(3, m.input_dim, generator=g)) * 2).to(DEV)
    u3 = torch.rand(m.n_arm, 100, 3, generator=g).to(DEV)
    m.set_explicit_state_noise(u3)
    r3, _ = m.state_changes(x3, 0, 1.0)
    assert tuple(r3.shape) == (m.n_arm, 100, 3, m.input_dim)
    for b in range(3):
        m.set_explicit_state_noise(u3[:, :, b:b + 1].contiguous())
        r1, _ = m.state_changes(x3[b:b + 1], 0, 1.0)
        assert torch.equal(r1, r3[:, :, b, :]), b
    # Philox: the same (seed, offset) gives the same output bit for bit; the next offset other draws
    m.set_explicit_state_noise(None)
    m._noise_seed, m._noise_offset = 1234, 10
    p1, z1 = m.state_changes(x3, 1, 1.0, n_samp=7)
    m._noise_offset = 10
    p2, _ = m.state_changes(x3, 1, 1.0, n_samp=7)
    p3, _ = m.state_changes(x3, 1, 1.0, n_samp=7)
    assert torch.equal(p1, p2) and not torch.equal(p1, p3) and not bool(z1.any())


@pytest.mark.parametrize("engine", ENGINES)
def test_state_changes_full_size(engine):
    A, D, H, L, Cc, S = 2, 5000, 100, 10, 92, 2
    m = _model(A, D, H, L, Cc, S, seed=9)
    m.gemm_dtype = engine
    g = torch.Generator().manual_seed(10)
    x = (torch.relu(torch.randn(1, D, generator=g)) * 2).to(DEV)
    u = torch.rand(A, 100, 1, generator=g)
    m.set_explicit_state_noise(u.to(DEV))
    recon, _ = m.state_changes(x, 1, 1.0)
    got = torch.empty_like(recon)
    got[:, torch.zeros(100).sort()[1]] = recon
    want = DR.state_changes(_sd64(m), x.double().cpu(), 1, u.double())[:, :, 0, :]
    tol = TRAV_TOL[engine]
    assert float((got.double() - want).abs().max()) < tol * float(want.abs().max()), engine

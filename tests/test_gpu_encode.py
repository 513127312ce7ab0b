"""GPU: mixVAE_model.encoder / intermed / encode and cpl_mixVAE.encode_dataset on the HIP engine (mmvae_encode /
mmvae_intermed) against ``forward`` (bit for bit: the same kernels), the restatement of tests/encode_restatement.py and the
reference's own outputs (tests/golden/encode_a2.npz).

Tolerances: against the reference fixture, x_low and c_prob at tests/test_gpu_parity.py's FWD_TOL (what that suite applies
to them on the fp32 engines); the bf16 engine, which that suite does not gate on these, at its configuration's 5e-2 gate
(tests/test_gpu_bf16.py LOSS_GATE, tests/test_gpu_decode.py TRAV_TOL).  intermed: per element, against the fp64 product of
its fp32 operands, |mu - ref| <= 2 (K + 2) 2^-24 (sum_i |w_i y_i| + |b|) with K = L + C (K products, K - 1 additions and
the bias in fp32, each within 2^-24 relative, with a factor two in hand), and for var = sigmoid(z) a quarter of that (the
sigmoid's largest slope) plus 2^-23 (its own exp, addition and division).  The largest state head the library accepts is
L + C = 64 + 128 = 192 (mmvae_check_dims: L <= 64, C <= 128), not the 255 of the sum's own limit: that is the K tested."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import encode_restatement as ER  # noqa: E402
from gpu_util import DEV  # noqa: E402
from test_gpu_parity import FWD_TOL  # noqa: E402
from distributed_vae_amd import _native as N  # noqa: E402
from distributed_vae_amd.nn_model import mixVAE_model  # noqa: E402

pytestmark = pytest.mark.gpu

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "encode_a2.npz"))
A, NC, D, H, L, Cc, S = [int(v) for v in G["cfg"]]
ENGINES = ["fp32_mfma", "bf16", "fp32x3"]
REF_TOL = {"fp32_mfma": FWD_TOL, "fp32x3": FWD_TOL, "bf16": 5e-2}
FWD = {"x_low": 3, "c": 4, "c_smp": 6, "s_mean": 7, "s_logvar": 8, "c_prob": 9}
KEPT = [0, 2, 3, 5]                       # a category mask that drops categories 1 and 4


def _model(A_, D_, H_, L_, C_, S_, sd=None, seed=0):
    torch.manual_seed(seed)
    m = mixVAE_model(input_dim=D_, fc_dim=H_, n_categories=C_, state_dim=S_, lowD_dim=L_, x_drop=0.5, s_drop=0.2, n_arm=A_,
                     lam=1, lam_pc=1, tau=0.005, beta=1.0, hard=False, variational=True, device=DEV, eps=1e-8, momentum=0.01,
                     ref_prior=False, loss_mode="MSE")
    if sd is not None:
        m.load_state_dict(sd)
    return m.to(DEV).eval()


def _fixture_sd():
    sd = {k[3:]: torch.from_numpy(np.asarray(G[k])) for k in G.files if k.startswith("sd/")}
    return {k: (v.float() if v.is_floating_point() else v) for k, v in sd.items()}


def _fixture_model(engine="fp32x3"):
    m = _model(A, D, H, L, Cc, S, _fixture_sd())
    m.gemm_dtype = engine
    return m


def _sd64(m):
    return {k: (v.detach().double().cpu() if v.is_floating_point() else v.detach().cpu()) for k, v in m.state_dict().items()}


def _cells(n, seed=1):
    g = torch.Generator().manual_seed(seed)
    return (torch.relu(torch.randn(n, D, generator=g)) * 2).to(DEV)


X = torch.from_numpy(G["x"]).float()


def _rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


# ---- 1. eval identity ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", [None, KEPT], ids=["nomask", "mask"])
@pytest.mark.parametrize("engine", ENGINES)
def test_eval_identity_with_forward(engine, mask):
    m = _fixture_model(engine)
    x = X.to(DEV)
    xs = x.expand(A, -1, -1)
    with torch.no_grad():
        out = m(xs, 1.0, eval=True, mask=mask)
    enc = m.encode(xs, 1.0, mask=mask)
    assert sorted(enc) == sorted(list(FWD) + ["labels"])
    for name, i in FWD.items():
        assert enc[name].device.type == "cuda" and torch.equal(enc[name], torch.stack(list(out[i]))), name
    assert enc["labels"].dtype == torch.int32 and torch.equal(enc["labels"].long(), torch.stack(list(out[4])).argmax(-1))
    if mask is None:
        assert torch.equal(enc["labels"], m.eval_labels(xs, 1.0))
    else:
        dropped = [k for k in range(Cc) if k not in KEPT]
        assert bool((enc["c"][:, :, dropped] == 0).all()) and bool((enc["c"][:, :, KEPT].sum(-1) > 0.99).all())
        assert not bool(torch.isin(enc["labels"].long(), torch.tensor(dropped, device=DEV)).any())
    for a in range(A):
        x_low, c_prob = m.encoder(x, a)
        assert x_low.device.type == "cuda" and tuple(x_low.shape) == (NC, L) and tuple(c_prob.shape) == (NC, Cc)
        assert torch.equal(x_low, out[3][a]) and torch.equal(c_prob, out[9][a]), a


# ---- 2. eval against the reference fixture ----------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", ENGINES)
def test_encoder_eval_matches_reference_fixture(engine):
    m = _fixture_model(engine)
    sd0 = {k: v.clone() for k, v in m.state_dict().items()}
    for a in range(A):
        x_low, c_prob = m.encoder(X.to(DEV), a)
        e1, e2 = _rel(x_low, G["f64/enc/x_low"][a]), _rel(c_prob, G["f64/enc/c_prob"][a])
        print(f"{engine} arm {a}: x_low {e1:.3e} c_prob {e2:.3e}")
        assert e1 < REF_TOL[engine] and e2 < REF_TOL[engine], (e1, e2)
    for k, v in m.state_dict().items():                 # eval must not touch the BatchNorm buffers
        assert torch.equal(v, sd0[k]), k


# ---- 3. training identity -------------------------------------------------------------------------------------------------
def _bn(m, a, i):
    lay = m._layout
    o, n = a * int(lay.bn_per_arm), int(lay.bn_dim[i])
    om, ov = o + int(lay.bn_mean_offset[i]), o + int(lay.bn_var_offset[i])
    return torch.cat((m._bn_flat[om:om + n], m._bn_flat[ov:ov + n])).clone(), int(m._nbt[a * N.N_BN + i])


def _train_noise(B, seed):
    g = torch.Generator().manual_seed(seed)
    return {"x_mask": (torch.rand(A, B, D, generator=g) < 0.5).to(torch.uint8).to(DEV),
            "u_gumbel": torch.rand(A, B, Cc, generator=g).clamp(1e-6, 1 - 1e-6).to(DEV),
            "u_state": torch.rand(A, B, S, generator=g).to(DEV),
            "s_mask": (torch.rand(A, B, S, generator=g) < 0.8).to(torch.uint8).to(DEV)}


@pytest.mark.parametrize("engine", ENGINES)
def test_training_identity_with_forward(engine):
    B = 32
    x = _cells(B, 2)
    m1, m2 = _fixture_model(engine).train(), _fixture_model(engine).train()
    noise = _train_noise(B, 3)
    m2.flat_parameters()                                # (packs the flat buffers: _bn reads them)
    before = [[_bn(m2, a, i) for i in range(6)] for a in range(A)]
    m1.set_explicit_noise(noise)
    m2.set_explicit_noise(noise)
    out = m1(x.expand(A, -1, -1), 1.0)
    for a in range(A):
        x_low, c_prob = m2.encoder(x, a)
        assert torch.equal(x_low, out[3][a]) and torch.equal(c_prob, out[9][a]), a
        if a == 0:                                      # a call for arm 0 leaves arm 1's statistics untouched
            for i in range(6):
                st, n = _bn(m2, 1, i)
                assert torch.equal(st, before[1][i][0]) and n == before[1][i][1], i
    for a in range(A):
        for i in range(5):
            (s1, n1), (s2, n2) = _bn(m1, a, i), _bn(m2, a, i)
            assert torch.equal(s1, s2) and n1 == n2 == before[a][i][1] + 1, (a, i)
            assert not torch.equal(s2, before[a][i][0]), (a, i)
        st, n = _bn(m2, a, 5)                           # the state BatchNorm belongs to forward
        assert torch.equal(st, before[a][5][0]) and n == before[a][5][1]
    # Philox at equal seed and offset: the draw is forward's
    for m in (m1, m2):
        m.set_explicit_noise(None)
        m._noise_seed, m._noise_offset = 1234, 10
    out = m1(x.expand(A, -1, -1), 1.0)
    for a in range(A):
        m2._noise_offset = 10
        x_low, _ = m2.encoder(x, a)
        assert m2._noise_offset == 11
        assert torch.equal(x_low, out[3][a]), a


# ---- 4. intermed ------------------------------------------------------------------------------------------------------------
def _check_intermed(m, a, y, mu, var):
    sd = _sd64(m)
    K = y.shape[1]
    y64 = y.double().cpu()
    u = 2.0 ** -24
    for name, got in (("fc_mu", mu), ("fc_sigma", var)):
        w, b = sd[f"{name}.{a}.weight"], sd[f"{name}.{a}.bias"]
        z = y64 @ w.T + b
        bound = 2 * (K + 2) * u * (y64.abs() @ w.abs().T + b.abs())
        if name == "fc_sigma":
            z, bound = torch.sigmoid(z), bound / 4 + 2.0 ** -23
        err = (got.double().cpu() - z).abs()
        print(f"intermed {name} K={K}: max err / bound {float((err / bound).max()):.3f}")
        assert bool((err <= bound).all()), (name, float((err / bound).max()))


def test_intermed_fixture_shape_and_forward_state_mean():
    m = _fixture_model()
    y = torch.from_numpy(G["im/y"]).float().to(DEV)
    for a in range(A):
        mu, var = m.intermed(y[a], a)
        assert mu.device.type == "cuda" and tuple(mu.shape) == tuple(var.shape) == (NC, S)
        _check_intermed(m, a, y[a], mu, var)
        assert _rel(mu, G["f64/im/mu"][a]) < 1e-5 and _rel(var, G["f64/im/var"][a]) < 1e-5
    with torch.no_grad():
        out = m(X.to(DEV).expand(A, -1, -1), 1.0, eval=True)
    for a in range(A):
        yf = torch.cat((out[3][a], out[6][a]), dim=1)
        mu, var = m.intermed(yf, a)
        _check_intermed(m, a, yf, out[7][a], var)          # forward's s_mean within the bound of the same product
        _check_intermed(m, a, yf, mu, var)
    m.train()                                           # no BatchNorm, no dropout: training mode computes the same
    assert torch.equal(m.intermed(yf, A - 1)[0], mu)


def test_intermed_largest_state_head():
    m = _model(2, 64, 16, 64, 128, 32, seed=4)          # K = L + C = 192, S = 32: the library's limits
    g = torch.Generator().manual_seed(5)
    for n in (1, 50):
        y = torch.cat((torch.randn(n, 64, generator=g), torch.softmax(3 * torch.randn(n, 128, generator=g), -1)), 1).to(DEV)
        for a in range(2):
            mu, var = m.intermed(y, a)
            assert tuple(mu.shape) == (n, 32)
            _check_intermed(m, a, y, mu, var)


# ---- 5. ragged sizes in eval mode, rows of a larger destination ------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 65, 129, 32769])
@pytest.mark.parametrize("engine", ENGINES)
def test_ragged_and_beyond_training_cap(engine, n):
    m = _fixture_model(engine)
    x = _cells(n, n)
    xs = x.expand(A, -1, -1)
    enc = m.encode(xs, 1.0)
    with torch.no_grad():
        out = m(xs, 1.0, eval=True)
    for name, i in FWD.items():
        assert torch.equal(enc[name], torch.stack(list(out[i]))), name
    sd = _sd64(m)
    for a in range(A):
        x_low, c_prob = m.encoder(x, a)
        assert torch.equal(x_low, enc["x_low"][a]) and torch.equal(c_prob, enc["c_prob"][a])
        r_low, r_prob, _ = ER.encoder(sd, a, x.double().cpu())
        assert _rel(x_low, r_low) < REF_TOL[engine] and _rel(c_prob, r_prob) < REF_TOL[engine]
    # rows [row0, row0 + n) of a larger destination, nothing else
    row0, rows = 5, n + 12
    widths = {"x_low": L, "c_prob": Cc, "c": Cc, "c_smp": Cc, "s_mean": S, "s_logvar": S}
    dst = {k: torch.full((A, rows, w), -777.0, device=DEV) for k, w in widths.items()}
    dst["labels"] = torch.full((A, rows), -7, dtype=torch.int32, device=DEV)
    m.encode(xs, 1.0, out=dst, row0=row0)
    for k, t in dst.items():
        assert torch.equal(t[:, row0:row0 + n], enc[k]), k
        sentinel = -7 if k == "labels" else -777.0
        assert bool((t[:, :row0] == sentinel).all()) and bool((t[:, row0 + n:] == sentinel).all()), k


# ---- 6. encode_dataset ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pruned", [False, True], ids=["unpruned", "pruned"])
def test_encode_dataset_equals_eval_model(pruned):
    from torch.utils.data import DataLoader, TensorDataset
    from distributed_vae_amd.cpl_mixvae import cpl_mixVAE
    t = cpl_mixVAE(saving_folder="", device=0, save_flag=False)
    t.init_model(n_categories=Cc, state_dim=S, input_dim=D, fc_dim=H, lowD_dim=L, x_drop=0.5, s_drop=0.2, n_arm=A, temp=1.0,
                 tau=0.005)
    t.model.load_state_dict(_fixture_sd())
    if pruned:
        with torch.no_grad():
            for a in range(A):
                t.model.fcc[a].bias[1] = 0.0
                t.model.fcc[a].bias[4] = 0.0
    x = _cells(70, 9).cpu()
    dl = DataLoader(TensorDataset(x, torch.arange(70, dtype=torch.float32)), batch_size=32, shuffle=False)
    got, want = t.encode_dataset(dl), t.eval_model(dl)
    keys = ["state_mu", "state_var", "state_cat", "prob_cat", "predicted_label", "data_indx", "z_prob", "z_sample", "x_low",
            "prune_indx", "cnss"]
    assert sorted(got) == sorted(keys)
    for k in keys:
        g_, w_ = np.asarray(got[k]), np.asarray(want[k])
        assert g_.shape == w_.shape and g_.dtype == w_.dtype, k
        assert np.array_equal(g_, w_), k
    assert list(got["prune_indx"]) == ([1, 4] if pruned else [])
    if pruned:
        assert not got["z_prob"][:, :, [1, 4]].any()


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals():
    m = _fixture_model()
    x = X.to(DEV)
    with pytest.raises(N.NativeError):
        m.encoder(X, 0)
    with pytest.raises(N.NativeError):
        m.intermed(torch.from_numpy(G["im/y"][0]).float(), 0)
    with pytest.raises(N.NativeError):
        m.encode(X.expand(A, -1, -1))
    for bad in (-1, A):
        with pytest.raises(IndexError):
            m.encoder(x, bad)
        with pytest.raises(IndexError):
            m.intermed(torch.zeros(3, L + Cc, device=DEV), bad)
    with pytest.raises(AssertionError):
        m.encoder(x[:, :D - 1], 0)
    with pytest.raises(IndexError):
        m.encode(x.expand(A, -1, -1), mask=[0, Cc])
    m.varitional = False
    with pytest.raises(AssertionError, match="Non-variational not implemented"):
        m.intermed(torch.zeros(3, L + Cc, device=DEV), 0)
    m.varitional = True
    m.train()
    with pytest.raises(RuntimeError):
        m.encode(x.expand(A, -1, -1))
    # training-mode mmvae_encode asked for c: mmvae_forward is the call for that
    eng = m._ensure(NC)
    out = {"x_low": torch.empty(A, NC, L, device=DEV), "c": torch.empty(A, NC, Cc, device=DEV)}
    with pytest.raises(NotImplementedError):
        eng.encode(m._hyper(1.0, False), N.make_noise(None, 1, 1), m._flat, m._bn_flat, m._nbt, x, 0, out)

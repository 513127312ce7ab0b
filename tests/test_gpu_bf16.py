"""-m gpu: BASELINE.json configs[2] -- bf16 operands in the five D x H GEMMs (fc1, fc11, d(d10), dW1, dW11), fp32
accumulation, everything else fp32 (``model.gemm_dtype = "bf16"`` -> ``mmvae_hyper.gemm_bf16``; csrc/gemm_bf16.hip).

Two kinds of checks:
  * the GEMM engine, exactly: every one of the five products is recomputed on the host in fp64 from the SAME operands the
    device kernel consumed (read back from the workspace), rounded to bf16 the way the kernel rounds them
    (round-to-nearest-even).  bf16 x bf16 products are exact in fp32, so device and host may differ by fp32 accumulation
    order only: 2e-5 of the result's largest magnitude, ragged shapes included (rows / genes / K not multiples of the
    128 x 128 x 64 tiles);
  * the configuration against the fp32 ORACLE ("bf16 config: report, don't gate, beyond rtol
    5e-2 on loss"): loss terms within 5e-2, gradients reported through their cosine with the oracle's.
"""
import numpy as np
import pytest
import torch

from oracle import restatement as R
from tests import golden_util as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ENGINE_TOL = 2e-5
LOSS_GATE = 5e-2


def bf16_round(t: torch.Tensor) -> torch.Tensor:
    from tests import gpu_util as U
    return U.bf16_round(t)


def _run(h, B, seed, dtype):
    from tests import gpu_util as U
    sd = R.init_state_dict(h, seed)
    x = R.synthetic_batch(B, h.input_dim, seed=seed + 1)
    noise = R.draw_noise(h, B, seed=seed + 2)
    m = U.build_model(h, sd)
    m.train()
    m.gemm_dtype = dtype
    m.set_explicit_noise(U.noise_to_device(noise))
    buf = m.fused_train_step(x.to(DEV).expand(h.n_arm, -1, -1), 1.0, None, do_adam=False).clone()
    torch.cuda.synchronize()
    return m, sd, x, noise, buf.cpu()


def _rel(a, b):
    return float((a - b).abs().max() / (b.abs().max() + 1e-300))


@pytest.mark.parametrize("shape", [(2, 300, 520, 100), (3, 130, 192, 100), (2, 257, 1000, 64)])
def test_the_five_gemms_reproduce_bf16_rounded_products(shape):
    A, B, D, H = shape
    h = R.Hyper(input_dim=D, fc_dim=H, n_categories=12, state_dim=2, lowD_dim=6, n_arm=A)
    m, sd, x, noise, _ = _run(h, B, 21, "bf16")
    from tests import gpu_util as U
    assert m._hyper(1.0, False).gemm_bf16 == 1
    grads = {k: gv.detach().cpu() for (k, _), gv in zip(m.named_parameters(), m._grad_views)}
    U.assert_five_bf16_products(m._engine, grads, sd, x, noise, h, ENGINE_TOL)


@pytest.mark.parametrize("name", ["tiny_a2", "tiny_a5_hard", "ragged_a2"])
def test_bf16_configuration_against_the_reference_fixtures(name):
    """The reference-generated golden cases through the bf16 configuration: loss terms within the stated 5e-2."""
    from tests import gpu_util as U
    g = G.load(name)
    h = G.hyper_of(g)
    m = U.build_model(h, G.state_dict_of(g))
    m.train()
    m.gemm_dtype = "bf16"
    x = torch.from_numpy(g["x"]).to(DEV)
    out, lt, grads = U.run_step(m, x, G.noise_of(g))
    for got, key in ((lt[0], "loss/total"), (lt[2], "loss/joint"), (lt[4], "loss/c_dist")):
        assert abs(float(got) - float(g[key])) <= LOSS_GATE * abs(float(g[key])), key
    assert G.rel_err(lt[1].cpu(), g["loss/rec"]) < LOSS_GATE
    cos = []
    for k, v in grads.items():
        ref = torch.from_numpy(g["grad/" + k]).double().flatten()
        if float(ref.norm()) > 0:
            cos.append(float(torch.dot(v.double().flatten(), ref) / (v.double().norm() * ref.norm() + 1e-300)))
    # (hard = straight-through argmax: a sample may switch category under bf16 noise, so the worst tensor is looser there)
    assert min(cos) > (0.6 if bool(g["hard"]) else 0.9) and float(np.median(cos)) > 0.99, (min(cos), float(np.median(cos)))


def test_bf16_configuration_at_full_size_against_the_oracle():
    """A = 2, B = D = 5000 (the benchmark shape): loss vector of the bf16 step against the fp32 oracle, and the
    gradients' agreement with it -- reported by pytest -s, gated at SURVEY.md's 5e-2 on the loss."""
    A, B, D = 2, 5000, 5000
    h = R.Hyper(input_dim=D, n_arm=A)
    m, sd, x, noise, buf = _run(h, B, 546, "bf16")
    _, lt, g_ref = R.grads_autograd({k: v.clone() for k, v in sd.items()}, [x] * A, h, noise)
    want = [float(lt[0]), float(lt[2]), float(lt[3]), float(lt[4]), float(lt[5])] + [float(v) for v in lt[1]]
    got = buf[:5 + A].double().tolist()
    errs = [abs(a - b) / (abs(b) + 1e-30) for a, b in zip(got, want)]
    print("bf16 vs fp32 oracle, relative error of (total, joint, c_ent, c_dist, c_l2, rec...):", ["%.2e" % e for e in errs])
    assert max(errs[i] for i in (0, 1, 3, 5, 6)) < LOSS_GATE, errs
    worst = 1.0
    for (k, _), gv in zip(m.named_parameters(), m._grad_views):
        ref = g_ref[k].double().flatten()
        v = gv.detach().cpu().double().flatten()
        c = float(torch.dot(v, ref) / (v.norm() * ref.norm() + 1e-300))
        worst = min(worst, c)
    print("bf16 vs fp32 oracle, worst gradient cosine over the parameter tensors: %.5f" % worst)
    assert worst > 0.9
    # and the fp32 configuration of the same model object is untouched by the switch
    m.gemm_dtype = "fp32_mfma"
    assert m._hyper(1.0, False).gemm_bf16 == 0


@pytest.mark.parametrize("cfg", [(16, 10, 640, 320, 3, 257), (50, 10, 5032, 500, 2, 5000)])
def test_bf16_augmenter_layers_reproduce_bf16_rounded_products(cfg):
    """The augmenter's ten large Linear layers through the bf16 tile engine (``netA.gemm_dtype = "bf16"``): against the
    oracle with both operands of exactly those products rounded to bf16 (fp64 accumulation) -- twelve chained layers, so
    the tolerance is the fp32 path's 1e-4 of the output scale, not the single-GEMM 2e-5 -- and, reported, against the
    plain fp32 oracle.  Second shape: the production one at the SmartSeq gene count (D / 5 = 1006: padded rows)."""
    import distributed_vae_amd  # noqa: F401
    from distributed_vae_amd.augmentation import Augmenter_smartseq
    from oracle import augmenter as OA
    NZ, Z, D, ND, A, B = cfg
    sd = OA.random_state_dict(NZ, Z, D, ND, seed=NZ + D)
    m = Augmenter_smartseq(noise_dim=NZ, latent_dim=Z, input_dim=D, n_dim=ND)
    m.load_state_dict(sd)
    m = m.to(DEV).eval()
    m.gemm_dtype = "bf16"
    g = torch.Generator().manual_seed(B)
    x = (torch.rand(B, D, generator=g) < 0.3).float() * torch.randn(B, D, generator=g).abs() * 3
    z0, eps = torch.randn(A, B, NZ, generator=g), torch.randn(A, B, Z, generator=g)
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    s_ref, x_ref = OA.forward_eval(sd64, x.double().expand(A, -1, -1), z0.double(), eps.double(), 0.1, gemm_round=bf16_round)
    s_f32, x_f32 = OA.forward_eval(sd64, x.double().expand(A, -1, -1), z0.double(), eps.double(), 0.1)
    m.set_explicit_noise(z0, eps)
    s, xa = m(x.to(DEV).expand(A, -1, -1), True, 0.1)
    # the host restatement rounds activations that differ from the device's by fp32 accumulation noise: a value that
    # sits on a bf16 rounding boundary may round the other way, which is one bf16 ulp (2^-8) of ONE operand element
    # -- and every such flip propagates through the remaining layers (a chaotic comparison by construction): 4e-3 at the
    # small shape (2.4e-3 measured on the planes x planes engine of round 4, whose fp32 accumulation order -- 256 x 256 tiles, K
    # steps of 16 -- differs from the 128 x 128 tile engine's 0.9e-3), 6e-3 across ten layers with K up to 5032, against ~1e-2
    # between the bf16 and fp32 configurations
    tol = 4e-3 if D < 2000 else 6e-3
    e_s, e_x = _rel(s.cpu().double(), s_ref), _rel(xa.cpu().double(), x_ref)
    print("bf16 augmenter vs bf16-rounded oracle: s %.2e  x_aug %.2e" % (e_s, e_x))
    assert e_s < tol and e_x < tol, (e_s, e_x)
    print("bf16 augmenter vs fp32 oracle: s %.2e  x_aug %.2e" % (_rel(s.cpu().double(), s_f32), _rel(xa.cpu().double(), x_f32)))
    assert _rel(xa.cpu().double(), x_f32) < LOSS_GATE
    m.gemm_dtype = "fp32"
    s2, xa2 = m(x.to(DEV).expand(A, -1, -1), True, 0.1)
    assert _rel(xa2.cpu().double(), x_f32) < 1e-4


def test_bf16_step_is_bit_reproducible_at_full_size():
    """Every reduction of the bf16 kernels has a fixed order too (split slabs, no float atomics, the fused d(d10)
    accumulates per wave in program order): identical state and noise give bit-identical losses and gradients."""
    from tests import gpu_util as U
    from distributed_vae_amd import _native as N
    A, B, D = 2, 5000, 5000
    h = R.Hyper(input_dim=D, n_arm=A)
    torch.manual_seed(546)
    m = U.build_model(h, None)
    m.train()
    m.gemm_dtype = "bf16"
    x = R.synthetic_batch(B, D).to(DEV)
    eng = m._ensure(B)
    hyper, noise = m._hyper(1.0, False), N.make_noise(None, 7, 3)
    assert hyper.gemm_bf16 == 1
    bn0, nbt0 = m._bn_flat.clone(), m._nbt.clone()
    ref = None
    for it in range(8):
        m._bn_flat.copy_(bn0)
        m._nbt.copy_(nbt0)
        buf = eng.train_step(hyper, noise, m._flat, m._bn_flat, m._nbt, x, 0, m._flat_grad, False, None, None, 1, 0.0)
        cur = (m._flat_grad.clone(), buf.clone())
        if ref is None:
            ref = cur
        else:
            assert torch.equal(cur[0], ref[0]) and torch.equal(cur[1], ref[1]), f"iteration {it} differs"
    assert torch.isfinite(ref[0]).all() and float(ref[0].abs().max()) > 0


# ---- bf16 storage (mmvae_train_step_rows(data_bf16)) -------------------------------------------------
def _rows_model(h, seed, noise):
    from tests import gpu_util as U
    m = U.build_model(h, R.init_state_dict(h, seed))
    m.train()
    m.gemm_dtype = "bf16"
    m.set_explicit_noise(U.noise_to_device(noise))
    return m


def test_to_bf16_rounds_to_nearest_even():
    import distributed_vae_amd  # noqa: F401
    from distributed_vae_amd import _native as N
    g = torch.Generator().manual_seed(3)
    x = torch.randn(301, 520, generator=g) * torch.logspace(-42, 30, 520)[None, :]       # denormals .. huge
    x[0, :8] = torch.tensor([0.0, -0.0, float("inf"), -float("inf"), 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 3.3895e38, -1e-45])
    base = torch.zeros(301, 528)                                                          # a row pitch beyond the width
    base[:, :520] = x
    d = base.to(DEV)[:, :520]
    got = N.to_bf16(d)
    assert got.stride() == d.stride() and got.dtype == torch.bfloat16
    want = x.to(torch.bfloat16)
    assert torch.equal(got.cpu().view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("shape", [(2, 300, 520, 100, 520), (3, 130, 192, 100, 200), (2, 257, 1000, 64, 1000)])
def test_bf16_storage_equals_the_step_on_the_rounded_matrix(shape):
    """The row-indexed bf16 step reading the matrix's bf16 COPY (and keeping dZ11 as bf16) against the same step on an fp32
    matrix that holds the rounded values: loss vector, gradients, BatchNorm statistics bit for bit -- the copy changes what
    is moved, not what is computed."""
    import distributed_vae_amd  # noqa: F401
    from distributed_vae_amd import _native as N
    A, B, D, H, ld = shape
    h = R.Hyper(input_dim=D, fc_dim=H, n_categories=12, state_dim=2, lowD_dim=6, n_arm=A)
    n_rows = 3 * B + 7
    base = torch.zeros(n_rows, ld)
    base[:, :D] = R.synthetic_batch(n_rows, D, seed=31)
    data = base.to(DEV)[:, :D]
    data16 = N.to_bf16(data)
    rounded = torch.zeros(n_rows, ld, device=DEV)
    rounded[:, :D] = data16.float()
    rounded = rounded[:, :D]
    g = torch.Generator().manual_seed(B)
    rows = torch.randint(0, n_rows, (B,), generator=g)
    rows[:4] = torch.tensor([0, n_rows - 1, 5, 5])                          # edges and a repeated row
    noise = R.draw_noise(h, B, seed=33)
    out = []
    for use16 in (False, True):
        m = _rows_model(h, 32, noise)
        buf = m.fused_train_step_rows(rounded if not use16 else data, rows.to(DEV), 1.0, None, do_adam=False,
                                      data16=data16 if use16 else None).clone()
        torch.cuda.synchronize()
        out.append((buf.cpu(), m.flat_grad().detach().cpu().clone(), m._bn_flat.detach().cpu().clone()))
    assert torch.equal(out[0][0], out[1][0])
    assert torch.equal(out[0][1], out[1][1])
    assert torch.equal(out[0][2], out[1][2])
    assert bool(torch.isfinite(out[1][1]).all()) and float(out[1][1].abs().max()) > 0


def test_bf16_storage_is_refused_where_it_does_not_apply():
    import distributed_vae_amd  # noqa: F401
    from distributed_vae_amd import _native as N
    h = R.Hyper(input_dim=520, fc_dim=100, n_categories=12, state_dim=2, lowD_dim=6, n_arm=2)
    data = R.synthetic_batch(400, 520, seed=1).to(DEV)
    rows = torch.arange(128, device=DEV)
    m = _rows_model(h, 2, R.draw_noise(h, 128, seed=3))
    m.gemm_dtype = "fp32"                                                   # the fp32x3 engine has no use for the copy
    with pytest.raises(NotImplementedError):
        m.fused_train_step_rows(data, rows, 1.0, None, do_adam=False, data16=N.to_bf16(data))
    m.gemm_dtype = "bf16"
    m.fused_train_step_rows(data, rows, 1.0, None, do_adam=False, data16=N.to_bf16(data))      # the same draw is still there
    h2 = R.Hyper(input_dim=52, fc_dim=100, n_categories=12, state_dim=2, lowD_dim=6, n_arm=2)   # 52 % 8 != 0
    d2 = R.synthetic_batch(200, 52, seed=1).to(DEV)
    m2 = _rows_model(h2, 2, R.draw_noise(h2, 128, seed=3))
    with pytest.raises(NotImplementedError):
        m2.fused_train_step_rows(d2, rows, 1.0, None, do_adam=False, data16=d2.to(torch.bfloat16))


def test_bf16_storage_at_full_size_against_the_oracle():
    """A = 2, B = D = 5000 on bf16 storage: the loss terms against the fp32 oracle on the UNROUNDED matrix stay inside the
    configuration's 5e-2 gate (the reconstruction loss now compares with the rounded x), gradients agree in direction."""
    import distributed_vae_amd  # noqa: F401
    from distributed_vae_amd import _native as N
    A, B, D = 2, 5000, 5000
    h = R.Hyper(input_dim=D, n_arm=A)
    sd = R.init_state_dict(h, 546)
    x = R.synthetic_batch(B, D, seed=547)
    noise = R.draw_noise(h, B, seed=548)
    m = _rows_model(h, 546, noise)
    data = x.to(DEV)
    buf = m.fused_train_step_rows(data, torch.arange(B, device=DEV), 1.0, None, do_adam=False, data16=N.to_bf16(data)).clone()
    torch.cuda.synchronize()
    _, lt, g_ref = R.grads_autograd({k: v.clone() for k, v in sd.items()}, [x] * A, h, noise)
    want = [float(lt[0]), float(lt[2]), float(lt[3]), float(lt[4]), float(lt[5])] + [float(v) for v in lt[1]]
    got = buf.cpu()[:5 + A].double().tolist()
    errs = [abs(a - b) / (abs(b) + 1e-30) for a, b in zip(got, want)]
    print("bf16 storage vs fp32 oracle, relative error of (total, joint, c_ent, c_dist, c_l2, rec...):", ["%.2e" % e for e in errs])
    assert max(errs[i] for i in (0, 1, 3, 5, 6)) < LOSS_GATE, errs
    worst = 1.0
    for (k, _), gv in zip(m.named_parameters(), m._grad_views):
        ref = g_ref[k].double().flatten()
        v = gv.detach().cpu().double().flatten()
        worst = min(worst, float(torch.dot(v, ref) / (v.norm() * ref.norm() + 1e-300)))
    print("bf16 storage vs fp32 oracle, worst gradient cosine: %.5f" % worst)
    assert worst > 0.9

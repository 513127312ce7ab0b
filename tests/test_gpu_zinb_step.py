"""GPU: training under the ZINB objective -- mmvae_zinb_train_step, mmvae_zinb_objective (csrc/api.hip) and what is built on
them: mixVAE_model.zinb_train_step / zinb_objective, cpl_mixVAE.fit_zinb -- against tests/zinb_step_restatement.py at the
operating points of tests/zinb_step_cases.py, where the ZINB term is the gradient of every encoder and latent tensor (pinned on
the CPU by tests/test_zinb_step_cpu.py).  Nothing here reads the reference.

Gates, none of them derived here:
  * the 28 tensors per arm: tests/test_gpu_loss_terms.py's rule through zinb_step_cases.grad_tolerance -- a tensor's worst entry,
    relative to the tensor's fp64 maximum, below max(GRAD_TOL, 3 x the fp32 restatement's own error in that tensor);
  * the three heads: DESIGN.md section 9m's gate on the device's own d10 -- |value - truth| / M, maximum and 90th percentile,
    within max(3 x float32 autograd's, 2^-23), truth float64 autograd of tests/zinb_grad_restatement.py;
  * the loss vector: gpu_util.assert_loss_vector at LOSS_TOL; rec[a] besides against mmvae_zinb_nll on the step's own d10 to the
    float32 rounding of the output;
  * Adam: torch.optim.Adam on the device's own gradients to 3e-8; the descent: tests/test_gpu_zinb_decoder.py's rtol 1e-4.
Every figure is printed before it is asserted (pytest -s)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import zinb_grad_restatement as RG  # noqa: E402
import zinb_restatement as ZR  # noqa: E402
from tests import golden_util as G  # noqa: E402
from tests import gpu_util as U  # noqa: E402
from tests import term_cases as T  # noqa: E402
from tests import zinb_step_cases as Z  # noqa: E402
from tests.test_gpu_loss_terms import FP32_ENGINES, FWD_TOL, LOSS_TOL  # noqa: E402
from distributed_vae_amd import _native as N  # noqa: E402
from distributed_vae_amd import nn_model as NM  # noqa: E402

pytestmark = pytest.mark.gpu

S = Z.S
DEV = U.DEV
MARGIN, FLOOR = 3.0, 2.0 ** -23
HEADS = (("rec", "fc11"), ("p", "fc11_p"), ("r", "fc11_r"))


def build(h, sd, mode="ZINB", engine="fp32x3", train=True):
    m = NM.mixVAE_model(input_dim=h.input_dim, fc_dim=h.fc_dim, n_categories=h.n_categories, state_dim=h.state_dim,
                        lowD_dim=h.lowD_dim, x_drop=h.x_drop, s_drop=h.s_drop, n_arm=h.n_arm, lam=h.lam, lam_pc=1, tau=h.tau,
                        beta=h.beta, hard=h.hard, variational=True, device=DEV, eps=h.eps, momentum=h.momentum, ref_prior=False,
                        loss_mode=mode)
    m.load_state_dict({k: v for k, v in sd.items() if mode == "ZINB" or not k.startswith(("fc11_p.", "fc11_r."))})
    m = m.to(DEV)
    m.train(train)
    m.gemm_dtype = engine
    return m


def grads_of(m):
    """{key: gradient} of the 28 tensors per arm (the flat gradient buffer's views) and of the p and r heads (their buffer)."""
    out = {k: gv.detach().cpu().clone() for (k, _), gv in zip(m.named_parameters(), m._grad_views) if gv is not None}
    _, hg = m.zinb_heads_flat()
    lay, D, H = m._heads_layout, m.input_dim, m.fc_dim
    for a in range(m.n_arm):
        for j, (name, kind) in enumerate(m._ZINB_PR):
            n = D * H if kind == "weight" else D
            o = int(lay.offset[j])
            out[f"{name}.{a}.{kind}"] = hg[a, o: o + n].view((D, H) if kind == "weight" else (D,)).detach().cpu().clone()
    return out


def step(o, engine, do_adam=False, **kw):
    """One zinb_train_step of a fresh model on the row's inputs and noise -> (model, loss vector on the host, gradients)."""
    h, row = o["h"], o["row"]
    m = build(h, o["sd"], engine=engine)
    m.set_explicit_noise(U.noise_to_device(o["noise"]))
    buf = m.zinb_train_step(o["x"].to(DEV).expand(h.n_arm, -1, -1), row.temp, do_adam=do_adam, **kw).clone()
    torch.cuda.synchronize()
    return m, buf.cpu(), grads_of(m)


def within(name, dev, cpu):
    print(f"    {name:<14} device max {dev[0]:.3e} p90 {dev[1]:.3e} | reference float32 max {cpu[0]:.3e} p90 {cpu[1]:.3e}")
    return dev[0] <= max(MARGIN * cpu[0], FLOOR) and dev[1] <= max(MARGIN * cpu[1], FLOOR)


# ---- 1. one pass over g: mmvae_zinb_step_grads is the two entries it replaces, bit for bit ------------------------------------
@pytest.mark.parametrize("heads", [("rec", "p", "r"), ("p", "r"), ("rec",)])
@pytest.mark.parametrize("n,D,H", [(65, 33, 7), (257, 130, 100), (257, 130, 128)])
def test_single_pass_equals_the_two_entries_bit_for_bit(n, D, H, heads):
    """The chains are the existing kernels': dW, db and the sums as mmvae_zinb_head_grads at the same cell segments, gd10 as
    mmvae_zinb_d10_grad with a segment a gene tile.  The step calls it with all three heads and the library's segment rule (0);
    1 and 2 are forced besides (257 cells are five cell tiles: segments of five, and of three and two)."""
    d10, L, X = RG.inputs(n, D, H)
    d10, X, L = d10.to(DEV), X.to(DEV), [t.to(DEV) for t in L]
    sc = 3.0 / (n * D)
    n_gt = -(-D // 64)
    for segments in (0, 1, 2):
        g1, cell1, gene1, gd1 = N.zinb_step_grads(d10, *L, X, scale=sc, heads=heads, segments=segments)
        g2, cell2, gene2 = N.zinb_head_grads(d10, *L, X, scale=sc, heads=heads, segments=segments)
        gd2 = N.zinb_d10_grad(d10, *L, X, scale=sc, heads=heads, segments=n_gt)
        assert sorted(g1) == sorted(g2) == sorted(heads)
        for h in heads:
            assert torch.equal(g1[h][0], g2[h][0]) and torch.equal(g1[h][1], g2[h][1]), (h, segments)
        assert torch.equal(cell1, cell2) and torch.equal(gene1, gene2) and torch.equal(gd1, gd2), segments
        assert bool(gd1.any()) and bool(torch.isfinite(gd1).all()) and gd1.shape == (n, H)


# ---- 2. the step's gradients and 3. its loss vector against the restatement ---------------------------------------------------
@pytest.mark.parametrize("engine", FP32_ENGINES)
@pytest.mark.parametrize("name", Z.ROW_IDS)
def test_step_gradients_and_loss_at_zinb_exposing_points(name, engine):
    Z.assert_exposes(name)
    o = Z.oracle(name)
    h, A = o["h"], o["h"].n_arm
    B, D, H = o["x"].shape[0], h.input_dim, h.fc_dim
    m, buf, grads = step(o, engine)
    assert bool(torch.isfinite(buf).all()) and all(bool(torch.isfinite(v).all()) for v in grads.values())
    assert set(grads) == set(o["g64"])
    # the forward the step ran: the latent block's outputs and d10
    width = {"x_low": h.lowD_dim, "c": h.n_categories, "s_smp": h.state_dim, "c_smp": h.n_categories, "s_mean": h.state_dim,
             "s_logvar": h.state_dim, "c_prob": h.n_categories}
    from tests.test_gpu_loss_terms import FWD
    for nm, w in width.items():
        err = G.rel_err(U.ws(m, nm, w), torch.stack(list(o["out64"][FWD[nm]])))
        assert err < FWD_TOL, (name, engine, nm, err)
    d10 = U.ws(m, "d10", H)
    assert G.rel_err(d10, torch.stack(o["d10"])) < FWD_TOL
    # the loss vector: total, joint, entropy, distance, L2, rec (ZINB), KL, ll (MSE-based)
    print(f"\n{name} {engine}: loss vector {[float('%.6g' % v) for v in buf.tolist()]}")
    print(f"    restatement total {float(o['lt64'][0]):.6g}, rec {[float('%.6g' % float(v)) for v in o['lt64'][1]]}")
    U.assert_loss_vector(buf, o["lt64"], A, LOSS_TOL)
    scale = max(A - 1, 1) / (float(B) * float(D))
    x = o["x"]
    ok = True
    for a in range(A):
        L = [o["sd"][f"{nm}.{a}.{k}"] for _, nm in HEADS for k in ("weight", "bias")]
        # rec[a] is zinb_loss on the step's own activations, to the rounding of the float32 it is stored in
        cell, _ = N.zinb_nll(d10[a].to(DEV), *(t.to(DEV) for t in L), x.to(DEV))
        want = float(cell.sum()) / (float(B) * float(D))
        got = float(buf[N.LOSS_REC0 + a])
        print(f"    arm {a}: rec {got!r}, zinb_nll on the step's d10 {want!r}")
        assert abs(got - want) <= float(np.spacing(np.float32(abs(want))))
        # the three heads are the existing entry's on the step's own d10 and x, bit for bit (every gene, every head) ...
        alone, _, _ = N.zinb_head_grads(d10[a].to(DEV), *(t.to(DEV) for t in L), x.to(DEV), scale=scale)
        for hd, nm in HEADS:
            for k, kind in enumerate(("weight", "bias")):
                assert torch.equal(alone[hd][k].cpu(), grads[f"{nm}.{a}.{kind}"]), (name, engine, nm, a, kind)
        # ... and within section 9m's gate on that d10
        truth = RG.autograd_heads(d10[a].double(), [t.double() for t in L], x.double(), scale=scale)
        ref = RG.autograd_heads(d10[a], L, x, scale=scale)
        M = RG.head_magnitudes(d10[a], L, x, scale=scale)
        for hd, nm in HEADS:
            for k, kind in enumerate(("weight", "bias")):
                ok &= within(f"{nm}.{a}.{kind[0]}", ZR.error_stat(grads[f"{nm}.{a}.{kind}"], truth[hd][k], M[hd][k]),
                             ZR.error_stat(ref[hd][k], truth[hd][k], M[hd][k]))
    assert ok
    # the 28 tensors per arm against the fp64 restatement of the whole step
    worst = (0.0, None)
    for k, ref in o["g64"].items():
        if k.startswith(("fc11_p.", "fc11_r.")):
            continue
        err, tol = G.rel_err(grads[k], ref), Z.grad_tolerance(name, k)
        if Z.is_pinned(k):
            worst = max(worst, (err / tol, k))
        assert err < tol, (name, engine, k, err, tol, "fp32 restatement: %.2e" % o["e32"][k])
    print(f"    worst encoder / latent gradient at {worst[0]:.2e} of its tolerance ({worst[1]})")
    # the running statistics
    sd = m.state_dict()
    for k, ref in o["bn64"].items():
        if "num_batches" in k:
            assert int(sd[k]) == int(ref), k
        else:
            assert G.rel_err(sd[k].cpu(), ref) < 1e-5, k


def test_objective_in_eval_mode_is_the_restatements():
    """zinb_objective: the eval forward (running statistics, no dropout, the noise-free sample) and the same scalars, with and
    without a category mask."""
    o = Z.oracle("a2_d72_h20_fast_sdrop")
    h, A = o["h"], o["h"].n_arm
    sd64, x64, n64 = T.to64(o["sd"], o["x"], o["noise"])
    for mask in (None, [0, 1, 2, 5, 7, 11]):
        with torch.no_grad():
            out, saved, terms, zl = S.objective_terms(dict(sd64), [x64] * A, h, n64, training=False, eval_flag=True, mask=mask)
            want = S.loss_tuple(out, [x64] * A, h, terms, zl)
            o32, _, t32, z32 = S.objective_terms(dict(o["sd"]), [o["x"]] * A, h, o["noise"], training=False, eval_flag=True, mask=mask)
            ref = S.loss_tuple(o32, [o["x"]] * A, h, t32, z32)
        m = build(h, o["sd"], train=False)
        m.set_explicit_noise(U.noise_to_device(o["noise"]))
        got = m.zinb_objective(o["x"].to(DEV).expand(A, -1, -1), o["row"].temp, mask=mask)
        vec = torch.stack([got[0], got[2], got[3], got[4], got[5], *got[1], *got[6], *got[8]]).cpu()
        print(f"\nmask {mask}: objective {[float('%.6g' % v) for v in vec.tolist()]}, restatement total {float(want[0]):.6g}")
        assert got[7] == [] and got[1].shape == (A,)
        # total, joint, rec, KL and ll at gpu_util.assert_loss_vector's tolerances.  The three means of the coupling (entropy,
        # distance, L2), which the objective carries at lam = 1e-13, at max(that tolerance, 3 x the float32 restatement's own
        # error): tau = 10 flattens c, its batch variances fall to 1e-8 and the distance's inverse standard deviations turn
        # float32 rounding of c into 1e-5 of the mean (the float32 restatement is printed beside the device).
        side = {2: 1e-4, 3: LOSS_TOL, 4: 1e-4}
        pos = {2: 3, 3: 4, 4: 5}
        for i, tol in side.items():
            w64, w32, g_ = float(want[pos[i]]), float(ref[pos[i]]), float(vec[i])
            print(f"    entry {i}: device {g_!r}, float64 {w64!r}, float32 restatement {w32!r}")
            assert abs(g_ - w64) <= max(tol * abs(w64), 3.0 * abs(w32 - w64)) + 1e-7
            vec[i] = w64
        U.assert_loss_vector(vec, want, A, LOSS_TOL)
        with pytest.raises(NotImplementedError, match="zinb_nll"):         # loss() itself stays refused
            m.loss([0] * A, [], [], None, [0] * A, [0] * A, [0] * A, [0] * A)


# ---- 4. Adam, and the BatchNorm buffers -------------------------------------------------------------------------------------
@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("name", ["a2_d70_h20", "a3_d132_h100_fast"])
def test_adam_step_is_torch_adam_on_the_device_gradients(name, wd):
    o = Z.oracle(name)
    _, buf0, g = step(o, "fp32x3")
    ref = {k: o["sd"][k].clone().requires_grad_() for k in g}
    for k, p in ref.items():
        p.grad = g[k].clone()
    torch.optim.Adam(list(ref.values()), lr=1e-3, weight_decay=wd).step()
    m, buf1, g1 = step(o, "fp32x3", do_adam=True, lr=1e-3, weight_decay=wd)
    assert torch.equal(buf0, buf1) and all(torch.equal(g[k], g1[k]) for k in g)       # the same step, then the update
    sd = m.state_dict()
    worst = max(float((sd[k].cpu() - ref[k].detach()).abs().max()) for k in g)
    moved = min(float((sd[k].cpu() - o["sd"][k]).abs().max()) for k in g)
    print(f"\n{name}, weight_decay {wd}: largest difference from torch's Adam {worst:.3e}; every tensor moved by at least {moved:.3e}")
    assert worst <= 3e-8 and moved > 1e-4
    assert m._zinb_state["step"] == 1
    # the alignment gaps of the flat buffer hold their zeros
    flat, lay = m.flat_parameters(), m._layout
    used = torch.zeros_like(flat, dtype=torch.bool)
    for a in range(m.n_arm):
        for t in range(N.N_PARAM_TENSORS):
            o_ = a * int(lay.per_arm) + int(lay.offset[t])
            used[o_: o_ + m._param_of(t, a).numel()] = True
    assert not bool(flat[~used].any())


@pytest.mark.parametrize("engine", FP32_ENGINES)
@pytest.mark.parametrize("name", ["a2_d70_h20", "a2_d72_h20_fast_sdrop"])
def test_batchnorm_buffers_are_the_mse_steps_bit_for_bit(name, engine):
    o = Z.oracle(name)
    h = o["h"]
    m, _, _ = step(o, engine)
    mse = build(h, o["sd"], mode="MSE", engine=engine)
    mse.set_explicit_noise(U.noise_to_device(o["noise"]))
    mse.fused_train_step(o["x"].to(DEV).expand(h.n_arm, -1, -1), o["row"].temp, None, do_adam=False)
    torch.cuda.synchronize()
    assert torch.equal(m._bn_flat, mse._bn_flat) and torch.equal(m._nbt, mse._nbt)
    assert bool(m._nbt.any())


# ---- 5. determinism, fit_zinb -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", FP32_ENGINES)
def test_two_runs_are_bit_identical(engine):
    o = Z.oracle("a3_d130_h100_hard_sdrop")
    (_, b1, g1), (_, b2, g2) = step(o, engine), step(o, engine)
    assert torch.equal(b1, b2) and all(torch.equal(g1[k], g2[k]) for k in g1)
    o = Z.oracle("a3_d132_h100_fast")
    (m1, b1, _), (m2, b2, _) = step(o, engine, do_adam=True, lr=1e-2), step(o, engine, do_adam=True, lr=1e-2)
    s1, s2 = m1.state_dict(), m2.state_dict()
    assert torch.equal(b1, b2) and all(torch.equal(s1[k], s2[k]) for k in s1)


A_, DM, HF, CC, SS, LD, N_ALL, N_CELLS, BATCH = 2, 70, 20, 5, 2, 6, 80, 60, 21


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
    return data, index


def loader(lo=0, hi=N_CELLS, batch=BATCH):
    from distributed_vae_amd.utils.dataloader import DeviceLoader
    data, index = cells()
    return DeviceLoader(data, index[lo:hi], batch, False, False)


def bits(m):
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def test_fit_zinb_resumes_bit_for_bit_and_leaves_other_models_alone():
    """2 + 2 epochs equal 4 (in-kernel Philox noise: the model's own seed and offset carry on across the calls); every layer
    moves; the validation loss is zinb_objective's; a second, MSE, model on the same device is untouched."""
    other = trainer(seed=7, mode="MSE")
    other_bits, other_flat = bits(other.model), other.model.flat_parameters().clone()
    t4, t22 = trainer(), trainer()
    t22.model.load_state_dict(bits(t4.model))
    before = bits(t4.model)
    for t in (t4, t22):
        t.model._noise_seed, t.model._noise_offset = 1234, 0
    r4 = t4.fit_zinb(loader(), 4, lr=1e-2, test_loader=loader(batch=64), weight_decay=0.01)
    r2 = t22.fit_zinb(loader(), 2, lr=1e-2, test_loader=loader(batch=64), weight_decay=0.01)
    r22 = t22.fit_zinb(loader(), 2, lr=1e-2, test_loader=loader(batch=64), weight_decay=0.01, state=r2["state"])
    n_loss = 5 + 3 * A_
    assert r4["train_loss"].shape == r4["val_loss"].shape == (4, n_loss) and np.all(np.isfinite(r4["train_loss"]))
    assert r2["state"]["step"] == 6 and r22["state"]["step"] == r4["state"]["step"] == 12
    assert np.array_equal(np.concatenate([r2["train_loss"], r22["train_loss"]]), r4["train_loss"])
    assert np.array_equal(np.concatenate([r2["val_loss"], r22["val_loss"]]), r4["val_loss"])
    for k in ("exp_avg", "exp_avg_sq", "hp_exp_avg", "hp_exp_avg_sq"):
        assert torch.equal(r22["state"][k], r4["state"][k]) and bool(r4["state"][k].any())
    sd4, sd22 = bits(t4.model), bits(t22.model)
    assert all(torch.equal(sd4[k], sd22[k]) for k in sd4)
    assert all(not torch.equal(before[k], sd4[k]) for k in before if not k.startswith("batch_s.")), "every tensor is trained"
    assert t4.model.training
    # the second model
    assert all(torch.equal(other_bits[k], v) for k, v in bits(other.model).items())
    assert torch.equal(other_flat, other.model.flat_parameters())
    # mode restored; a state of the decoder fit is refused
    t4.model.eval()
    t4.fit_zinb(loader(0, BATCH), 0)
    assert not t4.model.training
    with pytest.raises(ValueError, match="state"):
        t4.fit_zinb(loader(), 1, state=t4.fit_zinb_decoder(loader(), 0)["state"])
    with pytest.raises(ValueError, match="state"):
        t4.fit_zinb(loader(), 1, state=t4.fit_zinb_heads(loader(), 0)["state"])


# ---- 6. descent -------------------------------------------------------------------------------------------------------------
DESCENT = dict(steps=20, lr=1e-3)


@functools.lru_cache(maxsize=None)
def descent_case():
    """The first row's shape and hyper-parameters on counts up to 50, one noise draw held fixed over the steps (the objective is
    then one function of the parameters); the float64 restatement's totals before each step."""
    row = Z.BY_NAME["a2_d70_h20"]
    h, sd, _, noise = Z.inputs(row)
    x = ZR.counts_matrix(row.B, row.D, torch.Generator().manual_seed(5), max_count=50)
    return row, h, sd, x, noise, S.adam_losses(sd, x, h, [noise] * DESCENT["steps"], lr=DESCENT["lr"])


def test_twenty_steps_descend_as_the_restatement_does():
    row, h, sd, x, noise, want = descent_case()
    assert np.all(np.diff(want) < -1e-6), want                             # the restatement falls at every step
    m = build(h, sd)
    m.set_explicit_noise(U.noise_to_device(noise))                         # a dict, not a schedule: every step takes it
    xs = x.to(DEV).expand(h.n_arm, -1, -1)
    got = [float(m.zinb_train_step(xs, row.temp, lr=DESCENT["lr"])[N.LOSS_TOTAL]) for _ in range(DESCENT["steps"])]
    print(f"\n  total {got[0]:.6f} -> {got[-1]:.6f}; restatement {want[0]:.6f} -> {want[-1]:.6f}")
    assert np.all(np.diff(got) < 0), got
    assert np.allclose(got, want, rtol=1e-4, atol=0)


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_on_the_device():
    o = Z.oracle("a2_d70_h20")
    h, A = o["h"], o["h"].n_arm
    x = o["x"].to(DEV).expand(A, -1, -1)
    m = build(h, o["sd"])
    before, step_id, offset = bits(m), m._step_id, m._noise_offset
    with pytest.raises(RuntimeError, match=r"needs model\.train\(\)"):
        m.eval().zinb_train_step(x, 1.0)
    m.train()
    with pytest.raises(RuntimeError, match=r"needs model\.eval\(\)"):
        m.zinb_objective(x, 1.0)
    m.gemm_dtype = "bf16"
    with pytest.raises(NotImplementedError, match="bf16"):
        m.zinb_train_step(x, 1.0)
    m.gemm_dtype = "fp32x3"
    with pytest.raises(RuntimeError, match="loss_mode='ZINB'"):
        build(h, o["sd"], mode="MSE").zinb_train_step(x, 1.0)
    assert m._step_id == step_id and m._noise_offset == offset
    # the library's own refusals, before any launch: a category mask, the bf16 engine, eval mode, a short zws
    eng = m._ensure(x.shape[1])
    hp, hg = m.zinb_heads_flat()
    xt, xs = m._prep_x(x)
    args = lambda hy: (hy, N.make_noise(None, 1, 1), m._flat, hp, m._bn_flat, m._nbt, xt, xs, m._flat_grad, hg, False, None, None,
                       None, None, 1, 0.0)
    hy = m._hyper(1.0, False)
    hy.cat_mask[0] = 0b1011
    with pytest.raises(NotImplementedError, match="category mask"):
        eng.zinb_train_step(*args(hy))
    hy = m._hyper(1.0, False)
    hy.gemm_bf16 = 1
    with pytest.raises(NotImplementedError, match="bf16"):
        eng.zinb_train_step(*args(hy))
    hy = m._hyper(1.0, False)
    hy.training = 0
    with pytest.raises(NotImplementedError, match="training mode"):
        eng.zinb_train_step(*args(hy))
    eng._zws()
    full = eng.zws_bytes
    eng.zws_bytes = full - 8
    with pytest.raises(N.NativeError, match="zws too small"):
        eng.zinb_train_step(*args(m._hyper(1.0, False)))
    eng.zws_bytes = full
    torch.cuda.synchronize()
    after = bits(m)
    assert all(torch.equal(before[k], after[k]) for k in before) and not bool(m._flat_grad.any())


def test_the_pinned_refusals_still_hold():
    """What stays refused beside the new names: zinb_loss has no backward, the MSE entry points do not train a ZINB model, the
    training-mode forward and loss() stay refused."""
    t = trainer()
    h = torch.rand(4, DM, device=DEV)
    with pytest.raises(NotImplementedError, match="no backward"):
        NM.zinb_loss(h.clone().requires_grad_(), h, h, h)
    with pytest.raises(NotImplementedError, match="training under loss_mode='ZINB' is not built"):
        t.model.fused_train_step(h.expand(A_, -1, -1), 1.0, None, do_adam=False)
    with pytest.raises(NotImplementedError, match="training under loss_mode='ZINB' is not built"):
        t.model.fused_train_step_rows(h, torch.arange(4, device=DEV), 1.0, None, do_adam=False)
    with pytest.raises(NotImplementedError, match="training under loss_mode='ZINB' is not built"):
        t._step(h.expand(A_, -1, -1))
    with pytest.raises(AssertionError, match="ZINB not implemented"):
        t.model.train()(h.expand(A_, -1, -1), 1.0)
    with pytest.raises(NotImplementedError, match="zinb_nll"):
        t.model.loss([h] * A_, [], [], None, [h] * A_, [h] * A_, [h] * A_, [h] * A_)

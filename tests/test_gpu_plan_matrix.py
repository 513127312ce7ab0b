"""-m gpu: every row of tests/plan_cases.py on every GEMM engine -- first the plan read-back (a row that drifts off its kernel
path fails here, whatever its numbers), then the numbers of that path:

  * the fused step (no Adam, explicit noise) against the oracle at the project's existing gates: fp32-grade plans (engines
    fp32_mfma and fp32x3, and the bf16 engine where its plan falls to the fp32 kernels) hold the loss vector to 1e-5 (1e-4 on
    the entropy / L2 / KL terms) of the fp64 oracle and every gradient to tests/gpu_util.py::assert_gradients_tight on the
    device's own ReLU decisions; the bf16 tiles reproduce their five products from the operands in the workspace (2e-5) and
    keep the loss within 5e-2 of the fp32 oracle;
  * general-path and misaligned rows: fused step == forward / loss / backward on the same inputs (loss 1e-6, gradients 1e-5),
    and a misaligned run == the aligned run of the same shape to the same bounds where both runs took the same hidden ReLU
    decisions (else the rule of test_full_size_properties).  On the bf16 engine the two runs are different arithmetic -- the
    aligned one multiplies bf16-rounded operands, the general kernels fp32 ones -- so each is held to its own gate: the
    misaligned run to the fp32 gates, the aligned run's five products to 2e-5, their losses to 5e-2 of each other;
  * two Adam steps bit-reproducible run to run (engines bf16, fp32x3), the row-indexed step bit-identical to gather-then-step
    where the plan says `rowmap` and refused where it does not (the misaligned rows are left out here: this runs through the
    model's own step, which cannot be handed a misaligned pointer, and aligned they are row h100); the same identity on
    ragged tiles of a matrix whose pitch is not its width, fp32x3 and bf16, the latter also on the bf16 copy;
  * a NaN-filled workspace changes no bit on the plans with planes written and unread or not written at all;
  * decode / state_changes across the fc11 switch points (x_rec at the gates of tests/test_gpu_decode.py, decoder(forward's
    codes) bit-equal to the forward's x_rec on engine 0);
  * the eval-mode forward and eval_classify on the width and latent rows against the fp64 oracle: labels equal but for at
    most plan_cases.EVAL_LABEL_CAP cells, the forward's outputs at the gates of test_golden_eval_forward.

The engines here have their side stream; tests/test_gpu_noside.py runs the rows plan_cases.NOSIDE_GPU on engines without
one, through this module's helpers (`side=False`).

The engines are driven through _native.Engine directly (as tests/test_gpu_batchsums.py does): the Python boundary cannot hand
the library a misaligned pointer.
"""
import pytest
import torch

from oracle import restatement as R
from tests import golden_util as G
from tests import plan_cases as P

pytestmark = pytest.mark.gpu

LOSS_TOL, GRAD_TOL = 1e-5, 1e-3
ENGINE_TOL, LOSS_GATE = 2e-5, 5e-2        # tests/test_gpu_bf16.py
ENGINES = list(P.ENGINES)
ROW_IDS = [r.name for r in P.GPU_ROWS]


def _no_side_stream(monkeypatch):
    """The switch of the Python layer that builds engines without a side stream (_native.Engine reads it when it is built)."""
    monkeypatch.setenv("MMVAE_SIDE_STREAM", "0")


def _env(row, engine, seed=546, side=True, monkeypatch=None):
    """side=False: the engine is built under MMVAE_SIDE_STREAM=0, set through pytest's `monkeypatch` (the test's fixture; a
    caller without one -- a result shared between tests -- gets a context of its own, undone once the engine exists)."""
    from tests import gpu_util as U
    h = R.Hyper(input_dim=row.D, fc_dim=row.H, n_categories=row.C, state_dim=row.S, lowD_dim=row.L, x_drop=row.x_drop,
                s_drop=row.s_drop, n_arm=row.A, hard=row.hard)
    sd = R.init_state_dict(h, seed)
    x = R.synthetic_batch(row.B, row.D, seed=3)
    noise = R.draw_noise(h, row.B, seed=5)
    m = U.build_model(h, sd)
    m.train()
    m.gemm_dtype = engine
    if side:
        eng = m._ensure(row.B)
        assert eng.side is not None, "the matrix pins the plans of an engine with its side stream"
    else:
        with (pytest.MonkeyPatch.context() if monkeypatch is None else monkeypatch.context()) as mp:
            _no_side_stream(mp)
            eng = m._ensure(row.B)
        assert eng.side is None and not eng.ex.side_stream, "MMVAE_SIDE_STREAM=0 builds an engine without a side stream"
    return U, h, sd, x, noise, m, eng


def _place(m, x, misalign):
    """(params, x, arm stride) on the device as the row asks: views one float into their storage, or an odd arm stride."""
    from tests import gpu_util as U
    xd, params, xs = x.to(U.DEV), m._flat, 0
    A, n = m.n_arm, x.numel()
    if misalign == "x_off1":
        st = torch.zeros(n + 1, device=U.DEV)
        st[1:].copy_(xd.flatten())
        xd = st[1:].view_as(x)
    elif misalign == "p_off1":
        st = torch.zeros(m._flat.numel() + 1, device=U.DEV)
        st[1:].copy_(m._flat)
        params = st[1:]
    elif misalign == "xs_odd":
        st = torch.zeros(A * (n + 1), device=U.DEV)
        for a in range(A):
            st[a * (n + 1): a * (n + 1) + n].copy_(xd.flatten())
        xd, xs = st, n + 1
    if misalign in ("x_off1", "p_off1"):
        assert (params.data_ptr() if misalign == "p_off1" else xd.data_ptr()) % 16 == 4
    return params, xd, xs


def _assert_plan(row, engine, eng, hyper, params, xd, xs, kind="STEP", fields=None, side=True):
    """The live engine's plan for `kind` (a kind of plan_cases.KINDS) equals the table's; `fields`: only these (an engine
    whose A or B differ from the row's, as decode's); side=False: an engine without a side stream, held to
    plan_cases.without_side() of the table's plan."""
    from distributed_vae_amd import _native as N
    got = N.debug_plan(eng.dims, hyper, eng.ex, {"FORWARD_XREC": "FORWARD"}.get(kind, kind),
                       params_align=params.data_ptr() % 16 or 16, x_align=xd.data_ptr() % 16 or 16, x_arm_stride=xs,
                       fc11_grad=kind != "FORWARD_XREC")
    want = P.expected(row, engine, kind)
    if not side:
        assert not eng.ex.side_stream
        want = P.without_side(want)
    if not hyper.training:
        want["zero"] = "ZERO_NONE"                       # eval mode: nothing accumulates, no head fill
    if not fields:
        i_gd10, i_dw11 = P.slab_sources(want)
        sp = eng.splits()
        want["gd10_slabs"], want["dw11_slabs"] = sp[i_gd10], sp[i_dw11]
    diff = {k: (got[k], want[k]) for k in (fields or N.PLAN_NAMES) if got[k] != want[k]}
    assert not diff, (row.name, engine, kind, "got, want:", diff)
    lit = P.slabs_of(row.name, engine)
    if lit and kind == "STEP" and not fields:
        assert (got["gd10_slabs"], got["dw11_slabs"]) == lit, (row.name, engine, got["gd10_slabs"], got["dw11_slabs"], lit)
    return got


def _noise(noise_dev):
    """The call's mmvae_noise: explicit buffers (a dict of device tensors), or a ready one (the Philox mode of
    tests/test_gpu_noise.py)."""
    from distributed_vae_amd import _native as N
    return noise_dev if isinstance(noise_dev, N.Noise) else N.make_noise(noise_dev)


def _fused(m, eng, noise_dev, params, xd, xs, state0):
    m._bn_flat.copy_(state0[0])
    m._nbt.copy_(state0[1])
    g = torch.zeros_like(m._flat_grad)
    buf = eng.train_step(m._hyper(1.0, False), _noise(noise_dev), params, m._bn_flat, m._nbt, xd, xs, g, False, None, None, 1,
                         0.0).clone()
    torch.cuda.synchronize()
    return buf, g


def _api(m, eng, noise_dev, params, xd, xs, state0):
    m._bn_flat.copy_(state0[0])
    m._nbt.copy_(state0[1])
    hyper, nz = m._hyper(1.0, False), _noise(noise_dev)
    g = torch.zeros_like(m._flat_grad)
    eng.forward(hyper, nz, params, m._bn_flat, m._nbt, xd, xs, None, True)
    buf = eng.loss(hyper).clone()
    eng.backward(hyper, nz, params, xd, xs, g)
    torch.cuda.synchronize()
    return buf, g


def _named(m, g):
    """{parameter name: its gradient} from a flat gradient buffer laid out like the model's own."""
    base = m._flat_grad.data_ptr()
    out = {}
    for (k, _), gv in zip(m.named_parameters(), m._grad_views):
        o = (gv.data_ptr() - base) // 4
        out[k] = g[o: o + gv.numel()].view(gv.shape).cpu().clone()
    return out


def _same_to_api_gates(a, b, what):
    (la, ga), (lb, gb) = a, b
    assert float((la - lb).abs().max()) <= 1e-6 * float(lb.abs().max()), what
    for k in ga:
        sc = float(gb[k].abs().max())
        if sc > 0:
            assert G.rel_err(ga[k], gb[k]) < 1e-5, (what, k)
        else:
            assert float(ga[k].abs().max()) == 0.0, (what, k)


def _plan_then_fused_step_against_oracle(name, engine, side=True, monkeypatch=None):
    """The row's plan on the live engine, then its fused step (no Adam, explicit noise) against the oracle, at the gates the
    module's docstring names.  side=False: the same on an engine without a side stream (tests/test_gpu_noside.py)."""
    row = P.BY_NAME[name]
    U, h, sd, x, noise, m, eng = _env(row, engine, side=side, monkeypatch=monkeypatch)
    A = row.A
    noise_dev = U.noise_to_device(noise)
    params, xd, xs = _place(m, x, row.misalign)
    plan = _assert_plan(row, engine, eng, m._hyper(1.0, False), params, xd, xs, side=side)
    state0 = (m._bn_flat.clone(), m._nbt.clone())
    buf, g = _fused(m, eng, noise_dev, params, xd, xs, state0)
    assert bool(torch.isfinite(buf).all()) and bool(torch.isfinite(g).all())
    grads = _named(m, g)
    if plan["big"] == "GEMM_BF16":
        # the bf16 configuration: its five products exactly, the loss at the configuration's gate
        U.assert_five_bf16_products(eng, grads, sd, x, noise, h, ENGINE_TOL)
        _, lt, _ = R.grads_autograd({k: v.clone() for k, v in sd.items()}, [x] * A, h, noise)
        rel = abs(float(buf[0]) - float(lt[0])) / abs(float(lt[0]))
        print(f"{name} {engine}: loss {float(buf[0]):.6e} oracle {float(lt[0]):.6e} rel {rel:.2e}")
        assert rel <= LOSS_GATE
        rec = torch.stack([v.detach() for v in lt[1]]) if not torch.is_tensor(lt[1]) else lt[1].detach()
        assert G.rel_err(buf[5:5 + A].cpu(), rec) < LOSS_GATE
        return
    # fp32-grade plans: the fp64 oracle on the device's ReLU decisions, the fp32 CPU oracle as the noise floor
    fo = U.flip_aware_oracle(h, sd, x, noise, U.device_relu_patterns(eng, h), verbose=False)
    # (B == 2: the TOTAL at 5e-5, the figure tests/test_gpu_parity.py::test_vs_oracle_edge_shapes holds a two-cell total to;
    # every other entry at the usual gates)
    U.assert_loss_vector(buf.cpu(), fo["lt_64"], A, LOSS_TOL, total_tol=5e-5 if row.B == 2 else None)
    gmax = max(float(v.abs().max()) for v in fo["g_64"].values())
    live = {}
    for k, v in grads.items():
        if float(fo["g_64"][k].abs().max()) < 1e-6 * gmax:
            # (B = 2: BatchNorm of two rows is +-1 and its backward cancels exactly; the oracle has only rounding noise
            # upstream of it.  "Negligible", not "equal noise": tests/test_gpu_parity.py::test_vs_oracle_edge_shapes)
            assert float(v.abs().max()) < 1e-5 * gmax, k
        else:
            live[k] = v
    assert live
    if row.B == 2:
        # Two rows: every BatchNorm output is +-1 (or 0 where a unit is dead in both), its backward cancels exactly, and what
        # is left upstream of the last BatchNorm is rounding noise amplified by 1 / sqrt(var + eps) -- in the fp32 CPU oracle
        # as on the device (plan_cases.FP32_FLOOR records the oracle's own distance from fp64 on this row).  Such a tensor's
        # worst entry is held to 3 x the fp32 oracle's worst (the ratio assert_gradients_tight uses), the others to the gate.
        noisy, floor = {}, 0.0
        for k in list(live):
            ref = fo["g_64"][k]
            sc = float(ref.abs().max()) + 1e-30
            e_cpu = float((fo["g_32"][k].double() - ref).abs().max()) / sc
            e_gpu = float((live[k].double() - ref).abs().max()) / sc
            print(f"b2 {engine} {k}: scale/gmax {sc / gmax:.1e} fp32 oracle {e_cpu:.2e} device {e_gpu:.2e}")
            if e_cpu > GRAD_TOL:
                noisy[k] = e_gpu
                floor = max(floor, e_cpu)
                del live[k]
        # the row's floor: the fp32 oracle's worst distance from fp64 over these tensors (they are one phenomenon, and which of
        # them draws the worst entry is chance); it must be the one plan_cases.py records, to a factor of two
        assert noisy and 0.5 * P.FP32_FLOOR["b2"] <= floor <= 2.0 * P.FP32_FLOOR["b2"], floor
        for k, e_gpu in noisy.items():
            assert e_gpu < 3.0 * floor, (k, e_gpu, floor)
    U.assert_gradients_tight(live, fo, GRAD_TOL)


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("name", ROW_IDS)
def test_plan_then_fused_step_against_oracle(name, engine):
    _plan_then_fused_step_against_oracle(name, engine)


GENERAL = [r.name for r in P.GPU_ROWS if not P.STEP[r.name]["fp32_mfma"]["fast"]]


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("name", GENERAL)
def test_general_path_fused_step_matches_api_path(name, engine):
    """`fast == false` under the fused step (coupling on the side stream, loss finalised on the main one, dW11 not forked,
    dw11_slabs = ks_dw) against forward / loss / backward; a misaligned run against the aligned run of its shape."""
    row = P.BY_NAME[name]
    assert GENERAL == ["h102", "d522", "x_off1", "p_off1", "xs_odd"]
    U, h, sd, x, noise, m, eng = _env(row, engine)
    noise_dev = U.noise_to_device(noise)
    params, xd, xs = _place(m, x, row.misalign)
    hyper = m._hyper(1.0, False)
    _assert_plan(row, engine, eng, hyper, params, xd, xs, "STEP")
    _assert_plan(row, engine, eng, hyper, params, xd, xs, "FORWARD")
    _assert_plan(row, engine, eng, hyper, params, xd, xs, "BACKWARD")
    state0 = (m._bn_flat.clone(), m._nbt.clone())
    lf, gf = _fused(m, eng, noise_dev, params, xd, xs, state0)
    la, ga = _api(m, eng, noise_dev, params, xd, xs, state0)
    fused, api = (lf.cpu(), _named(m, gf)), (la.cpu(), _named(m, ga))
    _same_to_api_gates(fused, api, "fused vs api")
    if row.misalign:
        # the aligned run of the same shape takes the fast path (row h100): other kernels, the same numbers
        p0, x0, xs0 = _place(m, x, None)
        plan0 = _assert_plan(P.BY_NAME["h100"], engine, eng, hyper, p0, x0, xs0)
        assert plan0["fast"]
        l0, g0 = _fused(m, eng, noise_dev, p0, x0, xs0, state0)
        if engine == "bf16":
            # The aligned run multiplies bf16-rounded operands, the general kernels fp32 ones: two different computations, 1e-5
            # between them is not to be had.  Each is held to its own gate instead: the misaligned run to the fp32 oracle gates
            # (test_plan_then_fused_step_against_oracle, its plan being fp32 kernels), the aligned run's five products --
            # gradients of fc1 and fc11 included -- to the bf16 engine's 2e-5 from the operands in the workspace, and the
            # two losses to the configuration's 5e-2 of each other.
            assert plan0["big"] == "GEMM_BF16"
            U.assert_five_bf16_products(eng, _named(m, g0), sd, x, noise, h, ENGINE_TOL)
            assert float((l0 - lf).abs().max()) <= LOSS_GATE * float(lf.abs().max())
            cos = []
            for k, v in _named(m, g0).items():
                ref = fused[1][k].double().flatten()
                if float(ref.norm()) > 0:
                    cos.append(float(torch.dot(v.double().flatten(), ref) / (v.double().norm() * ref.norm() + 1e-300)))
            print(f"{name} bf16: aligned vs misaligned gradient cosines min {min(cos):.4f} median {sorted(cos)[len(cos) // 2]:.4f}")
            # (the bound of test_bf16_configuration_against_the_reference_fixtures for soft samples)
            assert min(cos) > 0.9 and sorted(cos)[len(cos) // 2] > 0.99, (min(cos), sorted(cos)[len(cos) // 2])
        else:
            # Summation-order noise only.  A pre-activation within fp32 rounding of zero may be decided differently by other
            # kernels, and one differing hidden decision moves a row of the weight gradients below it (measured on fp32x3:
            # one decision of r2 differs, fc1.weight by 5e-3 of its scale).  The rule of test_full_size_properties: the same
            # hidden decisions everywhere -> the tight bounds; otherwise at most 8 differ, each at a pre-activation within
            # rounding of zero, and the aligned run is held to the oracle gate on its own decisions (the misaligned run is, in
            # test_plan_then_fused_step_against_oracle).
            p0_pat = U.device_relu_patterns(eng, h)
            _fused(m, eng, noise_dev, params, xd, xs, state0)
            p1_pat = U.device_relu_patterns(eng, h)
            k_diff = sum(int((p0_pat[s_] != p1_pat[s_]).sum()) for s_ in U.HIDDEN_SITES)
            print(f"{name} {engine}: hidden ReLU decisions differing between the aligned and the misaligned run: {k_diff}")
            assert k_diff <= 8
            assert float((l0 - lf).abs().max()) <= 1e-6 * float(lf.abs().max())
            if k_diff == 0:
                _same_to_api_gates(fused, (l0.cpu(), _named(m, g0)), "misaligned vs aligned")
            else:
                fo = U.flip_aware_oracle(h, sd, x, noise, p0_pat, verbose=False)
                U.assert_gradients_tight(_named(m, g0), fo, GRAD_TOL)


def _two_adam_steps(row, engine, h, sd, data, rows, indexed, side=True, weight_decay=0.0, decoupled=False):
    """Two fused Adam steps on explicit noise: [loss vectors, parameters, gradients, running statistics, exp_avg, exp_avg_sq].
    side=False: on an engine without a side stream (one k_reduce launch with the update fused in over all tensors, not the
    fc11 tensors' on the side stream and the rest's on the main one)."""
    from tests import gpu_util as U
    from distributed_vae_amd.cpl_mixvae import FusedAdam
    m = U.build_model(h, sd)
    m.train()
    m.gemm_dtype = engine
    with pytest.MonkeyPatch.context() as mp:
        if not side:
            _no_side_stream(mp)
        eng = m._ensure(row.B)
    assert (eng.side is not None) == side and bool(eng.ex.side_stream) == side
    opt = FusedAdam(m, lr=1e-3, weight_decay=weight_decay, decoupled=decoupled)
    bufs = []
    for s in range(2):
        m.set_explicit_noise(U.noise_to_device(R.draw_noise(h, row.B, seed=40 + s)))
        r = torch.roll(rows, s).to(U.DEV)
        if indexed:
            bufs.append(m.fused_train_step_rows(data, r, 1.0, opt, do_adam=True).clone())
        else:
            bufs.append(m.fused_train_step(data[r].contiguous().expand(row.A, -1, -1), 1.0, opt, do_adam=True).clone())
    torch.cuda.synchronize()
    assert m._engine is eng and opt.step_count == 2
    return [torch.stack(bufs).cpu(), m.flat_parameters().detach().cpu().clone(), m._flat_grad.detach().cpu().clone(),
            m._bn_flat.detach().cpu().clone(), opt.exp_avg.detach().cpu().clone(), opt.exp_avg_sq.detach().cpu().clone()]


@pytest.mark.parametrize("engine", ["bf16", "fp32x3"])
@pytest.mark.parametrize("name", [r.name for r in P.GPU_ROWS if not r.misalign])
def test_two_adam_steps_reproduce_bit_for_bit_and_rows_equal_gather(name, engine):
    from tests import gpu_util as U
    row = P.BY_NAME[name]
    h = R.Hyper(input_dim=row.D, fc_dim=row.H, n_categories=row.C, state_dim=row.S, lowD_dim=row.L, x_drop=row.x_drop,
                s_drop=row.s_drop, n_arm=row.A, hard=row.hard)
    sd = R.init_state_dict(h, 31)
    n_rows = 3 * row.B + 5
    data = R.synthetic_batch(n_rows, row.D, seed=32).to(U.DEV)
    rows = torch.randint(0, n_rows, (row.B,), generator=torch.Generator().manual_seed(33))
    rows[:2] = torch.tensor([n_rows - 1, 0])
    a = _two_adam_steps(row, engine, h, sd, data, rows, False)
    b = _two_adam_steps(row, engine, h, sd, data, rows, False)
    assert bool(torch.isfinite(a[0]).all()) and bool(torch.isfinite(a[1]).all())
    for u, v in zip(a, b):
        assert torch.equal(u.view(torch.int32), v.view(torch.int32)), "run to run"
    if P.expected(row, engine, "STEP_ROWS")["rowmap"]:
        c = _two_adam_steps(row, engine, h, sd, data, rows, True)
        for u, v in zip(a, c):
            assert torch.equal(u.view(torch.int32), v.view(torch.int32)), "rows vs gather"
    else:
        # no row map in this plan (no input dropout, no head launch, a width past the fused fc11 kernels): refused, as today
        with pytest.raises(NotImplementedError):
            _two_adam_steps(row, engine, h, sd, data, rows, True)


@pytest.mark.parametrize("config", ["fp32x3", "bf16", "bf16_data16"])
def test_rows_equal_gather_on_ragged_tiles_of_a_pitched_matrix(config):
    """The row-mapped loaders of fc1 and dW1 (and, with the bf16 copy, the bf16-source ones of fc1, fc11, dW1 and dW11) at the
    smallest shape where they can go wrong: 129 cells (two 128-row tiles, the second ragged), 136 genes (two 128-gene tiles,
    the second ragged; a multiple of 8, as bf16 storage needs), a resident matrix of 400 rows whose pitch (144) is not its
    width.  The row-indexed step equals gather + step bit for bit: loss vector, gradients, BatchNorm statistics.  The matrix
    holds bf16-representable values, so reading its bf16 copy moves other bytes and computes the same numbers."""
    import distributed_vae_amd  # noqa: F401
    from distributed_vae_amd import _native as N
    from tests import gpu_util as U
    A, B, D, H, n_rows, ld = 2, 129, 136, 100, 400, 144
    h = R.Hyper(input_dim=D, fc_dim=H, n_categories=12, state_dim=2, lowD_dim=6, n_arm=A)
    sd = R.init_state_dict(h, 31)
    base = torch.zeros(n_rows, ld)
    base[:, :D] = R.synthetic_batch(n_rows, D, seed=32).to(torch.bfloat16).float()
    data = base.to(U.DEV)[:, :D]
    data16 = N.to_bf16(data) if config == "bf16_data16" else None
    rows = torch.randint(0, n_rows, (B,), generator=torch.Generator().manual_seed(33))
    rows[:4] = torch.tensor([n_rows - 1, 0, 5, 5])                          # edges and a repeated row
    rows = rows.to(U.DEV)
    noise = U.noise_to_device(R.draw_noise(h, B, seed=34))
    out = []
    for indexed in (False, True):
        m = U.build_model(h, sd)
        m.train()
        m.gemm_dtype = config.split("_")[0]
        m.set_explicit_noise(noise)
        if indexed:
            buf = m.fused_train_step_rows(data, rows, 1.0, None, do_adam=False, data16=data16)
        else:
            buf = m.fused_train_step(data[rows].contiguous().expand(A, -1, -1), 1.0, None, do_adam=False)
        torch.cuda.synchronize()
        out.append([buf.cpu().clone(), m.flat_grad().detach().cpu().clone(), m._bn_flat.detach().cpu().clone()])
    assert bool(torch.isfinite(out[0][0]).all()) and bool(torch.isfinite(out[0][1]).all()) and float(out[0][1].abs().max()) > 0
    for u, v in zip(*out):
        assert torch.equal(u.view(torch.int32), v.view(torch.int32)), "rows vs gather"


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("name", ["h112", "h124", "h128", "cs129", "h102"])
def test_nan_workspace_changes_no_bit(name, engine):
    """Plans with planes written and not read (h112, h124: d10 planes beside FC11_ZT), not written at all (h128, cs129) and the
    general path: what the workspace held before the call must not reach the results."""
    row = P.BY_NAME[name]
    U, h, sd, x, noise, m, eng = _env(row, engine)
    noise_dev = U.noise_to_device(noise)
    params, xd, xs = _place(m, x, None)
    state0 = (m._bn_flat.clone(), m._nbt.clone())
    for path in (_fused, _api):
        eng.ws.fill_(0.0)
        l0, g0 = path(m, eng, noise_dev, params, xd, xs, state0)
        eng.ws.fill_(float("nan"))
        l1, g1 = path(m, eng, noise_dev, params, xd, xs, state0)
        assert bool(torch.isfinite(l1).all()) and bool(torch.isfinite(g1).all()), path.__name__
        assert torch.equal(l0, l1) and torch.equal(g0, g1), path.__name__


# what does not depend on the arm count, the batch size or the side stream (decode engines: one arm, n rows, no side stream)
PATH_FIELDS = ("kind", "fast", "big", "small_x3", "fc11", "chain_planes", "lat_half", "narrow", "presplit", "bwd_small_planes",
               "d10_planes", "dz1_in_apply", "dec_planes", "zero", "rowmap", "dz11_bf16", "loss_on_side", "couple", "lat_fork_rides",
               "fc11_fork_rides", "dw11_side")
DECODE_ROWS = ["h108", "h112", "h124", "h128", "h102", "d522", "cs129"]


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("name", DECODE_ROWS)
def test_decode_and_state_changes_across_the_fc11_switch(name, engine):
    from tests import test_gpu_decode as TD
    row = P.BY_NAME[name]
    m = TD._model(row.A, row.D, row.H, row.L, row.C, row.S, seed=3)
    m.gemm_dtype = engine
    want = P.expected(row, engine, "DECODE")
    for n in (1, 129):
        c, s = TD._codes(row.A, n, row.C, row.S, 4 + n)
        xr = m.decoder(c[1], s[1], 1)
        torch.cuda.synchronize()
        eng = TD._dec_engine(m, 1, n)
        got = _assert_plan(row, engine, eng, m._hyper(1.0, True), m._flat, xr, 0, "DECODE", PATH_FIELDS)
        # (fc11's operands are bf16-rounded only where the plan runs the bf16 output kernel: past its tiles and off the fast
        # path the bf16 configuration decodes on the fp32 kernels)
        TD._check_decode(m, 1, c[1], s[1], xr, eng, engine="bf16" if got["fc11"] == "FC11_OUT_BF16" else "fp32x3")
    # decoder(forward's codes) against the forward's own x_rec
    g = torch.Generator().manual_seed(6)
    x = (torch.relu(torch.randn(129, row.D, generator=g)) * 2).to(TD.DEV)
    with torch.no_grad():
        out = m(x.expand(row.A, -1, -1), 1.0, eval=True)
    _assert_plan(row, engine, m._engine, m._hyper(1.0, True), m._flat, x, 0, "FORWARD_XREC", PATH_FIELDS)
    for a in range(row.A):
        xr = m.decoder(out[6][a], out[5][a], a)
        torch.cuda.synchronize()
        if engine == "fp32_mfma":
            assert torch.equal(xr, out[0][a])
        else:
            err = float((xr - out[0][a]).abs().max()) / float(out[0][a].abs().max())
            assert err < (2e-2 if want["fc11"] == "FC11_OUT_BF16" else TD.TOL), err
    # the traversal of one cell, 129 samples, against the fp64 restatement
    u = torch.rand(row.A, 129, 1, generator=g)
    m.set_explicit_state_noise(u.to(TD.DEV))
    recon, _ = m.state_changes(x[:1], 1, 1.0, n_samp=129)
    eng = TD._dec_engine(m, row.A, 1, 129)
    _assert_plan(row, engine, eng, m._hyper(1.0, True), m._flat, x, 0, "TRAVERSE", PATH_FIELDS)
    _assert_plan(row, engine, eng, m._hyper(1.0, True), m._flat, x, 0, "DECODE", PATH_FIELDS)
    got = torch.empty_like(recon)
    got[:, torch.zeros(129).sort()[1]] = recon
    ref = TD.DR.state_changes(TD._sd64(m), x[:1].double().cpu(), 1, u.double(), n_arm=row.A)[:, :, 0, :]
    err = float((got.double() - ref).abs().max()) / float(ref.abs().max())
    print(f"{name} {engine}: state_changes rel err {err:.2e}")
    assert err < TD.TRAV_TOL[engine], err


def _eval_case(row):
    """Parameters with running statistics that are not the initial (0, 1), one batch, the eval-mode noise (state draws only)."""
    h = R.Hyper(input_dim=row.D, fc_dim=row.H, n_categories=row.C, state_dim=row.S, lowD_dim=row.L, x_drop=row.x_drop,
                s_drop=row.s_drop, n_arm=row.A, hard=row.hard)
    sd = R.init_state_dict(h, 546)
    g = torch.Generator().manual_seed(77)
    for k in sd:
        if k.endswith("running_mean"):
            sd[k] = 0.3 * torch.randn(sd[k].shape, generator=g)
        elif k.endswith("running_var"):
            sd[k] = 0.5 + torch.rand(sd[k].shape, generator=g)
    return h, sd, R.synthetic_batch(row.B, row.D, seed=3), R.draw_noise(h, row.B, seed=5, training=False, eval_flag=True)


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("name", P.EVAL_ROWS)
def test_eval_forward_and_classify_labels_against_oracle(name, engine):
    """Eval mode (running statistics, no dropout, no Gumbel noise, hard sample; launch_chain_fwd_enc_eval, the latent kernel in
    both forms) on the width and latent rows: the labels of eval_classify and of the eval forward's c equal the fp64 oracle's
    but for at most plan_cases.EVAL_LABEL_CAP[row] cells (the fp32 CPU oracle's own count of differing labels, 0 on every
    row, plus 1), asserted again here against the fp32 oracle; the forward's outputs at the 1e-4 of test_golden_eval_forward
    on the cells whose label agrees (a cell with another label decodes another category).  Where the plan multiplies
    bf16-rounded operands (GEMM_BF16) the outputs are held to that configuration's 5e-2 instead; the label cap stays."""
    from tests import gpu_util as U
    row = P.BY_NAME[name]
    A = row.A
    h, sd, x, noise = _eval_case(row)
    with torch.no_grad():
        o32 = R.forward({k: v.clone() for k, v in sd.items()}, [x] * A, h, noise, training=False, eval_flag=True,
                        update_running=False)
        sd64 = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}
        n64 = {k: [t.double() for t in v] for k, v in noise.items()}
        o64 = R.forward(sd64, [x.double()] * A, h, n64, training=False, eval_flag=True, update_running=False)
    lab64 = torch.stack([c.argmax(1) for c in o64[4]])
    cap = P.EVAL_LABEL_CAP[name]
    assert int((torch.stack([c.argmax(1) for c in o32[4]]) != lab64).sum()) + 1 == cap
    m = U.build_model(h, sd)
    m.eval()
    m.gemm_dtype = engine
    xd = x.to(U.DEV)
    labels = m.eval_labels(xd.expand(A, -1, -1), 1.0).cpu().long()
    torch.cuda.synchronize()
    hyper = m._hyper(1.0, True)
    plan = _assert_plan(row, engine, m._engine, hyper, m._flat, xd, 0, "CLASSIFY")
    m.set_explicit_noise(U.noise_to_device(noise))
    with torch.no_grad():
        out = m(xd.expand(A, -1, -1), 1.0, eval=True)
    torch.cuda.synchronize()
    _assert_plan(row, engine, m._engine, hyper, m._flat, xd, 0, "FORWARD_XREC")
    lab_fwd = torch.stack([c.argmax(1) for c in out[4]]).cpu()
    n_cls, n_fwd = int((labels != lab64).sum()), int((lab_fwd != lab64).sum())
    print(f"{name} {engine}: labels differing from the fp64 oracle: eval_classify {n_cls}, eval forward {n_fwd} (cap {cap})")
    assert torch.equal(labels, lab_fwd)                  # the same encoder and latent kernels
    bf16 = plan["big"] == "GEMM_BF16"
    tol = LOSS_GATE if bf16 else 1e-4
    same = (lab_fwd == lab64)
    names = {3: "x_low", 7: "s_mean", 8: "s_logvar", 9: "c_prob"} if bf16 else \
        {0: "x_rec", 3: "x_low", 4: "c", 5: "s_smp", 6: "c_smp", 7: "s_mean", 8: "s_logvar", 9: "c_prob"}
    for i, nm in names.items():
        got, ref = torch.stack([t.cpu() for t in out[i]]).double(), torch.stack(list(o64[i]))
        keep = same.unsqueeze(-1).expand_as(ref)
        err = float(((got - ref).abs() * keep).max()) / float(ref.abs().max())
        print(f"   {nm}: {err:.2e}")
        assert err < tol, (nm, err)
    assert n_cls <= cap and n_fwd <= cap, (n_cls, n_fwd, cap)


def _replay(eng, ws0, stages, hyper, nz, params, xd, xs, poison=()):
    """The workspace after replaying `stages` on the state `ws0` (NaN in the `poison` views first: a replay must write them)."""
    eng.ws.copy_(ws0)
    for v in poison:
        v.fill_(float("nan"))
    for s in stages:
        eng.debug_stage(s, hyper, nz, params, xd, xs)
    torch.cuda.synchronize()
    return eng.ws.clone()


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("name", ["h100", "h108"])
def test_single_launch_stages_replay_the_combined_stages_bit_for_bit(name, engine):
    """Debug stages 10 / 11 (fc11's main launch, d(d10)) and 12 / 13 (dW1, dW11) are the launches of stages 1 and 2, one at a
    time: after a full step, replaying 10 then 11 leaves the workspace -- dZ11 and the d(d10) slabs in it -- bit-equal to
    replaying 1, and 12 then 13 (the dW1 / dW11 slabs) bit-equal to replaying 2.  The same kernels on the same inputs: no
    tolerance.  dZ11 and the slabs the decoder backward sums are NaN-filled before the fc11 replays and must come back finite.
    (fc_dim 100 and 108: FC11_ZG / FC11_ZT on engine 0, the fused kernels of the other two, whose stage 11 launches nothing.)"""
    from distributed_vae_amd import _native as N
    row = P.BY_NAME[name]
    U, h, sd, x, noise, m, eng = _env(row, engine)
    noise_dev = U.noise_to_device(noise)
    params, xd, xs = _place(m, x, None)
    hyper, nz = m._hyper(1.0, False), N.make_noise(noise_dev)
    plan = _assert_plan(row, engine, eng, hyper, params, xd, xs)
    _fused(m, eng, noise_dev, params, xd, xs, (m._bn_flat.clone(), m._nbt.clone()))
    ws0 = eng.ws.clone()
    dz11 = eng.ws_view("dz11", row.D)
    gd10 = eng.ws_raw("gd10_slab", plan["gd10_slabs"] * row.A * row.B * row.H)
    bits = lambda t: t.view(torch.int32)
    both = _replay(eng, ws0, (1,), hyper, nz, params, xd, xs, (dz11, gd10))
    assert bool(torch.isfinite(dz11).all()) and bool(torch.isfinite(gd10).all())
    apart = _replay(eng, ws0, (10, 11), hyper, nz, params, xd, xs, (dz11, gd10))
    assert bool(torch.isfinite(dz11).all()) and bool(torch.isfinite(gd10).all())
    assert torch.equal(bits(both), bits(apart)), "stage 1 vs 10 + 11"
    both = _replay(eng, ws0, (2,), hyper, nz, params, xd, xs)
    apart = _replay(eng, ws0, (12, 13), hyper, nz, params, xd, xs)
    assert torch.equal(bits(both), bits(apart)), "stage 2 vs 12 + 13"

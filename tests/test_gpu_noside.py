"""-m gpu: the fused step on engines WITHOUT a side stream (mmvae_exec.side_stream = NULL; MMVAE_SIDE_STREAM=0 of the Python
layer), on every GEMM engine, for the rows plan_cases.NOSIDE_GPU -- the smallest shapes that reach each thing make_plan
(csrc/api.hip) does differently then:

  * dW11 on the main stream behind the whole backward chain and dW1 (do_backward), not right behind fc11 on the side stream;
  * the coupling kernel and the loss finalisation behind fc11 (train_step_impl: do_loss), not beside the decoder chain and
    not as a role of its launch;
  * k_lat_fwd_h and the fused fc11 kernels through the plain launch, no fork event riding on them;
  * with Adam, ONE k_reduce launch over all 26 descriptors with the update fused in (which = 3), not the fc11 tensors' on the
    side stream (which = 1) and the rest's on the main one (which = 2).

Per row and engine: the plan read back from the live engine against plan_cases.without_side() of the table's; the numbers
against the oracle at the gates of tests/test_gpu_plan_matrix.py (its own helper, not a copy); every result BIT-IDENTICAL to
the engine with a side stream; fused == forward / loss / backward on the no-side engine; a NaN-filled workspace changes no
bit; the row-indexed step == gather-then-step; the data-parallel hand-off falls back to one all-reduce; a null mmvae_exec
through the C ABI == the no-side engine.

Why bit-identical, from the code (nothing here is measured): both engines run the same kernels on the same operands -- the
plans differ in the five fields without_side() names, and those choose streams, event mechanics and the launch a role rides
in, never arithmetic; default_splits and make_layout do not read side_stream, so the same number of slabs is summed in the
same order (tests/test_plan_cpu.py::test_splits_and_workspace_do_not_depend_on_the_side_stream); batch sums go through exact
fixed-point accumulators, whose integer adds commute; k_couple and its decoder-launch role are pinned bit-identical by
tests/test_gpu_launch_graph.py; launch_loss_finalize ends in mode 2 (the scalars alone, from the accumulators' T sums) on
either engine while the accumulators are on; k_reduce sums a descriptor's slabs in slab order whichever launch carries the
descriptor.  No comparison here has a tolerance of its own: bit patterns (`_same` of tests/test_gpu_launch_graph.py), or
the gates of tests/test_gpu_plan_matrix.py by name.
"""
import ctypes as C
import functools

import pytest
import torch

from oracle import restatement as R
from tests import plan_cases as P
from tests import test_gpu_plan_matrix as M
from tests.test_gpu_launch_graph import _same

pytestmark = pytest.mark.gpu

ENGINES = list(P.ENGINES)
ROWS = list(P.NOSIDE_GPU)
RESULTS = ("loss", "grads", "bn", "nbt")


def _results(m, buf, g):
    return {"loss": buf.detach().cpu().clone(), "grads": g.detach().cpu().clone(), "bn": m._bn_flat.detach().cpu().clone(),
            "nbt": m._nbt.detach().cpu().clone()}


@functools.lru_cache(maxsize=None)
def _step(name, engine, side):
    """One fused step (no Adam, explicit noise) of the row on an engine with or without a side stream, from the same model
    state, x and noise (tests/test_gpu_plan_matrix.py::_env draws them from fixed seeds): loss vector, flat gradient, running
    statistics, num_batches_tracked.  Computed once per case and shared; nobody writes to it."""
    row = P.BY_NAME[name]
    U, h, sd, x, noise, m, eng = M._env(row, engine, side=side)
    params, xd, xs = M._place(m, x, row.misalign)
    state0 = (m._bn_flat.clone(), m._nbt.clone())
    buf, g = M._fused(m, eng, U.noise_to_device(noise), params, xd, xs, state0)
    out = _results(m, buf, g)
    assert bool(torch.isfinite(out["loss"]).all()) and bool(torch.isfinite(out["grads"]).all()) and bool(torch.isfinite(out["bn"]).all())
    # a step happened: gradients, moved running statistics, one more batch tracked by the BatchNorms the forward pass runs
    assert float(out["grads"].abs().max()) > 0 and not torch.equal(out["bn"], state0[0].cpu())
    d_nbt = out["nbt"] - state0[1].cpu()
    assert int(d_nbt.min()) >= 0 and int(d_nbt.max()) == 1, d_nbt
    return out


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("name", ROWS)
def test_plan_without_side_then_fused_equals_api(name, engine, monkeypatch):
    """The live no-side engine's STEP, FORWARD and BACKWARD plans (and STEP_ROWS where the row has a row map) are
    without_side() of the table's; then the fused step equals forward / loss / backward on that engine at
    test_gpu_plan_matrix._same_to_api_gates (loss 1e-6, gradients 1e-5) -- on the fast rows too, where mmvae_backward with
    dw11_side = false runs nowhere else."""
    row = P.BY_NAME[name]
    U, h, sd, x, noise, m, eng = M._env(row, engine, side=False, monkeypatch=monkeypatch)
    noise_dev = U.noise_to_device(noise)
    params, xd, xs = M._place(m, x, row.misalign)
    hyper = m._hyper(1.0, False)
    plan = M._assert_plan(row, engine, eng, hyper, params, xd, xs, "STEP", side=False)
    assert (plan["dw11_side"], plan["loss_on_side"], plan["couple"], plan["lat_fork_rides"], plan["fc11_fork_rides"]) == \
        (False, False, "COUPLE_INLINE", False, False)
    M._assert_plan(row, engine, eng, hyper, params, xd, xs, "FORWARD", side=False)
    M._assert_plan(row, engine, eng, hyper, params, xd, xs, "BACKWARD", side=False)
    if P.expected(row, engine, "STEP_ROWS")["rowmap"]:
        assert M._assert_plan(row, engine, eng, hyper, params, xd, xs, "STEP_ROWS", side=False)["rowmap"]
    state0 = (m._bn_flat.clone(), m._nbt.clone())
    lf, gf = M._fused(m, eng, noise_dev, params, xd, xs, state0)
    la, ga = M._api(m, eng, noise_dev, params, xd, xs, state0)
    assert bool(torch.isfinite(lf).all()) and bool(torch.isfinite(gf).all()) and float(gf.abs().max()) > 0
    M._same_to_api_gates((lf.cpu(), M._named(m, gf)), (la.cpu(), M._named(m, ga)), "no side stream: fused vs api")


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("name", ROWS)
def test_fused_step_without_side_against_oracle(name, engine, monkeypatch):
    """tests/test_gpu_plan_matrix.py::test_plan_then_fused_step_against_oracle, the same checks at the same gates, on an
    engine without a side stream."""
    M._plan_then_fused_step_against_oracle(name, engine, side=False, monkeypatch=monkeypatch)


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("name", ROWS)
def test_fused_step_without_side_is_bit_identical_to_the_side_stream_engine(name, engine):
    """Loss vector, flat gradient, running statistics and num_batches_tracked of one fused step: the same bits with and
    without a side stream (why: the module's docstring)."""
    _same(_step(name, engine, False), _step(name, engine, True))


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("name", ROWS)
def test_early_grad_event_is_not_offered_without_a_side_stream(name, engine, monkeypatch):
    """The data-parallel hand-off (dist.py, two all-reduces where `eng.early_event is not None and eng.early_recorded()`): an
    engine without a side stream creates no event when asked for one, a step without Adam reports nothing recorded -- so the
    caller falls back to one all-reduce -- and the gradient is the plain no-side step's, bit for bit."""
    row = P.BY_NAME[name]
    U, h, sd, x, noise, m, eng = M._env(row, engine, side=False, monkeypatch=monkeypatch)
    eng.enable_early_grad_event(True)
    assert eng.early_event is None and not eng.ex.early_grad_event
    eng.ex.early_recorded = 1                             # (the call must clear it: do_backward writes 0 first)
    params, xd, xs = M._place(m, x, row.misalign)
    buf, g = M._fused(m, eng, U.noise_to_device(noise), params, xd, xs, (m._bn_flat.clone(), m._nbt.clone()))
    assert eng.early_recorded() is False
    _same(_results(m, buf, g), _step(name, engine, False))


# ---- two fused Adam steps: which = 3 against which = 1 + which = 2 -------------------------------------------------------
ADAM = ("loss", "params", "grads", "bn", "exp_avg", "exp_avg_sq")


@functools.lru_cache(maxsize=None)
def _adam_inputs(name):
    """The inputs of test_gpu_plan_matrix.test_two_adam_steps_reproduce_bit_for_bit_and_rows_equal_gather for the row."""
    from tests import gpu_util as U
    row = P.BY_NAME[name]
    h = R.Hyper(input_dim=row.D, fc_dim=row.H, n_categories=row.C, state_dim=row.S, lowD_dim=row.L, x_drop=row.x_drop,
                s_drop=row.s_drop, n_arm=row.A, hard=row.hard)
    n_rows = 3 * row.B + 5
    data = R.synthetic_batch(n_rows, row.D, seed=32).to(U.DEV)
    rows = torch.randint(0, n_rows, (row.B,), generator=torch.Generator().manual_seed(33))
    rows[:2] = torch.tensor([n_rows - 1, 0])
    return row, h, R.init_state_dict(h, 31), data, rows


@functools.lru_cache(maxsize=None)
def _adam(name, engine, side, indexed=False, weight_decay=0.0, decoupled=False):
    row, h, sd, data, rows = _adam_inputs(name)
    out = dict(zip(ADAM, M._two_adam_steps(row, engine, h, {k: v.clone() for k, v in sd.items()}, data, rows, indexed, side=side,
                                           weight_decay=weight_decay, decoupled=decoupled)))
    assert all(bool(torch.isfinite(v).all()) for v in out.values())
    # both moments took part: a first moment of either sign, a second moment that is nowhere negative and somewhere positive
    assert float(out["exp_avg"].min()) < 0 < float(out["exp_avg"].max())
    assert float(out["exp_avg_sq"].min()) >= 0 and float(out["exp_avg_sq"].max()) > 0
    return out


ADAM_CASES = [(n, e) for n in ROWS for e in ("bf16", "fp32x3")] + [("h100", "fp32_mfma")]


@pytest.mark.parametrize("name,engine", ADAM_CASES)
def test_two_adam_steps_without_side_are_bit_identical_to_the_side_stream_engine(name, engine):
    """Two fused Adam steps: loss vectors, parameters, gradients, running statistics AND both Adam moments (a wrong moment
    shows in the parameters only steps later), the same bits with and without a side stream -- the one k_reduce launch with
    the update fused in over all tensors (which = 3) against the fc11 tensors' launch on the side stream plus the rest's on
    the main one.  The update is elementwise on the reduced gradient, and a descriptor's slabs are summed in the same order in
    either launch."""
    _same(_adam(name, engine, False), _adam(name, engine, True))


@pytest.mark.parametrize("decoupled", [False, True])
@pytest.mark.parametrize("engine", ENGINES)
def test_two_adam_steps_with_weight_decay_without_side(engine, decoupled):
    """The same on row h100 with weight_decay = 0.01, coupled (Adam: added to the gradient) and decoupled (AdamW)."""
    a, b = _adam("h100", engine, False, False, 0.01, decoupled), _adam("h100", engine, True, False, 0.01, decoupled)
    _same(a, b)
    # the decay reached the update: other parameters than without it
    assert not torch.equal(a["params"], _adam("h100", engine, False)["params"])


@pytest.mark.parametrize("engine", ["bf16", "fp32x3"])
@pytest.mark.parametrize("name", ["h100", "b129"])
def test_row_indexed_step_without_side_equals_gather_then_step(name, engine):
    """Where the plan has `rowmap`: the no-side row-indexed step (two Adam steps) is bit-identical to gather-then-step."""
    assert P.without_side(P.expected(P.BY_NAME[name], engine, "STEP_ROWS"))["rowmap"]
    _same(_adam(name, engine, False, True), _adam(name, engine, False, False))


# ---- workspace independence ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("name", ["h100", "h112", "a4"])
def test_nan_workspace_changes_no_bit_without_side(name, engine, monkeypatch):
    """What the workspace held before the call must not reach the no-side step's results (dW11 reads dZ11 and the [d10 | 1]
    planes or D10 only after the whole backward chain has run): zero-filled against NaN-filled, as
    test_gpu_plan_matrix.test_nan_workspace_changes_no_bit does it."""
    row = P.BY_NAME[name]
    U, h, sd, x, noise, m, eng = M._env(row, engine, side=False, monkeypatch=monkeypatch)
    noise_dev = U.noise_to_device(noise)
    params, xd, xs = M._place(m, x, None)
    state0 = (m._bn_flat.clone(), m._nbt.clone())
    eng.ws.fill_(0.0)
    zero = _results(m, *M._fused(m, eng, noise_dev, params, xd, xs, state0))
    eng.ws.fill_(float("nan"))
    nan = _results(m, *M._fused(m, eng, noise_dev, params, xd, xs, state0))
    assert all(bool(torch.isfinite(nan[k]).all()) for k in ("loss", "grads", "bn"))
    _same(nan, zero)
    _same(nan, _step(name, engine, False))


# ---- a null mmvae_exec ---------------------------------------------------------------------------------------------------
def test_null_exec_through_the_c_abi_equals_the_no_side_engine(monkeypatch):
    """include/mmvae.h: `ex` may be NULL.  mmvae_workspace_bytes and mmvae_train_step called directly with a null mmvae_exec
    (engine fp32_mfma by the hyper, a fresh NaN-filled workspace, the caller's current stream) on row h100: the library's
    zeroed exec is what the Python layer's no-side engine 0 hands it (split and tune all zeros, asserted first), so loss
    vector, gradients and running statistics are that engine's, bit for bit."""
    from distributed_vae_amd import _native as N
    row = P.BY_NAME["h100"]
    U, h, sd, x, noise, m, eng = M._env(row, "fp32_mfma", side=False, monkeypatch=monkeypatch)
    zeroed = N.Exec()
    assert list(eng.ex.split) == list(zeroed.split) == [0] * 6
    assert list(eng.ex.tune) == list(zeroed.tune) == [0] * N.N_TUNE
    assert not eng.ex.side_stream and not eng.ex.early_grad_event
    L = N.lib()
    nbytes = int(L.mmvae_workspace_bytes(C.byref(eng.dims), None))
    assert nbytes == eng.ws_bytes > 0
    ws = torch.full((nbytes // 4,), float("nan"), dtype=torch.float32, device=U.DEV)
    assert ws.data_ptr() % 256 == 0
    noise_dev = U.noise_to_device(noise)
    params, xd, xs = M._place(m, x, None)
    hyper, nz = m._hyper(1.0, False), N.make_noise(noise_dev)
    assert hyper.gemm_bf16 == P.ENGINES["fp32_mfma"]
    g = torch.zeros_like(m._flat_grad)
    loss = torch.zeros(5 + 3 * row.A, dtype=torch.float32, device=U.DEV)
    N.check(L.mmvae_train_step(C.byref(eng.dims), C.byref(hyper), C.byref(nz), N._ptr(params), N._ptr(m._bn_flat), N._ptr(m._nbt),
                               N._ptr(xd), xs, N._ptr(ws), nbytes, N._ptr(g), N._ptr(loss), 0, None, None, 1, 0.0, 0.9, 0.999,
                               1e-8, 0.0, 0, None, N._stream(eng.device)), "mmvae_train_step(ex = NULL)")
    torch.cuda.synchronize()
    _same(_results(m, loss, g), _step("h100", "fp32_mfma", False))

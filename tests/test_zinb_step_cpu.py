"""CPU (no GPU): what training under the ZINB objective rests on that needs no device.

  * the precondition of tests/zinb_step_cases.py: at every row the ZINB term is at least MIN_SHARE of every encoder and latent
    tensor's gradient (at the default point it is not: measured here too, so the table cannot drift back);
  * tests/zinb_step_restatement.py against itself: autograd against central finite differences on a handful of entries, the
    terms add up to the total, the loss tuple's pieces are the reference restatement's;
  * mmvae_zinb_head_layout and mmvae_zinb_step_workspace_bytes against their stated formulas;
  * mmvae_debug_plan for call kind 11 on the rows of tests/zinb_plan_cases.py; kind 9 stays unknown; the ABI is still 5;
  * every refusal of zinb_train_step, zinb_objective and fit_zinb on a CPU model, before the engine is made or noise consumed.
"""
import ctypes as C

import pytest
import torch

import distributed_vae_amd  # noqa: F401
from distributed_vae_amd import _native as N
from distributed_vae_amd.nn_model import mk_vae
from oracle import restatement as R
from tests import plan_cases as P
from tests import term_cases as T
from tests import zinb_plan_cases as ZP
from tests import zinb_step_cases as Z

S = Z.S


# ---- 1. the precondition ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", Z.ROW_IDS)
def test_zinb_term_reaches_every_encoder_and_latent_tensor(name):
    Z.assert_exposes(name)
    o = Z.oracle(name)
    pinned = {k: s for k, s in o["share"].items() if Z.is_pinned(k)}
    print(f"{name}: ZINB share of the pinned tensors {min(pinned.values()):.3g} .. {max(pinned.values()):.3g}; "
          f"fp32 restatement's worst error {max(o['e32'].values()):.2e}")
    assert len(pinned) == 16 * o["h"].n_arm and len(o["g64"]) == 32 * o["h"].n_arm


def test_table_covers_the_combinations():
    rows = Z.ROWS
    assert {r.A for r in rows} == {2, 3} and {r.hard for r in rows} == {False, True}
    assert {r.s_drop > 0 for r in rows} == {False, True} and all(r.x_drop > 0 for r in rows)
    assert {r.B for r in rows} == {70, 129} and {70, 130} <= {r.D for r in rows} and {r.H for r in rows} == {20, 100, 128}
    assert any(r.D % 4 == 0 and r.H % 4 == 0 for r in rows) and any(r.D % 4 for r in rows)          # on and off the fast path
    assert all(r.D % 64 for r in rows)                                                               # a partial last gene tile


def test_default_point_does_not_pin_the_zinb_path():
    """tau = 0.005, temp = beta = lam = 1 on the first row's shape: the ZINB term is far below MIN_SHARE somewhere."""
    row = Z.ROWS[0]._replace(tau=0.005, beta=1.0, lam=1.0)
    h, sd, x, noise = Z.inputs(row)
    sd64, x64, n64 = T.to64(sd, x, noise)
    tg = S.term_grads(sd64, [x64] * h.n_arm, h, n64)
    share = []
    for k in S.param_keys(h):
        if Z.is_pinned(k):
            tot = sum(tg[t][k] for t in S.TERMS)
            share.append(float(tg["zinb"][k].abs().max()) / (float(tot.abs().max()) + 1e-300))
    assert min(share) < 0.1 * Z.MIN_SHARE, min(share)


# ---- 2. the restatement against itself --------------------------------------------------------------------------------------
def test_restatement_autograd_matches_finite_differences():
    """Central differences of the total at a gentle point of the first row's shape: counts up to 50, where the total is of
    order 10 and a step of 1e-6 leaves 1e-9 of rounding (at the table's counts of 1e5 the term, which has no lgamma(k + 1), makes
    the total -3e5).  Per tensor the non-zero entry of median magnitude: the largest ones sit where r = relu(a_rec) + eps is
    within a step of its kink, and a difference quotient says nothing there."""
    row = Z.BY_NAME["a2_d70_h20"]
    h, sd, _, noise = Z.inputs(row)
    x = Z.ZR.counts_matrix(row.B, row.D, torch.Generator().manual_seed(5), max_count=50)
    sd64, x64, n64 = T.to64(sd, x, noise)
    xs = [x64] * h.n_arm
    _, _, lt, g = S.grads_autograd({k: v.clone() for k, v in sd64.items()}, xs, h, n64)
    total = float(lt[0].detach())
    assert abs(S.objective_value(sd64, xs, h, n64) - total) <= 1e-12 * abs(total) and abs(total) < 1e3
    for key in ("fc1.0.weight", "fc3.1.bias", "fcc.0.weight", "fc_mu.1.weight", "fc_sigma.0.bias", "fc6.0.weight", "fc10.1.weight",
                "fc11.0.weight", "fc11.1.bias", "fc11_p.0.weight", "fc11_p.1.bias", "fc11_r.1.weight", "fc11_r.0.bias"):
        flat = g[key].flatten()
        nz = flat.abs().nonzero().flatten()
        i = int(nz[flat[nz].abs().argsort()[nz.numel() // 2]])
        step = 1e-6
        vals = []
        for sgn in (1.0, -1.0):
            sdp = {k: v.clone() for k, v in sd64.items()}
            sdp[key].view(-1)[i] += sgn * step
            vals.append(S.objective_value(sdp, xs, h, n64))
        fd = (vals[0] - vals[1]) / (2 * step)
        assert abs(fd - float(flat[i])) <= 1e-5 * abs(float(flat[i])) + 1e-8, (key, i, fd, float(flat[i]))


def test_restatement_terms_add_up_and_keep_the_reference_pieces():
    o = Z.oracle("a3_d132_h100_fast")
    h, lt = o["h"], o["lt64"]
    sd64, x64, n64 = T.to64(o["sd"], o["x"], o["noise"])
    xs = [x64] * h.n_arm
    with torch.no_grad():
        out, saved, terms, zl = S.objective_terms(dict(sd64), xs, h, n64, update_running=False)
        mse = R.loss(out, xs, h)
    am1 = max(h.n_arm - 1, 1)
    total = am1 * sum(float(z) + h.beta * float(k) for z, k in zip(zl, mse[6])) + float(mse[2])     # the issue's formula
    assert abs(total - float(lt[0])) <= 1e-12 * abs(total)
    assert torch.equal(lt[1], torch.stack(zl)) and float(lt[2]) == float(mse[2]) and [float(v) for v in lt[8]] == [float(v) for v in mse[8]]
    assert all(bool(torch.isfinite(z)) for z in zl)


# ---- 3. layout and workspace formulas ---------------------------------------------------------------------------------------
DIMS = [(2, 70, 70, 20, 8, 12, 3), (3, 129, 130, 100, 8, 12, 3), (2, 5000, 5032, 100, 10, 92, 2), (1, 2, 1, 1, 1, 1, 1), (8, 257, 130, 128, 10, 92, 2)]


@pytest.mark.parametrize("dims", DIMS)
def test_head_layout_and_workspace_formulas(dims):
    A, B, D, H = dims[:4]
    d = N.Dims(*dims)
    lay = N.zinb_head_layout(d)
    assert int(lay.per_arm) == 2 * (D * H + D) and list(lay.offset) == [0, D * H, D * H + D, 2 * D * H + D]
    L = N.lib()
    one_pass = int(L.mmvae_zinb_head_grads_workspace_bytes(B, D, H, 0)) + int(L.mmvae_zinb_d10_grad_workspace_bytes(B, D, H, -(-D // 64)))
    assert int(L.mmvae_zinb_step_grads_workspace_bytes(B, D, H, 0)) == one_pass
    assert int(L.mmvae_zinb_d10_grad_workspace_bytes(B, D, H, -(-D // 64))) == 8 * ((-(-D // 64) * B * H + 1) // 2)
    want = one_pass + 8 * (A * B + D + A)
    assert N.zinb_step_workspace_bytes(d) == want > 0
    ex = N.Exec()
    ex.side_stream = 1
    assert N.zinb_step_workspace_bytes(d, ex) == want
    assert int(L.mmvae_zinb_nll_workspace_bytes(B, D)) <= int(L.mmvae_zinb_head_grads_workspace_bytes(B, D, H, 0))


def test_layout_and_workspace_refuse_bad_dims():
    bad = N.Dims(2, 70, 70, 129, 8, 12, 3)                                 # fc_dim above 128
    assert N.zinb_step_workspace_bytes(bad) == 0
    out = N.ZinbHeadLayout()
    assert N.lib().mmvae_zinb_head_layout(C.byref(bad), C.byref(out)) == -2
    assert N.lib().mmvae_zinb_head_layout(C.byref(N.Dims(2, 70, 70, 20, 8, 12, 3)), None) == -1
    assert N.lib().mmvae_zinb_head_layout(None, C.byref(out)) == -1


# ---- 4. the plan of call kind 11 --------------------------------------------------------------------------------------------
def _hyper(row, engine):
    return N.Hyper(0.005, 1.0, 1.0, 1.0, 1e-8, 0.01, row.x_drop, row.s_drop, int(row.hard), 1, 0, ZP.ENGINES[engine])


def _exec(engine, side):
    ex = N.Exec()
    ex.tune[N.TUNE_ENGINE] = ZP.ENGINES[engine]
    if side:
        ex.side_stream = 1              # never dereferenced: "has a side stream"
    return ex


def _splits(d, ex):
    sp = (C.c_int32 * 6)()
    N.check(N.lib().mmvae_splits(C.byref(d), C.byref(ex), C.byref(sp)), "mmvae_splits")
    return list(sp)


@pytest.mark.parametrize("engine", list(ZP.ENGINES))
@pytest.mark.parametrize("name", Z.ROW_IDS)
def test_step_cases_take_their_literal_plan(name, engine):
    r = Z.BY_NAME[name]
    d = N.Dims(r.A, r.B, r.D, r.H, r.L, r.C, r.S)
    want = ZP.zinb_plan(ZP.LITERAL[name][engine])
    for side in (True, False):                                             # the side stream of the exec is not used
        ex = _exec(engine, side)
        got = N.debug_plan(d, _hyper(r, engine), ex, ZP.KIND)
        want["dw11_slabs"] = _splits(d, ex)[P.slab_sources(want)[1]]
        diff = {k: (got[k], want[k]) for k in N.PLAN_NAMES if got[k] != want[k]}
        assert not diff, (name, engine, side, diff)


@pytest.mark.parametrize("engine", list(ZP.ENGINES))
@pytest.mark.parametrize("row", P.ROWS, ids=lambda r: r.name)
def test_every_plan_row_is_the_step_without_a_side_stream(row, engine):
    d = N.Dims(row.A, row.B, row.D, row.H, row.L, row.C, row.S)
    ex = _exec(engine, row.side)
    got = N.debug_plan(d, _hyper(row, engine), ex, **ZP.plan_args(row))
    want = ZP.expected(row, engine)
    want["dw11_slabs"] = _splits(d, ex)[P.slab_sources(want)[1]]
    diff = {k: (got[k], want[k]) for k in N.PLAN_NAMES if got[k] != want[k]}
    assert not diff, (row.name, engine, diff)
    step = N.debug_plan(d, _hyper(row, engine), _exec(engine, False), **P.plan_args(row, "STEP"))
    assert {k: v for k, v in step.items() if k not in ("kind", "gd10_slabs")} == {k: v for k, v in got.items() if k not in ("kind", "gd10_slabs")}


def test_kind_numbers_and_abi():
    L = N.lib()
    out = (C.c_int32 * N.PLAN_FIELDS)()
    d, h = N.Dims(2, 300, 520, 100, 10, 92, 2), _hyper(P.BY_NAME["h100"], "fp32x3")
    assert L.mmvae_abi_version() == 5 == N.ABI_VERSION
    assert N.CALL_KINDS["ZINB_STEP"] == 11 and N.CALL_KINDS["ENCODE"] == 10 and 9 not in N.CALL_KINDS.values()
    assert L.mmvae_debug_plan(C.byref(d), C.byref(h), None, 11, 16, 16, 0, 0, 1, C.byref(out)) == 0
    assert out[0] == 11 and out[N.PLAN_NAMES.index("gd10_slabs")] == 1
    assert L.mmvae_debug_plan(C.byref(d), C.byref(h), None, 9, 16, 16, 0, 0, 1, C.byref(out)) == -1     # still unknown
    assert L.mmvae_debug_plan(C.byref(d), C.byref(h), None, 12, 16, 16, 0, 0, 1, C.byref(out)) == -1
    assert len(N.PLAN_NAMES) == N.PLAN_FIELDS == 23
    assert C.sizeof(N.Dims) == 28 and C.sizeof(N.ZinbHeadLayout) == 40


# ---- 5. refusals, without a device ------------------------------------------------------------------------------------------
def _zinb(mode="ZINB"):
    return mk_vae(7, 2, 64, "cpu", fc_dim=16, latent_dim=5, mode=mode)


def _no_engine(monkeypatch, m):
    # nothing past a refusal may run: a CPU model would otherwise fail later, at the engine, with another error
    monkeypatch.setattr(m, "_ensure", lambda *a, **k: pytest.fail("the refusal must come before the engine is made"))
    monkeypatch.setattr(m, "_next_noise", lambda *a, **k: pytest.fail("the refusal must come before noise is consumed"))


def test_zinb_train_step_refusals(monkeypatch):
    x = torch.zeros(2, 4, 64)
    mse = _zinb("MSE")
    _no_engine(monkeypatch, mse)
    with pytest.raises(RuntimeError, match="loss_mode='ZINB'"):
        mse.zinb_train_step(x, 1.0)
    with pytest.raises(RuntimeError, match="loss_mode='ZINB'"):
        mse.eval().zinb_objective(x, 1.0)
    m = _zinb()
    _no_engine(monkeypatch, m)
    with pytest.raises(RuntimeError, match=r"needs model\.train\(\)"):
        m.eval().zinb_train_step(x, 1.0)
    m.train()
    with pytest.raises(RuntimeError, match=r"needs model\.eval\(\)"):
        m.zinb_objective(x, 1.0)
    m.gemm_dtype = "bf16"
    with pytest.raises(NotImplementedError, match="bf16"):
        m.zinb_train_step(x, 1.0)
    m.gemm_dtype = "fp32"
    for kw in (dict(lr=-1.0), dict(weight_decay=-0.1), dict(eps=-1e-8), dict(betas=(0.9, 1.0)), dict(betas=(0.9,))):
        with pytest.raises(ValueError, match="zinb_train_step"):
            m.zinb_train_step(x, 1.0, **kw)
    with pytest.raises(ValueError, match="state"):
        m.zinb_train_step(x, 1.0, state={"step": 3, "exp_avg": torch.zeros(2, 5), "exp_avg_sq": torch.zeros(2, 5), "heads": ("rec",)})
    with pytest.raises(N.NativeError, match="GPU tensors"):
        m.zinb_train_step(x, 1.0)                                          # a CPU batch: refused at the device check
    assert m._step_id == 0 and m._noise_offset == 0
    # the pinned refusals hold beside the new names
    with pytest.raises(NotImplementedError, match="training under loss_mode='ZINB' is not built"):
        m.fused_train_step(x, 1.0, None, do_adam=False)
    with pytest.raises(AssertionError, match="ZINB not implemented"):
        m([torch.zeros(4, 64)] * 2, 1.0)


def _trainer(mode="ZINB"):
    from distributed_vae_amd.cpl_mixvae import cpl_mixVAE
    t = cpl_mixVAE(saving_folder="", device="cpu", save_flag=False)
    t.init_model(n_categories=5, state_dim=2, input_dim=24, fc_dim=6, lowD_dim=3, n_arm=2, mode=mode)
    return t


def test_fit_zinb_refusals(monkeypatch):
    from distributed_vae_amd import dist as DD
    with pytest.raises(RuntimeError, match="loss_mode='ZINB'"):
        _trainer("MSE").fit_zinb(None, 1)
    t = _trainer()
    m = t.model
    _no_engine(monkeypatch, m)
    for kw in (dict(n_epoch=-1), dict(n_epoch=1, lr=-1.0), dict(n_epoch=1, weight_decay=-0.1), dict(n_epoch=1, eps=-1.0),
               dict(n_epoch=1, betas=(1.0, 0.9))):
        with pytest.raises(ValueError, match="fit_zinb"):
            t.fit_zinb(None, **kw)
    m.gemm_dtype = "bf16"
    with pytest.raises(NotImplementedError, match="bf16"):
        t.fit_zinb(None, 1)
    m.gemm_dtype = "fp32"
    # the states of the two decoder fits hold other moments
    for other in ({"step": 2, "exp_avg": torch.zeros(2, 300), "exp_avg_sq": torch.zeros(2, 300), "heads": ("rec", "p", "r")},
                  {"kind": "zinb_step", "step": 2, "exp_avg": torch.zeros(7), "exp_avg_sq": torch.zeros(7),
                   "hp_exp_avg": torch.zeros(2, 300), "hp_exp_avg_sq": torch.zeros(2, 300)}):
        with pytest.raises(ValueError, match="state"):
            t.fit_zinb(None, 1, state=other)
    # a pruned model's mask is not offered in training
    with torch.no_grad():
        for a in range(2):
            m.fcc[a].bias[3] = 0.0
    with pytest.raises(NotImplementedError, match="pruned"):
        t.fit_zinb(None, 1)
    with torch.no_grad():
        for a in range(2):
            m.fcc[a].bias[3] = 0.1
    monkeypatch.setattr(DD, "is_dist", lambda: True)
    with pytest.raises(NotImplementedError, match="not data-parallel"):
        t.fit_zinb(None, 1)
    assert m._step_id == 0 and m._noise_offset == 0 and m.training


def test_zinb_step_state_is_checked_by_shape_only():
    m = _zinb()
    lay = N.param_layout(m._dims(2))
    n, hn = 2 * int(lay.per_arm), 2 * (64 * 16 + 64)
    good = {"kind": "zinb_step", "step": 0, "exp_avg": torch.zeros(n), "exp_avg_sq": torch.zeros(n),
            "hp_exp_avg": torch.zeros(2, hn), "hp_exp_avg_sq": torch.zeros(2, hn)}
    m._check_zinb_step_state("t", good)
    for k in ("kind", "step", "hp_exp_avg"):
        with pytest.raises(ValueError, match="state"):
            m._check_zinb_step_state("t", {kk: v for kk, v in good.items() if kk != k})

"""-m gpu: the step at the operating points of tests/term_cases.py, where the reconstruction, KL, entropy and distance terms
each reach the encoder's gradient (at the default point of every other parity test the distance term is all of it, the
others 1e-12: tests/test_terms_cpu.py), on both fp32-grade engines:

  * the API path (forward, loss, backward): the loss tuple at gpu_util.assert_loss_vector's per-term tolerances, the
    forward outputs at FWD_TOL, every gradient against the fp64 oracle;
  * the fused step without Adam: the same comparison (x_rec apart: the fused fc11 kernels do not write it), and equal to
    the API path at the gate of test_fused_step_matches_api_path_fc100 (loss 1e-6, gradients 1e-5);
  * the running BatchNorm statistics after either against the oracle's (momentum 0.01, 0.1 and 1.0 over the rows).

A gradient tensor's worst entry, relative to the tensor's fp64 maximum, stays below max(GRAD_TOL, 3 x the fp32 CPU oracle's
own error against fp64 in that tensor) -- the rule of gpu_util.assert_gradients_tight; term_cases.py records the fp32
oracle's error where a row needs the second bound (none does at present).  Every test first re-asserts its row's share
precondition.  The bf16 engine runs the rows for finiteness and its configuration's 5e-2 loss gate only: its latent
kernels are the fp32 code the other two engines pin.
"""
import pytest
import torch

from oracle import restatement as R
from tests import golden_util as G
from tests import term_cases as T

pytestmark = pytest.mark.gpu

FWD_TOL, LOSS_TOL = 1e-4, 1e-5                           # tests/test_gpu_parity.py
LOSS_GATE = 5e-2                                         # tests/test_gpu_bf16.py
FWD = {"x_rec": 0, "x_low": 3, "c": 4, "s_smp": 5, "c_smp": 6, "s_mean": 7, "s_logvar": 8, "c_prob": 9}
FP32_ENGINES = ["fp32x3", "fp32_mfma"]


def _model(o, engine):
    from tests import gpu_util as U
    m = U.build_model(o["h"], o["sd"])
    m.train()
    m.gemm_dtype = engine
    return m


def _loss_vector(lt):
    """A loss tuple as the library's loss vector (include/mmvae.h MMVAE_LOSS_*)."""
    return torch.stack([lt[0].detach(), lt[2], lt[3], lt[4], lt[5], *lt[1], *lt[6], *lt[8]]).cpu()


def _assert_forward(name, what, outs, o):
    for nm, ts in outs.items():
        err = G.rel_err(torch.stack([t.cpu() for t in ts]), torch.stack(list(o["out64"][FWD[nm]])))
        assert err < FWD_TOL, (name, what, nm, err)


def _assert_gradients(name, what, grads, o):
    worst = (0.0, None)
    for k, ref in o["g64"].items():
        err, tol = G.rel_err(grads[k], ref), T.grad_tolerance(name, k)
        if T.is_encoder(k):
            worst = max(worst, (err / tol, k))
        assert err < tol, (name, what, k, err, tol, "fp32 oracle: %.2e" % o["e32"][k])
    print(f"{name} {what}: worst encoder gradient at {worst[0]:.2e} of its tolerance ({worst[1]})")


def _assert_running_stats(name, what, m, o):
    sd = m.state_dict()
    for k, ref in o["bn64"].items():
        if "num_batches" in k:
            assert int(sd[k]) == int(ref) == (0 if k.startswith("batch_s.") else 1), (name, what, k)   # batch_s: unused by forward
        else:
            assert G.rel_err(sd[k].cpu(), ref) < 1e-5, (name, what, k)     # the bound of test_golden_forward_loss_grads


def _fused(o, engine):
    from tests import gpu_util as U
    h, row = o["h"], o["row"]
    m = _model(o, engine)
    m.set_explicit_noise(U.noise_to_device(o["noise"]))
    buf = m.fused_train_step(o["x"].to(U.DEV).expand(h.n_arm, -1, -1), row.temp, None, do_adam=False).clone()
    torch.cuda.synchronize()
    grads = {k: gv.detach().cpu().clone() for (k, _), gv in zip(m.named_parameters(), m._grad_views)}
    return m, buf.cpu(), grads


@pytest.mark.parametrize("engine", FP32_ENGINES)
@pytest.mark.parametrize("name", T.ROW_IDS)
def test_step_at_term_exposing_points(name, engine):
    from tests import gpu_util as U
    T.assert_exposes(name)
    o = T.oracle(name)
    h, row, A = o["h"], o["row"], o["h"].n_arm
    # ---- forward / loss / backward
    m1 = _model(o, engine)
    out, lt, g_api = U.run_step(m1, o["x"].to(U.DEV), o["noise"], temp=row.temp)
    l_api = _loss_vector(lt)
    assert bool(torch.isfinite(l_api).all())
    U.assert_loss_vector(l_api, o["lt64"], A, LOSS_TOL)
    _assert_forward(name, "api", {nm: out[i] for nm, i in FWD.items()}, o)
    _assert_gradients(name, "api", g_api, o)
    _assert_running_stats(name, "api", m1, o)
    # ---- the fused step, no Adam
    m2, l_fused, g_fused = _fused(o, engine)
    U.assert_loss_vector(l_fused, o["lt64"], A, LOSS_TOL)
    width = {"x_low": h.lowD_dim, "c": h.n_categories, "s_smp": h.state_dim, "c_smp": h.n_categories,
             "s_mean": h.state_dim, "s_logvar": h.state_dim, "c_prob": h.n_categories}
    _assert_forward(name, "fused", {nm: list(U.ws(m2, nm, w).unbind(0)) for nm, w in width.items()}, o)
    _assert_gradients(name, "fused", g_fused, o)
    _assert_running_stats(name, "fused", m2, o)
    # ---- fused == API (tests/test_gpu_parity.py::test_fused_step_matches_api_path_fc100)
    assert abs(float(l_fused[0]) - float(l_api[0])) <= 1e-6 * abs(float(l_api[0])) + 1e-7
    for k, v in g_fused.items():
        assert G.rel_err(v, g_api[k]) < 1e-5, (name, k)


@pytest.mark.parametrize("name", T.ROW_IDS)
def test_bf16_engine_stays_finite_and_within_its_loss_gate(name):
    T.assert_exposes(name)
    o = T.oracle(name)
    A = o["h"].n_arm
    _, buf, grads = _fused(o, "bf16")
    assert bool(torch.isfinite(buf).all()) and all(bool(torch.isfinite(v).all()) for v in grads.values())
    want = _loss_vector(o["lt64"]).double()
    errs = ((buf.double() - want).abs() / (want.abs() + 1e-30)).tolist()
    print(f"{name} bf16: relative error of (total, joint, c_ent, c_dist, c_l2, rec...):", ["%.2e" % e for e in errs[:5 + A]])
    assert max(errs[i] for i in [0, 1, 3] + list(range(5, 5 + A))) < LOSS_GATE, errs

"""CPU: the count distributions without a device -- tests/countdist_restatement.py against the reference's recorded returns
(tests/golden/countdist_kat.npz), the library's element code (csrc/countdist_core.hpp) through the host-only debug entries
against the restatement, the sampler against the exact pmf, the C boundary's refusals and the Python surface's.

Likelihood gate (tests/countdist_inputs.logp_gate, derived there): |got - truth| <= 2^-23 |truth| + c 2^-53 M_e.
Restatement against the recorded float64 reference: 2^-50 (M_e + 1) plus, where a softplus argument a exceeds 20, log1p(exp(-a))
-- the reference's softplus is the identity there, the restatement's is not (a stated departure).  The 1 beside M_e: lgamma
near its zeros at 1 and 2 is accurate to ulps of 1, not of its own value.
Sampler: every element of the host entry's output equals the restatement's draw, except elements whose decision margin the
restatement reports below 1e-9 -- of which the chosen seeds have none."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import countdist_inputs as CI  # noqa: E402
import countdist_restatement as CR  # noqa: E402
from distributed_vae_amd import _native as N  # noqa: E402
from distributed_vae_amd.nn_model import mk_vae  # noqa: E402
from distributed_vae_amd.utils import distributions as DS  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "countdist_kat.npz"))
CASES = [str(c) for c in G["cases"]]
MARGIN = 3.0
MARGIN_MIN = 1e-9


def fixture_arrays(name):
    return {k: G[f"{name}/{k}"] for k in ("x", "mu", "theta", "pi", "mu2", "theta2")}


# ---- 1. likelihoods ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fn", CI.LOGP_FUNCS)
@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_the_recorded_reference(name, fn):
    r = fixture_arrays(name)
    assert r["x"].dtype == np.float32 and (r["theta"].ndim == 1) == (name == "c1")
    truth, M = CI.logp_truth(fn, r)
    ref64 = G[f"{name}/{fn}/f64"]
    a = {k: v.astype(np.float64) for k, v in r.items()}
    gap = np.zeros_like(truth)
    if fn != "nb":                                   # the softplus arguments of the formula
        args = [-a["pi"]]
        if fn == "zinb":
            args.append(-a["pi"] + a["theta"] * (np.log(a["theta"] + 1e-8) - np.log(a["theta"] + a["mu"] + 1e-8)))
        for v in args:
            gap += np.where(v > 20.0, np.log1p(np.exp(-np.abs(v))), 0.0)
    err = np.abs(truth - ref64)
    print(f"\n  {name} {fn}: max |restatement - float64 reference| {err.max():.3e}, over the bound {float((err / (2.0 ** -50 * (M + 1) + gap)).max()):.3f}")
    assert truth.shape == ref64.shape and np.isfinite(truth).all()
    assert np.all(err <= 2.0 ** -50 * (M + 1) + gap)


@pytest.mark.parametrize("fn", CI.LOGP_FUNCS)
@pytest.mark.parametrize("shape,vec", [((65, 130), False), ((65, 130), True), ((1, 1), False)])
def test_host_terms_within_the_gate(shape, vec, fn):
    r = CI.regimes(*shape, seed=3, theta_vector=vec)
    kind, kw = CI.logp_args(fn, r)
    got = CI.host_logp(kind, **kw).astype(np.float64)
    truth, M = CI.logp_truth(fn, r)
    over = np.abs(got - truth) / CI.logp_gate(fn, truth, M).clip(1e-300)
    print(f"\n  {fn} {shape} vector {vec}: largest |got - truth| over the gate {float(over.max()):.3f}")
    assert np.isfinite(truth).all() and np.all(np.abs(got - truth) <= CI.logp_gate(fn, truth, M))


@pytest.mark.parametrize("fn", CI.LOGP_FUNCS)
@pytest.mark.parametrize("name", CASES)
def test_host_aggregate_against_the_recorded_float32_reference(name, fn):
    r = fixture_arrays(name)
    kind, kw = CI.logp_args(fn, r)
    got = CI.host_logp(kind, **kw).astype(np.float64)
    ref64, ref32 = G[f"{name}/{fn}/f64"], G[f"{name}/{fn}/f32"].astype(np.float64)
    scale = np.abs(ref64).mean()
    dev, cpu = np.abs(got - ref64).mean() / scale, np.abs(ref32 - ref64).mean() / scale
    print(f"\n  {name} {fn}: host entry {dev:.3e} | recorded float32 reference {cpu:.3e}")
    assert dev <= MARGIN * cpu


def test_zinb_branches_and_nan():
    x = np.array([[0.0, 1e-8, 3.0, np.nan, -1.0]], dtype=np.float32)
    one = np.ones_like(x)
    got = CI.host_logp("zinb", x, 2 * one, one, 0 * one)
    eps32 = float(np.float32(1e-8))
    assert got[0, 1] == 0.0 or eps32 != 1e-8        # float32(1e-8) is below 1e-8: the element takes the zero branch
    assert np.isnan(got[0, 3]) and np.isfinite(got[0, [0, 1, 2, 4]]).all()
    assert got[0, 0] == got[0, 4] == np.float32(CR.log_zinb(0.0, 2.0, 1.0, 0.0))
    # x == eps exactly (eps given as the float32 value): 0, as the reference's two masks give
    assert CI.host_logp("zinb", x, 2 * one, one, 0 * one, eps=eps32)[0, 1] == 0.0
    # the branch not selected is not evaluated: a zero-branch element whose non-zero branch is not finite
    assert np.isfinite(CI.host_logp("zinb", np.zeros((1, 1), np.float32), np.zeros((1, 1), np.float32), one[:, :1], one[:, :1], eps=0.0))


# ---- 2. the sampler against the restatement --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CI.SAMPLE_CASES))
def test_host_sampler_equals_the_restatement(name):
    case = CI.sample_case(name)
    ref = CI.restate_sample(case)
    low = ref["margin"] < MARGIN_MIN
    print(f"\n  {name}: {int(low.sum())} of {low.size} elements below the margin, {ref['exhausted']} exhausted, "
          f"{float(ref['calls'].mean()):.2f} Philox calls an element, largest draw {np.nanmax(ref['draw']):.0f}")
    assert int(low.sum()) == 0 and ref["exhausted"] == 0            # the seeds are chosen so
    got, exhausted = CI.host_sample(**case)
    assert exhausted == 0 and got.dtype == np.float32
    assert np.array_equal(got, CI.as_float32_draws(ref["draw"]))
    as_int, _ = CI.host_sample(**case, out_int32=True)
    assert as_int.dtype == np.int32 and np.array_equal(as_int.astype(np.float64), ref["draw"])
    logged, _ = CI.host_sample(**case, log1p=True)
    assert np.array_equal(logged, np.log1p(ref["draw"]).astype(np.float32))


def test_cases_cover_the_regimes():
    c = CI.sample_case("nb_65x130")
    mu, th = c["a"], c["b"]
    ref = CI.restate_sample(c)
    assert (th < 1e-5).any() and ((th > 0.2) & (th < 0.5)).any() and (th == 1).any() and (th > 5e3).any()
    assert (mu == 0).any() and ((mu > 0) & (mu < 10)).any() and ((mu > 10) & (mu < 20)).any() and (mu > 900).any()
    big = (mu == 1e9) & (th == 1e9)
    assert big.sum() == 4 and np.all(np.abs(ref["draw"][big] - 1e8) < 6e4)         # the 1e8 clamp: Poisson(1e8), sd 1e4
    assert np.all(ref["draw"][mu == 0] == 0)
    pi = CI.sample_case("zinb_logits_257x130")["zi"]
    assert (pi == 30).any() and (pi == -30).any() and (np.abs(pi) < 3).any()
    assert CI.SAMPLE_CASES["past_2^32"][4] * 130 > 1 << 32


def test_invalid_parameters_give_nan_without_a_loop():
    nan, inf = np.float32("nan"), np.float32("inf")
    mu = np.array([[nan, -1.0, 2.0, 2.0, inf, 2.0, 2.0, 0.0]], dtype=np.float32)
    th = np.array([[1.0, 1.0, 0.0, nan, 1.0, inf, 1.0, 1.0]], dtype=np.float32)
    zi = np.array([[0.0, 0.0, 0.0, 0.0, 0.0, 0.0, nan, 0.0]], dtype=np.float32)
    got, exhausted = CI.host_sample(mu, th, zi, "logits", seed=1)
    ref = CR.sample(mu, th, zi, "logits", seed=1)
    assert exhausted == 0 and np.isnan(got[0, :7]).all() and got[0, 7] == 0.0
    assert np.isnan(ref["draw"][0, :7]).all() and ref["draw"][0, 7] == 0.0 and int(ref["calls"].sum()) == 0
    as_int, _ = CI.host_sample(mu, th, zi, "logits", seed=1, out_int32=True)
    assert as_int.tolist() == [[-1] * 7 + [0]]


def test_batches_equal_one_call_and_keys_matter():
    case = CI.sample_case("zinb_logits_257x130")
    whole, _ = CI.host_sample(**case)
    parts = []
    for lo in range(0, 257, 100):
        sub = dict(case, a=case["a"][lo:lo + 100], b=case["b"][lo:lo + 100], zi=case["zi"][lo:lo + 100], cell0=case["cell0"] + lo)
        parts.append(CI.host_sample(**sub)[0])
    assert np.array_equal(np.concatenate(parts), whole, equal_nan=True)
    for change in (dict(seed=case["seed"] + 1), dict(offset=case["offset"] + 1), dict(cell0=case["cell0"] + 1),
                   dict(offset=case["offset"] + (1 << 32))):
        other, _ = CI.host_sample(**dict(case, **change))
        assert float((other != whole).mean()) > 0.2, change


# ---- 3. the sampler against the exact distribution -----------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(CI.SETTINGS)))
def test_draws_follow_the_exact_pmf(i):
    name, mu, theta, z = CI.SETTINGS[i]
    pmf = CR.zinb_pmf_table(mu, float(np.float32(theta)), z or 0.0)
    # the reference's own draws: the gate admits a correct sampler, and the pmf is right
    stat, dof = CR.pearson(G[f"{name}/values"], G[f"{name}/counts"], pmf)
    gate = CR.wilson_hilferty_gate(dof)
    print(f"\n  {name}: reference {stat:.1f}, dof {dof}, gate {gate:.1f}")
    assert int(G[f"{name}/counts"].sum()) == CI.N_DRAWS and dof >= 10 and stat <= gate
    n, D = CI.DRAW_SHAPE
    zi = None if z is None else np.full((n, D), np.float32(z))
    ref = CR.sample(np.full((n, D), np.float32(mu)), np.float32(theta), zi, None if z is None else "probs", seed=100 + i)
    got, exhausted = CI.host_sample(np.full((n, D), mu), np.full(D, theta), zi, None if z is None else "probs", seed=100 + i)
    assert exhausted == 0 and ref["exhausted"] == 0
    differ = got != ref["draw"].astype(np.float32)
    assert not (differ & (ref["margin"] >= MARGIN_MIN)).any() and int((ref["margin"] < MARGIN_MIN).sum()) <= n * D // 10_000
    for who, draws in (("restatement", ref["draw"]), ("host entry", got)):
        s, d = CR.pearson(*CR.histogram(draws), pmf)
        print(f"  {who} {s:.1f}, dof {d}; {float(ref['calls'].mean()):.2f} Philox calls an element")
        assert d == dof and s <= gate
    if z is not None:
        p0 = float(pmf[0])
        assert abs(float((got == 0).mean()) - p0) <= 6.0 * np.sqrt(p0 * (1.0 - p0) / (n * D))


def test_pmf_and_pearson_helpers():
    pmf = CR.zinb_pmf_table(3.0, 1.0)                                 # geometric with p = 1 / 4
    assert np.allclose(pmf[:4], 0.25 * 0.75 ** np.arange(4), rtol=1e-12) and abs(pmf.sum() - 1) < 1e-9
    assert np.isclose(CR.zinb_pmf_table(3.0, 1.0, 0.5)[0], 0.5 + 0.125)
    exact = np.round(4096 * pmf).astype(np.int64)
    stat, dof = CR.pearson(np.arange(pmf.size), exact, pmf)
    assert stat < 1.0 and dof > 5
    shifted, _ = CR.pearson(np.arange(pmf.size) + 1, exact, pmf)       # a sampler off by one fails the gate
    assert shifted > CR.wilson_hilferty_gate(dof)
    assert np.isclose(CR.wilson_hilferty_gate(100), 100 * (1 - 2 / 900 + 6 * np.sqrt(2 / 900)) ** 3)


# ---- 4. the C boundary -------------------------------------------------------------------------------------------------------------
PTR = 0x1000     # fake device pointers: every case must be refused before anything dereferences them
BAD, UNSUPPORTED, WORKSPACE = -1, -2, -4


def test_entry_points_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "mmvae.h")).read()
    for name in ("mmvae_count_logp", "mmvae_count_logp_workspace_bytes", "mmvae_count_sample", "mmvae_zinb_sample",
                 "mmvae_debug_count_logp_host", "mmvae_debug_count_sample_host"):
        assert name + "(" in hdr and hasattr(N.lib(), name), name
    assert N.lib().mmvae_abi_version() == 5 and N.ABI_VERSION == 5
    assert '"countdist.hip"' in open(os.path.join(ROOT, "distributed-vae_amd", "build.py")).read()
    for n, D in ((1, 1), (65, 130), (22365, 5032)):
        assert N.lib().mmvae_count_logp_workspace_bytes(n, D) == N.lib().mmvae_zinb_terms_workspace_bytes(n, D) > 0
    assert N.lib().mmvae_count_logp_workspace_bytes(0, 5) == 0


def _logp(**kw):
    import ctypes as C
    a = dict(kind=1, N=64, D=70, eps=1e-8, x=PTR, ldx=70, mu=PTR, ld_mu=70, theta=PTR, ld_theta=0, pi=PTR, ld_pi=70, mu2=PTR,
             ld_mu2=70, theta2=None, ld_theta2=0, terms=PTR, ld_t=70, cell_sum=PTR, gene_sum=PTR)
    call = dict(ws=PTR, ws_bytes=1 << 40)
    for k, v in kw.items():
        (call if k in call else a)[k] = v
    return N.lib().mmvae_count_logp(C.byref(N.CountLogp(**a)), call["ws"], call["ws_bytes"], None)


@pytest.mark.parametrize("kw,rc", [
    (dict(x=None), BAD), (dict(mu=None), BAD), (dict(theta=None), BAD), (dict(pi=None), BAD), (dict(kind=2, mu2=None), BAD),
    (dict(kind=3), BAD), (dict(kind=-1), BAD), (dict(N=0), BAD), (dict(D=0), BAD), (dict(ldx=69), BAD), (dict(ld_mu=69), BAD),
    (dict(ld_theta=69), BAD), (dict(ld_pi=69), BAD), (dict(ld_pi=0), BAD), (dict(kind=2, ld_mu2=69), BAD),
    (dict(kind=2, theta2=PTR, ld_theta2=1), BAD), (dict(ld_t=69), BAD), (dict(eps=-1e-8), BAD), (dict(eps=float("nan")), BAD),
    (dict(terms=None, cell_sum=None, gene_sum=None), BAD), (dict(gene_sum=None), BAD), (dict(ws=None), BAD), (dict(ws=PTR + 4), BAD),
    (dict(N=1 << 31, D=1 << 20, ldx=1 << 20, ld_mu=1 << 20, ld_pi=1 << 20, ld_t=1 << 20), UNSUPPORTED),
    (dict(ws_bytes=8 * (3 * 64 + 2 * 70) - 1), WORKSPACE)])
def test_count_logp_rejects_bad_arguments(kw, rc):
    assert _logp(**kw) == rc
    assert "count_logp" in N.lib().mmvae_last_error_string().decode()


def _sample(fused=False, **kw):
    import ctypes as C
    s = dict(param=1 if fused else 0, zi_kind=0 if fused else 1, N=64, D=70, cell0=0, eps=1e-6, seed=1, offset=0, a=PTR, ld_a=70,
             b=PTR, ld_b=0, zi=PTR, ld_zi=70, out_int32=0, log1p=0, out=PTR, ld_out=70, exhausted=PTR)
    call = dict(d10=PTR, ldh=100, H=100, W=PTR)
    for k, v in kw.items():
        (call if k in call else s)[k] = v
    st = C.byref(N.CountSample(**s))
    if fused:
        return N.lib().mmvae_zinb_sample(call["d10"], call["ldh"], call["H"], call["W"], PTR, PTR, PTR, PTR, PTR, st, None)
    return N.lib().mmvae_count_sample(st, None)


@pytest.mark.parametrize("kw,rc", [
    (dict(a=None), BAD), (dict(b=None), BAD), (dict(zi=None), BAD), (dict(out=None), BAD), (dict(exhausted=None), BAD),
    (dict(param=2), BAD), (dict(zi_kind=3), BAD), (dict(N=0), BAD), (dict(D=0), BAD), (dict(ld_a=69), BAD), (dict(ld_b=69), BAD),
    (dict(param=1, ld_b=0), BAD), (dict(ld_zi=69), BAD), (dict(ld_out=69), BAD), (dict(cell0=-1), BAD),
    (dict(cell0=(1 << 63) // 70), BAD), (dict(offset=1 << 56), BAD), (dict(out_int32=1, log1p=1), BAD),
    (dict(param=1, ld_b=70, eps=1.0), BAD)])
def test_count_sample_rejects_bad_arguments(kw, rc):
    assert _sample(**kw) == rc
    assert "count_sample" in N.lib().mmvae_last_error_string().decode()


@pytest.mark.parametrize("kw,rc", [
    (dict(d10=None), BAD), (dict(W=None), BAD), (dict(out=None), BAD), (dict(param=0), BAD), (dict(H=0), BAD), (dict(ldh=99), BAD),
    (dict(offset=1 << 56), BAD), (dict(eps=-1.0), BAD), (dict(H=129, ldh=129), UNSUPPORTED),
    (dict(N=1 << 31, D=1 << 20, ld_out=1 << 20), UNSUPPORTED)])
def test_zinb_sample_rejects_bad_arguments(kw, rc):
    assert _sample(fused=True, **kw) == rc
    assert "zinb_sample" in N.lib().mmvae_last_error_string().decode()


# ---- 5. the Python surface without a device --------------------------------------------------------------------------------------
def test_cpu_tensors_are_refused():
    t = torch.ones(3, 5)
    for call in (lambda: DS.log_nb_positive(t, t, t), lambda: DS.log_zinb_positive(t, t, t, t),
                 lambda: DS.log_mixture_nb(t, t, t, t, None, t), lambda: DS.NegativeBinomial(mu=t, theta=t),
                 lambda: DS.ZeroInflatedNegativeBinomial(mu=t, theta=t, zi_logits=t),
                 lambda: DS.NegativeBinomialMixture(t, t, t, t), lambda: N.count_sample(t, t),
                 lambda: N.count_logp("nb", t, t, t)):
        with pytest.raises(N.NativeError):
            call()
    with pytest.raises(ValueError):
        DS.NegativeBinomial(mu=t, theta=t, total_count=t)
    with pytest.raises(ValueError):
        DS.NegativeBinomial()
    with pytest.raises(ValueError):
        DS.log_nb_positive(t, t, t, reduce="mean")
    with pytest.raises(NotImplementedError, match="not built"):
        DS.NegativeBinomialMixture.sample(object.__new__(DS.NegativeBinomialMixture))
    tc, lg = DS._convert_mean_disp_to_counts_logits(t * 3, t * 2, eps=0.0)
    mu, theta = DS._convert_counts_logits_to_mean_disp(tc, lg)
    assert torch.allclose(mu, t * 3) and torch.equal(theta, t * 2)
    with pytest.raises(ValueError):
        DS._convert_mean_disp_to_counts_logits(t, None)


def test_model_surface_refusals_without_a_device():
    mse, z = (mk_vae(7, 2, 64, "cpu", fc_dim=16, latent_dim=5, mode=m).eval() for m in ("MSE", "ZINB"))
    c, s, h = torch.zeros(3, 7), torch.zeros(3, 2), torch.zeros(3, 64)
    for call in (lambda: mse.sample_zinb(c, s, 0, seed=1), lambda: mse.zinb_distribution(h, h, h),
                 lambda: mse.zinb_sample_batch(torch.zeros(2, 3, 64), seed=1)):
        with pytest.raises(RuntimeError, match="loss_mode='ZINB'"):
            call()
    with pytest.raises(IndexError):
        z.sample_zinb(c, s, 2, seed=1)
    with pytest.raises(N.NativeError):
        z.sample_zinb(c, s, 0, seed=1)
    with pytest.raises(N.NativeError):
        z.zinb_distribution(h, h, h)
    z.train()
    with pytest.raises(RuntimeError, match="eval"):
        z.zinb_sample_batch(torch.zeros(2, 3, 64), seed=1)

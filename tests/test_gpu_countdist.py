"""GPU: the count distributions on the HIP engine -- mmvae_count_logp, mmvae_count_sample, mmvae_zinb_sample
(csrc/countdist.hip) and what is built on them: distributed_vae_amd.utils.distributions, mixVAE_model.zinb_distribution /
sample_zinb / zinb_sample_batch, cpl_mixVAE.sample_counts -- against tests/countdist_restatement.py (held to the reference's
recorded returns and to the library's own element code on the host by tests/test_countdist_cpu.py) and the reference's outputs
recorded in tests/golden/countdist_kat.npz.  Nothing here reads the reference.

Shapes: 65 x 130 and 257 x 130 (tiles of 64 x 64, sub-tiles of 32 x 32), 1 x 1, every matrix given with a row pitch larger than
its width, theta as [N, D] and as [D], logical element indices past 2^32 through cell0.  The inputs cover the regimes listed in
tests/countdist_inputs.py.  The gates are those of tests/test_countdist_cpu.py; every figure is printed (pytest -s)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import countdist_inputs as CI  # noqa: E402
import countdist_restatement as CR  # noqa: E402
import zinb_restatement as ZR  # noqa: E402
from gpu_util import DEV  # noqa: E402
from distributed_vae_amd import _native as N  # noqa: E402
from distributed_vae_amd.nn_model import mixVAE_model  # noqa: E402
from distributed_vae_amd.utils import distributions as DS  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "countdist_kat.npz"))
GZ = np.load(os.path.join(ROOT, "tests", "golden", "zinb_kat.npz"))
MARGIN = 3.0
MARGIN_MIN = 1e-9


def pitched(a, pad=3):
    """numpy [n, w] (or a vector, which goes up as it is) on the device as rows of a wider matrix, the pad filled with NaN."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if t.dim() == 1:
        return t.to(DEV)
    buf = torch.full((t.shape[0], t.shape[1] + pad), float("nan"), dtype=t.dtype, device=DEV)
    buf[:, :t.shape[1]] = t.to(DEV)
    return buf[:, :t.shape[1]]


@functools.lru_cache(maxsize=None)
def logp_case(shape, vec, fn):
    """One case's inputs, truth and M_e (CPU, once) and the device's terms and sums."""
    r = CI.regimes(*shape, seed=3, theta_vector=vec)
    kind, kw = CI.logp_args(fn, r)
    truth, M = CI.logp_truth(fn, r)
    dev = {k: pitched(v) for k, v in kw.items()}
    terms, cell, gene = N.count_logp(kind, return_terms=True, return_sums=True, **dev)
    return dict(kind=kind, dev=dev, truth=truth, M=M, terms=terms, cell=cell, gene=gene)


# ---- 1. likelihoods ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fn", CI.LOGP_FUNCS)
@pytest.mark.parametrize("shape,vec", [((65, 130), False), ((257, 130), True), ((1, 1), False)])
def test_terms_within_the_gate_and_sums(shape, vec, fn):
    c = logp_case(shape, vec, fn)
    n, D = shape
    got = c["terms"].cpu().numpy().astype(np.float64)
    assert c["terms"].dtype == torch.float32 and got.shape == shape and np.isfinite(c["truth"]).all()
    gate = CI.logp_gate(fn, c["truth"], c["M"])
    over = np.abs(got - c["truth"]) / gate.clip(1e-300)
    print(f"\n  {fn} {shape} vector {vec}: largest |got - truth| over the gate {float(over.max()):.3f} (c = {CI.C_OPS[fn]:.0f})")
    assert np.all(np.abs(got - c["truth"]) <= gate)
    # the sums against the fp64 sums of fp64 terms: each term carries its gate's second part, the sum (n + 2) roundings
    cell, gene = c["cell"].cpu().numpy(), c["gene"].cpu().numpy()
    assert cell.dtype == gene.dtype == np.float64 and cell.shape == (n,) and gene.shape == (D,)
    t64 = c["truth"]
    for got_s, axis, m in ((cell, 1, D), (gene, 0, n)):
        bound = (m + 2) * 2.0 ** -53 * np.abs(t64).sum(axis) + CI.C_OPS[fn] * 2.0 ** -53 * c["M"].sum(axis)
        assert np.all(np.abs(got_s - t64.sum(axis)) <= bound)
    # sums only: no N x D output, the same bits
    _, cell2, gene2 = N.count_logp(c["kind"], return_terms=False, return_sums=True, **c["dev"])
    assert torch.equal(cell2, c["cell"]) and torch.equal(gene2, c["gene"])
    terms3, none_c, none_g = N.count_logp(c["kind"], return_terms=True, return_sums=False, **c["dev"])
    assert none_c is None and none_g is None and torch.equal(terms3, c["terms"])


@pytest.mark.parametrize("fn", CI.LOGP_FUNCS)
def test_sums_of_the_devices_own_terms(fn):
    """The sums within (n + 2) 2^-53 sum |term| of the fp64 sum of the device's own terms.  The device's own fp64 terms are
    read without a rounding to float32: the cell sums of one column alone are that column's terms (0.0 + t, and the other
    lanes' exact zeros)."""
    c = logp_case((257, 130), True, fn)
    cols = []
    for j in range(130):
        one = {k: (v[j:j + 1] if v.dim() == 1 else v[:, j:j + 1]) for k, v in c["dev"].items()}
        cols.append(N.count_logp(c["kind"], return_terms=False, return_sums=True, **one)[1])
    T = torch.stack(cols, dim=1)
    assert T.dtype == torch.float64 and torch.equal(T.float(), c["terms"])
    t = T.cpu().numpy()
    for got_s, axis, m in ((c["cell"].cpu().numpy(), 1, 130), (c["gene"].cpu().numpy(), 0, 257)):
        assert np.all(np.abs(got_s - t.sum(axis)) <= (m + 2) * 2.0 ** -53 * np.abs(t).sum(axis))


@pytest.mark.parametrize("fn", CI.LOGP_FUNCS)
@pytest.mark.parametrize("name", [str(c) for c in G["cases"]])
def test_aggregate_against_the_recorded_float32_reference(name, fn):
    r = {k: G[f"{name}/{k}"] for k in ("x", "mu", "theta", "pi", "mu2", "theta2")}
    kind, kw = CI.logp_args(fn, r)
    got = N.count_logp(kind, **{k: pitched(v) for k, v in kw.items()})[0].double().cpu().numpy()
    ref64, ref32 = G[f"{name}/{fn}/f64"], G[f"{name}/{fn}/f32"].astype(np.float64)
    scale = np.abs(ref64).mean()
    dev, cpu = np.abs(got - ref64).mean() / scale, np.abs(ref32 - ref64).mean() / scale
    print(f"\n  {name} {fn}: device {dev:.3e} | recorded float32 reference {cpu:.3e}")
    assert dev <= MARGIN * cpu


def test_likelihood_runs_are_bit_identical_and_a_cell_stands_alone():
    for fn in CI.LOGP_FUNCS:
        c = logp_case((257, 130), True, fn)
        again = N.count_logp(c["kind"], return_terms=True, return_sums=True, **c["dev"])
        assert torch.equal(again[0], c["terms"]) and torch.equal(again[1], c["cell"]) and torch.equal(again[2], c["gene"])
        among65 = N.count_logp(c["kind"], return_sums=True, **{k: (v if v.dim() == 1 else v[:65]) for k, v in c["dev"].items()})
        for i in (0, 5, 37, 64):
            alone = N.count_logp(c["kind"], return_sums=True, **{k: (v if v.dim() == 1 else v[i:i + 1]) for k, v in c["dev"].items()})
            assert torch.equal(alone[1][0], among65[1][i]) and torch.equal(alone[1][0], c["cell"][i]), (fn, i)
            assert torch.equal(alone[0][0], c["terms"][i])


def test_distribution_functions_and_classes():
    r = CI.regimes(65, 130, seed=3)
    d = {k: torch.from_numpy(v).to(DEV) for k, v in r.items()}
    x, mu, th, pi = d["x"], d["mu"], d["theta"], d["pi"]
    nb = DS.log_nb_positive(x, mu, th)
    assert nb.dtype == torch.float32 and nb.shape == x.shape and torch.equal(nb, N.count_logp("nb", x, mu, th)[0])
    assert torch.equal(DS.log_nb_positive(x, mu, th[0]), DS.log_nb_positive(x, mu, th[0].expand(65, -1)))     # theta [D]
    sums = DS.log_zinb_positive(x, mu, th, pi, reduce="sums")
    assert sorted(sums) == ["cell", "gene"] and sums["cell"].dtype == torch.float64 and sums["cell"].shape == (65,)
    z = DS.ZeroInflatedNegativeBinomial(mu=mu, theta=th, zi_logits=pi)
    assert torch.equal(z.log_prob(x), DS.log_zinb_positive(x, mu, th, pi)) and torch.equal(z.zi_probs, torch.sigmoid(pi))
    assert torch.equal(z.mean, (1 - torch.sigmoid(pi)) * mu)
    with pytest.raises(NotImplementedError):
        z.variance
    n1 = DS.NegativeBinomial(mu=mu, theta=th)
    assert torch.equal(n1.mean, mu) and torch.equal(n1.variance, mu + mu ** 2 / th) and torch.equal(n1.log_prob(x), nb)
    n2 = DS.NegativeBinomial(total_count=th, logits=torch.log(mu + 1.0) - torch.log(th))      # the other parameterisation
    assert torch.allclose(n2.mu, mu + 1.0, rtol=1e-5) and torch.equal(n2.theta, th)
    n3 = DS.NegativeBinomial(total_count=th, probs=torch.full_like(th, 0.75))
    assert torch.allclose(n3.mu, 3 * th, rtol=1e-5)
    m = DS.NegativeBinomialMixture(mu, d["mu2"], th, pi, theta2=d["theta2"])
    assert torch.equal(m.log_prob(x), DS.log_mixture_nb(x, mu, d["mu2"], th, d["theta2"], pi))
    assert torch.equal(m.mixture_probs, torch.sigmoid(pi)) and m.mean.shape == x.shape
    with pytest.raises(NotImplementedError, match="not built"):
        m.sample()
    # draws: the shape, reproducibility through torch's generator, sample_shape as further rows of the logical matrix
    small = DS.ZeroInflatedNegativeBinomial(mu=mu[:5], theta=th[:5], zi_probs=torch.sigmoid(pi[:5]))
    torch.manual_seed(11)
    a = small.sample((2, 3))
    torch.manual_seed(11)
    b = small.sample((2, 3))
    assert a.shape == (2, 3, 5, 130) and a.dtype == torch.float32 and torch.equal(a, b) and not torch.equal(a[0, 0], a[0, 1])
    assert torch.equal(small.sample(seed=9), small.sample(seed=9)) and not torch.equal(small.sample(seed=9), small.sample(seed=10))
    assert torch.equal(small.sample(seed=9, offset=4), N.count_sample(mu[:5], th[:5], torch.sigmoid(pi[:5]), "probs", seed=9, offset=4))
    # refusals
    with pytest.raises(ValueError):
        DS.log_nb_positive(x, mu[:, :100], th)
    with pytest.raises(ValueError):
        N.count_logp("nb", x, mu[:40], th)
    with pytest.raises(N.NativeError):
        DS.log_nb_positive(x, mu.cpu(), th)
    with pytest.raises(N.NativeError):
        N.count_sample(mu, th.cpu())
    assert N.lib().mmvae_abi_version() == 5


# ---- 2. the sampler against the restatement --------------------------------------------------------------------------------------
def _device_sample(case, **more):
    kw = {k: case[k] for k in ("zi_kind", "seed", "offset", "cell0", "heads_eps")}
    zi = None if case["zi"] is None else pitched(case["zi"])
    return N.count_sample(pitched(case["a"]), pitched(case["b"]), zi, **kw, **more)


@pytest.mark.parametrize("name", list(CI.SAMPLE_CASES))
def test_sampler_equals_the_restatement(name):
    case = CI.sample_case(name)
    ref = CI.restate_sample(case)
    low = ref["margin"] < MARGIN_MIN
    got = _device_sample(case)                                      # (raises if the exhaustion counter is not 0)
    want = CI.as_float32_draws(ref["draw"])
    differ = ~((got.cpu().numpy() == want) | (np.isnan(want) & np.isnan(got.cpu().numpy())))
    print(f"\n  {name}: {int(differ.sum())} of {differ.size} elements differ from the restatement; {int(low.sum())} below the margin; "
          f"{float(ref['calls'].mean()):.2f} Philox calls an element")
    assert got.dtype == torch.float32 and int(low.sum()) <= low.size // 10_000
    assert not (differ & ~low).any()
    as_int = _device_sample(case, out_int32=True)
    assert as_int.dtype == torch.int32 and torch.equal(as_int.float(), got)
    assert torch.equal(_device_sample(case, log1p=True), torch.log1p(got.double()).float())
    assert torch.equal(_device_sample(case), got)                   # run to run


def test_invalid_parameters_give_nan():
    nan, inf = float("nan"), float("inf")
    mu = torch.tensor([[nan, -1.0, 2.0, 2.0, inf, 2.0, 2.0, 0.0]], device=DEV)
    th = torch.tensor([[1.0, 1.0, 0.0, nan, 1.0, inf, 1.0, 1.0]], device=DEV)
    zi = torch.tensor([[0.0, 0.0, 0.0, 0.0, 0.0, 0.0, nan, 0.0]], device=DEV)
    got = N.count_sample(mu, th, zi, "logits", seed=1)
    assert bool(torch.isnan(got[0, :7]).all()) and float(got[0, 7]) == 0.0
    assert N.count_sample(mu, th, zi, "logits", seed=1, out_int32=True).tolist() == [[-1] * 7 + [0]]
    lp = DS.log_zinb_positive(torch.tensor([[nan, 0.0]], device=DEV), mu[:, 2:4] * 0 + 2, th[:, :2], zi[:, :2])
    assert bool(torch.isnan(lp[0, 0])) and bool(torch.isfinite(lp[0, 1]))


def test_batches_equal_one_call_and_keys_matter():
    case = CI.sample_case("zinb_logits_257x130")
    whole = _device_sample(case)
    parts = []
    for lo in range(0, 257, 100):
        sub = dict(case, a=case["a"][lo:lo + 100], b=case["b"][lo:lo + 100], zi=case["zi"][lo:lo + 100], cell0=case["cell0"] + lo)
        parts.append(_device_sample(sub))
    assert torch.equal(torch.cat(parts), whole)
    for change in (dict(seed=case["seed"] + 1), dict(offset=case["offset"] + 1), dict(offset=case["offset"] + (1 << 32))):
        assert float((_device_sample(dict(case, **change)) != whole).float().mean()) > 0.2, change


# ---- 3. the sampler against the exact distribution -----------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(CI.SETTINGS)))
def test_draws_follow_the_exact_pmf(i):
    name, mu, theta, z = CI.SETTINGS[i]
    n, D = CI.DRAW_SHAPE
    pmf = CR.zinb_pmf_table(mu, float(np.float32(theta)), z or 0.0)
    zi = None if z is None else torch.full((n, D), z, device=DEV)
    got = N.count_sample(torch.full((n, D), mu, device=DEV), torch.full((D,), theta, device=DEV), zi, None if z is None else "probs",
                         seed=100 + i).cpu().numpy()
    stat, dof = CR.pearson(*CR.histogram(got), pmf)
    gate = CR.wilson_hilferty_gate(dof)
    print(f"\n  {name}: Pearson {stat:.1f}, dof {dof}, gate {gate:.1f}")
    assert got.size == CI.N_DRAWS and dof >= 10 and stat <= gate
    if z is not None:
        p0 = float(pmf[0])
        assert abs(float((got == 0).mean()) - p0) <= 6.0 * np.sqrt(p0 * (1.0 - p0) / got.size)


# ---- 4. the fused form and the model ---------------------------------------------------------------------------------------------
def _fixture_model(name, mode="ZINB"):
    sd = {k[len(name) + 4:]: torch.from_numpy(np.asarray(GZ[k])) for k in GZ.files if k.startswith(f"{name}/sd/")}
    sd = {k: (v.float() if v.is_floating_point() else v) for k, v in sd.items()}
    if mode != "ZINB":
        sd = {k: v for k, v in sd.items() if not k.startswith(("fc11_p.", "fc11_r."))}
    A, _, D, H, L, Cc, S = [int(v) for v in GZ[f"{name}/cfg"]]
    m = mixVAE_model(input_dim=D, fc_dim=H, n_categories=Cc, state_dim=S, lowD_dim=L, x_drop=0.5, s_drop=0.2, n_arm=A, lam=1,
                     lam_pc=1, tau=0.005, beta=1.0, hard=False, variational=True, device=DEV, eps=1e-8, momentum=0.01,
                     ref_prior=False, loss_mode=mode)
    m.load_state_dict(sd)
    return m.to(DEV).eval()


@pytest.mark.parametrize("name", [str(c) for c in GZ["cases"]])
def test_sample_zinb_equals_heads_then_count_sample(name):
    m = _fixture_model(name)
    A = m.n_arm
    for a in range(A):
        c = torch.from_numpy(GZ[f"{name}/c"][a]).float().to(DEV)
        s = torch.from_numpy(GZ[f"{name}/s"][a]).float().to(DEV)
        heads = m.decoder_zinb(c, s, a)
        for kw in (dict(seed=5), dict(seed=5, offset=9, cell0=1 << 33), dict(seed=6, log1p=True)):
            got = m.sample_zinb(c, s, a, **kw)
            want = N.count_sample(*heads, heads_eps=1e-6, **kw)
            assert got.dtype == torch.float32 and got.shape == heads[0].shape and torch.equal(got, want), (a, kw)
        assert float((m.sample_zinb(c, s, a, seed=5) > 0).float().mean()) > 0.02
        # the distribution object of the same heads: parameters one float32 rounding from the fp64 mapping
        dist = m.zinb_distribution(*heads)
        mu, th, z = CR.heads_to_params(*(h.cpu().numpy() for h in heads))
        for t, v in ((dist.mu, mu), (dist.theta, th), (dist.zi_probs, z)):
            assert np.all(np.abs(t.double().cpu().numpy() - v) <= 2.0 ** -24 * np.abs(v))


@pytest.mark.parametrize("n,D,H", [(65, 130, 128), (257, 130, 128), (1, 1, 1)])
def test_zinb_sample_equals_heads_then_count_sample_on_tile_edges(n, D, H):
    """fc11 and d10 are integer-valued with sums far below 2^24, so the fused kernel's fp32 chain for x_rec is exact and
    relu(d10 W^T + b) computed in fp64 on the host is the float32 x_rec bit for bit; the two gates come from
    mmvae_zinb_heads, whose rounding the fused kernel must repeat."""
    g = torch.Generator().manual_seed(1000 * n + 10 * D + H)
    d10 = torch.randint(0, 4, (n, H), generator=g).float()
    spread = ZR.spread_layers(d10, D, g)
    W = torch.randint(-2, 3, (D, H), generator=g).float()
    b = torch.randint(-3, 4, (D,), generator=g).float()
    x_rec = torch.relu(d10.double() @ W.double().t() + b.double()).float()
    assert float(x_rec.max()) < 2 ** 20 and bool((x_rec == 0).any() or n * D < 4)
    L = [W.to(DEV), b.to(DEV)] + [t.to(DEV) for t in spread[2:]]
    d10 = pitched(d10.numpy())
    x_p, x_r = N.zinb_heads(d10, *L[2:])
    for kw in (dict(seed=3, offset=1, cell0=7), dict(seed=4, cell0=1 << 34, log1p=True), dict(seed=3, out_int32=True)):
        got = N.zinb_sample(d10, *L, **kw)
        want = N.count_sample(x_rec.to(DEV), x_p, x_r, heads_eps=1e-6, **kw)
        assert got.shape == (n, D) and torch.equal(got, want), kw
    whole = N.zinb_sample(d10, *L, seed=3, offset=1, cell0=7)
    rows = torch.cat([N.zinb_sample(d10[i:i + 64], *L, seed=3, offset=1, cell0=7 + i) for i in range(0, n, 64)])
    assert torch.equal(rows, whole)


def test_log_prob_of_the_models_distribution_is_the_zinb_term():
    """zinb_distribution(...).log_prob(k) + lgamma(k + 1) = -(the term of zinb_loss), as a statement about the two formulas at
    the same parameter values: the truth is -(zinb term) in fp64 at r = theta, p = mu / (mu + theta), z = the distribution's own
    float32 parameters (one rounding from the heads' fp64 mapping, checked in test_sample_zinb_equals_heads_then_count_sample).
    Compared: the elements away from the eps guards of both formulas -- log_prob's eps = 1e-8 inside its three logarithms moves
    the value by at most E = 1e-8 (mu / (theta + mu) + k / mu + k / (theta + mu)) (first order), and an element is compared
    where E is below a quarter of its gate; the gate is the zinb one with truth and M_e of log_zinb_positive."""
    name = str(GZ["cases"][0])
    m = _fixture_model(name)
    c = torch.from_numpy(GZ[f"{name}/c"][0]).float().to(DEV)
    s = torch.from_numpy(GZ[f"{name}/s"][0]).float().to(DEV)
    dist = m.zinb_distribution(*m.decoder_zinb(c, s, 0))
    X = torch.from_numpy(GZ[f"{name}/X"]).to(DEV)
    k = torch.round(torch.expm1(X.double())).float()
    got = (dist.log_prob(k).double() + torch.lgamma(k.double() + 1.0)).cpu().numpy()
    mu, th, zp = (t.double().cpu().numpy() for t in (dist.mu, dist.theta, dist.zi_probs))
    kk = k.double().cpu().numpy()
    lgam = CR.lgamma
    p, q = mu / (mu + th), th / (mu + th)
    truth = np.where(kk > 0, lgam(kk + th) - lgam(th) + kk * np.log(p) + th * np.log(q) + np.log1p(-zp),
                     np.log(zp + (1.0 - zp) * np.exp(th * np.log(q))))
    pi = np.log(zp) - np.log1p(-zp)
    lp_truth, M = CR.log_zinb(kk, mu, th, pi), CR.magnitudes_zinb(kk, mu, th, pi)
    gate = CI.logp_gate("zinb", lp_truth, M + np.abs(lgam(kk + 1.0))) + 2.0 ** -23 * np.abs(pi)     # pi reaches log_prob as float32
    E = 1e-8 * (mu / (th + mu) + kk / mu + kk / (th + mu))
    use = E <= 0.25 * gate
    print(f"\n  {int(use.sum())} of {use.size} elements compared; largest |got - truth| over the gate "
          f"{float((np.abs(got - truth)[use] / gate[use]).max()):.3f}")
    assert use.mean() > 0.5 and np.all(np.abs(got - truth)[use] <= gate[use] + E[use])


def test_sample_counts_on_a_device_loader():
    from distributed_vae_amd.cpl_mixvae import cpl_mixVAE
    from distributed_vae_amd.utils.dataloader import DeviceLoader
    Dm, Cc, S, A, n_all, n, B = 130, 5, 2, 2, 200, 150, 64
    torch.manual_seed(4)
    t = cpl_mixVAE(saving_folder="", device=0, save_flag=False)
    t.init_model(n_categories=Cc, state_dim=S, input_dim=Dm, fc_dim=20, lowD_dim=6, x_drop=0.5, s_drop=0.2, n_arm=A, temp=1.0,
                 tau=0.005, mode="ZINB")
    m = t.model
    data = ZR.counts_matrix(n_all, Dm, torch.Generator().manual_seed(8)).to(DEV)
    index = torch.from_numpy(np.random.default_rng(2).permutation(n_all)[:n])
    u = torch.rand(A, n, S, generator=torch.Generator().manual_seed(9)).to(DEV)
    batches = lambda: m.set_explicit_noise([{"u_state": u[:, i:i + B].contiguous()} for i in range(0, n, B)])   # noqa: E731
    batches()
    got = t.sample_counts(DeviceLoader(data, index, B, False, False), seed=21)
    assert sorted(got) == ["counts", "data_indx"] and got["counts"].shape == (A, n, Dm) and got["counts"].dtype == np.float32
    assert np.array_equal(got["data_indx"].astype(np.int64), index.numpy()) and m.training          # order kept, mode restored
    assert np.all(got["counts"] >= 0) and np.all(got["counts"] == np.round(got["counts"])) and (got["counts"] > 0).any()
    batches()
    one_arm = t.sample_counts(DeviceLoader(data, index, B, False, False), seed=21, arm=1, log1p=True)
    assert one_arm["counts"].shape == (1, n, Dm)
    assert np.array_equal(one_arm["counts"][0], np.log1p(got["counts"][1].astype(np.float64)).astype(np.float32))
    # the batches of 64 against one call at the same per-cell draws of the forward: the same counts, keyed by position
    m.eval()
    m.set_explicit_noise({"u_state": u})
    x = data[index.to(DEV)]
    one = m.zinb_sample_batch(x.expand(A, -1, -1), 21, t.temp)
    assert np.array_equal(one.cpu().numpy(), got["counts"])
    out = m(x.expand(A, -1, -1), t.temp, eval=True)
    m.set_explicit_noise({"u_state": u})
    for a in range(A):
        want = N.count_sample(out[0][a], out[1][a], out[2][a], heads_eps=1e-6, seed=21)
        assert torch.equal(one[a], want), a
    m.set_explicit_noise(None)
    with pytest.raises(ValueError):
        t.sample_counts(DeviceLoader(data, index, B, False, False), seed=1, arm=2)
    mse = cpl_mixVAE(saving_folder="", device=0, save_flag=False)
    mse.init_model(n_categories=Cc, state_dim=S, input_dim=Dm, fc_dim=20, lowD_dim=6, n_arm=A)
    with pytest.raises(RuntimeError, match="loss_mode='ZINB'"):
        mse.sample_counts(DeviceLoader(data, index, B, False, False), seed=1)
    with pytest.raises(RuntimeError, match="loss_mode='ZINB'"):
        _fixture_model(str(GZ["cases"][0]), "MSE").sample_zinb(torch.zeros(2, 6, device=DEV), torch.zeros(2, 2, device=DEV), 0, seed=1)

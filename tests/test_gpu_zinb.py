"""GPU: ZINB inference on the HIP engine -- mmvae_zinb_heads, mmvae_zinb_nll, mmvae_zinb_terms (csrc/zinb.hip) and what is
built on them: mixVAE_model.decoder_zinb / forward(eval=True) / zinb_nll, nn_model.zinb_loss, cpl_mixVAE.score_zinb --
against tests/zinb_restatement.py (pinned to the live reference by tests/test_zinb_cpu.py) and the reference's own outputs
recorded in tests/golden/zinb_kat.npz.  Nothing here reads the reference.

Shapes: N in {1, 63, 65, 257}, D in {1, 31, 33, 130}, H in {1, 7, 100, 128} in eight combinations (tiles of 64 x 64, sub-tiles
of 32 x 32, k = 2); every matrix the kernels read is given with a row pitch larger than its width; X = log1p(counts), counts
<= 1000, about 70 % zeros, row 0 all zero and row 1 all positive; the gates' pre-activations spread to +-8 and stay within.

Error rule of the terms and sums (the issue's): the statistic is |value - fp64| / M, its maximum and 90th percentile, M the sum
of the magnitudes of the term's addends in fp64 (summed over the reduced elements for cell_sum and gene_sum); the reference's
arithmetic in float32 on the CPU is measured with the same statistic on the same inputs in the same run, and the device must
stay within 3 x that.  Both figures are printed per case (pytest -s) and are in DESIGN.md section 9k."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import zinb_restatement as ZR  # noqa: E402
from gpu_util import DEV  # noqa: E402
from distributed_vae_amd import _native as N  # noqa: E402
from distributed_vae_amd import nn_model as NM  # noqa: E402
from distributed_vae_amd.nn_model import mixVAE_model  # noqa: E402

pytestmark = pytest.mark.gpu

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "zinb_kat.npz"))
FIXTURES = [str(c) for c in G["cases"]]
SHAPES = [(1, 1, 1), (63, 31, 7), (65, 33, 100), (257, 130, 128), (257, 31, 100), (1, 130, 7), (63, 1, 128), (65, 130, 1)]
MARGIN = 3.0
U32 = 2.0 ** -24


def pitched(t, pad=3):
    """``t`` [n, w] on the device as rows of a wider matrix: row pitch w + pad, the pad filled with NaN."""
    buf = torch.full((t.shape[0], t.shape[1] + pad), float("nan"), dtype=t.dtype, device=DEV)
    buf[:, :t.shape[1]] = t.to(DEV)
    v = buf[:, :t.shape[1]]
    assert v.stride(0) == t.shape[1] + pad
    return v


@functools.lru_cache(maxsize=None)
def case(n, D, H):
    """One shape's inputs and everything the CPU computes from them, once."""
    g = torch.Generator().manual_seed(1000 * n + 10 * D + H)
    d10 = torch.relu(torch.randn(n, H, generator=g))
    if not bool((d10 > 0).any()):
        d10[0, 0] = 0.75
    L = ZR.spread_layers(d10, D, g)
    X = ZR.counts_matrix(n, D, g)
    L64 = [t.double() for t in L]
    for a in ZR.pre_activations(d10.double(), *L64[2:]):
        assert float(a.abs().max()) <= 8.0
    h64 = ZR.heads(d10.double(), *L64)
    h32 = ZR.heads(d10, *L)
    c = {"d10": d10, "L": L, "X": X, "h32": h32,
         "t64": ZR.terms(*h64, X.double()), "M": ZR.magnitudes(*h64, X), "t32": ZR.terms(*h32, X),
         # given heads: the truth is the fp64 term of the SAME float32 heads
         "g64": ZR.terms(*(h.double() for h in h32), X.double()), "gM": ZR.magnitudes(*h32, X)}
    assert bool(torch.isfinite(c["t32"]).all()) and bool(torch.isfinite(c["t64"]).all())
    return c


def within(name, dev, cpu):
    print(f"    {name:<12} device max {dev[0]:.3e} p90 {dev[1]:.3e} | reference float32 max {cpu[0]:.3e} p90 {cpu[1]:.3e}")
    return dev[0] <= MARGIN * cpu[0] and dev[1] <= MARGIN * cpu[1]


# ---- 1. lane maps, exactly ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,D,H", [(65, 33, 7), (63, 31, 1), (257, 130, 100)])
def test_heads_lane_maps_exact(n, D, H):
    """d10 in multiples of 1/4, weights in multiples of 1/16 and biases in multiples of 1/64, all small: every product and
    every partial sum is a multiple of 2^-6 below 2^10, exact in float32, so the pre-activation is exact whatever the order.
    x_p, x_r are then the float32 roundings of the fp64 sigmoid of it: within 1 ulp (the kernel rounds once: 0.5 ulp, and the
    fp64 sigmoid here and there may differ in its last bits).  The weights are random, hence asymmetric; H = 7 and 1 are no
    multiples of the instruction's k = 2."""
    g = torch.Generator().manual_seed(n + D + H)
    d10 = torch.randint(-3, 4, (n, H), generator=g).float() / 4
    Wp, Wr = (torch.randint(-5, 6, (D, H), generator=g).float() / 16 for _ in range(2))
    bp, br = (torch.randint(-40, 41, (D,), generator=g).float() / 64 for _ in range(2))
    k = min(D, H)
    assert k == 1 or not torch.equal(Wp[:k, :k], Wp[:k, :k].T)
    x_p, x_r = N.zinb_heads(pitched(d10), Wp.to(DEV), bp.to(DEV), Wr.to(DEV), br.to(DEV))
    assert x_p.shape == (n, D) and x_p.dtype == torch.float32
    for got, W, b in ((x_p, Wp, bp), (x_r, Wr, br)):
        a = d10.double() @ W.double().T + b.double()              # exact
        assert torch.equal(a, (d10 @ W.T + b).double())         # (float32 on the CPU is exact on these too)
        want = torch.sigmoid(a)
        ulp = torch.from_numpy(np.spacing(want.float().numpy())).double()
        err = (got.cpu().double() - want).abs()
        assert bool((err <= ulp).all()), float((err / ulp).max())
        assert float(a.abs().max()) > 0.5


# ---- 2. decoder_zinb -----------------------------------------------------------------------------------------------------------
def _fixture_model(name, mode="ZINB"):
    sd = {k[len(name) + 4:]: torch.from_numpy(np.asarray(G[k])) for k in G.files if k.startswith(f"{name}/sd/")}
    sd = {k: (v.float() if v.is_floating_point() else v) for k, v in sd.items()}
    if mode != "ZINB":
        sd = {k: v for k, v in sd.items() if not k.startswith(("fc11_p.", "fc11_r."))}
    A, _, D, H, L, Cc, S = [int(v) for v in G[f"{name}/cfg"]]
    m = mixVAE_model(input_dim=D, fc_dim=H, n_categories=Cc, state_dim=S, lowD_dim=L, x_drop=0.5, s_drop=0.2, n_arm=A, lam=1,
                     lam_pc=1, tau=0.005, beta=1.0, hard=False, variational=True, device=DEV, eps=1e-8, momentum=0.01,
                     ref_prior=False, loss_mode=mode)
    m.load_state_dict(sd)
    return m.to(DEV).eval()


@pytest.mark.parametrize("name", FIXTURES)
def test_decoder_zinb(name):
    """x_rec is ``decoder``'s output bit for bit.  Each gate against the fp64 restatement on the device's own d10:
        |x - sigmoid(a64)| <= (H + 2) 2^-24 (sum_k |w_k h_k| + |b|) / 4 + 0.51 ulp(x)
    -- the error of a float32 fma chain of H + 1 terms, times the sigmoid's largest slope 1/4, plus the one rounding of the
    kernel's fp64 sigmoid.  The reference's recorded float32 heads must lie within the same bound plus their own recorded
    distance from the recorded fp64 heads plus what the decode chain's own gate (tests/test_gpu_decode.py: d10 within 1e-5 of
    its scale) lets d10 differ from the reference's: 1e-5 max|d10| sum_k |w_k| / 4."""
    m = _fixture_model(name)
    A, H = m.n_arm, m.fc_dim
    c = torch.from_numpy(G[f"{name}/c"]).float().to(DEV)
    s = torch.from_numpy(G[f"{name}/s"]).float().to(DEV)
    for a in range(A):
        x_rec, x_p, x_r = m.decoder_zinb(c[a], s[a], a)
        eng = next(e for k, e in m._dec_engines.items() if k[0] == 1 and k[1] == c.shape[1] and k[2] is None)
        d10 = eng.ws_view("d10", H)[0].double().cpu()
        assert torch.equal(x_rec, m.decoder(c[a], s[a], a))
        assert float(d10.abs().max()) > 0
        for key, got, lin in (("p", x_p, m.fc11_p[a]), ("r", x_r, m.fc11_r[a])):
            W, b = lin.weight.detach().double().cpu(), lin.bias.detach().double().cpu()
            want = torch.sigmoid(d10 @ W.T + b)
            pre = (H + 2) * U32 * (d10.abs() @ W.abs().T + b.abs())
            ulp = torch.from_numpy(np.spacing(want.float().numpy())).double()
            bound = pre / 4 + 0.51 * ulp
            got = got.cpu().double()
            err = (got - want).abs()
            assert bool((err <= bound).all()), (key, float((err / bound).max()))
            r32, r64 = torch.from_numpy(G[f"{name}/f32/{key}"][a]).double(), torch.from_numpy(G[f"{name}/f64/{key}"][a])
            chain = 1e-5 * float(d10.abs().max()) * W.abs().sum(dim=1)[None, :] / 4
            err = (got - r32).abs()
            assert bool((err <= bound + (r32 - r64).abs() + chain).all()), key
            assert float((got - r64).abs().max()) < 1e-4            # and plainly close to the recorded fp64
    mse = _fixture_model(name, "MSE")
    with pytest.raises(RuntimeError, match="loss_mode='ZINB'"):
        mse.decoder_zinb(c[0], s[0], 0)


# ---- 3. terms and sums -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,D,H", SHAPES)
def test_terms_and_sums(n, D, H):
    c = case(n, D, H)
    print(f"\n  N = {n}, D = {D}, H = {H}")
    ok = True
    # mmvae_zinb_nll: heads formed on the device from d10; truth: fp64 from the same float32 d10, weights and X
    cell, gene = N.zinb_nll(pitched(c["d10"]), *(t.to(DEV) for t in c["L"]), pitched(c["X"]))
    assert cell.shape == (n,) and gene.shape == (D,) and cell.dtype == gene.dtype == torch.float64
    t64, M, t32 = c["t64"], c["M"], c["t32"].double()
    ok &= within("nll cell", ZR.error_stat(cell.cpu(), t64.sum(1), M.sum(1)), ZR.error_stat(t32.sum(1), t64.sum(1), M.sum(1)))
    ok &= within("nll gene", ZR.error_stat(gene.cpu(), t64.sum(0), M.sum(0)), ZR.error_stat(t32.sum(0), t64.sum(0), M.sum(0)))
    # mmvae_zinb_terms: the float32 heads given; truth: the fp64 term of those heads
    cell2, gene2, terms = N.zinb_terms(*(pitched(h) for h in c["h32"]), pitched(c["X"]), return_terms=True)
    g64, gM = c["g64"], c["gM"]
    ok &= within("terms", ZR.error_stat(terms.cpu(), g64, gM), ZR.error_stat(t32, g64, gM))
    ok &= within("terms cell", ZR.error_stat(cell2.cpu(), g64.sum(1), gM.sum(1)), ZR.error_stat(t32.sum(1), g64.sum(1), gM.sum(1)))
    ok &= within("terms gene", ZR.error_stat(gene2.cpu(), g64.sum(0), gM.sum(0)), ZR.error_stat(t32.sum(0), g64.sum(0), gM.sum(0)))
    assert ok
    # the sums without the terms written are the same bits
    cell3, gene3, none = N.zinb_terms(*(pitched(h, 5) for h in c["h32"]), pitched(c["X"], 1))
    assert none is None and torch.equal(cell2, cell3) and torch.equal(gene2, gene3)


# ---- 4. zinb_loss ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_zinb_loss(name):
    """On the reference's recorded float32 heads: |loss - fp64| / M against the recorded float32 loss's, M the mean of the
    elements' M; the same rule as the sums (the fp64 value is the restatement's on those heads)."""
    X = torch.from_numpy(G[f"{name}/X"])
    for a in range(int(G[f"{name}/cfg"][0])):
        h = [torch.from_numpy(G[f"{name}/f32/{k}"][a]) for k in ("rec", "p", "r")]
        got = NM.zinb_loss(*(pitched(t) for t in h), pitched(X))
        assert got.dim() == 0 and got.dtype == torch.float32 and got.device.type == "cuda"
        truth = float(ZR.loss(*(t.double() for t in h), X.double()))
        M = float(ZR.magnitudes(*h, X).mean())
        dev, cpu = abs(float(got) - truth) / M, abs(float(G[f"{name}/f32/loss"][a]) - truth) / M
        print(f"\n  {name} arm {a}: device {dev:.3e} | recorded float32 {cpu:.3e} (loss {truth:.6f})")
        assert dev <= MARGIN * cpu
        # a 3-D input is flattened over its leading dimensions
        got3 = NM.zinb_loss(*(t.to(DEV)[None] for t in h), X.to(DEV)[None])
        assert torch.equal(got3, got)
    t = h[0].to(DEV)
    with pytest.raises(NotImplementedError, match="no backward"):
        NM.zinb_loss(t.clone().requires_grad_(), h[1].to(DEV), h[2].to(DEV), X.to(DEV))


# ---- 5. forward(eval=True) ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_forward_eval_under_zinb(name):
    mz, mm = _fixture_model(name), _fixture_model(name, "MSE")
    A, D = mz.n_arm, mz.input_dim
    x = torch.from_numpy(G[f"{name}/X"]).to(DEV)
    for m in (mz, mm):
        m._noise_seed, m._noise_offset = 77, 0
    oz = mz(x.expand(A, -1, -1), 1.0, eval=True)
    om = mm(x.expand(A, -1, -1), 1.0, eval=True)
    assert len(oz) == len(om) == 10 and om[1] == [] and om[2] == []
    for i in (0, 3, 4, 5, 6, 7, 8, 9):
        assert all(torch.equal(p, q) for p, q in zip(oz[i], om[i])), i
    assert len(oz[1]) == len(oz[2]) == A
    for a in range(A):
        assert oz[1][a].shape == (x.shape[0], D) and oz[1][a].dtype == torch.float32
        x_rec, x_p, x_r = mz.decoder_zinb(oz[6][a], oz[5][a], a)
        assert torch.equal(oz[1][a], x_p) and torch.equal(oz[2][a], x_r), a
    with pytest.raises(NotImplementedError, match="zinb_nll"):
        mz.loss(oz[0], oz[1], oz[2], x.expand(A, -1, -1), oz[7], oz[8], oz[4], oz[6])
    with pytest.raises(AssertionError, match="ZINB not implemented"):
        mz(x.expand(A, -1, -1), 1.0, eval=False)
    mz.train()
    with pytest.raises(AssertionError, match="ZINB not implemented"):
        mz(x.expand(A, -1, -1), 1.0, eval=True)
    with pytest.raises(NotImplementedError, match="training under loss_mode='ZINB' is not built"):
        mz.fused_train_step(x.expand(A, -1, -1), 1.0, None, do_adam=False)


# ---- 6. determinism ------------------------------------------------------------------------------------------------------------------
def test_runs_are_bit_identical_and_a_cell_stands_alone():
    c = case(257, 130, 128)
    d10, X, L = pitched(c["d10"]), pitched(c["X"]), [t.to(DEV) for t in c["L"]]
    heads = [pitched(h) for h in c["h32"]]
    first = N.zinb_nll(d10, *L, X)
    again = N.zinb_nll(d10, *L, X)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    t1, t2 = N.zinb_terms(*heads, X, return_terms=True), N.zinb_terms(*heads, X, return_terms=True)
    assert all(torch.equal(p, q) for p, q in zip(t1, t2))
    hp1, hp2 = N.zinb_heads(d10, *L[2:]), N.zinb_heads(d10, *L[2:])
    assert torch.equal(hp1[0], hp2[0]) and torch.equal(hp1[1], hp2[1])
    for i in (0, 5, 37, 64):       # (cell 64 alone sits in row 0 of its tile, among 65 in row 0 of the second tile)
        alone = N.zinb_nll(d10[i:i + 1], *L, X[i:i + 1])[0]
        among65 = N.zinb_nll(d10[:65], *L, X[:65])[0]
        assert torch.equal(alone[0], among65[i]) and torch.equal(alone[0], first[0][i]), i
        alone_t = N.zinb_terms(*(h[i:i + 1] for h in heads), X[i:i + 1])[0]
        among_t = N.zinb_terms(*(h[:65] for h in heads), X[:65])[0]
        assert torch.equal(alone_t[0], among_t[i]) and torch.equal(alone_t[0], t1[0][i]), i
        assert torch.equal(N.zinb_heads(d10[i:i + 1], *L[2:])[0][0], hp1[0][i])


# ---- 7. score_zinb ---------------------------------------------------------------------------------------------------------------------
def test_score_zinb_on_a_device_loader():
    """The eval forward draws s_smp (the reference's ``reparameterize`` samples in eval mode too), so a cell's likelihood
    depends on its draw: the batches and the one call are given the same explicit U(0,1) draw per cell."""
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
    m.set_explicit_noise([{"u_state": u[:, i:i + B].contiguous()} for i in range(0, n, B)])
    got = t.score_zinb(DeviceLoader(data, index, B, False, False))
    assert sorted(got) == ["cell", "data_indx", "gene", "mean"]
    assert got["cell"].shape == (A, n) and got["gene"].shape == (A, Dm) and got["mean"].shape == (A,)
    assert got["cell"].dtype == got["gene"].dtype == got["mean"].dtype == np.float64
    assert np.array_equal(got["data_indx"].astype(np.int64), index.numpy())          # the loader's order
    assert m.training                                                                 # the mode is restored
    m.eval()
    m.set_explicit_noise({"u_state": u})
    x = data[index.to(DEV)]
    out = m(x.expand(A, -1, -1), t.temp, eval=True)
    one = m.zinb_nll(x.expand(A, -1, -1), t.temp)
    assert one["n"] == n and one["cell"].shape == (A, n) and one["gene"].shape == (A, Dm)
    for a in range(A):
        # the mean is zinb_loss of the materialised heads.  Both are fp64 sums of fp64 terms; zinb_loss reads heads rounded to
        # float32, zinb_nll does not.  A relative 2^-24 on x_p moves k log p by k 2^-24 and r log(1 - p) by r 2^-24 p / (1 - p),
        # on x_r it moves log(1 - z) by 2^-24 z / (1 - z) (and the zero branch by less), on x_rec the r terms by
        # 2^-24 r (|psi| + |log(1 - p)|) <= 2^-24 r (k + 4) here: with both gates inside (0.2, 0.8) at most
        # 2^-24 (k + 4 r + 4 + r (k + 4)) an element; doubled, plus the float32 rounding of zinb_loss's result
        for gate in (out[1][a], out[2][a]):
            assert 0.2 < float(gate.min()) and float(gate.max()) < 0.8
        loss = float(NM.zinb_loss(out[0][a], out[1][a], out[2][a], x))
        k, r = torch.expm1(x.double().cpu()), out[0][a].double().cpu() + 1e-6
        bound = 2 * U32 * float((k + 4 * r + 4 + r * (k + 4)).mean()) + U32 * abs(loss)
        mean_one = float(one["cell"][a].sum()) / (n * Dm)
        print(f"\n  arm {a}: mean {got['mean'][a]:.9f}, one call {mean_one:.9f}, zinb_loss of the heads {loss:.9f}, bound {bound:.3e}")
        assert abs(mean_one - loss) <= bound, (mean_one, loss, bound)
        assert got["mean"][a] == pytest.approx(got["cell"][a].sum() / (n * Dm), rel=1e-14)
    # the batches of 64 against the one call: the same bits per cell; the per-gene sums within the fp64 summation bound
    d = np.abs(got["cell"] - one["cell"].cpu().numpy())
    print(f"  cells whose bits differ between batches of {B} and one call: {int((d > 0).sum())} of {d.size}, "
          f"largest relative difference {float((d / np.abs(got['cell'])).max()):.3e}")
    assert np.array_equal(got["cell"], one["cell"].cpu().numpy())
    for a in range(A):
        tm = ZR.terms(out[0][a].double().cpu(), out[1][a].double().cpu(), out[2][a].double().cpu(), x.double().cpu())
        bound = (n + 2) * 2.0 ** -53 * tm.abs().sum(0).numpy() * 1.01
        assert np.all(np.abs(got["gene"][a] - one["gene"][a].cpu().numpy()) <= bound)
        assert abs(got["mean"][a] - float(one["cell"][a].sum()) / (n * Dm)) <= 1e-14 * abs(got["mean"][a])
    m.set_explicit_noise(None)
    mse = cpl_mixVAE(saving_folder="", device=0, save_flag=False)
    mse.init_model(n_categories=Cc, state_dim=S, input_dim=Dm, fc_dim=20, lowD_dim=6, n_arm=A)
    with pytest.raises(RuntimeError, match="loss_mode='ZINB'"):
        mse.score_zinb(DeviceLoader(data, index, B, False, False))
    with pytest.raises(NotImplementedError, match="training under loss_mode='ZINB' is not built"):
        t._step(x.expand(A, -1, -1))

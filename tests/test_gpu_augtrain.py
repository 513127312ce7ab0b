"""Augmenter training on the device (csrc/augtrain.hip) against tests/augtrain_restatement.py.

Gates (section 9m's).  An element's error is |value - truth| / M, truth the float64 restatement on the same inputs and M the sum
of the magnitudes of the addends of the element's last sum (``augtrain_restatement._magnitudes``); a tensor's figures are the
largest element error and the 90th percentile.  The device must stay within max(3 x the float32 restatement's figure on the
same inputs and the same ReLU decisions, 2^-23) in both.  The eleven biases in front of
a non-affine BatchNorm have an exactly zero gradient: what is returned is rounding noise, gated by B 2^-24 sum_b |dY_bj|."""
import pytest
import torch

from tests import augtrain_cases as AC
from tests import augtrain_restatement as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U23 = 2.0 ** -23


def _model(case, sd=None):
    import distributed_vae_amd  # noqa: F401
    from distributed_vae_amd.augmentation import Augmenter_smartseq
    NZ, Z, D, n_dim, B = case
    m = Augmenter_smartseq(noise_dim=NZ, latent_dim=Z, input_dim=D, n_dim=n_dim, p_drop=AC.P_DROP)
    if sd is not None:
        m.load_state_dict(sd)
    return m.to(DEV).train()


_INPUTS = {}


def _inputs(case, n_pass=1):
    key = (case, n_pass)
    if key not in _INPUTS:
        NZ, Z, D, n_dim, B = case
        s_sd, s_x, s_n = AC.seeds(case)
        _INPUTS[key] = (R.random_state_dict(NZ, Z, D, n_dim, s_sd), R.synthetic_batch(B, D, s_x),
                        R.draw_noise(B, D, NZ, Z, AC.P_DROP, s_n, n_pass))
    return _INPUTS[key]


def _err(got, truth, M):
    """max and 90th percentile of |value - truth| / M over the elements (M = 0 only where every addend is zero)."""
    truth, M = truth.double().cpu(), M.double().cpu()
    e = ((got.double().cpu() - truth).abs() / M.clamp_min(1e-300)).flatten()
    return float(e.max()), float(torch.quantile(e[:: max(1, e.numel() // 1_000_000)], 0.9))


def _gate(name, got, ref32, truth, M):
    d, r = _err(got, truth, M), _err(ref32, truth, M)
    print(f"{name}: device max / p90 {d[0]:.3e} / {d[1]:.3e}; float32 restatement {r[0]:.3e} / {r[1]:.3e}")
    assert d[0] <= max(3 * r[0], U23) and d[1] <= max(3 * r[1], U23), (name, d, r)


def _check_step(case, dev_rest="cpu", force=0):
    """One step without Adam and without the statistics pass: outputs, gradients, ReLU decisions."""
    sd, x, (mask, z0, eps) = _inputs(case)
    NZ, Z, D, n_dim, B = case
    m = _model(case, sd)
    m._exec().tune[3] = force                    # MMVAE_TUNE_AUG_TILE
    m.set_explicit_noise(z0, eps)
    m.set_explicit_dropout(mask)
    r = m.train_step(x.to(DEV), do_adam=False, stat_pass=False, keep=True)
    dec = R.decisions(r["h"], r["x_aug"])
    dec = [d.to(dev_rest) for d in dec]
    free = R.step(sd, x, mask[0], z0[0], eps[0], AC.P_DROP, torch.float64, device=dev_rest)
    free32 = R.step(sd, x, mask[0], z0[0], eps[0], AC.P_DROP, torch.float32, device=dev_rest)
    t64 = R.step(sd, x, mask[0], z0[0], eps[0], AC.P_DROP, torch.float64, relu_override=dec, device=dev_rest)
    t32 = R.step(sd, x, mask[0], z0[0], eps[0], AC.P_DROP, torch.float32, relu_override=dec, device=dev_rest)
    # decisions: the device may differ from float64 only where the float64 pre-activation is within float32 rounding of zero
    flips = total = 0
    pre64 = free["pre"] + [free["y11"]]
    pre32 = free32["pre"] + [free32["y11"]]
    for i in range(11):
        diff = dec[i] != (pre64[i] > 0)
        tol = max(3 * float((pre32[i].double() - pre64[i]).abs().max()), U23 * float(pre64[i].abs().max()))
        assert bool((pre64[i][diff].abs() <= tol).all()), (i, float(pre64[i][diff].abs().max()), tol)
        flips += int(diff.sum())
        total += diff.numel()
    print(f"ReLU decisions that differ from float64: {flips} of {total}")
    assert flips <= 1e-4 * total
    M = t64["M"]
    _gate("s", r["s"], t32["s"], t64["s"], M["s"])
    _gate("x_aug", r["x_aug"], t32["x_aug"], t64["x_aug"], M["x_aug"])
    assert abs(r["mse"] - t64["mse"]) <= max(3 * abs(t32["mse"] - t64["mse"]), U23 * t64["mse"])
    assert r["mismatch"] == int(((r["x_aug"].cpu() > 1e-3) != (x > 1e-4)).sum())
    assert abs(r["recon_loss"] - (r["mse"] + 100.0 * r["mismatch"] / (B * D)) / 2) <= 1e-12 * r["recon_loss"]
    m.bind_grads()
    named = dict(m.named_parameters())
    assert list(named) == R.PARAM_ORDER
    for k in R.PARAM_ORDER:
        g = named[k].grad
        if k in R.ZERO_GRAD_BIASES:
            dy = t64["dlin"][k[:-5]].abs().sum(0).cpu()
            worst = float((g.double().cpu().abs() / (B * 2.0 ** -24 * dy + 1e-300)).max())
            print(f"{k}: |g| / (B 2^-24 sum |dY|) = {worst:.3e}")
            assert worst <= 1.0, (k, worst)
        else:
            _gate(k, g, t32["grads"][k], t64["grads"][k], M[k])
    return m, r


@pytest.mark.parametrize("case", AC.CASES)
def test_forward_and_running_statistics(case):
    sd, x, (mask, z0, eps) = _inputs(case, 2)
    NZ, Z, D, n_dim, B = case
    # the training-mode forward alone: statistics move once
    m = _model(case, sd)
    m.set_explicit_noise(z0[1], eps[1])
    m.set_explicit_dropout(mask[1])
    s, xa = m(x.to(DEV), False, 1.0)
    t64 = R.step(sd, x, mask[1], z0[1], eps[1], AC.P_DROP, torch.float64)
    t32 = R.step(sd, x, mask[1], z0[1], eps[1], AC.P_DROP, torch.float32)
    assert s.shape == (B, Z) and xa.shape == (B, D)
    _gate("s", s, t32["s"], t64["s"], t64["M"]["s"])
    _gate("x_aug", xa, t32["x_aug"], t64["x_aug"], t64["M"]["x_aug"])
    got = m.state_dict()
    for k, v in t64["running"].items():
        if k.endswith(R.MAG):
            continue
        if k.endswith("num_batches_tracked"):
            assert int(got[k]) == int(v) == 4
        else:
            _gate(k, got[k], t32["running"][k], v, t64["running"][k + R.MAG])
    # a step with its statistics pass: they move twice
    m = _model(case, sd)
    m.set_explicit_noise(z0, eps)
    m.set_explicit_dropout(mask)
    m.train_step(x.to(DEV), do_adam=False, stat_pass=True)
    st = (mask[0], z0[0], eps[0])
    t64 = R.step(sd, x, mask[1], z0[1], eps[1], AC.P_DROP, torch.float64, stat=st)
    t32 = R.step(sd, x, mask[1], z0[1], eps[1], AC.P_DROP, torch.float32, stat=st)
    got = m.state_dict()
    for k, v in t64["running"].items():
        if k.endswith(R.MAG):
            continue
        if k.endswith("num_batches_tracked"):
            assert int(got[k]) == int(v) == 5
        else:
            _gate(k, got[k], t32["running"][k], v, t64["running"][k + R.MAG])


@pytest.mark.parametrize("case", AC.CASES)
def test_gradients(case):
    _check_step(case)


def test_refusals_on_the_device():
    """The refusals that lie behind the device check: one row (torch refuses one value per channel), another GEMM engine."""
    case = AC.CASES[0]
    sd, x, _ = _inputs(case)
    m = _model(case, sd)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        m(x[:1].to(DEV), False, 1.0)
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        m.train_step(x[:1].to(DEV))
    for dt in ("bf16", "fp32_mfma"):
        m.gemm_dtype = dt
        with pytest.raises(NotImplementedError, match="gemm_dtype"):
            m(x.to(DEV), False, 1.0)
        with pytest.raises(NotImplementedError, match="gemm_dtype"):
            m.train_step(x.to(DEV))
    for k, v in m.state_dict().items():
        assert torch.equal(v, before[k]), k          # a refused call moves nothing


@pytest.mark.parametrize("code", AC.FORCED)
def test_every_tile_and_k_split_of_the_engine(code):
    """The engine's tile and K split follow from a product's shape, so which of them the listed cases reach is the engine's
    business.  Forced here (MMVAE_AUG_TILE = tile + 10 x KS, for every product of the step alike) at AC.FORCED_CASE, every tile
    shape and K splits of 2, 3 and 8 -- dW included, whose K is the batch -- must pass the step's gates like the default choice."""
    _check_step(AC.FORCED_CASE, force=code)


def test_adam_follows_torch_and_determinism():
    case = AC.CASES[2]
    sd, x, (mask, z0, eps) = _inputs(case, 2)
    outs = []
    for rep in range(2):
        m = _model(case, sd)
        m.set_explicit_noise(z0, eps)
        m.set_explicit_dropout(mask)
        r = m.train_step(x.to(DEV), lr=1e-3, keep=True)
        r2 = m.train_step(x.to(DEV), lr=1e-3)
        outs.append((m, r, r2))
    (ma, ra, ra2), (mb, rb, rb2) = outs
    assert ra["mse"] == rb["mse"] and ra2["mse"] == rb2["mse"] and ra["mismatch"] == rb["mismatch"]
    assert torch.equal(ra["x_aug"], rb["x_aug"]) and torch.equal(ra["s"], rb["s"]) and torch.equal(ma.flat_grad(), mb.flat_grad())
    for (k, a), b in zip(ma.state_dict().items(), mb.state_dict().values()):
        assert torch.equal(a, b), k
    # one step: torch.optim.Adam on the device's own gradients
    one = _model(case, sd)
    one.set_explicit_noise(z0, eps)
    one.set_explicit_dropout(mask)
    one.train_step(x.to(DEV), lr=1e-3)
    m = _model(case, sd)
    m.set_explicit_noise(z0, eps)
    m.set_explicit_dropout(mask)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    m.train_step(x.to(DEV), do_adam=False)
    m.bind_grads()
    opt.step()
    worst = 0.0
    for (k, p), q in zip(m.named_parameters(), one.parameters()):
        if k in R.ZERO_GRAD_BIASES:      # rounding-noise gradients: Adam turns the noise into steps of lr in either implementation
            continue
        assert float((p - sd[k].to(DEV)).abs().max()) > 1e-4, k      # the step moved the tensor
        worst = max(worst, float((p - q).abs().max()))
    print(f"one Adam step, device against torch.optim.Adam on the device's gradients: {worst:.3e}")
    assert worst <= ADAM_GATE


ADAM_GATE = 6e-8      # twice the measured distance, 2.98e-8 = one float32 ulp of a weight in [0.25, 0.5)


def test_descent_follows_float64():
    case = AC.CASES[1]
    NZ, Z, D, n_dim, B = case
    sd, x, _ = _inputs(case)
    mask, z0, eps = R.draw_noise(B, D, NZ, Z, AC.P_DROP, 99, 20)
    m = _model(case, sd)
    m.set_explicit_noise(None, None)
    dev_mse = []
    for t in range(20):
        m.set_explicit_noise(z0[t], eps[t])
        m.set_explicit_dropout(mask[t])
        dev_mse.append(m.train_step(x.to(DEV), lr=1e-3, stat_pass=False)["mse"])
    traj = {}
    for dt in (torch.float64, torch.float32):
        cur = {k: v.clone().to(dt) if v.is_floating_point() else v.clone() for k, v in sd.items()}
        ps = [cur[k].requires_grad_(True) for k in R.PARAM_ORDER]
        opt = torch.optim.Adam(ps, lr=1e-3)
        out = []
        for t in range(20):
            r = R.step(cur, x, mask[t], z0[t], eps[t], AC.P_DROP, dt)
            for k, p in zip(R.PARAM_ORDER, ps):
                p.grad = r["grads"][k].to(dt)
            opt.step()
            for k, v in r["running"].items():
                cur[k] = v
            out.append(r["mse"])
        traj[dt] = out
    t64, t32 = traj[torch.float64], traj[torch.float32]
    assert t64[-1] < t64[0]
    dep32 = max(abs(a - b) / b for a, b in zip(t32, t64))
    dep = max(abs(a - b) / b for a, b in zip(dev_mse, t64))
    print(f"mse {t64[0]:.6f} -> {t64[-1]:.6f} (float64), device {dev_mse[0]:.6f} -> {dev_mse[-1]:.6f}; departure device {dep:.3e}, "
          f"float32 restatement {dep32:.3e}")
    assert dep <= max(3 * dep32, U23)


def test_driver_resume_and_consistency(tmp_path):
    import distributed_vae_amd  # noqa: F401
    from distributed_vae_amd.augmentation import Augmenter_smartseq, mk_augmenter, train_augmenter
    from distributed_vae_amd.cpl_mixvae import cpl_mixVAE
    from oracle import augmenter as OA
    NZ, Z, D, n_dim, B = AC.CASES[1]
    data = R.synthetic_batch(3 * B, D, 4)
    loader = [(data[i * B:(i + 1) * B], None) for i in range(3)]

    def run(epochs, folder, resume=None):
        torch.manual_seed(5)
        netA = Augmenter_smartseq(NZ, Z, D, n_dim)
        torch.manual_seed(6)
        par = {"num_epochs": epochs, "learning_rate": 1e-3, "lambda": [1, 0.5, 0.1, 0.5], "batch_size": B, "save": True,
               "saving_path": str(folder) + "/", "num_n": NZ, "num_z": Z, "n_features": D, "initial_w": False, "mode": "MSE"}
        hist = train_augmenter(netA, None, loader, par, DEV, resume=resume)
        return netA, hist, str(folder) + "/augmenter.pth"
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    full, hist, f_full = run(4, tmp_path / "a")
    _, _, f_half = run(2, tmp_path / "b")
    cont, hist2, f_cont = run(4, tmp_path / "b", resume=f_half)
    assert hist["mse"] == hist2["mse"] and len(hist["mse"]) == 12 and len(hist["epoch_mse"]) == 4
    ca, cb = torch.load(f_full, weights_only=True), torch.load(f_cont, weights_only=True)
    for k in ca["netA"]:
        assert torch.equal(ca["netA"][k], cb["netA"][k]), k
    for i in ca["optimA"]["state"]:
        assert torch.equal(ca["optimA"]["state"][i]["exp_avg_sq"], cb["optimA"]["state"][i]["exp_avg_sq"])
    assert int(ca["netA"]["batch_fc1.num_batches_tracked"]) == 24
    torch.optim.Adam(Augmenter_smartseq(NZ, Z, D, n_dim).parameters(), lr=1e-3).load_state_dict(ca["optimA"])
    # the eval forward of the trained module sees the trained weights and statistics
    full.eval()
    g = torch.Generator().manual_seed(1)
    z0, eps = torch.randn(1, B, NZ, generator=g), torch.randn(1, B, Z, generator=g)
    full.set_explicit_noise(z0, eps)
    s, xa = full(data[:B].to(DEV), False, 1.0)
    sd = {k: v.cpu() for k, v in full.state_dict().items()}
    s_ref, xa_ref = OA.forward_eval(sd, data[:B], z0[0], eps[0], 1.0)
    assert float((xa.cpu() - xa_ref).abs().max()) <= 1e-4 * float(xa_ref.abs().max())
    assert float((s.cpu() - s_ref).abs().max()) <= 1e-4 * float(s_ref.abs().max())
    _, par, loaded = mk_augmenter(f_full)
    assert par["n_features"] == D and torch.equal(loaded.state_dict()["fc11.weight"], sd["fc11.weight"])
    t = cpl_mixVAE(saving_folder="", aug_file=f_full, device=DEV, save_flag=False)
    assert t.netA is not None and not t.netA.training


def test_production_shape():
    case = AC.PRODUCTION
    m, r = _check_step(case, dev_rest=DEV)
    g1, xa1, s1 = m.flat_grad().clone(), r["x_aug"].clone(), r["s"].clone()
    r2 = m.train_step(_inputs(case)[1].to(DEV), do_adam=False, stat_pass=False, keep=True)
    assert torch.equal(m.flat_grad(), g1) and torch.equal(r2["x_aug"], xa1) and torch.equal(r2["s"], s1) and r2["mse"] == r["mse"]

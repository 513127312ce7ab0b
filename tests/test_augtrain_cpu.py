"""Augmenter training without a GPU: the restatement against the reference-recorded fixture, the zero-gradient finding, the
refusals and the checkpoint format."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle.ref_loader import REFERENCE_ROOT as REFERENCE      # where the reference project lies, if it is there
from tests import augtrain_cases as AC
from tests import augtrain_restatement as R

GOLD = os.path.join(os.path.dirname(__file__), "golden", "augtrain_ref.npz")


def test_float32_restatement_reproduces_the_fixture():
    g = np.load(GOLD)
    NZ, Z, D, n_dim, B = (int(v) for v in g["dims"])
    lam3, lr, p = float(g["lam3"]), float(g["lr"]), float(g["p_drop"])
    T = lambda k: torch.from_numpy(g[k])      # noqa: E731
    cur = {k[4:]: T(k).clone() for k in g.files if k.startswith("sd0/")}
    ps = [cur[k].requires_grad_(True) for k in R.PARAM_ORDER]
    opt = torch.optim.Adam(ps, lr=lr)
    for t in range(3):
        r = R.step(cur, T(f"x/{t}"), T(f"mask/{t}/1"), T(f"z0/{t}/1"), T(f"eps/{t}/1"), p, torch.float32, weight=lam3 / 2,
                   stat=(T(f"mask/{t}/0"), T(f"z0/{t}/0"), T(f"eps/{t}/0")))
        assert abs(r["recon_loss"] - float(g[f"recon_loss/{t}"])) <= 1e-5 * float(g[f"recon_loss/{t}"])
        if t == 0:
            for k in R.PARAM_ORDER:
                ref = T("grad0/" + k)
                if k in R.ZERO_GRAD_BIASES:
                    assert float(ref.abs().max()) < 1e-7 and float(r["grads"][k].abs().max()) < 1e-7
                else:
                    assert float((r["grads"][k] - ref).abs().max()) <= 2e-5 * float(ref.abs().max()), k
        for k, q in zip(R.PARAM_ORDER, ps):
            q.grad = r["grads"][k]
        opt.step()
        cur.update(r["running"])
    for k in (k[4:] for k in g.files if k.startswith("sd1/")):
        ref, got = T("sd1/" + k), cur[k].detach()
        if k.endswith("num_batches_tracked"):
            assert int(got) == int(ref) == 3 + 6
        elif k in R.ZERO_GRAD_BIASES:
            continue        # rounding-noise gradients under Adam: a random walk of lr per step that BatchNorm cancels
        elif k in R.PARAM_ORDER:
            # the typical entry must be tight: an entry whose gradient is rounding noise may go either way by lr per step, so the
            # largest difference (at most 6 lr between any two Adam trajectories of three steps) says nothing and is not gated
            d = (got - ref).abs()
            assert float(d.median()) <= 2e-5, (k, float(d.median()), float(d.max()))
        else:
            assert float((got - ref).abs().max()) <= 1e-4 * max(float(ref.abs().max()), 1.0), k


class _SmallD(torch.nn.Module):
    def __init__(self, D):
        super().__init__()
        self.a, self.b = torch.nn.Linear(D, 8), torch.nn.Linear(8, 1)

    def forward(self, x):
        z = torch.relu(self.a(x))
        return z, torch.sigmoid(self.b(z))


def _a_loss(fwd, netD, x, lam, full):
    """The reference's A_loss (train.py:61-115) on two forwards, own code; full=False: the MSE term alone."""
    _, f1 = fwd()
    _, f2 = fwd()
    mse = torch.nn.functional.mse_loss(1.0 * f2, x)
    if not full:
        return lam[3] * 0.5 * mse
    bce = torch.nn.BCELoss()
    xb = 0.0 * x
    xb[x > 1e-4] = 1.0
    b1, b2 = 0.0 * f1, 0.0 * f2
    b1[f1 > 1e-3] = 1.0
    b2[f2 > 1e-3] = 1.0
    z1, p1 = netD(b1)
    z2, p2 = netD(b2)
    one = torch.ones(x.shape[0])
    gen = (bce(p1.view(-1), one) + bce(p2.view(-1), one)) / 2
    trip = torch.relu(bce(b2, xb) - bce(b1, xb) + 0.2).mean()      # TripletLoss(anchor = xb, positive = b2, negative = b1)
    recon = (mse + bce(b2, xb)) / 2
    return lam[0] * gen + lam[1] * trip + lam[2] * torch.nn.functional.mse_loss(z1, z2) + lam[3] * recon


def _grads_of(make, full):
    net, fwd, netD, x = make()
    _a_loss(fwd, netD, x, [1.0, 0.5, 0.1, 0.5], full).backward()
    return [p.grad.clone() for p in net.parameters()]


def test_only_the_mse_term_has_a_gradient():
    """Own restatement of the forward as a module-free function of leaf tensors."""
    NZ, Z, D, n_dim, B = AC.CASES[0]
    sd = R.random_state_dict(NZ, Z, D, n_dim, 5)
    x = R.synthetic_batch(B, D, 6)

    class Net:
        def __init__(self):
            self.P = {k: v.clone().requires_grad_(True) for k, v in sd.items() if k in R.PARAM_ORDER}
            self.run = {k: v.clone() for k, v in sd.items() if k not in R.PARAM_ORDER}

        def parameters(self):
            return [self.P[k] for k in R.PARAM_ORDER]

    def make():
        torch.manual_seed(9)
        net, netD = Net(), _SmallD(D)
        mask, z0, eps = R.draw_noise(B, D, NZ, Z, 0.5, 8, 2)
        it = iter(range(2))

        def fwd():
            i = next(it)
            return R.forward(net.P, net.run, x, mask[i], z0[i], eps[i], 0.5)
        return net, fwd, netD, x
    a, b = _grads_of(make, True), _grads_of(make, False)
    assert len(a) == 29 and all(torch.equal(u, v) for u, v in zip(a, b))
    assert sum(float(u.abs().sum()) for u in a) > 0


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "mmidas")), reason="the reference project is not present")
def test_only_the_mse_term_has_a_gradient_reference_classes():
    """The same with the reference's own Augmenter_smartseq, Discriminator and TripletLoss: A_loss as train.py:98-114 forms it."""
    sys.path.insert(0, REFERENCE)
    try:
        from mmidas.augmentation.aug_utils import TripletLoss
        from mmidas.augmentation.udagan import Augmenter_smartseq as Ref
        from mmidas.augmentation.udagan import Discriminator
    finally:
        sys.path.remove(REFERENCE)
    NZ, Z, D, n_dim, B = AC.CASES[0]
    sd = R.random_state_dict(NZ, Z, D, n_dim, 5)
    x = R.synthetic_batch(B, D, 6)
    lam, alpha = [1.0, 0.5, 0.1, 0.5], 0.2

    def grads(full):
        torch.manual_seed(9)
        net, netD = Ref(NZ, Z, D, n_dim, 0.5), Discriminator(input_dim=D)
        net.load_state_dict(sd)
        net.train()
        netD.train()
        torch.manual_seed(10)
        _, f1 = net(x, False)
        _, f2 = net(x, False)
        mse = torch.nn.functional.mse_loss(1.0 * f2, x)
        if full:
            bce = torch.nn.BCELoss()
            xb = 0.0 * x
            xb[x > 1e-4] = 1.0
            b1, b2 = 0.0 * f1, 0.0 * f2
            b1[f1 > 1e-3] = 1.0
            b2[f2 > 1e-3] = 1.0
            z1, p1 = netD(b1)
            z2, p2 = netD(b2)
            one = torch.full((B,), 1.0)
            gen = (bce(p1.view(-1), one) + bce(p2.view(-1), one)) / 2
            trip = TripletLoss(xb.view(B, -1), b2.view(B, -1), b1.view(B, -1), alpha, "BCE")
            recon = (mse + bce(b2, xb)) / 2
            loss = lam[0] * gen + lam[1] * trip + lam[2] * torch.nn.MSELoss()(z1, z2) + lam[3] * recon
        else:
            loss = lam[3] * 0.5 * mse
        loss.backward()
        return [p.grad.clone() for p in net.parameters()]
    a, b = grads(True), grads(False)
    assert len(a) == 29 and all(torch.equal(u, v) for u, v in zip(a, b))
    assert sum(float(u.abs().sum()) for u in a) > 0


def test_bce_of_binary_tensors_is_100_times_the_mismatch_share():
    g = torch.Generator().manual_seed(0)
    a, b = (torch.rand(37, 53, generator=g) > 0.4).float(), (torch.rand(37, 53, generator=g) > 0.6).float()
    bce = float(torch.nn.BCELoss()(a, b))
    assert abs(bce - 100.0 * float((a != b).float().mean())) <= 1e-5 * bce


def _module(case=AC.CASES[0]):
    import distributed_vae_amd  # noqa: F401
    from distributed_vae_amd.augmentation import Augmenter_smartseq
    NZ, Z, D, n_dim, B = case
    return Augmenter_smartseq(NZ, Z, D, n_dim)


def test_refusals():
    from distributed_vae_amd import _native as N
    from distributed_vae_amd.augmentation import train_augmenter
    NZ, Z, D, n_dim, B = AC.CASES[0]
    m = _module().train()
    with pytest.raises(NotImplementedError):
        m(torch.zeros(2, 4, D), True, 0.1)
    with pytest.raises(N.NativeError):
        m(torch.zeros(4, D), False, 1.0)
    with pytest.raises(N.NativeError):
        m.train_step(torch.zeros(4, D))
    par = {"num_epochs": 1, "learning_rate": 1e-3, "lambda": [1, 0.5, 0.1, 0.5], "batch_size": 4, "save": False, "saving_path": "",
           "num_n": NZ, "num_z": Z, "n_features": D, "initial_w": False, "mode": "MSE"}
    with pytest.raises(NotImplementedError, match="zero"):
        train_augmenter(m, _SmallD(D), [], par, "cuda:0")
    with pytest.raises(NotImplementedError, match="ZINB"):
        train_augmenter(m, None, [], dict(par, mode="ZINB"), "cuda:0")
    with pytest.raises(N.NativeError):
        train_augmenter(m, None, [], par, "cpu")
    # B == 1 is a matter of the shape, whatever the device: the library's own check says so without a GPU
    import ctypes as C
    d = N.AugDims(1, 1, D, D // 5, n_dim, n_dim // 5, Z, NZ)
    assert N.lib().mmvae_aug_train_workspace_bytes(C.byref(d)) == 0
    assert N.lib().mmvae_aug_param_layout(C.byref(d), C.byref(N.AugTrainLayout())) != 0
    m.eval()
    with pytest.raises(RuntimeError):
        m.train_step(torch.zeros(4, D))


def test_param_layout_follows_parameters():
    import ctypes as C

    from distributed_vae_amd import _native as N
    for case in AC.CASES + [AC.PRODUCTION]:
        NZ, Z, D, n_dim, B = case
        m = _module(case)
        lay = N.AugTrainLayout()
        d = N.AugDims(1, B, D, D // 5, n_dim, n_dim // 5, Z, NZ)
        assert N.lib().mmvae_aug_param_layout(C.byref(d), C.byref(lay)) == 0
        where = {}
        for i, name in enumerate(N.AUG_LINEARS):
            where[name + ".weight"] = (lay.w_off[i], lay.rows[i] * lay.cols[i])
            if lay.b_off[i] >= 0:
                where[name + ".bias"] = (lay.b_off[i], lay.rows[i])
        where["bnz.weight"], where["bnz.bias"] = (lay.bnz_w_off, NZ), (lay.bnz_b_off, NZ)
        end = 0
        for k, p in m.named_parameters():
            o, n = where[k]
            assert n == p.numel() and o >= end and o % 4 == 0, k
            end = o + n
        assert lay.total >= end and N.lib().mmvae_aug_train_workspace_bytes(C.byref(d)) > 0


def test_checkpoint_round_trips_through_mk_augmenter(tmp_path):
    """The file train_augmenter writes, made here from its own pieces (no device): weights_only loads it, mk_augmenter rebuilds
    the module, torch.optim.Adam takes the optimizer state."""
    from distributed_vae_amd import augmentation as AU
    NZ, Z, D, n_dim, B = AC.CASES[0]
    m = _module()
    m._flat = {"offs": [0] * 29}
    par = {"num_epochs": np.int64(2), "learning_rate": 1e-3, "lambda": (1, 0.5, 0.1, 0.5), "num_n": NZ, "num_z": Z, "n_features": D,
           "saving_path": tmp_path, "n_dim": n_dim, "p_drop": 0.5}
    f = str(tmp_path / "augmenter.pth")
    torch.save({"netA": m.state_dict(), "optimA": AU._adam_state_dict(m, {"step": 0}, 1e-3), "parameters": AU._plain(par)}, f)
    ck, p, net = AU.mk_augmenter(f)
    assert p["num_epochs"] == 2 and p["lambda"] == [1, 0.5, 0.1, 0.5] and isinstance(p["saving_path"], str)
    assert all(torch.equal(a, b) for a, b in zip(net.state_dict().values(), m.state_dict().values()))
    torch.optim.Adam(net.parameters(), lr=1e-3).load_state_dict(ck["optimA"])


@pytest.mark.parametrize("case", AC.SMALL)
def test_small_cases_keep_pre_activations_off_zero(case):
    NZ, Z, D, n_dim, B = case
    s_sd, s_x, s_n = AC.seeds(case)
    sd, x = R.random_state_dict(NZ, Z, D, n_dim, s_sd), R.synthetic_batch(B, D, s_x)
    mask, z0, eps = R.draw_noise(B, D, NZ, Z, AC.P_DROP, s_n, 1)
    r = R.step(sd, x, mask[0], z0[0], eps[0], AC.P_DROP, torch.float64)
    r32 = R.step(sd, x, mask[0], z0[0], eps[0], AC.P_DROP, torch.float32)
    for a, b in zip(r["pre"] + [r["y11"]], r32["pre"] + [r32["y11"]]):
        assert float(a.abs().min()) > 1e-4
        assert torch.equal(a > 0, b > 0)          # the float32 restatement takes the float64 decisions

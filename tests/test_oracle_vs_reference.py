"""CPU: oracle/restatement.py against what the reference model itself computed.

tests/golden/ref_restatement.npz and ref_masked.npz hold the reference's own results (mmidas/nn_model.py forward :297,
loss :495, autograd; written by oracle/gen_golden_ref.py, which runs the reference through oracle/ref_loader.py) on cases
that are not in the other fixtures.  The restatement is evaluated here on the same seeded inputs and checked in fp64 (where the two must agree
to rounding) and fp32.
"""
import os
import warnings

import numpy as np
import pytest
import torch

from oracle import packed as PK
from oracle import restatement as R

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")

CASES = [
    # A, B, D, H, L, C, S, hard, s_drop
    (2, 24, 40, 12, 4, 6, 2, False, 0.0),
    (3, 33, 50, 10, 3, 8, 2, False, 0.3),
    (4, 20, 36, 8, 4, 5, 1, True, 0.0),
]
TAG = {torch.float64: "f64", torch.float32: "f32"}


@pytest.fixture(scope="module")
def gold():
    return PK.Packed(os.path.join(GOLDEN, "ref_restatement.npz"))


@pytest.fixture(scope="module")
def gold_masked():
    return PK.Packed(os.path.join(GOLDEN, "ref_masked.npz"))


def _t(a):
    return torch.from_numpy(np.array(a))


def _hyper(cfg):
    A, B, D, H, L, C, S, hard, sdrop = cfg
    return R.Hyper(input_dim=D, fc_dim=H, n_categories=C, state_dim=S, lowD_dim=L, x_drop=0.5,
                   s_drop=sdrop, n_arm=A, hard=hard)


def _sub(gold, pre):
    """{name: tensor} of the fixture's arrays under ``pre/``, in the order they were written."""
    return {k: _t(v) for k, v in gold.under(pre).items()}


@pytest.mark.parametrize("cfg", CASES)
@pytest.mark.parametrize("dtype,tol", [(torch.float64, 1e-11), (torch.float32, 2e-4)])
def test_restatement_equals_reference(gold, cfg, dtype, tol):
    warnings.simplefilter("ignore")
    pre = f"rs/{CASES.index(cfg)}/{TAG[dtype]}"
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        h = _hyper(cfg)
        A, B, D = cfg[:3]
        sd = R.init_state_dict(h, 99, dtype=dtype)
        init = gold.digests_under(f"{pre}/init")    # the reference's initial state_dict, as digests
        assert list(init) == list(sd)
        for k in init:
            assert gold.matches(f"{pre}/init/{k}", sd[k]), k          # same constructor RNG order
        x = R.synthetic_batch(B, D, seed=5, dtype=dtype)
        noise = R.draw_noise(h, B, seed=11)
        out2, lt, grads = R.grads_autograd(sd, [x] * A, h, noise)
        _, _, gman, _ = R.grads_manual(R.init_state_dict(h, 99, dtype=dtype), [x] * A, h, noise)
        rel = lambda a, b: float((a - b).abs().max() / (b.abs().max() + 1e-30))
        lo = float(gold[f"{pre}/loss"])
        assert abs(float(lt[0]) - lo) <= tol * abs(lo)
        for i in (0, 3, 4, 5, 6, 7, 8, 9):
            for a in range(A):
                assert rel(out2[i][a], _t(gold[f"{pre}/out/{i}/{a}"])) < max(tol, 1e-12), (i, a)
        ref_grads = _sub(gold, f"{pre}/grad")
        assert ref_grads and set(ref_grads) <= set(grads)
        for k, g in ref_grads.items():
            assert rel(grads[k], g) < tol, k
            assert rel(gman[k], g) < tol, k
        running = _sub(gold, f"{pre}/state")
        assert running
        for k, v in running.items():
            assert rel(sd[k], v) < max(tol, 1e-12), k
    finally:
        torch.set_default_dtype(old)


def test_two_reference_snapshots_agree(gold):
    """build/lib snapshot has identical arithmetic to the current file (both losses recorded by
    oracle/gen_golden_ref.py on CASES[0], fp32), and the restatement reproduces that loss."""
    assert float(gold["snap/loss_current"]) == float(gold["snap/loss_old"])
    cfg = CASES[0]
    A, B, D = cfg[:3]
    h = _hyper(cfg)
    x = R.synthetic_batch(B, D, seed=5)
    _, lt, _ = R.grads_autograd(R.init_state_dict(h, 99), [x] * A, h, R.draw_noise(h, B, seed=11))
    lo = float(gold["snap/loss_current"])
    assert abs(float(lt[0].detach()) - lo) <= 2e-4 * abs(lo)


class _RefModelStandIn:
    """The reference model's state_dict layout as recorded in the fixture (keys in the reference's order, shapes and
    types), with the reference's parameters in their order: what a strict ``load_state_dict`` and
    ``torch.optim.Adam.load_state_dict`` check a checkpoint against."""

    def __init__(self, gold):
        layout = gold.list("ckpt/layout")
        self.keys = [k for k, _, _ in layout]
        self.param_keys = gold.list("ckpt/param_keys")
        self.values = {k: torch.zeros(shape, dtype=getattr(torch, dt)) for k, shape, dt in layout}
        self.params = [torch.nn.Parameter(self.values[k].clone()) for k in self.param_keys]

    def state_dict(self):
        from collections import OrderedDict
        return OrderedDict((k, self.values[k]) for k in self.keys)

    def load_state_dict(self, sd, strict=True):
        missing = [k for k in self.keys if k not in sd]
        unexpected = [k for k in sd if k not in self.values]
        for k in self.keys:
            if k in sd:
                assert tuple(sd[k].shape) == tuple(self.values[k].shape) and sd[k].dtype == self.values[k].dtype, k
                self.values[k] = sd[k].clone()
        return missing, unexpected

    def parameters(self):
        return iter(self.params)


def test_checkpoints_round_trip_with_the_reference(gold, tmp_path):
    """a checkpoint written by this package's trainer (cpl_mixvae.py:783-786 layout) loads into
    the reference model's layout and torch.optim.Adam with strict key checking, and a checkpoint written the reference's
    way loads back here -- so the reference's evaluation scripts keep working on these files."""
    warnings.simplefilter("ignore")
    import distributed_vae_amd  # noqa: F401
    from distributed_vae_amd.cpl_mixvae import FusedAdam, cpl_mixVAE
    cfg = (3, 8, 40, 12, 4, 6, 2, False, 0.0)
    A, B, D, H, L, C, S = cfg[:7]
    t = cpl_mixVAE(saving_folder=str(tmp_path), device="cpu", save_flag=True)
    t.init_model(n_categories=C, state_dim=S, input_dim=D, fc_dim=H, lowD_dim=L, x_drop=0.5, s_drop=0.0, n_arm=A)
    t.optimizer._bind()
    t.optimizer.step_count = 3
    t.optimizer.exp_avg.uniform_(-1, 1)
    t.optimizer.exp_avg_sq.uniform_(0, 1)
    path = str(tmp_path / "ckpt.pth")
    t.save_checkpoint(path)
    loaded = torch.load(path, map_location="cpu", weights_only=True)
    assert set(loaded) == {"model_state_dict", "optimizer_state_dict"}
    m_ref = _RefModelStandIn(gold)
    assert list(loaded["model_state_dict"]) == m_ref.keys
    missing, unexpected = m_ref.load_state_dict(loaded["model_state_dict"], strict=True)
    assert not missing and not unexpected
    for k, v in m_ref.state_dict().items():
        assert torch.equal(v, t.model.state_dict()[k]), k
    opt_ref = torch.optim.Adam(m_ref.parameters(), lr=1e-3)
    opt_ref.load_state_dict(loaded["optimizer_state_dict"])
    assert int(opt_ref.state[next(iter(m_ref.parameters()))]["step"]) == 3
    for p in m_ref.parameters():
        assert opt_ref.state[p]["exp_avg"].shape == p.shape and opt_ref.state[p]["exp_avg_sq"].shape == p.shape
    # the other direction: the reference's save (cpl_mixvae.py:783-786) -> this trainer's load_model
    ref_path = str(tmp_path / "ref.pth")
    torch.save({"model_state_dict": m_ref.state_dict(), "optimizer_state_dict": opt_ref.state_dict()}, ref_path)
    t2 = cpl_mixVAE(saving_folder=str(tmp_path), device="cpu", save_flag=False)
    t2.init_model(n_categories=C, state_dim=S, input_dim=D, fc_dim=H, lowD_dim=L, x_drop=0.5, s_drop=0.0, n_arm=A,
                  trained_model=ref_path)
    for k, v in t2.model.state_dict().items():
        assert torch.equal(v, m_ref.state_dict()[k]), k
    assert t2.optimizer.step_count == 3
    t3 = cpl_mixVAE(saving_folder=str(tmp_path), device="cpu", save_flag=False)
    t3.init_model(n_categories=C, state_dim=S, input_dim=D, fc_dim=H, lowD_dim=L, x_drop=0.5, s_drop=0.0, n_arm=A)
    t3.load_model(ref_path)
    assert torch.equal(t3.model.state_dict()["fc1.0.weight"], m_ref.state_dict()["fc1.0.weight"])


@pytest.mark.parametrize("dtype,tol", [(torch.float64, 1e-11), (torch.float32, 2e-4)])
def test_masked_forward_equals_reference(gold_masked, dtype, tol):
    """forward(mask=kept categories) -- the pruning-time forward, nn_model.py:332-335 -- train mode (with loss and
    gradients) and eval mode, restatement against the reference's recorded results."""
    warnings.simplefilter("ignore")
    pre = f"mask/{TAG[dtype]}"
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        cfg = (3, 33, 50, 10, 3, 8, 2, False, 0.0)
        h = _hyper(cfg)
        A, B, D = cfg[:3]
        mask = [1, 2, 4, 7]
        sd = R.init_state_dict(h, 99, dtype=dtype)
        x = R.synthetic_batch(B, D, seed=5, dtype=dtype)
        noise = R.draw_noise(h, B, seed=11)
        rel = lambda a, b: float((a - b).abs().max() / (b.abs().max() + 1e-30))
        out2, lt, grads = R.grads_autograd(sd, [x] * A, h, noise, mask=mask)
        _, _, gman, _ = R.grads_manual(R.init_state_dict(h, 99, dtype=dtype), [x] * A, h, noise, mask=mask)
        lo = float(gold_masked[f"{pre}/loss"])
        assert abs(float(lt[0]) - lo) <= tol * abs(lo)
        for i in (0, 3, 4, 5, 6, 7, 8, 9):
            for a in range(A):
                assert rel(out2[i][a], _t(gold_masked[f"{pre}/out/{i}/{a}"])) < max(tol, 1e-12), (i, a)
        for a in range(A):
            assert float(out2[4][a][:, [0, 3, 5, 6]].abs().max()) == 0.0        # masked-out categories: exactly zero
        ref_grads = _sub(gold_masked, f"{pre}/grad")
        assert ref_grads and set(ref_grads) <= set(grads)
        for k, g in ref_grads.items():
            assert rel(grads[k], g) < tol, k
            assert rel(gman[k], g) < tol, k
        ne = R.draw_noise(h, B, seed=12, training=False, eval_flag=True)
        oe2 = R.forward(sd, [x] * A, h, ne, training=False, eval_flag=True, mask=mask)
        for i in (0, 3, 4, 5, 6, 7, 8, 9):
            for a in range(A):
                assert rel(oe2[i][a], _t(gold_masked[f"{pre}/eout/{i}/{a}"])) < max(tol, 1e-12), (i, a)
    finally:
        torch.set_default_dtype(old)

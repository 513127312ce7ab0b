"""CPU (no GPU): what ``cpl_mixVAE.train`` on a model built with ``mode="ZINB"`` rests on that needs no device.

  * the refusals of ZINB training through the trainer -- the bf16 configuration, a pruned model or a set ``_prune_mask``,
    ``prune()``, AdamW through ``FusedAdam`` -- arrive before the engine is made and before noise is consumed;
  * ``_step`` on a ZINB model keeps its pinned refusal beside ``_zinb_step``;
  * ``FusedAdam.state_dict()`` of a ZINB model has one entry per ``model.parameters()`` (32 per arm) of the parameter's shape, the
    four head tensors per arm taken from the heads' moment buffers at ``mmvae_zinb_head_layout``'s offsets, and round-trips
    through ``torch.optim.Adam``; ``bind_grads`` gives every parameter its own view.
"""
import os

import pytest
import torch

import distributed_vae_amd  # noqa: F401
from distributed_vae_amd import _native as N
from distributed_vae_amd.cpl_mixvae import FusedAdam, cpl_mixVAE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_lib = pytest.mark.skipif(not os.path.exists(os.path.join(ROOT, "distributed-vae_amd", "libmmvae_hip.so")),
                               reason="libmmvae_hip.so not built")
A, C_, S_, D_, H_, L_ = 2, 5, 2, 24, 6, 3


def _trainer(mode="ZINB"):
    t = cpl_mixVAE(saving_folder="", device="cpu", save_flag=False)
    t.init_model(n_categories=C_, state_dim=S_, input_dim=D_, fc_dim=H_, lowD_dim=L_, n_arm=A, mode=mode)
    return t


def _no_engine(monkeypatch, m):
    # nothing past a refusal may run: a CPU model would otherwise fail later, at the engine, with another error
    monkeypatch.setattr(m, "_ensure", lambda *a, **k: pytest.fail("the refusal must come before the engine is made"))
    monkeypatch.setattr(m, "_next_noise", lambda *a, **k: pytest.fail("the refusal must come before noise is consumed"))


class _NoLoader:
    def __iter__(self):
        pytest.fail("the refusal must come before the loader is read")

    def __len__(self):
        return 1


def test_trainer_refusals_come_before_the_engine_and_the_noise(monkeypatch):
    t = _trainer()
    m = t.model
    _no_engine(monkeypatch, m)
    xs = torch.zeros(A, 4, D_)
    # the bf16 configuration
    m.gemm_dtype = "bf16"
    with pytest.raises(NotImplementedError, match="bf16"):
        t._zinb_step(xs)
    with pytest.raises(NotImplementedError, match="bf16"):
        t.train(_NoLoader(), None, 1)
    with pytest.raises(NotImplementedError, match="bf16"):
        next(t.epoch_steps(_NoLoader()))
    m.gemm_dtype = "fp32"
    # a set mask, and a model whose fcc bias has zeros
    t._prune_mask = [0, 1, 2]
    with pytest.raises(NotImplementedError, match="pruned"):
        t._zinb_step(xs)
    with pytest.raises(NotImplementedError, match="pruned"):
        t.train(_NoLoader(), None, 1)
    t._prune_mask = None
    with torch.no_grad():
        for a in range(A):
            m.fcc[a].bias[3] = 0.0
    with pytest.raises(NotImplementedError, match="pruned"):
        t.train(_NoLoader(), None, 1)
    with pytest.raises(NotImplementedError, match="pruned"):
        next(t.epoch_steps(_NoLoader()))
    with torch.no_grad():
        for a in range(A):
            m.fcc[a].bias[3] = 0.1
    # prune() itself
    with pytest.raises(NotImplementedError, match="ZINB"):
        t.prune(_NoLoader(), None, 1)
    # AdamW through FusedAdam: at construction, and when switched on afterwards
    with pytest.raises(NotImplementedError, match="decoupled"):
        FusedAdam(m, decoupled=True)
    t.optimizer.decoupled = True
    for call in (lambda: t._zinb_step(xs), lambda: t.train(_NoLoader(), None, 1), t.optimizer.step, t.optimizer.zinb_state):
        with pytest.raises(NotImplementedError, match="decoupled"):
            call()
    t.optimizer.decoupled = False
    # an MSE model has no ZINB step
    with pytest.raises(RuntimeError, match="loss_mode='ZINB'"):
        _trainer("MSE")._zinb_step(xs)
    assert FusedAdam(_trainer("MSE").model, decoupled=True).decoupled
    assert m._step_id == 0 and m._noise_offset == 0 and m.training and t.optimizer.step_count == 0


def test_step_keeps_its_pinned_refusal(monkeypatch):
    t = _trainer()
    _no_engine(monkeypatch, t.model)
    with pytest.raises(NotImplementedError, match="training under loss_mode='ZINB' is not built"):
        t._step(torch.zeros(A, 4, D_))
    assert t.model._step_id == 0 and t.model._noise_offset == 0


@needs_lib
def test_state_dict_covers_every_parameter_and_loads_into_torch_adam():
    t = _trainer()
    m, opt = t.model, t.optimizer
    params = list(m.parameters())
    assert len(params) == 32 * A
    assert opt.state_dict()["state"] == {} and len(opt.state_dict()["param_groups"][0]["params"]) == 32 * A     # no step yet
    st = opt.zinb_state()
    assert st is opt.zinb_state() and st["exp_avg"] is opt.exp_avg and st["hp_exp_avg_sq"] is opt.hp_exp_avg_sq
    m._check_zinb_step_state("test", st)
    hn = 2 * (D_ * H_ + D_)
    assert tuple(opt.hp_exp_avg.shape) == (A, hn) and opt.exp_avg.numel() == m.flat_parameters().numel()
    # recognisable moments: every buffer entry its own value
    opt.exp_avg.copy_(torch.arange(opt.exp_avg.numel(), dtype=torch.float32))
    opt.exp_avg_sq.copy_(torch.arange(opt.exp_avg.numel(), dtype=torch.float32) + 0.5)
    opt.hp_exp_avg.copy_(-1.0 - torch.arange(A * hn, dtype=torch.float32).view(A, hn))
    opt.hp_exp_avg_sq.copy_(-1.5 - torch.arange(A * hn, dtype=torch.float32).view(A, hn))
    st["step"] = 3                                              # what zinb_train_step does to the dict it is handed
    assert opt.step_count == 3
    sd = opt.state_dict()
    assert sorted(sd["state"]) == list(range(32 * A))
    for i, p in enumerate(params):
        e = sd["state"][i]
        assert e["exp_avg"].shape == p.shape and e["exp_avg_sq"].shape == p.shape and float(e["step"]) == 3.0
    # the head tensors sit at mmvae_zinb_head_layout's offsets of their arm's row; the 28 at mmvae_param_layout's
    index = {id(p): i for i, p in enumerate(params)}
    lay, hl = m._layout, N.zinb_head_layout(m._dims(2))
    offs = [0, D_ * H_, D_ * H_ + D_, 2 * D_ * H_ + D_]
    assert list(hl.offset) == offs
    for a in range(A):
        for j, (name, kind) in enumerate(m._ZINB_PR):
            p = getattr(getattr(m, name)[a], kind)
            e = sd["state"][index[id(p)]]
            assert torch.equal(e["exp_avg"].flatten(), opt.hp_exp_avg[a, offs[j]: offs[j] + p.numel()])
            assert torch.equal(e["exp_avg_sq"].flatten(), opt.hp_exp_avg_sq[a, offs[j]: offs[j] + p.numel()])
        for tn in range(N.N_PARAM_TENSORS):
            p = m._param_of(tn, a)
            o = a * int(lay.per_arm) + int(lay.offset[tn])
            assert torch.equal(sd["state"][index[id(p)]]["exp_avg"].flatten(), opt.exp_avg[o: o + p.numel()])
    assert len({float(e["exp_avg"].flatten()[0]) for e in sd["state"].values()}) == 32 * A      # no two share a view
    # into torch.optim.Adam and back
    adam = torch.optim.Adam(m.parameters(), lr=0.5)
    adam.load_state_dict(sd)
    assert adam.param_groups[0]["lr"] == 1e-3
    for i, p in enumerate(params):
        assert torch.equal(adam.state[p]["exp_avg"], sd["state"][i]["exp_avg"]) and float(adam.state[p]["step"]) == 3.0
    t2 = _trainer()
    t2.optimizer.load_state_dict(adam.state_dict())
    o2 = t2.optimizer
    assert o2.step_count == 3 and o2.zinb_state()["step"] == 3
    for k in ("exp_avg", "exp_avg_sq", "hp_exp_avg", "hp_exp_avg_sq"):
        got, want = getattr(o2, k), getattr(opt, k)
        if k.startswith("hp_"):
            assert torch.equal(got, want), k
        else:                                                   # the alignment gaps of the flat buffer belong to no parameter
            used = torch.zeros(want.numel(), dtype=torch.bool)
            for a in range(A):
                for tn in range(N.N_PARAM_TENSORS):
                    o = a * int(lay.per_arm) + int(lay.offset[tn])
                    used[o: o + m._param_of(tn, a).numel()] = True
            assert torch.equal(got[used], want[used]) and not bool(got[~used].any()), k


@needs_lib
def test_bind_grads_gives_every_parameter_its_own_view():
    t = _trainer()
    m = t.model
    m.bind_grads()
    _, hg = m.zinb_heads_flat()
    flat_g = m.flat_grad()
    lo, hi = flat_g.data_ptr(), flat_g.data_ptr() + 4 * flat_g.numel()
    hlo, hhi = hg.data_ptr(), hg.data_ptr() + 4 * hg.numel()
    seen = set()
    for k, p in m.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape, k
        ptr = p.grad.data_ptr()
        head = k.startswith(("fc11_p.", "fc11_r."))
        assert (hlo <= ptr < hhi) if head else (lo <= ptr < hi), k
        assert ptr not in seen
        seen.add(ptr)
    # a head's gradient view is its arm's row of the buffer at the layout's offset, as its parameter is of the heads' buffer
    hp, _ = m.zinb_heads_flat()
    for a, j, p, o in m._zinb_head_params():
        assert p.grad.data_ptr() == hg[a, o:].data_ptr() and p.data_ptr() == hp[a, o:].data_ptr()
    # an MSE model: 28 per arm, as before
    mse = _trainer("MSE").model
    mse.bind_grads()
    assert len(list(mse.parameters())) == 28 * A and all(p.grad is not None for p in mse.parameters())

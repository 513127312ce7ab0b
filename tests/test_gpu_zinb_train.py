"""GPU: a model built with ``mode="ZINB"`` through the trainer's own loop -- ``cpl_mixVAE.train`` / ``_zinb_step`` / ``validate`` /
``eval_model`` / ``summarize_inference``, ``FusedAdam`` on the four moment buffers, ``dist.dp_zinb_train_step`` -- against
the calls they are made of: ``mixVAE_model.zinb_train_step`` and ``zinb_objective``, which tests/test_gpu_zinb_step.py holds
against the fp64 restatement.  No new kernel runs here, so nearly every comparison is bit for bit; the three that are not state
their bound where they are made:
  * a stock ``torch.optim.Adam`` behind the step against ``torch.optim.Adam`` on the host: 3e-8, the gate of
    tests/test_gpu_zinb_step.py::test_adam_step_is_torch_adam_on_the_device_gradients;
  * the history's float32 epoch sums against float64 sums of the same loss vectors: one float32 rounding per operation;
  * the validation entries, accumulated in float64 on the device, against the same float64 sums on the host: 1e-12.
Shapes: the trainer, cells and loader of tests/test_gpu_zinb_step.py (60 cells of 70 genes in batches of 21, 21, 18) and the
row a2_d72_h20_fast_sdrop of tests/zinb_step_cases.py.  Nothing here reads the reference."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import zinb_restatement as ZR  # noqa: E402
from oracle import augmenter as OA  # noqa: E402
from oracle import restatement as R  # noqa: E402
from tests import gpu_util as U  # noqa: E402
from tests import zinb_step_cases as Z  # noqa: E402
from tests.test_gpu_zinb_step import A_, BATCH, CC, DM, HF, LD, N_CELLS, SS, bits, build, grads_of, loader, trainer  # noqa: E402
from distributed_vae_amd import _native as N  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = U.DEV
S = Z.S
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOMENTS = ("exp_avg", "exp_avg_sq", "hp_exp_avg", "hp_exp_avg_sq")
NEVER = 2.0                                              # good_enuf_consensus that no consensus reaches: every epoch runs
VAL = dict(lo=0, hi=40, batch=16)                        # validation batches of 16, 16 and 8 cells


def seeded(t, offset=0):
    t.model._noise_seed, t.model._noise_offset = 1234, offset
    return t


def expand(x):
    return x.to(DEV).expand(A_, -1, -1)


def moments(opt):
    opt._bind()
    return {k: getattr(opt, k).detach().clone() for k in MOMENTS}


def assert_same_model(a, b, what=""):
    sa, sb = bits(a), bits(b)
    assert sorted(sa) == sorted(sb)
    diff = [k for k in sa if not torch.equal(sa[k], sb[k])]
    assert not diff, (what, diff)


def assert_same_moments(got, want, what=""):
    for k in MOMENTS:
        assert torch.equal(got[k].reshape(-1), want[k].reshape(-1)), (what, k)
        assert bool(want[k].any()), (what, k)


def vec_of(t9):
    """zinb_objective's 9-tuple in the order of the loss vector."""
    return torch.stack([t9[0], t9[2], t9[3], t9[4], t9[5], *t9[1], *t9[6], *t9[8]])


@functools.lru_cache(maxsize=None)
def trained(n_epoch, with_val):
    t = seeded(trainer())
    hist = t.train(loader(), loader(**VAL) if with_val else None, n_epoch=n_epoch, good_enuf_consensus=NEVER)
    torch.cuda.synchronize()
    return t, hist


@functools.lru_cache(maxsize=None)
def explicit(n_epoch, with_val):
    """The calls ``train`` is made of, in its order: per epoch ``zinb_train_step`` on every batch, ``consensus`` on the training
    loader, then (with a validation loader) ``zinb_objective`` on every validation batch.  Returns the trainer, the state the
    steps updated, the per-epoch lists of step loss vectors and validation loss vectors, and the consensus values."""
    from distributed_vae_amd._utils import confmat_counts, consensus_from_counts
    t = seeded(trainer())
    m = t.model
    st = m.zinb_step_state()
    steps, vals, cons, cons_val = [], [], [], []
    for _ in range(n_epoch):
        m.train()
        steps.append([m.zinb_train_step(expand(x), t.temp, state=st, do_adam=True, lr=1e-3).clone() for x, _ in loader()])
        cons.append(t.consensus(loader(), whole_set=False))
        if with_val:
            m.eval()
            counts = confmat_counts(A_, CC, DEV)
            ep = []
            for x, _ in loader(**VAL):
                ep.append(vec_of(m.zinb_objective(expand(x), t.temp)))
                N.confmat_accumulate(N.classify(m._engine.ws_view("c", CC)), CC, counts)
            vals.append(ep)
            cons_val.append(float(np.mean(consensus_from_counts(counts).cpu().numpy())))
            m.train()
    torch.cuda.synchronize()
    return t, st, steps, vals, cons, cons_val


# ---- 1. train() is the ZINB step ---------------------------------------------------------------------------------------------
def test_train_is_the_zinb_step_bit_for_bit():
    """Two epochs of ``train`` on an unshuffled device loader against the explicit loop, and -- ``consensus`` consuming no
    noise -- against ``fit_zinb`` with the optimizer's hyper-parameters: the flat parameters, the heads, the BatchNorm buffers
    and counters (all in the state dict) and all four moment buffers.  On the parent commit ``train`` raises."""
    # consensus consumes no noise and no step id: the explicit loop's order is then fit_zinb's
    t0 = seeded(trainer())
    before = (t0.model._noise_offset, t0.model._step_id)
    t0.consensus(loader(), whole_set=False)
    assert (t0.model._noise_offset, t0.model._step_id) == before

    t, hist = trained(2, False)
    te, st, steps, _, cons, _ = explicit(2, False)
    n_steps = 2 * len(loader())
    assert len(loader()) == -(-N_CELLS // BATCH) == 3 and all(len(ep) == 3 for ep in steps)
    assert t.optimizer.step_count == st["step"] == n_steps and t.model._noise_offset == te.model._noise_offset == n_steps
    assert_same_model(t.model, te.model, "train against the explicit loop")
    assert_same_moments(moments(t.optimizer), st, "train against the explicit loop")
    assert hist["consensus_train"] == cons and hist["stopped_at"] == 1 and hist["bf16_storage"] is False
    assert not t.used_bf16_storage and t.model.training
    # fit_zinb
    tf = seeded(trainer())
    r = tf.fit_zinb(loader(), 2, lr=1e-3)
    assert_same_model(t.model, tf.model, "train against fit_zinb")
    assert_same_moments(moments(t.optimizer), r["state"], "train against fit_zinb")
    # every tensor moved
    start = bits(trainer().model)
    after = bits(t.model)
    assert all(not torch.equal(start[k], after[k]) for k in start if not k.startswith("batch_s.")), "every tensor is trained"
    # the unpipelined loop gives the same bits
    tu = seeded(trainer())
    tu.pipeline = False
    tu.train(loader(), None, n_epoch=2, good_enuf_consensus=NEVER)
    assert_same_model(t.model, tu.model, "pipelined against pipeline=False")
    assert_same_moments(moments(t.optimizer), moments(tu.optimizer), "pipelined against pipeline=False")


# ---- 2. the history ----------------------------------------------------------------------------------------------------------
def test_history_is_formed_from_the_step_loss_vectors_and_zinb_objective():
    """``losses``, ``c_dists`` and ``loss_recs`` are float32 sums of the steps' loss vectors divided in float32 (``rec[a] / D /
    steps`` taken literally): against float64 sums of the same vectors, one float32 rounding of at most 2^-24 of the sum of
    magnitudes per operation -- n - 1 additions and one division (two for ``loss_recs``), and one more for the second-order
    terms.  The validation entries are float64 sums on the device: 1e-12."""
    t, hist = trained(2, True)
    te, st, steps, vals, cons, cons_val = explicit(2, True)
    assert_same_model(t.model, te.model, "train with a validation loader against the explicit loop")
    assert_same_moments(moments(t.optimizer), st)
    u = 2.0 ** -24
    for e in range(2):
        V = torch.stack(steps[e]).double().cpu().numpy()
        n = V.shape[0]
        assert n == 3 and np.all(np.isfinite(V))

        def check(name, got, col, div, ops):
            want, mag = V[:, col].sum() / div, np.abs(V[:, col]).sum() / div
            print(f"  epoch {e} {name}: history {float(got)!r}, float64 {want!r}, bound {ops * u * mag:.3e}")
            assert abs(float(got) - want) <= ops * u * mag, (name, e)

        check("losses", hist["losses"][e], N.LOSS_TOTAL, n, n + 1)
        check("c_dists", hist["c_dists"][e], N.LOSS_CDIST, n, n + 1)
        check("loss_joints", hist["loss_joints"][e], N.LOSS_JOINT, n, n + 1)
        for a in range(A_):
            check(f"loss_recs[{a}]", hist["loss_recs"][a][e], N.LOSS_REC0 + a, DM * n, n + 2)
        W = torch.stack(vals[e]).double().cpu().numpy()
        nb = len(loader(**VAL))
        assert W.shape[0] == nb == 3
        want_loss = W[:, N.LOSS_TOTAL].sum() / nb
        want_rec = W[:, N.LOSS_REC0: N.LOSS_REC0 + A_].sum() / DM / nb / A_
        print(f"  epoch {e} validation: {hist['validation_loss'][e]!r} / {want_loss!r}, rec {hist['validation_rec_loss'][e]!r} / {want_rec!r}")
        assert abs(hist["validation_loss"][e] - want_loss) <= 1e-12 * abs(want_loss)
        assert abs(hist["validation_rec_loss"][e] - want_rec) <= 1e-12 * abs(want_rec)
        assert hist["consensus_val"][e] == cons_val[e] and hist["consensus_train"][e] == cons[e]
    assert len(hist["epoch_times"]) == 2 and hist["stopped_at"] == 1


# ---- 3. the gradient path ----------------------------------------------------------------------------------------------------
ROW = "a2_d72_h20_fast_sdrop"


def row_trainer(o, optimizer=None):
    """A trainer around a model at the row's operating point, weights and noise."""
    from distributed_vae_amd.cpl_mixvae import FusedAdam, cpl_mixVAE
    h, row = o["h"], o["row"]
    t = cpl_mixVAE(saving_folder="", device=0, save_flag=False)
    t.init_model(n_categories=row.C, state_dim=row.S, input_dim=row.D, fc_dim=row.H, lowD_dim=row.L, n_arm=row.A, temp=row.temp,
                 mode="ZINB")
    t.model = build(h, o["sd"])
    t.model.set_explicit_noise(U.noise_to_device(o["noise"]))
    t.optimizer = FusedAdam(t.model, lr=1e-3) if optimizer is None else optimizer(t.model.parameters())
    return t


def test_stock_adam_behind_the_step_is_torch_adam_on_the_device_gradients():
    Z.assert_exposes(ROW)
    o = Z.oracle(ROW)
    h, row = o["h"], o["row"]
    xs = o["x"].to(DEV).expand(h.n_arm, -1, -1)
    # the device's gradients, and torch's Adam on them on the host
    m0 = build(h, o["sd"])
    m0.set_explicit_noise(U.noise_to_device(o["noise"]))
    buf0 = m0.zinb_train_step(xs, row.temp, do_adam=False).clone()
    g = grads_of(m0)
    assert len(g) == 32 * h.n_arm
    ref = {k: o["sd"][k].clone().requires_grad_() for k in g}
    for k, p in ref.items():
        p.grad = g[k].clone()
    torch.optim.Adam(list(ref.values()), lr=1e-3).step()
    # one _zinb_step with a stock optimizer assigned to the trainer
    t = row_trainer(o, lambda ps: torch.optim.Adam(ps, lr=1e-3))
    buf = t._zinb_step(xs).clone()
    torch.cuda.synchronize()
    assert torch.equal(buf, buf0)
    for k, p in t.model.named_parameters():
        assert p.grad is not None and torch.equal(p.grad.cpu(), g[k]), k       # bind_grads: every parameter its own gradient
    sd = t.model.state_dict()
    worst = max(float((sd[k].cpu() - ref[k].detach()).abs().max()) for k in g)
    moved = min(float((sd[k].cpu() - o["sd"][k]).abs().max()) for k in g)
    print(f"\n{ROW}: largest difference from torch's Adam {worst:.3e}; every tensor moved by at least {moved:.3e}")
    assert worst <= 3e-8 and moved > 1e-4
    # FusedAdam.step() behind zinb_train_step(do_adam=False): both buffers, as the fused step updates them
    tf = row_trainer(o)
    tf.model.zinb_train_step(xs, row.temp, do_adam=False)
    tf.optimizer.step()
    tg = row_trainer(o)
    tg._zinb_step(xs)
    torch.cuda.synchronize()
    assert_same_model(tf.model, tg.model, "step() behind do_adam=False against the fused update")
    assert_same_moments(moments(tf.optimizer), moments(tg.optimizer))


def test_fused_adam_step_is_zinb_train_step_with_the_optimizers_state():
    o = Z.oracle(ROW)
    h, row = o["h"], o["row"]
    xs = o["x"].to(DEV).expand(h.n_arm, -1, -1)
    t = row_trainer(o)
    st0 = t.optimizer.zinb_state()
    buf = t._zinb_step(xs).clone()
    m = build(h, o["sd"])
    m.set_explicit_noise(U.noise_to_device(o["noise"]))
    st = m.zinb_step_state()
    want = m.zinb_train_step(xs, row.temp, state=st, do_adam=True, lr=1e-3).clone()
    torch.cuda.synchronize()
    assert torch.equal(buf, want)
    assert_same_model(t.model, m)
    assert_same_moments(moments(t.optimizer), st)
    # the state handed to the step is the optimizer's own: the same dict, the same buffers, one step count
    assert t.optimizer.zinb_state() is st0 and st0["exp_avg"] is t.optimizer.exp_avg and st0["hp_exp_avg"] is t.optimizer.hp_exp_avg
    assert t.optimizer.step_count == st0["step"] == st["step"] == 1
    # lr, betas, eps and weight_decay come from param_groups[0]
    t2, m2 = row_trainer(o), build(h, o["sd"])
    m2.set_explicit_noise(U.noise_to_device(o["noise"]))
    t2.optimizer.param_groups[0].update(lr=3e-3, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.01)
    t2._zinb_step(xs)
    m2.zinb_train_step(xs, row.temp, state=m2.zinb_step_state(), lr=3e-3, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.01)
    torch.cuda.synchronize()
    assert_same_model(t2.model, m2)
    assert not torch.equal(t2.model.flat_parameters(), t.model.flat_parameters())


# ---- 4. the checkpoint -------------------------------------------------------------------------------------------------------
def test_checkpoint_resumes_bit_for_bit_and_round_trips_through_torch_adam(tmp_path):
    """2 epochs, ``save_checkpoint``, a fresh trainer through ``init_model(trained_model=...)`` and 2 more epochs equal 4.  A
    trainer made from a checkpoint has ``init = False``, with which ``train`` returns at once as the reference's does (it goes
    on to its pruning phase): the test sets ``init`` back.  The Philox offset is the model's, not the checkpoint's: carried over
    by hand, as tests/test_gpu_zinb_step.py's resumed ``fit_zinb`` carries it in the model it keeps."""
    from distributed_vae_amd.cpl_mixvae import cpl_mixVAE
    t4, _ = trained(4, False)
    t2 = seeded(trainer())
    t2.train(loader(), None, n_epoch=2, good_enuf_consensus=NEVER)
    path = str(tmp_path / "zinb.pth")
    t2.save_checkpoint(path)
    ck = torch.load(path, map_location="cpu", weights_only=True)
    n_params = len(list(t2.model.parameters()))
    assert n_params == 32 * A_ and sorted(ck["optimizer_state_dict"]["state"]) == list(range(n_params))
    torch.manual_seed(99)                                                    # other initial weights: the checkpoint's must win
    t3 = cpl_mixVAE(saving_folder="", device=0, save_flag=False)
    t3.init_model(n_categories=CC, state_dim=SS, input_dim=DM, fc_dim=HF, lowD_dim=LD, x_drop=0.5, s_drop=0.2, n_arm=A_, temp=1.0,
                  tau=0.005, mode="ZINB", trained_model=path)
    assert t3.init is False and t3.train(loader(), None, n_epoch=2) == {}
    assert_same_model(t3.model, t2.model, "the loaded checkpoint")
    assert_same_moments(moments(t3.optimizer), moments(t2.optimizer), "the loaded checkpoint")
    assert t3.optimizer.step_count == t2.optimizer.step_count == 6
    t3.init = True
    seeded(t3, offset=t2.model._noise_offset)
    t3.train(loader(), None, n_epoch=2, good_enuf_consensus=NEVER)
    torch.cuda.synchronize()
    assert_same_model(t3.model, t4.model, "2 + 2 epochs against 4")
    assert_same_moments(moments(t3.optimizer), moments(t4.optimizer), "2 + 2 epochs against 4")
    assert t3.optimizer.step_count == t4.optimizer.step_count == 12
    # the saved optimizer state into torch.optim.Adam, and from there back into a FusedAdam
    adam = torch.optim.Adam(t2.model.parameters())
    adam.load_state_dict(ck["optimizer_state_dict"])
    for i, p in enumerate(t2.model.parameters()):
        e = ck["optimizer_state_dict"]["state"][i]
        assert adam.state[p]["exp_avg"].shape == p.shape and torch.equal(adam.state[p]["exp_avg"].cpu(), e["exp_avg"])
        assert torch.equal(adam.state[p]["exp_avg_sq"].cpu(), e["exp_avg_sq"]) and float(adam.state[p]["step"]) == 6.0
    t5 = trainer()
    t5.optimizer.load_state_dict(adam.state_dict())
    assert_same_moments(moments(t5.optimizer), moments(t2.optimizer), "through torch.optim.Adam")
    assert t5.optimizer.step_count == 6


# ---- 5. the augmenter --------------------------------------------------------------------------------------------------------
DA, NZ, ZD, ND = 72, 8, 4, 40                            # the augmenter reads rows of 16 bytes: D = 72, one full gene tile and 8


@functools.lru_cache(maxsize=None)
def cells72():
    return ZR.counts_matrix(N_CELLS, DA, torch.Generator().manual_seed(9)).to(DEV)


def aug_trainer(pipe):
    from distributed_vae_amd.augmentation import Augmenter_smartseq
    from distributed_vae_amd.cpl_mixvae import cpl_mixVAE
    torch.manual_seed(4)
    t = cpl_mixVAE(saving_folder="", device=0, save_flag=False)
    t.init_model(n_categories=CC, state_dim=SS, input_dim=DA, fc_dim=HF, lowD_dim=LD, x_drop=0.5, s_drop=0.2, n_arm=A_, temp=1.0,
                 tau=0.005, mode="ZINB")
    netA = Augmenter_smartseq(NZ, ZD, DA, ND)
    netA.load_state_dict(OA.random_state_dict(NZ, ZD, DA, ND, seed=2))
    t.set_augmenter(netA)
    t.pipeline = pipe
    return seeded(t)


def loader72():
    from distributed_vae_amd.utils.dataloader import DeviceLoader
    return DeviceLoader(cells72(), torch.arange(N_CELLS), BATCH, False, False)


def test_augmented_epoch_pipelined_equals_unpipelined_and_feeds_each_arm_its_own_batch():
    res = []
    for pipe in (True, False):
        t = aug_trainer(pipe)
        torch.manual_seed(77)                                   # the augmenter's torch.randn draws
        bufs = [b.clone() for b in t.epoch_steps(loader72())]
        torch.cuda.synchronize()
        res.append((torch.stack(bufs), bits(t.model), moments(t.optimizer)))
    assert res[0][0].shape[0] == 3 and bool(torch.isfinite(res[0][0]).all())
    assert torch.equal(res[0][0], res[1][0]) and all(torch.equal(res[0][1][k], res[1][1][k]) for k in res[0][1])
    assert_same_moments(res[0][2], res[1][2])
    # the first step by hand: the augmenter, then zinb_train_step on its per-arm output
    x0 = cells72()[:BATCH]
    th = aug_trainer(False)
    torch.manual_seed(77)
    xa = th.netA(x0.expand(A_, -1, -1), True, 0.1)[1]
    assert xa.shape == (A_, BATCH, DA) and not torch.equal(xa[0], xa[1]) and bool((xa >= 0).all())
    m = th.model
    buf = m.zinb_train_step(xa, th.temp, do_adam=False).clone()
    assert torch.equal(buf, res[1][0][0])
    # rec[a] is the ZINB loss of arm a's OWN augmented batch: mmvae_zinb_nll on the step's d10 and xa[a], to the rounding of
    # the float32 it is stored in (the check of tests/test_gpu_zinb_step.py), and not the other arm's batch
    d10 = m._engine.ws_view("d10", HF)
    for a in range(A_):
        own, other = (float(N.zinb_nll(d10[a], *m._zinb_layers(a), xa[b].contiguous())[0].sum()) / (BATCH * DA) for b in (a, 1 - a))
        got = float(buf[N.LOSS_REC0 + a])
        print(f"  arm {a}: rec {got!r}, zinb_nll on its own augmented batch {own!r}, on the other arm's {other!r}")
        assert abs(got - own) <= float(np.spacing(np.float32(abs(own)))) < abs(got - other)
    # and with the update: the trainer's first step
    t1, t2 = aug_trainer(False), aug_trainer(False)
    torch.manual_seed(77)
    b1 = t1.train_step(x0).clone()
    torch.manual_seed(77)
    xa2 = t2.netA(x0.expand(A_, -1, -1), True, 0.1)[1]
    b2 = t2.model.zinb_train_step(xa2, t2.temp, state=t2.model.zinb_step_state(), lr=1e-3).clone()
    torch.cuda.synchronize()
    assert torch.equal(xa2, xa) and torch.equal(b1, b2) and torch.equal(b1, buf)
    assert_same_model(t1.model, t2.model, "train_step against the augmenter and zinb_train_step by hand")


# ---- 6. evaluation -----------------------------------------------------------------------------------------------------------
SUMMARY_KEYS = {"recon_loss", "dc", "d_qc", "con_min", "con_mean", "num_pruned", "pred_label", "consensus", "armA_vs_armB",
                "prune_indx", "nprune_indx", "state_mu", "state_var", "sample_id", "c_prob", "lowD_x", "x_rec"}


def test_eval_model_validate_and_summarize_inference(tmp_path):
    from distributed_vae_amd.eval_models import summarize_inference
    tz = trainer()                                           # a copy of the shared two-epoch run: that one stays as it is
    tz.model.load_state_dict(bits(trained(2, False)[0].model))
    ck0 = str(tmp_path / "a.pth")
    tz.save_checkpoint(ck0)
    tm = trainer(mode="MSE")
    tm.model.load_state_dict({k: v for k, v in bits(tz.model).items() if not k.startswith(("fc11_p.", "fc11_r."))})
    dl = loader(**VAL)
    ez, em = seeded(tz).eval_model(dl), seeded(tm).eval_model(dl)
    assert list(ez) == list(em)
    for k in ez:
        if k == "total_loss_rec":
            continue
        a, b = np.asarray(ez[k]), np.asarray(em[k])
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), k
    assert tz.model.training and tm.model.training           # eval_model restores the mode
    # total_loss_rec: the mean over batches of zinb_objective's rec
    seeded(tz).model.eval()
    vecs = torch.stack([vec_of(tz.model.zinb_objective(expand(x), tz.temp, mask=np.arange(CC))) for x, _ in dl])
    lv = vecs.double().cpu().numpy()
    want = lv[:, N.LOSS_REC0:N.LOSS_REC0 + A_].mean(axis=0)
    print(f"\n  total_loss_rec {ez['total_loss_rec']}, zinb_objective {want}; MSE twin {em['total_loss_rec']}")
    assert ez["total_loss_rec"].dtype == np.float64 and np.array_equal(ez["total_loss_rec"], want)
    assert np.array_equal(ez["total_likelihood"], lv[:, N.LOSS_REC0 + 2 * A_:].mean(axis=0))
    assert not np.array_equal(ez["total_loss_rec"], em["total_loss_rec"])
    # validate(full=True): the same formulas on zinb_objective (float64 sums on the device: 1e-12)
    tz.model.train()
    val_loss, val_rec, val_cons = seeded(tz).validate(dl, full=True)
    assert tz.model.training
    nb = len(dl)
    want_loss, want_rec = lv[:, N.LOSS_TOTAL].sum() / nb, lv[:, N.LOSS_REC0:N.LOSS_REC0 + A_].sum() / DM / nb / A_
    assert abs(val_loss - want_loss) <= 1e-12 * abs(want_loss) and abs(val_rec - want_rec) <= 1e-12 * abs(want_rec)
    assert val_cons == ez["cnss"] and seeded(tz).validate(dl) == val_rec
    # summarize_inference on two checkpoints
    t1 = seeded(trainer())
    t1.train(loader(), None, n_epoch=1, good_enuf_consensus=NEVER)
    ck1 = str(tmp_path / "b.pth")
    t1.save_checkpoint(ck1)
    ts = trainer()
    evs = []
    seeded(ts)
    for f in (ck0, ck1):
        ts.load_model(f)
        evs.append(ts.eval_model(dl))
    seeded(ts)
    summ = summarize_inference(ts, [ck0, ck1], dl)
    assert set(summ) == SUMMARY_KEYS
    for a in range(A_):
        assert len(summ["recon_loss"][a]) == 2
        for f in range(2):
            assert summ["recon_loss"][a][f] == evs[f]["total_loss_rec"][a]
    assert np.array_equal(evs[0]["total_loss_rec"], ez["total_loss_rec"])      # the checkpoint of the model evaluated above
    assert not np.array_equal(evs[0]["total_loss_rec"], evs[1]["total_loss_rec"])
    assert np.array_equal(summ["state_mu"], evs[1]["state_mu"]) and np.array_equal(summ["pred_label"][0], evs[0]["predicted_label"])


# ---- 7. two ranks on one GPU over gloo ---------------------------------------------------------------------------------------
WS, STEPS = 2, 3
ROW_DP = Z.BY_NAME[ROW]._replace(B=70)                   # B = 70 per rank, D = 72, H = 20


def _dp_hyper():
    r = ROW_DP
    return R.Hyper(input_dim=r.D, fc_dim=r.H, n_categories=r.C, state_dim=r.S, lowD_dim=r.L, x_drop=r.x_drop, s_drop=r.s_drop,
                   n_arm=r.A)


def _dp_state_dict():
    h = _dp_hyper()
    sd = R.init_state_dict(h, 546)
    sd.update(S.init_heads(h, 547))
    return sd


def _dp_data():
    return ZR.counts_matrix(WS * STEPS * ROW_DP.B, ROW_DP.D, torch.Generator().manual_seed(31))


def _dp_noise(rank, step):
    return R.draw_noise(_dp_hyper(), ROW_DP.B, seed=7000 + 100 * rank + step)


def _dp_trainer(dev):
    from distributed_vae_amd.cpl_mixvae import cpl_mixVAE
    r = ROW_DP
    t = cpl_mixVAE(saving_folder="", device=dev, save_flag=False)
    t.init_model(n_categories=r.C, state_dim=r.S, input_dim=r.D, fc_dim=r.H, lowD_dim=r.L, x_drop=r.x_drop, s_drop=r.s_drop,
                 n_arm=r.A, mode="ZINB")
    return t


def _dp_loader(data, rank):
    from distributed_vae_amd.utils.dataloader import DeviceLoader
    return DeviceLoader(data, torch.arange(data.shape[0]), ROW_DP.B, True, True, seed=546, world_size=WS, rank=rank)


def _dp_rank(rank, port, out_dir):
    """Child process: one rank of the two (fresh interpreter, started before it touches the GPU)."""
    sys.path.insert(0, ROOT)
    os.environ["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    import distributed_vae_amd  # noqa: F401
    from distributed_vae_amd import dist as D

    torch.cuda.set_device(0)
    D.init_dist_env(rank, WS, "127.0.0.1", port, backend="gloo")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    ld = _dp_loader(_dp_data().to(dev), rank)
    order = ld.index[ld.epoch_order_device()].cpu().numpy()
    torch.manual_seed(7 + rank)                  # replicas start different: train() broadcasts rank 0's parameters and heads
    t = _dp_trainer(dev)
    if rank == 0:
        t.model.load_state_dict(_dp_state_dict())
    t.model.set_explicit_noise([U.noise_to_device(_dp_noise(rank, s), dev) for s in range(STEPS)])
    ld.set_epoch(0)
    hist = t.train(ld, None, n_epoch=1, rank=rank, ws=WS, good_enuf_consensus=NEVER)
    torch.cuda.synchronize()
    assert not t.model._explicit_noise and t.optimizer.step_count == STEPS
    t.optimizer._bind()
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), order=order, losses=np.array(hist["losses"]),
             **{"m/" + k: getattr(t.optimizer, k).detach().cpu().numpy() for k in MOMENTS},
             **{"p/" + k: v.detach().cpu().numpy() for k, v in t.model.state_dict().items()})
    D.dist.barrier()
    D.dist.destroy_process_group()


def test_two_ranks_on_one_gpu_against_the_virtual_rank_loop(tmp_path):
    """Bit for bit, not within a tolerance: both sides run the same deterministic kernels on the same device.  The ranks'
    gradient average over gloo is (g0 + g1) / 2 in float32 -- one addition, which commutes, and one division -- so every rank
    holds the same bits, and the virtual-rank loop forms exactly that; Adam is then ``FusedAdam.step()`` on both sides.
    (tests/test_gpu_dp.py compares the MSE path with a CPU oracle's trajectory and therefore needs a tolerance.)"""
    import multiprocessing as mp
    from distributed_vae_amd import dist as D
    port = D.find_port()
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_dp_rank, args=(r, port, str(tmp_path))) for r in range(WS)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(300)
        assert p.exitcode == 0, p.exitcode
    out = [np.load(os.path.join(str(tmp_path), f"rank{r}.npz")) for r in range(WS)]
    B = ROW_DP.B
    o0, o1 = out[0]["order"], out[1]["order"]
    assert len(o0) == len(o1) == STEPS * B and not set(o0.tolist()) & set(o1.tolist())
    keys = [k for k in out[0].files if k.startswith("p/")]
    params = [k for k in keys if "running" not in k and "num_batches" not in k]
    assert len(params) == 32 * ROW_DP.A and len(keys) == 46 * ROW_DP.A + 4 * ROW_DP.A
    # 1. the replicas: parameters, heads and moments bit-equal; BatchNorm statistics rank-local
    for k in params + ["m/" + k for k in MOMENTS]:
        assert np.array_equal(out[0][k], out[1][k]), k
    assert any(not np.array_equal(out[0][k], out[1][k]) for k in keys if "running_mean" in k)
    assert out[0]["losses"][0] == out[1]["losses"][0] and np.isfinite(out[0]["losses"][0])
    # 2. the virtual-rank loop: two models on the same weights, each its shard and noise, the gradients averaged as
    #    allreduce_mean_ forms them over gloo (sum, then division by the world size), FusedAdam.step() on each
    X = _dp_data().to(DEV)
    ts = [_dp_trainer(torch.device(DEV)) for _ in range(WS)]
    for r, t in enumerate(ts):
        t.model.load_state_dict(_dp_state_dict())
        t.model.train()
        t.model.set_explicit_noise([U.noise_to_device(_dp_noise(r, s)) for s in range(STEPS)])
    for s in range(STEPS):
        for r, t in enumerate(ts):
            rows = torch.from_numpy(out[r]["order"][s * B:(s + 1) * B]).to(DEV)
            t.model.zinb_train_step(X[rows].expand(ROW_DP.A, -1, -1), t.temp, do_adam=False)
        for pick in (lambda m: m.flat_grad(), lambda m: m.zinb_heads_flat()[1]):
            mean = pick(ts[0].model) + pick(ts[1].model)
            mean.div_(WS)
            for t in ts:
                pick(t.model).copy_(mean)
        for t in ts:
            t.optimizer.step()
    torch.cuda.synchronize()
    for r, t in enumerate(ts):
        sd = t.model.state_dict()
        for k in keys:                                   # parameters and heads; rank r's own BatchNorm buffers and counters
            assert np.array_equal(out[r][k], sd[k[2:]].detach().cpu().numpy()), (r, k)
        for k in MOMENTS:
            assert np.array_equal(out[r]["m/" + k], getattr(t.optimizer, k).cpu().numpy()), (r, k)
    moved = min(float(np.abs(out[0][k] - _dp_state_dict()[k[2:]].numpy()).max()) for k in params)
    assert moved > 1e-4, moved


# ---- 8. what stays refused ---------------------------------------------------------------------------------------------------
def test_pinned_refusals_hold_beside_the_new_path(monkeypatch):
    from distributed_vae_amd import dist as DD
    from distributed_vae_amd import nn_model as NM
    from distributed_vae_amd.cpl_mixvae import FusedAdam
    t = seeded(trainer())
    m = t.model
    h = torch.rand(4, DM, device=DEV)
    xs = h.expand(A_, -1, -1)
    msg = "training under loss_mode='ZINB' is not built"
    with pytest.raises(NotImplementedError, match=msg):
        m.fused_train_step(xs, 1.0, None, do_adam=False)
    with pytest.raises(NotImplementedError, match=msg):
        m.fused_train_step_rows(h, torch.arange(4, device=DEV), 1.0, None, do_adam=False)
    with pytest.raises(NotImplementedError, match=msg):
        DD.dp_train_step(m, xs, 1.0, None, rehearse=True)
    with pytest.raises(NotImplementedError, match=msg):
        t._step(xs)
    with pytest.raises(NotImplementedError, match="zinb_nll"):
        m.loss([h] * A_, [], [], None, [h] * A_, [h] * A_, [h] * A_, [h] * A_)
    with pytest.raises(AssertionError, match="ZINB not implemented"):
        m.train()(xs, 1.0)
    with pytest.raises(NotImplementedError, match="no backward"):
        NM.zinb_loss(h.clone().requires_grad_(), h, h, h)
    # the engine's refusal of a category mask
    eng = m._ensure(4)
    hp, hg = m.zinb_heads_flat()
    xt, xst = m._prep_x(xs)
    hy = m._hyper(1.0, False)
    hy.cat_mask[0] = 0b1011
    with pytest.raises(NotImplementedError, match="category mask"):
        eng.zinb_train_step(hy, N.make_noise(None, 1, 1), m._flat, hp, m._bn_flat, m._nbt, xt, xst, m._flat_grad, hg, False, None,
                            None, None, None, 1, 0.0)
    # the trainer's own refusals on the device, and fit_zinb's, with their messages
    before = bits(m)
    m.gemm_dtype = "bf16"
    for call in (lambda: t._zinb_step(xs), lambda: t.train(loader(), None, 1), lambda: t.fit_zinb(loader(), 1)):
        with pytest.raises(NotImplementedError, match="bf16"):
            call()
    m.gemm_dtype = "fp32"
    with torch.no_grad():
        for a in range(A_):
            m.fcc[a].bias[3] = 0.0
    for call in (lambda: t.train(loader(), None, 1), lambda: t.fit_zinb(loader(), 1)):
        with pytest.raises(NotImplementedError, match="pruned"):
            call()
    m.load_state_dict(before)
    t._prune_mask = [0, 1]
    with pytest.raises(NotImplementedError, match="pruned"):
        t._zinb_step(xs)
    t._prune_mask = None
    with pytest.raises(NotImplementedError, match="ZINB"):
        t.prune(loader(), None, 1)
    with pytest.raises(NotImplementedError, match="decoupled"):
        FusedAdam(m, decoupled=True)
    monkeypatch.setattr(DD, "is_dist", lambda: True)
    with pytest.raises(NotImplementedError, match="not data-parallel"):
        t.fit_zinb(loader(), 1)
    monkeypatch.undo()
    assert m._noise_offset == 0 and t.optimizer.step_count == 0
    after = bits(m)
    assert all(torch.equal(before[k], after[k]) for k in before)
    assert N.lib().mmvae_abi_version() == 5 and len(N.PLAN_NAMES) == 23

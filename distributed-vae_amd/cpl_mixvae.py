"""Drop-in for the hot path of the reference trainer ``mmidas/cpl_mixvae.py::cpl_mixVAE``.

Mirrors ``__init__`` (:153-186), ``init_model`` (:193-286), ``load_model`` (:317-321) and the
training loop of ``train`` (:323-492: per-batch driver :415-478, epoch reductions :480-492,
checkpoints :777-788) on top of the fused HIP train step.  Out of the hot path and therefore not
here: wandb/matplotlib reporting.  The augmenter in front of the step
(:182-186, :422-423) is ``distributed_vae_amd.augmentation``.  The pruning phase (:996-1444), which upstream
switches off inside ``train``, is the opt-in ``cpl_mixVAE.prune``.
"""
from __future__ import annotations

import os
import time
from typing import Optional

import numpy as np
import torch
from torch import nn

from . import _native as N
from . import dist as D
from .nn_model import VAEConfig, mixVAE_model  # noqa: F401


class FusedAdam(torch.optim.Optimizer):
    """torch.optim.Adam / AdamW semantics (cpl_mixvae.py:274, train.py:144-147) as ONE HIP kernel over
    the model's flat parameter buffer.  ``state_dict()`` is torch.optim.Adam-compatible so reference
    checkpoints (``optimizer_state_dict``, cpl_mixvae.py:783-786) load and save unchanged.

    On a model built with ``mode="ZINB"`` it owns four moment buffers and one step count: ``exp_avg`` / ``exp_avg_sq`` over
    the flat buffer of the 28 tensors per arm, ``hp_exp_avg`` / ``hp_exp_avg_sq`` over the [A, 2 (D H + D)] buffer of
    ``fc11_p`` / ``fc11_r`` (``mixVAE_model.zinb_heads_flat``).  ``step()`` is then two mmvae_adam_step launches,
    ``state_dict()`` covers all 32 parameters per arm, and ``zinb_state()`` hands the same buffers to
    ``mixVAE_model.zinb_train_step(state=...)``.  ``decoupled=True`` (AdamW) is refused there: the fused ZINB step has not been
    checked against ``torch.optim.AdamW``."""

    def __init__(self, model: mixVAE_model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
                 decoupled=False):
        if decoupled and getattr(model, "loss_mode", "MSE") == "ZINB":
            raise NotImplementedError("FusedAdam(decoupled=True) on a model built with loss_mode='ZINB' is not offered")
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False,
                        foreach=None, capturable=False, differentiable=False, fused=None)
        # the one place the step count lives: the dict ``zinb_state()`` hands to ``zinb_train_step``, which counts in it
        self._zstate = {"kind": "zinb_step", "step": 0}
        super().__init__(list(model.parameters()), defaults)
        self.model = model
        self.decoupled = bool(decoupled)
        self.exp_avg = self.exp_avg_sq = None
        self.hp_exp_avg = self.hp_exp_avg_sq = None

    @property
    def step_count(self) -> int:
        return int(self._zstate["step"])

    @step_count.setter
    def step_count(self, n):
        self._zstate["step"] = int(n)

    def _zinb(self) -> bool:
        return getattr(self.model, "loss_mode", "MSE") == "ZINB"

    def _refuse_decoupled(self):
        if self.decoupled and self._zinb():
            raise NotImplementedError("FusedAdam(decoupled=True) on a model built with loss_mode='ZINB' is not offered")

    def _bind(self, model=None):
        flat = self.model.flat_parameters()
        if self.exp_avg is None or self.exp_avg.device != flat.device or self.exp_avg.numel() != flat.numel():
            old = (self.exp_avg, self.exp_avg_sq)
            self.exp_avg = torch.zeros_like(flat)
            self.exp_avg_sq = torch.zeros_like(flat)
            if old[0] is not None and old[0].numel() == flat.numel():
                self.exp_avg.copy_(old[0])
                self.exp_avg_sq.copy_(old[1])
        if self._zinb():
            hp, _ = self.model.zinb_heads_flat()
            if self.hp_exp_avg is None or self.hp_exp_avg.device != hp.device or self.hp_exp_avg.shape != hp.shape:
                old = (self.hp_exp_avg, self.hp_exp_avg_sq)
                self.hp_exp_avg = torch.zeros_like(hp)
                self.hp_exp_avg_sq = torch.zeros_like(hp)
                if old[0] is not None and old[0].shape == hp.shape:
                    self.hp_exp_avg.copy_(old[0])
                    self.hp_exp_avg_sq.copy_(old[1])

    def zinb_state(self):
        """The state ``mixVAE_model.zinb_train_step(state=...)`` updates in place, made of this optimizer's own four moment
        buffers and its step count (the same dict at every call): a fused ZINB step is this optimizer's step."""
        self._refuse_decoupled()
        self._bind()
        self._zstate.update(exp_avg=self.exp_avg, exp_avg_sq=self.exp_avg_sq, hp_exp_avg=self.hp_exp_avg,
                            hp_exp_avg_sq=self.hp_exp_avg_sq)
        return self._zstate

    @torch.no_grad()
    def step(self, closure=None):
        self._refuse_decoupled()
        self._bind()
        self.step_count += 1
        g = self.param_groups[0]
        N.adam_step(self.model.flat_parameters(), self.model.flat_grad(), self.exp_avg, self.exp_avg_sq,
                    self.step_count, g["lr"], g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"],
                    self.decoupled)
        if self._zinb():
            hp, hg = self.model.zinb_heads_flat()
            N.adam_step(hp, hg, self.hp_exp_avg, self.hp_exp_avg_sq, self.step_count, g["lr"], g["betas"][0],
                        g["betas"][1], g["eps"], g["weight_decay"], False)

    def zero_grad(self, set_to_none: bool = False):
        self.model.flat_grad().zero_()
        if self._zinb():
            self.model.zinb_heads_flat()[1].zero_()

    def _views(self, buf, hbuf=None):
        lay, A = self.model._layout, self.model.n_arm
        out = {}
        for a in range(A):
            for t in range(N.N_PARAM_TENSORS):
                p = self.model._param_of(t, a)
                o = a * int(lay.per_arm) + int(lay.offset[t])
                out[id(p)] = buf[o: o + p.numel()].view(p.shape)
        if hbuf is not None:
            for a, _, p, o in self.model._zinb_head_params():
                out[id(p)] = hbuf[a, o: o + p.numel()].view(p.shape)
        return [out[id(p)] for p in self.model.parameters()]

    def state_dict(self):
        self._bind()
        m, v = self._views(self.exp_avg, self.hp_exp_avg), self._views(self.exp_avg_sq, self.hp_exp_avg_sq)
        n = len(m)
        state = {}
        if self.step_count > 0:
            for i in range(n):
                state[i] = {"step": torch.tensor(float(self.step_count)), "exp_avg": m[i].clone(),
                            "exp_avg_sq": v[i].clone()}
        groups = []
        for g in self.param_groups:
            gg = {k: v_ for k, v_ in g.items() if k != "params"}
            gg["params"] = list(range(n))
            groups.append(gg)
        return {"state": state, "param_groups": groups}

    def load_state_dict(self, sd):
        self._bind()
        m, v = self._views(self.exp_avg, self.hp_exp_avg), self._views(self.exp_avg_sq, self.hp_exp_avg_sq)
        for i, st in sd.get("state", {}).items():
            i = int(i)
            m[i].copy_(st["exp_avg"])
            v[i].copy_(st["exp_avg_sq"])
            self.step_count = int(float(st["step"]))
        for g, src in zip(self.param_groups, sd.get("param_groups", [])):
            for k in ("lr", "betas", "eps", "weight_decay"):
                if k in src:
                    g[k] = tuple(src[k]) if k == "betas" else src[k]


def get_device(device=None) -> torch.device:
    """cpl_mixvae.py:110-125."""
    if device in ("cpu", "mps"):
        return torch.device(device)
    if device == "cuda":
        return torch.device("cuda")
    if isinstance(device, int):
        torch.cuda.set_device(device)
        return torch.device("cuda", device)
    if isinstance(device, torch.device):
        return device
    if device is None:
        return torch.device("cuda") if torch.cuda.is_available() else torch.device("cpu")
    return torch.device(device)


def prune_start(bias):
    """cpl_mixvae.py:998-1000: ``(kept, pruned)`` index arrays from the ``fcc`` bias of arm 0 -- a category is pruned iff its
    bias is exactly zero, so a checkpoint of an already pruned model resumes where it stopped."""
    bias = np.asarray(bias)
    return np.where(bias != 0.0)[0], np.where(bias == 0.0)[0]


def prune_decision(c_agreement, kept, min_con, pr, max_prun_it):
    """cpl_mixvae.py:1108-1132: the category to prune next, or None to stop.  ``c_agreement``: float64 [C]
    (``cpl_mixVAE.category_agreement``); ``kept``: the indices still in use, ascending.  While ``pr < max_prun_it`` and the
    smallest agreement among the kept categories is at most ``min_con``, that category goes (``np.argmin``: the first on
    ties).  The last kept category is never pruned (the reference would go on to a forward over an empty mask, which fails)."""
    kept = np.asarray(kept, dtype=np.int64)
    if kept.size <= 1 or not pr < max_prun_it:
        return None
    agreement = np.asarray(c_agreement, dtype=np.float64)[kept]
    if not np.min(agreement) <= min_con:
        return None
    return int(kept[np.argmin(agreement)])


class cpl_mixVAE:
    def __init__(self, saving_folder="", aug_file="", device=None, eps=1e-8, save_flag=True, load_weights=True):
        self.eps = eps
        self.save = save_flag
        self.folder = saving_folder
        self.aug_file = aug_file
        self.models = []
        self.device = get_device(device)
        self.aug_model, self.aug_param, self.netA = None, None, None
        self.pipeline = os.environ.get("MMVAE_PIPELINE", "1") != "0"   # see epoch_steps
        # bf16 configuration with a device-resident loader: the step reads x through a bf16 COPY of the matrix and keeps dZ11 as
        # bf16 (the reconstruction loss then sees bf16-rounded x; +50 % resident memory).  An attribute of the trainer (default
        # from MMVAE_BF16_STORAGE, on), recorded per run in ``used_bf16_storage`` and in train()'s history.
        self.bf16_storage = os.environ.get("MMVAE_BF16_STORAGE", "1") != "0"
        self.used_bf16_storage = False
        self._prune_mask = None          # the kept categories while ``prune`` retrains (``_step`` / ``_step_rows`` pass it on)
        if aug_file:                                            # cpl_mixvae.py:182-186
            from .augmentation import mk_augmenter
            self.aug_model, self.aug_param, netA = mk_augmenter(aug_file, load_weights)
            self.set_augmenter(netA)

    def set_augmenter(self, netA):
        """Install an ``Augmenter_smartseq`` (distributed_vae_amd.augmentation) in eval mode on the trainer's device,
        as cpl_mixvae.py:184; ``None`` returns to raw ``x.expand``."""
        self.netA = None if netA is None else netA.to(self.device).eval()
        if self.netA is not None and getattr(self, "model", None) is not None:
            self.netA.gemm_dtype = self.model.gemm_dtype     # the bf16 configuration covers the augmenter's GEMMs too

    def init_model(self, n_categories, state_dim, input_dim, fc_dim=100, lowD_dim=10, x_drop=0.5, s_drop=0.2,
                   lr=0.001, lam=1, lam_pc=1, n_arm=2, temp=1.0, tau=0.005, beta=1.0, hard=False, variational=True,
                   ref_prior=False, trained_model="", n_pr=0, momentum=0.01, mode="MSE", gemm_dtype="fp32"):
        """cpl_mixvae.py:193-286.  ``gemm_dtype`` (not in the reference): "fp32", or "bf16" for BASELINE.json's bf16
        configuration (bf16 operands in the five D x H GEMMs, fp32 everywhere else)."""
        self.lowD_dim = lowD_dim
        self.n_categories = n_categories
        self.state_dim = state_dim
        self.input_dim = input_dim
        self.temp = temp
        self.n_arm = n_arm
        self.fc_dim = fc_dim
        self.ref_prior = ref_prior
        self.model = mixVAE_model(input_dim=input_dim, fc_dim=fc_dim, n_categories=n_categories,
                                  state_dim=state_dim, lowD_dim=lowD_dim, x_drop=x_drop, s_drop=s_drop, n_arm=n_arm,
                                  lam=lam, lam_pc=lam_pc, tau=tau, beta=beta, hard=hard, variational=variational,
                                  device=self.device, eps=self.eps, ref_prior=ref_prior, momentum=momentum,
                                  loss_mode=mode)
        self.model = self.model.to(self.device)
        self.model.gemm_dtype = gemm_dtype
        if self.netA is not None:
            self.netA.gemm_dtype = gemm_dtype
        self.optimizer = FusedAdam(self.model, lr=lr)
        if len(trained_model) > 0:
            loaded = torch.load(trained_model, map_location="cpu", weights_only=True)
            self.model.load_state_dict(loaded["model_state_dict"])
            self.optimizer.load_state_dict(loaded["optimizer_state_dict"])
            self.init = False
            self.n_pr = n_pr
        else:
            self.init = True
            self.n_pr = 0

    def load_model(self, trained_model):
        """cpl_mixvae.py:317-321."""
        loaded = torch.load(trained_model, map_location="cpu", weights_only=True)
        self.model.load_state_dict(loaded["model_state_dict"])
        self.current_time = time.strftime("%Y-%m-%d-%H-%M-%S")

    def save_checkpoint(self, path):
        """Checkpoint dict of cpl_mixvae.py:783-786."""
        torch.save({"model_state_dict": self.model.state_dict(),
                    "optimizer_state_dict": self.optimizer.state_dict()}, path)

    # ---------------------------------------------------------------------------------------
    def _step(self, xs: torch.Tensor):
        """zero_grad / forward / loss / backward / optimizer.step of cpl_mixvae.py:434-463 for one batch.  With the
        trainer's own ``FusedAdam`` the update rides on the gradient reduction of the fused step; any other
        ``torch.optim`` optimizer assigned to ``self.optimizer`` (the reference pattern ``cplMixVAE.optimizer =
        optim.Adam(model.parameters())``, train.py:144-147) gets the gradients of the fused step through each
        parameter's ``.grad`` and steps itself."""
        if D.is_dist():
            return D.dp_train_step(self.model, xs, self.temp, self.optimizer)
        mask = self._prune_mask
        if isinstance(self.optimizer, FusedAdam) and self.optimizer.model is self.model:
            return self.model.fused_train_step(xs, self.temp, self.optimizer, do_adam=True, mask=mask)
        buf = self.model.fused_train_step(xs, self.temp, None, do_adam=False, mask=mask)
        self.model.bind_grads()
        self.optimizer.step()
        if mask is not None:
            self.model.prune_apply(mask, grads=False)            # weight_orig * mask behind a stock optimizer's step
        return buf

    def _is_zinb(self) -> bool:
        return getattr(getattr(self, "model", None), "loss_mode", "MSE") == "ZINB"

    def _zinb_refusals(self, what):
        """What ZINB training does not offer, refused before any device work and before noise is consumed: the bf16
        configuration, a category mask (set by ``prune``, or implied by a model whose ``fcc`` bias has zeros), AdamW through
        ``FusedAdam``."""
        m = self.model
        if m.gemm_dtype == "bf16":
            raise NotImplementedError(f"{what}: gemm_dtype='bf16' is not offered under the ZINB objective (bf16 heads are not built)")
        if (self._prune_mask is not None
                or int(np.count_nonzero(m.fcc[0].bias.detach().cpu().numpy() != 0.0)) < self.n_categories):
            raise NotImplementedError(f"{what}: the model has pruned categories; a category mask is not offered in ZINB training")
        if isinstance(self.optimizer, FusedAdam):
            self.optimizer._refuse_decoupled()

    def _zinb_step(self, xs: torch.Tensor):
        """``_step`` for a model built with ``mode="ZINB"`` (``_step`` itself refuses one): one
        ``mixVAE_model.zinb_train_step`` on ``xs``.  With the trainer's own ``FusedAdam`` the update is the fused step's, on
        the optimizer's own moment buffers and step count (``FusedAdam.zinb_state``) and with ``param_groups[0]``'s ``lr``,
        ``betas``, ``eps`` and ``weight_decay``; any other optimizer assigned to ``self.optimizer`` gets the gradients through
        each parameter's ``.grad`` (``bind_grads``: ``fc11_p`` / ``fc11_r`` included) and steps itself.  Under a process group:
        ``dist.dp_zinb_train_step``.  Returns the device loss vector; no host synchronisation."""
        m, opt = self.model, self.optimizer
        m._need_zinb("_zinb_step()")
        if m.gemm_dtype == "bf16":
            raise NotImplementedError("_zinb_step(): gemm_dtype='bf16' is not offered under the ZINB objective (bf16 heads are not built)")
        if self._prune_mask is not None:
            raise NotImplementedError("_zinb_step(): the model has pruned categories; a category mask is not offered in ZINB training")
        if D.is_dist():
            return D.dp_zinb_train_step(m, xs, self.temp, opt)
        if isinstance(opt, FusedAdam) and opt.model is m:
            g = opt.param_groups[0]
            return m.zinb_train_step(xs, self.temp, state=opt.zinb_state(), do_adam=True, lr=g["lr"], betas=g["betas"],
                                     eps=g["eps"], weight_decay=g["weight_decay"])
        buf = m.zinb_train_step(xs, self.temp, do_adam=False)
        m.bind_grads()
        opt.step()
        return buf

    def _step_rows(self, data: torch.Tensor, rows: torch.Tensor, data16=None):
        """``_step`` on the batch ``data[rows]`` read in place (``mixVAE_model.fused_train_step_rows``); ``data16``: the
        matrix's bf16 copy for the bf16 configuration (bf16 storage)."""
        if D.is_dist():
            return D.dp_train_step(self.model, None, self.temp, self.optimizer, rows=(data, rows, data16))
        mask = self._prune_mask
        if isinstance(self.optimizer, FusedAdam) and self.optimizer.model is self.model:
            return self.model.fused_train_step_rows(data, rows, self.temp, self.optimizer, do_adam=True, data16=data16,
                                                    mask=mask)
        buf = self.model.fused_train_step_rows(data, rows, self.temp, None, do_adam=False, data16=data16, mask=mask)
        self.model.bind_grads()
        self.optimizer.step()
        if mask is not None:
            self.model.prune_apply(mask, grads=False)
        return buf

    def train_step(self, x: torch.Tensor):
        """One batch of cpl_mixvae.py:416-463 (x -> device, x.expand over arms, [augmenter,] zero_grad, forward,
        loss, backward, optimizer step).  Returns the device loss vector; no host synchronisation."""
        x = x.to(self.device, non_blocking=True)
        xs = x.expand(self.n_arm, -1, -1)
        if self.netA is not None:
            xs = self.netA(xs, True, 0.1)[1]                    # cpl_mixvae.py:422-423
        return (self._zinb_step if self._is_zinb() else self._step)(xs)

    def epoch_steps(self, loader):
        """Generator over the loss vectors of one pass over ``loader`` (the inner loop of cpl_mixvae.py:415-478).

        The loop is software-pipelined over two HIP streams: batch i+1 is *produced* -- fetched from the loader (row
        gather of the device-resident loaders, or the H2D copy of a host batch) and, with an augmenter, passed through
        the frozen eval-mode augmenter -- on a high-priority side stream beside the train step of batch i.  The
        augmenter's GEMMs fill the matrix pipe while the step sits in its latency-bound chain kernels (measured at the
        benchmark shape: 2.93 ms per augmented batch against 3.21 ms back to back).  Same arithmetic and the same order
        of random draws as the unpipelined loop (``pipeline = False`` / MMVAE_PIPELINE=0).

        The step function is picked once per epoch: ``_step``, or ``_zinb_step`` for a model built with ``mode="ZINB"``, which
        always runs this gathered-batch loop (with an augmenter, on each arm's own augmented batch) and never the
        row-indexed steps below."""
        A = self.n_arm
        # a model built with mode="ZINB": ``_zinb_step`` on gathered batches (there is no row-indexed ZINB step), after the
        # refusals of ZINB training; chosen once per epoch
        zinb = self._is_zinb()
        if zinb:
            self._zinb_refusals("epoch_steps()")
            self.used_bf16_storage = False
        step = self._zinb_step if zinb else self._step

        def first(b):
            return b[0] if isinstance(b, (tuple, list)) else b

        # A device-resident loader without an augmenter in front of the step: the batch is never assembled -- the step reads the
        # resident matrix through the epoch's row indices (mmvae_train_step_rows: fc1, the fused fc11 kernel and dW1 take a
        # row map), so a shuffled epoch costs what fixed batches do (the 100 MB row gather per step, and the hook that hid it
        # beside the encoder chain, are gone from this path).  Where the library does not offer it (other GEMM engines,
        # matrices beyond 4 GB) the first step says so and the epoch falls back to gathered batches.
        if (not zinb and self.netA is None and self.device.type == "cuda" and hasattr(loader, "iter_rows")
                and getattr(loader, "data", None) is not None and os.environ.get("MMVAE_ROWS", "1") != "0"
                and getattr(self, "_rows_ok", True)):
            it = loader.iter_rows()
            first_rows = next(it, None)
            if first_rows is None:
                return
            # the bf16 configuration on bf16 storage: the loader keeps a bf16 copy of its matrix (made
            # once) and the GEMMs read that; MMVAE_BF16_STORAGE=0 keeps them on the fp32 matrix
            data16 = None
            if getattr(self.model, "gemm_dtype", "fp32") == "bf16" and hasattr(loader, "data_bf16") and self.bf16_storage:
                data16 = loader.data_bf16()
            self.used_bf16_storage = data16 is not None
            try:
                buf = self._step_rows(loader.data, first_rows, data16)
            except NotImplementedError:
                self._rows_ok = False
                if hasattr(loader, "unread_epoch"):
                    loader.unread_epoch()            # the abandoned iterator had taken this epoch's permutation
            else:
                yield buf
                for rows in it:
                    yield self._step_rows(loader.data, rows, data16)
                return
        if self.device.type != "cuda" or not self.pipeline:
            for b in loader:
                yield self.train_step(first(b))
            return
        # ring buffers (loader batches, augmenter outputs) are reused every few batches: batch k may only be produced once
        # the step that read its slot last (step k - lag) is over; a one-slot ring cannot be pipelined at all
        aug_ring = 3
        lring = int(getattr(loader, "ring", 0))
        lag = min(lring if lring > 0 else aug_ring, aug_ring)
        if lag < 2:
            for b in loader:
                yield self.train_step(first(b))
            return
        main = torch.cuda.current_stream(self.device)
        side = N.shared_stream(self.device, "produce")
        # With an augmenter in front of the step and a device-resident loader the batch is not assembled either: the loader keeps
        # its matrix as the augmenter engine's slice planes (made once) and the augmenter's first layer reads the epoch's rows in
        # place (Augmenter_smartseq.forward_rows: no row gather, no per-batch conversion; same results bit for bit).
        # MMVAE_ROWS=0 keeps gathered batches.
        planes, np_aug = None, 0
        if (self.netA is not None and hasattr(loader, "iter_rows") and hasattr(loader, "data_planes")
                and getattr(loader, "data", None) is not None and os.environ.get("MMVAE_ROWS", "1") != "0"
                and hasattr(self.netA, "planes_needed")):
            np_aug = self.netA.planes_needed()
            if np_aug and loader.data.shape[1] == self.netA._dims[0]:
                planes = loader.data_planes(np_aug)
        self.used_aug_rows = planes is not None
        it = loader.iter_rows() if planes is not None else iter(loader)
        aug_out = {}
        done = {}                                               # step index -> main-stream event at its end
        count = [0]

        def produce():
            k = count[0]
            if k - lag in done:
                side.wait_event(done.pop(k - lag))
            b = next(it, None)
            if b is None:
                return None
            if planes is not None:
                key = (k % aug_ring, b.shape[0])
                if key not in aug_out:
                    aug_out[key] = (torch.empty(A, b.shape[0], self.netA._dims[4], device=self.device),
                                    torch.empty(A, b.shape[0], loader.data.shape[1], device=self.device))
                xs = self.netA.forward_rows(planes, loader.data.shape[0], b, A, 0.1, out=aug_out[key])[1]   # cpl_mixvae.py:422-423
                count[0] += 1
                ev = torch.cuda.Event()
                ev.record(side)
                return xs, b, ev
            x = first(b).to(self.device, non_blocking=True)
            xs = x.expand(A, -1, -1)
            if self.netA is not None:
                key = (k % aug_ring, x.shape[0])
                if key not in aug_out:                          # persistent outputs: no allocator traffic per batch
                    aug_out[key] = (torch.empty(A, x.shape[0], self.netA._dims[4], device=self.device),
                                    torch.empty(A, x.shape[0], x.shape[1], device=self.device))
                xs = self.netA(xs, True, 0.1, out=aug_out[key])[1]   # cpl_mixvae.py:422-423
            count[0] += 1
            ev = torch.cuda.Event()
            ev.record(side)
            return xs, x, ev

        side.wait_stream(main)                                  # parameters / loader state written on the main stream
        with torch.cuda.stream(side):
            cur = produce()
        # Without an augmenter the production of a batch is a copy (row gather of a loader the row-indexed step above does
        # not cover, or the H2D copy of a host batch): it is issued BEHIND the step's call, so that it reaches the device
        # some 300 us into the step instead of beside fc1 (measured at the benchmark shape: 0.75 against 0.80 ms per
        # shuffled step).  With an augmenter the production is a 1.7 ms chain of GEMMs: it starts in front of the step.
        late = self.netA is None and not D.is_dist()
        k = 0
        while cur is not None:
            if not late:
                with torch.cuda.stream(side):
                    nxt = produce()
            xs, x, ev = cur
            main.wait_event(ev)
            buf = step(xs)
            if late:
                with torch.cuda.stream(side):
                    nxt = produce()
            x.record_stream(main)                               # produced on the side stream, read on the main one
            fin = torch.cuda.Event()
            fin.record(main)
            done[k] = fin
            done.pop(k - 2 * lag, None)
            k += 1
            yield buf
            cur = nxt

    def train(self, train_loader, test_loader, n_epoch, n_epoch_p=0, c_p=0, c_onehot=0, min_con=0.5,
              max_prun_it=0, rank=None, run=None, ws=1, good_enuf_consensus=0.75):
        """Training loop of cpl_mixvae.py:397-492, the per-epoch consensus on the training set (:563-657), the
        validation block (:665-775), the 10-epoch checkpoint (:777-788) and the stop at ``good_enuf_consensus``
        (:851-927: checkpoint ``cns_cpl_mixVAE_model_before_pruning_A{A}_...pth``, then ``break``).  Pruning
        (:996-1444) is disabled upstream and not offered.  Returns the per-epoch history (the reference returns None and
        hands the same numbers to its logger ``run``).

        A model built with ``mode="ZINB"`` trains through the same loop: ``epoch_steps`` runs ``_zinb_step`` (the fused step
        under the ZINB objective) and ``validate`` takes its losses from ``zinb_objective``; everything else is the same
        code.  ``loss_recs[a]`` keeps the reference's formula taken literally, ``rec[a] / D / steps`` (:475, :491), now
        applied to the ZINB loss -- which is already a mean over the D genes, so the entry is that mean divided by D once
        more.  Refused before any device work (NotImplementedError): ``gemm_dtype="bf16"``, a model with pruned
        categories, AdamW through ``FusedAdam``."""
        A, Dm = self.n_arm, self.input_dim
        dev = self.device
        if not self.init:
            return {}
        if self.n_arm == 1:
            raise ZeroDivisionError("division by zero")   # nn_model.py:592-594
        if self._is_zinb():
            self._zinb_refusals("train()")
        if D.is_dist():
            D.broadcast_flat(self.model.flat_parameters())
            if self._is_zinb():
                D.broadcast_flat(self.model.zinb_heads_flat()[0])          # fc11_p / fc11_r live outside the 28 tensors
        hist = {"losses": [], "loss_joints": [], "loss_recs": [[] for _ in range(A)], "c_ents": [], "c_l2_dists": [],
                "c_dists": [], "validation_loss": [], "validation_rec_loss": [], "consensus_train": [], "consensus_aug": [],
                "consensus_val": [], "epoch_times": [], "stopped_at": None}
        self.current_time = time.strftime("%Y-%m-%d-%H-%M-%S")
        # the reference classifies the training set batch by batch only when the TEST loader's batch size exceeds one,
        # otherwise the whole ``train_loader.dataset.tensors`` (:567 / :617): every row, no shuffle consumed
        whole_train = test_loader is not None and not ((getattr(test_loader, "batch_size", None) or 0) > 1)
        from ._utils import confmat_counts, consensus_from_counts
        E = n_epoch
        for e in range(E):
            t0 = time.time()
            self.model.train()
            acc = torch.zeros(5 + 3 * A, dtype=torch.float32, device=dev)   # sums of the loss vector
            counts_aug = confmat_counts(A, self.n_categories, dev)            # labels of the TRAINING forwards (:510-525)
            nb = 0
            for buf in self.epoch_steps(train_loader):
                acc += buf                                                   # :469-475 without .item()
                nb += 1
                eng = self.model._engine
                N.confmat_accumulate(N.classify(eng.ws_view("c", self.n_categories)), self.n_categories, counts_aug)
            red = torch.cat([acc, torch.tensor([float(nb)], device=dev)])
            both = torch.stack([D.allreduce_sum_(red.clone()), red]).cpu().numpy()   # :480-483 folded into one
            red, loc = both[0], both[1]
            nsteps = red[-1]
            Bs = max(nb, 1)                                                  # len(train_loader) of this rank
            hist["losses"].append(red[N.LOSS_TOTAL] / nsteps)                # :485 (all-reduced sum / all-reduced count)
            hist["loss_joints"].append(loc[N.LOSS_JOINT] / Bs)               # :486-488: rank-local sums / len(loader)
            hist["c_ents"].append(loc[N.LOSS_CENT] / Bs)
            hist["c_l2_dists"].append(loc[N.LOSS_CL2] / Bs)
            hist["c_dists"].append(red[N.LOSS_CDIST] / nsteps)               # :489
            for a in range(A):
                hist["loss_recs"][a].append(red[N.LOSS_REC0 + a] / Dm / nsteps)   # :475, :491
            hist["consensus_aug"].append(float(np.mean(consensus_from_counts(counts_aug).cpu().numpy())) if nb else float("nan"))
            # consensus between the arms on the training set (cpl_mixvae.py:563-657), on the device
            cons = self.consensus(train_loader, whole_set=whole_train)
            hist["consensus_train"].append(cons)
            # validation loss (cpl_mixvae.py:665-775): eval mode, no Gumbel noise, hard sample
            if test_loader is not None:
                val_tot, val, val_cons = self.validate(test_loader, full=True)
            else:
                val_tot = val = val_cons = float("nan")
            hist["validation_loss"].append(val_tot)                # :764
            hist["validation_rec_loss"].append(val)                # :763
            hist["consensus_val"].append(val_cons)                 # :762
            dt = time.time() - t0
            hist["epoch_times"].append(dt)
            if rank in (None, 0, dev) or not D.is_dist():
                print(f"epoch {e} | loss: {hist['losses'][-1]:.2f} | rec: {hist['loss_recs'][0][-1]:.2f} | "
                      f"distance: {hist['c_dists'][-1]:.2f} | l2 distance: {hist['c_l2_dists'][-1]:.2f} | "
                      f"aug-cns: {hist['consensus_aug'][-1]:.2f} | train-cns: {cons:.2f} | val: {val:.2f} | "
                      f"time: {dt:.2f}", flush=True)
            if run:
                run.log({"train/total-loss": hist["losses"][-1], "train/joint-loss": hist["loss_joints"][-1],
                         "train/negative-joint-entropy": hist["c_ents"][-1],
                         "train/simplex-distance": hist["c_dists"][-1], "train/l2-distance": hist["c_l2_dists"][-1],
                         "train/time": dt, "train/consensus_aug": hist["consensus_aug"][-1],
                         **{f"train/rec-loss{a}": hist["loss_recs"][a][-1] for a in range(A)}})
                run.log({"train/consensus": cons})
                run.log({"val/total-loss": val_tot, "val/rec-loss": val, "val/consensus": val_cons})
            if self.save and self.folder and (e > 0) and (e % 10 == 0):    # :777-788
                os.makedirs(os.path.join(self.folder, "model"), exist_ok=True)
                self.save_checkpoint(os.path.join(self.folder, "model", f"cpl_mixVAE_model_epoch_{e}.pth"))
            if cons >= good_enuf_consensus or e == E - 1:                   # :851-927 (a NaN consensus never stops)
                if self.folder:
                    os.makedirs(os.path.join(self.folder, "model"), exist_ok=True)
                    self.save_checkpoint(os.path.join(
                        self.folder, "model", f"cns_cpl_mixVAE_model_before_pruning_A{A}_{self.current_time}.pth"))
                hist["stopped_at"] = e
                break
        if self.save and self.folder and n_epoch > 0:                       # :958-972
            os.makedirs(os.path.join(self.folder, "model"), exist_ok=True)
            self.save_checkpoint(os.path.join(self.folder, "model",
                                              f"cpl_mixVAE_model_before_pruning_A{A}_{self.current_time}.pth"))
        # Pruning phase (:996-1444): upstream forces ``stop_prune = True`` at :1007 whatever ``n_epoch_p`` is, so its
        # ``while not stop_prune`` body never runs; what remains of the phase are these two lines of output.
        if rank in (None, 0, dev) or not D.is_dist():
            print("warning: stopping pruning")                              # :1008
            print("Training is done!")                                      # :1446
        hist["bf16_storage"] = bool(self.used_bf16_storage)    # (not in the reference: which copy of x the run's losses were taken against)
        return hist

    def prune(self, train_loader, test_loader, n_epoch_p, min_con=0.5, max_prun_it=0, c_p=0, c_onehot=0, rank=None,
              run=None):
        """The pruning phase of cpl_mixvae.py:996-1444 with its loop live (upstream forces ``stop_prune`` at :1007 and :1135,
        which is why ``train(n_epoch_p > 0)`` does nothing; this method is the opt-in).  Repeats: assess the agreement of
        the arms per category on the training set under the mask of the kept categories (``category_agreement``), prune the
        kept category with the smallest agreement while that is at most ``min_con`` and fewer than ``max_prun_it`` rounds
        have run (``prune_decision``; rounds count from ``self.n_pr``), retrain ``n_epoch_p`` epochs with that category
        switched off (``epoch_steps`` under ``mask=``: the fused step with ``mmvae_hyper.cat_mask`` and ``prune_apply`` behind
        it), write ``model/cpl_mixVAE_model_after_pruning_{round}_{time}.pth`` when ``self.folder`` is set.  Starts from
        the categories whose ``fcc`` bias is non-zero, so a checkpoint of a pruned model resumes.

        Effective weights are torch's ``weight_orig * mask`` after every step.  Deviation: with ``FusedAdam`` the Adam moments
        of pruned entries are held at 0 where ``torch.nn.utils.prune`` leaves decaying remnants in the optimizer state;
        they never reach an effective weight.  No plots.  Returns the history: ``pruned`` (every pruned category in the
        order of the reference's ``ind``: those of the starting model first), ``kept``, ``agreement`` (one float64 [C] array
        per assessment), ``rounds`` and the per-epoch lists of ``train`` (all retraining epochs in sequence).  A model built with
        ``mode="ZINB"`` is refused: the ZINB step takes no category mask."""
        if self._is_zinb():
            raise NotImplementedError("cpl_mixVAE.prune on a model built with loss_mode='ZINB': the ZINB train step takes no "
                                      "category mask")
        if D.is_dist():
            raise NotImplementedError("cpl_mixVAE.prune under data parallelism: the category mask is not plumbed through "
                                      "dist.dp_train_step yet (issue 'Add the pruning phase: cpl_mixVAE.prune on a masked "
                                      "fused train step', out of scope there)")
        A, Dm, dev = self.n_arm, self.input_dim, self.device
        hist = {"pruned": [], "kept": [], "agreement": [], "rounds": 0, "losses": [], "loss_joints": [],
                "loss_recs": [[] for _ in range(A)], "c_ents": [], "c_l2_dists": [], "c_dists": [], "validation_loss": [],
                "validation_rec_loss": [], "consensus_val": [], "epoch_times": []}
        if n_epoch_p <= 0:
            return hist
        if A == 1:
            raise ZeroDivisionError("division by zero")   # nn_model.py:592-594
        kept, pruned = prune_start(self.model.fcc[0].bias.detach().cpu().numpy())       # :998-1000
        hist["pruned"], hist["kept"] = [int(k) for k in pruned], [int(k) for k in kept]
        pr = int(getattr(self, "n_pr", 0) or 0)                                          # :1005
        if not getattr(self, "current_time", None):
            self.current_time = time.strftime("%Y-%m-%d-%H-%M-%S")
        fused = isinstance(self.optimizer, FusedAdam) and self.optimizer.model is self.model
        # the row convention of train()'s consensus: the whole set in its base order unless the test loader has batches
        whole_train = test_loader is not None and not ((getattr(test_loader, "batch_size", None) or 0) > 1)
        while True:
            agreement = self.category_agreement(train_loader, mask=kept, whole_set=whole_train)    # :1010-1107
            hist["agreement"].append(agreement)
            k = prune_decision(agreement, kept, min_con, pr, max_prun_it)                           # :1108-1132
            if k is None:
                print("No more pruning!")
                break
            kept = kept[kept != k]
            hist["pruned"].append(k)
            hist["kept"] = [int(i) for i in kept]
            print("Continue training with pruning ...")
            print(f"Pruned categories: {np.asarray(hist['pruned'])}")
            # prune.custom_from_mask (:1153-1161): the effective weights are masked from here on
            self.model.prune_apply(kept, self.optimizer if fused else None)
            self._prune_mask = kept
            try:
                for _ in range(n_epoch_p):                                                          # :1163-1394
                    t0 = time.time()
                    self.model.train()
                    acc = torch.zeros(5 + 3 * A, dtype=torch.float32, device=dev)
                    nb = 0
                    for buf in self.epoch_steps(train_loader):
                        acc += buf
                        nb += 1
                    s = acc.cpu().numpy()                                     # the per-epoch means of train()
                    n = np.float32(max(nb, 1))
                    hist["losses"].append(s[N.LOSS_TOTAL] / n)
                    hist["loss_joints"].append(s[N.LOSS_JOINT] / n)
                    hist["c_ents"].append(s[N.LOSS_CENT] / n)
                    hist["c_l2_dists"].append(s[N.LOSS_CL2] / n)
                    hist["c_dists"].append(s[N.LOSS_CDIST] / n)
                    for a in range(A):
                        hist["loss_recs"][a].append(s[N.LOSS_REC0 + a] / Dm / n)
                    if test_loader is not None:
                        val_tot, val, val_cons = self.validate(test_loader, full=True, mask=kept)
                    else:
                        val_tot = val = val_cons = float("nan")
                    hist["validation_loss"].append(val_tot)
                    hist["validation_rec_loss"].append(val)
                    hist["consensus_val"].append(val_cons)
                    hist["epoch_times"].append(time.time() - t0)
                    print(f"====> Pruning round {pr + 1} | loss: {hist['losses'][-1]:.2f} | rec: "
                          f"{hist['loss_recs'][0][-1]:.2f} | val: {val:.2f}", flush=True)
                    if run:
                        run.log({"prune/total-loss": hist["losses"][-1], "prune/val-rec-loss": val, "prune/round": pr + 1})
            finally:
                self._prune_mask = None
            # prune.remove (:1396-1401): the masked values become the parameters themselves
            self.model.prune_apply(kept, self.optimizer if fused else None)
            if self.folder:                                                                         # :1403-1417
                os.makedirs(os.path.join(self.folder, "model"), exist_ok=True)
                self.save_checkpoint(os.path.join(
                    self.folder, "model", f"cpl_mixVAE_model_after_pruning_{pr + 1}_{self.current_time}.pth"))
            pr += 1
            hist["rounds"] += 1
        self.n_pr = pr
        return hist

    @torch.no_grad()
    def consensus(self, loader, whole_set: Optional[bool] = None, chunk: Optional[int] = None, mask=None) -> float:
        """Mean over arm pairs of ``confmat_mean(confmat_normalize(compute_confmat(labels_a, labels_b, C)))`` with
        ``labels = classify(c)`` of the eval-mode forward (cpl_mixvae.py:563-657).  ``whole_set``: classify every row
        of ``loader.dataset.tensors`` in its base order (what the reference does when the test loader's batch size is
        one, :617) instead of walking the loader (:567; a shuffled drop_last loader would skip its tail rows and spend a
        permutation); None decides from the loader's own batch size, as the validation block does.  Eval mode uses the
        running statistics, so cells are independent and the whole set is processed in chunks of ``chunk`` rows
        (default: the loader's batch size) with identical labels.  Labels, counts and the normalisation stay on the
        device: one host read of A(A-1)/2 doubles per epoch.  Under data parallelism every rank counts its own shard and
        the integer counts are summed (the reference, never run distributed, would report rank-local values).
        ``mask``: the kept categories of a pruned model, as ``forward(mask=)`` takes them."""
        from ._utils import consensus_from_counts
        counts, seen = self._label_counts(loader, whole_set, chunk, mask)
        if seen == 0:
            return float("nan")
        return float(np.mean(consensus_from_counts(counts).cpu().numpy()))   # np.mean(np.array(consensus)), :654

    @torch.no_grad()
    def _label_counts(self, loader, whole_set=None, chunk=None, mask=None):
        """Between-arm confusion counts (int64 [pairs, C, C], on the device) of the eval-mode labels over ``loader``, and the
        number of cells seen: the counting half of ``consensus`` and ``category_agreement``."""
        from ._utils import confmat_counts
        was_training = self.model.training
        self.model.eval()
        counts = confmat_counts(self.n_arm, self.n_categories, self.device)
        seen = 0
        for x in self._eval_batches(loader, whole_set, chunk):
            x = x.to(self.device)
            if x.shape[0] < 1:
                continue
            self.model.eval_labels(x.expand(self.n_arm, -1, -1), self.temp, counts, mask=mask)
            seen += x.shape[0]
        if D.is_dist():
            D.allreduce_sum_(counts)
        self.model.train(was_training)
        return counts, seen

    @torch.no_grad()
    def category_agreement(self, loader, mask=None, whole_set: Optional[bool] = None, chunk: Optional[int] = None) -> np.ndarray:
        """The pruning phase's assessment (cpl_mixvae.py:1010-1107): per category, the mean over arm pairs of the diagonal of
        the pair's confusion matrix of eval-mode labels under ``mask``, each column divided by max(its row sum, its column
        sum) and 0 where that is 0 -- ``confmat_normalize``'s arithmetic, so the counts and the normalisation are
        ``consensus``'s (on the device, ``_native.consensus(counts, want_norm=True)``); float64 [C], the mean over pairs
        taken by numpy on the host.  A category no arm predicts has agreement 0."""
        counts, _ = self._label_counts(loader, whole_set, chunk, mask)
        _, norm = N.consensus(counts, want_norm=True)
        diag = torch.diagonal(norm, dim1=1, dim2=2).contiguous().cpu().numpy()    # [pairs, C]: np.diag of every pair, :1080
        return np.mean(diag, axis=0)                                                # :1107

    @staticmethod
    def _eval_batches(loader, whole_set: Optional[bool] = None, chunk: Optional[int] = None):
        """The reference walks a loader batch by batch when its ``batch_size > 1`` and otherwise takes the whole set
        as ONE batch from ``loader.dataset.tensors`` (cpl_mixvae.py:567-640, :670-760; the default test loader has
        ``batch_size=1``).  Yields x tensors accordingly.  ``chunk``: rows per yielded piece of the whole set (only
        for per-cell work such as the evaluation labels; None = one piece, as the loss needs)."""
        has_set = hasattr(loader, "dataset") and hasattr(loader.dataset, "tensors")
        if whole_set is None:
            whole_set = getattr(loader, "batch_size", None) == 1 and has_set
        if whole_set and has_set:
            if chunk is None and getattr(loader, "batch_size", None) == 1:
                yield loader.dataset.tensors[0]
                return
            step = int(chunk or getattr(loader, "batch_size", None) or 1)
            if hasattr(loader, "row_chunks"):          # device-resident loader: gather piece by piece
                yield from loader.row_chunks(step)
                return
            x = loader.dataset.tensors[0]
            for i in range(0, x.shape[0], step):
                yield x[i:i + step]
            return
        for batch in loader:
            yield batch[0] if isinstance(batch, (tuple, list)) else batch

    @torch.no_grad()
    def validate(self, loader, full: bool = False, mask=None):
        """The validation block of cpl_mixvae.py:665-775 in eval mode: ``validation_rec_loss = sum over batches and arms
        of loss_rec[a] / D, divided by len(loader) and n_arm`` (:742-763), ``validation_loss = sum of the total loss /
        len(loader)`` (:741, :764) and the between-arm consensus of the labels (:752-762, on the device).  Returns the
        rec loss, or the triple ``(validation_loss, validation_rec_loss, consensus_val)`` with ``full=True``.  With
        the reference's default test loader (batch_size 1) the whole set is one batch and ``len(loader)`` its row
        count, as in the reference.  ``mask``: the kept categories of a pruned model, as ``forward(mask=)`` takes them (the
        pruning phase validates under its mask, :1317-1323, :1362-1369).  On a model built with ``mode="ZINB"`` the
        per-batch loss vector is the ZINB objective's (``mixVAE_model.zinb_objective``: ``loss_rec[a]`` the ZINB loss) on the
        same eval forward; the formulas, the skipped one-cell batch and the consensus are the same."""
        from ._utils import confmat_counts, consensus_from_counts
        was_training = self.model.training
        self.model.eval()
        A = self.n_arm
        zinb = self._is_zinb()
        counts = confmat_counts(A, self.n_categories, self.device)
        tot = torch.zeros((), dtype=torch.float64, device=self.device)
        rec = torch.zeros((), dtype=torch.float64, device=self.device)
        seen = 0
        for x in self._eval_batches(loader):
            x = x.to(self.device)
            if x.shape[0] < 2:     # a one-cell batch has no batch variance: the reference's loss is NaN there (nn_model.py:75)
                continue
            xs = x.expand(A, -1, -1)
            if zinb:
                if A == 1:
                    raise ZeroDivisionError("division by zero")              # nn_model.py:592-594, as loss() raises it
                out = self.model._forward(xs, self.temp, True, mask, False)  # what _zinb_objective_vec runs, c kept
                vec = self.model._zinb_objective_here()
                self.model._ctx = None
                tot += vec[N.LOSS_TOTAL].double()
                rec += vec[N.LOSS_REC0: N.LOSS_REC0 + A].double().sum() / self.input_dim
                labels = torch.stack([N.classify(c) for c in out[4]])
            else:
                out = self.model(xs, self.temp, 0.0, eval=True, mask=mask)
                lt = self.model.loss(out[0], [], [], xs, out[7], out[8], out[4], out[6], 0.0)
                tot += lt[0].double()                                             # :741 val_loss += loss.data.item()
                rec += lt[1].double().sum() / self.input_dim                      # :742-743 sum_a loss_rec[a] / D
                labels = torch.stack([N.classify(c) for c in out[4]])            # :744 / :752 classify(cs[a])
            N.confmat_accumulate(labels, self.n_categories, counts)
            seen += 1
        self.model.train(was_training)
        nb = max(len(loader), 1) if hasattr(loader, "__len__") else max(seen, 1)
        val_loss, val_rec = float(tot) / nb, float(rec) / nb / A
        if not full:
            return val_rec
        cons = float(np.mean(consensus_from_counts(counts).cpu().numpy())) if seen and A > 1 else float("nan")
        return val_loss, val_rec, cons

    @torch.no_grad()
    def eval_model(self, dl, c_p=0, c_onehot=0):
        """``cpl_mixVAE.eval_model`` (cpl_mixvae.py:1450-1619): eval-mode forward + loss over every batch ``(x, index)`` of
        ``dl`` and the reference's dictionary -- same keys, shapes and dtypes (float64 numpy arrays, as ``np.zeros``
        gives them): ``state_mu`` / ``state_var`` (s_mean, s_logvar) [A,N,S], ``state_cat`` (argmax c + 1) and
        ``prob_cat`` (max c) [A,N], ``total_loss_rec`` / ``total_likelihood`` [A] (means over batches),
        ``total_dist_z`` / ``total_dist_qz`` (mean simplex / l2 distance), ``mean_test_rec`` (zeros), ``predicted_label``
        [A,N], ``data_indx`` [N], ``z_prob`` (c) and ``z_sample`` (c_smp) [A,N,C], ``x_low`` [A,N,L], ``recon_c``
        (x_rec) [A,N,D], ``prune_indx`` (categories whose fcc bias is zero) and ``cnss`` (between-arm consensus of the
        labels).  Forward, loss, labels, confusion counts and consensus run on the device; the per-batch outputs are
        collected in device buffers and copied to the host once.  On a model built with ``mode="ZINB"`` the loss is the ZINB
        objective on the workspace of the same eval forward (one forward per batch, ``x_p`` / ``x_r`` never written):
        ``total_loss_rec`` is the per-arm mean over batches of the ZINB loss, ``total_likelihood`` the reference's MSE-based
        ``ll`` that the objective carries; every other key is what the MSE path gives."""
        if self.ref_prior:
            raise NotImplementedError("ref_prior is rejected by the reference loss (nn_model.py:578)")
        A, Cc, Dm, L, S = self.n_arm, self.n_categories, self.input_dim, self.lowD_dim, self.state_dim
        zinb = self._is_zinb()
        if zinb and A == 1:
            raise ZeroDivisionError("division by zero")                   # nn_model.py:592-594, as loss() raises it
        n_rows = len(dl.dataset)
        B = dl.batch_size
        if B is None:
            raise ValueError("error: expected non-None value")            # unwrap(dl.batch_size), cpl_mixvae.py:104-107
        dev = self.device
        was_training = self.model.training
        self.model.eval()
        bias = self.model.fcc[0].bias.detach().cpu().numpy()
        pruning_mask = np.where(bias != 0.0)[0]
        prune_indx = np.where(bias == 0.0)[0]
        f32 = dict(dtype=torch.float32, device=dev)
        x_recs, s_means = torch.zeros(A, n_rows, Dm, **f32), torch.zeros(A, n_rows, S, **f32)
        s_logvars, cs = torch.zeros(A, n_rows, S, **f32), torch.zeros(A, n_rows, Cc, **f32)
        c_smps, x_lows = torch.zeros(A, n_rows, Cc, **f32), torch.zeros(A, n_rows, L, **f32)
        data_indx = torch.zeros(n_rows, dtype=torch.float64, device=dev)
        loss_vecs = []
        from ._utils import confmat_counts, consensus_from_counts
        for i, (x, data_idx) in enumerate(dl):
            n_fst, n_lst = i * B, min((i + 1) * B, n_rows)
            x = x.to(dev)
            xs = x.expand(A, -1, -1)                                      # xs = [x for _ in range(A)], :1519
            if zinb:
                # no x_p / x_r are written: the ZINB objective forms the heads tile by tile from the workspace's d10
                out = self.model._forward(xs, self.temp, True, pruning_mask, False)
                loss_vecs.append(self.model._zinb_objective_here())
                self.model._ctx = None
            else:
                out = self.model(xs, self.temp, prior_c=0.0, eval=True, mask=pruning_mask)
                self.model.loss(out[0], out[1], out[2], xs, out[7], out[8], out[4], out[6], 0.0)
                loss_vecs.append(self.model._engine.loss_buf.clone())     # the 9-tuple's scalars, still on the device
            for dst, k in ((s_means, 7), (s_logvars, 8), (cs, 4), (c_smps, 6), (x_lows, 3), (x_recs, 0)):
                dst[:, n_fst:n_lst] = torch.stack(list(out[k]))
            data_indx[n_fst:n_lst] = torch.as_tensor(data_idx).to(dev).to(torch.int64).to(torch.float64)
        labels = N.classify(cs)                                            # argmax c, first maximum (np.argmax), [A,N]
        prob = cs.max(dim=-1).values
        counts = N.confmat_accumulate(labels, Cc, confmat_counts(A, Cc, dev))
        cnss = float(np.mean(consensus_from_counts(counts).cpu().numpy())) if A > 1 and n_rows else float("nan")
        lv = torch.stack(loss_vecs).double().cpu().numpy() if loss_vecs else np.zeros((0, 5 + 3 * A))
        self.model.train(was_training)
        to64 = lambda t: t.double().cpu().numpy()
        lab1 = to64(labels) + 1.0
        return {
            "state_mu": to64(s_means),
            "state_var": to64(s_logvars),
            "state_cat": lab1.copy(),
            "prob_cat": to64(prob),
            "total_loss_rec": lv[:, N.LOSS_REC0:N.LOSS_REC0 + A].mean(axis=0),
            "total_likelihood": lv[:, N.LOSS_REC0 + 2 * A:N.LOSS_REC0 + 3 * A].mean(axis=0),
            "total_dist_z": np.mean(lv[:, N.LOSS_CDIST]),
            "total_dist_qz": np.mean(lv[:, N.LOSS_CL2]),
            "mean_test_rec": np.zeros(A),
            "predicted_label": lab1,
            "data_indx": data_indx.cpu().numpy(),
            "z_prob": to64(cs),
            "z_sample": to64(c_smps),
            "x_low": to64(x_lows),
            "recon_c": to64(x_recs),
            "prune_indx": prune_indx,
            "cnss": cnss,
        }

    def _encode_all(self, dl, counts=None):
        """The device encode of every batch ``(x, index)`` of ``dl`` (``fill_latents``, under the category mask of
        ``eval_model``) in eval mode, the training mode restored afterwards whether or not the pass raises -> (the [A, N, .]
        float32 device buffers ``x_low``, ``c``, ``c_smp``, ``s_mean``, ``s_logvar`` and the int32 ``labels`` [A, N]; the
        batches' indices, float64 [N] on the device).  ``counts``: the between-arm confusion counts to add to, or None."""
        from ._utils import mk_masks
        from .model import fill_latents
        A, Cc, L, S = self.n_arm, self.n_categories, self.lowD_dim, self.state_dim
        n_rows = len(dl.dataset)
        pruning_mask = mk_masks(self.model.fcc[0].bias)[0]
        f32 = dict(dtype=torch.float32, device=self.device)
        out = {"x_low": torch.zeros(A, n_rows, L, **f32), "c": torch.zeros(A, n_rows, Cc, **f32),
               "c_smp": torch.zeros(A, n_rows, Cc, **f32), "s_mean": torch.zeros(A, n_rows, S, **f32),
               "s_logvar": torch.zeros(A, n_rows, S, **f32),
               "labels": torch.zeros(A, n_rows, dtype=torch.int32, device=self.device)}
        was_training = self.model.training
        self.model.eval()
        try:
            return out, fill_latents(dl, [(self.model, pruning_mask, out, counts)], self.temp)
        finally:
            self.model.train(was_training)

    @torch.no_grad()
    def encode_dataset(self, dl, c_p=0, c_onehot=0):
        """``eval_model`` without everything that needs the decoder: the latents of every batch ``(x, index)`` of ``dl`` from
        the encoder and the latent block alone (``mixVAE_model.encode``: no decoder chain, no fc11, no x_rec, no loss),
        each batch written straight into its rows of [A, N, .] device buffers, one copy to the host at the end.  Returns
        ``eval_model``'s keys ``state_mu``, ``state_var``, ``state_cat``, ``prob_cat``, ``predicted_label``, ``data_indx``,
        ``z_prob``, ``z_sample``, ``x_low``, ``prune_indx`` and ``cnss`` with its shapes, dtypes and values; ``recon_c`` and
        the loss means are not in it."""
        if self.ref_prior:
            raise NotImplementedError("ref_prior is rejected by the reference loss (nn_model.py:578)")
        if dl.batch_size is None:
            raise ValueError("error: expected non-None value")            # unwrap(dl.batch_size), cpl_mixvae.py:104-107
        from ._utils import confmat_counts, consensus_from_counts, mk_masks
        A = self.n_arm
        counts = confmat_counts(A, self.n_categories, self.device)
        out, data_indx = self._encode_all(dl, counts if A > 1 else None)
        prune_indx = mk_masks(self.model.fcc[0].bias)[1]
        prob = out["c"].max(dim=-1).values
        cnss = float(np.mean(consensus_from_counts(counts).cpu().numpy())) if A > 1 and len(dl.dataset) else float("nan")
        to64 = lambda t: t.double().cpu().numpy()
        lab1 = to64(out["labels"]) + 1.0
        return {
            "state_mu": to64(out["s_mean"]),
            "state_var": to64(out["s_logvar"]),
            "state_cat": lab1.copy(),
            "prob_cat": to64(prob),
            "predicted_label": lab1,
            "data_indx": data_indx.cpu().numpy(),
            "z_prob": to64(out["c"]),
            "z_sample": to64(out["c_smp"]),
            "x_low": to64(out["x_low"]),
            "prune_indx": prune_indx,
            "cnss": cnss,
        }

    @torch.no_grad()
    def score_zinb(self, dl):
        """The ZINB negative log-likelihood of the cells of ``dl`` under a model built with ``mode="ZINB"``:
        ``mixVAE_model.zinb_nll`` (eval forward, ``temp = self.temp``, the category mask of ``eval_model``) on every batch
        ``(x, index)`` in order.  Returns numpy arrays: ``cell`` float64 [A, N], a cell's term summed over the genes, batches
        concatenated in the loader's order; ``gene`` float64 [A, D], the batches' per-gene sums added batch by batch in
        fp64; ``mean`` float64 [A], the sum of ``cell`` over N D (``zinb_loss`` of the whole set); ``data_indx`` [N]."""
        if D.is_dist():
            raise NotImplementedError("score_zinb is not data-parallel: run it on one rank, outside the process group")
        self.model._need_zinb("score_zinb()")
        A, Dm = self.n_arm, self.input_dim
        n_rows = len(dl.dataset)
        B = dl.batch_size
        if B is None:
            raise ValueError("error: expected non-None value")            # unwrap(dl.batch_size), cpl_mixvae.py:104-107
        dev = self.device
        was_training = self.model.training
        self.model.eval()
        pruning_mask = np.where(self.model.fcc[0].bias.detach().cpu().numpy() != 0.0)[0]
        cell = torch.zeros(A, n_rows, dtype=torch.float64, device=dev)
        gene = torch.zeros(A, Dm, dtype=torch.float64, device=dev)
        inds = torch.zeros(n_rows, dtype=torch.float64, device=dev)
        try:
            for i, (x, i_x) in enumerate(dl):
                n_fst, n_lst = i * B, min((i + 1) * B, n_rows)
                out = self.model.zinb_nll(x.to(dev).expand(A, -1, -1), self.temp, mask=pruning_mask)
                cell[:, n_fst:n_lst] = out["cell"]
                gene += out["gene"]
                inds[n_fst:n_lst] = torch.as_tensor(i_x).to(dev).to(torch.float64)
        finally:
            self.model.train(was_training)
        mean = cell.sum(dim=1) / (float(n_rows) * float(Dm)) if n_rows else torch.full((A,), float("nan"), dtype=torch.float64)
        return {"cell": cell.cpu().numpy(), "gene": gene.cpu().numpy(), "mean": mean.cpu().numpy(),
                "data_indx": inds.cpu().numpy()}

    @torch.no_grad()
    def fit_zinb_heads(self, train_loader, n_epoch, lr=1e-3, heads=("rec", "p", "r"), test_loader=None, betas=(0.9, 0.999),
                       eps=1e-8, weight_decay=0.0, state=None):
        """Fit the decoder's ZINB heads of a model built with ``mode="ZINB"`` to the ZINB likelihood of the cells of
        ``train_loader``, the trunk frozen: ``heads`` selects among "rec" (``fc11``), "p" (``fc11_p``) and "r" (``fc11_r``).
        The model is in ``eval()`` throughout (no dropout, BatchNorm on its running statistics, ``temp = self.temp``, the
        category mask of ``eval_model``); nothing but the selected heads is written.  Per batch ``(x, index)``:
        ``mixVAE_model.zinb_head_grads`` (the gradient of the batch's mean term), then one mmvae_adam_step per arm on a flat
        float32 buffer that holds the arm's selected heads (Adam with L2 ``weight_decay``, as ``torch.optim.Adam``).  The
        heads' ``nn.Linear`` parameters hold the result afterwards -- and only then: during the fit the buffer is ahead of them
        (they receive it before every ``score_zinb`` of a ``test_loader`` and on exit), so whatever reads ``model.fc11*``
        between two batches, the eval forward's own ``x_rec`` included, sees the heads as they were at the last of those
        points.  Returns ``{"train_loss": float64 [n_epoch, A], the mean
        term over the epoch's cells (each batch under the heads it met); "val_loss": float64 [n_epoch, A] from
        ``score_zinb(test_loader)["mean"]`` after each epoch, or None without a ``test_loader``; "state": Adam's step count
        and moment buffers}``.  ``state=`` takes such a state back and resumes: two epochs and two more equal four in one
        call bit for bit, given the same noise.  The model's mode is restored on exit, also after an exception.
        RuntimeError for a model built with ``mode="MSE"``, NotImplementedError inside a process group, ValueError for an
        unknown head, a negative ``n_epoch``, ``lr`` or ``weight_decay``, or ``betas`` outside [0, 1)."""
        return self._fit_zinb("fit_zinb_heads", False, train_loader, n_epoch, lr, heads, test_loader, betas, eps, weight_decay, state)

    @torch.no_grad()
    def fit_zinb_decoder(self, train_loader, n_epoch, lr=1e-3, heads=("rec", "p", "r"), test_loader=None, betas=(0.9, 0.999),
                         eps=1e-8, weight_decay=0.0, state=None):
        """Fit the whole decoder of a model built with ``mode="ZINB"`` -- the trunk ``fc6`` .. ``fc10`` and the selected heads
        -- to the ZINB likelihood of the cells of ``train_loader``, the encoder frozen.  ``fit_zinb_heads``' contract, extended
        by the trunk: the model is in ``eval()`` throughout (``temp = self.temp``, the category mask of ``eval_model``); per
        batch ``mixVAE_model.zinb_decoder_grads`` (mmvae_zinb_head_grads, mmvae_zinb_d10_grad and mmvae_decoder_trunk_grads
        per arm), then mmvae_adam_step on the trunk and on the selected heads.  The trunk's step runs in place on the arm's
        ``fc6`` .. ``fc10`` range of the model's flat parameter buffer, which the eval forward reads: the forward of the next
        batch sees the trunk of this step.  The padding between two tensors of that range is zero, has a zero gradient and so
        stays exactly zero; the column of ``fc6`` of a category that ``prune`` switched off meets a zero input and stays exactly
        zero too.  The heads keep ``fit_zinb_heads``' buffer and its write-back points.  The encoder, the latent block, the
        BatchNorm statistics and the unselected heads are not written.  Return value, ``state=`` (its moments are [A, trunk
        range + heads]: a state of ``fit_zinb_heads`` is refused), restored mode and refusals as ``fit_zinb_heads``."""
        return self._fit_zinb("fit_zinb_decoder", True, train_loader, n_epoch, lr, heads, test_loader, betas, eps, weight_decay, state)

    def _fit_zinb(self, what, trunk, train_loader, n_epoch, lr, heads, test_loader, betas, eps, weight_decay, state):
        """``fit_zinb_heads`` (``trunk=False``) and ``fit_zinb_decoder`` (``trunk=True``)."""
        if D.is_dist():
            raise NotImplementedError(f"{what} is not data-parallel: run it on one rank, outside the process group")
        m = self.model
        m._need_zinb(f"{what}()")
        N.zinb_head_mask(heads)
        if int(n_epoch) < 0 or not (0.0 <= lr < float("inf")) or not (0.0 <= weight_decay < float("inf")) or not eps >= 0.0:
            raise ValueError(f"{what}: n_epoch = {n_epoch}, lr = {lr}, eps = {eps}, weight_decay = {weight_decay} must not "
                             "be negative (or infinite)")
        if len(betas) != 2 or not all(0.0 <= b < 1.0 for b in betas):
            raise ValueError(f"{what}: betas = {betas} outside [0, 1)")
        sel = [h for h in N.ZINB_HEADS if h in ((heads,) if isinstance(heads, str) else tuple(heads))]
        A, Dm, H = self.n_arm, self.input_dim, m.fc_dim
        dev = self.device
        flat = m.flat_parameters()                # the parameters sit where the engine reads them before views are taken
        layer = {"rec": m.fc11, "p": m.fc11_p, "r": m.fc11_r}
        per_head = Dm * H + Dm
        n = len(sel) * per_head
        buf = torch.empty(A, n, dtype=torch.float32, device=dev)
        grad = torch.zeros_like(buf)
        # the trunk: tensors 16 .. 25 of the parameter layout, one range of an arm's segment of the flat buffer
        lay = m._layout
        o_lo, o_hi, per_arm = int(lay.offset[16]), int(lay.offset[26]), int(lay.per_arm)
        T = o_hi - o_lo if trunk else 0
        tgrad = torch.zeros(A, T, dtype=torch.float32, device=dev)
        tviews = [[tgrad[a, int(lay.offset[t]) - o_lo: int(lay.offset[t]) - o_lo + m._param_of(t, a).numel()].view(m._param_of(t, a).shape)
                   for t in range(16, 26)] for a in range(A)] if trunk else None

        def views(t, a):
            return {h: (t[a, j * per_head: j * per_head + Dm * H].view(Dm, H), t[a, j * per_head + Dm * H: (j + 1) * per_head])
                    for j, h in enumerate(sel)}

        if state is None:
            step = 0
            m1, m2 = (torch.zeros(A, T + n, dtype=torch.float32, device=dev) for _ in range(2))
        else:
            if tuple(state["heads"]) != tuple(sel) or tuple(state["exp_avg"].shape) != (A, T + n):
                raise ValueError(f"{what}: state is of heads {tuple(state['heads'])} and moments "
                                 f"{tuple(state['exp_avg'].shape)}; this fit has {tuple(sel)} and {(A, T + n)}")
            step = int(state["step"])
            m1, m2 = state["exp_avg"].to(dev).clone(), state["exp_avg_sq"].to(dev).clone()
        pv = [views(buf, a) for a in range(A)]
        gv = [views(grad, a) for a in range(A)]
        layers = []
        for a in range(A):
            for h in sel:
                pv[a][h][0].copy_(layer[h][a].weight.detach())
                pv[a][h][1].copy_(layer[h][a].bias.detach())
            layers.append([t for h in N.ZINB_HEADS
                           for t in (pv[a][h] if h in sel else (layer[h][a].weight.detach(), layer[h][a].bias.detach()))])

        def write_back():
            for a in range(A):
                for h in sel:
                    layer[h][a].weight.data.copy_(pv[a][h][0])
                    layer[h][a].bias.data.copy_(pv[a][h][1])

        train_loss = np.zeros((int(n_epoch), A))
        val_loss = np.zeros((int(n_epoch), A)) if test_loader is not None else None
        was_training = m.training
        m.eval()
        pruning_mask = np.where(m.fcc[0].bias.detach().cpu().numpy() != 0.0)[0]
        try:
            for epoch in range(int(n_epoch)):
                total = torch.zeros(A, dtype=torch.float64, device=dev)
                cells = 0
                for x, _ in train_loader:
                    B = int(x.shape[0])
                    xb = x.to(dev).expand(A, -1, -1)
                    if trunk:
                        res = m._zinb_decoder_grads(xb, self.temp, pruning_mask, sel, layers, gv, tviews, False)
                    else:
                        res = m._zinb_head_grads(xb, self.temp, pruning_mask, sel, layers, gv)
                    step += 1
                    for a in range(A):
                        if trunk:
                            N.adam_step(flat[a * per_arm + o_lo: a * per_arm + o_hi], tgrad[a], m1[a, :T], m2[a, :T], step, lr,
                                        betas[0], betas[1], eps, weight_decay, False)
                        N.adam_step(buf[a], grad[a], m1[a, T:], m2[a, T:], step, lr, betas[0], betas[1], eps, weight_decay, False)
                        total[a] += res[a]["loss"] * B
                    cells += B
                train_loss[epoch] = (total / max(cells, 1)).cpu().numpy()
                if test_loader is not None:
                    write_back()
                    val_loss[epoch] = self.score_zinb(test_loader)["mean"]
        finally:
            write_back()
            m.train(was_training)
        return {"train_loss": train_loss, "val_loss": val_loss,
                "state": {"step": step, "exp_avg": m1, "exp_avg_sq": m2, "heads": tuple(sel)}}

    @torch.no_grad()
    def fit_zinb(self, train_loader, n_epoch, lr=1e-3, test_loader=None, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, state=None):
        """Train the whole model -- encoder, latent block, decoder and the three heads -- of a model built with ``mode="ZINB"``
        under the ZINB objective: the reference's ``loss()`` with its reconstruction term replaced by ``zinb_loss``.  The model
        is in ``train()`` throughout (input and state dropout, batch-statistic BatchNorm, ``temp = self.temp``); per batch
        ``(x, index)`` one ``mixVAE_model.zinb_train_step`` on the gathered batch ``x.expand`` over the arms (Adam with L2
        ``weight_decay``, as ``torch.optim.Adam``).  The rows path and the augmenter are not used.  Returns ``{"train_loss":
        float64 [n_epoch, 5 + 3 A], the epoch's mean of every entry of the loss vector (MMVAE_LOSS_*: total, joint, .. , rec[a]
        the ZINB loss, kl[a], ll[a]) over its batches; "val_loss": float64 [n_epoch, 5 + 3 A], the same entries from
        ``zinb_objective`` (eval mode) over the batches of ``test_loader`` after each epoch, or None without one; "state":
        Adam's step count and both moment pairs}``.  ``state=`` takes such a state back and resumes: two epochs and two more
        equal four in one call bit for bit, given the same noise.  The model's mode is restored on exit, also after an
        exception.  Refusals, all before any device work or noise is consumed: RuntimeError for a model built with
        ``mode="MSE"``; NotImplementedError inside a process group ("not data-parallel"), for ``gemm_dtype="bf16"`` and for a
        model whose categories ``prune`` has switched off (its mask is not offered in training); ValueError for a negative
        ``n_epoch``, ``lr``, ``eps`` or ``weight_decay``, ``betas`` outside [0, 1), or a state of ``fit_zinb_heads`` /
        ``fit_zinb_decoder``."""
        what = "fit_zinb"
        if D.is_dist():
            raise NotImplementedError(f"{what} is not data-parallel: run it on one rank, outside the process group")
        m = self.model
        m._need_zinb(f"{what}()")
        if int(n_epoch) < 0 or not (0.0 <= lr < float("inf")) or not (0.0 <= weight_decay < float("inf")) or not eps >= 0.0:
            raise ValueError(f"{what}: n_epoch = {n_epoch}, lr = {lr}, eps = {eps}, weight_decay = {weight_decay} must not "
                             "be negative (or infinite)")
        if len(betas) != 2 or not all(0.0 <= b < 1.0 for b in betas):
            raise ValueError(f"{what}: betas = {betas} outside [0, 1)")
        if m.gemm_dtype == "bf16":
            raise NotImplementedError(f"{what}: gemm_dtype='bf16' is not offered under the ZINB objective (bf16 heads are not built)")
        if state is not None:
            m._check_zinb_step_state(what, state)
        if int(np.count_nonzero(m.fcc[0].bias.detach().cpu().numpy() != 0.0)) < self.n_categories:
            raise NotImplementedError(f"{what}: the model has pruned categories; a category mask is not offered in ZINB training")
        A, dev = self.n_arm, self.device
        if state is None:
            st = m.zinb_step_state()
        else:
            st = {k: (v.to(dev).clone() if isinstance(v, torch.Tensor) else v) for k, v in state.items()}
            st["exp_avg"], st["exp_avg_sq"] = st["exp_avg"].reshape(-1), st["exp_avg_sq"].reshape(-1)
        n_loss = 5 + 3 * A
        train_loss = np.zeros((int(n_epoch), n_loss))
        val_loss = np.zeros((int(n_epoch), n_loss)) if test_loader is not None else None
        was_training = m.training
        try:
            for epoch in range(int(n_epoch)):
                m.train()
                acc = torch.zeros(n_loss, dtype=torch.float64, device=dev)
                batches = 0
                for x, _ in train_loader:
                    buf = m.zinb_train_step(x.to(dev).expand(A, -1, -1), self.temp, state=st, do_adam=True, lr=lr, betas=betas,
                                            eps=eps, weight_decay=weight_decay)
                    acc += buf.to(torch.float64)
                    batches += 1
                train_loss[epoch] = (acc / max(batches, 1)).cpu().numpy()
                if test_loader is not None:
                    m.eval()
                    acc.zero_()
                    batches = 0
                    for x, _ in test_loader:
                        acc += m._zinb_objective_vec(x.to(dev).expand(A, -1, -1), self.temp, None).to(torch.float64)
                        batches += 1
                    val_loss[epoch] = (acc / max(batches, 1)).cpu().numpy()
        finally:
            m.train(was_training)
        return {"train_loss": train_loss, "val_loss": val_loss, "state": st}

    @torch.no_grad()
    def sample_counts(self, dl, seed, arm=None, log1p=False):
        """Synthetic counts for the cells of ``dl`` from a model built with ``mode="ZINB"``: per batch ``(x, index)`` an eval
        forward as ``score_zinb`` runs it (``temp = self.temp``, the category mask of ``eval_model``), then one ZINB draw per
        gene under each arm's heads (``mixVAE_model.zinb_sample_batch``; the heads are never written).  A draw is keyed by
        ``seed`` and the cell's position in the loader's order, so the result does not depend on the batch size beyond what the
        forward itself does.  ``arm=None`` draws for every arm.  Returns numpy arrays: ``counts`` float32 [A, n, D] (A = 1 for a
        chosen arm; ``log1p`` of the counts on request) and ``data_indx`` [n].  The training mode is restored afterwards;
        RuntimeError for a model built with ``mode="MSE"``."""
        if D.is_dist():
            raise NotImplementedError("sample_counts is not data-parallel: run it on one rank, outside the process group")
        self.model._need_zinb("sample_counts()")
        if arm is not None and not 0 <= int(arm) < self.n_arm:
            raise ValueError(f"arm = {arm} outside [0, {self.n_arm})")
        arms = list(range(self.n_arm)) if arm is None else [int(arm)]
        n_rows = len(dl.dataset)
        B = dl.batch_size
        if B is None:
            raise ValueError("error: expected non-None value")            # unwrap(dl.batch_size), cpl_mixvae.py:104-107
        dev = self.device
        was_training = self.model.training
        self.model.eval()
        pruning_mask = np.where(self.model.fcc[0].bias.detach().cpu().numpy() != 0.0)[0]
        counts = np.empty((len(arms), n_rows, self.input_dim), dtype=np.float32)
        inds = np.zeros(n_rows, dtype=np.float64)
        try:
            for i, (x, i_x) in enumerate(dl):
                n_fst, n_lst = i * B, min((i + 1) * B, n_rows)
                out = self.model.zinb_sample_batch(x.to(dev).expand(self.n_arm, -1, -1), seed, self.temp, mask=pruning_mask,
                                                   cell0=n_fst, log1p=log1p, arms=arms)
                counts[:, n_fst:n_lst] = out.cpu().numpy()
                inds[n_fst:n_lst] = torch.as_tensor(i_x).double().cpu().numpy()
        finally:
            self.model.train(was_training)
        return {"counts": counts, "data_indx": inds}

    @torch.no_grad()
    def state_gene_corr(self, dl, arm: int = 0, by_category: bool = True):
        """Which genes follow the state variable: the reference's ``corr_analysis`` (mmidas/utils/tree_based_analysis.py:7-59)
        of arm ``arm``'s ``s_mean`` with the expression of the cells of ``dl``, for every category of that arm at once ("S
        conditioning on Z = k"; ``by_category=False``: over all cells).  ``dl`` is encoded through the device encode path
        (``fill_latents``, as ``encode_dataset``); ``s_mean`` and the arm's labels stay on the device, and
        ``mmvae_state_corr`` reads the expression where it lies: a ``DeviceLoader``'s resident matrix through the batches'
        row indices, or, for a plain loader, the concatenation of its batches on the device.  Neither the matrix nor the
        latents are copied to the host.  Returns ``{"corr": float64 [G, S, D], "n": int64 [G, D], "categories": int64 [G]}``:
        the signed Pearson r over the category's cells that express the gene (0 where at most four do, NaN where the
        expression or the state is constant over them), their number, and the 0-based categories (all ``n_categories`` of
        them; a category with no cell gives a row of zeros); G = 1 and category -1 with ``by_category=False``.  The loader
        must serve every row once (no ``drop_last``)."""
        if D.is_dist():
            raise NotImplementedError("state_gene_corr is not data-parallel: run it on one rank, outside the process group")
        if self.ref_prior:
            raise NotImplementedError("ref_prior is rejected by the reference loss (nn_model.py:578)")
        if not 0 <= int(arm) < self.n_arm:
            raise ValueError(f"arm = {arm} outside [0, {self.n_arm})")
        from .utils.dataloader import DeviceLoader
        from .utils.tree_based_analysis import grouped_state_corr
        Cc = self.n_categories
        resident = isinstance(dl, DeviceLoader)
        if resident and (dl.world_size > 1 or (dl.drop_last and len(dl.dataset) % dl.batch_size)):
            raise ValueError("state_gene_corr needs a loader that serves every row once (no drop_last, no sharding)")
        if not resident:
            dl = _Replay(dl, self.device)                                 # one walk of the loader: the same batches twice
        out, inds = self._encode_all(dl)
        if resident:
            data, rows = dl.data, inds.to(torch.int64)                     # the batches' indices are rows of the matrix
        else:
            data, rows = dl.matrix(), None
        codes = out["labels"][int(arm)].to(torch.int64) if by_category else None
        r, cnt = grouped_state_corr(out["s_mean"][int(arm)], data, rows, codes, Cc if by_category else 1)
        cats = np.arange(Cc, dtype=np.int64) if by_category else np.array([-1], dtype=np.int64)
        return {"corr": r.cpu().numpy(), "n": cnt.cpu().numpy(), "categories": cats}

    @torch.no_grad()
    def category_markers(self, dl, arm: int = 0, n_top: int = 20, eps: float = 0.0, block_cells=None):
        """Which genes mark category k: the Wilcoxon rank-sum test of every gene, the cells of each category of arm ``arm``
        against all the others (``utils.marker_analysis.rank_sum_test``; scipy's ``mannwhitneyu`` without continuity
        correction, scanpy's tie-corrected ``wilcoxon`` score).  ``dl`` is encoded through the device encode path as for
        ``state_gene_corr``, the arm's eval labels are the groups, and ``mmvae_rank_sum`` reads the expression where it lies:
        a ``DeviceLoader``'s resident matrix through the batches' row indices, or, for a plain loader, the concatenation of
        its batches on the device.  Returns the ``rank_sum_test`` dict (all ``n_categories`` groups; a category with no cell
        has n = 0, z = 0 and p = 1) plus ``"categories"`` (the 0-based categories, int64 [G]) and ``"markers"``
        (``marker_genes(result, n_top)``: per category the ``n_top`` genes by z).  ``eps``: a cell expresses a gene where
        x > eps.  At most 32768 cells; with ``block_cells`` = "auto" or a block size (``rank_sum_test``'s keyword: the blocked
        rank sums, the same integers) at most 1048576.  The loader must serve every row once (no ``drop_last``)."""
        if D.is_dist():
            raise NotImplementedError("category_markers is not data-parallel: run it on one rank, outside the process group")
        if self.ref_prior:
            raise NotImplementedError("ref_prior is rejected by the reference loss (nn_model.py:578)")
        if not 0 <= int(arm) < self.n_arm:
            raise ValueError(f"arm = {arm} outside [0, {self.n_arm})")
        from .utils import marker_analysis as MA
        from .utils.dataloader import DeviceLoader
        resident = isinstance(dl, DeviceLoader)
        drops = bool(getattr(dl, "drop_last", False)) and dl.batch_size and len(dl.dataset) % dl.batch_size
        if (resident and dl.world_size > 1) or drops:
            raise ValueError("category_markers needs a loader that serves every row once (no drop_last, no sharding)")
        if block_cells is None and len(dl.dataset) > MA.MAX_CELLS:
            raise NotImplementedError(f"category_markers: {len(dl.dataset)} cells above the cap of {MA.MAX_CELLS} cells of one "
                                      "rank-sum call (run it on a subset of the cells, or pass block_cells=\"auto\")")
        MA._block_of(block_cells, len(dl.dataset), "category_markers")     # (a bad block and the blocked cap, before the encode)
        if not resident:
            dl = _Replay(dl, self.device)                                 # one walk of the loader: the same batches twice
        out, inds = self._encode_all(dl)
        if resident:
            data, rows = dl.data, inds.to(torch.int64)                     # the batches' indices are rows of the matrix
        else:
            data, rows = dl.matrix(), None
        cats = np.arange(self.n_categories, dtype=np.int64)
        res = MA.rank_sum_test(data, out["labels"][int(arm)].to(torch.int64), groups=cats, rows=rows, eps=eps,
                               block_cells=block_cells)
        res["categories"] = cats
        res["markers"] = MA.marker_genes(res, n_top=n_top)
        return res

    @torch.no_grad()
    def classify_latents(self, dl, labels, kfold: int = 10, seed=0, arm: int = 0, on: str = "x_low", kind: str = "qda"):
        """How well a Gaussian classifier recovers ``labels`` from arm ``arm``'s latents under k-fold cross-validation: the
        reference's ``QDA_classifier`` / ``LDA_classifier`` (mmidas/utils/cluster_analysis.py:38-83; ``kind`` "qda" or
        "lda") on ``on`` = "x_low" (the low-dimensional representation), "state_mu" (the state's mean) or "z_prob" (the
        categorical probabilities: points on the simplex, for which use "lda" or expect QDA to lean on its regulariser).
        ``dl`` is encoded through the device encode path (``fill_latents``, as ``encode_dataset``) and the latents never
        leave the device.  ``labels``: 1-D, one label per row of the data set; the label of a cell is ``labels[index]`` for
        the index its batch carries, so the cells are classified in the order the loader serves them.  Returns
        ``{"acc", "ref_labels", "pred_labels"}`` (lists over the folds, as the reference's dict entries for one label set),
        ``"margin"`` float64 [n] (best minus second-best score of every cell, in the loader's order; +inf where only one
        class is known), ``"fold"`` int64 [n] and ``"data_indx"``.  The loader must serve every row once (no ``drop_last``)."""
        if D.is_dist():
            raise NotImplementedError("classify_latents is not data-parallel: run it on one rank, outside the process group")
        from .utils import cluster_analysis as CA
        points, y, data_indx = self._latents_to_classify(dl, labels, arm, on, "classify_latents")
        return self._cv_result(CA.classify_points(points, y, kfold, seed, kind), data_indx)

    @torch.no_grad()
    def latent_neighbors(self, dl, k: int = 15, arm: int = 0, on: str = "x_low"):
        """The k-nearest-neighbour graph of the cells of ``dl`` in arm ``arm``'s latent space: what UMAP, Leiden and scanpy's
        ``pp.neighbors`` start from.  ``on`` = "x_low", "state_mu" or "z_prob", ``dl`` and the loaders refused as for
        ``classify_latents``; the latents never leave the device (``utils.neighbors.knn`` on them: Euclidean, a cell is not
        its own neighbour, ties by index, the same bits on every run).  Returns ``{"indices": int32 [n, k], "distances":
        float32 [n, k], "data_indx"}``: the cells in the order the loader serves them, ``indices`` positions in that order
        (``data_indx[indices]`` the data set's rows; -1 and +inf where n <= k).  ``utils.neighbors.csr_from_neighbors`` makes
        the CSR graph of them."""
        if D.is_dist():
            raise NotImplementedError("latent_neighbors is not data-parallel: run it on one rank, outside the process group")
        from .utils import neighbors as NB
        points, _, data_indx = self._latents_to_classify(dl, None, arm, on, "latent_neighbors")
        idx, dist = NB.knn(points, k)
        return {"indices": idx.cpu().numpy(), "distances": dist.cpu().numpy(), "data_indx": data_indx}

    @torch.no_grad()
    def classify_neighbors(self, dl, labels, k: int = 15, kfold: int = 10, seed=0, arm: int = 0, on: str = "x_low"):
        """How well the ``k`` nearest training cells recover ``labels`` from arm ``arm``'s latents under k-fold
        cross-validation: ``utils.neighbors.KNN_classifier``, the member of the ``classify_latents`` family that assumes no
        cluster shape.  ``dl``, ``labels``, ``arm``, ``on``, the folds and the loaders refused are ``classify_latents``'s; the
        latents never leave the device.  Returns its dict -- ``"acc"``, ``"ref_labels"``, ``"pred_labels"``, ``"fold"``,
        ``"data_indx"`` and ``"margin"`` float64 [n], here (the prediction's votes minus the most votes of another label) /
        k -- and ``"purity"`` float64 [n] (the share of a cell's k training neighbours with its own label) and
        ``"kth_distance"`` float32 [n], in the loader's order."""
        if D.is_dist():
            raise NotImplementedError("classify_neighbors is not data-parallel: run it on one rank, outside the process group")
        from .utils import neighbors as NB
        points, y, data_indx = self._latents_to_classify(dl, labels, arm, on, "classify_neighbors")
        classified = NB.classify_points(points, y, kfold, seed, k)
        res = self._cv_result(classified, data_indx, per=float(int(k)))
        res["purity"], res["kth_distance"] = classified[3]["purity"], classified[3]["kth_distance"]
        return res

    @torch.no_grad()
    def classify_tree(self, dl, labels, list_changes, leaves, kfold: int = 10, seed=0, arm: int = 0, on: str = "x_low", levels=None):
        """How well the cell types are recovered from arm ``arm``'s latents at EVERY resolution of the taxonomy: the
        reference's ``predict_leaf_gmm`` (mmidas/utils/analysis_tree_helpers.py) under k-fold cross-validation and at all
        merge levels of the dendrogram at once (``utils.analysis_tree_helpers.merge_sweep``).  ``labels``: one leaf label per row
        of the data set; ``list_changes`` and ``leaves``: the merge sequence and the leaf names (``parse_dend``); ``levels``:
        the numbers of merges to evaluate (default: every one that leaves at least two labels).  ``dl``, ``arm`` and ``on`` as
        for ``classify_latents``; the latents never leave the device.  Every cell is scored under the leaf Gaussians fitted to
        the folds it is not in (``kfold_of``): one ``mmvae_group_moments`` launch, one ``mmvae_gauss_scores`` launch with
        kfold models, one ``mmvae_leaf_merge``.  Returns ``{"n_classes" [T], "acc" [kfold, T], "pred" [T, n], "prob" [T, n],
        "fold" [n], "data_indx"}`` and ``"levels"`` and ``"keep"`` [n]: the accuracy of a fold is over its kept cells, those
        whose label is a leaf that has a model in their fold (NaN where a fold keeps none), in the loader's order."""
        if D.is_dist():
            raise NotImplementedError("classify_tree is not data-parallel: run it on one rank, outside the process group")
        from .utils import analysis_tree_helpers as TH
        points, y, data_indx = self._latents_to_classify(dl, labels, arm, on, "classify_tree")
        res = TH.classify_tree_points(points, y, list_changes, leaves, kfold, seed, levels)
        res["data_indx"] = data_indx
        return res

    def _latents_to_classify(self, dl, labels, arm, on, who, also=()):
        """What ``classify_latents`` and ``classify_forest`` share: their refusals, the encode of ``dl`` on the device and the
        labels of the cells it serves -> (arm ``arm``'s latents ``on``, float32 [n, .] on the device; the cells' labels;
        ``data_indx``).  ``also``: what else the caller takes for ``on``, for the message."""
        if self.ref_prior:
            raise NotImplementedError("ref_prior is rejected by the reference loss (nn_model.py:578)")
        if not 0 <= int(arm) < self.n_arm:
            raise ValueError(f"arm = {arm} outside [0, {self.n_arm})")
        names = {"x_low": "x_low", "state_mu": "s_mean", "z_prob": "c"}
        if on not in names:
            raise ValueError(f"on = {on!r}: one of {sorted(names) + list(also)}")
        from .utils.dataloader import DeviceLoader
        resident = isinstance(dl, DeviceLoader)
        if resident and (dl.world_size > 1 or (dl.drop_last and len(dl.dataset) % dl.batch_size)):
            raise ValueError(f"{who} needs a loader that serves every row once (no drop_last, no sharding)")
        out, inds = self._encode_all(dl if resident else _Replay(dl, self.device))
        data_indx = inds.cpu().numpy()
        y = None if labels is None else np.asarray(labels)[data_indx.astype(np.int64)]     # (latent_neighbors has no labels)
        return out[names[on]][int(arm)], y, data_indx

    def _expression_to_classify(self, dl, labels, who):
        """What ``classify_pcs`` and ``classify_forest(on="pcs")`` share: the loaders they refuse and the expression of the cells
        ``dl`` serves -> (the matrix on the device; its rows in visiting order, or None for all; the cells' labels;
        ``data_indx``)."""
        from .utils.dataloader import DeviceLoader
        resident = isinstance(dl, DeviceLoader)
        if resident and (dl.world_size > 1 or (dl.drop_last and len(dl.dataset) % dl.batch_size)):
            raise ValueError(f"{who} needs a loader that serves every row once (no drop_last, no sharding)")
        if resident:
            rows = torch.cat(list(dl.iter_rows()))                         # the epoch's rows of the matrix, in visiting order
            data, inds = dl.data, rows
        else:
            dl = _Replay(dl, self.device)
            data, rows = dl.matrix(), None
            inds = torch.cat([torch.as_tensor(i_x).reshape(-1) for _, i_x in dl])
        data_indx = inds.cpu().numpy()
        return data, rows, np.asarray(labels)[data_indx.astype(np.int64)], data_indx

    @staticmethod
    def _cv_result(classified, data_indx, per=1.0):
        """The dict of ``classify_latents``, ``classify_pcs`` and ``classify_forest`` from the (acc, ref_labels, pred_labels,
        prediction dict) of one label set; ``margin`` = (best - second) / ``per``: the scores' difference as it is, or the
        votes' as a share of the ``per`` trees."""
        acc, ref, pred, res = classified
        margin = (res["best"].astype(np.float64) - res["second"].astype(np.float64)) / per
        return {"acc": acc, "ref_labels": ref, "pred_labels": pred, "margin": margin, "fold": res["fold"], "data_indx": data_indx}

    @torch.no_grad()
    def classify_pcs(self, dl, labels, num_pc: int = 10, kfold: int = 10, seed=0, kind: str = "qda"):
        """The linear baseline beside ``classify_latents``: how well the same Gaussian classifier recovers ``labels`` from
        the top ``num_pc`` principal components of the expression of the cells of ``dl`` ("Linear vs Non-linear embedding" of
        the reference's clusterability notebook).  The components are those of the cells the loader serves
        (``utils.pca.pca_fit``: covariance, subspace iteration and projection on the device in fp64), read from a
        ``DeviceLoader``'s resident matrix through the epoch's row indices, in the loader's order, without a host copy; a
        plain loader's batches are concatenated on the device.  The model is not used: the answer depends on the data and
        the labels alone.  ``labels``, the folds, ``kind`` and the returned dict (``"acc"``, ``"ref_labels"``,
        ``"pred_labels"``, ``"margin"``, ``"fold"``, ``"data_indx"``) are those of ``classify_latents``, and so are the
        loaders it refuses (``drop_last`` with a remainder, sharding)."""
        if D.is_dist():
            raise NotImplementedError("classify_pcs is not data-parallel: run it on one rank, outside the process group")
        from .utils import cluster_analysis as CA
        from .utils.pca import pca_project
        data, rows, y, data_indx = self._expression_to_classify(dl, labels, "classify_pcs")
        checked = CA._cv_refusals(y, int(data_indx.shape[0]), kfold, seed, kind)       # every refusal before any device work
        z = pca_project(data, num_pc, rows=rows, out="device")
        return self._cv_result(CA.classify_points(z, y, kfold, seed, kind, checked), data_indx)

    @torch.no_grad()
    def classify_forest(self, dl, labels, kfold: int = 10, seed=0, arm: int = 0, on: str = "x_low", n_trees: int = 100,
                        num_pc: int = 10):
        """How well a random forest recovers ``labels`` under k-fold cross-validation: the reference's ``RF_classifier``
        (mmidas/utils/cluster_analysis.py:14-35; ``utils.cluster_analysis.forest_cv_predict`` states the forest and its
        departures from sklearn's) on arm ``arm``'s latents -- ``on`` = "x_low", "state_mu" or "z_prob", as
        ``classify_latents`` -- or, with ``on="pcs"``, on the top ``num_pc`` principal components of the expression of the
        cells of ``dl``, the linear baseline of ``classify_pcs`` (the model is then not used).  Nothing leaves the device
        between the encoder (or the projection) and the forest.  ``labels``, the loaders it takes and refuses and the
        returned dict (``"acc"``, ``"ref_labels"``, ``"pred_labels"``, ``"margin"``, ``"fold"``, ``"data_indx"``) are those of
        ``classify_latents``; ``"margin"`` float64 [n] is (the prediction's votes minus the most votes of another class) /
        ``n_trees``, in the loader's order."""
        if D.is_dist():
            raise NotImplementedError("classify_forest is not data-parallel: run it on one rank, outside the process group")
        from .utils import cluster_analysis as CA
        if on == "pcs":
            from .utils.pca import pca_project
            data, rows, y, data_indx = self._expression_to_classify(dl, labels, "classify_forest")
            checked = CA._forest_refusals(y, int(data_indx.shape[0]), int(num_pc), kfold, seed, n_trees, "sqrt")    # before the projection
            points = pca_project(data, num_pc, rows=rows, out="device")
        else:
            points, y, data_indx = self._latents_to_classify(dl, labels, arm, on, "classify_forest", also=("pcs",))
            checked = CA._forest_refusals(y, int(points.shape[0]), int(points.shape[1]), kfold, seed, n_trees, "sqrt")
        return self._cv_result(CA.classify_forest_points(CA._bins_on_device(points), y, kfold, seed, n_trees, checked), data_indx,
                               float(n_trees))


class _Replay:
    """The batches ``(x, index)`` of one walk of a loader, kept on the device: ``fill_latents`` and the matrix they form see the
    same cells in the same order whatever the loader's shuffling."""

    def __init__(self, loader, device):
        if loader.batch_size is None:
            raise ValueError("the loader needs a batch size")
        self.batch_size = loader.batch_size
        self._batches = [(x.to(device=device, dtype=torch.float32), i_x) for x, i_x in loader]
        self.dataset = range(sum(int(x.shape[0]) for x, _ in self._batches))

    def __iter__(self):
        return iter(self._batches)

    def matrix(self) -> torch.Tensor:
        return torch.cat([x for x, _ in self._batches])

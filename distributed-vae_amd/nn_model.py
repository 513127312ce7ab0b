"""Drop-in for the reference's ``mmidas/nn_model.py`` hot path, running on the HIP engine.

Mirrors (names, argument meaning, return contract, error behaviour):

* ``mixVAE_model``            mmidas/nn_model.py:89   (``__init__`` :112-261, ``forward`` :297-368,
                              ``loss`` :495-598, ``decoder`` :277-287, ``decoder_zinb`` :289-295,
                              ``state_changes`` :370-411)
* ``zinb_loss``               mmidas/nn_model.py:642-676 (the value; no backward)
* ``zinb_loss_grad``          no counterpart: the gradient of ``zinb_loss``'s value with respect to its three heads
* ``mk_vae``                  mmidas/nn_model.py:679-721
* ``VAEConfig``               mmidas/nn_model.py:14-36

``state_dict()`` has the reference's 46-keys-per-arm layout (``fc1.{a}.weight`` ...
``batch_s.{a}.num_batches_tracked``); every parameter is a view into one flat fp32 buffer that the
kernels read directly (include/mmvae.h).  All arithmetic happens in libmmvae_hip.so; there is no
PyTorch fallback -- without a GPU (or without the built library) ``forward`` raises.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional

import torch
from torch import nn
from torch.nn import ModuleList as mdl

from . import _native as N

# construction order of the reference (nn_model.py:184-203): decides RNG consumption at init
_LINEAR_ORDER = ["fc1", "fc2", "fc3", "fc4", "fc5", "fcc", "fc_mu", "fc_sigma", "fc6", "fc7", "fc8", "fc9", "fc10",
                 "fc11"]
_BN_ORDER = ["batch_l1", "batch_l2", "batch_l3", "batch_l4", "batch_l5", "batch_s"]


@dataclass
class VAEConfig:
    n_categories: int = 92
    state_dim: int = 2
    input_dim: int = 5032
    fc_dim: int = 100
    lowD_dim: int = 10
    x_drop: float = 0.5
    s_drop: float = 0.2
    lr: float = 0.001
    lam: float = 1
    lam_pc: float = 1
    n_arm: int = 2
    temp: float = 1.0
    tau: float = 0.005
    beta: float = 1.0
    hard: bool = False
    variational: bool = True
    ref_prior: bool = False
    trained_model: Optional[str] = None
    n_pr: int = 0
    momentum: float = 0.01
    mode: str = "MSE"


class _LossFn(torch.autograd.Function):
    """``loss.backward()`` (cpl_mixvae.py:462): routes into mmvae_backward and hands each parameter a
    view of the flat gradient buffer."""

    @staticmethod
    def forward(ctx, model, loss_value, *params):
        ctx.model = model
        ctx.step_id = model._step_id
        return loss_value.clone()

    @staticmethod
    def backward(ctx, grad_out):
        model = ctx.model
        if ctx.step_id != model._step_id or model._ctx is None:
            raise RuntimeError("backward() must follow the forward()/loss() pair that produced this loss")
        c = model._ctx
        model._engine.backward(c["hyper"], c["noise"], model._flat, c["x"], c["x_arm_stride"], model._flat_grad,
                               grad_scale=float(grad_out))
        return (None, None) + tuple(model._grad_views)


class mixVAE_model(nn.Module):
    """Multi-arm coupled mixture VAE (cpl-mixVAE); same constructor as nn_model.py:112-134."""

    def __init__(self, input_dim, fc_dim, n_categories, state_dim, lowD_dim, x_drop, s_drop, n_arm, lam, lam_pc,
                 tau, beta, hard, variational, device, eps, momentum, ref_prior, loss_mode, norm="batch"):
        super().__init__()
        self.input_dim = input_dim
        self.fc_dim = fc_dim
        self.lowD_dim = lowD_dim
        self.state_dim = state_dim
        self.n_categories = n_categories
        self.x_dp = nn.Dropout(x_drop)
        self.s_dp = nn.Dropout(s_drop)
        self.hard = hard
        self.n_arm = n_arm
        self.lam = lam
        self.lam_pc = lam_pc
        self.tau = tau
        self.beta = beta
        self.varitional = variational   # (sic) attribute name of the reference, nn_model.py:175
        self.eps = eps
        self.ref_prior = ref_prior
        self.momentum = momentum
        self.device = device
        self.loss_mode = loss_mode

        D, H, L, Cc, S = input_dim, fc_dim, lowD_dim, n_categories, state_dim
        shapes = {"fc1": (D, H), "fc2": (H, H), "fc3": (H, H), "fc4": (H, H), "fc5": (H, L), "fcc": (L, Cc),
                  "fc_mu": (L + Cc, S), "fc_sigma": (L + Cc, S), "fc6": (S + Cc, L), "fc7": (L, H), "fc8": (H, H),
                  "fc9": (H, H), "fc10": (H, H), "fc11": (H, D)}
        for name in _LINEAR_ORDER:
            i, o = shapes[name]
            setattr(self, name, mdl([nn.Linear(i, o) for _ in range(n_arm)]))
        if loss_mode == "ZINB":   # nn_model.py:204-206; used by decoder_zinb, the eval forward and zinb_nll, never trained
            self.fc11_p = mdl([nn.Linear(H, D) for _ in range(n_arm)])
            self.fc11_r = mdl([nn.Linear(H, D) for _ in range(n_arm)])
        bn_dims = {"batch_l1": H, "batch_l2": H, "batch_l3": H, "batch_l4": H, "batch_l5": L, "batch_s": S}
        for name in _BN_ORDER:
            setattr(self, name, mdl([nn.BatchNorm1d(num_features=bn_dims[name], eps=eps, momentum=momentum,
                                                    affine=False) for _ in range(n_arm)]))
        # engine state (created lazily on the parameters' device)
        self._engine: Optional[N.Engine] = None
        self._engines = {}
        self._flat = self._flat_grad = self._bn_flat = self._nbt = None
        self._grad_views: List[torch.Tensor] = []
        self._layout = None
        self._ctx = None
        self._step_id = 0
        self._explicit_noise = None
        self._noise_seed = None
        self._noise_offset = 0
        self._explicit_state_noise = None
        self._dec_engines = {}
        self._arm_engines = {}
        self._prune_dims = None
        self._exec: Optional[N.Exec] = None   # None: split factors / experiment switches from the environment
        # operand type of the five D x H GEMMs: "fp32" (the parity configuration) or "bf16" (BASELINE.json's bf16
        # configuration: operands rounded to bf16, fp32 accumulation; everything else and all parameters stay fp32)
        self.gemm_dtype = "fp32"

    # ------------------------------------------------------------------ flat parameter storage
    def _dims(self, B: int) -> N.Dims:
        return N.Dims(self.n_arm, B, self.input_dim, self.fc_dim, self.lowD_dim, self.n_categories, self.state_dim)

    def _param_of(self, t: int, a: int) -> nn.Parameter:
        name, kind = N.PARAM_NAMES[t].split(".")
        return getattr(getattr(self, name)[a], kind)

    def _is_packed(self) -> bool:
        if self._flat is None:
            return False
        p = self.fc1[0].weight
        lay = self._layout
        return (p.device == self._flat.device and p.data_ptr() == self._flat.data_ptr() + 4 * int(lay.offset[0])
                and self.fc11[self.n_arm - 1].bias.data_ptr()
                == self._flat.data_ptr() + 4 * (int(lay.per_arm) * (self.n_arm - 1) + int(lay.offset[27]))
                and self.batch_l1[0].running_mean.data_ptr() == self._bn_flat.data_ptr())

    def _pack(self):
        """(Re)build the flat buffers on the parameters' current device and re-point every parameter /
        BatchNorm buffer at a view of them.  Values are preserved."""
        dev = self.fc1[0].weight.device
        lay = N.param_layout(self._dims(2))
        A = self.n_arm
        flat = torch.zeros(A * int(lay.per_arm), dtype=torch.float32, device=dev)
        grad = torch.zeros_like(flat)
        bn = torch.zeros(A * int(lay.bn_per_arm), dtype=torch.float32, device=dev)
        nbt = torch.zeros(A * N.N_BN, dtype=torch.int64, device=dev)
        views = []
        with torch.no_grad():
            for a in range(A):
                for t in range(N.N_PARAM_TENSORS):
                    p = self._param_of(t, a)
                    o = a * int(lay.per_arm) + int(lay.offset[t])
                    v = flat[o: o + p.numel()].view(p.shape)
                    v.copy_(p.data.to(torch.float32))
                    p.data = v
                    gv = grad[o: o + p.numel()].view(p.shape)
                    if p.grad is not None:
                        gv.copy_(p.grad)
                        p.grad = gv
                    views.append((a, t, gv))
                for i, name in enumerate(_BN_ORDER):
                    m = getattr(self, name)[a]
                    n = int(lay.bn_dim[i])
                    om = a * int(lay.bn_per_arm) + int(lay.bn_mean_offset[i])
                    ov = a * int(lay.bn_per_arm) + int(lay.bn_var_offset[i])
                    bn[om: om + n].copy_(m.running_mean)
                    bn[ov: ov + n].copy_(m.running_var)
                    m.running_mean = bn[om: om + n]
                    m.running_var = bn[ov: ov + n]
                    nbt[a * N.N_BN + i] = m.num_batches_tracked
                    m.num_batches_tracked = nbt[a * N.N_BN + i]
        # gradient views in model.parameters() order (layer-major, then arm; nn_model.py:184-203)
        order = {id(p): k for k, p in enumerate(self.parameters())}
        gv_sorted = [None] * len(order)
        for a, t, gv in views:
            gv_sorted[order[id(self._param_of(t, a))]] = gv
        self._grad_views = gv_sorted
        self._flat, self._flat_grad, self._bn_flat, self._nbt, self._layout = flat, grad, bn, nbt, lay
        self._engine = None
        self._engines = {}
        self._arm_engines = {}

    def _ensure(self, B: int) -> N.Engine:
        if not self._is_packed():
            self._pack()
        mode = N.gemm_mode(self.gemm_dtype)
        if (self._engine is None or self._engine.dims.B != B or self._engine.device != self._flat.device
                or self._engine.gemm_engine != mode):
            # a trainer alternates between a few batch sizes (training batch, evaluation chunks, their ragged tails):
            # keep the last few engines (workspace + events each) instead of reallocating 0.5 GB per switch.  The GEMM
            # engine is part of the key: the workspace's split factors are chosen for its workgroup shapes.
            key = (B, str(self._flat.device), id(self._exec), mode)
            eng = self._engines.pop(key, None)
            if eng is None:
                d = self._dims(B)
                eng = N.Engine(d.A, d.B, d.D, d.H, d.L, d.C, d.S, self._flat.device, self._exec, gemm_engine=mode)
            self._engines[key] = eng
            while len(self._engines) > 3:
                self._engines.pop(next(iter(self._engines)))
            self._engine = eng
        return self._engine

    def flat_parameters(self) -> torch.Tensor:
        """The flat fp32 parameter buffer (arm-major, layout of mmvae_param_layout)."""
        if not self._is_packed():
            self._pack()
        return self._flat

    def flat_grad(self) -> torch.Tensor:
        if not self._is_packed():
            self._pack()
        return self._flat_grad

    def bind_grads(self):
        """Point every parameter's ``.grad`` at its view of the flat gradient buffer (what ``loss.backward()`` does on
        the three-call path), so that a stock ``torch.optim`` optimizer can follow a fused step run with do_adam=False."""
        if not self._is_packed():
            self._pack()
        for p, gv in zip(self.parameters(), self._grad_views):
            p.grad = gv
        if self.loss_mode == "ZINB":      # the p and r heads: views of their own gradient buffer (``zinb_train_step`` fills it)
            _, hg = self.zinb_heads_flat()
            for a, _, p, o in self._zinb_head_params():
                p.grad = hg[a, o: o + p.numel()].view(p.shape)

    # ------------------------------------------------------------------ noise control
    def set_explicit_noise(self, noise):
        """Parity hook: x_mask uint8 [A,B,D], u_gumbel [A,B,C], u_state [A,B,S], s_mask uint8 [A,B,S]
        (device tensors) consumed by the next forward passes; None returns to in-kernel Philox.  A LIST of such
        dicts is a schedule: every forward / fused step takes the next entry (running out raises), which is how a
        recorded run of the reference trainer is replayed step by step."""
        self._explicit_noise = list(noise) if isinstance(noise, (list, tuple)) else noise

    def _hyper(self, temp: float, eval_flag: bool) -> N.Hyper:
        return N.Hyper(self.tau, float(temp), self.beta, self.lam, self.eps, self.momentum, float(self.x_dp.p),
                       float(self.s_dp.p), int(bool(self.hard)), int(self.training), int(bool(eval_flag)),
                       N.gemm_mode(self.gemm_dtype))

    def _next_noise(self) -> N.Noise:
        if isinstance(self._explicit_noise, list):
            if not self._explicit_noise:
                raise RuntimeError("explicit noise schedule exhausted")
            self._noise_keep = self._explicit_noise.pop(0)      # keeps the tensors alive while the kernels read them
            return N.make_noise(self._noise_keep)
        if self._explicit_noise is not None:
            return N.make_noise(self._explicit_noise)
        if self._noise_seed is None:
            self._noise_seed = int(torch.initial_seed()) & 0xFFFFFFFFFFFFFFFF
        self._noise_offset += 1
        return N.make_noise(None, self._noise_seed, self._noise_offset)

    # ------------------------------------------------------------------ reference API
    def _prep_x(self, x):
        """Accepts the reference's inputs: a list of A [B,D] tensors or an [A,B,D] tensor (typically
        ``x.expand(A,-1,-1)``, cpl_mixvae.py:425).  Returns (tensor, arm stride in floats)."""
        if isinstance(x, torch.Tensor):
            assert x.dim() == 3, "x must be [n_arm, batch, input_dim]"
            if x.stride(0) == 0:
                return x[0].contiguous().float(), 0
            xc = x.contiguous().float()
            return xc, xc.shape[1] * xc.shape[2]
        xs = list(x)
        if all(t.data_ptr() == xs[0].data_ptr() and t.shape == xs[0].shape for t in xs):
            return xs[0].contiguous().float(), 0
        xc = torch.stack([t.float() for t in xs]).contiguous()
        return xc, xc.shape[1] * xc.shape[2]

    def forward(self, x, temp, prior_c=[], eval=False, mask=None):
        """Same contract as nn_model.py:297-368: returns
        ``x_recs, [], [], x_lows, cs, s_smps, c_smps, s_means, s_logvars, c_probs`` (lists over arms).  A model built with
        ``loss_mode="ZINB"`` runs in eval mode with ``eval=True`` only (anything else asserts, as the reference does), and
        positions 1 and 2 then hold the per-arm ``x_p`` and ``x_r`` [B, D] (mmvae_zinb_heads on the workspace's d10)."""
        return self._forward(x, temp, eval, mask, True)

    def _forward(self, x, temp, eval, mask, heads):
        """``forward``; ``heads=False`` leaves the two ZINB heads out (``zinb_nll`` forms them tile by tile)."""
        zinb = self.loss_mode == "ZINB"
        # ZINB: the eval-mode forward only (the heads from the workspace's d10); training keeps the reference's refusal
        assert not zinb or (eval and not self.training), "ZINB not implemented"
        assert self.varitional, "Non-variational not implemented"
        assert len(x) == self.n_arm
        mask_words = None
        if mask is not None:
            # nn_model.py:332-335: c = softmax(c_prob[:, mask] / tau) on the kept categories, 0 elsewhere.  eval_model passes the
            # indices of the categories whose fcc bias is non-zero (cpl_mixvae.py:1476-1478, :1524): every category for an
            # unpruned model, a subset for a checkpoint of a pruned one.  (A boolean mask selects like an index list.)
            import numpy as _np
            mk = _np.asarray(mask.detach().cpu() if isinstance(mask, torch.Tensor) else mask)
            mk = _np.flatnonzero(mk) if mk.dtype == _np.bool_ else _np.unique(mk.astype(_np.int64))
            if mk.size == 0 or mk[0] < 0 or mk[-1] >= self.n_categories:
                raise IndexError(f"category mask {mk.tolist()} outside [0, {self.n_categories})")
            if mk.size < self.n_categories:
                mask_words = [0, 0, 0, 0]
                for k in mk.tolist():
                    mask_words[k >> 5] |= 1 << (k & 31)
        if self.ref_prior:
            raise NotImplementedError("ref_prior is rejected by the reference loss (nn_model.py:578)")
        xt, xs = self._prep_x(x)
        if xt.device.type != "cuda":
            raise N.NativeError("mixVAE_model.forward needs GPU tensors: the model runs only on the HIP engine")
        A, B, D = self.n_arm, xt.shape[-2], xt.shape[-1]
        assert D == self.input_dim
        eng = self._ensure(B)
        hyper = self._hyper(temp, eval)
        if mask_words is not None:
            for i in range(4):
                hyper.cat_mask[i] = mask_words[i]
        noise = self._next_noise()
        need_grad = bool(self.training and torch.is_grad_enabled())
        x_rec = torch.empty(A, B, D, dtype=torch.float32, device=xt.device)
        eng.forward(hyper, noise, self._flat, self._bn_flat, self._nbt if self.training else None, xt, xs, x_rec,
                    need_grad)
        self._step_id += 1
        self._ctx = {"hyper": hyper, "noise": noise, "x": xt, "x_arm_stride": xs, "need_grad": need_grad,
                     "keep": self._explicit_noise}
        L, Cc, S = self.lowD_dim, self.n_categories, self.state_dim
        grab = lambda name, w: list(eng.ws_view(name, w).clone().unbind(0))
        x_ps, x_rs = [], []
        if zinb and heads:              # positions 1 and 2: the older snapshot's zinb_pi and zinb_r
            d10 = eng.ws_view("d10", self.fc_dim)
            for a in range(A):
                x_p, x_r = N.zinb_heads(d10[a], *self._zinb_layers(a)[2:])
                x_ps.append(x_p)
                x_rs.append(x_r)
        out = (list(x_rec.unbind(0)), x_ps, x_rs, grab("x_low", L), grab("c", Cc), grab("s_smp", S), grab("c_smp", Cc),
               grab("s_mean", S), grab("s_logvar", S), grab("c_prob", Cc))
        self._ctx["outs"] = out           # loss() checks that it is handed exactly these, unmodified
        self._ctx["versions"] = {i: [t._version for t in out[i]] for i in (0, 4, 6, 7, 8)}
        self._ctx["x_in"] = x if isinstance(x, torch.Tensor) else list(x)
        return out

    @staticmethod
    def _same(given, kept, versions) -> bool:
        """Is ``given`` (a list of per-arm tensors, or one stacked tensor) the list ``forward`` returned, unmodified?"""
        if isinstance(given, torch.Tensor):
            given = list(given.unbind(0)) if given.dim() == kept[0].dim() + 1 else [given]
        try:
            given = list(given)
        except TypeError:
            return False
        return len(given) == len(kept) and all(
            isinstance(g, torch.Tensor) and g.data_ptr() == k.data_ptr() and g.shape == k.shape and g._version == v
            for g, k, v in zip(given, kept, versions))

    def loss(self, recon_x, p_x, r_x, x, mu, log_sigma, qc, c, prior_c=[]):
        """Same contract as nn_model.py:495-598; returns the reference's 9-tuple.

        The loss is evaluated by the kernels on what the preceding ``forward`` left in the workspace, so ``recon_x``,
        ``mu``, ``log_sigma``, ``qc`` and ``c`` MUST be the tensors that ``forward`` returned (outputs 0, 7, 8, 4, 6,
        unmodified) and ``x`` the input it was given: anything else raises instead of silently returning the loss of
        other tensors (the reference, mmidas/model.py:108-113, computes from whatever it is handed)."""
        assert len(recon_x) == len(c) == self.n_arm
        assert not self.ref_prior
        if self.loss_mode == "ZINB":
            raise NotImplementedError("loss() under loss_mode='ZINB' is not built (the reference asserts there, nn_model.py:548); "
                                      "zinb_nll() scores a batch under the model")
        if self._ctx is None:
            raise RuntimeError("loss() must follow forward()")
        A = self.n_arm
        kept = self._ctx["outs"]
        for name, given, idx in (("recon_x", recon_x, 0), ("mu", mu, 7), ("log_sigma", log_sigma, 8), ("qc", qc, 4),
                                 ("c", c, 6)):
            if not self._same(given, kept[idx], self._ctx["versions"][idx]):
                raise ValueError(f"loss(): `{name}` is not the unmodified output {idx} of the preceding forward(); the HIP "
                                 "engine evaluates the loss on the tensors its forward produced")
        x_in = self._ctx["x_in"]
        same_obj = x is x_in or (not isinstance(x, torch.Tensor) and not isinstance(x_in, torch.Tensor) and x is not None
                                 and len(x) == len(x_in) and all(p is q for p, q in zip(x, x_in)))
        if x is not None and not same_obj:   # (None: callers that only want the scalars of the last forward)
            xt, _ = self._prep_x(x)
            x0 = self._ctx["x"]
            if not (xt.data_ptr() == x0.data_ptr() or (xt.shape == x0.shape and torch.equal(xt, x0))):
                raise ValueError("loss(): `x` is not the input of the preceding forward()")
        eng = self._engine
        buf = eng.loss(self._ctx["hyper"])
        if A == 1:
            # the reference divides by len([]) here (nn_model.py:592-594)
            raise ZeroDivisionError("division by zero")
        vals = buf.clone()
        total = vals[N.LOSS_TOTAL]
        if self._ctx["need_grad"]:
            total = _LossFn.apply(self, total, *self.parameters())
        rec = vals[N.LOSS_REC0: N.LOSS_REC0 + A]
        kl = vals[N.LOSS_REC0 + A: N.LOSS_REC0 + 2 * A]
        ll = vals[N.LOSS_REC0 + 2 * A: N.LOSS_REC0 + 3 * A]
        return (total, rec.clone(), vals[N.LOSS_JOINT], vals[N.LOSS_CENT], vals[N.LOSS_CDIST], vals[N.LOSS_CL2],
                list(kl.unbind(0)), [], list(ll.unbind(0)))

    # ------------------------------------------------------------------ evaluation labels (consensus path)
    @torch.no_grad()
    def eval_labels(self, x, temp=1.0, counts=None, mask=None) -> torch.Tensor:
        """``classify(cs[a])`` of ``self(x, temp, eval=True)`` for every arm without leaving the device
        (cpl_mixvae.py:596-611): int32 [n_arm, batch].  Runs the encoder and the latent block only (BatchNorm running
        statistics, no Gumbel noise); ``counts`` (int64 [pairs, C, C], see ``_utils.confmat_counts``) also receives
        this batch's between-arm confusion counts.  ``mask``: the kept categories, as ``forward(mask=)`` takes them (the
        pruning phase's assessment, cpl_mixvae.py:1040-1042).  The module must be in eval mode, as in the reference's loop."""
        words = self._mask_words(mask)
        if self.training:
            raise RuntimeError("eval_labels() needs model.eval(): the reference classifies in eval mode "
                               "(cpl_mixvae.py:563)")
        xt, xs = self._prep_x(x)
        if xt.device.type != "cuda":
            raise N.NativeError("mixVAE_model.eval_labels needs GPU tensors: the model runs only on the HIP engine")
        eng = self._ensure(xt.shape[-2])
        labels = torch.empty(self.n_arm, xt.shape[-2], dtype=torch.int32, device=xt.device)
        hyper = self._hyper(temp, True)
        if words is not None:
            for i in range(4):
                hyper.cat_mask[i] = words[i]
        eng.eval_classify(hyper, self._flat, self._bn_flat, xt, xs, labels, counts)
        self._ctx = None
        return labels

    # ------------------------------------------------------------------ the encoder alone, latents without the decoder
    def _mask_words(self, mask):
        """The category subset of ``forward(mask=...)`` as the four words of mmvae_hyper.cat_mask, validated as ``forward``
        validates it; None: every category is kept."""
        if mask is None:
            return None
        import numpy as _np
        mk = _np.asarray(mask.detach().cpu() if isinstance(mask, torch.Tensor) else mask)
        mk = _np.flatnonzero(mk) if mk.dtype == _np.bool_ else _np.unique(mk.astype(_np.int64))
        if mk.size == 0 or mk[0] < 0 or mk[-1] >= self.n_categories:
            raise IndexError(f"category mask {mk.tolist()} outside [0, {self.n_categories})")
        if mk.size == self.n_categories:
            return None
        words = [0, 0, 0, 0]
        for k in mk.tolist():
            words[k >> 5] |= 1 << (k & 31)
        return words

    def _arm_engine(self, B: int) -> N.Engine:
        """The engine of a ONE-arm call on B cells (``encoder``): its split factors are those of the model's A-arm engine
        for this batch, so that fc1 sums its K pieces in the order ``forward`` does and the outputs agree bit for bit."""
        full = self._ensure(B)
        mode = N.gemm_mode(self.gemm_dtype)
        key = (B, str(self._flat.device), id(self._exec), mode)
        eng = self._arm_engines.pop(key, None)
        if eng is None:
            ex = N.Exec()
            for i in range(N.N_TUNE):
                ex.tune[i] = full.ex.tune[i]
            for i, k in enumerate(full.splits()):
                ex.split[i] = k
            d = full.dims
            eng = N.Engine(1, B, d.D, d.H, d.L, d.C, d.S, self._flat.device, ex, gemm_engine=mode)
        self._arm_engines[key] = eng
        while len(self._arm_engines) > 3:
            self._arm_engines.pop(next(iter(self._arm_engines)))
        return eng

    @torch.no_grad()
    def encoder(self, x, arm):
        """nn_model.py:263-269: ``(x_low, softmax(fcc(x_low)))`` of arm ``arm`` for x [N, D] on the device; returns the
        device tensors [N, L] and [N, C].  Eval mode: running statistics, any N.  Training mode, as in the reference: input
        dropout (the mask a ``forward`` at this point of the model's noise source would draw for this arm; one entry /
        offset is consumed), batch statistics, and ``batch_l1..5[arm]``'s running statistics and counters move."""
        arm = int(arm)
        if not (0 <= arm < self.n_arm):
            raise IndexError(f"arm {arm} outside [0, {self.n_arm})")
        if x.device.type != "cuda":
            raise N.NativeError("mixVAE_model.encoder needs GPU tensors: the model runs only on the HIP engine")
        xt = x.reshape(-1, x.shape[-1]).contiguous().float()
        n = xt.shape[0]
        assert xt.shape[1] == self.input_dim
        eng = self._arm_engine(n)
        hyper = self._hyper(1.0, True)
        noise = None
        if self.training:
            if self.x_dp.p > 0:
                if isinstance(self._explicit_noise, list):
                    if not self._explicit_noise:
                        raise RuntimeError("explicit noise schedule exhausted")
                    mask = self._explicit_noise.pop(0)["x_mask"][arm]
                elif self._explicit_noise is not None:
                    mask = self._explicit_noise["x_mask"][arm]
                else:
                    # the mask the A-arm forward would draw at this offset, written out; this arm's slice is explicit noise
                    full = self._ensure(n)
                    mask = full.dump_noise(self._hyper(1.0, False), self._next_noise())["x_mask"][arm]
                self._noise_keep = mask = mask.contiguous()
                noise = N.make_noise({"x_mask": mask})
            else:
                self._next_noise()
                noise = N.make_noise({})
        lay = self._layout
        params = self._flat[arm * int(lay.per_arm):]
        bn = self._bn_flat[arm * int(lay.bn_per_arm):]
        nbt = self._nbt[arm * N.N_BN:] if self.training else None
        out = {"x_low": torch.empty(1, n, self.lowD_dim, dtype=torch.float32, device=xt.device),
               "c_prob": torch.empty(1, n, self.n_categories, dtype=torch.float32, device=xt.device)}
        eng.encode(hyper, noise, params, bn, nbt, xt, 0, out)
        self._ctx = None
        return out["x_low"][0], out["c_prob"][0]

    @torch.no_grad()
    def intermed(self, y, arm):
        """nn_model.py:271-275: ``(fc_mu(y), sigmoid(fc_sigma(y)))`` of arm ``arm`` for y [N, L + C] on the device; returns
        the device tensors [N, S] each (the log with eps is ``forward``'s)."""
        assert self.varitional, "Non-variational not implemented"
        arm = int(arm)
        if not (0 <= arm < self.n_arm):
            raise IndexError(f"arm {arm} outside [0, {self.n_arm})")
        if y.device.type != "cuda":
            raise N.NativeError("mixVAE_model.intermed needs GPU tensors: the model runs only on the HIP engine")
        K = self.lowD_dim + self.n_categories
        yt = y.reshape(-1, y.shape[-1]).contiguous().float()
        assert yt.shape[1] == K
        if not self._is_packed():
            self._pack()
        n = yt.shape[0]
        mu = torch.empty(n, self.state_dim, dtype=torch.float32, device=yt.device)
        var = torch.empty_like(mu)
        d = N.Dims(1, n, self.input_dim, self.fc_dim, self.lowD_dim, self.n_categories, self.state_dim)
        with torch.cuda.device(yt.device):
            N.intermed(d, self._hyper(1.0, True), self._flat[arm * int(self._layout.per_arm):], yt, 0, mu, var)
        return mu, var

    @torch.no_grad()
    def encode(self, x, temp=1.0, mask=None, out=None, row0=0, counts=None):
        """The latents of ``self(x, temp, eval=True, mask=mask)`` for every arm without the decoder, fc11 or x_rec
        (mmvae_encode): a dict of device tensors ``x_low`` [A,N,L], ``c_prob``, ``c``, ``c_smp`` [A,N,C], ``s_mean``,
        ``s_logvar`` [A,N,S] and ``labels`` int32 [A,N] (argmax of c) -- the forward's values bit for bit.  x: as
        ``forward`` takes it ([A,N,D] or a list of A [N,D] tensors).  ``out``: such a dict of [A, rows, .] arrays to write
        at rows ``row0 .. row0 + N`` instead (how ``cpl_mixVAE.encode_dataset`` fills a data set's arrays chunk by chunk);
        ``counts``: int64 [pairs, C, C] that also receives this batch's between-arm confusion counts.  The module must be
        in eval mode."""
        if self.training:
            raise RuntimeError("encode() needs model.eval(): the reference classifies in eval mode "
                               "(cpl_mixvae.py:563)")
        words = self._mask_words(mask)
        xt, xs = self._prep_x(x)
        if xt.device.type != "cuda":
            raise N.NativeError("mixVAE_model.encode needs GPU tensors: the model runs only on the HIP engine")
        A, n = self.n_arm, xt.shape[-2]
        assert xt.shape[-1] == self.input_dim
        eng = self._ensure(n)
        hyper = self._hyper(temp, True)
        if words is not None:
            for i in range(4):
                hyper.cat_mask[i] = words[i]
        rows = n
        if out is None:
            f32 = dict(dtype=torch.float32, device=xt.device)
            L, Cc, S = self.lowD_dim, self.n_categories, self.state_dim
            out = {"x_low": torch.empty(A, n, L, **f32), "c_prob": torch.empty(A, n, Cc, **f32),
                   "c": torch.empty(A, n, Cc, **f32), "c_smp": torch.empty(A, n, Cc, **f32),
                   "s_mean": torch.empty(A, n, S, **f32), "s_logvar": torch.empty(A, n, S, **f32),
                   "labels": torch.empty(A, n, dtype=torch.int32, device=xt.device)}
        else:
            rows = next(t for t in out.values() if t is not None).shape[1]
        args = dict(out)
        if counts is not None:
            args["counts"] = counts
        eng.encode(hyper, None, self._flat, self._bn_flat, None, xt, xs, args, row0, rows)
        self._ctx = None
        return out

    # ------------------------------------------------------------------ decoding a chosen code, state traversal
    def _dec_engine(self, A: int, rows: int, n_samp=None) -> N.DecodeEngine:
        if not self._is_packed():
            self._pack()
        mode = N.gemm_mode(self.gemm_dtype)
        key = (A, rows, n_samp, str(self._flat.device), mode)
        eng = self._dec_engines.pop(key, None)
        if eng is None:
            eng = N.DecodeEngine(A, rows, self.input_dim, self.fc_dim, self.lowD_dim, self.n_categories, self.state_dim,
                                 self._flat.device, mode, n_samp, self._exec)
        self._dec_engines[key] = eng
        while len(self._dec_engines) > 3:
            self._dec_engines.pop(next(iter(self._dec_engines)))
        return eng

    def _decode_run(self, c, s, arm):
        """``decoder``: (x_rec [N, D], the decode engine whose workspace now holds the chain's activations)."""
        if self.training and self.s_dp.p > 0:
            raise NotImplementedError("decoder(): state dropout (training mode, s_drop > 0) is not supported; call model.eval()")
        if not (0 <= int(arm) < self.n_arm):
            raise IndexError(f"arm {arm} outside [0, {self.n_arm})")
        if c.device.type != "cuda" or s.device.type != "cuda":
            raise N.NativeError("mixVAE_model.decoder needs GPU tensors: the model runs only on the HIP engine")
        c = c.reshape(-1, self.n_categories).contiguous().float()
        s = s.reshape(-1, self.state_dim).contiguous().float()
        if c.shape[0] != s.shape[0]:
            raise ValueError(f"decoder(): c has {c.shape[0]} rows, s has {s.shape[0]}")
        n = c.shape[0]
        eng = self._dec_engine(1, n)
        x_rec = torch.empty(n, self.input_dim, dtype=torch.float32, device=c.device)
        per_arm = int(self._layout.per_arm)
        params = self._flat[int(arm) * per_arm:]                     # that arm's segment: a one-arm model
        eng.decode(self._hyper(1.0, True), params, c, 0, s, 0, x_rec)
        return x_rec, eng

    @torch.no_grad()
    def decoder(self, c, s, arm):
        """nn_model.py:277-287: ``relu(fc11(relu(fc10(... relu(fc6([c | s]))))))`` of arm ``arm`` for c [N, C], s [N, S]
        (device tensors); returns the device tensor [N, D].  State dropout is the identity in eval mode; in training mode
        with s_drop > 0 this raises NotImplementedError (the library does not offer a decode with state dropout)."""
        return self._decode_run(c, s, arm)[0]

    # ------------------------------------------------------------------ zero-inflated negative binomial inference
    def _need_zinb(self, what: str):
        if self.loss_mode != "ZINB":
            raise RuntimeError(f"{what} needs a model built with loss_mode='ZINB' (this one has loss_mode={self.loss_mode!r}: "
                               "it has no fc11_p / fc11_r heads)")

    def _zinb_layers(self, arm: int):
        """(fc11.weight, fc11.bias, fc11_p.weight, fc11_p.bias, fc11_r.weight, fc11_r.bias) of arm ``arm``, detached."""
        return tuple(t.detach() for m in (self.fc11[arm], self.fc11_p[arm], self.fc11_r[arm]) for t in (m.weight, m.bias))

    def _refuse_zinb_training(self):
        if self.loss_mode == "ZINB":
            raise NotImplementedError("training under loss_mode='ZINB' is not built")

    @torch.no_grad()
    def decoder_zinb(self, c, s, arm):
        """nn_model.py:289-295: ``(relu(fc11(h)), sigmoid(fc11_p(h)), sigmoid(fc11_r(h)))`` with h the decoder's last hidden
        layer, for c [N, C], s [N, S] (device tensors) -> three device tensors [N, D].  x_rec is ``decoder``'s output bit for
        bit (the same decode runs); the two heads come from that decode's fp32 d10 (mmvae_zinb_heads).  Refusals: those of
        ``decoder``; RuntimeError for a model not built with ``loss_mode="ZINB"``."""
        self._need_zinb("decoder_zinb()")
        x_rec, eng = self._decode_run(c, s, arm)
        x_p, x_r = N.zinb_heads(eng.ws_view("d10", self.fc_dim)[0], *self._zinb_layers(int(arm))[2:])
        return x_rec, x_p, x_r

    @torch.no_grad()
    def zinb_nll(self, x, temp=1.0, mask=None):
        """The ZINB negative log-likelihood of the batch ``x`` (as ``forward`` takes it) under the model: an eval forward, then
        mmvae_zinb_nll per arm on the forward workspace's d10 -- the three heads are formed tile by tile and never written.
        Returns ``{"cell": float64 [A, B] (the term summed over the genes), "gene": float64 [A, D] (over the cells), "n": B}``
        on the device.  The eval forward samples s_smp, as the reference's does: a cell's value depends on its draw
        (``set_explicit_noise`` fixes it).  Needs model.eval()."""
        self._need_zinb("zinb_nll()")
        if self.training:
            raise RuntimeError("zinb_nll() needs model.eval()")
        self._forward(x, temp, True, mask, False)
        eng, xt, xs = self._engine, self._ctx["x"], self._ctx["x_arm_stride"]
        A, B, D = self.n_arm, xt.shape[-2], self.input_dim
        d10 = eng.ws_view("d10", self.fc_dim)
        cell = torch.empty(A, B, dtype=torch.float64, device=xt.device)
        gene = torch.empty(A, D, dtype=torch.float64, device=xt.device)
        for a in range(A):
            xa = xt if xs == 0 else xt[a]
            cell[a], gene[a] = N.zinb_nll(d10[a], *self._zinb_layers(a), xa)
        self._ctx = None
        return {"cell": cell, "gene": gene, "n": B}

    @torch.no_grad()
    def zinb_head_grads(self, x, temp=1.0, mask=None, heads=("rec", "p", "r")):
        """The gradient of the batch's mean ZINB term (``zinb_loss`` of the batch) with respect to the weights and biases of
        the decoder's heads, the trunk held fixed: one eval forward, then mmvae_zinb_head_grads per arm on the forward
        workspace's d10 -- neither the pre-activations nor their gradients are written.  ``heads`` selects among "rec"
        (``fc11``), "p" (``fc11_p``) and "r" (``fc11_r``).  Returns, per arm, ``{"loss": float64 0-dim, "fc11": (dW, db),
        "fc11_p": (dW, db), "fc11_r": (dW, db)}`` on the device with the selected heads only; dW float32 [D, H], db float32
        [D].  Needs model.eval()."""
        return self._zinb_head_grads(x, temp, mask, heads, None, None)

    def _zinb_head_grads(self, x, temp, mask, heads, layers, out):
        """``zinb_head_grads`` for ``cpl_mixVAE.fit_zinb_heads``, which keeps the heads it fits and their gradients in flat
        buffers of its own: ``layers`` (per arm, the six tensors of ``_zinb_layers``) stands in for the heads the model holds,
        ``out`` (per arm, ``{head: (dW, db)}``) receives the gradients."""
        self._need_zinb("zinb_head_grads()")
        N.zinb_head_mask(heads)
        if self.training:
            raise RuntimeError("zinb_head_grads() needs model.eval()")
        self._forward(x, temp, True, mask, False)
        eng, xt, xs = self._engine, self._ctx["x"], self._ctx["x_arm_stride"]
        B, D = xt.shape[-2], self.input_dim
        d10 = eng.ws_view("d10", self.fc_dim)
        names = {"rec": "fc11", "p": "fc11_p", "r": "fc11_r"}
        res = []
        for a in range(self.n_arm):
            xa = xt if xs == 0 else xt[a]
            g, cell, _ = N.zinb_head_grads(d10[a], *(self._zinb_layers(a) if layers is None else layers[a]), xa, heads=heads,
                                           out=None if out is None else out[a])
            r = {"loss": cell.sum() / (float(B) * float(D))}
            r.update({names[h]: g[h] for h in N.ZINB_HEADS if h in g})
            res.append(r)
        self._ctx = None
        return res

    @torch.no_grad()
    def zinb_decoder_grads(self, x, temp=1.0, mask=None, heads=("rec", "p", "r")):
        """The gradient of the batch's mean ZINB term with respect to the whole decoder, the encoder held fixed: one eval
        forward, then per arm mmvae_zinb_head_grads (the selected heads), mmvae_zinb_d10_grad (the decoder's last hidden
        layer, through the selected heads) and mmvae_decoder_trunk_grads (``fc6`` .. ``fc10``) on the forward workspace's
        ``zin``, ``d6`` .. ``d10``; nothing N x D is written.  Returns, per arm, ``{"loss": float64 0-dim, "fc6": (dW, db) ..
        "fc10": (dW, db), "fc11" / "fc11_p" / "fc11_r": (dW, db) for the selected heads, "d10": float32 [B, H], "c": float32
        [B, C], "s": float32 [B, S]}`` on the device; "c" and "s" are the gradient with respect to the decoder's input
        ``[c | s]``.  Refusals: those of ``zinb_head_grads``."""
        return self._zinb_decoder_grads(x, temp, mask, heads, None, None, None, True)

    def _zinb_decoder_grads(self, x, temp, mask, heads, layers, out, trunk_out, want_gzin):
        """``zinb_decoder_grads`` for ``cpl_mixVAE.fit_zinb_decoder``: ``layers`` and ``out`` as ``_zinb_head_grads`` takes
        them, ``trunk_out`` (per arm, ten views of a flat gradient buffer) receives the trunk's gradients."""
        self._need_zinb("zinb_decoder_grads()")
        N.zinb_head_mask(heads)
        if self.training:
            raise RuntimeError("zinb_decoder_grads() needs model.eval()")
        self._forward(x, temp, True, mask, False)
        eng, xt, xs = self._engine, self._ctx["x"], self._ctx["x_arm_stride"]
        B, D, H, Cc = xt.shape[-2], self.input_dim, self.fc_dim, self.n_categories
        acts = [eng.ws_view("zin", Cc + self.state_dim), eng.ws_view("d6", self.lowD_dim)] + [eng.ws_view(f"d{k}", H) for k in (7, 8, 9, 10)]
        names = {"rec": "fc11", "p": "fc11_p", "r": "fc11_r"}
        res = []
        for a in range(self.n_arm):
            xa = xt if xs == 0 else xt[a]
            lay = self._zinb_layers(a) if layers is None else layers[a]
            act = [v[a] for v in acts]
            g, cell, _ = N.zinb_head_grads(act[5], *lay, xa, heads=heads, out=None if out is None else out[a])
            gd10 = N.zinb_d10_grad(act[5], *lay, xa, heads=heads)
            params = [t.detach() for nm in N.TRUNK_LAYERS for t in (getattr(self, nm)[a].weight, getattr(self, nm)[a].bias)]
            tg, gzin = N.decoder_trunk_grads(act, params, gd10, out=None if trunk_out is None else trunk_out[a], want_gzin=want_gzin)
            r = {"loss": cell.sum() / (float(B) * float(D))}
            r.update({nm: (tg[2 * k], tg[2 * k + 1]) for k, nm in enumerate(N.TRUNK_LAYERS)})
            r.update({names[h]: g[h] for h in N.ZINB_HEADS if h in g})
            r["d10"] = gd10
            if gzin is not None:
                r["c"], r["s"] = gzin[:, :Cc], gzin[:, Cc:]
            res.append(r)
        self._ctx = None
        return res

    # ------------------------------------------------------------------ training under the ZINB objective
    _ZINB_PR = (("fc11_p", "weight"), ("fc11_p", "bias"), ("fc11_r", "weight"), ("fc11_r", "bias"))

    def _heads_packed(self) -> bool:
        flat = getattr(self, "_heads_flat", None)
        if flat is None:
            return False
        lay, A = self._heads_layout, self.n_arm
        w0, bl = self.fc11_p[0].weight, self.fc11_r[A - 1].bias
        return (w0.device == flat.device and w0.data_ptr() == flat.data_ptr()
                and bl.data_ptr() == flat.data_ptr() + 4 * (int(lay.per_arm) * (A - 1) + int(lay.offset[3])))

    def _pack_heads(self):
        """The p and r heads in one flat buffer (mmvae_zinb_head_layout), as ``_pack`` keeps the 28 tensors: every
        ``fc11_p`` / ``fc11_r`` parameter becomes a view of it, so the modules hold the step's result at every moment (the
        write-back points of ``fit_zinb_heads`` -- before a ``score_zinb``, on exit -- are trivially met).  Values are kept."""
        dev = self.fc1[0].weight.device
        lay = N.zinb_head_layout(self._dims(2))
        A, per_arm = self.n_arm, int(lay.per_arm)
        flat = torch.zeros(A * per_arm, dtype=torch.float32, device=dev)
        with torch.no_grad():
            for a in range(A):
                for j, (name, kind) in enumerate(self._ZINB_PR):
                    p = getattr(getattr(self, name)[a], kind)
                    o = a * per_arm + int(lay.offset[j])
                    v = flat[o: o + p.numel()].view(p.shape)
                    v.copy_(p.data.to(torch.float32))
                    p.data = v
        self._heads_flat, self._heads_grad, self._heads_layout = flat, torch.zeros_like(flat), lay

    def zinb_heads_flat(self):
        """(the flat buffer of ``fc11_p`` / ``fc11_r``, its gradient buffer): [A, 2 (D H + D)] each, laid out per arm
        ``fc11_p.weight | fc11_p.bias | fc11_r.weight | fc11_r.bias`` (mmvae_zinb_head_layout)."""
        self._need_zinb("zinb_heads_flat()")
        if not self._heads_packed():
            self._pack_heads()
        return self._heads_flat.view(self.n_arm, -1), self._heads_grad.view(self.n_arm, -1)

    def _zinb_head_params(self):
        """(arm, index in the head layout, the ``nn.Parameter``, its offset in an arm's row of ``zinb_heads_flat``) for the
        four head tensors of every arm."""
        self.zinb_heads_flat()
        lay = self._heads_layout
        return [(a, j, getattr(getattr(self, name)[a], kind), int(lay.offset[j]))
                for a in range(self.n_arm) for j, (name, kind) in enumerate(self._ZINB_PR)]

    def zinb_step_state(self):
        """A fresh optimiser state of ``zinb_train_step``: Adam's step count and the two moment pairs, all zero."""
        self._need_zinb("zinb_step_state()")
        flat = self.flat_parameters()
        hp, _ = self.zinb_heads_flat()
        z = torch.zeros_like
        return {"kind": "zinb_step", "step": 0, "exp_avg": z(flat), "exp_avg_sq": z(flat), "hp_exp_avg": z(hp), "hp_exp_avg_sq": z(hp)}

    def _check_zinb_step_state(self, what, state):
        """ValueError for a state that is not ``zinb_step_state``'s of this model (``fit_zinb_heads`` / ``fit_zinb_decoder``
        return another); reads shapes only."""
        lay, A = N.param_layout(self._dims(2)), self.n_arm
        n, hn = A * int(lay.per_arm), 2 * (self.input_dim * self.fc_dim + self.input_dim)
        ok = (isinstance(state, dict) and state.get("kind") == "zinb_step"
              and all(k in state for k in ("step", "exp_avg", "exp_avg_sq", "hp_exp_avg", "hp_exp_avg_sq"))
              and all(int(state[k].numel()) == n for k in ("exp_avg", "exp_avg_sq"))
              and all(tuple(state[k].shape) == (A, hn) for k in ("hp_exp_avg", "hp_exp_avg_sq")))
        if not ok:
            raise ValueError(f"{what}: state is not a ZINB training state of this model (zinb_step_state(): step and the moments "
                             f"of the {n} flat parameters and of the [{A}, {hn}] p / r heads); the states of fit_zinb_heads / "
                             "fit_zinb_decoder hold other moments")

    @torch.no_grad()
    def zinb_train_step(self, x, temp, state=None, do_adam=True, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        """One training step under the ZINB objective in one C-ABI call (mmvae_zinb_train_step): the training-mode forward
        (input and state dropout, batch-statistic BatchNorm, Gumbel noise, reparameterised ``s``), the reference's ``loss()``
        with its reconstruction term replaced by ``zinb_loss`` (eps 1e-6), the backward through decoder, latent block and
        encoder, and Adam (L2 ``weight_decay``, as ``torch.optim.Adam``) on all parameters, ``fc11_p`` and ``fc11_r`` included.
        Consumes one noise draw and one ``_step_id``, as ``fused_train_step``.  Returns the device loss vector
        (MMVAE_LOSS_*; ``rec[a]`` is the ZINB loss of arm a, ``ll[a]`` the reference's MSE-based expression); no host sync.

        ``state``: ``zinb_step_state()``'s dict, updated in place (None: one the model keeps).  ``do_adam=False`` leaves the
        gradients in ``flat_grad()`` and ``zinb_heads_flat()[1]`` and touches no state.  Needs ``model.train()`` and a model
        built with ``loss_mode="ZINB"`` (RuntimeError otherwise); NotImplementedError for ``gemm_dtype="bf16"``.  Every
        refusal comes before any device work, and consumes no noise."""
        what = "zinb_train_step()"
        self._need_zinb(what)
        if not self.training:
            raise RuntimeError(f"{what} needs model.train()")
        if self.gemm_dtype == "bf16":
            raise NotImplementedError(f"{what}: gemm_dtype='bf16' is not offered under the ZINB objective (bf16 heads are not built)")
        if self.ref_prior:
            raise NotImplementedError("ref_prior is rejected by the reference loss (nn_model.py:578)")
        if do_adam:
            if (not (0.0 <= lr < float("inf")) or not (0.0 <= weight_decay < float("inf")) or not eps >= 0.0 or len(betas) != 2
                    or not all(0.0 <= b < 1.0 for b in betas)):
                raise ValueError(f"{what}: lr = {lr}, betas = {betas}, eps = {eps}, weight_decay = {weight_decay}")
            if state is not None:
                self._check_zinb_step_state(what, state)
        xt, xs = self._prep_x(x)
        if xt.device.type != "cuda":
            raise N.NativeError(f"{what} needs GPU tensors: the model runs only on the HIP engine")
        assert xt.shape[-1] == self.input_dim
        eng = self._ensure(xt.shape[-2])
        hp, hg = self.zinb_heads_flat()
        if do_adam and state is None:
            if getattr(self, "_zinb_state", None) is None:
                self._zinb_state = self.zinb_step_state()
            state = self._zinb_state
        hyper = self._hyper(temp, False)
        noise = self._next_noise()
        self._step_id += 1
        self._ctx = None
        if do_adam:
            state["step"] = int(state["step"]) + 1
            return eng.zinb_train_step(hyper, noise, self._flat, hp, self._bn_flat, self._nbt, xt, xs, self._flat_grad, hg, True,
                                       state["exp_avg"], state["exp_avg_sq"], state["hp_exp_avg"], state["hp_exp_avg_sq"],
                                       state["step"], float(lr), float(betas[0]), float(betas[1]), float(eps), float(weight_decay),
                                       False)
        return eng.zinb_train_step(hyper, noise, self._flat, hp, self._bn_flat, self._nbt, xt, xs, self._flat_grad, hg, False,
                                   None, None, None, None, 1, 0.0)

    @torch.no_grad()
    def zinb_objective(self, x, temp, mask=None):
        """The training objective of ``zinb_train_step`` evaluated in eval mode: ``_forward(x, temp, True, mask, False)``, then
        mmvae_zinb_objective on the workspace it left.  Returns the reference's 9-tuple as ``loss()`` does, with ``rec`` the
        per-arm ZINB loss: ``(total, rec [A], loss_joint, c_entropy, c_distance, c_l2, [KL_a], [], [ll_a])``, 0-dim device
        tensors.  ``loss()`` itself stays refused under ZINB.  Needs model.eval()."""
        vals = self._zinb_objective_vec(x, temp, mask)
        A = self.n_arm
        if A == 1:
            raise ZeroDivisionError("division by zero")          # the reference divides by len([]) here (nn_model.py:592-594)
        rec = vals[N.LOSS_REC0: N.LOSS_REC0 + A]
        kl = vals[N.LOSS_REC0 + A: N.LOSS_REC0 + 2 * A]
        ll = vals[N.LOSS_REC0 + 2 * A: N.LOSS_REC0 + 3 * A]
        return (vals[N.LOSS_TOTAL], rec.clone(), vals[N.LOSS_JOINT], vals[N.LOSS_CENT], vals[N.LOSS_CDIST], vals[N.LOSS_CL2],
                list(kl.unbind(0)), [], list(ll.unbind(0)))

    def _zinb_objective_vec(self, x, temp, mask):
        """``zinb_objective``'s loss vector (MMVAE_LOSS_*), a fresh device tensor."""
        self._need_zinb("zinb_objective()")
        if self.training:
            raise RuntimeError("zinb_objective() needs model.eval()")
        self._forward(x, temp, True, mask, False)
        vec = self._zinb_objective_here()
        self._ctx = None
        return vec

    def _zinb_objective_here(self):
        """mmvae_zinb_objective on the workspace the preceding eval ``_forward`` left (``cpl_mixVAE.eval_model`` keeps that
        forward's outputs and so runs it once per batch): the loss vector, a fresh device tensor."""
        hp, _ = self.zinb_heads_flat()
        return self._engine.zinb_objective(self._ctx["hyper"], self._flat, hp, self._ctx["x"], self._ctx["x_arm_stride"]).clone()

    @torch.no_grad()
    def zinb_sample_batch(self, x, seed, temp=1.0, mask=None, offset=0, cell0=0, log1p=False, arms=None):
        """One ZINB draw per (arm, cell, gene) of the batch ``x`` (as ``forward`` takes it) at the model's own codes: an eval
        forward, then mmvae_zinb_sample per arm of ``arms`` (all by default) on the forward workspace's d10, as ``zinb_nll``
        scores it.  Returns float32 [len(arms), B, D] on the device.  Every arm uses the same key, so two arms differ by
        their heads alone.  Needs model.eval()."""
        self._need_zinb("zinb_sample_batch()")
        if self.training:
            raise RuntimeError("zinb_sample_batch() needs model.eval()")
        self._forward(x, temp, True, mask, False)
        d10 = self._engine.ws_view("d10", self.fc_dim)
        arms = list(range(self.n_arm)) if arms is None else [int(a) for a in arms]
        out = torch.stack([N.zinb_sample(d10[a], *self._zinb_layers(a), seed=seed, offset=offset, cell0=cell0, log1p=log1p)
                           for a in arms])
        self._ctx = None
        return out

    def zinb_distribution(self, x_rec, x_p, x_r, eps=1e-6):
        """The likelihood of ``zinb_loss`` as a distribution object: with r = x_rec + eps and p = (1 - eps)(x_p + eps) the NB has
        ``theta = r`` and ``mu = r p / (1 - p)``, and z = (1 - eps)(x_r + eps) is the zero-inflation probability.  The three are
        formed in fp64 from the heads (``decoder_zinb``'s device tensors) and rounded once to float32.  Returns a
        ``utils.distributions.ZeroInflatedNegativeBinomial`` (``mean``, ``log_prob``, ``sample``)."""
        from .utils.distributions import ZeroInflatedNegativeBinomial
        self._need_zinb("zinb_distribution()")
        N._need_cuda("zinb_distribution()", x_rec, x_p, x_r)
        r = x_rec.detach().double() + eps
        p = (1.0 - eps) * (x_p.detach().double() + eps)
        z = (1.0 - eps) * (x_r.detach().double() + eps)
        return ZeroInflatedNegativeBinomial(mu=(r * p / (1.0 - p)).float(), theta=r.float(), zi_probs=z.float())

    @torch.no_grad()
    def sample_zinb(self, c, s, arm, seed, offset=0, cell0=0, log1p=False):
        """One count per (cell, gene) drawn from the model's ZINB likelihood at the codes c [N, C], s [N, S] of arm ``arm``: the
        decode runs, then mmvae_zinb_sample forms the three heads of every tile from the decode workspace's d10 and draws in
        the epilogue -- the N x D heads are never written.  Draws are keyed by (seed, offset, (cell0 + row) D + gene): batches
        with ``cell0`` advancing equal one call.  Returns float32 [N, D] on the device, ``log1p`` of the counts on request (the
        space the model's input lives in).  Refusals: those of ``decoder_zinb``."""
        self._need_zinb("sample_zinb()")
        _, eng = self._decode_run(c, s, arm)
        return N.zinb_sample(eng.ws_view("d10", self.fc_dim)[0], *self._zinb_layers(int(arm)), seed=seed, offset=offset,
                             cell0=cell0, log1p=log1p)

    def set_explicit_state_noise(self, u):
        """Test hook of ``state_changes`` (as ``set_explicit_noise`` is of ``forward``): u float32 [A, n_samp, B] on the
        device, the U(0,1) draws of the reference's ``torch.rand_like`` (nn_model.py:427) in its order -- arm, sample,
        cell -- used by every following call; None returns to the model's Philox stream."""
        self._explicit_state_noise = u

    @torch.no_grad()
    def state_changes(self, x, d_s, temp, n_samp=100):
        """nn_model.py:370-411, the continuous traversal of state dimension ``d_s``: returns (recon_x, state_smp_sorted)
        as CPU float32 tensors, recon_x [A, n_samp, D] for one cell and state_smp_sorted all zeros [A, n_samp], with the
        samples reordered by ``torch.zeros(n_samp).sort()``'s indices as the reference does.  ``temp`` has no effect
        (the reference's noise-free hard sample).  Extension: a batch of B > 1 cells (the reference raises) gives
        recon_x [A, n_samp, B, D].  Needs model.eval(), as the reference's BatchNorm does."""
        if self.training:
            raise RuntimeError("state_changes() needs model.eval(): the reference traverses in eval mode "
                               "(BatchNorm with one cell)")
        xt = x if x.dim() == 2 else x.reshape(-1, self.input_dim)
        if xt.device.type != "cuda":
            raise N.NativeError("mixVAE_model.state_changes needs GPU tensors: the model runs only on the HIP engine")
        xt = xt.contiguous().float()
        B, n_samp, d_s = xt.shape[0], int(n_samp), int(d_s)
        if not (0 <= d_s < self.state_dim):
            raise IndexError(f"d_s {d_s} outside [0, {self.state_dim})")
        if n_samp < 1:
            raise ValueError("n_samp must be >= 1")
        eng = self._dec_engine(self.n_arm, B, n_samp)
        if self._explicit_state_noise is not None:
            u = self._explicit_state_noise.contiguous().float()
            assert tuple(u.shape) == (self.n_arm, n_samp, B) and u.device == xt.device
            noise = N.make_noise({"u_state": u})
        else:
            if self._noise_seed is None:
                self._noise_seed = int(torch.initial_seed()) & 0xFFFFFFFFFFFFFFFF
            self._noise_offset += 1
            noise = N.make_noise(None, self._noise_seed, self._noise_offset)
        out = torch.empty(self.n_arm, n_samp, B, self.input_dim, dtype=torch.float32, device=xt.device)
        eng.state_changes(self._hyper(temp, True), noise, self._flat, self._bn_flat, xt, d_s, out)
        recon = out.cpu()
        state_smp_sorted = torch.zeros(self.n_arm, n_samp)
        for arm in range(self.n_arm):
            # the reference's reordering (nn_model.py:408-409): the sort indices of a zero vector, not the identity for
            # every n_samp
            _, sort_idx = torch.zeros(n_samp).sort()
            recon[arm] = recon[arm, sort_idx]
        return (recon[:, :, 0, :].contiguous() if B == 1 else recon), state_smp_sorted

    # ------------------------------------------------------------------ fused step (trainer path)
    def prune_apply(self, mask, opt=None, params=True, grads=True):
        """Exact zeros at the parameter positions of the categories ``mask`` (as ``forward(mask=)`` takes it: the KEPT
        categories) does not keep, in every arm: ``fcc.weight[k, :]``, ``fcc.bias[k]``, ``fc_mu.weight[:, L + k]``,
        ``fc_sigma.weight[:, L + k]``, ``fc6.weight[:, k]`` -- the five masks of the reference's pruning phase
        (cpl_mixvae.py:1124-1128, applied by ``prune.custom_from_mask``, :1153-1161).  ``params`` / ``grads``: the flat
        parameter / gradient buffer; ``opt`` (a ``FusedAdam`` of this model): its two moment buffers too.  One launch
        (mmvae_prune_apply) on the current stream; a mask that keeps every category does nothing."""
        self._prune_words(self._mask_words(mask), opt, params, grads)

    def _prune_words(self, words, opt, params, grads):
        if words is None:
            return
        if not self._is_packed():
            self._pack()
        m = v = None
        if opt is not None:
            opt._bind(self)
            m, v = opt.exp_avg, opt.exp_avg_sq
        if self._prune_dims is None:
            self._prune_dims = self._dims(2)                  # (the call reads A, L, C, S; kept: this is on the per-step path)
        with torch.cuda.device(self._flat.device):
            N.prune_apply(self._prune_dims, words, self._flat if params else None, self._flat_grad if grads else None, m, v,
                          n=self._flat.numel())

    def fused_train_step(self, x, temp, opt=None, do_adam=True, mask=None):
        """forward + loss + backward (+ Adam) in one C-ABI call: cpl_mixvae.py:434-463.
        Returns the device loss vector (see include/mmvae.h MMVAE_LOSS_*); no host sync.

        ``mask`` (the pruning phase, cpl_mixvae.py:1163-1394): the kept categories, as ``forward(mask=)`` takes them; the
        step runs under ``mmvae_hyper.cat_mask`` and the parameters of the other categories are held at zero
        (``prune_apply``).  With ``do_adam`` the parameters, gradients and both Adam moments are zeroed there behind the
        step, so the effective weights are torch's ``weight_orig * mask`` after every step; the moments of pruned entries
        are held at 0, where torch keeps decaying remnants that never reach an effective weight.  Without ``do_adam`` the
        gradients are zeroed there; the caller steps its optimizer and then calls ``prune_apply(mask, grads=False)``."""
        self._refuse_zinb_training()
        words = self._mask_words(mask)
        xt, xs = self._prep_x(x)
        eng = self._ensure(xt.shape[-2])
        hyper = self._hyper(temp, False)
        if words is not None:
            for i in range(4):
                hyper.cat_mask[i] = words[i]
        noise = self._next_noise()
        self._step_id += 1
        self._ctx = None
        if do_adam:
            opt._bind(self)
            opt.step_count += 1
            g = opt.param_groups[0]
            buf = eng.train_step(hyper, noise, self._flat, self._bn_flat, self._nbt, xt, xs, self._flat_grad, True,
                                 opt.exp_avg, opt.exp_avg_sq, opt.step_count, g["lr"], g["betas"][0], g["betas"][1],
                                 g["eps"], g["weight_decay"], opt.decoupled)
        else:
            buf = eng.train_step(hyper, noise, self._flat, self._bn_flat, self._nbt, xt, xs, self._flat_grad, False,
                                 None, None, 1, 0.0)
        if words is not None:
            # the step has joined its side stream (the fc11 reduction and update) before it returned: stream order suffices
            self._prune_words(words, opt if do_adam else None, bool(do_adam), True)
        return buf


    def fused_train_step_rows(self, data, rows, temp, opt=None, do_adam=True, data16=None, mask=None):
        """``fused_train_step`` on the batch ``data[rows]`` without materialising it (``x.expand`` over the arms): the step
        reads the cells x genes matrix through a row map (mmvae_train_step_rows; bit-identical to gather + step).  Raises
        ``NotImplementedError`` where the library does not offer it -- engines other than fp32x3, no input dropout, a
        matrix beyond 4 GB --: gather the batch and call ``fused_train_step`` then.  ``data16`` (``gemm_dtype == "bf16"``
        only): the matrix's bf16 copy (``_native.to_bf16``, ``DeviceLoader.data_bf16()``): bf16 storage, see DESIGN.md section 13.
        ``mask``: as ``fused_train_step`` takes it (the pruning phase), with the same zeroing behind the step."""
        self._refuse_zinb_training()
        words = self._mask_words(mask)
        if data.device.type != "cuda" or data.dtype != torch.float32 or data.shape[1] != self.input_dim:
            raise N.NativeError("fused_train_step_rows needs the float32 cells x genes matrix on the GPU")
        rows = rows.to(device=data.device, dtype=torch.int64).contiguous()
        eng = self._ensure(int(rows.numel()))
        hyper = self._hyper(temp, False)
        if words is not None:
            for i in range(4):
                hyper.cat_mask[i] = words[i]
        noise = self._next_noise()
        try:
            if do_adam:
                opt._bind(self)
                g = opt.param_groups[0]
                buf = eng.train_step_rows(hyper, noise, self._flat, self._bn_flat, self._nbt, data, rows, self._flat_grad, True,
                                          opt.exp_avg, opt.exp_avg_sq, opt.step_count + 1, g["lr"], g["betas"][0],
                                          g["betas"][1], g["eps"], g["weight_decay"], opt.decoupled, data16=data16)
                opt.step_count += 1
            else:
                buf = eng.train_step_rows(hyper, noise, self._flat, self._bn_flat, self._nbt, data, rows, self._flat_grad, False,
                                          None, None, 1, 0.0, data16=data16)
        except NotImplementedError:
            if self._explicit_noise is None:
                self._noise_offset -= 1            # the refused call consumed nothing
            elif isinstance(self._explicit_noise, list):
                self._explicit_noise.insert(0, self._noise_keep)
            raise
        self._step_id += 1
        self._ctx = None
        if words is not None:
            self._prune_words(words, opt if do_adam else None, bool(do_adam), True)
        return buf


def zinb_loss(rec_x, x_p, x_r, X, eps=1e-6):
    """nn_model.py:642-676: the mean over all elements of the ZINB term of ``X`` (the log1p matrix) under the heads ``rec_x``,
    ``x_p``, ``x_r`` -- device tensors of one shape [..., D]; returns a 0-dim float32 device tensor: the fp64 sum of
    mmvae_zinb_terms' per-cell sums divided by the element count.  No backward: an input that requires grad raises
    NotImplementedError."""
    ts = (rec_x, x_p, x_r, X)
    if any(t.requires_grad for t in ts):
        raise NotImplementedError("zinb_loss has no backward: training under loss_mode='ZINB' is not built; detach the inputs")
    if not all(t.shape == X.shape for t in ts) or X.dim() < 1 or X.numel() == 0:
        raise ValueError("zinb_loss: rec_x, x_p, x_r and X must have one non-empty shape")
    if any(t.device.type != "cuda" for t in ts):
        raise N.NativeError("zinb_loss needs GPU tensors: it runs only on the HIP engine")
    flat = [t.float().reshape(-1, X.shape[-1]) for t in ts]
    cell, _, _ = N.zinb_terms(*flat, eps=eps)
    return (cell.sum() / X.numel()).to(torch.float32)


def zinb_loss_grad(rec_x, x_p, x_r, X, eps=1e-6):
    """The gradient of ``zinb_loss``'s value with respect to ``rec_x``, ``x_p`` and ``x_r`` -- device tensors of one shape
    [..., D] as ``zinb_loss`` takes them; returns three float32 device tensors of that shape (mmvae_zinb_terms_grad: the
    term's derivative in fp64, times 1 / numel, rounded once).  ``rec_x`` is taken as given: no relu stands in front of it
    here, as none does in ``zinb_loss``.  ``zinb_loss`` itself stays without a backward."""
    ts = (rec_x, x_p, x_r, X)
    if not all(t.shape == X.shape for t in ts) or X.dim() < 1 or X.numel() == 0:
        raise ValueError("zinb_loss_grad: rec_x, x_p, x_r and X must have one non-empty shape")
    if any(t.device.type != "cuda" for t in ts):
        raise N.NativeError("zinb_loss_grad needs GPU tensors: it runs only on the HIP engine")
    flat = [t.detach().float().reshape(-1, X.shape[-1]) for t in ts]
    return tuple(g.reshape(X.shape) for g in N.zinb_terms_grad(*flat, eps=eps, scale=1.0 / X.numel()))


def mk_vae(C, state_dim, input_dim, device, eps=1e-8, fc_dim=100, latent_dim=10, x_drop=0.5, s_drop=0.2, lr=0.001,
           lam=1, lam_pc=1, A=2, tau=0.005, beta=1.0, hard=False, variational=True, ref_prior=False, momentum=0.01,
           mode="MSE") -> nn.Module:
    """nn_model.py:679-721."""
    return mixVAE_model(input_dim=input_dim, fc_dim=fc_dim, n_categories=C, state_dim=state_dim, lowD_dim=latent_dim,
                        x_drop=x_drop, s_drop=s_drop, n_arm=A, lam=lam, lam_pc=lam_pc, tau=tau, beta=beta, hard=hard,
                        variational=variational, device=device, eps=eps, ref_prior=ref_prior, momentum=momentum,
                        loss_mode=mode).to(device)

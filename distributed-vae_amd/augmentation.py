"""Drop-in for the augmenter the reference trainer runs in front of every train step.

``Augmenter_smartseq`` mirrors ``mmidas/augmentation/udagan.py:217-329`` (constructor arguments, sub-module names and
therefore ``state_dict`` keys, ``forward(x, batched, scale)`` returning ``(s, x_aug)``); ``mk_augmenter`` mirrors
``mmidas/cpl_mixvae.py:128-149``.  The eval-mode forward -- the one the trainer uses (``self.netA =
netA.to(self.device).eval()``, cpl_mixvae.py:184): Dropout is the identity and every BatchNorm1d normalises with its running
statistics -- runs in ``csrc/augment.hip``.  Training (``csrc/augtrain.hip``): the non-batched training-mode forward,
``train_step`` and ``train_augmenter``, the reference's ``mmidas/augmentation/train.py`` loop for the augmenter alone.
There is no CPU / PyTorch fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch
from torch import nn

from . import _native as N


class Augmenter_smartseq(nn.Module):
    def __init__(self, noise_dim, latent_dim, input_dim=5000, n_dim=500, p_drop=0.5):
        super().__init__()
        moment = 0.01
        self.noise_dim = noise_dim
        self.dp = nn.Dropout(p_drop)
        self.noise = nn.Linear(noise_dim, noise_dim, bias=False)
        self.bnz = nn.BatchNorm1d(noise_dim)
        n1, n5 = input_dim // 5, n_dim // 5
        bn = lambda n: nn.BatchNorm1d(num_features=n, eps=1e-10, momentum=moment, affine=False)  # noqa: E731
        # (name, in, out) in the reference's construction order (the order fixes the RNG stream of the initialisation)
        enc = [("fc1", input_dim, n1), ("fc2", n1, n1), ("fc3", n1, n_dim), ("fc4", n_dim, n_dim),
               ("fc5", n_dim + noise_dim, n5)]
        dec = [("fc6", latent_dim, n5), ("fc7", n5, n_dim), ("fc8", n_dim, n_dim), ("fc9", n_dim, n1), ("fc10", n1, n1)]
        for name, i, o in enc:
            setattr(self, name, nn.Linear(i, o))
            setattr(self, "batch_" + name, bn(o))
        self.fc_mu = nn.Linear(n5, latent_dim)
        self.fc_sigma = nn.Linear(n5, latent_dim)
        self.batch_fc_mu = bn(latent_dim)
        for name, i, o in dec:
            setattr(self, name, nn.Linear(i, o))
            setattr(self, "batch_" + name, bn(o))
        self.fc11 = nn.Linear(n1, input_dim)
        self._dims = (input_dim, n1, n_dim, n5, latent_dim, noise_dim)
        self.gemm_dtype = "fp32"          # "bf16": bf16 operands in the ten large Linear layers (fp32 accumulation)
        self._packed: Optional[torch.Tensor] = None
        self._ws: Optional[torch.Tensor] = None
        self._explicit = None
        self._explicit_mask = None
        self._flat = None                 # training: the flat buffers the parameters and running statistics are views of
        self._tws: Optional[torch.Tensor] = None
        self._adam = None

    # ------------------------------------------------------------------ packed weights
    def _apply(self, fn, *a, **k):
        self._packed = None
        return super()._apply(fn, *a, **k)

    def load_state_dict(self, *a, **k):
        self._packed = None
        return super().load_state_dict(*a, **k)

    def repack(self):
        """Call after modifying parameters or running statistics in place (the packed copy is otherwise kept)."""
        self._packed = None

    def _exec(self) -> N.Exec:
        if getattr(self, "_ex", None) is None:
            self._ex = N.exec_from_env()      # MMVAE_AUG_TILE (A/B timing); the library itself reads no environment
        return self._ex

    def _aug_dims(self, A, B) -> N.AugDims:
        D, n1, n3, n5, z, nz = self._dims
        return N.AugDims(A, B, D, n1, n3, n5, z, nz)

    def _pack(self, dims: N.AugDims):
        dev = self.fc1.weight.device
        t = N.AugTensors()
        keep = []

        def ptr(x):
            x = x.detach().contiguous().float()
            keep.append(x)
            return x.data_ptr()
        for i in range(11):
            lin = getattr(self, f"fc{i + 1}")
            t.w[i], t.b[i] = ptr(lin.weight), ptr(lin.bias)
        for i in range(10):
            b = getattr(self, f"batch_fc{i + 1}")
            t.bn_mean[i], t.bn_var[i] = ptr(b.running_mean), ptr(b.running_var)
        t.w_mu, t.b_mu = ptr(self.fc_mu.weight), ptr(self.fc_mu.bias)
        t.w_sigma, t.b_sigma = ptr(self.fc_sigma.weight), ptr(self.fc_sigma.bias)
        t.bn_mu_mean, t.bn_mu_var = ptr(self.batch_fc_mu.running_mean), ptr(self.batch_fc_mu.running_var)
        t.noise_w = ptr(self.noise.weight)
        t.bnz_weight, t.bnz_bias = ptr(self.bnz.weight), ptr(self.bnz.bias)
        t.bnz_mean, t.bnz_var = ptr(self.bnz.running_mean), ptr(self.bnz.running_var)
        n = int(N.lib().mmvae_aug_packed_floats(C.byref(dims)))
        if n == 0:
            N.check(-2, "mmvae_aug_packed_floats")
        packed = torch.empty(n, dtype=torch.float32, device=dev)
        N.check(N.lib().mmvae_aug_pack(C.byref(dims), C.byref(t), N._ptr(packed), N._stream(dev)), "mmvae_aug_pack")
        torch.cuda.current_stream(dev).synchronize()   # `keep` may be freed once the pack kernels have run
        self._packed = packed

    # ------------------------------------------------------------------ noise control (parity hook)
    def set_explicit_noise(self, z0: Optional[torch.Tensor], eps: Optional[torch.Tensor]):
        """z0 [A,B,noise_dim] and eps [A,B,latent_dim] standard-normal draws used by the next forward passes instead of
        torch.randn; (None, None) returns to torch.randn on the device."""
        self._explicit = None if z0 is None else (z0, eps)

    def set_explicit_dropout(self, mask: Optional[torch.Tensor]):
        """uint8 keep-mask of the input dropout used by the next training-mode forwards / steps instead of one drawn by torch
        on the device: [B, D], or [2, B, D] for a step with its statistics pass (entry 0: the statistics pass, as the explicit
        noise's [2, B, .]); None returns to torch."""
        self._explicit_mask = mask

    # ------------------------------------------------------------------ training (csrc/augtrain.hip)
    def _flat_ok(self, dev) -> bool:
        f = self._flat
        if f is None or f["params"].device != dev:
            return False
        base, lay = f["params"].data_ptr(), f["lay"]
        if not all(p.data_ptr() == base + 4 * o and p.dtype == torch.float32 for p, o in zip(self.parameters(), f["offs"])):
            return False
        rbase, nbase = f["running"].data_ptr(), f["nbt"].data_ptr()
        for i, name in enumerate(N.AUG_BATCHNORMS):        # the running statistics and counters are views too
            b = getattr(self, name)
            if (b.running_mean.data_ptr() != rbase + 4 * lay.rm_off[i] or b.running_var.data_ptr() != rbase + 4 * lay.rv_off[i]
                    or b.num_batches_tracked.data_ptr() != nbase + 8 * i or b.running_mean.dtype != torch.float32):
                return False
        return True

    def _flatten(self, dev):
        """Move parameters, running statistics and num_batches_tracked into flat device buffers (the layout of
        mmvae_aug_param_layout) and make the module's tensors views of them: the device step and Adam then act on what
        ``state_dict()`` and the eval forward (after ``repack()``) read."""
        dims = self._aug_dims(1, 2)
        lay = N.AugTrainLayout()
        N.check(N.lib().mmvae_aug_param_layout(C.byref(dims), C.byref(lay)), "mmvae_aug_param_layout")
        params = torch.zeros(lay.total, dtype=torch.float32, device=dev)
        grads = torch.zeros(lay.total, dtype=torch.float32, device=dev)
        running = torch.zeros(lay.run_total, dtype=torch.float32, device=dev)
        nbt = torch.zeros(12, dtype=torch.int64, device=dev)
        where = {}
        for i, name in enumerate(N.AUG_LINEARS):
            where[name + ".weight"] = lay.w_off[i]
            if lay.b_off[i] >= 0:
                where[name + ".bias"] = lay.b_off[i]
        where["bnz.weight"], where["bnz.bias"] = lay.bnz_w_off, lay.bnz_b_off
        offs, gviews = [], []
        with torch.no_grad():
            for k, p in self.named_parameters():
                o = where[k]
                v = params[o:o + p.numel()].view(p.shape)
                v.copy_(p.detach().to(dev, torch.float32))
                p.data = v
                p.grad = None
                offs.append(o)
                gviews.append(grads[o:o + p.numel()].view(p.shape))
            for i, name in enumerate(N.AUG_BATCHNORMS):
                b = getattr(self, name)
                n = b.num_features
                for attr, o in (("running_mean", lay.rm_off[i]), ("running_var", lay.rv_off[i])):
                    v = running[o:o + n]
                    v.copy_(getattr(b, attr).detach().to(dev, torch.float32))
                    getattr(b, attr).data = v
                nbt[i] = int(b.num_batches_tracked)
                b.num_batches_tracked.data = nbt[i]
        self._flat = {"params": params, "grads": grads, "running": running, "nbt": nbt, "offs": offs, "gviews": gviews,
                      "lay": lay, "keep": None}
        self._packed = None

    def _train_ready(self, x, what):
        if x.device.type != "cuda":
            raise N.NativeError(f"{what} needs GPU tensors: it runs only on the HIP engine")
        D = self._dims[0]
        if x.dim() != 2 or x.shape[-1] != D:
            raise ValueError(f"{what}: x must be [B, {D}], got {tuple(x.shape)}")
        if x.shape[0] < 2:
            raise ValueError(f"{what}: expected more than 1 value per channel when training, got input size {tuple(x.shape)}")
        if self.gemm_dtype != "fp32":
            raise NotImplementedError(f"{what}: gemm_dtype={self.gemm_dtype!r} is not offered in training (fp32 only)")
        xt = x.contiguous().float()
        dims = self._aug_dims(1, xt.shape[0])
        need = int(N.lib().mmvae_aug_train_workspace_bytes(C.byref(dims)))
        if need == 0:
            N.check(N.lib().mmvae_aug_param_layout(C.byref(dims), C.byref(N.AugTrainLayout())), what)
        if not self._flat_ok(xt.device):
            self._flatten(xt.device)
        if self._tws is None or self._tws.numel() * 4 < need or self._tws.device != xt.device:
            self._tws = None
            self._tws = torch.empty(need // 4, dtype=torch.float32, device=xt.device)
        self._packed = None           # the eval forward's packed copy is stale once parameters or statistics move
        return xt, dims

    def _train_noise(self, n_pass, B, dev):
        """(mask, z0, eps) for each of n_pass forwards, the statistics pass first: the explicit ones, or per pass a keep-mask
        from ``torch.rand >= p`` and ``torch.randn`` draws on the device, in that order."""
        D, _, _, _, Z, NZ = self._dims
        p = float(self.dp.p)

        def given(t, shape, dtype):
            t = t.to(dev)
            if t.dim() == len(shape):
                t = t[None]
            if tuple(t.shape) != (n_pass,) + shape:
                raise ValueError(f"explicit noise of shape {tuple(t.shape)}; this call needs {(n_pass,) + shape}")
            return t.to(dtype).contiguous()
        z0 = eps = mask = None
        if self._explicit is not None:
            z0, eps = given(self._explicit[0], (B, NZ), torch.float32), given(self._explicit[1], (B, Z), torch.float32)
        if self._explicit_mask is not None:
            mask = given(self._explicit_mask, (B, D), torch.uint8)
        out = []
        for i in range(n_pass):
            m = mask[i] if mask is not None else (torch.rand(B, D, device=dev) >= p).to(torch.uint8)
            a = z0[i] if z0 is not None else torch.randn(B, NZ, device=dev)
            b = eps[i] if eps is not None else torch.randn(B, Z, device=dev)
            out.append((m, a, b))
        return out

    @torch.no_grad()
    def _train_forward(self, x, scale):
        xt, dims = self._train_ready(x, "Augmenter_smartseq.forward (training)")
        f, B = self._flat, xt.shape[0]
        (mask, z0, eps), = self._train_noise(1, B, xt.device)
        s = torch.empty(B, self._dims[4], dtype=torch.float32, device=xt.device)
        out = torch.empty(B, self._dims[0], dtype=torch.float32, device=xt.device)
        N.check(N.lib().mmvae_aug_train_forward(C.byref(dims), N._ptr(f["params"]), N._ptr(f["running"]), N._ptr(f["nbt"]),
                                                N._ptr(xt), N._ptr(mask), float(self.dp.p), N._ptr(z0), N._ptr(eps),
                                                float(scale), N._ptr(self._tws), self._tws.numel() * 4, N._ptr(s), N._ptr(out),
                                                C.byref(self._exec()), N._stream(xt.device)), "mmvae_aug_train_forward")
        f["keep"] = (xt, mask, z0, eps)
        return s, out

    def flat_grad(self) -> torch.Tensor:
        """The flat gradient buffer the last ``train_step`` wrote (parameters() order, zero alignment gaps)."""
        if self._flat is None:
            raise RuntimeError("flat_grad(): no training step or training-mode forward has run")
        return self._flat["grads"]

    def bind_grads(self):
        """Point every parameter's ``.grad`` at its view of ``flat_grad()``: a stock ``torch.optim`` optimizer can then follow
        a ``train_step(do_adam=False)``."""
        self.flat_grad()
        for p, g in zip(self.parameters(), self._flat["gviews"]):
            p.grad = g

    def train_state(self, device=None):
        """A fresh Adam state for ``train_step``: ``{"step": 0, "exp_avg": flat, "exp_avg_sq": flat}``."""
        dev = torch.device(device) if device is not None else self.fc1.weight.device
        if not self._flat_ok(dev):
            self._flatten(dev)
        n = self._flat["params"].numel()
        return {"step": 0, "exp_avg": torch.zeros(n, device=dev), "exp_avg_sq": torch.zeros(n, device=dev)}

    @torch.no_grad()
    def train_step(self, x, state=None, do_adam=True, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, weight=0.25,
                   stat_pass=True, scale=1.0, keep=False):
        """One step of the reference's ``train_augmenter`` body (augmentation/train.py:71-118, MSE mode) in one C-ABI call
        (mmvae_aug_train_step): with ``stat_pass`` a training-mode forward that only moves the BatchNorm running statistics
        (the reference's ``fake_data1``), the training-mode forward, ``weight * mean((x_aug - x)**2)`` (``weight`` is
        ``lambda[3] / 2``: the only term of ``A_loss`` with a gradient with respect to the augmenter), its backward through
        all 29 tensors and Adam (L2 ``weight_decay``, as ``torch.optim.Adam``).

        Returns ``{"mse", "mismatch", "recon_loss", "loss" (the device's 3 doubles), "state"}``; ``mismatch`` counts the
        elements with ``(x_aug > 1e-3) != (x > 1e-4)`` and ``recon_loss = (mse + 100 * mismatch / (B * D)) / 2`` is what the
        reference logs.  ``do_adam=False`` leaves the gradients in ``flat_grad()``.  ``keep=True`` adds ``h`` (the post-ReLU
        activations h1..h10 of the saved normalised pre-activations), ``s`` and ``x_aug``.  The call reads the three loss
        numbers back, so it synchronises once per step."""
        what = "Augmenter_smartseq.train_step()"
        if not self.training:
            raise RuntimeError(f"{what} needs netA.train()")
        if do_adam and (not (0.0 <= lr < float("inf")) or not (0.0 <= weight_decay < float("inf")) or not eps >= 0.0
                        or len(betas) != 2 or not all(0.0 <= b < 1.0 for b in betas)):
            raise ValueError(f"{what}: lr = {lr}, betas = {betas}, eps = {eps}, weight_decay = {weight_decay}")
        xt, dims = self._train_ready(x, what)
        f, B, dev = self._flat, xt.shape[0], xt.device
        if do_adam:
            if state is None:
                if self._adam is None or self._adam["exp_avg"].device != dev:
                    self._adam = self.train_state(dev)
                state = self._adam
            if state["exp_avg"].shape != f["params"].shape or state["exp_avg"].device != dev:
                raise ValueError(f"{what}: the state does not belong to this model on {dev}")
        passes = self._train_noise(2 if stat_pass else 1, B, dev)
        (mask, z0, en) = passes[-1]
        st = passes[0] if stat_pass else (None, None, None)
        s = torch.empty(B, self._dims[4], dtype=torch.float32, device=dev)
        out = torch.empty(B, self._dims[0], dtype=torch.float32, device=dev)
        loss = torch.empty(3, dtype=torch.float64, device=dev)
        step = state["step"] + 1 if do_adam else 0
        N.check(N.lib().mmvae_aug_train_step(
            C.byref(dims), N._ptr(f["params"]), N._ptr(f["running"]), N._ptr(f["nbt"]), N._ptr(xt), N._ptr(mask), float(self.dp.p),
            N._ptr(z0), N._ptr(en), N._ptr(st[0]), N._ptr(st[1]), N._ptr(st[2]), float(scale), float(weight), N._ptr(self._tws),
            self._tws.numel() * 4, N._ptr(f["grads"]), N._ptr(s), N._ptr(out), N._ptr(loss), int(bool(do_adam)),
            N._ptr(state["exp_avg"]) if do_adam else None, N._ptr(state["exp_avg_sq"]) if do_adam else None, int(step),
            float(lr), float(betas[0]), float(betas[1]), float(eps), float(weight_decay), C.byref(self._exec()), N._stream(dev)),
            "mmvae_aug_train_step")
        f["keep"] = (xt, passes)
        if do_adam:
            state["step"] = step
        mse, mismatch, recon = loss.tolist()
        res = {"mse": mse, "mismatch": int(mismatch), "recon_loss": recon, "loss": loss, "state": state if do_adam else None}
        if keep:
            lay = N.AugTrainLayout()           # (the workspace offsets depend on the batch)
            N.check(N.lib().mmvae_aug_param_layout(C.byref(dims), C.byref(lay)), "mmvae_aug_param_layout")
            res["h"] = [torch.relu(self._tws[lay.act_off[i]:lay.act_off[i] + B * lay.bn_n[i]].view(B, lay.bn_n[i])) for i in range(10)]
            res["s"], res["x_aug"] = s, out
        return res

    # ------------------------------------------------------------------ reference API
    @torch.no_grad()
    def forward(self, x, batched, scale=1.0, out=None):
        """udagan.py:281-329 in eval mode.  batched: x is [A, B, D] (typically ``x.expand(A, -1, -1)``), returns
        ``(s [A,B,latent], x_aug [A,B,D])``; otherwise x is [B, D] and the leading axis is dropped.  ``out``: optional
        preallocated ``(s, x_aug)`` float32 device tensors of those shapes (the trainer's pipeline reuses a ring of them)."""
        if self.training:
            if batched or x.dim() != 2:
                raise NotImplementedError("the batched (3-D) training-mode forward is not built: the augmenter trains on the "
                                          "non-batched forward (train_step / train_augmenter); the trainer runs netA.eval() "
                                          "(cpl_mixvae.py:184)")
            if out is not None:
                raise ValueError("the training-mode forward allocates its outputs")
            return self._train_forward(x, scale)
        if x.device.type != "cuda":
            raise N.NativeError("Augmenter_smartseq.forward needs GPU tensors: it runs only on the HIP engine")
        D, n1, n3, n5, Z, NZ = self._dims
        if batched:
            assert x.dim() == 3 and x.shape[-1] == D
            A, B = x.shape[0], x.shape[1]
            if x.stride(0) == 0:
                xt, xs = x[0].contiguous().float(), 0
            else:
                xt, xs = x.contiguous().float(), B * D
        else:
            assert x.dim() == 2 and x.shape[-1] == D
            A, B = 1, x.shape[0]
            xt, xs = x.contiguous().float(), 0
        dims = self._aug_dims(A, B)
        if self._packed is None or self._packed.device != xt.device:
            self._pack(dims)
        if self._explicit is not None:
            z0, eps = (t.to(xt.device).float().contiguous() for t in self._explicit)
            assert z0.shape == (A, B, NZ) and eps.shape == (A, B, Z)
        else:
            z0 = torch.randn(A, B, NZ, device=xt.device)          # udagan.py:283-289
            eps = torch.randn(A, B, Z, device=xt.device)          # reparam_trick, aug_utils.py:64
        need = int(N.lib().mmvae_aug_workspace_bytes(C.byref(dims), int(xs == 0)))
        if self._ws is None or self._ws.numel() * 4 < need or self._ws.device != xt.device:
            self._ws = torch.empty(need // 4, dtype=torch.float32, device=xt.device)
        if out is not None:
            s, out = out
            assert s.shape == (A, B, Z) and out.shape == (A, B, D) and s.is_contiguous() and out.is_contiguous()
            assert s.dtype == out.dtype == torch.float32 and out.device == xt.device
        else:
            s = torch.empty(A, B, Z, dtype=torch.float32, device=xt.device)
            out = torch.empty(A, B, D, dtype=torch.float32, device=xt.device)
        N.check(N.lib().mmvae_augment(C.byref(dims), N._ptr(self._packed), N._ptr(xt), xs, N._ptr(z0), N._ptr(eps),
                                      float(scale), N._ptr(self._ws), self._ws.numel() * 4, N._ptr(s), N._ptr(out),
                                      N.gemm_mode(self.gemm_dtype), C.byref(self._exec()), N._stream(xt.device)),
                "mmvae_augment")
        return (s, out) if batched else (s[0], out[0])


    # ------------------------------------------------------------------ row-indexed forward (no reference counterpart)
    def planes_needed(self) -> int:
        """Slice planes per matrix element the row-indexed forward wants from ``DeviceLoader.data_planes`` for the current
        ``gemm_dtype``: 3 (fp32: the exact fp32x3 slices), 1 (bf16), 0 = not offered (the fp32 matrix-instruction engine)."""
        mode = N.gemm_mode(self.gemm_dtype)
        return 3 if mode == 2 else (1 if mode == 1 else 0)

    @torch.no_grad()
    def forward_rows(self, planes, n_rows, rows, n_arm, scale=1.0, out=None):
        """``forward(data[rows].expand(n_arm, -1, -1), True, scale)`` for a batch that is rows of a resident matrix held as
        the GEMM engine's slice planes (``_native.tp_planes(data, self.planes_needed())``): the first layer reads the rows in
        place -- no gathered batch, no per-batch conversion; same results bit for bit.  rows: int64 [B] on the device."""
        if self.training:
            raise NotImplementedError("the HIP augmenter implements eval mode only")
        D, n1, n3, n5, Z, NZ = self._dims
        A, B = int(n_arm), int(rows.shape[0])
        dev = rows.device
        dims = self._aug_dims(A, B)
        if self._packed is None or self._packed.device != dev:
            self._pack(dims)
        if self._explicit is not None:
            z0, eps = (t.to(dev).float().contiguous() for t in self._explicit)
            assert z0.shape == (A, B, NZ) and eps.shape == (A, B, Z)
        else:
            z0 = torch.randn(A, B, NZ, device=dev)          # udagan.py:283-289
            eps = torch.randn(A, B, Z, device=dev)          # reparam_trick, aug_utils.py:64
        need = int(N.lib().mmvae_aug_workspace_bytes(C.byref(dims), 1))
        if self._ws is None or self._ws.numel() * 4 < need or self._ws.device != dev:
            self._ws = torch.empty(need // 4, dtype=torch.float32, device=dev)
        if out is not None:
            s, out = out
            assert s.shape == (A, B, Z) and out.shape == (A, B, D) and s.is_contiguous() and out.is_contiguous()
        else:
            s = torch.empty(A, B, Z, dtype=torch.float32, device=dev)
            out = torch.empty(A, B, D, dtype=torch.float32, device=dev)
        rows = rows.to(torch.int64).contiguous()
        N.check(N.lib().mmvae_augment_rows(C.byref(dims), N._ptr(self._packed), N._ptr(planes), int(n_rows), self.planes_needed(),
                                           N._ptr(rows), N._ptr(z0), N._ptr(eps), float(scale), N._ptr(self._ws),
                                           self._ws.numel() * 4, N._ptr(s), N._ptr(out), N.gemm_mode(self.gemm_dtype),
                                           C.byref(self._exec()), N._stream(dev)), "mmvae_augment_rows")
        return s, out


_PLAIN = (bool, int, float, str, type(None))


def _plain(v):
    """A value ``torch.load(weights_only=True)`` takes: numbers, strings and containers of them."""
    if isinstance(v, _PLAIN):
        return v
    if isinstance(v, (list, tuple)):
        return [_plain(e) for e in v]
    if isinstance(v, dict):
        return {str(k): _plain(e) for k, e in v.items()}
    if hasattr(v, "item") and getattr(v, "ndim", 1) == 0:
        return v.item()
    if hasattr(v, "tolist"):
        return _plain(v.tolist())
    return str(v)


def _adam_state_dict(netA, state, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
    """``torch.optim.Adam(netA.parameters(), lr).state_dict()`` with the moments of a ``train_step`` state."""
    f = netA._flat
    st = {}
    if state["step"] > 0:
        for i, (p, o) in enumerate(zip(netA.parameters(), f["offs"])):
            st[i] = {"step": torch.tensor(float(state["step"])),
                     "exp_avg": state["exp_avg"][o:o + p.numel()].view(p.shape).detach().cpu().clone(),
                     "exp_avg_sq": state["exp_avg_sq"][o:o + p.numel()].view(p.shape).detach().cpu().clone()}
    group = {"lr": float(lr), "betas": [float(betas[0]), float(betas[1])], "eps": float(eps), "weight_decay": float(weight_decay),
             "amsgrad": False, "maximize": False, "foreach": None, "capturable": False, "differentiable": False, "fused": None,
             "params": list(range(len(f["offs"])))}
    return {"state": st, "param_groups": [group]}


def train_augmenter(netA, netD, dataloader, parameters, device=None, resume=None):
    """The reference's ``train_augmenter`` (mmidas/augmentation/train.py:10-157, MSE mode) on the device, for ``netA`` alone.

    In that loop the generator loss, the triplet loss, ``mseDist(z1, z2)`` and the BCE half of ``recon_loss`` reach ``netA``
    only through ``0. * fake_data`` followed by an in-place fill: their gradients with respect to ``netA`` are exact zeros,
    and ``A_loss.backward()`` leaves bit for bit the ``.grad`` of ``lambda[3] * 0.5 * mse_loss(fake_data2, real_data)``
    alone.  The discriminator therefore never influences the augmenter and is not built: ``netD`` must be None.

    ``parameters``: ``num_epochs, learning_rate, lambda`` (only ``[3]``), ``batch_size, save, saving_path, num_n, num_z,
    n_features``; ``initial_w`` is accepted and has no effect (the reference's ``weights_init`` touches Conv2d and
    BatchNorm2d modules only); ``mode == 'ZINB'`` raises.  ``dataloader`` yields ``(data, _)`` pairs.  Per step: two
    training-mode forwards (``Augmenter_smartseq.train_step`` with its statistics pass) and Adam.  With ``save`` it writes
    ``saving_path + 'augmenter.pth'``: ``netA``, ``optimA`` (a ``torch.optim.Adam`` state dict), ``parameters`` (plain
    values), the epoch count and the random generators' states, which ``resume=<file>`` continues from bit for bit.
    Returns ``{"mse", "recon_loss"}`` per step and ``{"epoch_mse", "epoch_recon_loss"}`` per epoch."""
    import time
    if netD is not None:
        raise NotImplementedError(
            "train_augmenter: netD must be None.  In the reference's loop every term of A_loss but lambda[3] * 0.5 * mse_loss "
            "reaches netA through `0. * fake_data` followed by an in-place fill, so its gradient with respect to netA is exactly "
            "zero: the discriminator never influences the augmenter, and it is not built here")
    if str(parameters.get("mode", "MSE")).upper() == "ZINB":
        raise NotImplementedError("train_augmenter: mode 'ZINB' is not offered (Augmenter_smartseq has no fc11_p head)")
    D, NZ, Z = netA._dims[0], netA._dims[5], netA._dims[4]
    for key, have in (("n_features", D), ("num_n", NZ), ("num_z", Z)):
        if int(parameters[key]) != have:
            raise ValueError(f"train_augmenter: parameters[{key!r}] = {parameters[key]} but netA has {have}")
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device() if torch.cuda.is_available() else 0)
    if dev.type != "cuda":
        raise N.NativeError("train_augmenter needs a GPU: the step runs only on the HIP engine")
    lr = float(parameters["learning_rate"])
    weight = float(parameters["lambda"][3]) / 2.0
    n_epochs = int(parameters["num_epochs"])
    netA.to(dev).train()
    state = netA.train_state(dev)
    first = 0
    hist = {"mse": [], "recon_loss": [], "epoch_mse": [], "epoch_recon_loss": []}
    if resume is not None:
        ck = torch.load(resume, map_location="cpu", weights_only=True)
        netA.load_state_dict(ck["netA"])
        if not netA._flat_ok(dev):     # (should load_state_dict have replaced a tensor)
            netA._flatten(dev)
        f = netA._flat
        for i, (p, o) in enumerate(zip(netA.parameters(), f["offs"])):
            e = ck["optimA"]["state"].get(i)
            if e is not None:
                state["exp_avg"][o:o + p.numel()].copy_(e["exp_avg"].reshape(-1))
                state["exp_avg_sq"][o:o + p.numel()].copy_(e["exp_avg_sq"].reshape(-1))
                state["step"] = int(e["step"])
        first = int(ck.get("epoch", 0))
        if "rng_cpu" in ck:
            torch.set_rng_state(ck["rng_cpu"])
            torch.cuda.set_rng_state(ck["rng_cuda"], dev)
        hist = {k: list(v) for k, v in ck.get("history", hist).items()}
    for epoch in range(first, n_epochs):
        t0 = time.time()
        mse_e = rec_e = 0.0
        n_it = 0
        for batch in dataloader:
            data = batch[0] if isinstance(batch, (tuple, list)) else batch
            if data.shape[0] < 2:          # (a one-row remainder has no batch statistics; the reference's fixed-size labels refuse it too)
                continue
            r = netA.train_step(data.to(dev), state, lr=lr, weight=weight)
            hist["mse"].append(r["mse"])
            hist["recon_loss"].append(r["recon_loss"])
            mse_e += r["mse"]
            rec_e += r["recon_loss"]
            n_it += 1
        n_it = max(n_it, 1)
        hist["epoch_mse"].append(mse_e / n_it)
        hist["epoch_recon_loss"].append(rec_e / n_it)
        # (the reference's line with the terms there are: its generator, discriminator and triplet terms need netD)
        print("=====> Epoch:{}, MSE Loss: {:.4f}, Recon Loss: {:.4f}, Elapsed Time:{:.2f}".format(
            epoch, mse_e / n_it, rec_e / n_it, time.time() - t0))
    netA.repack()
    if parameters.get("save"):
        torch.save({"netA": {k: v.detach().cpu().clone() for k, v in netA.state_dict().items()},
                    "optimA": _adam_state_dict(netA, state, lr),
                    "parameters": _plain(dict(parameters, n_dim=netA._dims[2], p_drop=float(netA.dp.p))),
                    "epoch": max(n_epochs, first),
                    "rng_cpu": torch.get_rng_state(), "rng_cuda": torch.cuda.get_rng_state(dev),
                    "history": hist},
                   str(parameters["saving_path"]) + "augmenter.pth")
    return hist


def mk_augmenter(pretrained: str, load: bool = True):
    """cpl_mixvae.py:128-149: the checkpoint holds ``parameters`` (num_n, num_z, n_features) and ``netA``.  Loaded with
    ``weights_only=True`` (tensors and plain containers only)."""
    aug_model = torch.load(pretrained, map_location="cpu", weights_only=True)
    aug_param = aug_model["parameters"]
    # (n_dim / p_drop: written by this project's train_augmenter; the reference's files carry neither and mean the defaults)
    netA = Augmenter_smartseq(noise_dim=aug_param["num_n"], latent_dim=aug_param["num_z"],
                              input_dim=aug_param["n_features"], n_dim=aug_param.get("n_dim", 500),
                              p_drop=aug_param.get("p_drop", 0.5))
    if load:
        netA.load_state_dict(aug_model["netA"])
    return aug_model, aug_param, netA

"""Guarded, pre-filled allocations for the package's uninitialised buffers (workspaces and `torch.empty` outputs).

`guarded(modules, fill)` replaces the global name `torch` of each listed package module by a proxy.  The proxy forwards
every attribute to the real torch except `empty`, `empty_like` and `empty_strided`: a device allocation made through one of
those is a view into a larger uint8 tensor

    [ alignment slack | guard 4096 B of 0xA5 | payload, every byte = fill | guard 4096 B of 0xA5 ]

whose payload starts at a multiple of 256 bytes.  Shape, dtype and strides are those the same call gives on the `meta`
device, so the caller sees exactly the tensor it asked for.  The context keeps every buffer alive until it exits (nothing is
recycled inside it) and records the call site, shape and dtype of each.  `check()` synchronises the device (all streams) and
asserts that every guard byte is intact; a failure names the allocation, the side and the first damaged offset.

Two fills, because they expose different readers of memory the call never wrote:
  0xFF  every float32 / float64 lane is a NaN, every integer -1: poisons sums;
  0x5A  float32 ~ 1.5e16, int32 1515870810: a NaN compares false with everything, so a stale value that only feeds a
        branch, a max or an index stays hidden under 0xFF; a large finite value takes the other side of those.

What this does NOT see: a write more than 4096 bytes past either end of a buffer (as undetected as without the harness; up
to 4096 bytes it lands in memory the harness owns, cannot fault, corrupts nothing else and is reported); allocations made
some other way (`Tensor.new_empty`, `torch.zeros` -- the package has no `new_empty` site); zero-byte requests and `out=`
calls, which pass through; CPU allocations unless `guard_cpu=True` (the harness's own self-test).
"""
import contextlib
import importlib
import os
import sys
import types

import torch as _torch

GUARD = 4096
GUARD_BYTE = 0xA5
ALIGN = 256
PACKAGE = "distributed_vae_amd"
# every package module in which a grep finds torch.empty / empty_like / empty_strided
MODULES = ("_native", "augmentation", "nn_model", "cpl_mixvae", "dist", "utils.dataloader", "utils.cluster_analysis")
_HERE = os.path.abspath(__file__)


class GuardError(AssertionError):
    pass


class _Alloc:
    __slots__ = ("raw", "lo", "hi", "site", "shape", "dtype", "nbytes", "view")

    def describe(self):
        return f"{self.site} shape={tuple(self.shape)} dtype={self.dtype} ({self.nbytes} bytes)"


def _call_site():
    f = sys._getframe(1)
    while f is not None and os.path.abspath(f.f_code.co_filename) == _HERE:
        f = f.f_back
    if f is None:
        return "?"
    return f"{os.path.basename(f.f_code.co_filename)}:{f.f_lineno}"


class Guard:
    """The state of one `guarded` context: the allocations made under it, `check()`, and the proxy."""

    def __init__(self, fill, guard_cpu=False):
        assert 0 <= int(fill) <= 255
        self.fill = int(fill)
        self.guard_cpu = guard_cpu
        self.allocs = []
        self.proxy = _TorchProxy(self)

    # -- allocation -------------------------------------------------------------------------------------------------
    def _device_of(self, fn, args, kw):
        dev = kw.get("device")
        if dev is None and fn is _torch.empty_like:
            dev = args[0].device if args else kw["input"].device
        if dev is None:
            dev = _torch.get_default_device() if hasattr(_torch, "get_default_device") else "cpu"
        return _torch.device(dev)

    def alloc(self, fn, args, kw):
        if kw.get("out") is not None:
            return fn(*args, **kw)
        dev = self._device_of(fn, args, kw)
        if dev.type == "meta" or (dev.type == "cpu" and not self.guard_cpu):
            return fn(*args, **kw)
        mkw = {k: v for k, v in kw.items() if k not in ("pin_memory", "requires_grad")}
        mkw["device"] = "meta"
        meta = fn(*args, **mkw)
        if meta.numel() == 0:
            return fn(*args, **kw)
        assert not meta.is_sparse and meta.layout == _torch.strided, "guarded allocations are strided tensors"
        item = meta.element_size()
        extent = 1 + sum((n - 1) * s for n, s in zip(meta.shape, meta.stride()))
        nbytes = extent * item
        if dev.type == "cuda" and dev.index is None:
            dev = _torch.device("cuda", _torch.cuda.current_device())
        raw = _torch.empty(ALIGN + GUARD + nbytes + GUARD, dtype=_torch.uint8, device=dev)
        off = (-(raw.data_ptr() + GUARD)) % ALIGN
        a = _Alloc()
        a.raw = raw
        a.lo = raw[off: off + GUARD]
        a.hi = raw[off + GUARD + nbytes: off + GUARD + nbytes + GUARD]
        payload = raw[off + GUARD: off + GUARD + nbytes]
        a.lo.fill_(GUARD_BYTE)
        a.hi.fill_(GUARD_BYTE)
        payload.fill_(self.fill)
        t = payload.view(meta.dtype).as_strided(tuple(meta.shape), tuple(meta.stride()))
        assert t.data_ptr() % ALIGN == 0 and t.data_ptr() == raw.data_ptr() + off + GUARD
        if kw.get("requires_grad"):
            t.requires_grad_(True)
        a.site, a.shape, a.dtype, a.nbytes, a.view = _call_site(), meta.shape, meta.dtype, nbytes, t
        self.allocs.append(a)
        return t

    # -- verification -----------------------------------------------------------------------------------------------
    def check(self):
        """Synchronise (device-wide: every stream) and require every guard byte of every allocation to be intact."""
        if _torch.cuda.is_available() and any(a.raw.is_cuda for a in self.allocs):
            _torch.cuda.synchronize()
        by_dev = {}
        for a in self.allocs:
            by_dev.setdefault(a.raw.device, []).append(a)
        errors = []
        for dev, allocs in by_dev.items():
            for i0 in range(0, len(allocs), 1024):
                part = allocs[i0: i0 + 1024]
                bad = _torch.stack([g for a in part for g in (a.lo, a.hi)]).ne(GUARD_BYTE)
                rows = bad.any(dim=1).nonzero().flatten().tolist()
                for r in rows:
                    a, side = part[r // 2], ("before" if r % 2 == 0 else "after")
                    first = int(bad[r].nonzero()[0])
                    n = int(bad[r].sum())
                    where = (f"{GUARD - first} bytes before the payload's first byte" if side == "before"
                             else f"{first} bytes past the payload's end")
                    errors.append(f"guard {side} the allocation of {a.describe()} damaged: first damaged byte at guard "
                                  f"offset {first} ({where}), {n} byte(s) changed")
        if errors:
            raise GuardError("\n".join(errors))

    def sites(self):
        return [a.describe() for a in self.allocs]


class _TorchProxy(types.ModuleType):
    """Stands in for a module's global `torch`: everything is the real torch's except the uninitialised allocators."""

    def __init__(self, guard):
        super().__init__("torch")
        self.__dict__["_guard"] = guard

    def __getattr__(self, name):
        return getattr(_torch, name)

    def empty(self, *args, **kw):
        return self._guard.alloc(_torch.empty, args, kw)

    def empty_like(self, *args, **kw):
        return self._guard.alloc(_torch.empty_like, args, kw)

    def empty_strided(self, *args, **kw):
        return self._guard.alloc(_torch.empty_strided, args, kw)


def _resolve(m):
    return m if isinstance(m, types.ModuleType) else importlib.import_module(f"{PACKAGE}.{m}")


@contextlib.contextmanager
def guarded(modules=MODULES, fill=0xFF, guard_cpu=False, monkeypatch=None):
    """Run a block with the listed modules' uninitialised allocations guarded and pre-filled; yields the `Guard`.
    monkeypatch: pytest's fixture, through which the proxy is then installed (so that a test that dies inside the block in
    a way that skips the `finally` still leaves the modules as it found them)."""
    put = (lambda m, v: monkeypatch.setattr(m, "torch", v)) if monkeypatch is not None else (
        lambda m, v: m.__dict__.__setitem__("torch", v))
    g = Guard(fill, guard_cpu)
    mods = [_resolve(m) for m in modules]
    saved = []
    try:
        for m in mods:
            assert m.__dict__.get("torch") is _torch, f"{m.__name__} has no global `torch` to replace"
            saved.append(m)
            put(m, g.proxy)
        yield g
    finally:
        for m in saved:
            put(m, _torch)
        if _torch.cuda.is_available() and any(a.raw.is_cuda for a in g.allocs):
            _torch.cuda.synchronize()
        g.allocs.clear()

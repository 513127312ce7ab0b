"""The allocation harness itself (tests/alloc_guard.py), on the CPU with a toy module, and the completeness of
tests/alloc_cases.py: every device entry point of include/mmvae.h that the Python layer binds has a case or a stated reason
for having none.  Needs neither a GPU nor the built library."""
import ctypes
import os
import re
import types

import pytest
import torch

from tests import alloc_cases
from tests.alloc_guard import GUARD, GuardError, guarded

TOY_SRC = '''\
import torch


def correct(n):
    out = torch.empty(n, dtype=torch.float32)
    out.copy_(torch.arange(n, dtype=torch.float32))
    return out


def write_past_end(n, poke):
    out = torch.empty(n, dtype=torch.float32)
    out.zero_()
    poke(out.data_ptr() + out.numel() * 4)
    return out


def write_before_start(n, poke):
    out = torch.empty(n, dtype=torch.float32)
    out.zero_()
    poke(out.data_ptr() - 1)
    return out


def leaves_last_unwritten(n):
    out = torch.empty(n, dtype=torch.float32)
    out[: n - 1] = 1.0
    return out


def branches_on_unwritten(n):
    ws = torch.empty(n, dtype=torch.float32)          # a "workspace" whose last slot nobody writes
    ws[: n - 1] = 1.0
    out = torch.zeros(1)
    if bool(ws[n - 1] > 100.0):                       # false for a NaN, true for 1.5e16
        out += 1.0
    return out


def shapes():
    a = torch.empty(3, 5, dtype=torch.float64)
    b = torch.empty((3, 5), dtype=torch.int32)
    c = torch.empty_like(a)
    d = torch.empty_like(a.t())
    e = torch.empty_strided((4, 6), (8, 1), dtype=torch.float32)
    z = torch.empty(0, 7)
    return a, b, c, d, e, z
'''
TOY_FILE = "alloc_guard_toy.py"


def _line_of(text):
    return 1 + next(i for i, line in enumerate(TOY_SRC.splitlines()) if text in line)


@pytest.fixture
def toy():
    m = types.ModuleType("alloc_guard_toy")
    exec(compile(TOY_SRC, TOY_FILE, "exec"), m.__dict__)
    assert m.torch is torch
    return m


def _poke(addr):
    ctypes.memset(addr, 0, 1)        # inside the harness's own buffer: the guard is there to take exactly this


def _bits(t):
    return t.contiguous().view(torch.uint8).clone()


def test_correct_function_passes(toy, monkeypatch):
    for fill in (0xFF, 0x5A):
        with guarded([toy], fill, guard_cpu=True, monkeypatch=monkeypatch) as g:
            out = toy.correct(37)
            g.check()
            assert len(g.allocs) == 1 and g.allocs[0].site == f"{TOY_FILE}:{_line_of('def correct') + 1}"
            assert torch.equal(out, torch.arange(37, dtype=torch.float32))
        assert toy.torch is torch


def test_write_one_byte_past_the_end_is_reported(toy):
    with guarded([toy], 0xFF, guard_cpu=True) as g:
        toy.write_past_end(37, _poke)
        with pytest.raises(GuardError) as e:
            g.check()
    msg = str(e.value)
    assert f"{TOY_FILE}:{_line_of('def write_past_end') + 1}" in msg and "guard after" in msg and "offset 0 " in msg, msg
    assert "shape=(37,)" in msg and "torch.float32" in msg


def test_write_one_byte_before_the_start_is_reported(toy):
    with guarded([toy], 0x5A, guard_cpu=True) as g:
        toy.write_before_start(37, _poke)
        with pytest.raises(GuardError) as e:
            g.check()
    msg = str(e.value)
    assert f"{TOY_FILE}:{_line_of('def write_before_start') + 1}" in msg and "guard before" in msg, msg
    assert f"offset {GUARD - 1} " in msg and "1 bytes before" in msg


def test_unwritten_element_differs_between_the_fills(toy):
    outs = []
    for fill in (0xFF, 0x5A):
        with guarded([toy], fill, guard_cpu=True) as g:
            outs.append(_bits(toy.leaves_last_unwritten(9)))
            g.check()
    assert not torch.equal(outs[0], outs[1])
    assert torch.equal(outs[0][:-4], outs[1][:-4])                      # the written part agrees
    assert outs[0][-4:].tolist() == [0xFF] * 4 and outs[1][-4:].tolist() == [0x5A] * 4
    with guarded([toy], 0xFF, guard_cpu=True):
        assert not bool(torch.isfinite(toy.leaves_last_unwritten(9)).all())


def test_branch_on_unwritten_needs_the_finite_fill(toy):
    res = {}
    for fill in (0xFF, 0x5A):
        with guarded([toy], fill, guard_cpu=True) as g:
            res[fill] = float(toy.branches_on_unwritten(9))
            g.check()
    # the NaN fill alone gives the "clean" answer (and a finite one); the large finite fill takes the other branch
    assert res[0xFF] == 0.0 and res[0x5A] == 1.0


def test_alignment_shapes_and_passthrough(toy):
    with guarded([toy], 0x5A, guard_cpu=True) as g:
        a, b, c, d, e, z = toy.shapes()
        assert len(g.allocs) == 5                                        # the zero-byte request passes through
        for t in (a, b, c, d, e):
            assert t.data_ptr() % 256 == 0
        assert a.shape == (3, 5) and a.dtype == torch.float64 and a.is_contiguous()
        assert b.shape == (3, 5) and b.dtype == torch.int32 and bool((b == 0x5A5A5A5A).all())
        assert c.shape == (3, 5) and c.stride() == (5, 1)
        assert d.shape == (5, 3) and d.stride() == (1, 5)                # empty_like keeps a dense permutation
        assert e.shape == (4, 6) and e.stride() == (8, 1)
        assert z.shape == (0, 7)
        assert abs(float(torch.empty(1).copy_(e[0, 0])) - 1.5e16) < 1e15
        # the pitched allocation owns its padding: writing the whole 4 x 8 footprint but the last 2 stays inside
        e.as_strided((30,), (1,)).fill_(0.0)
        g.check()
    with guarded([toy], 0xFF, guard_cpu=False) as g:                     # CPU allocations pass through by default
        toy.shapes()
        assert g.allocs == []


def test_proxy_forwards_everything_else(toy):
    with guarded([toy], 0xFF, guard_cpu=True) as g:
        proxy = toy.torch
        assert proxy is g.proxy and proxy is not torch
        assert proxy.float32 is torch.float32 and proxy.Tensor is torch.Tensor and proxy.nn is torch.nn
        assert isinstance(toy.correct(3), proxy.Tensor)
        assert proxy.zeros is torch.zeros and proxy.cuda is torch.cuda
        with pytest.raises(AttributeError):
            proxy.no_such_attribute
    assert toy.torch is torch


def test_modules_are_restored_after_an_exception(toy):
    with pytest.raises(ZeroDivisionError):
        with guarded([toy], 0xFF, guard_cpu=True):
            1 / 0
    assert toy.torch is torch


# ---- completeness of tests/alloc_cases.py ---------------------------------------------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "distributed-vae_amd")


def bound_entry_points():
    with open(os.path.join(PKG, "_native.py")) as f:
        names = set(re.findall(r"L\.(mmvae_\w+)\.argtypes", f.read()))
    with open(os.path.join(PKG, "augmentation.py")) as f:
        names |= set(re.findall(r"\b(mmvae_\w+)\(", f.read()))
    return names


def test_every_entry_point_has_a_case_or_a_reason():
    names = bound_entry_points()
    assert len(names) > 100
    covered = set()
    for case in alloc_cases.CASES:
        assert case.covers, case.name
        covered |= set(case.covers)
    assert covered <= names, sorted(covered - names)                     # a case names only what exists
    excluded = set(alloc_cases.EXCLUDED)
    assert all(isinstance(r, str) and r.strip() for r in alloc_cases.EXCLUDED.values())
    assert not (covered & excluded), sorted(covered & excluded)
    assert excluded <= names, sorted(excluded - names)
    missing = sorted(names - covered - excluded)
    assert not missing, f"device entry points without an allocation case or a stated reason: {missing}"


def test_case_names_are_unique():
    names = [c.name for c in alloc_cases.CASES]
    assert len(names) == len(set(names))


def test_guarded_modules_are_the_ones_that_allocate():
    """alloc_guard.MODULES is every package module where a grep finds an uninitialised allocation; none uses new_empty."""
    from tests.alloc_guard import MODULES
    found = set()
    for dirpath, _, files in os.walk(PKG):
        for fn in files:
            if fn.endswith(".py"):
                with open(os.path.join(dirpath, fn)) as f:
                    src = f.read()
                assert "new_empty" not in src, fn
                if re.search(r"torch\.empty(_like|_strided)?\(", src):
                    rel = os.path.relpath(os.path.join(dirpath, fn), PKG)[:-3].replace(os.sep, ".")
                    found.add(rel)
    assert found == set(MODULES), (sorted(found), sorted(MODULES))

"""-m gpu: no entry point writes outside the workspace and outputs it is given, reads workspace or output memory it did not
write, or leaves an output element unwritten.

Every case of tests/alloc_cases.py runs three times: as it is, and under tests/alloc_guard.py with every uninitialised
allocation of the package pre-filled with 0xFF (NaN in every float lane, -1 in every integer) and with 0x5A (float32 1.5e16,
int32 1515870810; a value a branch, a max or an index reacts to where it ignores a NaN), each allocation between two 4096-byte
guard zones.  Required:
  1. every guard byte is intact after each guarded run (device-wide synchronisation first: the side stream included);
  2. the three result dicts are equal bit for bit (compared as bytes, so that NaN results compare equal);
  3. every result of a guarded run is finite wherever the unguarded run's is;
  4. the padding of a pitched output (keys "pad:...") still holds the fill.

Every entry point covered here is documented as bit-identical from run to run (README.md: fixed summation orders,
integer atomics only), so no case is exempt from 2.  The models draw their noise from explicit buffers or from Philox
counters that restart with each freshly built model, so the three runs see the same draws.

The file's wall time is printed at the end of the session's output for this module (pytest -s) and recorded in DESIGN.md.
"""
import time

import pytest
import torch

from tests import alloc_cases
from tests.alloc_guard import MODULES, guarded

pytestmark = pytest.mark.gpu

FILLS = (0xFF, 0x5A)
_T0 = [None]
_SPENT = [0.0]


def _bytes(t):
    return t.contiguous().reshape(-1).view(torch.uint8)


def _finite(t):
    return torch.isfinite(t) if t.is_floating_point() else torch.ones_like(t, dtype=torch.bool)


@pytest.mark.parametrize("case", alloc_cases.CASES, ids=[c.name for c in alloc_cases.CASES])
def test_no_overrun_no_stale_read_no_unwritten_output(case, monkeypatch):
    t0 = time.perf_counter()
    if _T0[0] is None:
        _T0[0] = t0
    plain = case.run()
    torch.cuda.synchronize()
    assert plain, case.name
    for fill in FILLS:
        with guarded(MODULES, fill, monkeypatch=monkeypatch) as g:
            got = case.run()
            g.check()                                                        # 1.
            n_allocs = len(g.allocs)
        assert n_allocs > 0, "the case made no guarded allocation"
        assert set(got) == set(plain), (case.name, sorted(set(got) ^ set(plain)))
        for k, want in plain.items():
            have = got[k]
            if k.startswith("pad:"):
                assert have.numel() > 0 and bool((have == fill).all()), \
                    (case.name, k, hex(fill), "padding written", int((have != fill).sum()))     # 4.
                continue
            assert have.shape == want.shape and have.dtype == want.dtype, (case.name, k, have.shape, want.shape)
            lost = _finite(want) & ~_finite(have)
            assert not bool(lost.any()), (case.name, k, hex(fill), "non-finite where the unguarded run is finite",
                                          int(lost.sum()), lost.nonzero()[:4].tolist())            # 3.
            if not torch.equal(_bytes(have), _bytes(want)):                 # 2.
                diff = (have != want) & ~((have != have) & (want != want)) if have.is_floating_point() else have != want
                idx = diff.nonzero()[:4].tolist()
                raise AssertionError((case.name, k, hex(fill), "differs from the unguarded run", int(diff.sum()), "of", have.numel(),
                                      "first at", idx, [have[tuple(i)].item() for i in idx], [want[tuple(i)].item() for i in idx]))
    dt = time.perf_counter() - t0
    _SPENT[0] += dt
    print(f"\n{case.name}: {dt:.2f} s ({n_allocs} guarded allocations); file so far {_SPENT[0]:.1f} s")


def test_the_guard_reports_a_device_write_outside_the_payload(monkeypatch):
    """The harness on the device, as tests/test_alloc_guard_cpu.py holds it on the host: one float written just past the end of
    a `_native` workspace and one just before an output (both inside the harness's own guard zones) are reported with their
    allocation site; a clean allocation is not."""
    import distributed_vae_amd  # noqa: F401
    from distributed_vae_amd import _native as N
    with guarded(MODULES, 0x5A, monkeypatch=monkeypatch) as g:
        ws = N._workspace(1000, "cuda:0")
        out = N.torch.empty(7, 3, dtype=torch.float32, device="cuda:0")
        clean = N.torch.empty_like(out)
        assert ws.data_ptr() % 256 == 0 and out.data_ptr() % 256 == 0 and float(out[0, 0]) > 1e16 and len(g.allocs) == 3
        g.check()
        ws.as_strided((ws.numel() + 1,), (1,))[ws.numel()] = 0.0
        raw = g.allocs[1].raw
        raw[out.data_ptr() - raw.data_ptr() - 4: out.data_ptr() - raw.data_ptr()] = 0
        clean.zero_()
        with pytest.raises(AssertionError) as e:
            g.check()
    msg = str(e.value)
    assert msg.count(" damaged: ") == 2 and "_native.py:" in msg and "guard after" in msg and "guard before" in msg, msg
    assert "test_gpu_alloc_contract.py:" in msg and "offset 0 " in msg and "offset 4092 " in msg, msg


def test_every_case_ran_and_total_wall_time():
    """Prints the file's wall time (a record, not a gate)."""
    print(f"\ntests/test_gpu_alloc_contract.py: {len(alloc_cases.CASES)} cases, {_SPENT[0]:.1f} s in the cases, "
          f"{(time.perf_counter() - _T0[0]) if _T0[0] else 0.0:.1f} s wall")

"""CPU: the encoder / intermed restatement (tests/encode_restatement.py) against the reference's own outputs
(tests/golden/encode_a2.npz, tools/gen_golden_encode.py), and the host-side contract of mmvae_encode / mmvae_intermed:
declared, exported, every bad argument rejected before any device work, ABI version unchanged, and the plan of
MMVAE_CALL_ENCODE in eval mode equal to MMVAE_CALL_CLASSIFY's at every shape of tests/plan_cases.py."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import encode_restatement as ER  # noqa: E402
import plan_cases as P  # noqa: E402

G = np.load(os.path.join(ROOT, "tests", "golden", "encode_a2.npz"))
A, NC, D, H, L, Cc, S = [int(v) for v in G["cfg"]]
LIB = os.path.join(ROOT, "distributed-vae_amd", "libmmvae_hip.so")
N_KIND_ENCODE = 10          # (9 stays an unknown kind: tests/test_plan_cpu.py pins mmvae_debug_plan refusing it)
NEW = ("mmvae_encode", "mmvae_encode_workspace_bytes", "mmvae_intermed")
TOL = {"f64": 1e-11, "f32": 1e-5}          # the bounds of tests/test_decode_cpu.py
DT = [("f64", torch.float64), ("f32", torch.float32)]


def _sd(dtype, prefix="sd/"):
    out = {}
    for k in G.files:
        if k.startswith(prefix):
            v = torch.from_numpy(np.asarray(G[k]))
            out[k[len(prefix):]] = v.to(dtype) if v.is_floating_point() else v
    return out


def _close(got, want, tag, dtype):
    torch.testing.assert_close(got, torch.from_numpy(np.asarray(want)).to(dtype), rtol=TOL[tag], atol=TOL[tag])


@pytest.mark.parametrize("tag,dtype", DT)
def test_encoder_eval_restatement_matches_reference(tag, dtype):
    sd, x = _sd(dtype), torch.from_numpy(G["x"]).to(dtype)
    for a in range(A):
        x_low, c_prob, bn = ER.encoder(sd, a, x)
        _close(x_low, G[f"{tag}/enc/x_low"][a], tag, dtype)
        _close(c_prob, G[f"{tag}/enc/c_prob"][a], tag, dtype)
        assert all(torch.equal(v, sd[k]) for k, v in bn.items())
    assert float(np.abs(G["f64/enc/x_low"]).max()) > 0.1


@pytest.mark.parametrize("tag,dtype", DT)
def test_encoder_training_restatement_matches_reference(tag, dtype):
    sd, x = _sd(dtype), torch.from_numpy(G["x"]).to(dtype)
    after = _sd(dtype, f"{tag}/tr/sd/")
    for a in range(A):
        # an all-ones keep-mask at p = 0 is the reference's x_drop = 0
        x_low, c_prob, bn = ER.encoder(sd, a, x, training=True, keep=torch.ones_like(x), p=0.0)
        _close(x_low, G[f"{tag}/tr/x_low"][a], tag, dtype)
        _close(c_prob, G[f"{tag}/tr/c_prob"][a], tag, dtype)
        for k, v in bn.items():
            if k.endswith("num_batches_tracked"):
                assert int(v) == int(after[k]) == int(sd[k]) + 1, k
            else:
                torch.testing.assert_close(v, after[k], rtol=TOL[tag], atol=TOL[tag])
        assert torch.equal(after[f"batch_s.{a}.running_mean"], sd[f"batch_s.{a}.running_mean"])
        assert int(after[f"batch_s.{a}.num_batches_tracked"]) == int(sd[f"batch_s.{a}.num_batches_tracked"])
    assert float(np.abs(G["f64/tr/x_low"] - G["f64/enc/x_low"]).max()) > 1e-3, "batch statistics should differ from running"


@pytest.mark.parametrize("tag,dtype", DT)
def test_intermed_restatement_matches_reference(tag, dtype):
    sd, y = _sd(dtype), torch.from_numpy(G["im/y"]).to(dtype)
    for a in range(A):
        mu, var = ER.intermed(sd, a, y[a])
        _close(mu, G[f"{tag}/im/mu"][a], tag, dtype)
        _close(var, G[f"{tag}/im/var"][a], tag, dtype)


def test_new_entry_points_declared_and_abi_unchanged():
    hdr = open(os.path.join(ROOT, "include", "mmvae.h")).read()
    for fn in NEW:
        assert re.search(r"\b" + fn + r"\(", hdr), fn
    assert re.search(r"#define MMVAE_CALL_ENCODE 10\b", hdr) and N_KIND_ENCODE == 10
    src = open(os.path.join(ROOT, "distributed-vae_amd", "csrc", "api.hip")).read()
    assert "int mmvae_abi_version(void) { return 5; }" in src


needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason="libmmvae_hip.so not built")


@pytest.fixture(scope="module")
def N():
    sys.path.insert(0, os.path.join(ROOT, "distributed-vae_amd"))
    import importlib.util
    spec = importlib.util.spec_from_file_location("_mmvae_native_enc", os.path.join(ROOT, "distributed-vae_amd", "_native.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@needs_lib
def test_new_entry_points_exported(N):
    lib = N.lib()
    assert lib.mmvae_abi_version() == 5
    for fn in NEW:
        assert hasattr(lib, fn), fn


def _dims(N, **kw):
    d = dict(A=2, B=5, D=64, H=16, L=4, C=6, S=2)
    d.update(kw)
    return N.Dims(d["A"], d["B"], d["D"], d["H"], d["L"], d["C"], d["S"])


def _hyper(N, **kw):
    h = N.Hyper(0.005, 1.0, 1.0, 1.0, 1e-8, 0.01, 0.5, 0.2, 0, 0, 1, 0)
    for k, v in kw.items():
        setattr(h, k, v)
    return h


# fake device pointers: every case must be refused on the host, before anything dereferences them
PTR = 0x1000
FIELDS = ("x_low", "c_prob", "c", "c_smp", "s_mean", "s_logvar", "labels", "counts")


def _encode(N, d, h, nz=None, params=PTR, bn=PTR, x=PTR, out="all", row0=0, rows=5, ws=PTR, ws_bytes=1 << 40, xs=0):
    eo = None
    if out is not None:
        eo = N.EncodeOut()
        for f in (FIELDS if out == "all" else out):
            setattr(eo, f, PTR)
    return N.lib().mmvae_encode(C.byref(d) if d is not None else None, C.byref(h) if h is not None else None,
                                C.byref(nz) if nz is not None else None, params, bn, None, x, xs,
                                C.byref(eo) if eo is not None else None, row0, rows, ws, ws_bytes, None, None)


@needs_lib
@pytest.mark.parametrize("case,rc", [
    ("null_dims", -1), ("null_hyper", -1), ("null_params", -1), ("null_bn", -1), ("null_x", -1), ("null_out", -1),
    ("null_ws", -1), ("all_outputs_null", -1), ("rows_short", -1), ("row0_past", -1), ("row0_neg", -1), ("b0", -1),
    ("engine3", -1), ("engine_neg", -1), ("counts_one_arm", -1), ("neg_stride", -1), ("H129", -2), ("S33", -2), ("A9", -2),
    ("LC256", -2), ("eval_flag0", -2), ("train_c", -2), ("train_labels", -2), ("train_null_noise", -1),
    ("train_null_mask", -1), ("train_b1", -1), ("train_cap", -2), ("small_ws", -4)])
def test_encode_rejects_bad_arguments(N, case, rc):
    d, h, kw = _dims(N), _hyper(N), {}
    head = ("x_low", "c_prob")
    if case == "null_dims": d = None
    elif case == "null_hyper": h = None
    elif case == "null_out": kw["out"] = None
    elif case.startswith("null_"): kw[case[5:]] = None
    elif case == "all_outputs_null": kw["out"] = ()
    elif case == "rows_short": kw["rows"] = 4
    elif case == "row0_past": kw.update(row0=3, rows=7)
    elif case == "row0_neg": kw.update(row0=-1, rows=10)
    elif case == "b0": d = _dims(N, B=0)
    elif case == "engine3": h = _hyper(N, gemm_bf16=3)
    elif case == "engine_neg": h = _hyper(N, gemm_bf16=-1)
    elif case == "counts_one_arm": d = _dims(N, A=1)
    elif case == "neg_stride": kw["xs"] = -1
    elif case == "H129": d = _dims(N, H=129)
    elif case == "S33": d = _dims(N, S=33)
    elif case == "A9": d = _dims(N, A=9)
    elif case == "LC256": d = _dims(N, L=64, C=128 + 64)
    elif case == "eval_flag0": h = _hyper(N, eval_flag=0)
    elif case == "train_c": h, kw = _hyper(N, training=1), dict(out=head + ("c",), nz=N.make_noise(None, 1, 1))
    elif case == "train_labels": h, kw = _hyper(N, training=1), dict(out=head + ("labels",), nz=N.make_noise(None, 1, 1))
    elif case == "train_null_noise": h, kw = _hyper(N, training=1), dict(out=head)
    elif case == "train_null_mask": h, kw = _hyper(N, training=1), dict(out=head, nz=N.make_noise({}))
    elif case == "train_b1": d, h, kw = _dims(N, B=1), _hyper(N, training=1), dict(out=head, nz=N.make_noise(None, 1, 1), rows=1)
    elif case == "train_cap":
        d, h, kw = _dims(N, B=40000), _hyper(N, training=1), dict(out=head, nz=N.make_noise(None, 1, 1), rows=40000)
    elif case == "small_ws": kw["ws_bytes"] = 1024
    assert _encode(N, d, h, **kw) == rc, N.lib().mmvae_last_error_string()


def _intermed(N, d, h, params=PTR, y=PTR, mu=PTR, var=PTR, ys=0):
    return N.lib().mmvae_intermed(C.byref(d) if d is not None else None, C.byref(h) if h is not None else None, params, y,
                                  ys, mu, var, None)


@needs_lib
@pytest.mark.parametrize("case,rc", [
    ("null_dims", -1), ("null_hyper", -1), ("null_params", -1), ("null_y", -1), ("null_mu", -1), ("null_var", -1),
    ("n0", -1), ("n_neg", -1), ("engine3", -1), ("neg_stride", -1), ("S33", -2), ("C129", -2), ("LC256", -2), ("A9", -2)])
def test_intermed_rejects_bad_arguments(N, case, rc):
    d, h, kw = _dims(N), _hyper(N), {}
    if case == "null_dims": d = None
    elif case == "null_hyper": h = None
    elif case.startswith("null_"): kw[case[5:]] = None
    elif case == "n0": d = _dims(N, B=0)
    elif case == "n_neg": d = _dims(N, B=-3)
    elif case == "engine3": h = _hyper(N, gemm_bf16=3)
    elif case == "neg_stride": kw["ys"] = -1
    elif case == "S33": d = _dims(N, S=33)
    elif case == "C129": d = _dims(N, C=129)
    elif case == "LC256": d = _dims(N, L=64, C=192)
    elif case == "A9": d = _dims(N, A=9)
    assert _intermed(N, d, h, **kw) == rc, N.lib().mmvae_last_error_string()


@needs_lib
def test_workspace_rules(N):
    lib = N.lib()
    ex = N.Exec()
    for B in (3, 300, 40000):            # evaluation is not bound by the training batch cap
        d = _dims(N, B=B)
        assert lib.mmvae_encode_workspace_bytes(C.byref(d), C.byref(ex)) == lib.mmvae_workspace_bytes(C.byref(d), C.byref(ex)) > 0
    assert lib.mmvae_encode_workspace_bytes(C.byref(_dims(N, H=129)), C.byref(ex)) == 0


@needs_lib
@pytest.mark.parametrize("engine", list(P.ENGINES))
@pytest.mark.parametrize("row", P.ROWS, ids=lambda r: r.name)
def test_encode_plan_is_classify_plan_in_eval_mode(N, row, engine):
    d = N.Dims(row.A, row.B, row.D, row.H, row.L, row.C, row.S)
    h = N.Hyper(0.005, 1.0, 1.0, 1.0, 1e-8, 0.01, row.x_drop, row.s_drop, int(row.hard), 0, 1, P.ENGINES[engine])
    for side in (False, True):
        ex = N.Exec()
        ex.tune[N.TUNE_ENGINE] = P.ENGINES[engine]
        if side:
            ex.side_stream = 1          # never dereferenced: "has a side stream"
        args = P.plan_args(row, "CLASSIFY")
        want = N.debug_plan(d, h, ex, **args)
        got = N.debug_plan(d, h, ex, **dict(args, kind="ENCODE"))
        assert want.pop("kind") == "CLASSIFY" and got.pop("kind") == "ENCODE"
        assert got == want, (row.name, engine, side)
        # training mode: the forward half of mmvae_forward's plan -- the fields that name what runs up to the latent block
        h.training, h.eval_flag = 1, 0
        fwd = N.debug_plan(d, h, ex, **P.plan_args(row, "FORWARD"))
        enc = N.debug_plan(d, h, ex, **dict(P.plan_args(row, "FORWARD"), kind="ENCODE"))
        for k in ("fast", "big", "chain_planes", "lat_half", "presplit", "zero", "lat_fork_rides"):
            assert enc[k] == fwd[k], (row.name, engine, side, k)
        h.training, h.eval_flag = 0, 1

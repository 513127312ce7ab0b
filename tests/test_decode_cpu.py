"""CPU: the decoder / state traversal restatement (tests/decode_restatement.py) against the reference's own outputs
(tests/golden/decode_a2.npz, tools/gen_golden_decode.py), and the host-side contract of mmvae_decode /
mmvae_state_changes: declared, exported, every bad argument rejected before any device work, ABI version unchanged."""
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

import decode_restatement as DR  # noqa: E402

G = np.load(os.path.join(ROOT, "tests", "golden", "decode_a2.npz"))
A, _, D, H, L, Cc, S = [int(v) for v in G["cfg"]]
LIB = os.path.join(ROOT, "distributed-vae_amd", "libmmvae_hip.so")
NEW = ("mmvae_decode", "mmvae_decode_workspace_bytes", "mmvae_state_changes", "mmvae_state_changes_workspace_bytes")


def _sd(dtype):
    return {k[3:]: torch.from_numpy(np.asarray(G[k])).to(dtype) if np.asarray(G[k]).dtype.kind == "f"
            else torch.from_numpy(np.asarray(G[k])) for k in G.files if k.startswith("sd/")}


def _tol(tag):
    return (1e-11, 1e-11) if tag == "f64" else (1e-5, 1e-5)


@pytest.mark.parametrize("tag,dtype", [("f64", torch.float64), ("f32", torch.float32)])
def test_decoder_restatement_matches_reference(tag, dtype):
    sd = _sd(dtype)
    c, s = torch.from_numpy(G["dec/c"]).to(dtype), torch.from_numpy(G["dec/s"]).to(dtype)
    got = torch.stack([DR.decode(sd, a, c[a], s[a]) for a in range(A)])
    want = torch.from_numpy(G[f"{tag}/dec/out"]).to(dtype)
    rtol, atol = _tol(tag)
    assert float(want.abs().max()) > 0.1
    torch.testing.assert_close(got, want, rtol=rtol, atol=atol)


@pytest.mark.parametrize("tag,dtype", [("f64", torch.float64), ("f32", torch.float32)])
def test_state_changes_restatement_matches_reference(tag, dtype):
    sd = _sd(dtype)
    x = torch.from_numpy(G["sc/x"]).to(dtype)
    u = torch.from_numpy(G["sc/u"]).to(dtype)
    d_s = int(G["sc/d_s"])
    got = DR.state_changes(sd, x, d_s, u)[:, :, 0, :]          # sample order
    perm = torch.from_numpy(G["sc/perm"])
    want = torch.empty_like(got)
    want[:, perm] = torch.from_numpy(G[f"{tag}/sc/recon"]).to(dtype)   # undo the reference's reordering
    rtol, atol = _tol(tag)
    torch.testing.assert_close(got, want, rtol=rtol, atol=atol)
    assert float((got[:, 0] - got[:, 1]).abs().max()) > 0, "the traversal should move the reconstruction"
    assert not np.asarray(G[f"{tag}/sc/sorted"]).any()


def test_reference_reordering_is_torch_zero_sort():
    # the permutation the wrapper recomputes on the host is the one the reference applied
    assert torch.equal(torch.zeros(100).sort()[1], torch.from_numpy(G["sc/perm"]))


def test_new_entry_points_declared_and_abi_unchanged():
    hdr = open(os.path.join(ROOT, "include", "mmvae.h")).read()
    for fn in NEW:
        assert re.search(r"\b" + fn + r"\(", hdr), fn
    src = open(os.path.join(ROOT, "distributed-vae_amd", "csrc", "api.hip")).read()
    assert "int mmvae_abi_version(void) { return 5; }" in src


needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason="libmmvae_hip.so not built")


@pytest.fixture(scope="module")
def N():
    sys.path.insert(0, os.path.join(ROOT, "distributed-vae_amd"))
    import importlib.util
    spec = importlib.util.spec_from_file_location("_mmvae_native_dec", os.path.join(ROOT, "distributed-vae_amd", "_native.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@needs_lib
def test_new_entry_points_exported(N):
    L = N.lib()
    assert L.mmvae_abi_version() == 5
    for fn in NEW:
        assert hasattr(L, fn), fn


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
P = C.c_void_p(0x1000)


def _decode(N, d, h, params=P, c=P, s=P, x_rec=P, ws=P, ws_bytes=1 << 40, cs=0, ss=0):
    return N.lib().mmvae_decode(C.byref(d) if d is not None else None, C.byref(h) if h is not None else None, params, c,
                                cs, s, ss, x_rec, ws, ws_bytes, None, None)


@needs_lib
@pytest.mark.parametrize("case,rc", [
    ("null_dims", -1), ("null_hyper", -1), ("null_params", -1), ("null_c", -1), ("null_s", -1), ("null_x_rec", -1),
    ("null_ws", -1), ("n0", -1), ("n_neg", -1), ("engine3", -1), ("engine_neg", -1), ("H129", -2), ("S33", -2),
    ("A9", -2), ("train_sdrop", -2), ("train2", -2), ("neg_stride", -1), ("small_ws", -4)])
def test_decode_rejects_bad_arguments(N, case, rc):
    d, h, kw = _dims(N), _hyper(N), {}
    if case == "null_dims": d = None
    elif case == "null_hyper": h = None
    elif case.startswith("null_"): kw[case[5:]] = None
    elif case == "n0": d = _dims(N, B=0)
    elif case == "n_neg": d = _dims(N, B=-3)
    elif case == "engine3": h = _hyper(N, gemm_bf16=3)
    elif case == "engine_neg": h = _hyper(N, gemm_bf16=-1)
    elif case == "H129": d = _dims(N, H=129)
    elif case == "S33": d = _dims(N, S=33)
    elif case == "A9": d = _dims(N, A=9)
    elif case == "train_sdrop": h = _hyper(N, training=1)
    elif case == "train2": h = _hyper(N, training=2, s_drop=0.0)
    elif case == "neg_stride": kw["cs"] = -1
    elif case == "small_ws": kw["ws_bytes"] = 1024
    assert _decode(N, d, h, **kw) == rc, N.lib().mmvae_last_error_string()


def _sc(N, d, h, nz, params=P, bn=P, x=P, d_s=0, n_samp=10, x_rec=P, ws=P, ws_bytes=1 << 40):
    return N.lib().mmvae_state_changes(C.byref(d) if d is not None else None, C.byref(h) if h is not None else None,
                                       C.byref(nz) if nz is not None else None, params, bn, x, d_s, n_samp, x_rec, ws,
                                       ws_bytes, None, None)


@needs_lib
@pytest.mark.parametrize("case,rc", [
    ("null_dims", -1), ("null_hyper", -1), ("null_noise", -1), ("null_params", -1), ("null_bn", -1), ("null_x", -1),
    ("null_x_rec", -1), ("null_ws", -1), ("null_u", -1), ("mode2", -1), ("ds_neg", -1), ("ds_S", -1), ("nsamp0", -1),
    ("nsamp_neg", -1), ("b0", -1), ("engine3", -1), ("H129", -2), ("C129", -2), ("training", -2), ("small_ws", -4)])
def test_state_changes_rejects_bad_arguments(N, case, rc):
    d, h, nz, kw = _dims(N, B=1), _hyper(N), N.make_noise(None, 1, 1), {}
    if case == "null_dims": d = None
    elif case == "null_hyper": h = None
    elif case == "null_noise": nz = None
    elif case == "null_u": nz = N.make_noise({"u_state": None})
    elif case == "mode2": nz.mode = 2
    elif case.startswith("null_"): kw[case[5:]] = None
    elif case == "ds_neg": kw["d_s"] = -1
    elif case == "ds_S": kw["d_s"] = 2
    elif case == "nsamp0": kw["n_samp"] = 0
    elif case == "nsamp_neg": kw["n_samp"] = -5
    elif case == "b0": d = _dims(N, B=0)
    elif case == "engine3": h = _hyper(N, gemm_bf16=3)
    elif case == "H129": d = _dims(N, B=1, H=129)
    elif case == "C129": d = _dims(N, B=1, C=129)
    elif case == "training": h = _hyper(N, training=1, s_drop=0.0)
    elif case == "small_ws": kw["ws_bytes"] = 1024
    assert _sc(N, d, h, nz, **kw) == rc, N.lib().mmvae_last_error_string()


@needs_lib
def test_workspace_rules(N):
    L = N.lib()
    d = _dims(N, B=3)
    d300 = _dims(N, B=300)
    ex = N.Exec()
    assert L.mmvae_decode_workspace_bytes(C.byref(d), C.byref(ex)) == L.mmvae_workspace_bytes(C.byref(d), C.byref(ex))
    assert (L.mmvae_state_changes_workspace_bytes(C.byref(d), 100, C.byref(ex))
            == L.mmvae_workspace_bytes(C.byref(d), C.byref(ex)) + L.mmvae_workspace_bytes(C.byref(d300), C.byref(ex)))
    assert L.mmvae_state_changes_workspace_bytes(C.byref(d), 0, C.byref(ex)) == 0
    # evaluation is not bound by the training batch cap
    big = _dims(N, B=40000)
    assert L.mmvae_decode_workspace_bytes(C.byref(big), C.byref(ex)) > 0

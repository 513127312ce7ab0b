"""ctypes binding of libmmvae_hip.so (C ABI: include/mmvae.h).

This is the only door between the Python host code and the HIP kernels.  There is no CPU or
PyTorch fallback: if the shared library is missing or a call fails, this module raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, Optional, Tuple

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MMVAE_LIB") or os.path.join(HERE, "libmmvae_hip.so")   # env override: A/B timing of builds

ABI_VERSION = 5
N_PARAM_TENSORS = 28
N_BN = 6
MAX_ARMS = 8

# tensor order of mmvae_param_layout_t (include/mmvae.h)
PARAM_NAMES = [
    "fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias", "fc3.weight", "fc3.bias", "fc4.weight", "fc4.bias",
    "fc5.weight", "fc5.bias", "fcc.weight", "fcc.bias", "fc_mu.weight", "fc_sigma.weight", "fc_mu.bias",
    "fc_sigma.bias", "fc6.weight", "fc6.bias", "fc7.weight", "fc7.bias", "fc8.weight", "fc8.bias",
    "fc9.weight", "fc9.bias", "fc10.weight", "fc10.bias", "fc11.weight", "fc11.bias",
]
BN_NAMES = ["batch_l1", "batch_l2", "batch_l3", "batch_l4", "batch_l5", "batch_s"]

WS_IDS = {name: i for i, name in enumerate([
    "x_low", "c_prob", "c", "c_smp", "s_mean", "s_logvar", "s_smp", "y_soft",
    "r1", "r2", "r3", "r4", "r5", "d6", "d7", "d8", "d9", "d10", "zin", "dz11", "dz1", "gzin", "gzc", "g5",
    "bn_mean1", "gd10_slab", "g1", "g2", "g3", "g4", "dz2", "dz3", "dz4", "dz5",
])}

LOSS_TOTAL, LOSS_JOINT, LOSS_CENT, LOSS_CDIST, LOSS_CL2, LOSS_REC0 = 0, 1, 2, 3, 4, 5


class Dims(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("A", "B", "D", "H", "L", "C", "S")]


class Hyper(C.Structure):
    _fields_ = [("tau", C.c_float), ("temp", C.c_float), ("beta", C.c_float), ("lam", C.c_float),
                ("eps", C.c_float), ("bn_momentum", C.c_float), ("x_drop", C.c_float), ("s_drop", C.c_float),
                ("hard", C.c_int32), ("training", C.c_int32), ("eval_flag", C.c_int32), ("gemm_bf16", C.c_int32),
                ("cat_mask", C.c_uint32 * 4)]


class Noise(C.Structure):
    _fields_ = [("mode", C.c_int32), ("_pad", C.c_int32), ("x_mask", C.c_void_p), ("u_gumbel", C.c_void_p),
                ("u_state", C.c_void_p), ("s_mask", C.c_void_p), ("seed", C.c_uint64), ("offset", C.c_uint64)]


class ParamLayout(C.Structure):
    _fields_ = [("per_arm", C.c_int64), ("offset", C.c_int64 * N_PARAM_TENSORS),
                ("rows", C.c_int64 * N_PARAM_TENSORS), ("cols", C.c_int64 * N_PARAM_TENSORS),
                ("bn_per_arm", C.c_int64), ("bn_mean_offset", C.c_int64 * N_BN),
                ("bn_var_offset", C.c_int64 * N_BN), ("bn_dim", C.c_int64 * N_BN)]


class AugDims(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("A", "B", "D", "N1", "N3", "N5", "Z", "NZ")]


class AugTensors(C.Structure):
    _fields_ = [("w", C.c_void_p * 11), ("b", C.c_void_p * 11), ("bn_mean", C.c_void_p * 10), ("bn_var", C.c_void_p * 10),
                ("w_mu", C.c_void_p), ("b_mu", C.c_void_p), ("w_sigma", C.c_void_p), ("b_sigma", C.c_void_p),
                ("bn_mu_mean", C.c_void_p), ("bn_mu_var", C.c_void_p), ("noise_w", C.c_void_p),
                ("bnz_weight", C.c_void_p), ("bnz_bias", C.c_void_p), ("bnz_mean", C.c_void_p), ("bnz_var", C.c_void_p)]


class AugTrainLayout(C.Structure):
    """mmvae_aug_train_layout: Linear layers 0..13 = fc1..fc11, fc_mu, fc_sigma, noise; BatchNorms 0..11 = batch_fc1..batch_fc10,
    batch_fc_mu, bnz."""
    _fields_ = [("w_off", C.c_int64 * 14), ("b_off", C.c_int64 * 14), ("rows", C.c_int64 * 14), ("cols", C.c_int64 * 14),
                ("bnz_w_off", C.c_int64), ("bnz_b_off", C.c_int64), ("total", C.c_int64),
                ("rm_off", C.c_int64 * 12), ("rv_off", C.c_int64 * 12), ("bn_n", C.c_int64 * 12), ("run_total", C.c_int64),
                ("act_off", C.c_int64 * 10)]


AUG_LINEARS = [f"fc{i}" for i in range(1, 12)] + ["fc_mu", "fc_sigma", "noise"]
AUG_BATCHNORMS = [f"batch_fc{i}" for i in range(1, 11)] + ["batch_fc_mu", "bnz"]


class EncodeOut(C.Structure):
    """mmvae_encode_out: the arrays an encode is to write; each may be None."""
    _fields_ = [(n, C.c_void_p) for n in ("x_low", "c_prob", "c", "c_smp", "s_mean", "s_logvar", "labels", "counts")]


class CountLogp(C.Structure):
    """mmvae_count_logp_t"""
    _fields_ = [("kind", C.c_int), ("N", C.c_int64), ("D", C.c_int), ("eps", C.c_double),
                ("x", C.c_void_p), ("ldx", C.c_int64), ("mu", C.c_void_p), ("ld_mu", C.c_int64),
                ("theta", C.c_void_p), ("ld_theta", C.c_int64), ("pi", C.c_void_p), ("ld_pi", C.c_int64),
                ("mu2", C.c_void_p), ("ld_mu2", C.c_int64), ("theta2", C.c_void_p), ("ld_theta2", C.c_int64),
                ("terms", C.c_void_p), ("ld_t", C.c_int64), ("cell_sum", C.c_void_p), ("gene_sum", C.c_void_p)]


class CountSample(C.Structure):
    """mmvae_count_sample_t"""
    _fields_ = [("param", C.c_int), ("zi_kind", C.c_int), ("N", C.c_int64), ("D", C.c_int), ("cell0", C.c_int64),
                ("eps", C.c_double), ("seed", C.c_uint64), ("offset", C.c_uint64),
                ("a", C.c_void_p), ("ld_a", C.c_int64), ("b", C.c_void_p), ("ld_b", C.c_int64),
                ("zi", C.c_void_p), ("ld_zi", C.c_int64), ("out_int32", C.c_int), ("log1p", C.c_int),
                ("out", C.c_void_p), ("ld_out", C.c_int64), ("exhausted", C.c_void_p)]


N_EVENTS = 8
N_TUNE = 24
# mmvae_exec.tune indices (private: csrc/tune.h; public: MMVAE_TUNE_ENGINE in include/mmvae.h) and the
# environment switch that sets each one: the LIBRARY reads
# no environment variables, this module translates them (experiments and A/B timing only; none is needed in production)
TUNE_ENV = {
    "MMVAE_AUG_TILE": (3, int), "MMVAE_COUPLE_SIDE": (13, int), "MMVAE_BN_PARTIALS": (19, int), "MMVAE_CHAIN_FP32": (21, int),
}
TUNE_ENGINE = 17    # MMVAE_TUNE_ENGINE: the GEMM engine the caller runs (the layout's split factors are chosen for it)


class Exec(C.Structure):
    """mmvae_exec: the caller-owned execution context of one engine (side stream, fork / join events, split factors,
    experiment switches)."""
    _fields_ = [("side_stream", C.c_void_p), ("ev", C.c_void_p * N_EVENTS), ("early_grad_event", C.c_void_p),
                ("early_recorded", C.c_int32), ("split", C.c_int32 * 6), ("tune", C.c_int32 * N_TUNE)]


def exec_from_env(engine: int = 0) -> Exec:
    """An Exec with the split factors (MMVAE_SPLIT<i>) and experiment switches the environment asks for; ``engine`` is the
    GEMM engine the caller is going to run (gemm_mode(...))."""
    ex = Exec()
    ex.tune[TUNE_ENGINE] = engine
    for w in range(6):
        v = os.environ.get(f"MMVAE_SPLIT{w}")
        if v:
            ex.split[w] = int(v)
    for name, (idx, conv) in TUNE_ENV.items():
        v = os.environ.get(name)
        if v:
            ex.tune[idx] = conv(v)
    return ex


class ZinbHeadLayout(C.Structure):
    """mmvae_zinb_head_layout_t: the flat buffer of the p and r heads, per arm [fc11_p.w | fc11_p.b | fc11_r.w | fc11_r.b]"""
    _fields_ = [("per_arm", C.c_int64), ("offset", C.c_int64 * 4)]


class NativeError(RuntimeError):
    pass


# mmvae_debug_plan (include/mmvae.h): the fields of csrc/common.hpp's Plan in declaration order, the call kinds and the
# enumerators by value
PLAN_FIELDS = 23
PLAN_NAMES = ("kind", "fast", "big", "small_x3", "fc11", "gd10_slabs", "dw11_slabs", "chain_planes", "lat_half", "narrow",
              "presplit", "bwd_small_planes", "d10_planes", "dz1_in_apply", "dec_planes", "zero", "rowmap", "dz11_bf16",
              "dw11_side", "loss_on_side", "couple", "lat_fork_rides", "fc11_fork_rides")
CALL_KINDS = {"STEP": 0, "STEP_ROWS": 1, "FORWARD": 2, "BACKWARD": 3, "LOSS": 4, "CLASSIFY": 5, "REPLAY": 6, "DECODE": 7,
              "TRAVERSE": 8, "ENCODE": 10, "ZINB_STEP": 11}
PLAN_ENUMS = {
    "big": ("GEMM_GENERAL", "GEMM_FP32", "GEMM_BF16", "GEMM_X3"),
    "fc11": ("FC11_GENERAL", "FC11_ZG", "FC11_ZT", "FC11_BF16", "FC11_X3", "FC11_OUT_BF16", "FC11_OUT_X3"),
    "zero": ("ZERO_NONE", "ZERO_MEMSET", "ZERO_XBITS", "ZERO_PRESPLIT"),
    "couple": ("COUPLE_INLINE", "COUPLE_SIDE", "COUPLE_IN_DEC"),
}


def debug_plan(dims: "Dims", hyper: "Hyper", ex: Optional["Exec"], kind: str, params_align: int = 16, x_align: int = 16,
               x_arm_stride: int = 0, has_x16: bool = False, fc11_grad: bool = True) -> Dict[str, object]:
    """The plan a call of ``kind`` (a key of CALL_KINDS) with these arguments would take (mmvae_debug_plan: host only, no
    device needed): {field: int, bool, or the enumerator's name}."""
    out = (C.c_int32 * PLAN_FIELDS)()
    check(lib().mmvae_debug_plan(C.byref(dims), C.byref(hyper), C.byref(ex) if ex is not None else None, CALL_KINDS[kind],
                                 int(params_align), int(x_align), int(x_arm_stride), int(bool(has_x16)), int(bool(fc11_grad)),
                                 C.byref(out)), "mmvae_debug_plan")
    plan = {}
    for name, v in zip(PLAN_NAMES, out):
        if name in PLAN_ENUMS:
            plan[name] = PLAN_ENUMS[name][v]
        elif name == "kind":
            plan[name] = next(k for k, i in CALL_KINDS.items() if i == v)
        elif name in ("gd10_slabs", "dw11_slabs"):
            plan[name] = int(v)
        else:
            plan[name] = bool(v)
    return plan


_lib = None


def lib():
    """Load libmmvae_hip.so; raises (never falls back) when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeError(
            f"{LIB_PATH} not found: build the HIP extension first "
            "(python -c 'import __graft_entry__ as g; g.build()' or python distributed-vae_amd/build.py). "
            "There is no CPU fallback.")
    L = C.CDLL(LIB_PATH)
    vp, i64, f32, i32 = C.c_void_p, C.c_int64, C.c_float, C.c_int
    # (restype is set only where it is not int, ctypes' default)
    L.mmvae_last_error_string.restype = C.c_char_p
    L.mmvae_check_dims.argtypes = [C.POINTER(Dims)]
    L.mmvae_param_layout.argtypes = [C.POINTER(Dims), C.POINTER(ParamLayout)]
    ex = C.POINTER(Exec)
    L.mmvae_workspace_bytes.argtypes = [C.POINTER(Dims), ex]
    L.mmvae_workspace_bytes.restype = C.c_size_t
    L.mmvae_ws_offset.argtypes = [C.POINTER(Dims), ex, C.c_int]
    L.mmvae_ws_offset.restype = i64
    L.mmvae_splits.argtypes = [C.POINTER(Dims), ex, C.POINTER(C.c_int32 * 6)]
    L.mmvae_forward.argtypes = [C.POINTER(Dims), C.POINTER(Hyper), C.POINTER(Noise), vp, vp, vp, vp, i64, vp, i32,
                                vp, C.c_size_t, ex, vp]
    L.mmvae_loss.argtypes = [C.POINTER(Dims), C.POINTER(Hyper), vp, C.c_size_t, vp, ex, vp]
    L.mmvae_backward.argtypes = [C.POINTER(Dims), C.POINTER(Hyper), C.POINTER(Noise), vp, vp, i64, f32, vp,
                                 C.c_size_t, vp, ex, vp]
    L.mmvae_adam_step.argtypes = [i64, vp, vp, vp, vp, i64, f32, f32, f32, f32, f32, i32, vp]
    L.mmvae_train_step.argtypes = [C.POINTER(Dims), C.POINTER(Hyper), C.POINTER(Noise), vp, vp, vp, vp, i64, vp,
                                   C.c_size_t, vp, vp, i32, vp, vp, i64, f32, f32, f32, f32, f32, i32, ex, vp]
    L.mmvae_train_step_rows.argtypes = [C.POINTER(Dims), C.POINTER(Hyper), C.POINTER(Noise), vp, vp, vp, vp, vp, i64, i64, vp, vp,
                                        C.c_size_t, vp, vp, i32, vp, vp, i64, f32, f32, f32, f32, f32, i32, ex, vp]
    L.mmvae_to_bf16.argtypes = [vp, i64, i64, i32, vp, vp]
    L.mmvae_debug_stage.argtypes = [C.POINTER(Dims), C.POINTER(Hyper), C.POINTER(Noise), i32, vp, vp, i64, vp,
                                    C.c_size_t, vp, ex, vp]
    L.mmvae_dump_noise.argtypes = [C.POINTER(Dims), C.POINTER(Hyper), C.POINTER(Noise), vp, vp, vp, vp, vp]
    L.mmvae_debug_plan.argtypes = [C.POINTER(Dims), C.POINTER(Hyper), ex, i32, i32, i32, i64, i32, i32,
                                   C.POINTER(C.c_int32 * PLAN_FIELDS)]
    L.mmvae_eval_classify.argtypes = [C.POINTER(Dims), C.POINTER(Hyper), vp, vp, vp, i64, vp, C.c_size_t, vp, vp, ex,
                                      vp]
    L.mmvae_classify.argtypes = [vp, i64, i32, vp, vp]
    L.mmvae_confmat_accumulate.argtypes = [vp, i32, i64, i32, vp, vp]
    L.mmvae_consensus.argtypes = [vp, i32, i32, vp, vp, vp]
    L.mmvae_pair_stats.argtypes = [vp, vp, i32, i64, i32, vp, i32, vp, vp, vp]
    L.mmvae_debug_pair_stats.argtypes = [vp, vp, i32, i64, i32, vp, i32, vp, vp, i32, vp]
    L.mmvae_pair_stats_finish.argtypes = [vp, vp, i32, i32, vp, vp, vp, vp, vp, vp]
    L.mmvae_mutinfo_counts.argtypes = [vp, i32, i64, i32, vp, i32, i64, i32, vp, vp, vp, vp]
    L.mmvae_debug_mutinfo_counts.argtypes = [vp, i32, i64, i32, vp, i32, i64, i32, vp, vp, vp, i32, vp]
    L.mmvae_ami_binary_workspace_bytes.argtypes = [i64]
    L.mmvae_ami_binary_workspace_bytes.restype = C.c_size_t
    L.mmvae_ami_binary.argtypes = [vp, vp, vp, i32, i32, i32, i64, vp, C.c_size_t, vp, vp]
    L.mmvae_silhouette_workspace_bytes.argtypes = [i64, i32]
    L.mmvae_silhouette_workspace_bytes.restype = C.c_size_t
    L.mmvae_silhouette.argtypes = [vp, i64, i64, i32, vp, i32, vp, vp, C.c_size_t, vp, vp]
    L.mmvae_state_corr_workspace_bytes.argtypes = [i64, i32, i32, i32]
    L.mmvae_state_corr_workspace_bytes.restype = C.c_size_t
    L.mmvae_state_corr.argtypes = [vp, i64, i64, i32, vp, vp, i64, i64, i32, vp, i32, vp, C.c_size_t, vp, vp, vp]
    L.mmvae_debug_state_corr.argtypes = [vp, i64, i64, i32, vp, vp, i64, i64, i32, vp, i32, vp, C.c_size_t, vp, vp, i32, vp]
    L.mmvae_group_moments_workspace_bytes.argtypes = [i64, i32, i32]
    L.mmvae_group_moments_workspace_bytes.restype = C.c_size_t
    L.mmvae_group_moments.argtypes = [vp, i64, i64, i32, vp, i32, vp, vp, C.c_size_t, vp, vp, vp]
    L.mmvae_debug_group_moments.argtypes = [vp, i64, i64, i32, vp, i32, vp, vp, C.c_size_t, vp, vp, i32, vp]
    L.mmvae_gauss_scores_workspace_bytes.argtypes = [i64, i32, i32, i32]
    L.mmvae_gauss_scores_workspace_bytes.restype = C.c_size_t
    L.mmvae_gauss_scores.argtypes = [vp, i64, i64, i32, vp, i32, i32, vp, vp, vp, vp, vp, C.c_size_t, vp, vp, vp, vp, vp]
    L.mmvae_leaf_merge_workspace_bytes.argtypes = [i64, i32, i32]
    L.mmvae_leaf_merge_workspace_bytes.restype = C.c_size_t
    L.mmvae_leaf_merge.argtypes = [vp, i64, i64, i32, vp, i32, vp, i64, i32, vp, i64, vp, C.c_size_t, vp, vp, vp, vp, i32, vp]
    L.mmvae_zinb_heads.argtypes = [vp, i64, i64, i32, i32, vp, vp, vp, vp, vp, vp, i64, vp]
    L.mmvae_zinb_nll_workspace_bytes.argtypes = [i64, i32]
    L.mmvae_zinb_nll_workspace_bytes.restype = C.c_size_t
    zinb_in = [vp, i64, i64, i32, i32, vp, vp, vp, vp, vp, vp, vp, i64, C.c_double]     # d10, ldh, N, H, D, three layers, X, ldx, eps
    zinb_grad_in = zinb_in + [C.c_double, i32, i32, vp, C.c_size_t]                   # scale, head mask, segments, workspace
    L.mmvae_zinb_nll.argtypes = zinb_in + [vp, C.c_size_t, vp, vp, vp]
    L.mmvae_zinb_terms_workspace_bytes.argtypes = [i64, i32]
    L.mmvae_zinb_terms_workspace_bytes.restype = C.c_size_t
    L.mmvae_zinb_terms.argtypes = [vp, i64, vp, i64, vp, i64, vp, i64, i64, i32, C.c_double, vp, C.c_size_t, vp, vp, vp, i64, vp]
    L.mmvae_zinb_head_grads_workspace_bytes.argtypes = [i64, i32, i32, i32]
    L.mmvae_zinb_head_grads_workspace_bytes.restype = C.c_size_t
    L.mmvae_zinb_head_grads_segments.argtypes = [i64, i32, i32]
    L.mmvae_zinb_head_grads.argtypes = zinb_grad_in + [vp] * 9
    L.mmvae_zinb_terms_grad.argtypes = [vp, i64, vp, i64, vp, i64, vp, i64, i64, i32, C.c_double, C.c_double, vp, vp, vp, i64, vp]
    L.mmvae_zinb_d10_grad_workspace_bytes.argtypes = [i64, i32, i32, i32]
    L.mmvae_zinb_d10_grad_workspace_bytes.restype = C.c_size_t
    L.mmvae_zinb_d10_grad_segments.argtypes = [i64, i32, i32]
    L.mmvae_zinb_d10_grad.argtypes = zinb_grad_in + [vp, i64, vp]
    L.mmvae_zinb_step_grads_workspace_bytes.argtypes = [i64, i32, i32, i32]
    L.mmvae_zinb_step_grads_workspace_bytes.restype = C.c_size_t
    L.mmvae_zinb_step_grads.argtypes = zinb_grad_in + [vp] * 9 + [i64, vp]
    L.mmvae_decoder_trunk_grads_workspace_bytes.argtypes = [i64, i32, i32, i32, i32]
    L.mmvae_decoder_trunk_grads_workspace_bytes.restype = C.c_size_t
    L.mmvae_decoder_trunk_grads_segments.argtypes = [i64, i32]
    L.mmvae_decoder_trunk_grads.argtypes = [i64, i32, i32, i32, vp, vp, vp, vp, i64, i32, vp, C.c_size_t, vp, vp, i64, vp]
    L.mmvae_zinb_head_layout.argtypes = [C.POINTER(Dims), C.POINTER(ZinbHeadLayout)]
    L.mmvae_zinb_step_workspace_bytes.argtypes = [C.POINTER(Dims), ex]
    L.mmvae_zinb_step_workspace_bytes.restype = C.c_size_t
    L.mmvae_zinb_train_step.argtypes = [C.POINTER(Dims), C.POINTER(Hyper), C.POINTER(Noise), vp, vp, vp, vp, vp, i64, C.c_double, vp,
                                        C.c_size_t, vp, C.c_size_t, vp, vp, vp, i32, vp, vp, vp, vp, i64, f32, f32, f32, f32, f32, i32,
                                        ex, vp]
    L.mmvae_zinb_objective.argtypes = [C.POINTER(Dims), C.POINTER(Hyper), vp, vp, vp, i64, C.c_double, vp, C.c_size_t, vp, C.c_size_t,
                                       vp, ex, vp]
    L.mmvae_debug_zinb_grad_host.argtypes = [i64, vp, vp, vp, vp, C.c_double, vp, vp]
    L.mmvae_debug_digamma_host.argtypes = [i64, vp, vp]
    L.mmvae_count_logp_workspace_bytes.argtypes = [i64, i32]
    L.mmvae_count_logp_workspace_bytes.restype = C.c_size_t
    L.mmvae_count_logp.argtypes = [C.POINTER(CountLogp), vp, C.c_size_t, vp]
    L.mmvae_debug_count_logp_host.argtypes = [C.POINTER(CountLogp)]
    L.mmvae_count_sample.argtypes = [C.POINTER(CountSample), vp]
    L.mmvae_debug_count_sample_host.argtypes = [C.POINTER(CountSample)]
    L.mmvae_zinb_sample.argtypes = [vp, i64, i32, vp, vp, vp, vp, vp, vp, C.POINTER(CountSample), vp]
    L.mmvae_forest_workspace_bytes.argtypes = [i64, i32, i32, i32, i32]
    L.mmvae_forest_workspace_bytes.restype = C.c_size_t
    L.mmvae_forest_cv.argtypes = [vp, i64, i64, i32, vp, vp, i32, i32, i32, i32, C.c_uint64, vp, C.c_size_t, vp, vp, vp, vp, vp, vp, vp]
    L.mmvae_gram_workspace_bytes.argtypes = [i64, i32]
    L.mmvae_gram_workspace_bytes.restype = C.c_size_t
    L.mmvae_gram_segments.argtypes = [i64, i32, C.POINTER(C.c_int64)]
    L.mmvae_gram.argtypes = [vp, i64, i64, vp, i64, i32, vp, vp, C.c_size_t, vp, vp, i32, vp]
    L.mmvae_debug_gram.argtypes = [vp, i64, i64, vp, i64, i32, vp, vp, C.c_size_t, vp, vp, i32, i32, vp]
    L.mmvae_symm_mul_workspace_bytes.argtypes = [i32, i32]
    L.mmvae_symm_mul_workspace_bytes.restype = C.c_size_t
    L.mmvae_symm_mul.argtypes = [vp, i64, i32, vp, i32, vp, vp]
    L.mmvae_pca_project_workspace_bytes.argtypes = [i64, i32, i32]
    L.mmvae_pca_project_workspace_bytes.restype = C.c_size_t
    L.mmvae_pca_project.argtypes = [vp, i64, i64, vp, i64, i32, vp, vp, i32, vp, vp]
    f64 = C.c_double
    L.mmvae_cpm_dense.argtypes = [vp, i32, i64, i64, i32, vp, i64, vp, i32, f64, i32, vp, i32, vp, vp]
    L.mmvae_debug_cpm_dense.argtypes = [vp, i32, i64, i64, i32, vp, i64, vp, i32, f64, i32, vp, i32, vp, i32, vp]
    L.mmvae_cpm_csr.argtypes = [vp, vp, vp, i32, i64, i64, i32, vp, i64, vp, i32, f64, i32, vp, i32, vp, vp]
    L.mmvae_gene_stats_workspace_bytes.argtypes = [i64, i32]
    L.mmvae_gene_stats_workspace_bytes.restype = C.c_size_t
    L.mmvae_gene_stats.argtypes = [vp, i32, i64, i64, i32, vp, i64, f64, vp, C.c_size_t, vp, vp, vp, vp]
    L.mmvae_debug_gene_stats.argtypes = [vp, i32, i64, i64, i32, vp, i64, f64, vp, C.c_size_t, vp, vp, vp, i32, vp]
    L.mmvae_aug_packed_floats.argtypes = [C.POINTER(AugDims)]
    L.mmvae_aug_packed_floats.restype = C.c_size_t
    L.mmvae_aug_workspace_bytes.argtypes = [C.POINTER(AugDims), i32]
    L.mmvae_aug_workspace_bytes.restype = C.c_size_t
    L.mmvae_aug_pack.argtypes = [C.POINTER(AugDims), C.POINTER(AugTensors), vp, vp]
    L.mmvae_augment.argtypes = [C.POINTER(AugDims), vp, vp, i64, vp, vp, f32, vp, C.c_size_t, vp, vp, i32, ex, vp]
    L.mmvae_aug_param_layout.argtypes = [C.POINTER(AugDims), C.POINTER(AugTrainLayout)]
    L.mmvae_aug_train_workspace_bytes.argtypes = [C.POINTER(AugDims)]
    L.mmvae_aug_train_workspace_bytes.restype = C.c_size_t
    L.mmvae_aug_train_forward.argtypes = [C.POINTER(AugDims), vp, vp, vp, vp, vp, f32, vp, vp, f32, vp, C.c_size_t, vp, vp, ex, vp]
    L.mmvae_aug_train_step.argtypes = [C.POINTER(AugDims), vp, vp, vp, vp, vp, f32, vp, vp, vp, vp, vp, f32, f32, vp, C.c_size_t,
                                       vp, vp, vp, vp, i32, vp, vp, i64, f32, f32, f32, f32, f32, ex, vp]
    L.mmvae_gather_rows.argtypes = [vp, i64, i64, vp, i64, i32, vp, vp]
    L.mmvae_tp_planes_bytes.argtypes = [i64, i32, i32]
    L.mmvae_tp_planes_bytes.restype = C.c_size_t
    L.mmvae_tp_planes.argtypes = [vp, i64, i64, i32, i32, vp, vp]
    L.mmvae_augment_rows.argtypes = [C.POINTER(AugDims), vp, vp, i64, i32, vp, vp, vp, f32, vp, C.c_size_t, vp, vp, i32, ex, vp]
    L.mmvae_decode_workspace_bytes.argtypes = [C.POINTER(Dims), ex]
    L.mmvae_decode_workspace_bytes.restype = C.c_size_t
    L.mmvae_decode.argtypes = [C.POINTER(Dims), C.POINTER(Hyper), vp, vp, i64, vp, i64, vp, vp, C.c_size_t, ex, vp]
    L.mmvae_state_changes_workspace_bytes.argtypes = [C.POINTER(Dims), i32, ex]
    L.mmvae_state_changes_workspace_bytes.restype = C.c_size_t
    L.mmvae_state_changes.argtypes = [C.POINTER(Dims), C.POINTER(Hyper), C.POINTER(Noise), vp, vp, vp, i32, i32, vp, vp,
                                      C.c_size_t, ex, vp]
    L.mmvae_encode_workspace_bytes.argtypes = [C.POINTER(Dims), ex]
    L.mmvae_encode_workspace_bytes.restype = C.c_size_t
    L.mmvae_encode.argtypes = [C.POINTER(Dims), C.POINTER(Hyper), C.POINTER(Noise), vp, vp, vp, vp, i64, C.POINTER(EncodeOut),
                               i64, i64, vp, C.c_size_t, ex, vp]
    L.mmvae_intermed.argtypes = [C.POINTER(Dims), C.POINTER(Hyper), vp, vp, i64, vp, vp, vp]
    L.mmvae_prune_apply.argtypes = [C.POINTER(Dims), C.POINTER(C.c_uint32 * 4), vp, vp, vp, vp, vp]
    L.mmvae_dp_unique_id.argtypes = [vp]
    L.mmvae_dp_init.argtypes = [vp, i32, i32, C.POINTER(C.c_void_p)]
    L.mmvae_allreduce_grads.argtypes = [vp, vp, i64, vp]
    L.mmvae_dp_destroy.argtypes = [vp]
    if L.mmvae_abi_version() != ABI_VERSION:
        raise NativeError("libmmvae_hip.so ABI version mismatch (rebuild: python distributed-vae_amd/build.py)")
    _lib = L
    return L


def check(rc: int, what: str):
    if rc != 0:
        msg = lib().mmvae_last_error_string().decode()
        if rc == -2:
            raise NotImplementedError(f"{what}: {msg}")
        raise NativeError(f"{what} failed (code {rc}): {msg}")


def param_layout(dims: Dims) -> ParamLayout:
    pl = ParamLayout()
    check(lib().mmvae_param_layout(C.byref(dims), C.byref(pl)), "mmvae_param_layout")
    return pl


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream(device=None):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


# ---- what the wrappers of the evaluation and analysis entry points share ----
LOAD_PATHS = {"auto": -1, "narrow": 0, "wide": 1}     # the load forms of a kernel that reads a matrix where it lies


def _need_cuda(what: str, *tensors):
    if any(t is not None and t.device.type != "cuda" for t in tensors):
        raise NativeError(f"{what} needs CUDA tensors (no CPU fallback)")


def _row_major(t: torch.Tensor) -> torch.Tensor:
    """``t`` [n, D] as the kernels read it: rows may be strided, columns not -- ``t`` itself where it is that, else a copy."""
    D = int(t.shape[1])
    return t if D == 0 or (t.stride(1) == 1 and t.stride(0) >= D) else t.contiguous()


def _row_map(what: str, rows: Optional[torch.Tensor], n_total: int) -> Tuple[Optional[torch.Tensor], int]:
    """(the int64 row map or None, the number of selected rows)"""
    if rows is None:
        return None, n_total
    if rows.dtype != torch.int64 or rows.dim() != 1:
        raise TypeError(f"{what}: rows must be int64 [n]")
    return rows.contiguous(), int(rows.numel())


def _workspace(nbytes: int, device) -> torch.Tensor:
    """An 8-byte aligned workspace of ``nbytes`` (never empty, so that it has an address)."""
    return torch.empty(max(int(nbytes) // 8, 1), dtype=torch.float64, device=device)


def _path(what: str, table: Dict[str, int], path: str) -> int:
    if path not in table:
        raise ValueError(f"{what}: path must be one of {sorted(table)}; got {path!r}")
    return table[path]


def _wide16(t: torch.Tensor) -> bool:
    """The launcher's rule (wide16, csrc/common.hpp): the 16-byte loads where the matrix's base is 16-byte aligned and its
    row pitch a whole number of 16 bytes (float32: a multiple of 4)."""
    return t.data_ptr() % 16 == 0 and (t.stride(0) * t.element_size()) % 16 == 0


def make_noise(explicit: Optional[Dict[str, torch.Tensor]] = None, seed: int = 0, offset: int = 0) -> Noise:
    """explicit: dict with x_mask (uint8 [A,B,D]), u_gumbel, u_state (float32), s_mask -> mode 0;
    otherwise Philox mode keyed by (seed, offset)."""
    n = Noise()
    if explicit is not None:
        n.mode = 0
        n.x_mask = explicit["x_mask"].data_ptr() if explicit.get("x_mask") is not None else None
        n.u_gumbel = explicit["u_gumbel"].data_ptr() if explicit.get("u_gumbel") is not None else None
        n.u_state = explicit["u_state"].data_ptr() if explicit.get("u_state") is not None else None
        n.s_mask = explicit["s_mask"].data_ptr() if explicit.get("s_mask") is not None else None
    else:
        n.mode = 1
        n.seed = seed & 0xFFFFFFFFFFFFFFFF
        n.offset = offset & 0xFFFFFFFFFFFFFFFF
    return n


_STREAMS: Dict = {}


def shared_stream(device, name: str) -> "torch.cuda.Stream":
    """One high-priority stream per (device, role) for the whole process.  HIP multiplexes streams onto a few hardware
    queues: every further stream an engine or a trainer created made it more likely that two streams meant to overlap
    share a queue (measured: the third engine of a process ran its steps in 2.0 ms instead of 1.05 ms).  Roles: "step"
    (dW11 / coupling beside the backward chain) and "produce" (next batch: gather, augmenter)."""
    key = (torch.device(device).index or 0, name)
    st = _STREAMS.get(key)
    if st is None:
        # (MMVAE_SIDE_PRIORITY / MMVAE_PRODUCE_PRIORITY: A/B timing; -1 = high)
        prio = os.environ.get("MMVAE_PRODUCE_PRIORITY" if name == "produce" else "MMVAE_SIDE_PRIORITY", "-1")
        st = torch.cuda.Stream(device=device, priority=int(prio))
        _STREAMS[key] = st
    return st


class Engine:
    """Owns the workspace and the execution context (mmvae_exec: side stream, events, split factors, switches) of one
    (dims, device) and issues the C-ABI calls on torch's current stream OF THAT DEVICE.  Nothing is shared between
    engines except the process-wide side stream of a device (see ``shared_stream``): each engine has its own events."""

    def __init__(self, A, B, D, H, L, Cc, S, device, ex: Optional[Exec] = None, gemm_engine: int = 0):
        self.dims = Dims(A, B, D, H, L, Cc, S)
        self.gemm_engine = gemm_engine             # which engine the layout's split factors are chosen for
        check(lib().mmvae_check_dims(C.byref(self.dims)), "mmvae_check_dims")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise NativeError("the HIP engine needs a GPU device (no CPU fallback)")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        # the engine's OWN execution context: from a caller's Exec only the split factors and the switches are taken --
        # stream, events and the hook are per engine (two engines built from one Exec must not share them)
        self.ex = exec_from_env(self.gemm_engine)
        if ex is not None:
            for i in range(6):
                self.ex.split[i] = ex.split[i]
            for i in range(N_TUNE):
                self.ex.tune[i] = ex.tune[i]
        self.side = None
        self.early_event = None
        self._events = []
        with torch.cuda.device(self.device):
            self.ws_bytes = int(lib().mmvae_workspace_bytes(C.byref(self.dims), C.byref(self.ex)))
            self.ws = torch.empty(self.ws_bytes // 4, dtype=torch.float32, device=self.device)
            assert self.ws.data_ptr() % 256 == 0
            self.loss_buf = torch.zeros(5 + 3 * A, dtype=torch.float32, device=self.device)
            # side stream: the dW11 GEMM overlaps the latency-bound backward chain (MMVAE_SIDE_STREAM=0 disables)
            if os.environ.get("MMVAE_SIDE_STREAM", "1") != "0":
                # High priority: HIP maps streams of one priority onto a small set of hardware queues round-robin; once
                # RCCL has created its streams the side stream can share a queue with the main stream and the overlap
                # is silently lost (measured with an initialised process group: 1.146 ms per step against 1.028 ms with
                # a high-priority side stream; no difference without a process group).
                self.side = shared_stream(self.device, "step")
                self.ex.side_stream = self.side.cuda_stream
                for i in range(N_EVENTS):
                    ev = torch.cuda.Event()
                    ev.record(self.side)               # creates the underlying hipEvent_t on this device
                    self._events.append(ev)
                    self.ex.ev[i] = ev.cuda_event

    def _s(self):
        return _stream(self.device)

    def _x(self):
        return C.byref(self.ex)

    def enable_early_grad_event(self, on: bool = True):
        """Data-parallel overlap: the next train_step(do_adam=False) records ``self.early_event`` on the side stream
        once the fc11 gradients are final (see ``early_recorded``)."""
        if on and self.early_event is None and self.side is not None:
            with torch.cuda.device(self.device):
                self.early_event = torch.cuda.Event()
                self.early_event.record(self.side)     # creates the underlying hipEvent_t
            self.ex.early_grad_event = self.early_event.cuda_event
        elif not on:
            self.early_event = None
            self.ex.early_grad_event = None

    def early_recorded(self) -> bool:
        return bool(self.ex.early_recorded)

    def ws_view(self, name: str, width: int) -> torch.Tensor:
        off = int(lib().mmvae_ws_offset(C.byref(self.dims), self._x(), WS_IDS[name]))
        if off < 0:
            raise NativeError(f"unknown workspace region {name}")
        d = self.dims
        return self.ws[off: off + d.A * d.B * width].view(d.A, d.B, width)

    def splits(self):
        """Split factors of the layout (order of mmvae_exec.split)."""
        out = (C.c_int32 * 6)()
        check(lib().mmvae_splits(C.byref(self.dims), self._x(), C.byref(out)), "mmvae_splits")
        return list(out)

    def ws_raw(self, name: str, numel: int) -> torch.Tensor:
        off = int(lib().mmvae_ws_offset(C.byref(self.dims), self._x(), WS_IDS[name]))
        return self.ws[off: off + numel]

    def forward(self, hyper: Hyper, noise: Noise, params, bn_running, nbt, x, x_arm_stride, x_rec, need_grad):
        check(lib().mmvae_forward(C.byref(self.dims), C.byref(hyper), C.byref(noise), _ptr(params), _ptr(bn_running),
                                  _ptr(nbt), _ptr(x), x_arm_stride, _ptr(x_rec), int(need_grad), _ptr(self.ws),
                                  self.ws_bytes, self._x(), self._s()), "mmvae_forward")

    def loss(self, hyper: Hyper) -> torch.Tensor:
        check(lib().mmvae_loss(C.byref(self.dims), C.byref(hyper), _ptr(self.ws), self.ws_bytes, _ptr(self.loss_buf),
                               self._x(), self._s()), "mmvae_loss")
        return self.loss_buf

    def backward(self, hyper: Hyper, noise: Noise, params, x, x_arm_stride, grads, grad_scale=1.0):
        check(lib().mmvae_backward(C.byref(self.dims), C.byref(hyper), C.byref(noise), _ptr(params), _ptr(x),
                                   x_arm_stride, float(grad_scale), _ptr(self.ws), self.ws_bytes, _ptr(grads),
                                   self._x(), self._s()), "mmvae_backward")

    def train_step(self, hyper, noise, params, bn_running, nbt, x, x_arm_stride, grads, do_adam, exp_avg,
                   exp_avg_sq, step, lr, b1=0.9, b2=0.999, adam_eps=1e-8, wd=0.0, decoupled=False):
        check(lib().mmvae_train_step(C.byref(self.dims), C.byref(hyper), C.byref(noise), _ptr(params),
                                     _ptr(bn_running), _ptr(nbt), _ptr(x), x_arm_stride, _ptr(self.ws), self.ws_bytes,
                                     _ptr(grads), _ptr(self.loss_buf), int(do_adam), _ptr(exp_avg), _ptr(exp_avg_sq),
                                     int(step), lr, b1, b2, adam_eps, wd, int(decoupled), self._x(), self._s()),
              "mmvae_train_step")
        return self.loss_buf

    def train_step_rows(self, hyper, noise, params, bn_running, nbt, data, rows, grads, do_adam, exp_avg,
                        exp_avg_sq, step, lr, b1=0.9, b2=0.999, adam_eps=1e-8, wd=0.0, decoupled=False, data16=None):
        """The fused step on a batch that is never materialised: cell b = row rows[b] of the resident matrix ``data``
        (mmvae_train_step_rows).  ``data16``: the matrix's bf16 copy (``to_bf16``; bf16 engine only).  Raises
        NotImplementedError where the library does not offer it (gather then)."""
        assert data.dim() == 2 and data.stride(1) == 1 and rows.dtype == torch.int64 and rows.numel() == self.dims.B
        if data16 is not None:
            assert (data16.dtype == torch.bfloat16 and data16.shape == data.shape and data16.stride() == data.stride()
                    and data16.device == data.device)
        check(lib().mmvae_train_step_rows(C.byref(self.dims), C.byref(hyper), C.byref(noise), _ptr(params),
                                          _ptr(bn_running), _ptr(nbt), _ptr(data), _ptr(data16), int(data.stride(0)), int(data.shape[0]),
                                          _ptr(rows), _ptr(self.ws), self.ws_bytes, _ptr(grads), _ptr(self.loss_buf),
                                          int(do_adam), _ptr(exp_avg), _ptr(exp_avg_sq), int(step), lr, b1, b2, adam_eps, wd,
                                          int(decoupled), self._x(), self._s()), "mmvae_train_step_rows")
        return self.loss_buf

    def _zws(self):
        """The ZINB kernels' workspace of ``zinb_train_step`` / ``zinb_objective`` (mmvae_zinb_step_workspace_bytes), made once."""
        if getattr(self, "zws", None) is None:
            with torch.cuda.device(self.device):
                self.zws_bytes = int(lib().mmvae_zinb_step_workspace_bytes(C.byref(self.dims), self._x()))
                if self.zws_bytes == 0:
                    raise NotImplementedError("mmvae_zinb_step_workspace_bytes: the ZINB step does not take these dimensions")
                self.zws = _workspace(self.zws_bytes, self.device)
        return self.zws

    def zinb_train_step(self, hyper, noise, params, heads_pr, bn_running, nbt, x, x_arm_stride, grads, head_grads, do_adam,
                        exp_avg, exp_avg_sq, hp_exp_avg, hp_exp_avg_sq, step, lr, b1=0.9, b2=0.999, adam_eps=1e-8, wd=0.0,
                        decoupled=False, zinb_eps=1e-6):
        """mmvae_zinb_train_step: the fused step under the ZINB objective; returns the device loss vector."""
        zws = self._zws()
        check(lib().mmvae_zinb_train_step(C.byref(self.dims), C.byref(hyper), C.byref(noise), _ptr(params), _ptr(heads_pr),
                                          _ptr(bn_running), _ptr(nbt), _ptr(x), x_arm_stride, float(zinb_eps), _ptr(self.ws),
                                          self.ws_bytes, _ptr(zws), self.zws_bytes, _ptr(grads), _ptr(head_grads),
                                          _ptr(self.loss_buf), int(do_adam), _ptr(exp_avg), _ptr(exp_avg_sq), _ptr(hp_exp_avg),
                                          _ptr(hp_exp_avg_sq), int(step), lr, b1, b2, adam_eps, wd, int(decoupled), self._x(),
                                          self._s()), "mmvae_zinb_train_step")
        return self.loss_buf

    def zinb_objective(self, hyper, params, heads_pr, x, x_arm_stride, zinb_eps=1e-6):
        """mmvae_zinb_objective on what the preceding ``forward`` left in the workspace; returns the device loss vector."""
        zws = self._zws()
        check(lib().mmvae_zinb_objective(C.byref(self.dims), C.byref(hyper), _ptr(params), _ptr(heads_pr), _ptr(x), x_arm_stride,
                                         float(zinb_eps), _ptr(self.ws), self.ws_bytes, _ptr(zws), self.zws_bytes,
                                         _ptr(self.loss_buf), self._x(), self._s()), "mmvae_zinb_objective")
        return self.loss_buf

    def eval_classify(self, hyper: Hyper, params, bn_running, x, x_arm_stride, labels, counts=None):
        """Encoder + latent block in eval mode, labels[a, b] = argmax c; counts (int64 [pairs, C, C]) accumulate."""
        check(lib().mmvae_eval_classify(C.byref(self.dims), C.byref(hyper), _ptr(params), _ptr(bn_running), _ptr(x),
                                        x_arm_stride, _ptr(self.ws), self.ws_bytes, _ptr(labels), _ptr(counts),
                                        self._x(), self._s()), "mmvae_eval_classify")
        return labels

    def encode(self, hyper: Hyper, noise: Optional[Noise], params, bn_running, nbt, x, x_arm_stride, out: Dict[str, torch.Tensor],
               row0: int = 0, rows: Optional[int] = None):
        """mmvae_encode: the encoder (and, in eval mode, the latent block) without decoder or fc11.  ``out``: the arrays to
        write by field name of mmvae_encode_out ([A, rows, .] each, contiguous); cell b of arm a lands at row row0 + b."""
        d = self.dims
        rows = d.B if rows is None else int(rows)
        eo = EncodeOut()
        widths = {"x_low": d.L, "c_prob": d.C, "c": d.C, "c_smp": d.C, "s_mean": d.S, "s_logvar": d.S}
        for name, t in out.items():
            if t is None:
                continue
            if name == "counts":
                assert t.dtype == torch.int64 and t.is_contiguous() and t.numel() == max(d.A * (d.A - 1) // 2, 1) * d.C * d.C
            elif name == "labels":
                assert t.dtype == torch.int32 and t.is_contiguous() and tuple(t.shape) == (d.A, rows)
            else:
                assert t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (d.A, rows, widths[name]), name
            assert t.device == self.device
            setattr(eo, name, t.data_ptr())
        check(lib().mmvae_encode(C.byref(self.dims), C.byref(hyper), C.byref(noise) if noise is not None else None, _ptr(params),
                                 _ptr(bn_running), _ptr(nbt), _ptr(x), int(x_arm_stride), C.byref(eo), int(row0), rows,
                                 _ptr(self.ws), self.ws_bytes, self._x(), self._s()), "mmvae_encode")
        return out

    def debug_stage(self, stage: int, hyper: Hyper, noise: Noise, params, x, x_arm_stride, grads=None):
        check(lib().mmvae_debug_stage(C.byref(self.dims), C.byref(hyper), C.byref(noise), int(stage), _ptr(params),
                                      _ptr(x), x_arm_stride, _ptr(self.ws), self.ws_bytes, _ptr(grads), self._x(),
                                      self._s()), "mmvae_debug_stage")

    def dump_noise(self, hyper: Hyper, noise: Noise):
        d = self.dims
        xm = torch.empty(d.A, d.B, d.D, dtype=torch.uint8, device=self.device)
        ug = torch.empty(d.A, d.B, d.C, dtype=torch.float32, device=self.device)
        us = torch.empty(d.A, d.B, d.S, dtype=torch.float32, device=self.device)
        sm = torch.empty(d.A, d.B, d.S, dtype=torch.uint8, device=self.device)
        check(lib().mmvae_dump_noise(C.byref(self.dims), C.byref(hyper), C.byref(noise), _ptr(xm), _ptr(ug), _ptr(us),
                                     _ptr(sm), self._s()), "mmvae_dump_noise")
        return {"x_mask": xm, "u_gumbel": ug, "u_state": us, "s_mask": sm}


class DecodeEngine:
    """Workspace and execution context of mmvae_decode (rows = dims.B) or, with ``n_samp``, of mmvae_state_changes
    (dims.B cells, n_samp samples each).  No side stream: both calls run on torch's current stream of the device."""

    def __init__(self, A, B, D, H, L, Cc, S, device, gemm_engine: int = 0, n_samp: Optional[int] = None,
                 ex: Optional[Exec] = None):
        self.dims = Dims(A, B, D, H, L, Cc, S)
        self.gemm_engine = gemm_engine
        self.n_samp = n_samp
        check(lib().mmvae_check_dims(C.byref(self.dims)), "mmvae_check_dims")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise NativeError("the HIP engine needs a GPU device (no CPU fallback)")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.ex = exec_from_env(gemm_engine)
        if ex is not None:
            for i in range(6):
                self.ex.split[i] = ex.split[i]
            for i in range(N_TUNE):
                self.ex.tune[i] = ex.tune[i]
        if n_samp is None:
            self.ws_bytes = int(lib().mmvae_decode_workspace_bytes(C.byref(self.dims), C.byref(self.ex)))
        else:
            self.ws_bytes = int(lib().mmvae_state_changes_workspace_bytes(C.byref(self.dims), int(n_samp), C.byref(self.ex)))
        if self.ws_bytes == 0:
            raise NativeError("decode workspace: unsupported dims / n_samp")
        with torch.cuda.device(self.device):
            self.ws = torch.empty(self.ws_bytes // 4, dtype=torch.float32, device=self.device)

    def ws_view(self, name: str, width: int) -> torch.Tensor:
        """A decode's region (mmvae_ws_offset of these dims): e.g. "zin", "d6" .. "d10" hold the decoder's activations."""
        off = int(lib().mmvae_ws_offset(C.byref(self.dims), C.byref(self.ex), WS_IDS[name]))
        d = self.dims
        return self.ws[off: off + d.A * d.B * width].view(d.A, d.B, width)

    def decode(self, hyper: Hyper, params, c, c_arm_stride, s, s_arm_stride, x_rec):
        check(lib().mmvae_decode(C.byref(self.dims), C.byref(hyper), _ptr(params), _ptr(c), int(c_arm_stride), _ptr(s),
                                 int(s_arm_stride), _ptr(x_rec), _ptr(self.ws), self.ws_bytes, C.byref(self.ex),
                                 _stream(self.device)), "mmvae_decode")
        return x_rec

    def state_changes(self, hyper: Hyper, noise: Noise, params, bn_running, x, d_s, x_rec):
        check(lib().mmvae_state_changes(C.byref(self.dims), C.byref(hyper), C.byref(noise), _ptr(params), _ptr(bn_running),
                                        _ptr(x), int(d_s), int(self.n_samp), _ptr(x_rec), _ptr(self.ws), self.ws_bytes,
                                        C.byref(self.ex), _stream(self.device)), "mmvae_state_changes")
        return x_rec


def intermed(dims: Dims, hyper: Hyper, params, y: torch.Tensor, y_arm_stride: int, mu: torch.Tensor, var: torch.Tensor):
    """mmvae_intermed: mu = fc_mu(y), var = sigmoid(fc_sigma(y)) for dims.B rows of dims.A arms (no workspace)."""
    check(lib().mmvae_intermed(C.byref(dims), C.byref(hyper), _ptr(params), _ptr(y), int(y_arm_stride), _ptr(mu), _ptr(var),
                               _stream(y.device)), "mmvae_intermed")
    return mu, var


def prune_apply(dims: Dims, mask_words, params=None, grads=None, exp_avg=None, exp_avg_sq=None, n: Optional[int] = None):
    """mmvae_prune_apply: +0.0 at the positions of the categories ``mask_words`` (the four words of mmvae_hyper.cat_mask: bit k
    set = category k kept) does not keep -- fcc.weight[k, :], fcc.bias[k], fc_mu.weight[:, L + k], fc_sigma.weight[:, L + k],
    fc6.weight[:, k] of every arm -- in each given flat buffer of the parameter layout; one launch on torch's current stream of
    the buffers' device.  ``n``: the floats every buffer must hold, A * per_arm (None: asked of mmvae_param_layout; a caller
    on a per-step path passes the number it already has)."""
    bufs = [t for t in (params, grads, exp_avg, exp_avg_sq) if t is not None]
    if n is None:
        n = dims.A * int(param_layout(dims).per_arm)
    for t in bufs:
        if t.device.type != "cuda":
            raise NativeError("prune_apply needs CUDA tensors (no CPU fallback)")
        assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() >= n and t.device == bufs[0].device
    words = (C.c_uint32 * 4)(*[int(w) & 0xFFFFFFFF for w in mask_words])
    stream = _stream(bufs[0].device) if bufs else None
    check(lib().mmvae_prune_apply(C.byref(dims), C.byref(words), _ptr(params), _ptr(grads), _ptr(exp_avg), _ptr(exp_avg_sq),
                                  stream), "mmvae_prune_apply")


def adam_step(params, grads, exp_avg, exp_avg_sq, step, lr, b1=0.9, b2=0.999, eps=1e-8, wd=0.0, decoupled=False):
    check(lib().mmvae_adam_step(params.numel(), _ptr(params), _ptr(grads), _ptr(exp_avg), _ptr(exp_avg_sq), int(step),
                                lr, b1, b2, eps, wd, int(decoupled), _stream(params.device)), "mmvae_adam_step")


def classify(probs: torch.Tensor) -> torch.Tensor:
    """argmax over the last axis of a float32 CUDA tensor -> int32 labels (first maximum on ties)."""
    if probs.device.type != "cuda":
        raise NativeError("classify needs a CUDA tensor (no CPU fallback)")
    p = probs.contiguous().float()
    n, Cc = p.numel() // p.shape[-1], p.shape[-1]
    out = torch.empty(p.shape[:-1], dtype=torch.int32, device=p.device)
    check(lib().mmvae_classify(_ptr(p), n, Cc, _ptr(out), _stream(p.device)), "mmvae_classify")
    return out


def confmat_accumulate(labels: torch.Tensor, Cc: int, counts: Optional[torch.Tensor] = None) -> torch.Tensor:
    """labels int32 [A, n] on the GPU -> counts int64 [A(A-1)/2, C, C] (+= when given)."""
    _need_cuda("confmat_accumulate", labels)
    lab = labels.contiguous().to(torch.int32)
    A, n = lab.shape
    if counts is None:
        counts = torch.zeros(max(A * (A - 1) // 2, 1), Cc, Cc, dtype=torch.int64, device=lab.device)
    check(lib().mmvae_confmat_accumulate(_ptr(lab), A, n, Cc, _ptr(counts), _stream(lab.device)),
          "mmvae_confmat_accumulate")
    return counts


def consensus(counts: torch.Tensor, want_norm: bool = False):
    """counts int64 [pairs, C, C] -> consensus float64 [pairs] (and the normalised matrices when want_norm)."""
    _need_cuda("consensus", counts)
    cnt = counts.contiguous()
    P, Cc, _ = cnt.shape
    out = torch.empty(P, dtype=torch.float64, device=cnt.device)
    norm = torch.empty(P, Cc, Cc, dtype=torch.float64, device=cnt.device) if want_norm else None
    check(lib().mmvae_consensus(_ptr(cnt), P, Cc, _ptr(norm), _ptr(out), _stream(cnt.device)), "mmvae_consensus")
    return (out, norm) if want_norm else out


PAIR_STATS_LDS_MAX_C = 116      # PS_LDS_MAX_C of csrc/common.hpp: the largest C whose histogram fits a workgroup's LDS
PAIR_STATS_PATHS = {"auto": -1, "lds": 0, "wave": 1}


def pair_stats(labels: torch.Tensor, probs: torch.Tensor, pairs, Cc: int, counts: Optional[torch.Tensor] = None,
               dist_acc: Optional[torch.Tensor] = None, path: str = "auto"):
    """mmvae_pair_stats: labels int32 [T, n], probs float32 [T, n, C] on the GPU, ``pairs`` a host table [n_pairs][4] of arm
    indices (lab1, prob1, lab2, prob2) -> (counts int64 [n_pairs, C, C], dist_acc int64 [n_pairs, C, C, 2]), both ``+=`` when
    given.  ``path``: "auto" (the launcher's rule), "lds" or "wave" (mmvae_debug_pair_stats: the same sums on a named path)."""
    _need_cuda("pair_stats", labels, probs)
    import numpy as np
    tab = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 4))
    lab, pr = labels.contiguous(), probs.contiguous()
    if lab.dtype != torch.int32 or pr.dtype != torch.float32:
        raise TypeError("pair_stats: labels must be int32 and probs float32")
    T, n = lab.shape
    if tuple(pr.shape) != (T, n, Cc):
        raise ValueError(f"pair_stats: probs {tuple(pr.shape)} is not [T, n, C] = {(T, n, Cc)}")
    P = tab.shape[0]
    if counts is None:
        counts = torch.zeros(P, Cc, Cc, dtype=torch.int64, device=lab.device)
    if dist_acc is None:
        dist_acc = torch.zeros(P, Cc, Cc, 2, dtype=torch.int64, device=lab.device)
    for t, shape in ((counts, (P, Cc, Cc)), (dist_acc, (P, Cc, Cc, 2))):
        if t.dtype != torch.int64 or tuple(t.shape) != shape or not t.is_contiguous() or t.device != lab.device:
            raise ValueError(f"pair_stats: accumulator must be a contiguous int64 {shape} tensor on {lab.device}")
    if n == 0 or P == 0:
        return counts, dist_acc
    tp = tab.ctypes.data_as(C.c_void_p)
    if path == "auto":
        rc = lib().mmvae_pair_stats(_ptr(lab), _ptr(pr), T, n, Cc, tp, P, _ptr(counts), _ptr(dist_acc), _stream(lab.device))
    else:
        rc = lib().mmvae_debug_pair_stats(_ptr(lab), _ptr(pr), T, n, Cc, tp, P, _ptr(counts), _ptr(dist_acc),
                                          PAIR_STATS_PATHS[path], _stream(lab.device))
    check(rc, "mmvae_pair_stats")
    return counts, dist_acc


def pair_stats_finish(counts: torch.Tensor, dist_acc: torch.Tensor) -> Dict[str, torch.Tensor]:
    """mmvae_pair_stats_finish on the accumulators of ``pair_stats``: float64 device tensors ``cm_norm``, ``emp``,
    ``dist_norm`` [n_pairs, C, C], ``diag_mean``, ``diag_min`` [n_pairs].  They are views of one buffer, ``packed`` (in this
    order), so that a caller can bring everything to the host with a single copy."""
    _need_cuda("pair_stats_finish", counts, dist_acc)
    cnt, acc = counts.contiguous(), dist_acc.contiguous()
    P, Cc, _ = cnt.shape
    if cnt.dtype != torch.int64 or acc.dtype != torch.int64 or tuple(acc.shape) != (P, Cc, Cc, 2):
        raise ValueError("pair_stats_finish: counts int64 [P, C, C] and dist_acc int64 [P, C, C, 2] expected")
    m = P * Cc * Cc
    packed = torch.empty(3 * m + 2 * P, dtype=torch.float64, device=cnt.device)
    out = {"cm_norm": packed[0:m].view(P, Cc, Cc), "emp": packed[m:2 * m].view(P, Cc, Cc),
           "dist_norm": packed[2 * m:3 * m].view(P, Cc, Cc), "diag_mean": packed[3 * m:3 * m + P],
           "diag_min": packed[3 * m + P:], "packed": packed}
    if P:
        check(lib().mmvae_pair_stats_finish(_ptr(cnt), _ptr(acc), P, Cc, _ptr(out["cm_norm"]), _ptr(out["emp"]),
                                            _ptr(out["dist_norm"]), _ptr(out["diag_mean"]), _ptr(out["diag_min"]),
                                            _stream(cnt.device)), "mmvae_pair_stats_finish")
    return out


MUTINFO_LDS_MAX_WORDS = 16384   # MI_LDS_MAX_WORDS of csrc/common.hpp: F * C + C + F counts at most for the LDS histograms
MUTINFO_PATHS = {"auto": -1, "lds": 0, "global": 1}


def mutinfo_counts(labels: torch.Tensor, targets: torch.Tensor, Cc: int, F: Optional[int] = None, out=None, path: str = "auto"):
    """mmvae_mutinfo_counts: labels int32 [A, n] and a 0/1 matrix ``targets`` [n, >= F] (uint8, bool or int32; rows may be
    strided, columns not) on the GPU -> (counts int64 [A, F, C], t_sum int64 [F], p_sum int64 [A, C]); ``out``: the three
    accumulators of an earlier call, which this one adds to.  ``F``: the leading columns used (default: all).  ``path``:
    "auto" (the launcher's rule), "lds" or "global" (mmvae_debug_mutinfo_counts: the same counts on a named path)."""
    _need_cuda("mutinfo_counts", labels, targets)
    lab = labels.contiguous()
    tg = targets.view(torch.uint8) if targets.dtype == torch.bool else targets
    if lab.dtype != torch.int32 or lab.dim() != 2 or tg.dtype not in (torch.uint8, torch.int32) or tg.dim() != 2:
        raise TypeError("mutinfo_counts: labels must be int32 [A, n] and targets uint8 / bool / int32 [n, F]")
    A, n = lab.shape
    F = int(tg.shape[1] if F is None else F)
    if tg.shape[0] != n or not 1 <= F <= tg.shape[1]:
        raise ValueError(f"mutinfo_counts: targets {tuple(tg.shape)} do not give {n} cells x {F} columns")
    if n > 1 and tg.stride(1) != 1:
        tg = tg.contiguous()
    ldt = int(tg.stride(0)) if n > 1 else max(int(tg.shape[1]), F)
    shapes = ((A, F, Cc), (F,), (A, Cc))
    if out is None:
        out = tuple(torch.zeros(s, dtype=torch.int64, device=lab.device) for s in shapes)
    for t, s in zip(out, shapes):
        if t.dtype != torch.int64 or tuple(t.shape) != s or not t.is_contiguous() or t.device != lab.device:
            raise ValueError(f"mutinfo_counts: accumulator must be a contiguous int64 {s} tensor on {lab.device}")
    counts, t_sum, p_sum = out
    args = (_ptr(lab), A, n, Cc, _ptr(tg), tg.element_size(), ldt, F, _ptr(counts), _ptr(t_sum), _ptr(p_sum))
    if path == "auto":
        rc = lib().mmvae_mutinfo_counts(*args, _stream(lab.device))
    else:
        rc = lib().mmvae_debug_mutinfo_counts(*args, MUTINFO_PATHS[path], _stream(lab.device))
    check(rc, "mmvae_mutinfo_counts")
    return counts, t_sum, p_sum


def ami_binary(counts: torch.Tensor, t_sum: torch.Tensor, p_sum: torch.Tensor, n_cells: int, table: bool = True) -> torch.Tensor:
    """mmvae_ami_binary on the counts of ``mutinfo_counts`` -> float64 [A, F, C] on the device: sklearn's adjusted mutual
    information of every (cell-type column, cluster) pair of binary labelings of ``n_cells`` cells, NaN where p_sum == 0.
    ``table``: log-gamma and log from a table in a workspace a first launch fills (the default), or evaluated per term."""
    _need_cuda("ami_binary", counts)
    cnt, ts, ps = counts.contiguous(), t_sum.contiguous(), p_sum.contiguous()
    A, F, Cc = cnt.shape
    if any(t.dtype != torch.int64 for t in (cnt, ts, ps)) or tuple(ts.shape) != (F,) or tuple(ps.shape) != (A, Cc):
        raise ValueError("ami_binary: counts int64 [A, F, C], t_sum int64 [F] and p_sum int64 [A, C] expected")
    out = torch.empty(A, F, Cc, dtype=torch.float64, device=cnt.device)
    ws, ws_bytes = None, 0
    if table:
        ws_bytes = int(lib().mmvae_ami_binary_workspace_bytes(int(n_cells)))
        ws = _workspace(ws_bytes, cnt.device)
    check(lib().mmvae_ami_binary(_ptr(cnt), _ptr(ts), _ptr(ps), A, F, Cc, int(n_cells), _ptr(ws), ws_bytes, _ptr(out),
                                 _stream(cnt.device)), "mmvae_ami_binary")
    return out


# launch_silhouette (csrc/silhouette.hip; the constants are those of csrc/common.hpp)
SILHOUETTE_SEG_COLS = 512       # SIL_SEG_COLS: a cluster of more columns is cut into segments of this many
SILHOUETTE_ROW_TILE = 256       # SIL_ROW_TILE: rows per workgroup, one thread each
SILHOUETTE_LDS_FLOATS = 4096    # SIL_LDS_FLOATS: a pass stages SILHOUETTE_LDS_FLOATS // (4 * dv) columns
SILHOUETTE_DV = (1, 2, 3, 4, 6, 8, 12, 16, 24, 32)   # SIL_DV: float4 pieces per point the kernel is built for
SILHOUETTE_MAX_D = 128


def silhouette_dv(d: int) -> int:
    """The instance of the row kernel that runs dimension ``d``: the smallest entry of SILHOUETTE_DV with 4 * dv >= d."""
    return next(v for v in SILHOUETTE_DV if 4 * v >= d)


def silhouette(x_sorted: torch.Tensor, offsets: torch.Tensor, perm: Optional[torch.Tensor] = None, out=None,
               path: str = "auto") -> torch.Tensor:
    """mmvae_silhouette: float32 points [n, d] on the GPU (rows may be strided, columns not) ordered by cluster, int64
    ``offsets`` [K + 1] (cluster k is the rows offsets[k] .. offsets[k + 1] - 1) and, optionally, the int64 permutation
    ``perm`` [n] that sorted them (sorted row r is the caller's row perm[r]) -> sklearn's silhouette samples, float64 [n] on
    the device, in the caller's order.  ``path``: the launcher has one path, "auto"."""
    _need_cuda("silhouette", x_sorted, offsets, perm)
    if path != "auto":
        raise ValueError(f"silhouette: the launcher has one path, 'auto'; got {path!r}")
    if x_sorted.dtype != torch.float32 or x_sorted.dim() != 2 or offsets.dtype != torch.int64 or offsets.dim() != 1:
        raise TypeError("silhouette: x_sorted must be float32 [n, d] and offsets int64 [K + 1]")
    n, d = (int(v) for v in x_sorted.shape)
    x = _row_major(x_sorted)
    off = offsets.contiguous()
    K = int(off.numel()) - 1
    if perm is not None:
        if perm.dtype != torch.int64 or tuple(perm.shape) != (n,):
            raise TypeError(f"silhouette: perm must be int64 [{n}]")
        perm = perm.contiguous()
    if out is None:
        out = torch.empty(n, dtype=torch.float64, device=x.device)
    elif out.dtype != torch.float64 or tuple(out.shape) != (n,) or not out.is_contiguous() or out.device != x.device:
        raise ValueError(f"silhouette: out must be a contiguous float64 [{n}] tensor on {x.device}")
    ws_bytes = int(lib().mmvae_silhouette_workspace_bytes(n, K))
    ws = _workspace(ws_bytes, x.device)
    check(lib().mmvae_silhouette(_ptr(x), int(x.stride(0)), n, d, _ptr(off), K, _ptr(perm), _ptr(ws), ws_bytes, _ptr(out),
                                 _stream(x.device)), "mmvae_silhouette")
    return out


# launch_state_corr (csrc/statecorr.hip; the constants are those of csrc/common.hpp)
STATECORR_SEG_ROWS = 256        # SC_SEG_ROWS: a group of more rows is cut into segments of this many
STATECORR_TILE = 256            # SC_TILE: genes per wave of k_sc_partial, four consecutive genes a lane
STATECORR_MAX_S = 32            # SC_MAX_S
STATECORR_PATHS = LOAD_PATHS
state_corr_wide = _wide16


def state_corr(data: torch.Tensor, state: torch.Tensor, rows: Optional[torch.Tensor] = None,
               offsets: Optional[torch.Tensor] = None, path: str = "auto") -> Tuple[torch.Tensor, torch.Tensor]:
    """mmvae_state_corr: float32 ``data`` [n_total, D] on the GPU (rows may be strided, columns not; read where it lies),
    float32 ``state`` [n, S], optionally the int64 row map ``rows`` [n] (state row r belongs to ``data[rows[r]]``; None:
    rows 0..n-1) and the int64 ``offsets`` [G + 1] that cut the n cells, ordered by group, into G groups (None: one group)
    -> (r float64 [G, S, D], count int64 [G, D]) on the device: the Pearson correlation of every state with every gene over
    the group's cells with x > 0, exactly 0 where there are at most four of them, NaN where x or the state is constant over
    them.  Inputs must be finite.  ``path``: "auto" (the launcher's rule), "narrow", "wide" -- the load forms, equal bits."""
    _need_cuda("state_corr", data, state, rows, offsets)
    path = _path("state_corr", STATECORR_PATHS, path)
    if data.dtype != torch.float32 or data.dim() != 2 or state.dtype != torch.float32 or state.dim() != 2:
        raise TypeError("state_corr: data must be float32 [n_total, D] and state float32 [n, S]")
    n_total, Dm = (int(v) for v in data.shape)
    n, S = (int(v) for v in state.shape)
    x, st = _row_major(data), _row_major(state)
    if rows is not None:
        if rows.dtype != torch.int64 or tuple(rows.shape) != (n,):
            raise TypeError(f"state_corr: rows must be int64 [{n}]")
        rows = rows.contiguous()
    G = 1
    if offsets is not None:
        if offsets.dtype != torch.int64 or offsets.dim() != 1 or offsets.numel() < 2:
            raise TypeError("state_corr: offsets must be int64 [G + 1]")
        offsets = offsets.contiguous()
        G = int(offsets.numel()) - 1
    r = torch.empty(G, S, Dm, dtype=torch.float64, device=x.device)
    count = torch.empty(G, Dm, dtype=torch.int64, device=x.device)
    ws_bytes = int(lib().mmvae_state_corr_workspace_bytes(n, Dm, S, G))
    ws = _workspace(ws_bytes, x.device)
    check(lib().mmvae_debug_state_corr(_ptr(x), int(x.stride(0)), n_total, Dm, _ptr(rows), _ptr(st), int(st.stride(0)), n, S,
                                       _ptr(offsets), G, _ptr(ws), ws_bytes, _ptr(r), _ptr(count), path,
                                       _stream(x.device)), "mmvae_state_corr")
    return r, count


# launch_group_moments / launch_gauss_scores (csrc/gaussclf.hip; the constants are those of csrc/common.hpp)
GAUSSCLF_SEG_ROWS = 256         # GC_SEG_ROWS: a group of more rows is cut into segments of this many
GAUSSCLF_ROW_CHUNK = 32         # GC_ROW_CHUNK: rows of a segment staged in LDS at a time
GAUSSCLF_DC = (16, 32, 64, 128)  # GC_DC: the largest d of each instance of the segment kernel
GAUSSCLF_ROW_TILE = 64          # GC_ROW_TILE: cells per workgroup of the score kernel, one a lane
GAUSSCLF_SCORE_WAVES = 16       # GC_SCORE_WAVES: its waves at most, min(K, 16) of them; wave w scores the w-th run of classes
GAUSSCLF_COL_BLOCK = 8          # GC_COL_BLOCK: columns of W carried at once; the d % 8 last ones go one by one
GAUSSCLF_MAX_D, GAUSSCLF_MAX_K, GAUSSCLF_MAX_F = 128, 4096, 64
GAUSSCLF_PATHS = {"auto": -1, "d16": 0, "d32": 1, "d64": 2, "d128": 3}


def gaussclf_dclass(d: int) -> str:
    """The instance of the segment kernel that the launcher runs dimension ``d`` on: a key of GAUSSCLF_PATHS."""
    return next(f"d{v}" for v in GAUSSCLF_DC if d <= v)


def group_moments(x_sorted: torch.Tensor, offsets: torch.Tensor, pivot: torch.Tensor,
                  path: str = "auto") -> Tuple[torch.Tensor, torch.Tensor]:
    """mmvae_group_moments: float32 points [n, d] on the GPU (rows may be strided, columns not) ordered by group, int64
    ``offsets`` [G + 1] and the float32 ``pivot`` [d] -> (s float64 [G, d], M float64 [G, d (d + 1) / 2]) on the device: per
    group the sum of x - pivot and the packed upper triangle of the sum of (x - pivot)(x - pivot)^T, the differences formed
    in fp64.  Inputs must be finite.  ``path``: "auto" (the launcher's rule) or "d16" / "d32" / "d64" / "d128", the
    instances of the segment kernel -- equal bits."""
    _need_cuda("group_moments", x_sorted, offsets, pivot)
    path = _path("group_moments", GAUSSCLF_PATHS, path)
    if x_sorted.dtype != torch.float32 or x_sorted.dim() != 2 or offsets.dtype != torch.int64 or offsets.dim() != 1:
        raise TypeError("group_moments: x_sorted must be float32 [n, d] and offsets int64 [G + 1]")
    n, d = (int(v) for v in x_sorted.shape)
    if pivot.dtype != torch.float32 or tuple(pivot.shape) != (d,):
        raise TypeError(f"group_moments: pivot must be float32 [{d}]")
    x = _row_major(x_sorted)
    off, piv = offsets.contiguous(), pivot.contiguous()
    G = int(off.numel()) - 1
    s = torch.empty(max(G, 0), d, dtype=torch.float64, device=x.device)
    M = torch.empty(max(G, 0), d * (d + 1) // 2, dtype=torch.float64, device=x.device)
    ws_bytes = int(lib().mmvae_group_moments_workspace_bytes(n, d, G))
    ws = _workspace(ws_bytes, x.device)
    check(lib().mmvae_debug_group_moments(_ptr(x), int(x.stride(0)), n, d, _ptr(off), G, _ptr(piv), _ptr(ws), ws_bytes, _ptr(s),
                                          _ptr(M), path, _stream(x.device)), "mmvae_group_moments")
    return s, M


def gauss_scores(x: torch.Tensor, model: torch.Tensor, mu: torch.Tensor, W: torch.Tensor, c0: torch.Tensor,
                 perm: Optional[torch.Tensor] = None, return_scores: bool = False):
    """mmvae_gauss_scores: float32 points [n, d] on the GPU (rows may be strided, columns not), the int32 ``model`` [n] of
    every row (sort the rows by it), float64 ``mu`` [F, K, d], ``W`` [F, K, d, d] and ``c0`` [F, K] and, optionally, the
    int64 permutation ``perm`` [n] (row r is the caller's row perm[r]) -> (label int32 [n], best float64 [n], second
    float64 [n], scores float64 [n, K] or None) on the device, in the caller's order:
    score = c0 - |W^T (x - mu)|^2 / 2 under the row's own model, label its arg-max (the lowest index on ties)."""
    _need_cuda("gauss_scores", x, model, mu, W, c0, perm)
    if x.dtype != torch.float32 or x.dim() != 2:
        raise TypeError("gauss_scores: x must be float32 [n, d]")
    n, d = (int(v) for v in x.shape)
    if c0.dtype != torch.float64 or c0.dim() != 2:
        raise TypeError("gauss_scores: c0 must be float64 [F, K]")
    F, K = (int(v) for v in c0.shape)
    if mu.dtype != torch.float64 or tuple(mu.shape) != (F, K, d) or W.dtype != torch.float64 or tuple(W.shape) != (F, K, d, d):
        raise TypeError(f"gauss_scores: mu must be float64 [{F}, {K}, {d}] and W float64 [{F}, {K}, {d}, {d}]")
    if model.dtype != torch.int32 or tuple(model.shape) != (n,):
        raise TypeError(f"gauss_scores: model must be int32 [{n}]")
    if perm is not None:
        if perm.dtype != torch.int64 or tuple(perm.shape) != (n,):
            raise TypeError(f"gauss_scores: perm must be int64 [{n}]")
        perm = perm.contiguous()
    xs = _row_major(x)
    mu, W, c0, model = mu.contiguous(), W.contiguous(), c0.contiguous(), model.contiguous()
    label = torch.empty(n, dtype=torch.int32, device=xs.device)
    best = torch.empty(n, dtype=torch.float64, device=xs.device)
    second = torch.empty(n, dtype=torch.float64, device=xs.device)
    scores = torch.empty(n, K, dtype=torch.float64, device=xs.device) if return_scores else None
    check(lib().mmvae_gauss_scores(_ptr(xs), int(xs.stride(0)), n, d, _ptr(model), F, K, _ptr(mu), _ptr(W), _ptr(c0), _ptr(perm),
                                   None, 0, _ptr(label), _ptr(best), _ptr(second), _ptr(scores), _stream(xs.device)),
          "mmvae_gauss_scores")
    return label, best, second, scores


# launch_leaf_merge (csrc/leafmerge.hip; the constants are those of csrc/common.hpp)
LEAFMERGE_WAVES = 4             # LM_WAVES: waves per workgroup of both kernels, one cell a wave
LEAFMERGE_MAX_L, LEAFMERGE_MAX_K, LEAFMERGE_MAX_T = GAUSSCLF_MAX_K, 4096, 4096


def merge_tables(levels):
    """The three int32 tables of ``mmvae_leaf_merge`` from ``levels``, a list over the merge levels of lists over the labels
    of lists of leaf indices -> (level_start [T + 1], start [K_total + 1], leaf [nnz]), numpy arrays on the host."""
    level_start, start, leaf = [0], [0], []
    for labels in levels:
        for members in labels:
            leaf.extend(int(v) for v in members)
            start.append(len(leaf))
        level_start.append(len(start) - 1)
    return np.array(level_start, dtype=np.int32), np.array(start, dtype=np.int32), np.array(leaf, dtype=np.int32)


def leaf_merge(p: torch.Tensor, level_start, start, leaf, return_second: bool = True, return_merged: bool = False):
    """mmvae_leaf_merge: the float64 scores ``p`` [n, L] on the GPU (rows may be strided, columns not; -inf for a leaf without
    a model) BECOME THE POSTERIORS IN PLACE, and the merge tables (``merge_tables``; int arrays on the host, uploaded here)
    -> (label int32 [T, n], prob float64 [T, n], second float64 [T, n] or None, merged float64 [n, K_0] or None) on the
    device: per level the arg-max over its labels of the posteriors added over each label's leaves, that sum, the largest
    sum among the other labels, and every sum of level 0.  The tables are checked here, where they can be read: ValueError
    unless they are non-decreasing from 0, every level has a label and every leaf is a column of ``p``."""
    _need_cuda("leaf_merge", p)
    if p.dtype != torch.float64 or p.dim() != 2:
        raise TypeError("leaf_merge: p must be float64 [n, L]")
    if p.shape[1] > 1 and p.stride(1) != 1 or p.shape[0] > 1 and p.stride(0) < p.shape[1]:
        raise TypeError("leaf_merge: p is written in place: its columns must be contiguous")
    n, L = (int(v) for v in p.shape)
    ls, st, lf = (np.asarray(a) for a in (level_start, start, leaf))
    if any(a.ndim != 1 or (a.size and a.dtype.kind not in "iu") for a in (ls, st, lf)) or ls.size < 2 or st.size < 2:
        raise TypeError("leaf_merge: level_start [T + 1], start [K_total + 1] and leaf [nnz] must be 1-D integer arrays")
    ls, st, lf = ls.astype(np.int64), st.astype(np.int64), lf.astype(np.int64)
    T, K_total, nnz = ls.size - 1, st.size - 1, lf.size
    sizes = np.diff(ls)
    if ls[0] != 0 or ls[-1] != K_total or (sizes < 1).any():
        raise ValueError("leaf_merge: level_start must rise from 0 to the number of labels, every level with a label")
    if st[0] != 0 or st[-1] != nnz or (np.diff(st) < 0).any():
        raise ValueError("leaf_merge: start must be non-decreasing from 0 to the number of leaf entries")
    if nnz and (lf.min() < 0 or lf.max() >= L):
        raise ValueError(f"leaf_merge: a leaf index outside [0, L = {L})")
    dev = p.device
    i32 = lambda a: torch.from_numpy(a.astype(np.int32)).to(dev)
    d_ls, d_st = i32(ls), i32(st)
    d_lf = i32(lf) if nnz else torch.zeros(1, dtype=torch.int32, device=dev)
    K_max, K0 = int(sizes.max()), int(sizes[0])
    label = torch.empty(T, n, dtype=torch.int32, device=dev)
    prob = torch.empty(T, n, dtype=torch.float64, device=dev)
    second = torch.empty(T, n, dtype=torch.float64, device=dev) if return_second else None
    merged = torch.empty(n, K0, dtype=torch.float64, device=dev) if return_merged else None
    check(lib().mmvae_leaf_merge(_ptr(p), int(p.stride(0)) if n > 1 else max(L, 1), n, L, _ptr(d_ls), T, _ptr(d_st), K_total, K_max,
                                 _ptr(d_lf), nnz, None, 0, _ptr(label), _ptr(prob), _ptr(second), _ptr(merged), K0,
                                 _stream(dev)), "mmvae_leaf_merge")
    return label, prob, second, merged


# zero-inflated negative binomial inference (csrc/zinb.hip)
ZINB_MAX_H = 128                # ZB_MAX_H: the K extent one LDS tile holds


def _zinb_mat(what: str, name: str, t: torch.Tensor, cols: Optional[int] = None) -> torch.Tensor:
    if t.dtype != torch.float32 or t.dim() != 2 or (cols is not None and t.shape[1] != cols):
        raise TypeError(f"{what}: {name} must be float32 [n, {cols if cols is not None else 'width'}]; got {t.dtype} {tuple(t.shape)}")
    return _row_major(t)


def _zinb_pitch(t: torch.Tensor) -> int:
    return int(t.stride(0)) if t.shape[0] > 1 else int(t.shape[1])


def _zinb_layer(what: str, name: str, W: torch.Tensor, b: torch.Tensor, D: int, H: int):
    if W.dtype != torch.float32 or b.dtype != torch.float32 or tuple(W.shape) != (D, H) or tuple(b.shape) != (D,):
        raise TypeError(f"{what}: {name} must be a float32 weight [{D}, {H}] and bias [{D}]")
    return W.contiguous(), b.contiguous()


def _zinb_inputs(what: str, d10, W, b, Wp, bp, Wr, br, X, eps, scale=None, heads=None, segments: int = 0):
    """What the entries on d10 [N, H], the three layers and X [N, D] check and pass alike -> (keep, n, H, D, dev, mask, args).
    ``args`` are the leading ctypes arguments: mmvae_zinb_nll's 14, through eps, with ``heads=None``; else the gradient
    entries' 17, through ``scale`` (None: 1 / (N D)), the head mask and ``segments``.  ``keep`` holds the tensors the
    pointers belong to: the caller keeps it until the call has been made."""
    mask = zinb_head_mask(heads) if heads is not None else None
    _need_cuda(what, d10, W, b, Wp, bp, Wr, br, X)
    d10 = _zinb_mat(what, "d10", d10)
    n, H = (int(v) for v in d10.shape)
    D = int(W.shape[0])
    X = _zinb_mat(what, "X", X, D)
    if X.shape[0] != n:
        raise ValueError(f"{what}: X has {X.shape[0]} rows, d10 has {n}")
    if segments < 0:
        raise ValueError(f"{what}: segments = {segments} below 0")
    layers = [t for nm, Wj, bj in (("fc11", W, b), ("fc11_p", Wp, bp), ("fc11_r", Wr, br)) for t in _zinb_layer(what, nm, Wj, bj, D, H)]
    args = [_ptr(d10), _zinb_pitch(d10), n, H, D, *(_ptr(t) for t in layers), _ptr(X), _zinb_pitch(X), float(eps)]
    if heads is not None:
        args += [1.0 / (float(n) * float(D)) if scale is None else float(scale), mask, int(segments)]
    return (d10, X, layers), n, H, D, d10.device, mask, args


def _zinb_given_heads(what: str, x_rec, x_p, x_r, X, eps):
    """What mmvae_zinb_terms and mmvae_zinb_terms_grad check and pass alike: four float32 [N, D] matrices
    -> (keep, n, D, dev, args), ``args`` the leading ctypes arguments through eps."""
    _need_cuda(what, x_rec, x_p, x_r, X)
    X = _zinb_mat(what, "X", X)
    n, D = (int(v) for v in X.shape)
    x_rec, x_p, x_r = (_zinb_mat(what, nm, t, D) for nm, t in (("rec_x", x_rec), ("x_p", x_p), ("x_r", x_r)))
    if not (x_rec.shape[0] == x_p.shape[0] == x_r.shape[0] == n):
        raise ValueError(f"{what}: the four matrices must have the same number of rows")
    keep = (x_rec, x_p, x_r, X)
    return keep, n, D, X.device, [v for t in keep for v in (_ptr(t), _zinb_pitch(t))] + [n, D, float(eps)]


def _zinb_sums(n: int, D: int, dev):
    return torch.empty(n, dtype=torch.float64, device=dev), torch.empty(D, dtype=torch.float64, device=dev)


def zinb_head_layout(dims: Dims) -> ZinbHeadLayout:
    """mmvae_zinb_head_layout: the offsets of the p and r heads in their flat buffer (host only)."""
    out = ZinbHeadLayout()
    check(lib().mmvae_zinb_head_layout(C.byref(dims), C.byref(out)), "mmvae_zinb_head_layout")
    return out


def zinb_step_workspace_bytes(dims: Dims, ex: Optional[Exec] = None) -> int:
    """mmvae_zinb_step_workspace_bytes (host only); 0 for dimensions the ZINB step refuses."""
    return int(lib().mmvae_zinb_step_workspace_bytes(C.byref(dims), C.byref(ex) if ex is not None else None))


def zinb_heads(d10: torch.Tensor, Wp, bp, Wr, br):
    """mmvae_zinb_heads: (sigmoid(d10 Wp^T + bp), sigmoid(d10 Wr^T + br)), float32 [N, D] each, from float32 d10 [N, H] on
    the GPU (rows may be strided) and two ``nn.Linear`` layers' weight [D, H] and bias [D]."""
    what = "zinb_heads"
    _need_cuda(what, d10, Wp, bp, Wr, br)
    d10 = _zinb_mat(what, "d10", d10)
    n, H = (int(v) for v in d10.shape)
    D = int(Wp.shape[0])
    (Wp, bp), (Wr, br) = _zinb_layer(what, "fc11_p", Wp, bp, D, H), _zinb_layer(what, "fc11_r", Wr, br, D, H)
    x_p = torch.empty(n, D, dtype=torch.float32, device=d10.device)
    x_r = torch.empty_like(x_p)
    with torch.cuda.device(d10.device):
        check(lib().mmvae_zinb_heads(_ptr(d10), _zinb_pitch(d10), n, H, D, _ptr(Wp), _ptr(bp), _ptr(Wr), _ptr(br), _ptr(x_p),
                                     _ptr(x_r), D, _stream(d10.device)), "mmvae_zinb_heads")
    return x_p, x_r


def zinb_nll(d10: torch.Tensor, W, b, Wp, bp, Wr, br, X: torch.Tensor, eps: float = 1e-6):
    """mmvae_zinb_nll: the ZINB term of every element of X [N, D] under the three heads of d10 [N, H] (fc11: W, b; fc11_p: Wp,
    bp; fc11_r: Wr, br), summed -> (cell_sum float64 [N], gene_sum float64 [D]) on the device; no head is written."""
    what = "zinb_nll"
    keep, n, H, D, dev, _, args = _zinb_inputs(what, d10, W, b, Wp, bp, Wr, br, X, eps)
    with torch.cuda.device(dev):
        nbytes = int(lib().mmvae_zinb_nll_workspace_bytes(n, D))
        ws = _workspace(nbytes, dev)
        cell, gene = _zinb_sums(n, D, dev)
        check(lib().mmvae_zinb_nll(*args, _ptr(ws), nbytes, _ptr(cell), _ptr(gene), _stream(dev)), "mmvae_zinb_nll")
    return cell, gene


def zinb_terms(x_rec: torch.Tensor, x_p: torch.Tensor, x_r: torch.Tensor, X: torch.Tensor, eps: float = 1e-6,
               return_terms: bool = False):
    """mmvae_zinb_terms: the ZINB term of every element from given heads (float32 [N, D] on the GPU, rows may be strided)
    -> (cell_sum float64 [N], gene_sum float64 [D], terms float32 [N, D] or None) on the device."""
    what = "zinb_terms"
    keep, n, D, dev, args = _zinb_given_heads(what, x_rec, x_p, x_r, X, eps)
    with torch.cuda.device(dev):
        nbytes = int(lib().mmvae_zinb_terms_workspace_bytes(n, D))
        ws = _workspace(nbytes, dev)
        cell, gene = _zinb_sums(n, D, dev)
        terms = torch.empty(n, D, dtype=torch.float32, device=dev) if return_terms else None
        check(lib().mmvae_zinb_terms(*args, _ptr(ws), nbytes, _ptr(cell), _ptr(gene), _ptr(terms), D, _stream(dev)), "mmvae_zinb_terms")
    return cell, gene, terms


# gradients of the ZINB term with respect to the heads (csrc/zinb_grad.hip)
ZINB_HEADS = ("rec", "p", "r")          # fc11, fc11_p, fc11_r: bits 1, 2, 4 of the head mask
ZINB_PSI_SERIES = 10.0                  # ZB_PSI_SERIES: where psi leaves the recurrence for the asymptotic series


def zinb_head_mask(heads) -> int:
    """The 3-bit mask of a selection of ``ZINB_HEADS``; ValueError for an unknown name or an empty selection."""
    heads = (heads,) if isinstance(heads, str) else tuple(heads)
    bad = [h for h in heads if h not in ZINB_HEADS]
    if bad or not heads:
        raise ValueError(f"heads must be a non-empty selection of {ZINB_HEADS}; got {heads!r}")
    return sum(1 << ZINB_HEADS.index(h) for h in set(heads))


def _zinb_head_outputs(what: str, mask: int, out, D: int, H: int, dev):
    """The per-head outputs of a gradient entry -> (grads, ptrs): ``grads`` ``{head: (dW [D, H], db [D])}`` of the selected
    heads, taken from ``out`` (checked) or new; ``ptrs`` the six tensors or None in the order of the C arguments."""
    grads, ptrs = {}, []
    for j, h in enumerate(ZINB_HEADS):
        if not mask >> j & 1:
            ptrs += list(out[h]) if out is not None and h in out else [None, None]     # handed on, never written
            continue
        if out is not None:
            dW, db = out[h]
            if (dW.dtype != torch.float32 or db.dtype != torch.float32 or tuple(dW.shape) != (D, H) or tuple(db.shape) != (D,)
                    or not dW.is_contiguous() or not db.is_contiguous() or dW.device != dev or db.device != dev):
                raise TypeError(f"{what}: out[{h!r}] must be contiguous float32 ([{D}, {H}], [{D}]) on {dev}")
        else:
            dW = torch.empty(D, H, dtype=torch.float32, device=dev)
            db = torch.empty(D, dtype=torch.float32, device=dev)
        grads[h] = (dW, db)
        ptrs += [dW, db]
    return grads, ptrs


def zinb_head_grads_segments(n: int, D: int, segments: int = 0) -> int:
    """The number of cell segments mmvae_zinb_head_grads uses for n cells and D genes when ``segments`` are asked for
    (0: the library's rule)."""
    return int(lib().mmvae_zinb_head_grads_segments(int(n), int(D), int(segments)))


def zinb_head_grads(d10: torch.Tensor, W, b, Wp, bp, Wr, br, X: torch.Tensor, eps: float = 1e-6, scale: Optional[float] = None,
                    heads=ZINB_HEADS, segments: int = 0, out=None):
    """mmvae_zinb_head_grads: the gradient of ``scale`` x the sum of the ZINB terms of X [N, D] under the three heads of d10
    [N, H] with respect to the weights and biases of the heads in ``heads`` ("rec": fc11, "p": fc11_p, "r": fc11_r).
    ``scale=None`` is 1 / (N D), the mean that ``zinb_loss`` returns.  ``segments``: the number of cell segments, 0 the
    library's rule.  ``out``: ``{head: (dW float32 [D, H], db float32 [D])}`` to write into (contiguous, on the device;
    views of one flat buffer will do), by default new tensors.  Returns ``(grads, cell_sum, gene_sum)``: ``grads`` as ``out``
    with the selected heads only; the float64 sums are mmvae_zinb_nll's bit for bit."""
    what = "zinb_head_grads"
    keep, n, H, D, dev, mask, args = _zinb_inputs(what, d10, W, b, Wp, bp, Wr, br, X, eps, scale, heads, segments)
    grads, ptrs = _zinb_head_outputs(what, mask, out, D, H, dev)
    with torch.cuda.device(dev):
        nbytes = int(lib().mmvae_zinb_head_grads_workspace_bytes(n, D, H, int(segments)))
        ws = _workspace(nbytes, dev)
        cell, gene = _zinb_sums(n, D, dev)
        check(lib().mmvae_zinb_head_grads(*args, _ptr(ws), nbytes, *(_ptr(t) for t in ptrs), _ptr(cell), _ptr(gene), _stream(dev)),
              "mmvae_zinb_head_grads")
    return grads, cell, gene


def zinb_d10_grad_segments(n: int, D: int, segments: int = 0) -> int:
    """The number of gene segments mmvae_zinb_d10_grad uses for n cells and D genes when ``segments`` are asked for (0: the
    library's rule)."""
    return int(lib().mmvae_zinb_d10_grad_segments(int(n), int(D), int(segments)))


def zinb_d10_grad(d10: torch.Tensor, W, b, Wp, bp, Wr, br, X: torch.Tensor, eps: float = 1e-6, heads=ZINB_HEADS, segments: int = 0,
                  scale: Optional[float] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """mmvae_zinb_d10_grad: the gradient of ``scale`` x the sum of the ZINB terms of X [N, D] with respect to d10 [N, H] through
    the heads in ``heads`` (an unselected head still shapes the likelihood; its own path to d10 is left out).  ``scale=None``
    is 1 / (N D); ``segments``: the number of gene segments, 0 the library's rule; ``out``: float32 [N, H] on the device to
    write into (rows may be strided).  Returns gd10 float32 [N, H]."""
    what = "zinb_d10_grad"
    keep, n, H, D, dev, _, args = _zinb_inputs(what, d10, W, b, Wp, bp, Wr, br, X, eps, scale, heads, segments)
    if out is None:
        out = torch.empty(n, H, dtype=torch.float32, device=dev)
    elif (out.dtype != torch.float32 or tuple(out.shape) != (n, H) or out.device != dev or out.stride(1) != 1
          or (n > 1 and out.stride(0) < H)):
        raise TypeError(f"{what}: out must be float32 [{n}, {H}] on {dev} with unit column stride")
    with torch.cuda.device(dev):
        nbytes = int(lib().mmvae_zinb_d10_grad_workspace_bytes(n, D, H, int(segments)))
        ws = _workspace(nbytes, dev)
        check(lib().mmvae_zinb_d10_grad(*args, _ptr(ws), nbytes, _ptr(out), _zinb_pitch(out), _stream(dev)), "mmvae_zinb_d10_grad")
    return out


TRUNK_LAYERS = ("fc6", "fc7", "fc8", "fc9", "fc10")


def zinb_step_grads(d10: torch.Tensor, W, b, Wp, bp, Wr, br, X: torch.Tensor, eps: float = 1e-6, scale: Optional[float] = None,
                    heads=ZINB_HEADS, segments: int = 0):
    """mmvae_zinb_step_grads: ``zinb_head_grads`` (at ``segments`` cell segments) and ``zinb_d10_grad`` (at a segment a gene
    tile) from one evaluation of g.  Returns ``(grads, cell_sum, gene_sum, gd10)``, each bit for bit what the two give."""
    what = "zinb_step_grads"
    keep, n, H, D, dev, mask, args = _zinb_inputs(what, d10, W, b, Wp, bp, Wr, br, X, eps, scale, heads, segments)
    grads, ptrs = _zinb_head_outputs(what, mask, None, D, H, dev)
    with torch.cuda.device(dev):
        nbytes = int(lib().mmvae_zinb_step_grads_workspace_bytes(n, D, H, int(segments)))
        ws = _workspace(nbytes, dev)
        cell, gene = _zinb_sums(n, D, dev)
        gd10 = torch.empty(n, H, dtype=torch.float32, device=dev)
        check(lib().mmvae_zinb_step_grads(*args, _ptr(ws), nbytes, *(_ptr(t) for t in ptrs), _ptr(cell), _ptr(gene), _ptr(gd10), H,
                                          _stream(dev)), "mmvae_zinb_step_grads")
    return grads, cell, gene, gd10


def decoder_trunk_grads_segments(n: int, segments: int = 0) -> int:
    """The number of cell segments mmvae_decoder_trunk_grads uses for n cells when ``segments`` are asked for (0: the rule)."""
    return int(lib().mmvae_decoder_trunk_grads_segments(int(n), int(segments)))


def decoder_trunk_grads(acts, params, gd10: torch.Tensor, segments: int = 0, out=None, want_gzin: bool = True):
    """mmvae_decoder_trunk_grads: the backward of one arm's decoder trunk.  ``acts``: (zin [N, C+S], d6 [N, L], d7, d8, d9, d10
    [N, H]) float32 on the device as an eval forward leaves them (rows may be strided); ``params``: the ten tensors
    fc6.weight, fc6.bias .. fc10.weight, fc10.bias in ``nn.Linear``'s layout; ``gd10`` float32 [N, H].  ``out``: ten
    contiguous float32 tensors of the parameters' shapes to write into (views of one flat buffer will do), by default new
    ones.  Returns ``(grads, gzin)``: the ten gradients in the order of ``params`` and the gradient with respect to zin
    [N, C+S] (None with ``want_gzin=False``)."""
    what = "decoder_trunk_grads"
    acts, params = list(acts), list(params)
    if len(acts) != 6 or len(params) != 10:
        raise ValueError(f"{what}: needs six activations (zin, d6 .. d10) and ten parameter tensors (fc6.weight .. fc10.bias)")
    _need_cuda(what, *acts, *params, gd10)
    acts = [_zinb_mat(what, nm, t) for nm, t in zip(("zin", "d6", "d7", "d8", "d9", "d10"), acts)]
    n = int(acts[0].shape[0])
    Z, L, H = int(acts[0].shape[1]), int(acts[1].shape[1]), int(acts[2].shape[1])
    width = [Z, L, H, H, H, H]
    if any(tuple(a.shape) != (n, w) for a, w in zip(acts, width)):
        raise ValueError(f"{what}: the activations must be [{n}, w] with w = {width}; got {[tuple(a.shape) for a in acts]}")
    gd10 = _zinb_mat(what, "gd10", gd10, H)
    if gd10.shape[0] != n:
        raise ValueError(f"{what}: gd10 has {gd10.shape[0]} rows, the activations have {n}")
    if not 0 <= int(segments) <= 1024:
        raise ValueError(f"{what}: segments = {segments} outside [0, 1024]")
    dev = gd10.device
    shapes = [s for l in range(5) for s in ((width[l + 1], width[l]), (width[l + 1],))]
    for k, (p, s) in enumerate(zip(params, shapes)):
        if p.dtype != torch.float32 or tuple(p.shape) != s:
            raise TypeError(f"{what}: {TRUNK_LAYERS[k // 2]}.{'bias' if k % 2 else 'weight'} must be float32 {s}; got {p.dtype} "
                            f"{tuple(p.shape)}")
    params = [p.contiguous() for p in params]
    if out is None:
        out = [torch.empty(s, dtype=torch.float32, device=dev) for s in shapes]
    else:
        out = list(out)
        if len(out) != 10 or any(g.dtype != torch.float32 or tuple(g.shape) != s or not g.is_contiguous() or g.device != dev
                                 for g, s in zip(out, shapes)):
            raise TypeError(f"{what}: out must be ten contiguous float32 tensors of the parameters' shapes on {dev}")
    gzin = torch.empty(n, Z, dtype=torch.float32, device=dev) if want_gzin else None
    vp6, vp10 = C.c_void_p * 6, C.c_void_p * 10
    with torch.cuda.device(dev):
        nbytes = int(lib().mmvae_decoder_trunk_grads_workspace_bytes(n, Z, L, H, int(segments)))
        ws = _workspace(nbytes, dev)
        check(lib().mmvae_decoder_trunk_grads(n, Z, L, H, vp6(*(_ptr(a) for a in acts)), (C.c_int64 * 6)(*(_zinb_pitch(a) for a in acts)),
                                              vp10(*(_ptr(p) for p in params)), _ptr(gd10), _zinb_pitch(gd10), int(segments),
                                              _ptr(ws), nbytes, vp10(*(_ptr(g) for g in out)), _ptr(gzin), Z, _stream(dev)),
              "mmvae_decoder_trunk_grads")
    return out, gzin


def zinb_terms_grad(x_rec: torch.Tensor, x_p: torch.Tensor, x_r: torch.Tensor, X: torch.Tensor, eps: float = 1e-6,
                    scale: float = 1.0):
    """mmvae_zinb_terms_grad: ``scale`` x the gradient of every element's ZINB term with respect to the given heads (float32
    [N, D] on the GPU, rows may be strided) -> (g_rec, g_p, g_r) float32 [N, D] on the device."""
    what = "zinb_terms_grad"
    keep, n, D, dev, args = _zinb_given_heads(what, x_rec, x_p, x_r, X, eps)
    with torch.cuda.device(dev):
        g = [torch.empty(n, D, dtype=torch.float32, device=dev) for _ in range(3)]
        check(lib().mmvae_zinb_terms_grad(*args, float(scale), _ptr(g[0]), _ptr(g[1]), _ptr(g[2]), D, _stream(dev)),
              "mmvae_zinb_terms_grad")
    return tuple(g)


def debug_zinb_grad_host(X, a_rec, a_p, a_r, eps: float = 1e-6):
    """mmvae_debug_zinb_grad_host: the kernels' element code on the host, no GPU.  float32 arrays of one shape: X and the three
    pre-activations -> (g float64 [3, ...] = d term / d (a_rec, a_p, a_r) before the rounding, term float64 [...])."""
    arrs = [np.ascontiguousarray(np.asarray(t, dtype=np.float32)) for t in (X, a_rec, a_p, a_r)]
    if any(a.shape != arrs[0].shape for a in arrs) or arrs[0].size == 0:
        raise ValueError("debug_zinb_grad_host: X, a_rec, a_p, a_r must have one non-empty shape")
    g = np.empty((3,) + arrs[0].shape, dtype=np.float64)
    term = np.empty(arrs[0].shape, dtype=np.float64)
    check(lib().mmvae_debug_zinb_grad_host(arrs[0].size, *(a.ctypes.data for a in arrs), float(eps), g.ctypes.data, term.ctypes.data),
          "mmvae_debug_zinb_grad_host")
    return g, term


def debug_digamma_host(x):
    """mmvae_debug_digamma_host: the kernels' psi on the host, float64 in and out."""
    x = np.ascontiguousarray(np.asarray(x, dtype=np.float64))
    if x.size == 0:
        raise ValueError("debug_digamma_host: empty input")
    out = np.empty_like(x)
    check(lib().mmvae_debug_digamma_host(x.size, x.ctypes.data, out.ctypes.data), "mmvae_debug_digamma_host")
    return out


# count distributions (csrc/countdist.hip)
COUNT_KINDS = {"nb": 0, "zinb": 1, "mixture": 2}
COUNT_ZI = {None: 0, "logits": 1, "probs": 2}


def _count_theta(what: str, name: str, t: torch.Tensor, n: int, D: int):
    """(theta as the kernels read it, its pitch): float32 [D] (pitch 0) or [n, D]."""
    if t.dtype == torch.float32 and t.dim() == 1 and t.shape[0] == D:
        return t.contiguous(), 0
    if t.dim() != 2 or t.shape[0] != n:
        raise ValueError(f"{what}: {name} must be float32 [{D}] or [{n}, {D}]; got {t.dtype} {tuple(t.shape)}")
    t = _zinb_mat(what, name, t, D)
    return t, _zinb_pitch(t)


def _count_mat(what: str, name: str, t: torch.Tensor, n: int, D: int):
    t = _zinb_mat(what, name, t, D)
    if t.shape[0] != n:
        raise ValueError(f"{what}: {name} has {t.shape[0]} rows where {n} are expected")
    return t, _zinb_pitch(t)


def count_logp(kind: str, x: torch.Tensor, mu: torch.Tensor, theta: torch.Tensor, pi: Optional[torch.Tensor] = None,
               mu2: Optional[torch.Tensor] = None, theta2: Optional[torch.Tensor] = None, eps: float = 1e-8,
               return_terms: bool = True, return_sums: bool = False):
    """mmvae_count_logp: the log-likelihood of every element of x [N, D] (float32 on the GPU, rows may be strided) under NB
    (``kind`` "nb"), ZINB ("zinb": ``pi`` the zero-inflation logits) or the NB mixture ("mixture": ``mu2``, optional ``theta2``,
    ``pi`` the mixture logits); theta float32 [D] or [N, D].  -> (terms float32 [N, D] or None, cell_sum float64 [N] or None,
    gene_sum float64 [D] or None) on the device."""
    what = "count_logp"
    if kind not in COUNT_KINDS:
        raise ValueError(f"{what}: kind must be one of {sorted(COUNT_KINDS)}; got {kind!r}")
    if (pi is None) != (kind == "nb") or (mu2 is None) != (kind != "mixture") or (theta2 is not None and kind != "mixture"):
        raise ValueError(f"{what}: kind {kind!r} takes pi for zinb and mixture, mu2 (and theta2) for mixture only")
    _need_cuda(what, x, mu, theta, pi, mu2, theta2)
    x = _zinb_mat(what, "x", x)
    n, D = (int(v) for v in x.shape)
    a = CountLogp(kind=COUNT_KINDS[kind], N=n, D=D, eps=float(eps), x=x.data_ptr(), ldx=_zinb_pitch(x))
    keep = [x]
    for name, t, vec in (("mu", mu, False), ("theta", theta, True), ("pi", pi, False), ("mu2", mu2, False), ("theta2", theta2, True)):
        if t is None:
            continue
        t, ld = _count_theta(what, name, t, n, D) if vec else _count_mat(what, name, t, n, D)
        keep.append(t)
        setattr(a, name, t.data_ptr())
        setattr(a, "ld_" + name, ld)
    dev = x.device
    with torch.cuda.device(dev):
        terms = torch.empty(n, D, dtype=torch.float32, device=dev) if return_terms else None
        cell = gene = ws = None
        nbytes = 0
        if return_sums:
            nbytes = int(lib().mmvae_count_logp_workspace_bytes(n, D))
            ws = _workspace(nbytes, dev)
            cell = torch.empty(n, dtype=torch.float64, device=dev)
            gene = torch.empty(D, dtype=torch.float64, device=dev)
            a.cell_sum, a.gene_sum = cell.data_ptr(), gene.data_ptr()
        if terms is not None:
            a.terms, a.ld_t = terms.data_ptr(), D
        check(lib().mmvae_count_logp(C.byref(a), _ptr(ws), nbytes, _stream(dev)), "mmvae_count_logp")
    return terms, cell, gene


def _count_sample_out(n: int, D: int, dev, out_int32: bool):
    return (torch.empty(n, D, dtype=torch.int32 if out_int32 else torch.float32, device=dev),
            torch.zeros(1, dtype=torch.int32, device=dev))


def _count_exhausted(what: str, counter: torch.Tensor):
    k = int(counter.item())
    if k:
        raise NativeError(f"{what}: {k} elements ran out of attempts in a bounded rejection loop and took the fallback value")


def count_sample(mu: torch.Tensor, theta: torch.Tensor, zi: Optional[torch.Tensor] = None, zi_kind: Optional[str] = None,
                 seed: int = 0, offset: int = 0, cell0: int = 0, out_int32: bool = False, log1p: bool = False,
                 heads_eps: Optional[float] = None):
    """mmvae_count_sample: one draw per element of NB(mu, theta) or, with ``zi`` (``zi_kind`` "logits" or "probs"), of
    ZINB(mu, theta, zi); mu float32 [N, D] on the GPU, theta [D] or [N, D].  With ``heads_eps`` the three arguments are the
    model's heads (x_rec, x_p, x_r) and are mapped under zinb_loss's eps guards.  Draws are keyed by (seed, offset,
    (cell0 + row) D + gene).  -> float32 (``log1p``: log1p of the count) or int32 [N, D]; raises if any element exhausted a
    bounded loop."""
    what = "count_sample"
    heads = heads_eps is not None
    if heads and (zi is None or zi_kind is not None):
        raise ValueError(f"{what}: the heads' mapping takes x_r as zi and no zi_kind")
    if not heads and ((zi is None) != (zi_kind is None) or zi_kind not in COUNT_ZI):
        raise ValueError(f"{what}: zi comes with zi_kind 'logits' or 'probs'; got zi_kind {zi_kind!r}")
    _need_cuda(what, mu, theta, zi)
    mu = _zinb_mat(what, "x_rec" if heads else "mu", mu)
    n, D = (int(v) for v in mu.shape)
    theta, ld_th = _count_mat(what, "x_p", theta, n, D) if heads else _count_theta(what, "theta", theta, n, D)
    s = CountSample(param=int(heads), zi_kind=0 if heads else COUNT_ZI[zi_kind], N=n, D=D, cell0=int(cell0),
                    eps=float(heads_eps) if heads else 0.0, seed=int(seed) & 0xFFFFFFFFFFFFFFFF, offset=int(offset),
                    a=mu.data_ptr(), ld_a=_zinb_pitch(mu), b=theta.data_ptr(), ld_b=ld_th, out_int32=int(out_int32),
                    log1p=int(log1p), ld_out=D)
    if zi is not None:
        zi, s.ld_zi = _count_mat(what, "x_r" if heads else "zi", zi, n, D)
        s.zi = zi.data_ptr()
    dev = mu.device
    with torch.cuda.device(dev):
        out, counter = _count_sample_out(n, D, dev, out_int32)
        s.out, s.exhausted = out.data_ptr(), counter.data_ptr()
        check(lib().mmvae_count_sample(C.byref(s), _stream(dev)), "mmvae_count_sample")
        _count_exhausted(what, counter)
    return out


def zinb_sample(d10: torch.Tensor, W, b, Wp, bp, Wr, br, seed: int, offset: int = 0, cell0: int = 0, eps: float = 1e-6,
                out_int32: bool = False, log1p: bool = False):
    """mmvae_zinb_sample: one ZINB draw per (cell, gene) under the three heads of d10 [N, H] (fc11: W, b; fc11_p: Wp, bp;
    fc11_r: Wr, br), the heads never written: bit for bit ``count_sample(x_rec, x_p, x_r, heads_eps=eps)`` on the heads that
    the decode and ``zinb_heads`` write.  -> float32 or int32 [N, D]."""
    what = "zinb_sample"
    _need_cuda(what, d10, W, b, Wp, bp, Wr, br)
    d10 = _zinb_mat(what, "d10", d10)
    n, H = (int(v) for v in d10.shape)
    D = int(W.shape[0])
    (W, b), (Wp, bp), (Wr, br) = (_zinb_layer(what, "fc11", W, b, D, H), _zinb_layer(what, "fc11_p", Wp, bp, D, H),
                                  _zinb_layer(what, "fc11_r", Wr, br, D, H))
    dev = d10.device
    with torch.cuda.device(dev):
        out, counter = _count_sample_out(n, D, dev, out_int32)
        s = CountSample(param=1, N=n, D=D, cell0=int(cell0), eps=float(eps), seed=int(seed) & 0xFFFFFFFFFFFFFFFF,
                        offset=int(offset), out_int32=int(out_int32), log1p=int(log1p), out=out.data_ptr(), ld_out=D,
                        exhausted=counter.data_ptr())
        check(lib().mmvae_zinb_sample(_ptr(d10), _zinb_pitch(d10), H, _ptr(W), _ptr(b), _ptr(Wp), _ptr(bp), _ptr(Wr), _ptr(br),
                                      C.byref(s), _stream(dev)), "mmvae_zinb_sample")
        _count_exhausted(what, counter)
    return out


# launch_forest (csrc/forest.hip; the constants are those of csrc/common.hpp)
FOREST_BINS = 256               # RF_BINS: bins of a feature
FOREST_MAX_D, FOREST_MAX_K, FOREST_MAX_F, FOREST_MAX_T, FOREST_MAX_N = 128, 128, 64, 4096, 1 << 24
FOREST_TREE_BYTES_PER_ROW = 56  # RF_TREE_BYTES_PER_ROW: a tree's node table, stack and index lists per row of the call
FOREST_CHUNK_BYTES = 1 << 30    # RF_CHUNK_BYTES: per-tree tables of one chunk of launches at most


def forest_chunk(n: int, F: int, T: int) -> int:
    """The trees of one chunk of launches (rf_chunk, csrc/forest.hip)."""
    return min(F * T, max(1, FOREST_CHUNK_BYTES // (FOREST_TREE_BYTES_PER_ROW * n + 4)))


def forest_cv(bins: torch.Tensor, codes: torch.Tensor, fold: torch.Tensor, K: int, F: int, T: int, mtry: int, seed: int,
              return_votes: bool = False, return_trees: bool = False):
    """mmvae_forest_cv: uint8 ``bins`` [n, d] on the GPU (rows may be strided, columns not), int32 ``codes`` [n] in [0, K) and
    ``fold`` [n] in [0, F) -> (label, best, second int32 [n], votes int32 [n, K] or None, trees or None) on the device:
    ``T`` trees a fold grown on the rows outside it, every row voted on by its own fold's trees.  trees = {"count": int32
    [F T], "nodes": int32 [F T, 2 n, 4]}: node j of tree g is (feature, thr, left child, rows) or (-1, class, 0, rows); rows
    past the count are zero."""
    _need_cuda("forest_cv", bins, codes, fold)
    if bins.dtype != torch.uint8 or bins.dim() != 2:
        raise TypeError("forest_cv: bins must be uint8 [n, d]")
    n, d = (int(v) for v in bins.shape)
    if codes.dtype != torch.int32 or tuple(codes.shape) != (n,) or fold.dtype != torch.int32 or tuple(fold.shape) != (n,):
        raise TypeError(f"forest_cv: codes and fold must be int32 [{n}]")
    b, codes, fold = _row_major(bins), codes.contiguous(), fold.contiguous()
    i32 = dict(dtype=torch.int32, device=b.device)
    label, best, second = (torch.empty(n, **i32) for _ in range(3))
    votes = torch.empty(n, K, **i32) if return_votes else None
    count = torch.zeros(F * T, **i32) if return_trees else None
    nodes = torch.zeros(F * T, 2 * n, 4, **i32) if return_trees else None
    ws_bytes = int(lib().mmvae_forest_workspace_bytes(n, d, F, K, T))
    ws = _workspace(ws_bytes, b.device)
    check(lib().mmvae_forest_cv(_ptr(b), int(b.stride(0)), n, d, _ptr(codes), _ptr(fold), K, F, T, mtry,
                                int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(ws), ws_bytes, _ptr(label), _ptr(best), _ptr(second),
                                _ptr(votes), _ptr(count), _ptr(nodes), _stream(b.device)), "mmvae_forest_cv")
    return label, best, second, votes, ({"count": count, "nodes": nodes} if return_trees else None)


# launch_gram / launch_symm_mul / launch_pca_project (csrc/pca.hip; the constants are those of csrc/common.hpp)
GRAM_TILE = 64                  # GRAM_TILE: rows and columns of G per workgroup
GRAM_KC = 32                    # GRAM_KC: rows staged in LDS at a time
GRAM_SEG_ROWS = 256             # GRAM_SEG_ROWS: rows per segment where the rows are cut, until GRAM_MAX_SEGS are in use
GRAM_MAX_SEGS = 3               # GRAM_MAX_SEGS: segments at most
GRAM_FILL_TILES = 256           # GRAM_FILL_TILES: upper-triangle tiles from which the rows are not cut
GRAM_MAX_D = 32768
PCA_MAX_BLOCK = 64              # RM_CHUNK: the most columns of Q (mmvae_symm_mul) and of V (mmvae_pca_project)
GRAM_PATHS = LOAD_PATHS
gram_wide = _wide16


def gram_segments(n: int, D: int) -> Tuple[int, int]:
    """(number of segments, rows per segment) that mmvae_gram cuts ``n`` rows of ``D`` columns into; (0, 0) where it refuses."""
    rows = C.c_int64(0)
    nseg = int(lib().mmvae_gram_segments(n, D, C.byref(rows)))
    return nseg, int(rows.value) if nseg else 0


def _rows_of(what: str, data: torch.Tensor, rows: Optional[torch.Tensor]):
    """(the matrix as the kernels read it, the row map or None, n) after the checks mmvae_gram and mmvae_pca_project share."""
    if data.dtype != torch.float32 or data.dim() != 2:
        raise TypeError(f"{what}: data must be float32 [n_total, D]")
    return (_row_major(data),) + _row_map(what, rows, int(data.shape[0]))


def gram(data: torch.Tensor, pivot: torch.Tensor, rows: Optional[torch.Tensor] = None, cov: bool = False,
         path: str = "auto") -> Tuple[torch.Tensor, torch.Tensor]:
    """mmvae_gram: float32 ``data`` [n_total, D] on the GPU (rows may be strided, columns not; read where it lies), the
    float32 ``pivot`` [D] and optionally the int64 row map ``rows`` [n] (None: every row) -> (s float64 [D], G float64
    [D, D]) on the device: with t = (double)x - (double)pivot, s = sum t and G = sum t t^T over the n rows, G exactly
    symmetric; with ``cov`` G is the unbiased covariance (G - s s^T / n) / (n - 1) instead.  Inputs must be finite.
    ``path``: "auto" (the launcher's rule), "narrow", "wide" -- the load forms, equal bits."""
    _need_cuda("gram", data, pivot, rows)
    path = _path("gram", GRAM_PATHS, path)
    x, rows, n = _rows_of("gram", data, rows)
    n_total, Dm = (int(v) for v in x.shape)
    if pivot.dtype != torch.float32 or tuple(pivot.shape) != (Dm,):
        raise TypeError(f"gram: pivot must be float32 [{Dm}]")
    piv = pivot.contiguous()
    s = torch.empty(Dm, dtype=torch.float64, device=x.device)
    G = torch.empty(Dm, Dm, dtype=torch.float64, device=x.device)
    ws_bytes = int(lib().mmvae_gram_workspace_bytes(n, Dm))
    ws = _workspace(ws_bytes, x.device)
    check(lib().mmvae_debug_gram(_ptr(x), int(x.stride(0)), n_total, _ptr(rows), n, Dm, _ptr(piv), _ptr(ws), ws_bytes, _ptr(s),
                                 _ptr(G), int(bool(cov)), path, _stream(x.device)), "mmvae_gram")
    return s, G


def symm_mul(Cm: torch.Tensor, Q: torch.Tensor) -> torch.Tensor:
    """mmvae_symm_mul: float64 ``Cm`` [D, D] (rows may be strided, columns not) times float64 ``Q`` [D, b], b <= 64, on the
    GPU -> Y float64 [D, b] on the device, every entry one fma chain in coordinate order."""
    _need_cuda("symm_mul", Cm, Q)
    if Cm.dtype != torch.float64 or Cm.dim() != 2 or Cm.shape[0] != Cm.shape[1]:
        raise TypeError("symm_mul: C must be float64 [D, D]")
    Dm = int(Cm.shape[0])
    if Q.dtype != torch.float64 or Q.dim() != 2 or int(Q.shape[0]) != Dm:
        raise TypeError(f"symm_mul: Q must be float64 [{Dm}, b]")
    Cc = _row_major(Cm)
    Qc = Q.contiguous()
    b = int(Q.shape[1])
    Y = torch.empty(Dm, b, dtype=torch.float64, device=Cc.device)
    check(lib().mmvae_symm_mul(_ptr(Cc), int(Cc.stride(0)), Dm, _ptr(Qc), b, _ptr(Y), _stream(Cc.device)), "mmvae_symm_mul")
    return Y


def pca_project(data: torch.Tensor, mean: torch.Tensor, V: torch.Tensor, rows: Optional[torch.Tensor] = None) -> torch.Tensor:
    """mmvae_pca_project: float32 ``data`` [n_total, D] on the GPU (read where it lies), float64 ``mean`` [D] and ``V``
    [D, k], k <= 64, optionally the int64 row map ``rows`` [n] -> Z float64 [n, k] on the device: ((double)x - mean) V, row r
    of Z the sample rows[r], every entry one fma chain in coordinate order."""
    _need_cuda("pca_project", data, mean, V, rows)
    x, rows, n = _rows_of("pca_project", data, rows)
    n_total, Dm = (int(v) for v in x.shape)
    if mean.dtype != torch.float64 or tuple(mean.shape) != (Dm,) or V.dtype != torch.float64 or V.dim() != 2 or int(V.shape[0]) != Dm:
        raise TypeError(f"pca_project: mean must be float64 [{Dm}] and V float64 [{Dm}, k]")
    mean, V = mean.contiguous(), V.contiguous()
    k = int(V.shape[1])
    Z = torch.empty(n, k, dtype=torch.float64, device=x.device)
    check(lib().mmvae_pca_project(_ptr(x), int(x.stride(0)), n_total, _ptr(rows), n, Dm, _ptr(mean), _ptr(V), k, _ptr(Z),
                                  _stream(x.device)), "mmvae_pca_project")
    return Z


# launch_cpm_dense / launch_cpm_csr / launch_gene_stats (csrc/dataprep.hip; the constants are those of csrc/common.hpp)
CPM_THREADS = 256               # CPM_THREADS: threads of the workgroup that owns a selected row
CPM_WINDOW = 4096               # CPM_WINDOW: columns of the dense row that the CSR kernel rebuilds in LDS at a time
CPM_MAX_G = 1 << 20             # CPM_MAX_G: genes at most
GENESTATS_SEG_ROWS = 256        # GS_SEG_ROWS: rows per segment
GENESTATS_TILE = 256            # GS_TILE: genes per wave, four consecutive genes a lane
CPM_VTYPES = {torch.int32: 0, torch.float32: 1, torch.float64: 2}
CPM_OTYPES = {torch.float32: 0, torch.float64: 1}
CPM_PATHS = GENESTATS_PATHS = LOAD_PATHS
cpm_wide = _wide16              # (the rule of mmvae_cpm_dense and of mmvae_gene_stats)


def cpm_dense(x: torch.Tensor, rows: Optional[torch.Tensor] = None, genes: Optional[torch.Tensor] = None, scaler: float = 1.0,
              log: bool = False, out_dtype: torch.dtype = torch.float64, path: str = "auto") -> Tuple[torch.Tensor, torch.Tensor]:
    """mmvae_cpm_dense: ``x`` [n_total, G] int32, float32 or float64 on the GPU (rows may be strided, columns not; read where
    it lies), optionally the int64 row map ``rows`` [n] and the int32 gene list ``genes`` [ng] -> (out [n, ng] of
    ``out_dtype`` float32 or float64, norms float64 [n]) on the device: out = x / norm * scaler, or log1p of that with
    ``log``, norm the row's sum |x| over all G genes (1 where that is 0), norms the sums themselves.  ``path``: "auto" (the
    launcher's rule), "narrow", "wide" -- the load forms, equal bits."""
    _need_cuda("cpm_dense", x, rows, genes)
    path = _path("cpm_dense", CPM_PATHS, path)
    if x.dtype not in CPM_VTYPES or x.dim() != 2 or out_dtype not in CPM_OTYPES:
        raise TypeError("cpm_dense: x must be int32, float32 or float64 [n_total, G] and out_dtype float32 or float64")
    n_total, G = (int(v) for v in x.shape)
    xm = _row_major(x)
    rows, n = _row_map("cpm_dense", rows, n_total)
    ng = G
    if genes is not None:
        if genes.dtype != torch.int32 or genes.dim() != 1:
            raise TypeError("cpm_dense: genes must be int32 [ng]")
        genes = genes.contiguous()
        ng = int(genes.numel())
    out = torch.empty(n, ng, dtype=out_dtype, device=xm.device)
    norms = torch.empty(n, dtype=torch.float64, device=xm.device)
    check(lib().mmvae_debug_cpm_dense(_ptr(xm), CPM_VTYPES[xm.dtype], int(xm.stride(0)), n_total, G, _ptr(rows), n, _ptr(genes), ng,
                                      float(scaler), int(bool(log)), _ptr(out), CPM_OTYPES[out_dtype], _ptr(norms), path,
                                      _stream(xm.device)), "mmvae_cpm_dense")
    return out, norms


def cpm_csr(indptr: torch.Tensor, indices: torch.Tensor, data: torch.Tensor, shape: Tuple[int, int], inv: torch.Tensor, ng: int,
            rows: Optional[torch.Tensor] = None, scaler: float = 1.0, log: bool = False,
            out_dtype: torch.dtype = torch.float64) -> Tuple[torch.Tensor, torch.Tensor]:
    """mmvae_cpm_csr: the canonical CSR matrix (``indptr`` int64 [n_total + 1], ``indices`` int32 [nnz], ``data`` int32,
    float32 or float64 [nnz]) of ``shape`` (n_total, G) on the GPU, the inverse gene map ``inv`` int32 [G] (the output column
    of a gene, -1: not selected) onto ``ng`` columns, optionally the int64 row map ``rows`` [n] -> (out [n, ng], norms
    float64 [n]) as ``cpm_dense`` on the dense matrix, bit for bit."""
    _need_cuda("cpm_csr", indptr, indices, data, inv, rows)
    n_total, G = int(shape[0]), int(shape[1])
    if indptr.dtype != torch.int64 or tuple(indptr.shape) != (n_total + 1,):
        raise TypeError(f"cpm_csr: indptr must be int64 [{n_total + 1}]")
    if indices.dtype != torch.int32 or indices.dim() != 1 or data.dim() != 1 or indices.numel() != data.numel():
        raise TypeError("cpm_csr: indices must be int32 [nnz] and data [nnz]")
    if data.dtype not in CPM_VTYPES or out_dtype not in CPM_OTYPES:
        raise TypeError("cpm_csr: data must be int32, float32 or float64 and out_dtype float32 or float64")
    if inv.dtype != torch.int32 or tuple(inv.shape) != (G,):
        raise TypeError(f"cpm_csr: inv must be int32 [{G}]")
    indptr, indices, data, inv = indptr.contiguous(), indices.contiguous(), data.contiguous(), inv.contiguous()
    rows, n = _row_map("cpm_csr", rows, n_total)
    out = torch.empty(n, int(ng), dtype=out_dtype, device=data.device)
    norms = torch.empty(n, dtype=torch.float64, device=data.device)
    nnz = int(data.numel())
    check(lib().mmvae_cpm_csr(_ptr(indptr), _ptr(indices) if nnz else None, _ptr(data) if nnz else None, CPM_VTYPES[data.dtype],
                              nnz, n_total, G, _ptr(rows), n, _ptr(inv), int(ng), float(scaler), int(bool(log)), _ptr(out),
                              CPM_OTYPES[out_dtype], _ptr(norms), _stream(data.device)), "mmvae_cpm_csr")
    return out, norms


def gene_stats(x: torch.Tensor, eps: float, rows: Optional[torch.Tensor] = None,
               path: str = "auto") -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """mmvae_gene_stats: ``x`` [n_total, D] float32 or float64 on the GPU (rows may be strided, columns not; read where it
    lies), optionally the int64 row map ``rows`` [n] -> (n_above int64 [D], mean float64 [D], std float64 [D]) on the
    device: per gene the number of selected rows with x > eps (eps rounded to x's dtype), the mean and the population
    standard deviation.  Inputs must be finite.  ``path``: "auto", "narrow", "wide" -- the load forms, equal bits."""
    _need_cuda("gene_stats", x, rows)
    path = _path("gene_stats", GENESTATS_PATHS, path)
    if x.dtype not in (torch.float32, torch.float64) or x.dim() != 2:
        raise TypeError("gene_stats: x must be float32 or float64 [n_total, D]")
    n_total, Dm = (int(v) for v in x.shape)
    xm = _row_major(x)
    rows, n = _row_map("gene_stats", rows, n_total)
    n_above = torch.empty(Dm, dtype=torch.int64, device=xm.device)
    mean = torch.empty(Dm, dtype=torch.float64, device=xm.device)
    sd = torch.empty(Dm, dtype=torch.float64, device=xm.device)
    ws_bytes = int(lib().mmvae_gene_stats_workspace_bytes(n, Dm))
    ws = _workspace(ws_bytes, xm.device)
    check(lib().mmvae_debug_gene_stats(_ptr(xm), CPM_VTYPES[xm.dtype], int(xm.stride(0)), n_total, Dm, _ptr(rows), n, float(eps),
                                       _ptr(ws), ws_bytes, _ptr(n_above), _ptr(mean), _ptr(sd), path,
                                       _stream(xm.device)), "mmvae_gene_stats")
    return n_above, mean, sd


def to_bf16(data: torch.Tensor) -> torch.Tensor:
    """The bf16 copy of a resident float32 matrix (round to nearest even; same shape and strides in elements) for the bf16
    engine's row-indexed step (mmvae_to_bf16; made once per data set)."""
    if data.device.type != "cuda":
        raise NativeError("to_bf16 needs a CUDA tensor (no CPU fallback)")
    assert data.dim() == 2 and data.dtype == torch.float32 and data.stride(1) == 1
    ld = int(data.stride(0))
    # (a column-offset view of a wider matrix spans (rows - 1) * ld + D elements, not rows * ld: the copy owns exactly that,
    # rounded up to whole 8-byte pieces; the kernel touches only the rows' own columns)
    span = (data.shape[0] - 1) * ld + ((data.shape[1] + 3) // 4) * 4
    out = torch.empty(span, dtype=torch.bfloat16, device=data.device).as_strided(data.shape, data.stride())
    check(lib().mmvae_to_bf16(_ptr(data), ld, data.shape[0], data.shape[1], _ptr(out), _stream(data.device)), "mmvae_to_bf16")
    return out


def tp_planes(data: torch.Tensor, n_planes: int) -> Optional[torch.Tensor]:
    """A resident float32 matrix as the planes x planes GEMM engine's tiled bf16 slice planes (mmvae_tp_planes; made once per
    data set: 3 planes = the exact slices of the fp32x3 engine, 1 = the matrix rounded to bf16) for the augmenter's row-indexed
    forward (mmvae_augment_rows).  Returns an opaque uint16 device tensor, or None where the library does not offer it."""
    if data.device.type != "cuda":
        raise NativeError("tp_planes needs a CUDA tensor (no CPU fallback)")
    assert data.dim() == 2 and data.dtype == torch.float32 and data.stride(1) == 1
    nbytes = int(lib().mmvae_tp_planes_bytes(data.shape[0], data.shape[1], n_planes))
    if nbytes == 0:
        return None
    out = torch.zeros(nbytes // 2, dtype=torch.int16, device=data.device)     # (padding rows of the planes are read, never used)
    check(lib().mmvae_tp_planes(_ptr(data), int(data.stride(0)), data.shape[0], data.shape[1], n_planes, _ptr(out),
                                _stream(data.device)), "mmvae_tp_planes")
    return out


def gather_rows(data: torch.Tensor, idx: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[i] = data[idx[i]] for a 2-D float32 CUDA matrix (rows may be strided) and int64 CUDA indices."""
    _need_cuda("gather_rows", data, idx)
    assert data.dim() == 2 and data.dtype == torch.float32 and data.stride(1) == 1
    idx = idx.to(torch.int64).contiguous()
    n, Dm = idx.numel(), data.shape[1]
    if out is None:
        out = torch.empty(n, Dm, dtype=torch.float32, device=data.device)
    if n:
        check(lib().mmvae_gather_rows(_ptr(data), data.stride(0), data.shape[0], _ptr(idx), n, Dm, _ptr(out),
                                      _stream(data.device)), "mmvae_gather_rows")
    return out


# ---------------------------------------------------------------------------------------------------------------
# operand type of the large GEMMs (mmvae_hyper.gemm_bf16 / mmvae_augment's gemm_bf16 argument)
#   "fp32"       fp32 results; the library's fastest fp32-grade engine ("fp32x3", see FP32_ENGINE below; shapes the split
#                engine does not take -- fc_dim > 111, D % 4 != 0 -- run the fp32 matrix instruction by themselves)
#   "fp32_mfma"  fp32 operands on the fp32 matrix instruction (v_mfma_f32_32x32x2_f32: an exact fmaf chain)
#   "fp32x3"     fp32 operands split exactly into three bf16 slices, six slice products per product on the bf16 matrix
#                pipe, fp32 accumulation: truncation <= 2^-26 per product, below the fp32 rounding of the accumulation
#   "bf16"       operands rounded to bf16 (BASELINE.json's bf16 configuration)
# MMVAE_FP32_ENGINE=fp32_mfma|fp32x3 picks what "fp32" means (A/B timing, and running the parity suite on either).
# ---------------------------------------------------------------------------------------------------------------
FP32_ENGINE = os.environ.get("MMVAE_FP32_ENGINE", "fp32x3")
_GEMM_MODES = {"fp32_mfma": 0, "bf16": 1, "fp32x3": 2}


def gemm_mode(dtype: str) -> int:
    if dtype == "fp32":
        dtype = FP32_ENGINE
    if dtype not in _GEMM_MODES:
        raise ValueError(f"gemm_dtype must be 'fp32', 'fp32_mfma', 'fp32x3' or 'bf16', got {dtype!r}")
    return _GEMM_MODES[dtype]

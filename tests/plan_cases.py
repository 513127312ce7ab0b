"""The switch points of make_plan (csrc/api.hip) as one table: shapes that sit on either side of every shape rule, and the
plan each of them must take on each GEMM engine.  Used by tests/test_plan_cpu.py (the plan read-back, host only),
tests/test_gpu_plan_matrix.py (the same rows on the GPU: plan first, then the numbers) and tests/test_gpu_noside.py (the rows
of NOSIDE_GPU on engines built without a side stream: `without_side()` of the same plans, then the numbers).

A new `Plan` field or shape rule comes with a row here.

The expectations are written by hand from the rules in csrc/common.hpp (fast_dims, bf16_tiles_fit: H <= 124, x3_fc11_fits:
H + 1 <= 112, chain_planes_fit: C + S <= 128, lat_half: C <= 96, L <= 32, 2 S <= 32) and from make_plan's text; nothing
here calls the library (the other call kinds' plans are derived from the step's by `expected()`, a restatement of
make_plan's per-kind differences that is maintained beside it).  Every row states the plan of the FUSED STEP (mmvae_train_step) with a side stream, in training
mode; `expected()` turns that into the other entry points' plans through the differences make_plan states per call kind
(no side-stream work outside the step, no head launch in a backward call, the output-only fc11 of decode, ...).

The two slab counts are split factors (mmvae_splits order: ks_fc1, ns_fc11, ks_dw, ks_small, ks_gd10, ks_dw11): the table says
WHICH factor the plan must carry -- ks_gd10 / ks_dw11 on the fast path, ns_fc11 / ks_dw off it -- and, where a clamp of
default_splits decides the value whatever the fill heuristic says, the value itself (SLABS).
"""
from collections import namedtuple

ENGINES = {"fp32_mfma": 0, "bf16": 1, "fp32x3": 2}
KINDS = ("STEP", "STEP_ROWS", "FORWARD", "FORWARD_XREC", "BACKWARD", "CLASSIFY", "DECODE", "TRAVERSE")

Row = namedtuple("Row", "name A B D H L C S hard s_drop x_drop misalign side")


def _r(name, A, B, D, H, L=10, C=92, S=2, hard=False, s_drop=0.0, x_drop=0.5, misalign=None, side=True):
    return Row(name, A, B, D, H, L, C, S, hard, s_drop, x_drop, misalign, side)


# misalign: "x_off1" / "p_off1": x / the flat parameters are a view one float into their storage (4-byte aligned);
#           "xs_odd": one x per arm with an arm stride of B * D + 1 floats
ROWS = [
    _r("h100", 2, 300, 520, 100),                       # the production width: k_fc11_zg on engine 0
    _r("h104", 2, 300, 520, 104), _r("h108", 2, 300, 520, 108),
    _r("h112", 2, 300, 520, 112), _r("h124", 2, 300, 520, 124),
    _r("h128", 2, 300, 520, 128),
    _r("h102", 2, 300, 520, 102), _r("d522", 2, 300, 522, 100),
    _r("x_off1", 2, 300, 520, 100, misalign="x_off1"), _r("p_off1", 2, 300, 520, 100, misalign="p_off1"),
    _r("xs_odd", 2, 300, 520, 100, misalign="xs_odd"),
    _r("a4", 4, 200, 256, 100), _r("a6", 6, 200, 256, 100), _r("a8", 8, 200, 256, 100),
    _r("lat_c97", 2, 200, 256, 100, C=97), _r("lat_l33", 2, 200, 256, 100, L=33), _r("lat_s17", 2, 200, 256, 100, S=17),
    _r("cs129", 2, 200, 256, 100, C=125, S=4),
    # the wave-form latent kernels on a ragged batch: 57 = 48 + 9 = 7 * 8 + 1 (LAT_ROWS / LAT_ROWS_BWD cells per workgroup)
    _r("lat_c97_b57", 2, 57, 256, 100, C=97),
    _r("d_min_h100", 2, 70, 4, 100), _r("d_min_h64", 2, 70, 4, 64),
    _r("d36_h100", 2, 70, 36, 100), _r("d36_h64", 2, 70, 36, 64),
    _r("d132_h100", 2, 300, 132, 100), _r("d132_h64", 2, 300, 132, 64),
    _r("d1004_h100", 2, 300, 1004, 100), _r("d1004_h64", 2, 300, 1004, 64),
    _r("b2", 2, 2, 256, 100), _r("b31", 2, 31, 256, 100), _r("b127", 2, 127, 256, 100), _r("b128", 2, 128, 256, 100),
    _r("b129", 2, 129, 256, 100), _r("b385", 2, 385, 256, 100),
    _r("xdrop0", 2, 300, 520, 100, x_drop=0.0),
    _r("sdrop_hard", 3, 130, 192, 100, hard=True, s_drop=0.2),
    # the step without a side stream, as a literal row (every other row's plan without one: without_side(); on the GPU:
    # NOSIDE_GPU, tests/test_gpu_noside.py)
    _r("noside", 2, 300, 520, 100, side=False),
]
BY_NAME = {r.name: r for r in ROWS}
GPU_ROWS = [r for r in ROWS if r.side]
# The rows the GPU runs on engines WITHOUT a side stream (tests/test_gpu_noside.py), the smallest shapes that reach each thing
# make_plan does differently then:
#   h100         FC11_ZG / FC11_BF16 / FC11_X3 without a riding fork; dW11 inline behind dW1
#   h104         engine 0: FC11_ZT, d(d10) as a launch of its own
#   h112         fp32x3: [d10 | 1] planes written, fc11 on the fp32 pair
#   a4           planes engines: COUPLE_IN_DEC with a side stream becomes the inline k_couple
#   lat_c97_b57  wave-form latent kernels, ragged batch
#   b129         ragged row tiles; dw11_slabs 5
#   xdrop0       ZERO_MEMSET, no head fill
#   sdrop_hard   A = 3, hard samples, state dropout
#   h102         general path: COUPLE_SIDE joined on the main stream becomes inline
NOSIDE_GPU = ("h100", "h104", "h112", "a4", "lat_c97_b57", "b129", "xdrop0", "sdrop_hard", "h102")

# ---- the fused step's plan, by hand -----------------------------------------------------------------------------------
# engine 0, fast path, fc_dim 100: d(d10) folded into the fc11 kernel, keep-mask bit image, everything fp32
_E0 = dict(fast=True, big="GEMM_FP32", small_x3=False, fc11="FC11_ZG", chain_planes=False, lat_half=True, narrow=False,
           presplit=False, bwd_small_planes=False, d10_planes=False, dz1_in_apply=False, dec_planes=False, zero="ZERO_XBITS",
           rowmap=False, dz11_bf16=False, dw11_side=True, loss_on_side=True, couple="COUPLE_SIDE", lat_fork_rides=True,
           fc11_fork_rides=False)
_E0_ZT = dict(_E0, fc11="FC11_ZT")                       # any other width: fc11 and d(d10) as two kernels
# engine 1, H <= 124: bf16 tiles, the chain kernels on slice planes (hence the head k_presplit launch), EV_FORK on the fc11 kernel
_E1 = dict(_E0, big="GEMM_BF16", small_x3=True, fc11="FC11_BF16", chain_planes=True, presplit=True, zero="ZERO_PRESPLIT",
           fc11_fork_rides=True)
# engine 2, H <= 108: the same tiles on three slices, [d10 | 1] planes from the decoder chain, dZ1 planes from k_bn_bwd_apply
_E2 = dict(_E1, big="GEMM_X3", fc11="FC11_X3", d10_planes=True, dz1_in_apply=True)
# engine 2, 112 <= H <= 124: x3 GEMMs, but [d10 | 1] does not fit k_x3_fc11g's 112 columns: the fp32 fc11 pair, d10 planes unread
_E2_ZT = dict(_E2, fc11="FC11_ZT", fc11_fork_rides=False)
# off the fast path: the general kernels, a fill for the zeroing, nothing but the coupling on the side stream
_GEN = dict(_E0, fast=False, big="GEMM_GENERAL", fc11="FC11_GENERAL", zero="ZERO_MEMSET", dw11_side=False, loss_on_side=False)
_GEN1 = dict(_GEN, small_x3=True)                        # (the small-layer products keep the engine's tiles on either path)
_GEN2 = dict(_GEN1, d10_planes=True, dz1_in_apply=True)  # (written, and read by no general kernel)
_STD = {"fp32_mfma": _E0, "bf16": _E1, "fp32x3": _E2}
_STD_OTHER_H = {"fp32_mfma": _E0_ZT, "bf16": _E1, "fp32x3": _E2}
_GENERAL = {"fp32_mfma": _GEN, "bf16": _GEN1, "fp32x3": _GEN2}
_IN_DEC = dict(couple="COUPLE_IN_DEC", lat_fork_rides=False)
_NO_HALF = dict(lat_half=False, lat_fork_rides=False)


def _each(base, **kw):
    return {e: dict(p, **kw) for e, p in base.items()}


STEP = {
    "h100": _STD,
    "h104": _STD_OTHER_H, "h108": _STD_OTHER_H,
    "h112": {"fp32_mfma": _E0_ZT, "bf16": _E1, "fp32x3": _E2_ZT},
    "h124": {"fp32_mfma": _E0_ZT, "bf16": _E1, "fp32x3": _E2_ZT},
    # past the bf16 tiles: engines 1 and 2 are engine 0 (fp32 matrix instruction, no planes, keep-mask bit image)
    "h128": {"fp32_mfma": _E0_ZT, "bf16": _E0_ZT, "fp32x3": _E0_ZT},
    "h102": _GENERAL, "d522": _GENERAL, "x_off1": _GENERAL, "p_off1": _GENERAL, "xs_odd": _GENERAL,
    # the coupling as a role of the decoder chain's launch from four arms (it needs the chain planes: not on engine 0), to five
    "a4": {"fp32_mfma": _E0, "bf16": dict(_E1, **_IN_DEC), "fp32x3": dict(_E2, **_IN_DEC)},
    "a6": _STD, "a8": _STD,
    "lat_c97": _each(_STD, **_NO_HALF),
    "lat_c97_b57": _each(_STD, **_NO_HALF),
    "lat_l33": _each(_STD, **_NO_HALF),
    "lat_s17": _each(_STD, **_NO_HALF),
    # C + S = 129: no chain planes (bf16: then no head launch either); C = 125 is also past the half-wave latent kernels
    "cs129": {"fp32_mfma": dict(_E0, **_NO_HALF),
              "bf16": dict(_E1, chain_planes=False, presplit=False, zero="ZERO_XBITS", **_NO_HALF),
              "fp32x3": dict(_E2, chain_planes=False, **_NO_HALF)},
    "d_min_h100": _STD, "d_min_h64": _STD_OTHER_H, "d36_h100": _STD, "d36_h64": _STD_OTHER_H,
    "d132_h100": _STD, "d132_h64": _STD_OTHER_H, "d1004_h100": _STD, "d1004_h64": _STD_OTHER_H,
    "b2": _STD, "b31": _STD, "b127": _STD, "b128": _STD, "b129": _STD, "b385": _STD,
    "xdrop0": _each(_STD, zero="ZERO_MEMSET"),           # no keep-mask: nothing for k_make_xbits / the head launch to fold the fill into
    "sdrop_hard": _STD,
    # no side stream: everything inline, no fork to ride
    "noside": _each(_STD, dw11_side=False, loss_on_side=False, couple="COUPLE_INLINE", lat_fork_rides=False,
                    fc11_fork_rides=False),
}

# Slab counts by hand, {row: {engine or "*": (gd10_slabs, dw11_slabs)}} (None: left to the fill heuristic), for the STEP plan.
# These shapes are far smaller than the chip (a few workgroups per split on 256 .. 768 slots), so default_splits' fill
# search never reaches 93 % and ends at its cap of 16 splits (the fp32x3 / bf16 dW11 targets, 140 / 160 workgroups, ask for
# even more); a clamp then decides wherever it is below 16:
#   gd10_slabs, fast path = ks_gd10 <= cdiv(D, 64) at fc_dim 100 (k_fc11_zg's gene split) and on the fp32x3 branch (taken
#               only while x3_fc11_fits), <= cdiv(D, 32) otherwise -- so h112 / h124 on fp32x3 carry 16 (the non-x3 branch;
#               the x3 branch would give cdiv(520, 64) = 9);
#   gd10_slabs, general path = ns_fc11 <= cdiv(D, 64);
#   dw11_slabs, fast path = ks_dw11 <= cdiv(B, 32);  general path = ks_dw <= cdiv(B, 32).
_G9 = {"*": (9, 10)}                                     # D = 520 or 522: cdiv(D, 64) = 9;  B = 300: cdiv(300, 32) = 10
_H_OTHER = {"fp32_mfma": (16, 10), "bf16": (16, 10), "fp32x3": (9, 10)}       # cdiv(520, 32) = 17: the cap; x3 branch: 9
SLABS = {
    "h100": _G9, "xdrop0": _G9, "h104": _H_OTHER, "h108": _H_OTHER,
    "h112": {"*": (16, 10)}, "h124": {"*": (16, 10)}, "h128": {"*": (16, 10)},
    "h102": _G9, "d522": _G9, "x_off1": _G9, "p_off1": _G9, "xs_odd": _G9,
    "d_min_h100": {"*": (1, 3)}, "d_min_h64": {"*": (1, 3)},                  # cdiv(4, 32 or 64) = 1;  cdiv(70, 32) = 3
    "d36_h100": {"*": (1, 3)},                                                 # cdiv(36, 64) = 1
    "d36_h64": {"fp32_mfma": (2, 3), "bf16": (2, 3), "fp32x3": (1, 3)},       # cdiv(36, 32) = 2;  x3 branch cdiv(36, 64) = 1
    "d132_h100": {"*": (3, 10)},                                               # cdiv(132, 64) = 3
    "d132_h64": {"fp32_mfma": (5, 10), "bf16": (5, 10), "fp32x3": (3, 10)},   # cdiv(132, 32) = 5;  x3 branch 3
    "d1004_h100": {"*": (16, 10)}, "d1004_h64": {"*": (16, 10)},              # cdiv(1004, 64) = 16 = the cap
    # D = 256, fc_dim 100: cdiv(256, 64) = 4;  cdiv(B, 32) = 1, 1, 4, 4, 5, 13
    "b2": {"*": (4, 1)}, "b31": {"*": (4, 1)}, "b127": {"*": (4, 4)}, "b128": {"*": (4, 4)}, "b129": {"*": (4, 5)},
    "b385": {"*": (4, 13)},
}


def slabs_of(row_name, engine):
    per = SLABS.get(row_name)
    return None if per is None else per.get(engine, per.get("*"))


# Eval-mode labels (eval forward and eval_classify) that may differ from the fp64 oracle's: the number the fp32 CPU oracle
# itself decides differently from fp64 on the row, plus 1.  Measured on the CPU when the rows were written: the fp32 oracle
# differs in no label on any of them (smallest relative gap between the fp64 oracle's top two probabilities: h112 7.9e-6,
# lat_l33 1.3e-5, h102 8.6e-5, h124 1.3e-4, h108 1.5e-4, lat_c97 1.6e-4, lat_s17 9.3e-4, the others above 1e-2).
EVAL_ROWS = ("h100", "h104", "h108", "h112", "h124", "h128", "h102", "lat_c97", "lat_l33", "lat_s17")
EVAL_LABEL_CAP = {name: 0 + 1 for name in EVAL_ROWS}

# Rows that cannot meet a gradient gate for a reason the fp32 CPU oracle shares: its own worst distance from the fp64 oracle
# on the row, measured on the CPU (tests allow 3 x that, the ratio assert_gradients_tight uses).
#   b2: two cells -- every BatchNorm output is +-1 and its backward cancels exactly, so the encoder gradients upstream of the
#       last BatchNorm are rounding noise amplified by 1 / sqrt(var + 1e-8): the fp32 oracle is up to 3.9e-2 of a tensor's
#       scale from fp64 there (fc5.0.weight; the device: 7.1e-2 on fp32_mfma, 2.6e-2 on fp32x3)
FP32_FLOOR = {"b2": 3.9e-2}


def slab_sources(plan):
    """(index into mmvae_splits of gd10_slabs, of dw11_slabs)."""
    return (4, 5) if plan["fast"] else (1, 2)


def expected(row, engine, kind, has_x16=False):
    """The plan of `kind` for a table row: the step's hand-written plan with the differences make_plan states per kind.

    Only the STEP table is literal.  This function is a second, independent statement of make_plan's per-kind logic
    (rowmap, narrow, dz1_in_apply, the decode fc11 families, what a call without a forward pass or without a step drops):
    it calls nothing of the library, but it has to be kept in step with make_plan by hand."""
    r = BY_NAME[row] if isinstance(row, str) else row
    p = dict(STEP[r.name][engine])
    step = kind in ("STEP", "STEP_ROWS")
    x3_fc11_fits = r.H + 1 <= 112
    if not step:                                         # side-stream placement and riding forks belong to the fused step
        p.update(loss_on_side=False, couple="COUPLE_INLINE", lat_fork_rides=False, fc11_fork_rides=False)
        if kind != "BACKWARD":
            p["dw11_side"] = False
    if kind == "STEP_ROWS":
        p["rowmap"] = p["zero"] == "ZERO_PRESPLIT" and p["fc11"] in ("FC11_X3", "FC11_BF16")
        if has_x16 and engine == "bf16" and r.H <= 124:
            p["narrow"] = r.D % 8 == 0
            p["dz1_in_apply"] = p["narrow"] and r.H % 2 == 0
            p["dz11_bf16"] = p["rowmap"] and p["fc11"] == "FC11_BF16"
    if kind == "FORWARD_XREC" and p["fc11"] in ("FC11_X3", "FC11_ZG"):
        p["fc11"] = "FC11_ZT"                             # x_rec is wanted: the fused gradient forms do not write it
    if kind == "BACKWARD":                               # no forward pass in this call: no head launch, nothing to zero
        p.update(presplit=False, zero="ZERO_NONE", bwd_small_planes=p["chain_planes"])
    if kind in ("CLASSIFY", "TRAVERSE", "DECODE"):       # eval mode
        p["zero"] = "ZERO_NONE"
    if kind == "DECODE":
        p["presplit"] = False
        if p["fast"]:
            p["fc11"] = ("FC11_OUT_X3" if p["big"] == "GEMM_X3" and x3_fc11_fits else
                         "FC11_OUT_BF16" if p["big"] == "GEMM_BF16" else "FC11_ZT")
        p["d10_planes"] = p["fc11"] in ("FC11_OUT_X3", "FC11_OUT_BF16")
        p["dec_planes"] = p["d10_planes"] or p["chain_planes"]
    p["kind"] = {"FORWARD_XREC": "FORWARD"}.get(kind, kind)
    return p


def without_side(plan):
    """`plan` (of any kind) as make_plan builds it for an mmvae_exec without a side stream: nothing runs beside the main
    stream and no fork event has a kernel to ride on; every other field is unchanged.  By hand from make_plan's text (`side`
    enters dw11_side, loss_on_side and couple; the two riding forks follow from those)."""
    return dict(plan, dw11_side=False, loss_on_side=False, couple="COUPLE_INLINE", lat_fork_rides=False, fc11_fork_rides=False)


def plan_args(row, kind):
    """Keyword arguments of _native.debug_plan for a row and a kind of KINDS."""
    r = BY_NAME[row] if isinstance(row, str) else row
    return dict(kind={"FORWARD_XREC": "FORWARD"}.get(kind, kind),
                params_align=4 if r.misalign == "p_off1" else 16, x_align=4 if r.misalign == "x_off1" else 16,
                x_arm_stride=r.B * r.D + 1 if r.misalign == "xs_odd" else 0, fc11_grad=kind != "FORWARD_XREC")

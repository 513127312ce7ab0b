"""The plan of mmvae_zinb_train_step (call kind MMVAE_CALL_ZINB_STEP = 11), by hand, for tests/test_zinb_step_cpu.py.

The ZINB step is the fused step run on one stream: its plan is the fused step's (tests/plan_cases.py, STEP) as make_plan
builds it WITHOUT a side stream -- whatever the mmvae_exec states -- with `kind` ZINB_STEP and `gd10_slabs` 1 (the one array
mmvae_zinb_d10_grad writes, as slab 0); `dw11_slabs` keeps the step's value and is not read (there is no dW11 GEMM).  The bf16
engine is refused by the entry point and has no rows.

Two tables:
  * LITERAL: the rows of tests/zinb_step_cases.py (the shapes the GPU runs) with the step's hand-written plan each takes, named
    by the building blocks of tests/plan_cases.py -- between them the general kernels, FC11_ZT, FC11_ZG and FC11_X3, both latent
    kernel forms;
  * every row of plan_cases.ROWS through `expected`: plan_cases.expected(row, engine, "STEP"), without_side, kind, gd10_slabs.
"""
from tests import plan_cases as P
from tests import zinb_step_cases as Z

ENGINES = {e: v for e, v in P.ENGINES.items() if e != "bf16"}
KIND = "ZINB_STEP"
GD10_SLABS = 1

_WAVE = dict(lat_half=False)
LITERAL = {
    # row of zinb_step_cases: {engine: the fused step's plan with a side stream (without_side is applied by `zinb_plan`)}
    "a2_d70_h20": {"fp32_mfma": P._GEN, "fp32x3": P._GEN2},                     # D % 4 != 0: the general kernels
    "a3_d130_h100_hard_sdrop": {"fp32_mfma": P._GEN, "fp32x3": P._GEN2},
    # H = 128 is past the bf16 tiles: fp32x3 is engine 0 there (no planes); L = 33, C = 97: the one-wave-per-cell latent kernels
    "a2_d130_h128_wave_hard": {"fp32_mfma": dict(P._GEN, **_WAVE), "fp32x3": dict(P._GEN, **_WAVE)},
    "a2_d72_h20_fast_sdrop": {"fp32_mfma": P._E0_ZT, "fp32x3": P._E2},          # the fast path: FC11_ZT / FC11_X3
    "a3_d132_h100_fast": {"fp32_mfma": P._E0, "fp32x3": P._E2},                 # fc_dim 100 on engine 0: FC11_ZG
}
assert set(LITERAL) == set(Z.ROW_IDS)


def zinb_plan(step_plan):
    """The ZINB step's plan from the fused step's: one stream, kind 11, one d(d10) slab."""
    return dict(P.without_side(step_plan), kind=KIND, gd10_slabs=GD10_SLABS)


def expected(row, engine):
    """For a row of plan_cases.ROWS."""
    return zinb_plan(P.expected(row, engine, "STEP"))


def plan_args(row):
    return dict(P.plan_args(row, "STEP"), kind=KIND)

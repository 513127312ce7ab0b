"""Operating points at which the ZINB term reaches the gradient of EVERY encoder and latent tensor, as one table.

At the default point (tau = 0.005, temp = beta = lam = 1) the coupling term is the encoder's whole gradient (README,
"Gradients by loss term"; tests/term_cases.py), and the ZINB term -- a mean over B D elements -- has a smaller share still:
split by term in fp64 (zinb_step_restatement.term_grads) it is 4e-3 of fc_sigma's bias gradient and below that in the encoder.
A step whose gd10 were wired to the slab wrongly would pass every gradient gate there.  The rows here move the step to points
where the ZINB term is at least MIN_SHARE of max |g_total| in every tensor of fc1 .. fc5, fcc, fc_mu and fc_sigma (weight and
bias, every arm): `assert_exposes`, held on the CPU by tests/test_zinb_step_cpu.py and again by the GPU test before it
compares.

How the points were found (CPU, fp64): lam = 1e-13 takes the distance term's coefficient out, as the "rec" rows of
tests/term_cases.py do; beta = 1e-3 takes KL out of the state head; the entropy term then carries the encoder (ZINB 0.01) until
tau = 10 flattens c towards the uniform point, where the entropy's gradient vanishes (ZINB 0.24; the inverse standard deviations
of the distance term grow there and bring it back to a share of 1 even at lam = 1e-13); counts up to 1e5 in place of 1e3 raise
the ZINB term's gradients by two orders: ZINB 0.98 .. 1 on every row.

fc11's bias is raised by FC11_BIAS_SHIFT = 1 on every row.  The term reads r = relu(a_rec) + 1e-6 and its derivatives grow as
1 / r, so where a pre-activation of fc11 lies near zero the rounding of ANY float32 evaluation of a_rec (1e-7 at these widths)
moves g by 1e-7 / r of itself: at nn.Linear's default initialisation the rows hold pre-activations down to 3e-7, and the
float32 restatement's own worst entry of fc11's gradient (section 9m's statistic) is then 5.8e-3 beside a 90th percentile of
2.6e-7 -- a maximum that records where one evaluation's rounding fell, on either side of the comparison.  With the shift every
a_rec is at least 0.6 (measured in fp64 per row and arm: 0.63 .. 0.89) and the maximum measures arithmetic again.  The dead
branch of fc11's ReLU is then not taken in these rows; it is covered where its kernels are tested for their bits
(tests/test_gpu_zinb_step.py::test_single_pass_equals_the_two_entries_bit_for_bit, tests/test_gpu_zinb_fit.py).

The combinations the rows cover: A = 2 and 3; hard on and off; s_drop 0 and 0.2; x_drop 0.5; B = 70 (one full and one partial
cell tile of 64) and 129 (two full, one of a single cell); D = 70 and 130 (a partial last gene tile; two and three tiles), off
the fast path (D % 4 != 0: the general kernels), and D = 72 and 132 on it (the fp32x3 / fp32 matrix-instruction engines, the
fused fc11 kernels); H = 20 and 100, and H = 128 (the ZINB kernels' tile passes 80 KB of LDS: one workgroup per CU); both
latent kernel forms ("wave": L = 33, C = 97)."""
import functools
import os
import sys
from collections import namedtuple

import torch

from oracle import restatement as R
from tests import term_cases as T

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import zinb_restatement as ZR  # noqa: E402
import zinb_step_restatement as S  # noqa: E402

MIN_SHARE = T.MIN_SHARE
PINNED = T.ENCODER + ("fc_mu", "fc_sigma")               # the tensors behind the decoder's input [c | s]
SEEDS = dict(weights=21, heads=22, batch=8, noise=13)
MAX_COUNT = 100000
FC11_BIAS_SHIFT = 1.0

Row = namedtuple("Row", "name A B D H L C S hard s_drop x_drop tau temp beta lam")


def _r(name, A, B, D, H, L=8, C=12, S_=3, hard=False, s_drop=0.0, x_drop=0.5, tau=10.0, temp=1.0, beta=1e-3, lam=1e-13):
    return Row(name, A, B, D, H, L, C, S_, hard, s_drop, x_drop, tau, temp, beta, lam)


ROWS = [
    # ZINB share over the pinned tensors (min), measured in fp64
    _r("a2_d70_h20", 2, 70, 70, 20),                                            # 0.996
    _r("a3_d130_h100_hard_sdrop", 3, 129, 130, 100, hard=True, s_drop=0.2),     # 0.984
    _r("a2_d130_h128_wave_hard", 2, 70, 130, 128, L=33, C=97, S_=2, hard=True),  # 0.989
    _r("a2_d72_h20_fast_sdrop", 2, 129, 72, 20, s_drop=0.2),                    # 0.983
    _r("a3_d132_h100_fast", 3, 70, 132, 100),                                   # 0.995
]
BY_NAME = {r.name: r for r in ROWS}
ROW_IDS = [r.name for r in ROWS]


def hyper(row) -> R.Hyper:
    return R.Hyper(input_dim=row.D, fc_dim=row.H, n_categories=row.C, state_dim=row.S, lowD_dim=row.L, x_drop=row.x_drop,
                   s_drop=row.s_drop, n_arm=row.A, lam=row.lam, tau=row.tau, beta=row.beta, hard=row.hard, temp=row.temp)


def inputs(row):
    """(hyper, fp32 state dict with the p and r heads, fp32 batch X = log1p(counts), noise) of a row."""
    h = hyper(row)
    sd = R.init_state_dict(h, SEEDS["weights"])
    sd.update(S.init_heads(h, SEEDS["heads"]))
    for a in range(h.n_arm):
        sd[f"fc11.{a}.bias"] = sd[f"fc11.{a}.bias"] + FC11_BIAS_SHIFT
    x = ZR.counts_matrix(row.B, row.D, torch.Generator().manual_seed(SEEDS["batch"]), max_count=MAX_COUNT)
    return h, sd, x, R.draw_noise(h, row.B, seed=SEEDS["noise"])


def is_pinned(key: str) -> bool:
    return key.split(".")[0] in PINNED


@functools.lru_cache(maxsize=None)
def oracle(name):
    """Everything the tests compare against, computed once per row and left unchanged: the fp64 restatement's forward outputs,
    loss tuple, gradients and running statistics after the step, the ZINB term's share of every gradient tensor, and the fp32
    restatement's own error against fp64 per gradient tensor (relative to the tensor's fp64 maximum)."""
    row = BY_NAME[name]
    h, sd, x, noise = inputs(row)
    A = h.n_arm
    sd64, x64, n64 = T.to64(sd, x, noise)
    tg = S.term_grads(sd64, [x64] * A, h, n64)
    after = {k: v.clone() for k, v in sd64.items()}
    out64, saved64, lt64, g64 = S.grads_autograd(after, [x64] * A, h, n64)
    _, _, _, g32 = S.grads_autograd({k: v.clone() for k, v in sd.items()}, [x] * A, h, noise)
    share, e32 = {}, {}
    for k, g in g64.items():
        sc = float(g.abs().max()) + 1e-300
        e32[k] = float((g32[k].double() - g).abs().max()) / sc
        share[k] = float(tg["zinb"][k].abs().max()) / sc
    out64 = tuple([t.detach() for t in o] for o in out64)
    lt64 = [[t.detach() for t in v] if isinstance(v, list) else v.detach() for v in lt64]
    a_rec_min = min(float((s["d10"].detach() @ sd64[f"fc11.{a}.weight"].T + sd64[f"fc11.{a}.bias"]).min()) for a, s in enumerate(saved64))
    return dict(row=row, h=h, sd=sd, x=x, noise=noise, out64=out64, lt64=lt64, g64=g64, share=share, e32=e32,
                d10=[s["d10"].detach() for s in saved64], a_rec_min=a_rec_min,
                bn64={k: v for k, v in after.items() if "running" in k or "num_batches" in k})


def assert_exposes(name):
    """The row's precondition: the ZINB term is at least MIN_SHARE of every pinned tensor's gradient maximum."""
    o = oracle(name)
    low = {k: s for k, s in o["share"].items() if is_pinned(k) and not s >= MIN_SHARE}
    assert not low, (name, low)
    assert o["a_rec_min"] >= 0.5, (name, o["a_rec_min"])                  # every pre-activation of fc11 far from its kink


def grad_tolerance(name, key) -> float:
    """max(GRAD_TOL, 3 x the fp32 restatement's own error in that tensor): the rule of tests/term_cases.grad_tolerance."""
    return max(T.GRAD_TOL, 3.0 * oracle(name)["e32"][key])

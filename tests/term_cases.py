"""Operating points at which each term of the loss reaches the ENCODER's gradients, as one table.

Every other parity test runs the step at tau = 0.005, temp = beta = lam = 1, eps = 1e-8 on `init_state_dict` weights and
`synthetic_batch` inputs.  There the cross-arm distance term (lam * c_dist, inverse standard deviations ~1e4) carries the
encoder's whole gradient: split by term in fp64 (restatement.term_grads), reconstruction, KL and entropy are each below
1e-11 of every encoder tensor's gradient, far under any gate, so the latent backward's state-head, Gumbel-softmax,
straight-through, decoder-input and entropy pieces could be absent from the encoder's gradient unnoticed.  The rows here
move the step to points where each term T of (rec, kl, ent, dist) is at least MIN_SHARE of max |g_total| in EVERY encoder
tensor (fc1..fc5, fcc; weight and bias; every arm), for every kernel-form group:

  half   A = 2, L = 8, C = 12, S = 3    the half-wave latent kernels
  wave   A = 2, L = 33, C = 97, S = 2   one past their limits: the one-wave-per-cell kernels
  a3     A = 3                          couple_body RB = 2, am1 = 2
  a4     A = 4                          the fused step runs the coupling as a role of the decoder chain (engines with planes)
  a8     A = 8                          RB = 1, 28 pairs

all at B = 70 (three 32-row blocks, the last ragged), D = 64, H = 32.  A row names the terms it `exposes`; `assert_exposes`
holds the share condition for exactly those, per tensor (tests/test_terms_cpu.py on the CPU, tests/test_gpu_loss_terms.py
again before it compares), and `test_terms_cpu` holds that every group's rows expose all four terms between them, so the
table cannot drift back into a dominated point.

How the points were found (CPU, fp64): lam = 1e-13 takes the distance term out (ent 0.7 .. 1); beta = 1e3 then brings KL
to ~1; the reconstruction term's share grows with the input scale (BatchNorm makes the encoder's activations independent
of it, the reconstruction error is not): x50 reaches 0.2 .. 1 on the small latent shapes, the 97-category shape needs
more.  The secondary settings (hard, s_drop, temp, tau, eps, x_drop, momentum) are spread over the rows so that each value
the default point never takes appears at least once (`test_terms_cpu` lists them).

`floor`: the fp32 CPU oracle's own worst distance from fp64 over the row's gradient tensors, relative to each tensor's
maximum, written here where it exceeds GRAD_TOL / 3 (the row then needs the 3 x floor of the tolerance rule); the CPU test
holds the recorded figure to the measured one within a factor of two.
"""
import functools
from collections import namedtuple

from oracle import restatement as R

MIN_SHARE = 0.1
GRAD_TOL = 1e-3                                          # tests/test_gpu_parity.py
ENCODER = ("fc1", "fc2", "fc3", "fc4", "fc5", "fcc")
SHAPES = {
    # group: A, B, D, H, L, C, S
    "half": (2, 70, 64, 32, 8, 12, 3),
    "wave": (2, 70, 64, 32, 33, 97, 2),
    "a3": (3, 70, 64, 32, 8, 12, 3),
    "a4": (4, 70, 64, 32, 8, 12, 3),
    "a8": (8, 70, 64, 32, 8, 12, 3),
}
SEEDS = dict(weights=21, batch=8, noise=13)              # those of tests/test_gpu_parity.py::test_vs_oracle_edge_shapes

Row = namedtuple("Row", "name group exposes xscale tau temp beta lam eps momentum hard s_drop x_drop floor")


def _r(name, group, exposes, xscale=1.0, tau=0.005, temp=1.0, beta=1.0, lam=1.0, eps=1e-8, momentum=0.01, hard=False,
       s_drop=0.0, x_drop=0.5, floor=None):
    return Row(name, group, tuple(exposes.split()), xscale, tau, temp, beta, lam, eps, momentum, hard, s_drop, x_drop, floor)


ROWS = [
    # shares measured in fp64 over the encoder tensors (min .. max), for the terms the row exposes
    _r("half_rec_ent", "half", "rec ent", xscale=50.0, lam=1e-13, temp=0.3, s_drop=0.2),     # rec 0.39 .. 1.3, ent 0.19 .. 0.95
    _r("half_kl", "half", "kl", lam=1e-13, beta=1e3, temp=2.0, momentum=0.1),                # kl 0.99 .. 1
    _r("half_dist", "half", "dist", tau=0.05, lam=1e-4, beta=30.0, eps=1e-4),                # dist 0.41 .. 1.2 (kl 0.04 .. 0.92)
    _r("wave_rec_ent", "wave", "rec ent", xscale=400.0, lam=1e-13, hard=True),               # rec 0.36 .. 0.83, ent 0.47 .. 1.1
    _r("wave_kl", "wave", "kl", lam=1e-13, beta=1e3, temp=0.3, s_drop=0.2, momentum=1.0),    # kl 0.97 .. 1
    _r("wave_dist", "wave", "dist", tau=0.05, temp=2.0),                                     # dist 1
    _r("a3_rec_ent", "a3", "rec ent", xscale=50.0, lam=1e-13, hard=True, s_drop=0.2),        # rec 0.16 .. 1.3, ent 0.36 .. 1.5
    _r("a3_kl", "a3", "kl", lam=1e-13, beta=1e3, tau=1.0, x_drop=0.0),                       # kl 1
    _r("a3_dist", "a3", "dist", tau=0.05, lam=1e-4, beta=30.0),                              # dist 0.39 .. 1.1 (kl 0.02 .. 0.61)
    _r("a4_rec_ent", "a4", "rec ent", xscale=50.0, lam=1e-13, temp=0.3),                     # rec 0.30 .. 2.2, ent 0.30 .. 2.3
    _r("a4_kl", "a4", "kl", lam=1e-13, beta=1e3, s_drop=0.2, hard=True),                     # kl 0.99 .. 1
    _r("a4_dist", "a4", "dist", eps=1e-4, momentum=0.1),                                     # dist 1
    _r("a8_rec_ent", "a8", "rec ent", xscale=50.0, lam=1e-13, temp=2.0),                     # rec 0.19 .. 1.7, ent 0.43 .. 2.7
    _r("a8_kl", "a8", "kl", lam=1e-13, beta=1e3, momentum=1.0),                              # kl 0.98 .. 1
    _r("a8_dist", "a8", "dist", tau=0.05, temp=0.3),                                         # dist 1
]
# the default operating point on the "half" shape: what every other parity test runs (test_terms_cpu measures its shares)
DEFAULT_POINT = _r("default_point", "half", "dist")
BY_NAME = {r.name: r for r in ROWS + [DEFAULT_POINT]}
ROW_IDS = [r.name for r in ROWS]


def hyper(row) -> R.Hyper:
    A, B, D, H, L, C, S = SHAPES[row.group]
    return R.Hyper(input_dim=D, fc_dim=H, n_categories=C, state_dim=S, lowD_dim=L, x_drop=row.x_drop, s_drop=row.s_drop,
                   n_arm=A, lam=row.lam, tau=row.tau, beta=row.beta, hard=row.hard, eps=row.eps, momentum=row.momentum,
                   temp=row.temp)


def inputs(row):
    """(hyper, fp32 state dict, fp32 batch, noise) of a row."""
    h = hyper(row)
    B = SHAPES[row.group][1]
    sd = R.init_state_dict(h, SEEDS["weights"])
    x = R.synthetic_batch(B, h.input_dim, seed=SEEDS["batch"]) * row.xscale
    return h, sd, x, R.draw_noise(h, B, seed=SEEDS["noise"])


def to64(sd, x, noise):
    sd64 = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    n64 = {k: [t.double() if t.is_floating_point() else t for t in v] for k, v in noise.items()}
    return sd64, x.double(), n64


def is_encoder(key: str) -> bool:
    return key.split(".")[0] in ENCODER


@functools.lru_cache(maxsize=None)
def oracle(name):
    """Everything the tests compare against, computed once per row and left unchanged: the fp64 oracle's forward outputs,
    loss tuple, gradients and running statistics after the step, its gradients by term and their shares, and the fp32 CPU
    oracle's own error against fp64 per gradient tensor (relative to the tensor's fp64 maximum)."""
    row = BY_NAME[name]
    h, sd, x, noise = inputs(row)
    A = h.n_arm
    sd64, x64, n64 = to64(sd, x, noise)
    tg = R.term_grads(sd64, [x64] * A, h, n64)
    sd64_after = {k: v.clone() for k, v in sd64.items()}
    out64, lt64, g64 = R.grads_autograd(sd64_after, [x64] * A, h, n64)
    _, _, g32 = R.grads_autograd({k: v.clone() for k, v in sd.items()}, [x] * A, h, noise)
    share = {t: {} for t in R.TERMS}
    e32 = {}
    for k, g in g64.items():
        sc = float(g.abs().max()) + 1e-300
        e32[k] = float((g32[k].double() - g).abs().max()) / sc
        for t in R.TERMS:
            share[t][k] = float(tg[t][k].abs().max()) / sc
    out64 = tuple([t.detach() for t in o] for o in out64)
    lt64 = [[t.detach() for t in v] if isinstance(v, list) else v.detach() for v in lt64]
    return dict(row=row, h=h, sd=sd, x=x, noise=noise, out64=out64, lt64=lt64, g64=g64, tg=tg, share=share, e32=e32,
                bn64={k: v for k, v in sd64_after.items() if "running" in k or "num_batches" in k})


def assert_exposes(name):
    """The row's precondition: every term it names is at least MIN_SHARE of every encoder tensor's gradient maximum."""
    o = oracle(name)
    for t in o["row"].exposes:
        low = {k: s for k, s in o["share"][t].items() if is_encoder(k) and not s >= MIN_SHARE}
        assert not low, (name, t, low)


def grad_tolerance(name, key) -> float:
    """max(GRAD_TOL, 3 x the fp32 CPU oracle's own error in that tensor): the rule of gpu_util.assert_gradients_tight."""
    return max(GRAD_TOL, 3.0 * oracle(name)["e32"][key])

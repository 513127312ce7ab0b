"""Inputs of the count-distribution tests (tests/test_countdist_cpu.py, tests/test_gpu_countdist.py) and numpy callers of the
library's host-only debug entries.

The regimes every matrix covers, element by element in a fixed pattern (with a float32 jitter so that no two elements repeat):
theta in {1e-6 (what a ReLU-zero x_rec gives), 0.3, 1, 1e4}; mu in {0, 2, 8, 12, 1e3} (Poisson means on both sides of 10);
mu = theta = 1e9 (the 1e8 clamp) at a few fixed places; logits in {-30, 0, 30}; x in {0, eps, 1, 7, 1e3}.  theta is given as a
matrix or, for the [D] form, as its first row's pattern."""
import ctypes as C

import numpy as np

from distributed_vae_amd import _native as N

THETAS = np.array([1e-6, 0.3, 1.0, 1e4])
MUS = np.array([0.0, 2.0, 8.0, 12.0, 1e3])
LOGITS = np.array([-30.0, 0.0, 30.0])
XS = np.array([0.0, 1e-8, 1.0, 7.0, 1e3])
EPS = 1e-8
SHAPES = [(65, 130), (257, 130), (1, 1)]


def regimes(n, D, seed, theta_vector=False, big=True):
    """{"x", "mu", "theta", "pi", "mu2", "theta2"}: float32 arrays [n, D] (theta [D] with ``theta_vector``)."""
    rng = np.random.default_rng(seed)
    i, j = np.meshgrid(np.arange(n), np.arange(D), indexing="ij")
    jit = lambda: 1.0 + 0.25 * rng.random((n, D))           # noqa: E731
    kth = (j if theta_vector else i + 2 * j) % 4
    th = THETAS[kth] * (jit()[0][None, :] if theta_vector else jit())
    th = np.where((kth == 2) & (j % 3 == 0), 1.0, th)                     # theta = 1 itself, too
    mu = MUS[(3 * i + j + 1) % 5] * jit()
    out = {"mu": mu, "theta": th, "pi": LOGITS[(i + j) % 3] + np.where((i + j) % 3 == 1, rng.standard_normal((n, D)), 0.0),
           "x": XS[(i + 3 * j) % 5], "mu2": MUS[(i + 2 * j + 1) % 5] * jit(), "theta2": THETAS[(2 * i + j) % 4] * jit()}
    if big and not theta_vector and n * D >= 16:
        for r, c in ((0, 0), (n // 2, D // 3), (n - 1, D - 1), (n // 3, D - 2)):
            out["mu"][r, c] = out["theta"][r, c] = 1e9
    out = {k: v.astype(np.float32) for k, v in out.items()}
    if theta_vector:
        out["theta"] = out["theta"][0].copy()
        out["theta2"] = out["theta2"][0].copy()
    return out


def _p(a):
    return None if a is None else a.ctypes.data


def _ld(a):
    return 0 if a.ndim == 1 else a.strides[0] // a.itemsize


def host_logp(kind, x, mu, theta, pi=None, mu2=None, theta2=None, eps=EPS):
    """mmvae_debug_count_logp_host on float32 numpy arrays -> terms float32 [n, D]."""
    arrs = {k: (None if v is None else np.ascontiguousarray(v, dtype=np.float32)) for k, v in
            dict(x=x, mu=mu, theta=theta, pi=pi, mu2=mu2, theta2=theta2).items()}
    n, D = arrs["x"].shape
    terms = np.empty((n, D), dtype=np.float32)
    a = N.CountLogp(kind=N.COUNT_KINDS[kind], N=n, D=D, eps=eps, x=_p(arrs["x"]), ldx=D, terms=_p(terms), ld_t=D)
    for k in ("mu", "theta", "pi", "mu2", "theta2"):
        if arrs[k] is not None:
            setattr(a, k, _p(arrs[k]))
            setattr(a, "ld_" + k, _ld(arrs[k]))
    N.check(N.lib().mmvae_debug_count_logp_host(C.byref(a)), "mmvae_debug_count_logp_host")
    return terms


def host_sample(a, b, zi=None, zi_kind=None, seed=0, offset=0, cell0=0, out_int32=False, log1p=False, heads_eps=None):
    """mmvae_debug_count_sample_host on float32 numpy arrays -> (draws float32 or int32 [n, D], the exhaustion counter)."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    zi = None if zi is None else np.ascontiguousarray(zi, dtype=np.float32)
    n, D = a.shape
    out = np.empty((n, D), dtype=np.int32 if out_int32 else np.float32)
    counter = np.full(1, -1, dtype=np.int32)
    s = N.CountSample(param=int(heads_eps is not None), zi_kind=0 if heads_eps is not None else N.COUNT_ZI[zi_kind], N=n, D=D,
                      cell0=cell0, eps=heads_eps or 0.0, seed=seed, offset=offset, a=_p(a), ld_a=D, b=_p(b), ld_b=_ld(b),
                      zi=_p(zi), ld_zi=D, out_int32=int(out_int32), log1p=int(log1p), out=_p(out), ld_out=D, exhausted=_p(counter))
    N.check(N.lib().mmvae_debug_count_sample_host(C.byref(s)), "mmvae_debug_count_sample_host")
    return out, int(counter[0])


# the parameter settings of the distribution tests: (name, mu, theta, zero-inflation probability or None)
SETTINGS = [("theta0.3_mu5", 5.0, 0.3, None), ("theta1_mu3", 3.0, 1.0, None), ("theta1e4_mu8", 8.0, 1e4, None),
            ("theta1e4_mu1e3", 1e3, 1e4, None), ("theta0.3_mu1e3", 1e3, 0.3, None), ("theta2_mu20_z0.5", 20.0, 2.0, 0.5),
            ("theta0.3_mu5_z0.2", 5.0, 0.3, 0.2)]
N_DRAWS = 1 << 16
DRAW_SHAPE = (256, 256)


# ---- the sampler's element-by-element cases: name -> (n, D, theta as a vector, mode, cell0, offset, seed) ----------------------
# mode: "nb", "logits", "probs" (zi = sigmoid(pi) as float32) or "heads" (x_rec, x_p, x_r under zinb_loss's eps = 1e-6).
# cell0 = 2^40 puts every logical element index past 2^32 (about 1.4e14) without allocating anything.  The seeds are chosen so
# that the restatement reports no element with a decision margin below 1e-9 (tests/test_countdist_cpu.py verifies and prints
# the count): the elements at risk are the few with mu = theta = 1e9, whose PTRS candidate near 1e8 lies within 0.1 of an
# integer one time in five.
SAMPLE_CASES = {
    "nb_65x130": (65, 130, False, "nb", 0, 0, 2),
    "zinb_logits_257x130": (257, 130, False, "logits", 5, 3, 0),
    "zinb_probs_vector_65x130": (65, 130, True, "probs", 7, 1 << 40, 1),
    "heads_65x130": (65, 130, False, "heads", 0, 2, 2),
    "one": (1, 1, False, "logits", 0, 0, 3),
    "past_2^32": (65, 130, False, "logits", 1 << 40, 0, 1),
}
HEADS_EPS = 1e-6


def sample_case(name):
    """The arguments of host_sample / count_sample for one case, as float32 numpy arrays."""
    n, D, vec, mode, cell0, offset, seed = SAMPLE_CASES[name]
    r = regimes(n, D, 1000 + n + D + len(name), theta_vector=vec)
    sig = lambda v: (1.0 / (1.0 + np.exp(-v.astype(np.float64)))).astype(np.float32)     # noqa: E731
    kw = dict(seed=seed, offset=offset, cell0=cell0)
    if mode == "heads":
        x_rec = np.where(r["theta"] < 1e-3, 0.0, np.minimum(r["mu"], 50.0)).astype(np.float32)   # ReLU zeros: theta = eps
        return dict(a=x_rec, b=sig(r["pi"] / 6.0), zi=sig(r["pi"]), zi_kind=None, heads_eps=HEADS_EPS, **kw)
    zi = None if mode == "nb" else (r["pi"] if mode == "logits" else sig(r["pi"]))
    return dict(a=r["mu"], b=r["theta"], zi=zi, zi_kind=None if mode == "nb" else mode, heads_eps=None, **kw)


def restate_sample(case):
    """tests/countdist_restatement.sample on a case of ``sample_case``."""
    import countdist_restatement as CR
    if case["heads_eps"] is not None:
        mu, th, z = CR.heads_to_params(case["a"], case["b"], case["zi"], case["heads_eps"])
        return CR.sample(mu, th, z, "probs", seed=case["seed"], offset=case["offset"], cell0=case["cell0"])
    zi = None if case["zi"] is None else case["zi"].astype(np.float64)
    return CR.sample(case["a"].astype(np.float64), case["b"].astype(np.float64), zi, case["zi_kind"], seed=case["seed"],
                     offset=case["offset"], cell0=case["cell0"])


def as_float32_draws(draw):
    """The restatement's fp64 draws as the float32 output holds them (NaN stays NaN)."""
    return draw.astype(np.float32)


LOGP_FUNCS = ("nb", "zinb", "mix", "mix1")


def logp_args(fn, r):
    """The keyword arguments of host_logp / count_logp for function ``fn`` on the arrays of ``regimes``."""
    kind = {"nb": "nb", "zinb": "zinb", "mix": "mixture", "mix1": "mixture"}[fn]
    kw = dict(x=r["x"], mu=r["mu"], theta=r["theta"])
    if fn != "nb":
        kw["pi"] = r["pi"]
    if kind == "mixture":
        kw["mu2"] = r["mu2"]
        if fn == "mix":
            kw["theta2"] = r["theta2"]
    return kind, kw


def logp_truth(fn, r):
    """(truth, M_e) in fp64 of function ``fn`` on the float32 arrays of ``regimes``."""
    import countdist_restatement as CR
    a = {k: np.asarray(v).astype(np.float64) for k, v in r.items()}
    if fn == "nb":
        args = (a["x"], a["mu"], a["theta"])
        return CR.log_nb(*args), CR.magnitudes_nb(*args)
    if fn == "zinb":
        args = (a["x"], a["mu"], a["theta"], a["pi"])
        return CR.log_zinb(*args), CR.magnitudes_zinb(*args)
    args = (a["x"], a["mu"], a["mu2"], a["theta"], a["theta2"] if fn == "mix" else None, a["pi"])
    return CR.log_mixture(*args), CR.magnitudes_mixture(*args)


# The per-element gate of a device (or host-entry) term: |got - truth| <= 2^-23 |truth| + c 2^-53 M_e.  c, the operation count
# of the evaluation order of csrc/countdist_core.hpp: truth and library run the same IEEE additions, products and quotients
# on the same inputs in the same order (the library is built without fma contraction), so they differ only in the libm calls.
# Per libm result 5 ulp = 10 units of 2^-53 of its own magnitude (4 ulp the device library's documented bound for lgamma, 1
# for numpy's), and every libm result enters M_e through the addends it is part of -- log(theta + mu + eps) through two of
# them -- once per use:
#   nb      3 logarithms in 4 addends + 3 lgammas: 7 addends each off by at most 10 units -> c = 10; the 6 additions that
#           join them are the same on both sides but are granted one unit each -> c = 16
#   zinb    the nb terms + two softplus (exp, log1p and one addition each: 21 units of a magnitude that M_e holds) -> c = 40
#   mixture two nb values (16 each, of the M_e of each), the logsumexp's exp and log1p (20) and the softplus (21) -> c = 80
C_OPS = {"nb": 16.0, "zinb": 40.0, "mix": 80.0, "mix1": 80.0}


def logp_gate(fn, truth, M):
    return 2.0 ** -23 * np.abs(truth) + C_OPS[fn] * 2.0 ** -53 * M

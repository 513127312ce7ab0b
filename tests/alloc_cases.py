"""One case per device entry point for tests/test_gpu_alloc_contract.py: `run()` builds its model or inputs, calls the Python
API and returns {name: CPU tensor} with every result and every piece of state the call updates in place.  Models and
engines are built inside `run()`, so their cached workspaces are allocated under the guard of tests/alloc_guard.py when one
is installed.  Shapes are the smallest at which a size formula can go wrong: two tiles or segments with the last one ragged,
a group smaller than a segment, the segment count forced where an argument allows it.

Conventions of the returned dict:
  * a key that starts with "pad:" holds the padding bytes of a pitched output (uint8); under a guard they must still hold
    the fill, and they take no part in the comparison between runs;
  * everything else is compared bit for bit between the unguarded run and the two guarded ones.

Buffers a case hands to an entry point itself (an `out=`, Adam moments, a pitched destination) are allocated through
`N.torch.empty`, i.e. through whatever stands for torch in `_native` at that moment: the guard's proxy when one is installed.

`EXCLUDED` lists the bound entry points that have no case, with the reason; tests/test_alloc_guard_cpu.py requires every
other one to appear in some case's `covers`.
"""
import contextlib
import functools
import os
import sys
from collections import namedtuple

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

Case = namedtuple("Case", "name covers run")
CASES = []
DEV = "cuda:0"


def zb_tile():
    """ZB_T of csrc/zb_tile.hpp (the ZINB kernels' cell and gene tile)."""
    import re
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "distributed-vae_amd", "csrc", "zb_tile.hpp")
    with open(path) as f:
        return int(re.search(r"constexpr\s+int\s+ZB_T\s*=\s*(\d+)\s*;", f.read()).group(1))


def case(name, covers):
    def deco(fn):
        CASES.append(Case(name, tuple(covers), fn))
        return fn
    return deco


def _N():
    import distributed_vae_amd  # noqa: F401
    from distributed_vae_amd import _native as N
    return N


# ---- turning results into {name: CPU tensor} ------------------------------------------------------------------------------
def flat(prefix, obj, out=None):
    out = {} if out is None else out
    if obj is None:
        return out
    if torch.is_tensor(obj):
        t = obj.detach()
        out[prefix] = (t.clone() if t.is_contiguous() else t.contiguous()).cpu()
    elif isinstance(obj, dict):
        for k, v in obj.items():
            flat(f"{prefix}.{k}", v, out)
    elif isinstance(obj, (list, tuple)):
        for i, v in enumerate(obj):
            flat(f"{prefix}.{i}", v, out)
    elif isinstance(obj, (bool, int, float)):
        out[prefix] = torch.tensor(float(obj), dtype=torch.float64)
    else:
        raise TypeError((prefix, type(obj)))
    return out


def padding(t, alloc_elems):
    """The bytes of the allocation behind the 2-D pitched tensor `t` (its storage: `alloc_elems` elements from t's first)
    that belong to no element of `t`."""
    n, w = t.shape
    ld = t.stride(0)
    whole = t.as_strided((alloc_elems,), (1,))
    i = torch.arange(alloc_elems, device=t.device)
    inside = ((i % ld) < w) & ((i // ld) < n)
    return whole[~inside].contiguous().view(torch.uint8).cpu()


def pitched(N, src, pitch, col0=0):
    """`src` [n, w] on the device as a window (columns col0 .. col0 + w) of a [n, pitch] matrix whose other columns are 7."""
    n, w = src.shape
    big = torch.full((n, pitch), 7.0, dtype=src.dtype, device=DEV)
    big[:, col0: col0 + w] = src.to(DEV)
    return big[:, col0: col0 + w]


# =====================================================================================================================
# the VAE: step, forward + loss + backward, classify, encode, intermed, decode, state_changes
# =====================================================================================================================
STEP_ROWS = ("b129", "d36_h64", "lat_c97_b57", "a4", "h112", "xdrop0")
CALL_ROWS = ("b129", "d36_h64")
ENGINES = ("fp32_mfma", "bf16", "fp32x3")


@functools.lru_cache(maxsize=None)
def _vae_inputs(row_name):
    from oracle import restatement as R
    from tests import plan_cases as P
    row = P.BY_NAME[row_name]
    h = R.Hyper(input_dim=row.D, fc_dim=row.H, n_categories=row.C, state_dim=row.S, lowD_dim=row.L, x_drop=row.x_drop,
                s_drop=row.s_drop, n_arm=row.A, hard=row.hard)
    sd = R.init_state_dict(h, 546)
    g = torch.Generator().manual_seed(77)
    for k in sd:                                          # running statistics off their initial (0, 1)
        if k.endswith("running_mean"):
            sd[k] = 0.3 * torch.randn(sd[k].shape, generator=g)
        elif k.endswith("running_var"):
            sd[k] = 0.5 + torch.rand(sd[k].shape, generator=g)
    n_rows = 2 * row.B + 5
    data = R.synthetic_batch(n_rows, row.D, seed=32)
    rows = torch.randint(0, n_rows, (row.B,), generator=torch.Generator().manual_seed(33))
    rows[:2] = torch.tensor([n_rows - 1, 0])
    noises = [R.draw_noise(h, row.B, seed=40 + s) for s in range(3)]
    eval_noise = R.draw_noise(h, row.B, seed=5, training=False, eval_flag=True)
    return row, h, sd, data, rows, noises, eval_noise


def _vae(row_name, engine, train):
    from tests import gpu_util as U
    row, h, sd, data, rows, noises, eval_noise = _vae_inputs(row_name)
    m = U.build_model(h, sd)
    m.train(train)
    m.gemm_dtype = engine
    return U, row, h, m, data, rows, noises, eval_noise


def _vae_state(m, opt=None):
    d = {"params": m.flat_parameters(), "grads": m.flat_grad(), "bn": m._bn_flat, "nbt": m._nbt}
    if opt is not None:
        d["exp_avg"], d["exp_avg_sq"] = opt.exp_avg, opt.exp_avg_sq
    return d


def _step_case(row_name, engine):
    def run():
        from distributed_vae_amd.cpl_mixvae import FusedAdam
        from tests import plan_cases as P
        U, row, h, m, data, rows, noises, _ = _vae(row_name, engine, True)
        opt = FusedAdam(m, lr=1e-3)
        m.set_explicit_noise([U.noise_to_device(n) for n in noises])
        x = data[rows].contiguous().to(DEV).expand(row.A, -1, -1)
        out = {}
        for s in range(2):
            flat(f"loss{s}", m.fused_train_step(x, 1.0, opt, do_adam=True), out)
        flat("after_two", _vae_state(m, opt), out)
        if P.expected(row, engine, "STEP_ROWS")["rowmap"]:
            flat("loss_rows", m.fused_train_step_rows(data.to(DEV), rows.to(DEV), 1.0, opt, do_adam=True), out)
            flat("after_rows", _vae_state(m, opt), out)
        torch.cuda.synchronize()
        return out
    covers = ["mmvae_train_step"]
    from tests import plan_cases as P
    if P.expected(P.BY_NAME[row_name], engine, "STEP_ROWS")["rowmap"]:
        covers.append("mmvae_train_step_rows")
    CASES.append(Case(f"step[{row_name}-{engine}]", tuple(covers), run))


def _calls_case(row_name, engine):
    def run():
        N = _N()
        U, row, h, m, data, rows, noises, eval_noise = _vae(row_name, engine, True)
        A = row.A
        x = data[: row.B].contiguous().to(DEV)
        xs = x.expand(A, -1, -1)
        out = {}
        # forward + loss + backward through the reference-shaped API (training mode)
        m.set_explicit_noise(U.noise_to_device(noises[0]))
        fw = m(xs, 1.0, 0.0)
        lt = m.loss(fw[0], [], [], xs, fw[7], fw[8], fw[4], fw[6], 0.0)
        m.zero_grad()
        lt[0].backward()
        flat("forward", [fw[i] for i in (0, 3, 4, 5, 6, 7, 8, 9)], out)
        flat("loss", [lt[0].detach(), lt[1], lt[2], lt[3], lt[4], lt[5], lt[6], lt[8]], out)
        flat("train", _vae_state(m), out)
        flat("dump_noise", m._engine.dump_noise(m._hyper(1.0, False), N.make_noise(None, 7, 3)), out)
        # the encoder alone in training mode (explicit mask), then everything in eval mode
        flat("encoder_train", m.encoder(x, 1), out)
        m.eval()
        m.set_explicit_noise(U.noise_to_device(eval_noise))
        with torch.no_grad():
            ev = m(xs, 1.0, eval=True)
        flat("eval_forward", [ev[i] for i in (0, 3, 4, 5, 6, 7, 8, 9)], out)
        counts = torch.zeros(max(A * (A - 1) // 2, 1), row.C, row.C, dtype=torch.int64, device=DEV)
        flat("eval_labels", m.eval_labels(xs, 1.0, counts=counts), out)
        flat("eval_counts", counts, out)
        flat("encode", m.encode(xs, 1.0), out)
        flat("encoder_eval", m.encoder(x, 0), out)
        y = torch.cat((ev[3][1], ev[4][1]), dim=1)
        flat("intermed", m.intermed(y, 1), out)
        flat("decoder", m.decoder(ev[6][1], ev[5][1], 1), out)
        g = torch.Generator().manual_seed(6)
        n_samp = 37
        m.set_explicit_state_noise(torch.rand(A, n_samp, 3, generator=g).to(DEV))
        flat("state_changes", m.state_changes(x[:3], 1, 1.0, n_samp=n_samp)[0], out)
        flat("state_after", _vae_state(m), out)
        torch.cuda.synchronize()
        return out
    CASES.append(Case(f"calls[{row_name}-{engine}]",
                      ("mmvae_forward", "mmvae_loss", "mmvae_backward", "mmvae_eval_classify", "mmvae_encode", "mmvae_intermed",
                       "mmvae_decode", "mmvae_state_changes", "mmvae_dump_noise"), run))


for _row in STEP_ROWS:
    for _e in ENGINES:
        _step_case(_row, _e)
for _row in CALL_ROWS:
    for _e in ENGINES:
        _calls_case(_row, _e)


# =====================================================================================================================
# the ZINB step and objective: the two smallest rows (by A B D H) of tests/zinb_plan_cases.py's literal table
# =====================================================================================================================
ZINB_STEP_ROWS = ("a2_d70_h20", "a2_d72_h20_fast_sdrop")            # the general kernels; the fast path with state dropout


def _zinb_step_case(row_name, engine):
    def run():
        from tests import gpu_util as U
        from tests import zinb_step_cases as Z
        from tests.test_gpu_zinb_step import build
        row = Z.BY_NAME[row_name]
        h, sd, x, noise = Z.inputs(row)
        m = build(h, sd, engine=engine)
        nd = U.noise_to_device(noise)
        m.set_explicit_noise([nd, nd])
        xs = x.to(DEV).expand(h.n_arm, -1, -1)
        out = {}
        state = m.zinb_step_state()
        for s in range(2):
            flat(f"loss{s}", m.zinb_train_step(xs, row.temp, state=state), out)
        hp, hg = m.zinb_heads_flat()
        flat("state", dict(_vae_state(m), heads=hp, head_grads=hg, **{k: v for k, v in state.items() if torch.is_tensor(v)}), out)
        m.eval()
        m.set_explicit_noise(U.noise_to_device(Z.R.draw_noise(h, row.B, seed=5, training=False, eval_flag=True)))
        obj = m.zinb_objective(xs, row.temp)
        flat("objective", [obj[0], obj[1], obj[2], obj[3], obj[4], obj[5], obj[6], obj[8]], out)
        flat("nll", m.zinb_nll(xs, row.temp), out)
        flat("decoder_grads", m.zinb_decoder_grads(xs, row.temp), out)
        torch.cuda.synchronize()
        return out
    CASES.append(Case(f"zinb_step[{row_name}-{engine}]", ("mmvae_zinb_train_step", "mmvae_zinb_objective"), run))


for _row in ZINB_STEP_ROWS:
    for _e in ("fp32_mfma", "fp32x3"):
        _zinb_step_case(_row, _e)


# =====================================================================================================================
# the ZINB and count-distribution entries on raw matrices: N = D = 2 ZB_T + 1, H odd, pitched X and d10, segments 1 and 3
# =====================================================================================================================
@functools.lru_cache(maxsize=None)
def _zinb_raw():
    import zinb_grad_restatement as RG
    n = D = 2 * zb_tile() + 1
    H = 33                                                # odd, and one past a 32-wide K chunk
    return (n, D, H) + tuple(RG.inputs(n, D, H))


def _zinb_dev(N):
    n, D, H, d10, L, X = _zinb_raw()
    return n, D, H, pitched(N, d10, H + 3), [t.to(DEV) for t in L], pitched(N, X, D + 3)


@case("zinb_heads_nll_terms", ("mmvae_zinb_heads", "mmvae_zinb_nll", "mmvae_zinb_terms", "mmvae_zinb_terms_grad"))
def _():
    N = _N()
    import zinb_restatement as ZR
    n, D, H, d10, L, X = _zinb_dev(N)
    out = {}
    x_p, x_r = N.zinb_heads(d10, *L[2:])
    flat("heads", (x_p, x_r), out)
    flat("nll", N.zinb_nll(d10, *L, X), out)
    x_rec = pitched(N, ZR.heads(*(t.cpu() for t in (d10, *L)))[0], D + 3)
    flat("terms", N.zinb_terms(x_rec, x_p, x_r, X, return_terms=True), out)
    flat("terms_sums_only", N.zinb_terms(x_rec, x_p, x_r, X), out)
    flat("terms_grad", N.zinb_terms_grad(x_rec, x_p, x_r, X, scale=0.5), out)
    return out


def _zinb_grads_case(segments):
    def run():
        N = _N()
        n, D, H, d10, L, X = _zinb_dev(N)
        out = {}
        for heads in (("rec", "p", "r"), ("p",)):
            tag = "".join(h[0] for h in heads)
            flat(f"head_grads.{tag}", N.zinb_head_grads(d10, *L, X, heads=heads, segments=segments), out)
            flat(f"step_grads.{tag}", N.zinb_step_grads(d10, *L, X, heads=heads, segments=segments), out)
            flat(f"d10_grad.{tag}", N.zinb_d10_grad(d10, *L, X, heads=heads, segments=segments), out)
        # ldg: gd10 into a pitched destination
        pitch = H + 5
        dst = N.torch.empty(n, pitch, dtype=torch.float32, device=DEV)
        view = dst[:, :H]
        N.zinb_d10_grad(d10, *L, X, segments=segments, out=view)
        flat("d10_grad.pitched", view, out)
        out["pad:d10_grad.pitched"] = padding(view, n * pitch)
        return out
    CASES.append(Case(f"zinb_grads[segments={segments}]",
                      ("mmvae_zinb_head_grads", "mmvae_zinb_d10_grad", "mmvae_zinb_step_grads"), run))


for _s in (1, 3):
    _zinb_grads_case(_s)


def _trunk_case(segments):
    def run():
        N = _N()
        import zinb_decoder_restatement as DR
        n = 2 * zb_tile() + 1
        acts, params, gd10 = DR.trunk_inputs(n, 9, 5, 33)
        acts = [pitched(N, a, a.shape[1] + 3) for a in acts]
        out = {}
        ref = N.decoder_trunk_grads(acts, [p.to(DEV) for p in params], pitched(N, gd10, 40), segments=segments)
        flat("grads", ref, out)
        flat("no_gzin", N.decoder_trunk_grads(acts, [p.to(DEV) for p in params], gd10.to(DEV), segments=segments, want_gzin=False),
             out)
        # ldgz: the gradient with respect to zin into a pitched destination (the wrapper always passes ldgz = Z, so this is the
        # wrapper's own call with another pitch)
        import ctypes as C
        Z, Lw, H = (int(a.shape[1]) for a in acts[:3])
        ps = [p.to(DEV).contiguous() for p in params]
        gs = [N.torch.empty(p.shape, dtype=torch.float32, device=DEV) for p in ps]
        gd = gd10.to(DEV)
        pitch = Z + 3
        dst = N.torch.empty(n, pitch, dtype=torch.float32, device=DEV)
        nbytes = int(N.lib().mmvae_decoder_trunk_grads_workspace_bytes(n, Z, Lw, H, segments))
        ws = N._workspace(nbytes, DEV)
        vp6, vp10 = C.c_void_p * 6, C.c_void_p * 10
        N.check(N.lib().mmvae_decoder_trunk_grads(n, Z, Lw, H, vp6(*(N._ptr(a) for a in acts)),
                                                  (C.c_int64 * 6)(*(N._zinb_pitch(a) for a in acts)), vp10(*(N._ptr(p) for p in ps)),
                                                  N._ptr(gd), H, segments, N._ptr(ws), nbytes, vp10(*(N._ptr(g) for g in gs)),
                                                  N._ptr(dst), pitch, N._stream(torch.device(DEV))), "mmvae_decoder_trunk_grads")
        assert torch.equal(dst[:, :Z], ref[1]) and all(torch.equal(a, b) for a, b in zip(gs, ref[0]))
        flat("pitched_gzin", [gs, dst[:, :Z]], out)
        out["pad:gzin.pitched"] = padding(dst[:, :Z], n * pitch)
        return out
    CASES.append(Case(f"decoder_trunk_grads[segments={segments}]", ("mmvae_decoder_trunk_grads",), run))


for _s in (1, 3):
    _trunk_case(_s)


@case("count_logp_sample", ("mmvae_count_logp", "mmvae_count_sample", "mmvae_zinb_sample"))
def _():
    N = _N()
    from tests import countdist_inputs as CI
    n, D, H, d10, L, X = _zinb_dev(N)
    r = {k: torch.from_numpy(v) for k, v in CI.regimes(n, D, 3, big=False).items()}
    p = {k: pitched(N, v, D + 3) for k, v in r.items()}
    rv = {k: torch.from_numpy(v).to(DEV) for k, v in CI.regimes(n, D, 4, theta_vector=True).items()}
    out = {}
    flat("logp.nb", N.count_logp("nb", p["x"], p["mu"], p["theta"], return_sums=True), out)
    flat("logp.nb_vec", N.count_logp("nb", rv["x"], rv["mu"], rv["theta"], return_terms=False, return_sums=True), out)
    flat("logp.zinb", N.count_logp("zinb", p["x"], p["mu"], p["theta"], pi=p["pi"], return_sums=True), out)
    flat("logp.mixture", N.count_logp("mixture", p["x"], p["mu"], p["theta"], pi=p["pi"], mu2=p["mu2"], theta2=p["theta2"],
                                      return_sums=True), out)
    flat("sample.nb", N.count_sample(p["mu"], p["theta"], seed=5, offset=2, cell0=7), out)
    flat("sample.zinb_int", N.count_sample(p["mu"], rv["theta"], zi=p["pi"], zi_kind="logits", seed=5, out_int32=True), out)
    flat("sample.log1p", N.count_sample(p["mu"], p["theta"], zi=torch.sigmoid(p["pi"]).contiguous(), zi_kind="probs", seed=6,
                                        log1p=True), out)
    flat("zinb_sample", N.zinb_sample(d10, *L, seed=11, offset=1, cell0=3), out)
    flat("zinb_sample.int", N.zinb_sample(d10, *L, seed=11, out_int32=True), out)
    return out


# =====================================================================================================================
# evaluation and analysis entries: the smallest ragged shapes of their own GPU tests; at least two segments, one group
# smaller than a segment; n <= 2000
# =====================================================================================================================
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _offsets(sizes):
    return torch.tensor([0] + list(np.cumsum(sizes)), dtype=torch.int64, device=DEV)


@contextlib.contextmanager
def production_twin(N, name):
    """Inside: the wrapper that calls mmvae_debug_<name>(..., path = auto, stream) reaches mmvae_<name>(..., stream), the
    production entry (the same arguments without the path)."""
    L = N.lib()
    dbg, prod = getattr(L, "mmvae_debug_" + name), getattr(L, "mmvae_" + name)

    def call(*a):
        assert a[-2] == -1, "the production entry has no path argument"
        return prod(*a[:-2], a[-1])
    setattr(L, "mmvae_debug_" + name, call)
    try:
        yield
    finally:
        setattr(L, "mmvae_debug_" + name, dbg)


def both_twins(N, name, fn, out):
    """`fn()` through the debug twin the wrapper calls and through the production entry."""
    flat(f"{name}.debug_twin", fn(), out)
    with production_twin(N, name):
        flat(f"{name}.production", fn(), out)


@case("silhouette", ("mmvae_silhouette",))
def _():
    N = _N()
    sizes = [700, 3, 130]                                 # SILHOUETTE_SEG_COLS = 512: two segments, a cluster of three
    assert sizes[0] > N.SILHOUETTE_SEG_COLS > sizes[2]
    n, d = sum(sizes), 5
    x = pitched(N, torch.randn(n, d, generator=_gen(1)), 8, 1)
    perm = torch.randperm(n, generator=_gen(2)).to(DEV)
    return flat("s", [N.silhouette(x, _offsets(sizes), perm), N.silhouette(x, _offsets(sizes))])


@case("state_corr", ("mmvae_state_corr", "mmvae_debug_state_corr"))
def _():
    N = _N()
    sizes = [300, 7, 130]                                 # STATECORR_SEG_ROWS = 256
    assert sizes[0] > N.STATECORR_SEG_ROWS > sizes[2]
    n, D, S, n_total = sum(sizes), N.STATECORR_TILE + 5, 3, 500
    data = pitched(N, torch.relu(torch.randn(n_total, D, generator=_gen(3))), D + 3)
    state = torch.randn(n, S, generator=_gen(4)).to(DEV)
    rows = torch.randint(0, n_total, (n,), generator=_gen(5)).to(DEV)
    out = {}
    both_twins(N, "state_corr", lambda: N.state_corr(data, state, rows, _offsets(sizes)), out)
    flat("one_group", N.state_corr(data[:n], state), out)
    return out


@case("group_moments_gauss_scores", ("mmvae_group_moments", "mmvae_debug_group_moments", "mmvae_gauss_scores"))
def _():
    N = _N()
    sizes = [300, 5, 100]                                 # GAUSSCLF_SEG_ROWS = 256
    assert sizes[0] > N.GAUSSCLF_SEG_ROWS > sizes[2]
    n, d = sum(sizes), 19
    x = pitched(N, torch.randn(n, d, generator=_gen(6)), d + 2)
    out = {}
    both_twins(N, "group_moments", lambda: N.group_moments(x, _offsets(sizes), torch.randn(d, generator=_gen(7)).to(DEV)), out)
    n, d, F, K = 2 * N.GAUSSCLF_ROW_TILE + 22, 11, 2, 5   # three 64-cell tiles, the last ragged; d % 8 != 0
    g = _gen(8)
    xs = pitched(N, torch.randn(n, d, generator=g), d + 1)
    model = torch.sort(torch.randint(0, F, (n,), generator=g))[0].to(torch.int32).to(DEV)
    mu = torch.randn(F, K, d, generator=g, dtype=torch.float64).to(DEV)
    W = torch.randn(F, K, d, d, generator=g, dtype=torch.float64).to(DEV)
    c0 = torch.randn(F, K, generator=g, dtype=torch.float64).to(DEV)
    perm = torch.randperm(n, generator=g).to(DEV)
    flat("gauss_scores", N.gauss_scores(xs, model, mu, W, c0, perm, return_scores=True), out)
    flat("gauss_scores.plain", N.gauss_scores(xs, model, mu, W, c0), out)
    return out


@case("leaf_merge", ("mmvae_leaf_merge",))
def _():
    N = _N()
    n, L = 2 * N.LEAFMERGE_WAVES + 1, 6                   # one cell a wave, four waves a workgroup: three workgroups, ragged
    levels = [[[0, 1], [2], [3, 4, 5]], [[0, 1, 2], [3, 4, 5]]]
    out = {}
    for tag, kw in (("all", dict(return_second=True, return_merged=True)), ("labels", dict(return_second=False))):
        p = pitched(N, torch.randn(n, L, generator=_gen(9), dtype=torch.float64), L + 2)
        flat(tag, N.leaf_merge(p, *N.merge_tables(levels), **kw), out)
        flat(tag + ".posterior", p, out)
    return out


@case("forest_cv", ("mmvae_forest_cv",))
def _():
    N = _N()
    n, d, K, F, T = 300, 7, 3, 2, 3
    g = _gen(10)
    bins = torch.randint(0, 256, (n, d + 1), generator=g, dtype=torch.uint8).to(DEV)[:, :d]
    codes = (torch.arange(n) % K).to(torch.int32)[torch.randperm(n, generator=g)].to(DEV)
    fold = (torch.arange(n) % F).to(torch.int32)[torch.randperm(n, generator=g)].to(DEV)
    out = {}
    res = N.forest_cv(bins, codes, fold, K, F, T, 3, 17, return_votes=True, return_trees=True)
    count, nodes = res[4]["count"].cpu(), res[4]["nodes"].cpu()
    for t in range(F * T):                                # rows past the count are zero (forest_cv's contract)
        assert 1 <= int(count[t]) < 2 * n and not bool(nodes[t, int(count[t]):].any()), (t, int(count[t]))
    flat("trees", res, out)
    flat("labels", N.forest_cv(bins, codes, fold, K, F, T, 3, 17), out)
    return out


@case("gram_symm_mul_pca_project", ("mmvae_gram", "mmvae_debug_gram", "mmvae_symm_mul", "mmvae_pca_project"))
def _():
    N = _N()
    n_total, n, D, k = 700, 2 * N.GRAM_SEG_ROWS + 88, N.GRAM_TILE + 6, 5
    assert N.gram_segments(n, D)[0] >= 2
    g = _gen(11)
    data = pitched(N, torch.randn(n_total, D, generator=g), D + 2)
    rows = torch.randint(0, n_total, (n,), generator=g).to(DEV)
    pivot = torch.randn(D, generator=g).to(DEV)
    out = {}
    both_twins(N, "gram", lambda: N.gram(data, pivot, rows), out)
    flat("gram.cov", N.gram(data, pivot, cov=True), out)
    Cm = N.gram(data, pivot, rows, cov=True)[1]
    Q = torch.randn(D, k, generator=g, dtype=torch.float64).to(DEV)
    flat("symm_mul", N.symm_mul(Cm, Q), out)
    mean = torch.randn(D, generator=g, dtype=torch.float64).to(DEV)
    flat("pca_project", [N.pca_project(data, mean, Q, rows), N.pca_project(data, mean, Q)], out)
    return out


@case("dataprep", ("mmvae_gene_stats", "mmvae_debug_gene_stats", "mmvae_cpm_dense", "mmvae_debug_cpm_dense", "mmvae_cpm_csr"))
def _():
    N = _N()
    n_total, n, D = 700, 2 * N.GENESTATS_SEG_ROWS + 88, N.GENESTATS_TILE + 5
    g = _gen(12)
    x = pitched(N, torch.relu(torch.randn(n_total, D, generator=g)), D + 3)
    rows = torch.randint(0, n_total, (n,), generator=g).to(DEV)
    out = {}
    both_twins(N, "gene_stats", lambda: N.gene_stats(x, 0.1, rows), out)
    flat("gene_stats.f64", N.gene_stats(x.double(), 0.1), out)
    n_total, G, n = 40, 300, 13
    counts = (torch.rand(n_total, G, generator=g) < 0.2).to(torch.int32) * torch.randint(1, 90, (n_total, G), generator=g, dtype=torch.int32)
    counts[5] = 0                                         # an empty row: norm 1
    rows = torch.randint(0, n_total, (n,), generator=g).to(DEV)
    genes = torch.randperm(G, generator=g)[:71].to(torch.int32)
    xc = counts.to(DEV)
    both_twins(N, "cpm_dense", lambda: N.cpm_dense(xc, rows, genes.to(DEV), scaler=1e6, log=True, out_dtype=torch.float32), out)
    flat("cpm_dense.all", N.cpm_dense(xc.float(), scaler=1e4), out)
    nz = counts != 0                                      # the canonical CSR form of `counts`, row by row
    indptr = torch.cat([torch.zeros(1, dtype=torch.int64), nz.sum(1).cumsum(0)])
    indices = nz.nonzero()[:, 1].to(torch.int32)
    inv = torch.full((G,), -1, dtype=torch.int32)
    inv[genes.long()] = torch.arange(genes.numel(), dtype=torch.int32)
    flat("cpm_csr", N.cpm_csr(indptr.to(DEV), indices.to(DEV), counts[nz].to(DEV), (n_total, G), inv.to(DEV), genes.numel(), rows,
                              scaler=1e6, log=True), out)
    return out


@case("mutinfo_ami", ("mmvae_mutinfo_counts", "mmvae_debug_mutinfo_counts", "mmvae_ami_binary"))
def _():
    N = _N()
    A, n, Cc, F = 2, 601, 7, 5
    g = _gen(13)
    labels = torch.randint(0, Cc, (A, n), generator=g, dtype=torch.int32).to(DEV)
    targets = (torch.rand(n, F + 2, generator=g) < 0.3).to(torch.uint8).to(DEV)
    out = {}
    acc = N.mutinfo_counts(labels, targets, Cc, F)
    flat("counts", acc, out)
    for path in ("lds", "global"):
        flat(f"counts.{path}", N.mutinfo_counts(labels, targets, Cc, F, path=path), out)
    flat("ami.table", N.ami_binary(*acc, n_cells=n), out)
    flat("ami.direct", N.ami_binary(*acc, n_cells=n, table=False), out)
    return out


@case("pair_stats_consensus", ("mmvae_pair_stats", "mmvae_debug_pair_stats", "mmvae_pair_stats_finish",
                               "mmvae_confmat_accumulate", "mmvae_consensus", "mmvae_classify"))
def _():
    N = _N()
    T, n, Cc = 3, 601, 7
    g = _gen(14)
    probs = torch.softmax(2 * torch.randn(T, n, Cc, generator=g), -1).to(DEV)
    out = {}
    labels = N.classify(probs)
    flat("classify", labels, out)
    pairs = [[0, 0, 1, 1], [0, 0, 2, 2], [1, 1, 2, 2]]
    acc = N.pair_stats(labels, probs, pairs, Cc)
    flat("pair_stats", acc, out)
    for path in ("lds", "wave"):
        flat(f"pair_stats.{path}", N.pair_stats(labels, probs, pairs, Cc, path=path), out)
    fin = N.pair_stats_finish(*acc)
    flat("finish", fin["packed"], out)
    counts = N.confmat_accumulate(labels, Cc)
    flat("confmat", counts, out)
    flat("consensus", N.consensus(counts, want_norm=True), out)
    flat("consensus.plain", N.consensus(counts), out)
    return out


# =====================================================================================================================
# the augmenter: forward, forward_rows (fp32 and bf16), training-mode forward, train_step with its statistics pass
# =====================================================================================================================
def _aug_case(code):
    def run():
        N = _N()
        from distributed_vae_amd.augmentation import Augmenter_smartseq
        from tests import augtrain_cases as AC
        from tests import augtrain_restatement as AR
        case_ = AC.CASES[1]
        NZ, Z, D, n_dim, B = case_
        s_sd, s_x, s_n = AC.seeds(case_)
        sd = AR.random_state_dict(NZ, Z, D, n_dim, s_sd)
        x = AR.synthetic_batch(B, D, s_x)
        mask, z0, eps = AR.draw_noise(B, D, NZ, Z, AC.P_DROP, s_n, 2)
        A, NR = 2, 2 * B + 3
        g = _gen(15)
        data = pitched(N, torch.cat([x, AR.synthetic_batch(NR - B, D, s_x + 1)]), D + 4)
        rows = torch.randint(0, NR, (B,), generator=g)
        rows[:2] = torch.tensor([NR - 1, 0])
        rows = rows.to(DEV)
        ez0, eeps = torch.randn(A, B, NZ, generator=g), torch.randn(A, B, Z, generator=g)

        def model(train, dtype="fp32"):
            m = Augmenter_smartseq(noise_dim=NZ, latent_dim=Z, input_dim=D, n_dim=n_dim, p_drop=AC.P_DROP)
            m.load_state_dict(sd)
            m = m.to(DEV).train(train)
            m.gemm_dtype = dtype
            m._exec().tune[3] = code                      # MMVAE_TUNE_AUG_TILE
            return m
        out = {}
        for dtype in ("fp32", "bf16"):
            m = model(False, dtype)
            m.set_explicit_noise(ez0, eeps)
            flat(f"forward.{dtype}", m(data[rows].expand(A, -1, -1), True, 0.1), out)
            flat(f"forward.{dtype}.per_arm", m(torch.stack([data[rows], data[:B]]), True, 0.1), out)
            planes = N.tp_planes(data, m.planes_needed())
            flat(f"forward_rows.{dtype}", m.forward_rows(planes, NR, rows, A, 0.1), out)
        m = model(True)
        m.set_explicit_noise(z0[1], eps[1])
        m.set_explicit_dropout(mask[1])
        flat("train_forward", m(x.to(DEV), False, 1.0), out)
        m.set_explicit_noise(z0, eps)
        m.set_explicit_dropout(mask)
        state = m.train_state()
        for s in range(2):
            r = m.train_step(x.to(DEV), state=state, stat_pass=True, keep=True)
            flat(f"train_step{s}", {k: r[k] for k in ("loss", "h", "s", "x_aug")}, out)
        f = m._flat
        flat("train_state", {"params": f["params"], "grads": f["grads"], "running": f["running"], "nbt": f["nbt"],
                             "exp_avg": state["exp_avg"], "exp_avg_sq": state["exp_avg_sq"]}, out)
        torch.cuda.synchronize()
        return out
    CASES.append(Case(f"augmenter[tile={code}]",
                      ("mmvae_aug_pack", "mmvae_augment", "mmvae_augment_rows", "mmvae_aug_train_forward", "mmvae_aug_train_step",
                       "mmvae_tp_planes"), run))


for _c in (0, 23, 84):
    _aug_case(_c)


# =====================================================================================================================
# the data path: gather_rows, to_bf16, tp_planes, adam_step, prune_apply on 37 x 52 and on a 301 x 520 window of 528 columns
# =====================================================================================================================
def _matrices(N):
    g = _gen(16)
    small = torch.randn(37, 52, generator=g).to(DEV)
    return {"37x52": small, "301x520of528": pitched(N, torch.randn(301, 520, generator=g), 528, 4)}


@case("gather_to_bf16_planes", ("mmvae_gather_rows", "mmvae_to_bf16", "mmvae_tp_planes"))
def _():
    N = _N()
    out = {}
    for tag, data in _matrices(N).items():
        n_rows, D = data.shape
        idx = torch.randint(0, n_rows, (2 * n_rows // 3 + 1,), generator=_gen(17))
        idx[:2] = torch.tensor([n_rows - 1, 0])
        idx = idx.to(DEV)
        flat(f"{tag}.gather", N.gather_rows(data, idx), out)
        dst = N.torch.empty(idx.numel(), D, dtype=torch.float32, device=DEV)
        flat(f"{tag}.gather_out", N.gather_rows(data, idx, out=dst), out)
        b16 = N.to_bf16(data)
        assert b16.stride() == data.stride()
        flat(f"{tag}.to_bf16", b16.float(), out)
        ld = data.stride(0)
        pad = padding(b16, (n_rows - 1) * ld + ((D + 3) // 4) * 4)
        assert (pad.numel() > 0) == (ld > D)
        if pad.numel():                                   # (the contiguous matrix has none)
            out[f"pad:{tag}.to_bf16"] = pad
        for planes in (1, 3):
            flat(f"{tag}.planes{planes}", N.tp_planes(data, planes), out)
    return out


@case("adam_prune", ("mmvae_adam_step", "mmvae_prune_apply"))
def _():
    N = _N()
    out = {}
    g = _gen(18)
    for n in (37 * 52, 301 * 520 + 1):
        bufs = []
        for k in range(4):
            t = N.torch.empty(n, dtype=torch.float32, device=DEV)
            t.copy_(torch.randn(n, generator=g).abs_() if k == 3 else torch.randn(n, generator=g))
            bufs.append(t)
        for step in (1, 2):
            N.adam_step(*bufs, step, 1e-3, wd=0.01, decoupled=(step == 2))
        flat(f"adam.{n}", bufs, out)
    dims = N.Dims(3, 2, 52, 37, 5, 9, 2)
    total = dims.A * int(N.param_layout(dims).per_arm)
    bufs = []
    for k in range(4):
        t = N.torch.empty(total, dtype=torch.float32, device=DEV)
        t.copy_(torch.randn(total, generator=g))
        bufs.append(t)
    N.prune_apply(dims, [0b101101011, 0, 0, 0], *bufs)
    flat("prune.all", bufs, out)
    N.prune_apply(dims, [0b001101001, 0, 0, 0], params=bufs[0])
    flat("prune.params", bufs[0], out)
    return out


# =====================================================================================================================
# bound entry points without a case
# =====================================================================================================================
_HOST = "host only: computes a size, count, offset or layout, or runs the kernels' element code on the host; touches no device memory"
_DP = "needs an initialised process group (RCCL, one process per GPU); tests/test_gpu_dp.py runs it"
EXCLUDED = {name: _HOST for name in (
    "mmvae_check_dims", "mmvae_param_layout", "mmvae_workspace_bytes", "mmvae_ws_offset", "mmvae_splits", "mmvae_debug_plan",
    "mmvae_ami_binary_workspace_bytes", "mmvae_silhouette_workspace_bytes", "mmvae_state_corr_workspace_bytes",
    "mmvae_group_moments_workspace_bytes", "mmvae_gauss_scores_workspace_bytes", "mmvae_leaf_merge_workspace_bytes",
    "mmvae_zinb_nll_workspace_bytes", "mmvae_zinb_terms_workspace_bytes", "mmvae_zinb_head_grads_workspace_bytes",
    "mmvae_zinb_head_grads_segments", "mmvae_zinb_d10_grad_workspace_bytes", "mmvae_zinb_d10_grad_segments",
    "mmvae_zinb_step_grads_workspace_bytes", "mmvae_decoder_trunk_grads_workspace_bytes", "mmvae_decoder_trunk_grads_segments",
    "mmvae_zinb_head_layout", "mmvae_zinb_step_workspace_bytes", "mmvae_debug_zinb_grad_host", "mmvae_debug_digamma_host",
    "mmvae_count_logp_workspace_bytes", "mmvae_debug_count_logp_host", "mmvae_debug_count_sample_host",
    "mmvae_forest_workspace_bytes", "mmvae_gram_workspace_bytes", "mmvae_gram_segments", "mmvae_symm_mul_workspace_bytes",
    "mmvae_pca_project_workspace_bytes", "mmvae_gene_stats_workspace_bytes", "mmvae_aug_packed_floats",
    "mmvae_aug_workspace_bytes", "mmvae_aug_param_layout", "mmvae_aug_train_workspace_bytes", "mmvae_tp_planes_bytes",
    "mmvae_decode_workspace_bytes", "mmvae_state_changes_workspace_bytes", "mmvae_encode_workspace_bytes")}
EXCLUDED.update({name: _DP for name in ("mmvae_dp_unique_id", "mmvae_dp_init", "mmvae_allreduce_grads", "mmvae_dp_destroy")})
EXCLUDED["mmvae_debug_stage"] = ("debug twin: replays single launches of mmvae_train_step / mmvae_forward / mmvae_backward in the "
                                 "step's own workspace; the production entries are covered by the step and calls cases")

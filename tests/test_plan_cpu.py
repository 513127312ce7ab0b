"""CPU (no GPU): make_plan's decision table, read back through mmvae_debug_plan (host only) and held to tests/plan_cases.py.

  * every (row, engine, call kind) of the table returns exactly its hand-written plan;
  * the same without a side stream: plan_cases.without_side() of that plan, on the same split factors and workspace size;
  * closure: over the table, the fused step reaches every kernel family, zero fill, coupling placement and both values of
    every bool -- or the value is named in UNREACHABLE with its reason, and a brute-force sweep proves it never appears;
  * the invariants make_plan states in its comments hold over the same sweep.
"""
import ctypes as C
import itertools

import pytest

import distributed_vae_amd  # noqa: F401
from distributed_vae_amd import _native as N
from tests import plan_cases as P

SKIP_FIELDS = ("kind", "gd10_slabs", "dw11_slabs")


def _hyper(row, engine, training=1):
    return N.Hyper(0.005, 1.0, 1.0, 1.0, 1e-8, 0.01, row.x_drop, row.s_drop, int(row.hard), training, 0 if training else 1,
                   P.ENGINES[engine])


def _exec(engine, side=True):
    ex = N.Exec()
    ex.tune[N.TUNE_ENGINE] = P.ENGINES[engine]
    if side:
        ex.side_stream = 1          # never dereferenced: "has a side stream"
    return ex


def _splits(dims, ex):
    sp = (C.c_int32 * 6)()
    N.check(N.lib().mmvae_splits(C.byref(dims), C.byref(ex), C.byref(sp)), "mmvae_splits")
    return list(sp)


def _check(row, engine, kind, has_x16=False, side=None):
    """side: None -- the exec has a side stream where the row says so; False -- it has none, and the plan is
    plan_cases.without_side() of the row's."""
    d = N.Dims(row.A, row.B, row.D, row.H, row.L, row.C, row.S)
    ex = _exec(engine, row.side if side is None else side)
    training = 0 if kind in ("DECODE", "TRAVERSE") else 1   # (CLASSIFY too is planned in eval mode whatever it is handed)
    got = N.debug_plan(d, _hyper(row, engine, training), ex, has_x16=has_x16, **P.plan_args(row, kind))
    want = P.expected(row, engine, kind, has_x16)
    if side is False:
        want = P.without_side(want)
    sp = _splits(d, ex)
    i_gd10, i_dw11 = P.slab_sources(want)
    want["gd10_slabs"], want["dw11_slabs"] = sp[i_gd10], sp[i_dw11]
    diff = {k: (got[k], want[k]) for k in N.PLAN_NAMES if got[k] != want[k]}
    assert not diff, (row.name, engine, kind, "got, want:", diff)
    lit = P.slabs_of(row.name, engine)
    if lit and kind == "STEP":
        for name, v in zip(("gd10_slabs", "dw11_slabs"), lit):
            assert v is None or got[name] == v, (row.name, engine, name, got[name], v)


@pytest.mark.parametrize("engine", list(P.ENGINES))
@pytest.mark.parametrize("row", P.ROWS, ids=lambda r: r.name)
def test_every_row_takes_its_hand_written_plan(row, engine):
    for kind in P.KINDS:
        _check(row, engine, kind)


SIDE_ROWS = [r for r in P.ROWS if r.side]


@pytest.mark.parametrize("engine", list(P.ENGINES))
@pytest.mark.parametrize("row", SIDE_ROWS, ids=lambda r: r.name)
def test_every_row_without_a_side_stream_takes_without_side_of_its_plan(row, engine):
    """An mmvae_exec without a side stream: every call kind's plan is the row's with exactly the five fields
    plan_cases.without_side() names changed; the slab counts are the same split factors."""
    for kind in P.KINDS:
        _check(row, engine, kind, side=False)


def test_without_side_is_the_literal_noside_row():
    for engine in P.ENGINES:
        assert P.STEP["noside"][engine] == P.without_side(P.STEP["h100"][engine]), engine
        assert P.without_side(P.STEP["noside"][engine]) == P.STEP["noside"][engine], engine
    assert P.BY_NAME["noside"]._replace(name="h100", side=True) == P.BY_NAME["h100"]
    assert set(P.NOSIDE_GPU) <= {r.name for r in P.GPU_ROWS} and len(set(P.NOSIDE_GPU)) == len(P.NOSIDE_GPU) == 9


@pytest.mark.parametrize("engine", list(P.ENGINES))
@pytest.mark.parametrize("row", P.ROWS, ids=lambda r: r.name)
def test_splits_and_workspace_do_not_depend_on_the_side_stream(row, engine):
    """default_splits and make_layout do not read mmvae_exec.side_stream: the same split factors and the same workspace size
    with and without one (and without an exec at all on engine 0, whose tune[] is all zeros).  The bit-identity checks of
    tests/test_gpu_noside.py rest on this: the same number of slabs summed in the same order on either engine."""
    d = N.Dims(row.A, row.B, row.D, row.H, row.L, row.C, row.S)
    L = N.lib()
    with_side, without = _exec(engine, True), _exec(engine, False)
    assert with_side.side_stream and not without.side_stream
    assert _splits(d, with_side) == _splits(d, without), (row.name, engine)
    nbytes = [int(L.mmvae_workspace_bytes(C.byref(d), C.byref(ex))) for ex in (with_side, without)]
    assert nbytes[0] == nbytes[1] > 0, (row.name, engine, nbytes)
    if engine == "fp32_mfma":
        sp = (C.c_int32 * 6)()
        assert L.mmvae_splits(C.byref(d), None, C.byref(sp)) == 0
        assert list(sp) == _splits(d, without) and int(L.mmvae_workspace_bytes(C.byref(d), None)) == nbytes[1]


def test_table_is_complete():
    assert set(P.STEP) == set(P.BY_NAME) and len(P.BY_NAME) == len(P.ROWS)
    for name, per_engine in P.STEP.items():
        assert set(per_engine) == set(P.ENGINES), name
        for e, p in per_engine.items():
            assert set(p) == set(N.PLAN_NAMES) - set(SKIP_FIELDS), (name, e)


@pytest.mark.parametrize("row,narrow", [("h100", True), ("h124", True), ("d132_h100", False), ("d1004_h64", False), ("h128", False)])
def test_bf16_storage_narrow_operands(row, narrow):
    """mmvae_train_step_rows with the matrix's bf16 copy: the narrow operands are read as bf16 where D % 8 == 0 and the bf16
    tiles fit; dZ11 then travels as bf16.  The other engines ignore the copy."""
    r = P.BY_NAME[row]
    for engine in P.ENGINES:
        _check(r, engine, "STEP_ROWS", has_x16=True)
    d = N.Dims(r.A, r.B, r.D, r.H, r.L, r.C, r.S)
    got = N.debug_plan(d, _hyper(r, "bf16"), _exec("bf16"), "STEP_ROWS", has_x16=True)
    assert got["narrow"] is narrow and got["dz11_bf16"] is (r.H <= 124)


def test_read_back_checks_its_arguments():
    L = N.lib()
    out = (C.c_int32 * N.PLAN_FIELDS)()
    d, h = N.Dims(2, 300, 520, 100, 10, 92, 2), _hyper(P.BY_NAME["h100"], "fp32x3")
    assert L.mmvae_debug_plan(C.byref(d), C.byref(h), None, 0, 16, 16, 0, 0, 1, C.byref(out)) == 0
    assert list(out)[:3] == [0, 1, 3]                                      # STEP, fast, GEMM_X3 (no exec: no side stream)
    assert L.mmvae_debug_plan(C.byref(d), C.byref(h), None, 9, 16, 16, 0, 0, 1, C.byref(out)) == -1
    assert L.mmvae_debug_plan(C.byref(d), None, None, 0, 16, 16, 0, 0, 1, C.byref(out)) == -1
    assert L.mmvae_debug_plan(C.byref(d), C.byref(h), None, 0, 16, 16, 0, 0, 1, None) == -1
    assert L.mmvae_debug_plan(C.byref(N.Dims(2, 300, 520, 129, 10, 92, 2)), C.byref(h), None, 0, 16, 16, 0, 0, 1, C.byref(out)) == -2
    h.gemm_bf16 = 3
    assert L.mmvae_debug_plan(C.byref(d), C.byref(h), None, 0, 16, 16, 0, 0, 1, C.byref(out)) == -1
    assert len(N.PLAN_NAMES) == N.PLAN_FIELDS == 23 and N.CALL_KINDS["TRAVERSE"] == 8


# ---- closure and invariants --------------------------------------------------------------------------------------------
# values of a Plan field the fused step (CALL_STEP) cannot take, each with the line of make_plan that says so
UNREACHABLE = {
    ("narrow", True): "needs the bf16 copy of the matrix, which only mmvae_train_step_rows takes (Ctx::x16)",
    ("rowmap", True): "kind == CALL_STEP_ROWS",
    ("dz11_bf16", True): "implies rowmap",
    ("bwd_small_planes", True): "kind == CALL_BACKWARD",
    ("dec_planes", True): "set under kind == CALL_DECODE only",
    ("fc11", "FC11_OUT_BF16"): "set under kind == CALL_DECODE only",
    ("fc11", "FC11_OUT_X3"): "set under kind == CALL_DECODE only",
    ("zero", "ZERO_NONE"): "a step is a forward pass in training mode (train_step_impl refuses eval mode)",
}


def _domain(name):
    return N.PLAN_ENUMS[name] if name in N.PLAN_ENUMS else (False, True)


def _sweep():
    """(dims tuple, engine, side, has_x16-rows call?, plan values, splits) over the shape rules' boundaries."""
    L = N.lib()
    Hs = sorted(set(range(4, 129, 4)) | set(range(97, 114)) | set(range(121, 129)) | {5, 6, 7})
    Ds = (4, 36, 100, 130, 132, 520, 522, 1004)                 # residues 4, 36, 100, 2, 4, 8, 10, 108 mod 128
    lat = ((10, 92, 2), (32, 96, 16), (33, 92, 2), (10, 97, 2), (10, 92, 17), (10, 125, 3), (10, 125, 4))
    Bs = (2, 31, 128, 129, 5000, 32768)
    out = (C.c_int32 * N.PLAN_FIELDS)()
    sp = (C.c_int32 * 6)()
    for eng in (0, 1, 2):
        h = N.Hyper(0.005, 1.0, 1.0, 1.0, 1e-8, 0.01, 0.5, 0.0, 0, 1, 0, eng)
        exs = []
        for side in (0, 1):
            ex = N.Exec()
            ex.tune[N.TUNE_ENGINE] = eng
            ex.side_stream = side or None
            exs.append(ex)
        for A, H, D, (Ld, Cc, S), B in itertools.product(range(1, 9), Hs, Ds, lat, Bs):
            d = N.Dims(A, B, D, H, Ld, Cc, S)
            assert L.mmvae_splits(C.byref(d), C.byref(exs[0]), C.byref(sp)) == 0
            spl = tuple(sp)
            for side in (0, 1):
                for kind, x16 in ((0, 0), (1, 1)):
                    assert L.mmvae_debug_plan(C.byref(d), C.byref(h), C.byref(exs[side]), kind, 16, 16, 0, x16, 1, C.byref(out)) == 0
                    yield (A, B, D, H, Ld, Cc, S), eng, side, kind, tuple(out), spl


@pytest.fixture(scope="module")
def sweep():
    """Distinct (kind, plan values, fast dims?, slab capacities) of the sweep, each with one shape that gave it."""
    seen = {}
    n = 0
    for dims, eng, side, kind, vals, spl in _sweep():
        n += 1
        fastdims = dims[2] % 4 == 0 and dims[3] % 4 == 0
        key = (kind, vals, max(spl[1], spl[4]), max(spl[2], spl[5]))
        if key not in seen:
            seen[key] = (dims, eng, side, fastdims)
    return n, seen


def test_the_table_reaches_every_value_the_step_can_take(sweep):
    names = [n for n in N.PLAN_NAMES if n not in SKIP_FIELDS]
    reached = {n: set() for n in names}
    for row in P.ROWS:
        for engine in P.ENGINES:
            for n in names:
                reached[n].add(P.STEP[row.name][engine][n])
    missing = {(n, v) for n in names for v in _domain(n) if v not in reached[n]}
    assert missing == set(UNREACHABLE), (sorted(map(str, missing - set(UNREACHABLE))), sorted(map(str, set(UNREACHABLE) - missing)))
    # ... and what the table does not reach, no shape does
    n_calls, seen = sweep
    assert n_calls > 500000
    idx = {n: i for i, n in enumerate(N.PLAN_NAMES)}
    for (kind, vals, _, _), where in seen.items():
        if kind != N.CALL_KINDS["STEP"]:
            continue
        for (name, v), why in UNREACHABLE.items():
            got = N.PLAN_ENUMS[name][vals[idx[name]]] if name in N.PLAN_ENUMS else bool(vals[idx[name]])
            assert got != v, (name, v, why, where)


def test_fused_fc11_loss_slots_always_fit(sweep):
    """fc11_slots_fit (and FC11_ZG's own slot check) can only refuse a shape if make_layout's n11 were smaller than the
    kernels' block count; n11 = (cdiv(B, 64) + 2) (max(ns_fc11, ks_gd10) + 1) + cdiv(D, 64) > cdiv(B, 128) ks_gd10 always.  So
    over the sweep a fast fp32x3 step within 112 columns is ALWAYS FC11_X3, and fc_dim 100 on engine 0 ALWAYS FC11_ZG."""
    _, seen = sweep
    idx = {n: i for i, n in enumerate(N.PLAN_NAMES)}
    for (kind, vals, _, _), (dims, eng, side, _) in seen.items():
        if kind != 0 or not vals[idx["fast"]]:
            continue
        fc11 = N.PLAN_ENUMS["fc11"][vals[idx["fc11"]]]
        H = dims[3]
        if eng == 2 and H + 1 <= 112:
            assert fc11 == "FC11_X3", dims
        if eng == 0 and H == 100:
            assert fc11 == "FC11_ZG", dims


def test_invariants_make_plan_states(sweep):
    _, seen = sweep
    idx = {n: i for i, n in enumerate(N.PLAN_NAMES)}
    for (kind, vals, cap_gd10, cap_dw11), (dims, eng, side, fastdims) in seen.items():
        p = {n: vals[i] for n, i in idx.items()}
        where = (dims, eng, side, kind)
        assert (N.PLAN_ENUMS["big"][p["big"]] == "GEMM_GENERAL") == (not p["fast"]), where
        assert p["fast"] == fastdims, where                        # (aligned pointers here, B D < 2^30)
        if p["rowmap"]:
            assert N.PLAN_ENUMS["zero"][p["zero"]] == "ZERO_PRESPLIT", where
        if p["dz11_bf16"]:
            assert p["rowmap"], where
        if p["fc11_fork_rides"]:
            assert p["loss_on_side"], where
        if p["loss_on_side"] or p["dw11_side"] or p["lat_fork_rides"]:
            assert side, where
        # the slab regions make_layout sized: GD10_slab for max(ns_fc11, ks_gd10) slabs, dw11_slab for max(ks_dw, ks_dw11)
        assert 1 <= p["gd10_slabs"] <= cap_gd10 and 1 <= p["dw11_slabs"] <= cap_dw11, where

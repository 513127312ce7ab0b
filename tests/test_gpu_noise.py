"""-m gpu: the noise the kernels draw in Philox mode (mmvae_noise.mode == 1) against the host restatement of the contract
(tests/noise_restatement.py, itself held to Random123's known answers in tests/test_noise_cpu.py), bit for bit:

  a. mmvae_dump_noise equals the restatement on every array, over every field width of the input mask, ragged shapes and the
     whole key / counter space (64-bit seeds, offsets past 2^32);
  b. every kernel path make_plan can choose consumes exactly what the dump says: each row of tests/plan_cases.py on each
     engine takes one fused step (and one forward / loss / backward) in Philox mode and again on the explicit replay of the
     dump at that seed and offset -- loss vector, flat gradient and BatchNorm buffers bit-identical; the same at an offset
     with a non-zero high word, on the row-indexed step, a pruned step, the bf16 copy, the training-mode encoder and the
     state traversal;
  c. three consecutive trainer steps advance the offset by one each.

Bit equality needs a path that is reproducible run to run: every case first repeats its explicit step and asserts that.
"""
import itertools

import pytest
import torch

from oracle import restatement as R
from tests import noise_restatement as NR
from tests import plan_cases as P
from tests import test_gpu_plan_matrix as PM

pytestmark = pytest.mark.gpu

SEED64 = 0x5EED0123456789
ENGINES = list(P.ENGINES)
ROW_IDS = [r.name for r in P.GPU_ROWS]
# x_drop -> field width m of the input mask (tests/test_noise_cpu.py::test_field_width_and_threshold_table)
P_OF_M = {1: 0.5, 2: 0.25, 4: 0.8125, 8: 0.98828125, 16: 0.3}


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _restated(A, B, D, C, S, x_drop, s_drop, seed, offset, device=None):
    d = {k: torch.from_numpy(v) for k, v in NR.dump_noise(A, B, D, C, S, x_drop, s_drop, seed, offset).items()}
    return d if device is None else {k: v.to(device) for k, v in d.items()}


# ---- a. the dump against the restatement ------------------------------------------------------------------------------
def _dump_cases():
    Ds, Bs, Cs, Ss, As = (4, 36, 50, 127, 129, 520), (2, 57, 129), (9, 97, 128), (1, 3, 17), (1, 2, 5, 8)
    cases = []
    # every field width at every D (a partial last group for every width, D % 32 != 0, D % 4 != 0); B, C, S, A rotate so that
    # each value meets each width, with B * C and B * S off multiples of 4 (a group of four words straddles rows)
    for i, (m, D) in enumerate(itertools.product(P_OF_M, Ds)):
        cases.append((As[i % 4], Bs[(i + i // 6) % 3], D, Cs[(i // 2) % 3], Ss[(i + i // 3) % 3], P_OF_M[m], (0.2, 0.25, 0.5)[i % 3],
                      SEED64, 7 + i))
    # the saturated thresholds: keep all / keep none
    cases += [(2, 57, 50, 9, 3, 0.0, 0.0, SEED64, 3), (2, 57, 50, 9, 3, 1.0, 1.0, SEED64, 3)]
    # key and counter words, one factor at a time at one shape, then the top of both together
    for seed in (1, 2 ** 32 - 1, 2 ** 32, SEED64, 2 ** 64 - 1):
        cases.append((5, 57, 129, 97, 3, 0.3, 0.2, seed, 11))
    for offset in (0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 5, 2 ** 40):
        cases.append((5, 57, 129, 97, 3, 0.25, 0.2, 1, offset))
    cases += [(8, 57, 129, 97, 3, 0.5, 0.2, 2 ** 64 - 1, 2 ** 40), (8, 57, 129, 97, 3, 0.98828125, 0.2, 2 ** 32, 2 ** 32 + 5)]
    return cases


DUMP_CASES = _dump_cases()


@pytest.mark.parametrize("case", DUMP_CASES, ids=lambda c: "A{}-B{}-D{}-C{}-S{}-x{}-s{}-k{:x}-o{:x}".format(*c))
def test_dump_equals_restatement(case):
    from distributed_vae_amd import _native as N
    from tests import gpu_util as U
    A, B, D, C, S, x_drop, s_drop, seed, offset = case
    eng = N.Engine(A, B, D, 16, 4, C, S, U.DEV)
    hyper = N.Hyper(0.005, 1.0, 1.0, 1.0, 1e-8, 0.01, x_drop, s_drop, 0, 1, 0, 0)
    got = eng.dump_noise(hyper, N.make_noise(None, seed, offset))
    torch.cuda.synchronize()
    want = _restated(A, B, D, C, S, x_drop, s_drop, seed, offset)
    for k in ("x_mask", "u_gumbel", "u_state", "s_mask"):
        assert got[k].dtype == want[k].dtype and tuple(got[k].shape) == tuple(want[k].shape), k
        g, w = _bits(got[k]), _bits(want[k])
        assert torch.equal(g, w), (k, int((g != w).sum()), (g != w).nonzero()[:4].tolist())


# ---- b. every kernel path consumes the dump ---------------------------------------------------------------------------
def _replay_identity(name, engine, seed, offset, paths=("fused", "api")):
    from distributed_vae_amd import _native as N
    row = P.BY_NAME[name]
    U, h, sd, x, _, m, eng = PM._env(row, engine)
    params, xd, xs = PM._place(m, x, row.misalign)
    hyper = m._hyper(1.0, False)
    dump = eng.dump_noise(hyper, N.make_noise(None, seed, offset))
    state0 = (m._bn_flat.clone(), m._nbt.clone())
    for path in paths:
        run = {"fused": PM._fused, "api": PM._api}[path]

        def step(nz):
            buf, g = run(m, eng, nz, params, xd, xs, state0)
            return buf.clone(), g.clone(), m._bn_flat.clone(), m._nbt.clone()
        ex1 = step(dump)
        ex2 = step(dump)
        ph = step(N.make_noise(None, seed, offset))
        assert bool(torch.isfinite(ph[0]).all()) and bool(torch.isfinite(ph[1]).all()) and float(ph[1].abs().max()) > 0
        # (every engine's fused step and forward / loss / backward proved bit-reproducible on every row: none is held to the
        # looser gates of test_gpu_plan_matrix._same_to_api_gates)
        for u, v in zip(ex1, ex2):
            assert _same_bits(u, v), (name, engine, path, "the explicit step is not reproducible run to run")
        for what, u, v in zip(("loss vector", "gradient", "BatchNorm statistics", "BatchNorm counters"), ph, ex1):
            assert _same_bits(u, v), (name, engine, path, what, int((_bits(u) != _bits(v)).sum()))


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("name", ROW_IDS)
def test_plan_row_philox_step_equals_replay_of_its_dump(name, engine):
    _replay_identity(name, engine, SEED64, 42)


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("name", ["h100", "sdrop_hard"])
def test_step_with_a_high_offset_word_equals_replay(name, engine):
    """offset = 2^32 + 5: step_hi = 1 reaches counter word 2 beside the stream id, in every kernel that draws."""
    from distributed_vae_amd import _native as N
    _replay_identity(name, engine, SEED64, 2 ** 32 + 5)
    # (and it is another step than offset 5: the high word is not dropped on the way to the kernels)
    row = P.BY_NAME[name]
    U, h, sd, x, _, m, eng = PM._env(row, engine)
    params, xd, xs = PM._place(m, x, None)
    state0 = (m._bn_flat.clone(), m._nbt.clone())
    hi = PM._fused(m, eng, N.make_noise(None, SEED64, 2 ** 32 + 5), params, xd, xs, state0)[0].clone()
    lo = PM._fused(m, eng, N.make_noise(None, SEED64, 5), params, xd, xs, state0)[0].clone()
    assert not _same_bits(hi, lo)


def _rows_case(row, seed=31):
    from tests import gpu_util as U
    h = R.Hyper(input_dim=row.D, fc_dim=row.H, n_categories=row.C, state_dim=row.S, lowD_dim=row.L, x_drop=row.x_drop,
                s_drop=row.s_drop, n_arm=row.A, hard=row.hard)
    sd = R.init_state_dict(h, seed)
    n_rows = 3 * row.B + 5
    # (bf16-representable values: the matrix's bf16 copy holds the same numbers)
    data = R.synthetic_batch(n_rows, row.D, seed=32).to(torch.bfloat16).float().to(U.DEV)
    rows = torch.randint(0, n_rows, (row.B,), generator=torch.Generator().manual_seed(33))
    rows[:2] = torch.tensor([n_rows - 1, 0])
    return U, h, sd, data, rows.to(U.DEV)


def _model_step(U, h, sd, engine, noise, step, offset=None):
    """One model, one step: `noise` explicit (a dict), or None for Philox at (SEED64, offset).  Returns the step's loss vector,
    gradient, BatchNorm buffers and the model."""
    m = U.build_model(h, sd)
    m.train()
    m.gemm_dtype = engine
    if noise is None:
        m._noise_seed, m._noise_offset = SEED64, offset - 1
    else:
        m.set_explicit_noise(noise)
    buf = step(m).clone()
    torch.cuda.synchronize()
    if noise is None:
        assert m._noise_offset == offset
    return [buf, m.flat_grad().clone(), m._bn_flat.clone(), m._nbt.clone()], m


def _assert_step_replays(U, h, sd, engine, B, step, offset, what):
    from distributed_vae_amd import _native as N
    ph, m = _model_step(U, h, sd, engine, None, step, offset)
    assert bool(torch.isfinite(ph[0]).all()) and float(ph[1].abs().max()) > 0
    dump = m._ensure(B).dump_noise(m._hyper(1.0, False), N.make_noise(None, SEED64, offset))
    ex1, _ = _model_step(U, h, sd, engine, dump, step)
    ex2, _ = _model_step(U, h, sd, engine, dump, step)
    for u, v in zip(ex1, ex2):
        assert _same_bits(u, v), (what, "the explicit step is not reproducible run to run")
    for u, v in zip(ph, ex1):
        assert _same_bits(u, v), (what, int((_bits(u) != _bits(v)).sum()))


ROWS_CASES = [(n, e) for n in ("h100", "b129", "d36_h100", "a4", "sdrop_hard") for e in ("bf16", "fp32x3")
              if P.expected(n, e, "STEP_ROWS")["rowmap"]]


@pytest.mark.parametrize("name,engine", ROWS_CASES)
def test_row_indexed_step_equals_replay_of_the_batch_rows_dump(name, engine):
    """The row-indexed step draws by BATCH row: cell b of the batch takes counter row b whichever resident row it reads (the
    map starts at the matrix's last row and its first).  Its Philox step equals the row-indexed step on the dump of a
    [A, B, D] batch at that seed and offset."""
    assert len(ROWS_CASES) >= 8
    row = P.BY_NAME[name]
    U, h, sd, data, rows = _rows_case(row)
    _assert_step_replays(U, h, sd, engine, row.B, lambda m: m.fused_train_step_rows(data, rows, 1.0, None, do_adam=False), 77,
                         (name, engine))


def test_row_indexed_step_on_the_bf16_copy_equals_replay():
    import distributed_vae_amd  # noqa: F401
    from distributed_vae_amd import _native as N
    row = P.BY_NAME["b129"]
    assert row.D % 8 == 0 and P.expected(row, "bf16", "STEP_ROWS", has_x16=True)["narrow"]
    U, h, sd, data, rows = _rows_case(row)
    data16 = N.to_bf16(data)
    _assert_step_replays(U, h, sd, "bf16", row.B,
                         lambda m: m.fused_train_step_rows(data, rows, 1.0, None, do_adam=False, data16=data16), 78, "data16")


@pytest.mark.parametrize("engine", ENGINES)
def test_pruned_step_equals_replay(engine):
    """A step under mmvae_hyper.cat_mask (the pruning phase) draws the same streams: the Gumbel uniform of category k is
    element b * C + k whether or not its neighbours are kept."""
    from tests import gpu_util as U
    row = P.BY_NAME["sdrop_hard"]
    h = R.Hyper(input_dim=row.D, fc_dim=row.H, n_categories=row.C, state_dim=row.S, lowD_dim=row.L, x_drop=row.x_drop,
                s_drop=row.s_drop, n_arm=row.A, hard=False)
    sd = R.init_state_dict(h, 31)
    x = R.synthetic_batch(row.B, row.D, seed=3).to(U.DEV)
    kept = [k for k in range(row.C) if k % 3 != 1 and k != 64]
    _assert_step_replays(U, h, sd, engine, row.B,
                         lambda m: m.fused_train_step(x.expand(row.A, -1, -1), 1.0, None, do_adam=False, mask=kept), 79,
                         ("pruned", engine))


@pytest.mark.parametrize("D,x_drop", [(52, 0.5), (50, 0.3), (136, 0.25)])
def test_training_mode_encoder_takes_the_restated_mask_of_its_arm(D, x_drop):
    """mixVAE_model.encoder in training mode: arm a's input mask is the restatement's x_mask[a] at the offset the call consumes
    (one per call) -- its outputs and the arm's BatchNorm buffers equal the call on that explicit mask bit for bit."""
    from tests import gpu_util as U
    A, n, offset = 3, 57, 2 ** 32 + 20
    h = R.Hyper(input_dim=D, fc_dim=20, n_categories=9, state_dim=2, lowD_dim=4, n_arm=A, x_drop=x_drop)
    sd = R.init_state_dict(h, 4)
    x = R.synthetic_batch(n, D).to(U.DEV)
    m1, m2 = U.build_model(h, sd), U.build_model(h, sd)
    m1.train()
    m2.train()
    m1._noise_seed, m1._noise_offset = SEED64, offset
    outs = []
    for i, arm in enumerate((2, 0, 1)):
        got = m1.encoder(x, arm)
        assert m1._noise_offset == offset + i + 1
        mask = _restated(A, n, D, 9, 2, x_drop, 0.0, SEED64, offset + i + 1, U.DEV)["x_mask"]
        m2.set_explicit_noise({"x_mask": mask})
        want = m2.encoder(x, arm)
        torch.cuda.synchronize()
        assert _same_bits(got[0], want[0]) and _same_bits(got[1], want[1]), arm
        outs.append(got[0].clone())
    assert _same_bits(m1._bn_flat, m2._bn_flat) and torch.equal(m1._nbt, m2._nbt)
    assert bool(torch.isfinite(outs[0]).all()) and not _same_bits(outs[0], outs[1])


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("n_samp", [1, 7])
def test_state_changes_draws_the_restated_uniforms(n_samp, engine):
    """state_changes in Philox mode == state_changes on the restated draws (element samp * B + b of each arm's state stream)."""
    from tests import test_gpu_decode as TD
    A, B, D, offset = 3, 5, 136, 2 ** 32 + 30
    m = TD._model(A, D, 100, 10, 12, 3, seed=3)
    m.gemm_dtype = engine
    x = (torch.relu(torch.randn(B, D, generator=torch.Generator().manual_seed(6))) * 2).to(TD.DEV)
    m._noise_seed, m._noise_offset = SEED64, offset - 1
    got, _ = m.state_changes(x, 1, 1.0, n_samp=n_samp)
    assert m._noise_offset == offset
    u = torch.from_numpy(NR.state_changes_draws(A, n_samp, B, SEED64, offset)).to(TD.DEV)
    m.set_explicit_state_noise(u)
    want, _ = m.state_changes(x, 1, 1.0, n_samp=n_samp)
    again, _ = m.state_changes(x, 1, 1.0, n_samp=n_samp)
    assert tuple(got.shape) == (A, n_samp, B, D) and bool(torch.isfinite(got).all())
    assert _same_bits(want, again), "the explicit traversal is not reproducible run to run"
    assert _same_bits(got, want), int((_bits(got) != _bits(want)).sum())
    # the draws matter: another offset gives another traversal
    m.set_explicit_state_noise(None)
    other, _ = m.state_changes(x, 1, 1.0, n_samp=n_samp)
    assert not _same_bits(got, other)


# ---- c. the trainer's offsets -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", ENGINES)
def test_three_trainer_steps_consume_offsets_one_by_one(engine):
    """fused_train_step draws step k of a model at offset _noise_offset + k: three Adam steps in Philox mode equal three steps
    on the restated dumps of offsets + 1 .. + 3, parameters and loss vectors bit for bit."""
    from distributed_vae_amd.cpl_mixvae import FusedAdam
    from tests import gpu_util as U
    A, B, offset = 3, 70, 2 ** 32 - 2          # the second step crosses into the high word
    h = R.Hyper(input_dim=132, fc_dim=100, n_categories=12, state_dim=3, lowD_dim=6, n_arm=A, x_drop=0.25, s_drop=0.25)
    sd = R.init_state_dict(h, 31)
    xs = [R.synthetic_batch(B, h.input_dim, seed=40 + s).to(U.DEV) for s in range(3)]
    res = []
    for mode in ("philox", "explicit"):
        m = U.build_model(h, sd)
        m.train()
        m.gemm_dtype = engine
        if mode == "philox":
            m._noise_seed, m._noise_offset = SEED64, offset
        else:
            m.set_explicit_noise([_restated(A, B, h.input_dim, 12, 3, 0.25, 0.25, SEED64, offset + 1 + s, U.DEV) for s in range(3)])
        opt = FusedAdam(m, lr=1e-3)
        bufs = [m.fused_train_step(xs[s].expand(A, -1, -1), 1.0, opt, do_adam=True).clone() for s in range(3)]
        torch.cuda.synchronize()
        if mode == "philox":
            assert m._noise_offset == offset + 3
        res.append([torch.stack(bufs), m.flat_parameters().detach().clone(), m._bn_flat.clone()])
    assert bool(torch.isfinite(res[0][0]).all()) and not _same_bits(res[0][0][0], res[0][0][1])
    for what, u, v in zip(("loss vectors", "parameters", "BatchNorm statistics"), *res):
        assert _same_bits(u, v), (what, int((_bits(u) != _bits(v)).sum()))

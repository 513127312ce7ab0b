"""-m gpu: the pruning phase on the device -- mmvae_prune_apply's exact write set, the fused train step under a category mask
against the fp64 masked oracle (tests/prune_restatement.py) and against the three-call path, the row-indexed masked step,
and the loop ``cpl_mixVAE.prune`` with its checkpoints and its resume.

Gates: those of tests/test_gpu_parity.py (LOSS_TOL, GRAD_TOL imported from it, not restated): the loss vector at
gpu_util.assert_loss_vector's per-term tolerances; every gradient tensor at ``rel_err < GRAD_TOL`` of its largest magnitude
against the plain fp64 masked oracle (prune_restatement.masked_grads) at the two golden shapes and the C = 70 shape.  The two
fc_dim = 100 shapes take what the suite applies at that width (test_full_size_against_oracle, test_gpu_plan_matrix):
gpu_util.flip_aware_oracle + assert_gradients_tight -- a step there takes tens of thousands of hidden ReLU decisions, and a
pre-activation within fp32 rounding of zero is decided either way by any fp32 evaluation (on the lat_half shape the fp32 CPU
oracle itself differs from fp64 in one decision, at a pre-activation of 8e-9; one such decision moves an encoder gradient
by 1e-1 of its scale while the loss agrees to 2e-7).  Parameters after three Adam steps as test_golden_adam_trajectory bounds them.  The oracle of step k starts from the device's
own parameters and running statistics at the start of step k (each step's arithmetic is compared on identical inputs: Adam
turns rounding noise on near-zero gradients into O(lr) parameter differences, which would otherwise compound)."""
import os

import numpy as np
import pytest
import torch

from oracle import restatement as R
from tests import golden_util as G
from tests import plan_cases as P
from tests import prune_restatement as PR
from tests.test_gpu_parity import GRAD_TOL, LOSS_TOL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FP32_ENGINES = ["fp32x3", "fp32_mfma"]

# name -> (A, B, D, H, L, C, S, s_drop, pruned)
_LAT_HALF, _LAT_WAVE = P.BY_NAME["b31"], P.BY_NAME["lat_c97_b57"]        # one row per latent kernel form (Plan::lat_half)
SHAPES = {
    "tiny_a2": (2, 32, 64, 16, 5, 7, 2, 0.0, [1, 4]),                    # tests/golden/tiny_a2.npz's shape
    "tiny_a3_sdrop": (3, 48, 96, 16, 5, 11, 2, 0.2, [0, 10]),            # tests/golden/tiny_a3_sdrop.npz's
    "c70_words": (2, 40, 64, 32, 10, 70, 2, 0.0, [0, 31, 32, 63, 64, 69]),   # both word boundaries of cat_mask
    "lat_half": (_LAT_HALF.A, _LAT_HALF.B, _LAT_HALF.D, _LAT_HALF.H, _LAT_HALF.L, _LAT_HALF.C, _LAT_HALF.S, 0.0,
                 [2, 30, 33, 91]),
    "lat_wave": (_LAT_WAVE.A, _LAT_WAVE.B, _LAT_WAVE.D, _LAT_WAVE.H, _LAT_WAVE.L, _LAT_WAVE.C, _LAT_WAVE.S, 0.0,
                 [0, 64, 95, 96]),
}


def test_shapes_are_the_goldens_and_one_per_latent_form():
    from distributed_vae_amd import _native as N
    for name in ("tiny_a2", "tiny_a3_sdrop"):
        assert tuple(int(v) for v in G.load(name)["cfg"]) == SHAPES[name][:7]
    for name, half in (("lat_half", True), ("lat_wave", False), ("c70_words", True)):
        A, B, D, H, L, C, S = SHAPES[name][:7]
        h = N.Hyper(0.005, 1.0, 1.0, 1.0, 1e-8, 0.01, 0.5, 0.0, 0, 1, 0, 2)
        assert N.debug_plan(N.Dims(A, B, D, H, L, C, S), h, None, "STEP")["lat_half"] is half


def _U():
    from tests import gpu_util as U
    return U


def _hyper(name):
    A, B, D, H, L, C, S, s_drop, pruned = SHAPES[name]
    h = R.Hyper(input_dim=D, fc_dim=H, n_categories=C, state_dim=S, lowD_dim=L, x_drop=0.5, s_drop=s_drop, n_arm=A)
    kept = [k for k in range(C) if k not in pruned]
    return h, B, kept, pruned


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def _positions(m, pruned):
    lay = m._layout
    return torch.from_numpy(PR.pruned_flat_positions(int(lay.per_arm), lay.offset, m.n_arm, m.lowD_dim, m.n_categories,
                                                     m.state_dim, pruned))


# ---------------------------------------------------------------------------------------------------
# 1. mmvae_prune_apply writes exactly its set
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A,L,C,S,H,pruned", [
    (2, 5, 7, 2, 16, [1, 4]), (3, 5, 11, 2, 16, [0, 10]), (1, 10, 70, 2, 32, [0, 31, 32, 63, 64, 69]),
    (5, 10, 70, 2, 32, [0, 31, 32, 63, 64, 69]), (2, 10, 92, 2, 100, [2, 30, 33, 91]), (2, 10, 97, 2, 100, [0, 64, 95, 96]),
    (5, 33, 97, 17, 100, list(range(1, 97)))])
def test_prune_apply_writes_exactly_its_set(A, L, C, S, H, pruned):
    from distributed_vae_amd import _native as N
    d = N.Dims(A, 4, 64, H, L, C, S)
    lay = N.param_layout(d)
    n = A * int(lay.per_arm)
    pos = torch.from_numpy(PR.pruned_flat_positions(int(lay.per_arm), lay.offset, A, L, C, S, pruned))
    words = [0, 0, 0, 0]
    for k in range(C):
        if k not in pruned:
            words[k >> 5] |= 1 << (k & 31)
    guard = 64                                              # floats behind the last arm: never written

    def fresh(salt):
        # a non-zero bit pattern, different in every element and buffer (sign bit set in half of them: -0.0 would show)
        v = (torch.arange(n + guard, dtype=torch.int64) * 2654435761 + salt) % (1 << 31)
        v = (v | 1).to(torch.int32) * torch.where(torch.arange(n + guard) % 2 == 0, 1, -1).to(torch.int32)
        return v.to(DEV).view(torch.float32)

    def check(bufs, before, written):
        torch.cuda.synchronize()
        for i, (b, b0) in enumerate(zip(bufs, before)):
            got = _bits(b)
            if i in written:
                assert bool((got[pos] == 0).all()), i                     # +0.0, bit for bit
                rest = torch.ones(n + guard, dtype=torch.bool)
                rest[pos] = False
                assert torch.equal(got[rest], b0[rest]), i                # every other element, gaps and guard included
            else:
                assert torch.equal(got, b0), i

    for given in ([0], [1], [0, 1], [2, 3], [0, 1, 2, 3]):
        bufs = [fresh(7 + i) for i in range(4)]
        before = [_bits(b) for b in bufs]
        assert all(bool((b0 != 0).all()) for b0 in before)
        args = [bufs[i] if i in given else None for i in range(4)]
        N.prune_apply(d, words, *args)
        check(bufs, before, given)
    # bits at or above C have no effect
    hi = list(words)
    for k in range(C, 128):
        hi[k >> 5] |= 1 << (k & 31)
    bufs = [fresh(11 + i) for i in range(4)]
    before = [_bits(b) for b in bufs]
    N.prune_apply(d, hi, *bufs)
    check(bufs, before, [0, 1, 2, 3])
    # the all-zero mask (no mask) and the full mask change nothing
    full = [0, 0, 0, 0]
    for k in range(C):
        full[k >> 5] |= 1 << (k & 31)
    for w in ([0, 0, 0, 0], full):
        bufs = [fresh(13 + i) for i in range(4)]
        before = [_bits(b) for b in bufs]
        N.prune_apply(d, w, *bufs)
        check(bufs, before, [])


# ---------------------------------------------------------------------------------------------------
# 2. the fused masked step against the fp64 masked oracle, three steps
# ---------------------------------------------------------------------------------------------------
def _batches(h, B, seed, n=3):
    xs = [R.synthetic_batch(B, h.input_dim, seed=seed + s) for s in range(n)]
    nz = [R.draw_noise(h, B, seed=seed + 50 + s) for s in range(n)]
    return xs, nz


@pytest.mark.parametrize("engine", FP32_ENGINES)
@pytest.mark.parametrize("name", list(SHAPES))
def test_fused_masked_step_against_the_fp64_masked_oracle(name, engine, monkeypatch):
    import functools
    U = _U()
    from distributed_vae_amd.cpl_mixvae import FusedAdam
    h, B, kept, pruned = _hyper(name)
    A = h.n_arm
    keep64 = PR.keep_masks(h, pruned)
    flip_aware = h.fc_dim == 100
    if flip_aware:
        # gpu_util.flip_aware_oracle evaluates oracle.restatement's forward: for these shapes that is the masked forward
        monkeypatch.setattr(R, "forward", functools.partial(R.forward, mask=kept))
    m = U.build_model(h, R.init_state_dict(h, 77))
    m.train()
    m.gemm_dtype = engine
    opt = FusedAdam(m, lr=1e-3)
    m.prune_apply(kept, opt)                                  # as cpl_mixVAE.prune does in front of the retraining
    pos = _positions(m, pruned)
    xs, nz = _batches(h, B, 300)
    for s in range(3):
        sd_k = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}     # effective: the pruned entries are 0
        m.set_explicit_noise(U.noise_to_device(nz[s]))
        buf = m.fused_train_step(xs[s].to(DEV).expand(A, -1, -1), 1.0, opt, do_adam=True, mask=kept).clone()
        torch.cuda.synchronize()
        grads = {k: gv.detach().cpu().clone() for (k, _), gv in zip(m.named_parameters(), m._grad_views)}
        if flip_aware:
            # the masked fp64 / fp32 oracles on the device's ReLU decisions; gradients of p = the effective weight's times keep
            fo = U.flip_aware_oracle(h, sd_k, xs[s], nz[s], U.device_relu_patterns(m._engine, h), verbose=False)
            for key in ("g_64", "g_32"):
                fo[key] = {k: (g * keep64[k].to(g.dtype) if k in keep64 else g) for k, g in fo[key].items()}
            lt64, g64 = fo["lt_64"], fo["g_64"]
        else:
            sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd_k.items()}
            n64 = {k: [t.double() if t.is_floating_point() else t for t in v] for k, v in nz[s].items()}
            _, lt64, g64, _ = PR.masked_grads(sd64, xs[s].double(), h, n64, kept, keep64)
        errs = {k: G.rel_err(grads[k], g64[k]) for k in g64 if float(g64[k].abs().max()) > 0}
        worst = max(errs, key=errs.get)
        print(f"{name} {engine} step {s}: total {float(buf[0]):.6e} (oracle {float(lt64[0]):.6e}), worst gradient "
              f"{worst} {errs[worst]:.2e}" + (f", ReLU decisions forced: hidden {fo['k_hidden']}, fc11 {fo['k_fc11']}" if flip_aware else ""))
        U.assert_loss_vector(buf.cpu(), lt64, A, LOSS_TOL)
        if flip_aware:
            U.assert_gradients_tight(grads, fo, GRAD_TOL)
        else:
            for k, e in errs.items():
                assert e < GRAD_TOL, (name, engine, s, k, e)
        c = U.ws(m, "c", h.n_categories)
        assert float(c[:, :, pruned].abs().max()) == 0.0                       # c is exactly 0 at pruned categories
        assert float((c.sum(-1) - 1).abs().max()) < 1e-5
        for t in (m._flat, m._flat_grad, opt.exp_avg, opt.exp_avg_sq):         # exact +0.0 after every step
            assert bool((_bits(t)[pos] == 0).all()), (name, s)
        assert opt.step_count == s + 1


# ---------------------------------------------------------------------------------------------------
# 3. fused == forward(mask=) + loss + backward() + torch.optim.Adam with prune_apply around the optimizer
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", FP32_ENGINES)
@pytest.mark.parametrize("name", list(SHAPES))
def test_fused_masked_step_equals_the_three_call_path(name, engine):
    U = _U()
    from distributed_vae_amd.cpl_mixvae import FusedAdam
    h, B, kept, pruned = _hyper(name)
    A = h.n_arm
    sd = R.init_state_dict(h, 78)
    xs, nz = _batches(h, B, 400)
    m1 = U.build_model(h, sd); m1.train(); m1.gemm_dtype = engine
    opt = FusedAdam(m1, lr=1e-3)
    m1.prune_apply(kept, opt)
    m2 = U.build_model(h, sd); m2.train(); m2.gemm_dtype = engine
    topt = torch.optim.Adam(m2.parameters(), lr=1e-3)
    m2.prune_apply(kept)
    for s in range(3):
        xd = xs[s].to(DEV).expand(A, -1, -1)
        m1.set_explicit_noise(U.noise_to_device(nz[s]))
        b1 = m1.fused_train_step(xd, 1.0, opt, do_adam=True, mask=kept).clone()
        m2.set_explicit_noise(U.noise_to_device(nz[s]))
        topt.zero_grad()
        out = m2(xd, 1.0, 0.0, mask=kept)
        lt = m2.loss(out[0], [], [], xd, out[7], out[8], out[4], out[6], 0.0)
        lt[0].backward()
        m2.bind_grads()                                       # .grad = the views of the flat buffer backward() filled
        m2.prune_apply(kept, params=False)                    # grads before the optimizer's step ...
        topt.step()
        m2.prune_apply(kept, grads=False)                     # ... parameters after it
        torch.cuda.synchronize()
        if s == 0:
            # the same parameters on both sides: the gates of test_fused_step_matches_api_path_fc100 (loss 1e-6, gradients
            # 1e-5 -- the first moment after one step is 0.1 x the gradient).  The moments may differ at pruned entries
            # only; here both hold 0 there (torch's Adam saw the zeroed gradient)
            assert abs(float(b1[0]) - float(lt[0])) <= 1e-6 * abs(float(lt[0])) + 1e-7
            mom1 = dict(zip([k for k, _ in m1.named_parameters()], opt._views(opt.exp_avg)))
            for k, p in m2.named_parameters():
                assert G.rel_err(mom1[k].cpu(), topt.state[p]["exp_avg"].cpu()) < 1e-5, k
    pos = _positions(m1, pruned)
    keep = PR.keep_masks(h, pruned, dtype=torch.float32)
    for t in (m1._flat, m2._flat, opt.exp_avg, opt.exp_avg_sq):
        assert bool((_bits(t)[pos] == 0).all())
    p2 = dict(m2.named_parameters())
    for k, p in m1.named_parameters():
        # effective parameters after three steps: the bound of test_golden_adam_trajectory
        diff = (p.detach() - p2[k].detach()).abs().cpu()
        assert float(diff.max()) < 3.1e-3 and float(diff.median()) < 2e-5, (k, float(diff.max()), float(diff.median()))
        if k in keep:                                         # torch's moments at pruned entries: 0 here as well
            assert float((topt.state[p2[k]]["exp_avg"].cpu() * (1 - keep[k])).abs().max()) == 0.0, k
    # the moments after three steps, at the kept entries (the pruned ones are exactly 0 on both sides, above): each path's
    # gradients are held to GRAD_TOL of the tensor's scale against the oracle, so two paths differ by at most 2 GRAD_TOL in
    # the first moment (a fixed linear combination of the gradients) and twice that in the second (their squares)
    mom = {k: (a, b) for (k, _), a, b in zip(m1.named_parameters(), opt._views(opt.exp_avg), opt._views(opt.exp_avg_sq))}
    worst = [0.0, 0.0]
    for k, p in m2.named_parameters():
        w = keep.get(k, torch.ones(()))
        st = topt.state[p]
        e1 = G.rel_err(mom[k][0].cpu() * w, st["exp_avg"].cpu() * w)
        e2 = G.rel_err(mom[k][1].cpu() * w, st["exp_avg_sq"].cpu() * w)
        worst = [max(worst[0], e1), max(worst[1], e2)]
        assert e1 < 2 * GRAD_TOL and e2 < 4 * GRAD_TOL, (k, e1, e2)
    print(f"{name} {engine}: moments after three steps, fused against three-call: exp_avg {worst[0]:.2e}, exp_avg_sq {worst[1]:.2e}")


# ---------------------------------------------------------------------------------------------------
# 4. the rows path: bit-identical to gather + masked step
# ---------------------------------------------------------------------------------------------------
def test_masked_row_indexed_step_is_bit_identical_to_gather_then_masked_step():
    U = _U()
    from distributed_vae_amd.cpl_mixvae import FusedAdam
    A, B, D, H, n_rows, seed = 2, 300, 520, 100, 1000, 41
    h = R.Hyper(input_dim=D, fc_dim=H, n_categories=12, state_dim=2, lowD_dim=6, n_arm=A)
    pruned = [0, 5, 11]
    kept = [k for k in range(12) if k not in pruned]
    sd = R.init_state_dict(h, seed)
    data = R.synthetic_batch(n_rows, D, seed=seed + 1).to(DEV)
    rows = torch.randint(0, n_rows, (B,), generator=torch.Generator().manual_seed(seed + 2))
    rows[:3] = torch.tensor([n_rows - 1, 0, n_rows - 1])
    res = []
    for indexed in (False, True):
        m = U.build_model(h, sd)
        m.train()
        m.gemm_dtype = "fp32x3"                               # the engine that offers the row map
        opt = FusedAdam(m, lr=1e-3)
        m.prune_apply(kept, opt)
        bufs = []
        for s in range(2):
            m.set_explicit_noise(U.noise_to_device(R.draw_noise(h, B, seed=seed + 10 + s)))
            r = torch.roll(rows, s).to(DEV)
            if indexed:
                bufs.append(m.fused_train_step_rows(data, r, 1.0, opt, do_adam=True, mask=kept).clone())
            else:
                bufs.append(m.fused_train_step(data[r].contiguous().expand(A, -1, -1), 1.0, opt, do_adam=True, mask=kept).clone())
        torch.cuda.synchronize()
        pos = _positions(m, pruned)
        for t in (m._flat, m._flat_grad, opt.exp_avg, opt.exp_avg_sq):
            assert bool((_bits(t)[pos] == 0).all())
        res.append((torch.stack(bufs), m._flat, m._flat_grad, m._bn_flat, opt.exp_avg, opt.exp_avg_sq))
    for u, v in zip(*res):
        assert torch.equal(_bits(u), _bits(v))
    assert bool(torch.isfinite(res[0][0]).all())


# ---------------------------------------------------------------------------------------------------
# 5. the loop
# ---------------------------------------------------------------------------------------------------
LOOP = dict(A=2, D=64, H=16, L=5, C=7, S=2, N=256, B=64)


def _loop_data():
    x = R.synthetic_batch(LOOP["N"], LOOP["D"], seed=546)                 # SURVEY.md section 8d's recipe
    x_te = R.synthetic_batch(64, LOOP["D"], seed=547)
    return x, x_te


def _loop_loaders(x, x_te):
    from torch.utils.data import DataLoader, TensorDataset
    ds = TensorDataset(x, torch.arange(len(x), dtype=torch.float32))
    tr = DataLoader(ds, batch_size=LOOP["B"], shuffle=False, drop_last=True)
    te = DataLoader(TensorDataset(x_te, torch.arange(len(x_te), dtype=torch.float32)), batch_size=1, shuffle=False)
    al = DataLoader(ds, batch_size=LOOP["B"], shuffle=False)
    return tr, te, al


def _loop_trainer(folder="", trained_model="", n_pr=0):
    import distributed_vae_amd  # noqa: F401
    from distributed_vae_amd.cpl_mixvae import cpl_mixVAE
    torch.manual_seed(5)
    t = cpl_mixVAE(saving_folder=folder, device=0, save_flag=bool(folder))
    t.init_model(n_categories=LOOP["C"], state_dim=LOOP["S"], input_dim=LOOP["D"], fc_dim=LOOP["H"], lowD_dim=LOOP["L"],
                 x_drop=0.5, s_drop=0.0, lr=1e-3, n_arm=LOOP["A"], temp=1.0, tau=0.005, trained_model=trained_model, n_pr=n_pr)
    return t


def _labels_before(t, x):
    """model.encode labels of the whole training set, taken in the trainer's evaluation chunks."""
    t.model.eval()
    lab = [t.model.encode(x[i:i + LOOP["B"]].to(DEV).expand(LOOP["A"], -1, -1), t.temp)["labels"].cpu()
           for i in range(0, len(x), LOOP["B"])]
    t.model.train()
    return torch.cat(lab, dim=1).numpy()


def _pruned_zero(sd, h, pruned):
    keep = PR.keep_masks(h, pruned, dtype=torch.float32)
    for k, w in keep.items():
        assert float((sd[k].cpu().float() * (1 - w)).abs().max()) == 0.0, k
        assert bool((sd[k].cpu()[w.bool()] != 0).any()), k          # ... and only there


@pytest.fixture(scope="module")
def always(tmp_path_factory):
    folder = str(tmp_path_factory.mktemp("prune"))
    x, x_te = _loop_data()
    tr, te, al = _loop_loaders(x, x_te)
    t = _loop_trainer(folder)
    labels = _labels_before(t, x)
    p0 = _bits(t.model.flat_parameters()).clone()
    hist = t.prune(tr, te, n_epoch_p=1, min_con=1.1, max_prun_it=2)
    return dict(t=t, hist=hist, labels=labels, p0=p0, folder=folder, loaders=(tr, te, al))


def _h_loop():
    return R.Hyper(input_dim=LOOP["D"], fc_dim=LOOP["H"], n_categories=LOOP["C"], state_dim=LOOP["S"], lowD_dim=LOOP["L"],
                   n_arm=LOOP["A"])


def test_loop_always_prune_two_rounds(always):
    t, hist = always["t"], always["hist"]
    assert hist["rounds"] == 2 and len(hist["pruned"]) == 2 and len(set(hist["pruned"])) == 2
    assert len(hist["agreement"]) == 3                        # two pruning assessments and the one that stops at max_prun_it
    want = PR.agreement(always["labels"], LOOP["C"])
    got = hist["agreement"][0]
    assert got.dtype == np.float64 and got.shape == (LOOP["C"],)
    assert np.array_equal(got.view(np.int64), want.view(np.int64)), (got, want)      # bit for bit
    assert hist["pruned"][0] == int(np.argmin(want))
    # the second round never looks at the pruned category
    assert hist["pruned"][1] == PR.decision(hist["agreement"][1], [k for k in range(LOOP["C"]) if k != hist["pruned"][0]],
                                            1.1, 1, 2)
    assert hist["kept"] == [k for k in range(LOOP["C"]) if k not in hist["pruned"]]
    assert len(hist["losses"]) == 2 and np.isfinite(hist["losses"]).all() and np.isfinite(hist["validation_loss"]).all()
    assert t.n_pr == 2 and t._prune_mask is None
    assert not torch.equal(_bits(t.model.flat_parameters()), always["p0"])
    for a in range(LOOP["A"]):
        b = t.model.fcc[a].bias.detach().cpu()
        assert float(b[hist["pruned"]].abs().max()) == 0.0 and bool((b[hist["kept"]] != 0).all())
    _pruned_zero(t.model.state_dict(), _h_loop(), hist["pruned"])
    ev = t.eval_model(always["loaders"][2])
    assert ev["prune_indx"].tolist() == sorted(hist["pruned"])
    assert float(np.abs(ev["z_prob"][:, :, hist["pruned"]]).max()) == 0.0


def test_loop_checkpoints_load_and_hold_zeros(always):
    hist, folder = always["hist"], always["folder"]
    files = sorted(f for f in os.listdir(os.path.join(folder, "model")) if "after_pruning" in f)
    assert [f.split("_after_pruning_")[1].split("_")[0] for f in files] == ["1", "2"], files
    for i, f in enumerate(files):
        assert f.startswith("cpl_mixVAE_model_after_pruning_") and f.endswith(".pth")
        ck = torch.load(os.path.join(folder, "model", f), map_location="cpu", weights_only=True)
        assert set(ck) == {"model_state_dict", "optimizer_state_dict"}
        _pruned_zero(ck["model_state_dict"], _h_loop(), hist["pruned"][:i + 1])
        if i == 0:                                            # the second category was still alive after round 1
            assert float(ck["model_state_dict"]["fcc.0.bias"][hist["pruned"][1]]) != 0.0


@pytest.mark.parametrize("kw", [dict(min_con=-1.0, max_prun_it=2), dict(min_con=1.1, max_prun_it=0)])
def test_loop_runs_no_round_and_leaves_the_parameters(kw):
    x, x_te = _loop_data()
    tr, te, _ = _loop_loaders(x, x_te)
    t = _loop_trainer()
    p0 = _bits(t.model.flat_parameters()).clone()
    bn0 = {k: v.detach().cpu().clone() for k, v in t.model.state_dict().items() if "batch_" in k}
    hist = t.prune(tr, te, n_epoch_p=1, **kw)
    torch.cuda.synchronize()
    assert hist["rounds"] == 0 and hist["pruned"] == [] and len(hist["agreement"]) == 1 and hist["losses"] == []
    assert torch.equal(_bits(t.model.flat_parameters()), p0)
    for k, v in bn0.items():
        assert torch.equal(t.model.state_dict()[k].cpu(), v), k
    assert t.n_pr == 0


def test_loop_resumes_from_a_pruned_checkpoint(always):
    hist0, folder = always["hist"], always["folder"]
    ck = [f for f in os.listdir(os.path.join(folder, "model")) if "after_pruning_2_" in f]
    assert len(ck) == 1
    x, x_te = _loop_data()
    tr, te, al = _loop_loaders(x, x_te)
    t = _loop_trainer(trained_model=os.path.join(folder, "model", ck[0]), n_pr=2)
    assert t.n_pr == 2
    hist = t.prune(tr, te, n_epoch_p=1, min_con=1.1, max_prun_it=3)
    assert hist["rounds"] == 1 and len(hist["agreement"]) == 2 and t.n_pr == 3
    assert hist["pruned"][:2] == sorted(hist0["pruned"]) and len(hist["pruned"]) == 3
    assert hist["pruned"][2] not in hist0["pruned"]
    for agr in hist["agreement"]:                              # a pruned category is never predicted under the mask
        assert all(agr[k] == 0.0 for k in hist0["pruned"])
    assert t.eval_model(al)["prune_indx"].tolist() == sorted(hist["pruned"])


def test_loop_with_a_stock_torch_optimizer():
    """``_step`` with ``torch.optim.Adam``: the fused step without its own Adam zeroes the pruned gradients, the optimizer
    steps, ``prune_apply`` zeroes the pruned parameters behind it."""
    x, x_te = _loop_data()
    tr, te, _ = _loop_loaders(x, x_te)
    t = _loop_trainer()
    t.optimizer = torch.optim.Adam(t.model.parameters(), lr=1e-3)
    p0 = _bits(t.model.flat_parameters()).clone()
    hist = t.prune(tr, te, n_epoch_p=1, min_con=1.1, max_prun_it=1)
    torch.cuda.synchronize()
    assert hist["rounds"] == 1 and len(hist["pruned"]) == 1 and np.isfinite(hist["losses"]).all()
    pos = _positions(t.model, hist["pruned"])
    for buf in (t.model._flat, t.model._flat_grad):
        assert bool((_bits(buf)[pos] == 0).all())
    _pruned_zero(t.model.state_dict(), _h_loop(), hist["pruned"])
    rest = torch.ones(p0.numel(), dtype=torch.bool)
    rest[pos] = False
    assert bool((_bits(t.model._flat)[rest] != p0[rest]).any())            # the optimizer did step
    for p in t.model.parameters():                                          # its moments never saw a pruned gradient
        assert "exp_avg" in t.optimizer.state[p]
    keep = PR.keep_masks(_h_loop(), hist["pruned"], dtype=torch.float32)
    for k, p in t.model.named_parameters():
        if k in keep:
            assert float((t.optimizer.state[p]["exp_avg"].cpu() * (1 - keep[k])).abs().max()) == 0.0, k


def test_prune_refuses_data_parallel_runs(monkeypatch):
    from distributed_vae_amd import dist as D
    t = _loop_trainer()
    monkeypatch.setattr(D, "is_dist", lambda: True)
    with pytest.raises(NotImplementedError, match="pruning phase"):
        t.prune(None, None, 1, min_con=1.1, max_prun_it=1)

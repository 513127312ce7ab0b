"""Build container only: run the REAL reference (oracle/ref_loader) on the cases that tests/test_oracle_vs_reference.py,
tests/test_consensus_cpu.py and tests/test_augmenter_cpu.py check the oracle against, and commit what the reference
computed as data-only fixtures, one per group of tests (FILES below, under tests/golden/, in the format of
oracle/packed.py: what a test compares within a tolerance is stored, what it requires to be exactly equal is stored as a
digest).  The tests rebuild the inputs
from the same seeds and compare the oracle with these outputs, so they need no reference at run time.

    python -m oracle.gen_golden_ref
"""
import os
import re
import warnings

import numpy as np
import torch

from oracle import augmenter as OA
from oracle import packed as PK
from oracle import ref_loader as RL
from oracle import restatement as R

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
# fixture file -> the entries it holds (by name prefix)
FILES = {
    "ref_restatement.npz": ("rs/", "snap/", "ckpt/"),       # tests/test_oracle_vs_reference.py
    "ref_masked.npz": ("mask/",),                           # tests/test_oracle_vs_reference.py (masked forward)
    "ref_consensus.npz": ("cons/",),                        # tests/test_consensus_cpu.py
    "ref_augmenter.npz": ("aug/", "mirror/"),               # tests/test_augmenter_cpu.py
}

# A, B, D, H, L, C, S, hard, s_drop (tests/test_oracle_vs_reference.py)
CASES = [
    (2, 24, 40, 12, 4, 6, 2, False, 0.0),
    (3, 33, 50, 10, 3, 8, 2, False, 0.3),
    (4, 20, 36, 8, 4, 5, 1, True, 0.0),
]
MASK_CASE = (3, 33, 50, 10, 3, 8, 2, False, 0.0)
MASK = [1, 2, 4, 7]
CKPT_CASE = (3, 8, 40, 12, 4, 6, 2, False, 0.0)
OUT_IDX = (0, 3, 4, 5, 6, 7, 8, 9)
DTYPES = {"f64": torch.float64, "f32": torch.float32}
# (K, n) of the consensus cases, drawn from np.random.default_rng(3) in this order (tests/test_consensus_cpu.py)
CONSENSUS = [(4, 50), (92, 5000), (92, 300), (128, 20000), (7, 1)]
# NZ, Z, D, ND, A, B (tests/test_augmenter_cpu.py)
AUG_CASES = [(5, 2, 40, 20, 2, 9), (16, 10, 100, 60, 4, 33)]


def _mk(ref, cfg):
    A, B, D, H, L, C, S, hard, sdrop = cfg
    torch.manual_seed(99)
    m = ref.mixVAE_model(input_dim=D, fc_dim=H, n_categories=C, state_dim=S, lowD_dim=L, x_drop=0.5,
                         s_drop=sdrop, n_arm=A, lam=1, lam_pc=1, tau=0.005, beta=1.0, hard=hard,
                         variational=True, device="cpu", eps=1e-8, momentum=0.01, ref_prior=False,
                         loss_mode="MSE")
    h = R.Hyper(input_dim=D, fc_dim=H, n_categories=C, state_dim=S, lowD_dim=L, x_drop=0.5,
                s_drop=sdrop, n_arm=A, hard=hard)
    return m, h


def _np(t):
    return t.detach().cpu().numpy().copy()


def _put_out(g, pre, out, A):
    for i in OUT_IDX:
        for a in range(A):
            g[f"{pre}/{i}/{a}"] = _np(out[i][a])


def restatement_cases(ref, g):
    for c, cfg in enumerate(CASES):
        for tag, dtype in DTYPES.items():
            old = torch.get_default_dtype()
            torch.set_default_dtype(dtype)
            try:
                m, h = _mk(ref, cfg)
                A, B, D = cfg[:3]
                pre = f"rs/{c}/{tag}"
                for k, v in m.state_dict().items():
                    g[f"{pre}/init/{k}"] = _np(v)
                x = R.synthetic_batch(B, D, seed=5, dtype=dtype)
                noise = R.draw_noise(h, B, seed=11)
                m.train()
                out, lo, _ = RL.reference_step(m, x.expand(A, -1, -1), 1.0, noise)
                lo[0].backward()
                g[f"{pre}/loss"] = np.array(float(lo[0]))
                _put_out(g, f"{pre}/out", out, A)
                for k, p in m.named_parameters():
                    g[f"{pre}/grad/{k}"] = _np(p.grad)
                for k, v in m.state_dict().items():
                    if "running" in k:
                        g[f"{pre}/state/{k}"] = _np(v)
            finally:
                torch.set_default_dtype(old)


def snapshot_losses(g):
    """The current reference file and the packaged older snapshot on CASES[0], fp32."""
    res = []
    for mod in (RL.load_reference_nn_model(), RL.load_reference_nn_model_old()):
        m, h = _mk(mod, CASES[0])
        A, B, D = CASES[0][:3]
        x = R.synthetic_batch(B, D, seed=5)
        m.train()
        out, lo, _ = RL.reference_step(m, x.expand(A, -1, -1), 1.0, R.draw_noise(h, B, seed=11))
        res.append(float(lo[0]))
    g["snap/loss_current"] = np.array(res[0], dtype=np.float32)
    g["snap/loss_old"] = np.array(res[1], dtype=np.float32)


def checkpoint_layout(ref, g):
    """The reference model's state_dict (keys in order, initial values for torch seed 99) and its parameter order: what
    a strict load_state_dict and torch.optim.Adam's load_state_dict check a checkpoint against."""
    m, _ = _mk(ref, CKPT_CASE)
    g["ckpt/layout"] = [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in m.state_dict().items()]
    g["ckpt/param_keys"] = [k for k, _ in m.named_parameters()]


def masked_cases(ref, g):
    for tag, dtype in DTYPES.items():
        old = torch.get_default_dtype()
        torch.set_default_dtype(dtype)
        try:
            m, h = _mk(ref, MASK_CASE)
            A, B, D = MASK_CASE[:3]
            pre = f"mask/{tag}"
            x = R.synthetic_batch(B, D, seed=5, dtype=dtype)
            xs = x.expand(A, -1, -1)
            noise = R.draw_noise(h, B, seed=11)
            m.train()
            with RL.explicit_noise(m, noise):
                out = m(xs, 1.0, 0.0, eval=False, mask=MASK)
            lo = m.loss(out[0], [], [], xs, out[7], out[8], out[4], out[6], 0.0)
            lo[0].backward()
            g[f"{pre}/loss"] = np.array(float(lo[0]))
            _put_out(g, f"{pre}/out", out, A)
            for k, p in m.named_parameters():
                g[f"{pre}/grad/{k}"] = _np(p.grad)
            m.eval()
            ne = R.draw_noise(h, B, seed=12, training=False, eval_flag=True)
            with torch.no_grad(), RL.explicit_noise(m, ne):
                oe = m(xs, 1.0, 0.0, eval=True, mask=MASK)
            _put_out(g, f"{pre}/eout", oe, A)
        finally:
            torch.set_default_dtype(old)


def consensus_cases(g):
    ref = RL.load_reference_consensus_utils()
    rng = np.random.default_rng(3)
    for K, n in CONSENSUS:
        l1 = rng.integers(0, K, n).astype(np.int64)
        l2 = np.where(rng.random(n) < 0.7, l1, rng.integers(0, K, n)).astype(np.int64)
        cm = ref.compute_confmat(l1, l2, K)
        pre = f"cons/{K}_{n}"
        g[f"{pre}/cm"] = cm
        g[f"{pre}/cm_naive"] = ref.compute_confmat_naive(l1, l2, K)
        g[f"{pre}/norm"] = ref.confmat_normalize(cm)
        g[f"{pre}/mean"] = np.array(ref.confmat_mean(ref.confmat_normalize(cm)), dtype=np.float64)
    p = rng.random((40, 9))
    g["cons/classify"] = np.asarray(ref.classify(p))


def augmenter_cases(g):
    cls = RL.load_reference_augmenter()
    for c, cfg in enumerate(AUG_CASES):
        NZ, Z, D, ND, A, B = cfg
        for tag, dtype in DTYPES.items():
            old = torch.get_default_dtype()
            torch.set_default_dtype(dtype)
            try:
                sd = OA.random_state_dict(NZ, Z, D, ND, seed=3, dtype=dtype)
                m = cls(noise_dim=NZ, latent_dim=Z, input_dim=D, n_dim=ND)
                m.load_state_dict(sd)
                m.eval()
                torch.manual_seed(2)
                x = torch.randn(B, D, dtype=dtype).abs()
                torch.manual_seed(1)
                with torch.no_grad():
                    s_ref, x_ref = m(x.expand(A, -1, -1), True, 0.1)
                pre = f"aug/{c}/{tag}"
                g[f"{pre}/x"] = _np(x)
                g[f"{pre}/s"] = _np(s_ref)
                g[f"{pre}/x_aug"] = _np(x_ref)
            finally:
                torch.set_default_dtype(old)
    # the reference constructor's initial parameters for torch seed 11 (the mirror class must draw the same)
    torch.manual_seed(11)
    r = cls(noise_dim=6, latent_dim=3, input_dim=52, n_dim=20)
    for k, v in r.state_dict().items():
        g[f"mirror/sd/{k}"] = _np(v)


# entries the tests require to be exactly equal (torch.equal / np.array_equal): kept as digests; the inputs x of the
# augmenter cases are drawn from a seeded generator by the tests and checked against theirs
EXACT = re.compile(r"^(rs/\d+/f\d\d/init/|mirror/sd/|cons/.*/(cm|cm_naive|norm)$|cons/classify$|aug/\d+/f\d\d/x$)")


def main():
    warnings.simplefilter("ignore")
    ref = RL.load_reference_nn_model()
    g = {}
    restatement_cases(ref, g)
    snapshot_losses(g)
    checkpoint_layout(ref, g)
    masked_cases(ref, g)
    consensus_cases(g)
    augmenter_cases(g)
    meta = {"generator": "oracle/gen_golden_ref.py", "cases": CASES, "mask_case": MASK_CASE, "mask": MASK,
            "ckpt_case": CKPT_CASE, "consensus": CONSENSUS, "augmenter": AUG_CASES}
    assert all(k.startswith(sum(FILES.values(), ())) for k in g)
    for name, prefixes in FILES.items():
        part = {k: v for k, v in g.items() if k.startswith(prefixes)}
        lists = {k: v for k, v in part.items() if isinstance(v, list)}
        exact = {k: v for k, v in part.items() if k not in lists and EXACT.match(k)}
        values = {k: v for k, v in part.items() if k not in lists and k not in exact}
        out = os.path.join(GOLDEN, name)
        PK.save(out, values, exact, lists, meta)
        print(out, os.path.getsize(out), "bytes:", len(values), "arrays,", len(exact), "digests,", len(lists), "lists")


if __name__ == "__main__":
    main()

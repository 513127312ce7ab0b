"""CPU (no GPU): the pruning phase's host side -- the decision function of ``cpl_mixVAE.prune`` against the numpy restatement
(tests/prune_restatement.py) on hand-made agreement vectors, the argument errors of mmvae_prune_apply (all returned before
any launch), and the element set of the five pruning masks restated from mmvae_param_layout (what tests/test_gpu_prune.py
compares the kernel's writes against)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import distributed_vae_amd  # noqa: F401
from distributed_vae_amd import _native as N
from distributed_vae_amd.cpl_mixvae import cpl_mixVAE, prune_decision, prune_start
from oracle import restatement as R
from tests import prune_restatement as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR = 0x1000        # fake device pointers: every case must be refused on the host, before anything dereferences them


# --------------------------------------------------------------------------- decision
def _both(agreement, kept, min_con, pr, max_prun_it):
    got = prune_decision(np.asarray(agreement, dtype=np.float64), np.asarray(kept), min_con, pr, max_prun_it)
    want = PR.decision(np.asarray(agreement, dtype=np.float64), np.asarray(kept), min_con, pr, max_prun_it)
    assert got == want, (got, want)
    return got


def test_decision_ties_go_to_the_first_index():
    assert _both([0.9, 0.2, 0.5, 0.2, 0.2], [0, 1, 2, 3, 4], 0.5, 0, 5) == 1
    assert _both([0.9, 0.2, 0.5, 0.2, 0.2], [0, 2, 3, 4], 0.5, 0, 5) == 3        # category 1 already gone
    assert _both([0.3, 0.3, 0.3], [0, 1, 2], 0.3, 0, 1) == 0                      # the comparison is <=


def test_decision_never_predicted_categories_have_agreement_zero():
    # 8 cells, C = 5: categories 3 and 4 are predicted by no arm -> their normalised diagonal is 0 -> 3 goes first
    labels = np.array([[0, 0, 1, 1, 2, 2, 2, 0], [0, 0, 1, 2, 2, 2, 2, 0]])
    agr = PR.agreement(labels, 5)
    assert agr.dtype == np.float64 and agr.shape == (5,)
    assert agr[3] == 0.0 and agr[4] == 0.0 and np.all(agr[:3] > 0)
    np.testing.assert_array_equal(agr[:3], [1.0, 0.5, 0.75])      # 3/3, 1/max(2,1), 3/max(3,4)
    assert _both(agr, [0, 1, 2, 3, 4], 0.1, 0, 9) == 3
    assert _both(agr, [0, 1, 2, 4], 0.1, 1, 9) == 4
    assert _both(agr, [0, 1, 2], 0.1, 2, 9) is None               # 0.5 > min_con


def test_decision_stops_at_max_prun_it():
    agr = [0.1, 0.2, 0.3]
    assert _both(agr, [0, 1, 2], 0.5, 1, 2) == 0
    assert _both(agr, [0, 1, 2], 0.5, 2, 2) is None               # pr == max_prun_it
    assert _both(agr, [0, 1, 2], 0.5, 0, 0) is None               # the default: no round at all
    assert _both(agr, [0, 1, 2], 0.5, 3, 2) is None


def test_decision_stops_when_the_minimum_is_above_min_con():
    assert _both([0.8, 0.6, 0.7], [0, 1, 2], 0.5, 0, 9) is None
    assert _both([0.8, 0.6, 0.7], [0, 1, 2], 0.6, 0, 9) == 1
    assert _both([0.0, 0.6, 0.7], [1, 2], 0.5, 0, 9) is None      # the pruned category's 0 does not count
    assert _both([0.8, 0.6, 0.7], [0, 1, 2], -1.0, 0, 9) is None
    assert _both([1.0, 1.0], [0, 1], 1.1, 0, 9) == 0              # min_con above 1: always prune
    assert _both([1.0, 0.0], [0], 1.1, 0, 9) is None              # the last category stays


def test_start_from_a_bias_vector_that_already_has_zeros():
    bias = np.array([0.3, 0.0, -0.2, 0.0, 1e-30], dtype=np.float32)
    kept, pruned = prune_start(bias)
    k2, p2 = PR.start(bias)
    np.testing.assert_array_equal(kept, k2)
    np.testing.assert_array_equal(pruned, p2)
    assert kept.tolist() == [0, 2, 4] and pruned.tolist() == [1, 3]
    assert _both([0.5, 0.0, 0.4, 0.0, 0.9], kept, 0.5, 2, 3) == 2  # resumes at round 2 and never re-selects 1 or 3
    kept, pruned = prune_start(np.ones(4, dtype=np.float32))
    assert kept.tolist() == [0, 1, 2, 3] and pruned.size == 0


def test_prune_without_epochs_returns_at_once():
    t = cpl_mixVAE(saving_folder="", device="cpu")
    t.n_arm, t.input_dim = 2, 8                                    # no model: n_epoch_p <= 0 must not touch one
    for n in (0, -1):
        hist = t.prune(None, None, n, min_con=1.1, max_prun_it=5)
        assert hist["pruned"] == [] and hist["agreement"] == [] and hist["rounds"] == 0


# --------------------------------------------------------------------------- mmvae_prune_apply: host contract
def test_entry_point_declared_exported_and_abi_unchanged():
    hdr = open(os.path.join(ROOT, "include", "mmvae.h")).read()
    assert re.search(r"\bmmvae_prune_apply\(", hdr)
    assert hasattr(N.lib(), "mmvae_prune_apply")
    assert N.lib().mmvae_abi_version() == N.ABI_VERSION == 5
    assert "mmvae_prune_apply" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def _call(d, words, params=PTR, grads=PTR, m=PTR, v=PTR):
    w = (C.c_uint32 * 4)(*words) if words is not None else None
    return N.lib().mmvae_prune_apply(C.byref(d) if d is not None else None, C.byref(w) if w is not None else None,
                                     params, grads, m, v, None)


def test_prune_apply_argument_errors_return_before_any_launch():
    d = N.Dims(2, 4, 16, 8, 3, 7, 2)
    some = [0b1011111, 0, 0, 0]                                    # category 5 pruned
    assert _call(None, some) == -1 and b"dims" in N.lib().mmvae_last_error_string()
    assert _call(d, some, None, None, None, None) == -1 and b"buffer" in N.lib().mmvae_last_error_string()
    assert _call(d, None) == -1
    # a mask that keeps nothing: bits set only at or above C = 7 count as keeping nothing
    for words in ([1 << 7, 0, 0, 0], [0xFFFFFF80, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF], [0, 1, 0, 0], [0, 0, 0, 1 << 31]):
        assert _call(d, words) == -1, words
        assert b"keeps none" in N.lib().mmvae_last_error_string()
    assert _call(N.Dims(2, 4, 16, 8, 3, 0, 2), some) == -1         # dims check_dims refuses as such
    assert _call(N.Dims(2, 4, 16, 8, 3, 129, 2), some) == -2
    # all words zero: nothing is pruned, 0 without a launch (the fake pointers are never touched; no device is needed)
    assert _call(d, [0, 0, 0, 0]) == 0
    assert _call(d, [0, 0, 0, 0], None, None, None, None) == -1    # ... but the buffers are still checked first
    with pytest.raises(N.NativeError):
        N.prune_apply(d, [1 << 7, 0, 0, 0], torch.zeros(1))        # (CPU tensor: refused by the binding)


# --------------------------------------------------------------------------- the element set
@pytest.mark.parametrize("A,L,Cc,S,H,pruned", [
    (2, 5, 7, 2, 16, [1, 4]), (3, 5, 11, 2, 16, [0, 10]), (1, 10, 70, 2, 100, [0, 31, 32, 63, 64, 69]),
    (5, 33, 97, 17, 100, [96]), (8, 64, 128, 32, 128, list(range(1, 128)))])
def test_element_set_restated_from_the_layout(A, L, Cc, S, H, pruned):
    """tests/prune_restatement.py::pruned_flat_positions against the state-dict views of the same layout: marking the
    five tensors' pruned rows / columns through (offset, rows, cols) gives exactly that index set."""
    d = N.Dims(A, 4, 64, H, L, Cc, S)
    lay = N.param_layout(d)
    per_arm = int(lay.per_arm)
    pos = PR.pruned_flat_positions(per_arm, lay.offset, A, L, Cc, S, pruned)
    assert len(pos) == A * len(pruned) * (2 * L + 1 + 2 * S)
    h = R.Hyper(input_dim=64, fc_dim=H, n_categories=Cc, state_dim=S, lowD_dim=L, n_arm=A)
    keep = PR.keep_masks(h, pruned)
    flat = np.zeros(A * per_arm, dtype=bool)
    for a in range(A):
        for t, nm in enumerate(N.PARAM_NAMES):
            layer, kind = nm.split(".")
            key = f"{layer}.{a}.{kind}"
            if key not in keep:
                continue
            n = int(lay.rows[t]) * int(lay.cols[t])
            assert tuple(keep[key].shape) in ((int(lay.rows[t]), int(lay.cols[t])), (int(lay.rows[t]),))
            o = a * per_arm + int(lay.offset[t])
            flat[o: o + n] = (keep[key].reshape(-1) == 0).numpy()
    np.testing.assert_array_equal(np.flatnonzero(flat), pos)
    # nothing outside an arm's tensors (alignment gaps) and nothing in another tensor
    ends = sorted((int(lay.offset[t]), int(lay.offset[t]) + int(lay.rows[t]) * int(lay.cols[t])) for t in range(N.N_PARAM_TENSORS))
    within = pos % per_arm
    assert all(any(lo <= p < hi for lo, hi in ends) for p in within.tolist())

"""GPU: ``summarize_inference`` and ``evaluate``.  On a stub trainer that returns the ``eval_model`` dictionaries of
tests/golden/summary_a3.npz the summary equals what the reference's own summarize_inference recorded, key for key and bit
for bit: the counts are integers, the consensus is one fp64 division per entry of the same operands, ``con_mean`` a ratio of
integers.  End to end on a real ``cpl_mixVAE`` with two checkpoints at the evals fixture's shape (A = 3, D = 64, H = 16,
L = 4, C = 7, N = 150 in batches of 64) the summary equals the restatement (tests/mutinfo_restatement.py::summarize) applied
to the dictionaries ``eval_model`` returned during the call -- recorded through a wrapper, so that the keys that depend on
the state noise are compared on the very draw the summary saw.

The end-to-end ``evaluate`` check compares the device's average MI with the restatement's on tables of N = 150 cells that no
fixture records.  Its bound is borrowed, not measured for these tables: the device's gate against sklearn (16 e_ref) plus the
restatement's (8 e_ref), with e_ref the largest recorded for the cases of N <= 300."""
import os
import pickle
import sys

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader, TensorDataset

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mutinfo_restatement as MR  # noqa: E402
from gpu_util import DEV  # noqa: E402
from distributed_vae_amd.eval_models import summarize_inference  # noqa: E402
from distributed_vae_amd.evaluation import evaluate  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
S = np.load(os.path.join(GOLDEN, "summary_a3.npz"))
G = np.load(os.path.join(GOLDEN, "evals2_a3.npz"))
A, NC, D, H, L, K_, S_DIM, BATCH, PRUNED = [int(v) for v in G["cfg"]]
ALSO_PRUNED = 5          # pruned in the second checkpoint on top of PRUNED: a category none of its arms takes (gen_b/preds)


class StubCpl:
    ref_prior = False

    def __init__(self, evals, arms, Cc):
        self.n_arm, self.n_categories, self.device, self.evals, self.loaded = arms, Cc, torch.device(DEV), evals, []

    def load_model(self, file):
        self.loaded.append(file)

    def eval_model(self, dl):
        return self.evals[len(self.loaded) - 1]


@pytest.mark.parametrize("arms", [3, 2])
def test_summary_of_the_fixture_dictionaries_equals_the_reference(arms, tmp_path, capsys):
    Cc = int(S["cfg"][1])
    cpl = StubCpl(MR.fixture_evals(S, arms), arms, Cc)
    files = ["run/model_0.pth", "run/model_1.pth"]
    got = summarize_inference(cpl, files, None, saving_folder=str(tmp_path))
    assert cpl.loaded == files
    assert capsys.readouterr().out.splitlines() == ["Model /model_0.pth", "Model /model_1.pth"]
    want = {k[3:]: S[k] for k in S.files if k.startswith(f"a{arms}/")}
    MR.assert_same_summary(MR.flatten_summary(got), want)
    assert got["x_rec"] == [] and got["num_pruned"] == [list(range(Cc))] * 2
    with open(tmp_path / f"summary_performance_K_{Cc}_narm_{arms}.p", "rb") as fh:
        MR.assert_same_summary(MR.flatten_summary(pickle.load(fh)), want)


def test_a_single_file_name_means_one_file():
    Cc = int(S["cfg"][1])
    one = summarize_inference(StubCpl(MR.fixture_evals(S, 3), 3, Cc), "run/model_0.pth", None)
    assert len(one["pred_label"]) == 1 and len(one["consensus"]) == 3
    assert np.array_equal(one["consensus"][2], S["a3/consensus/2"])


def _sd(tag, also_pruned=None):
    sd = {k[5:]: torch.from_numpy(np.asarray(G[k])) for k in G.files if k.startswith(f"sd_{tag}/")}
    sd = {k: (v.float() if v.is_floating_point() else v) for k, v in sd.items()}
    if also_pruned is not None:
        for k, v in sd.items():
            if "fcc" in k and k.endswith("bias"):
                v[also_pruned] = 0.0
    return sd


def test_summarize_and_evaluate_end_to_end_on_two_checkpoints(tmp_path):
    from distributed_vae_amd.cpl_mixvae import cpl_mixVAE
    t = cpl_mixVAE(saving_folder="", device=0, save_flag=False)
    t.init_model(n_categories=K_, state_dim=S_DIM, input_dim=D, fc_dim=H, lowD_dim=L, x_drop=0.5, s_drop=0.2, n_arm=A, temp=1.0,
                 tau=0.005)
    files = []
    for epoch, (tag, extra) in enumerate((("a", None), ("b", ALSO_PRUNED)), start=1):
        t.model.load_state_dict(_sd(tag, extra))
        files.append(str(tmp_path / f"cpl_mixVAE_model_epoch_{epoch}.pth"))
        t.save_checkpoint(files[-1])
    x = torch.from_numpy(G["x"]).float()
    dl = DataLoader(TensorDataset(x, torch.arange(NC, dtype=torch.float32)), batch_size=BATCH, shuffle=False)   # 64, 64, 22
    seen, inner = [], t.eval_model
    t.eval_model = lambda loader: seen.append(inner(loader)) or seen[-1]
    got = summarize_inference(t, files, dl, saving_folder=str(tmp_path))
    assert len(seen) == 2
    assert seen[0]["prune_indx"].tolist() == [PRUNED] and seen[1]["prune_indx"].tolist() == sorted({ALSO_PRUNED, PRUNED})
    assert not np.array_equal(seen[0]["predicted_label"], seen[1]["predicted_label"])      # two different models
    want = MR.flatten_summary(MR.summarize(seen, A, K_))
    MR.assert_same_summary(MR.flatten_summary(got), want)
    assert got["consensus"][0].shape == (K_ - 1, K_ - 1) and got["consensus"][3].shape == (K_ - 2, K_ - 2)
    assert got["c_prob"].shape == (A, NC, K_) and np.isfinite(np.asarray(got["recon_loss"])).all()
    with open(tmp_path / f"summary_performance_K_{K_}_narm_{A}.p", "rb") as fh:
        MR.assert_same_summary(MR.flatten_summary(pickle.load(fh)), want)
    # evaluate: the glob picks the highest epoch; one-hot targets from the first model's labels of arm 0, numbered densely
    # (the reference reads the columns 0..F_used-1, so the cell types in use must be the leading ones)
    targets = np.eye(K_, dtype=np.int64)[np.unique(seen[0]["predicted_label"][0], return_inverse=True)[1]]
    res = evaluate(t, str(tmp_path / "cpl_mixVAE_model_epoch_*.pth"), dl, targets)
    assert list(res) == ["pairwise", "all", "mi", "avg_mi", "arms"] and res["arms"] == A and len(res["mi"]) == A
    last = seen[-1]
    assert len(seen) == 3 and np.array_equal(last["predicted_label"], seen[1]["predicted_label"])    # epoch 2 was loaded
    assert {k: res[k] for k in ("all", "pairwise")} == MR.avg_consensus(last["predicted_label"])
    # the tables are those of the restatement: the device's values sit within 16 x the largest recorded e_ref of it
    K = np.load(os.path.join(GOLDEN, "mutinfo_kat.npz"))
    ref, dens = MR.mutinfo_arms(last["z_prob"], targets, with_dens=True)
    assert len(dens) and dens.min() >= 1e-3
    tol = (16 + 8) * max(float(K[f"c{k}/e_ref"]) for k in range(3))                          # N = 150 <= 300
    for a in range(A):
        assert abs(res["mi"][a] - MR.avg(ref[a])) <= tol
    assert res["avg_mi"] == np.mean(res["mi"]).item() and all(isinstance(v, float) for v in res["mi"])

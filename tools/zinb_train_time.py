"""Timing of ZINB training through ``cpl_mixVAE.train`` at A = 2, N = 22 365, D = 5032, H = 100, batches of
5000 cells of a resident matrix (``DeviceLoader``, unshuffled: 4 batches of 5000 and one of 2365), on synthetic counts of
tools/zinb_time.py's kind.  Wall clock with a device synchronisation on either side, medians of --repeats:

  * an epoch's steps through the trainer (``epoch_steps``: ``_zinb_step`` on gathered batches, pipelined) beside an epoch of
    ``cpl_mixVAE.fit_zinb`` -- which this change leaves as it was -- in the same process, A / B / A / B;
  * the consensus pass on the training loader and the validation block on a 2237-cell loader, as ``train`` runs them;
  * ``train(n_epoch=1)`` whole, without and with the validation loader;
  * ``eval_model`` on 5000 cells in batches of 1000, the ZINB model beside its MSE twin (the same weights without the p / r
    heads).

    python tools/zinb_train_time.py [--repeats R] [--out profiles/zinb_train_time.json]"""
import argparse
import contextlib
import io
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import distributed_vae_amd  # noqa: F401,E402
import zinb_restatement as ZR  # noqa: E402

NB, NC, NV, NE, BE, D, H, SEED = 5000, 22365, 2237, 5000, 1000, 5032, 100, 0
DEV = "cuda:0"


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def median(v):
    return sorted(v)[len(v) // 2]


def trainer(mode):
    from distributed_vae_amd.cpl_mixvae import cpl_mixVAE
    torch.manual_seed(SEED)
    t = cpl_mixVAE(saving_folder="", device=0, save_flag=False)
    t.init_model(n_categories=92, state_dim=2, input_dim=D, fc_dim=H, lowD_dim=10, n_arm=2, temp=1.0, tau=0.005, mode=mode)
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "zinb_train_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("zinb_train_time needs a GPU")
    from distributed_vae_amd.utils.dataloader import DeviceLoader
    data = ZR.counts_matrix(NC + NV, D, torch.Generator().manual_seed(SEED + 1)).to(DEV)
    dl = DeviceLoader(data, torch.arange(NC), NB, False, False)
    vl = DeviceLoader(data, torch.arange(NC, NC + NV), NB, False, False)
    el = DeviceLoader(data, torch.arange(NE), BE, False, False)
    t, f = trainer("ZINB"), trainer("ZINB")
    quiet = contextlib.redirect_stdout(io.StringIO())

    def steps():
        acc = torch.zeros(5 + 3 * t.n_arm, device=DEV)
        for buf in t.epoch_steps(dl):
            acc += buf

    state = [f.fit_zinb(dl, 1)["state"]]                  # warm-up epochs of both
    t.model.train()
    steps()

    def fit():
        state[0] = f.fit_zinb(dl, 1, state=state[0])["state"]

    ab = {"train_steps": [], "fit_zinb": []}
    for _ in range(a.repeats):                            # A / B / A / B
        ab["train_steps"].append(wall_ms(steps))
        ab["fit_zinb"].append(wall_ms(fit))
    out = {"shape": {"A": 2, "N": NC, "D": D, "H": H, "batch": NB, "batches": len(dl), "validation_cells": NV},
           "repeats": a.repeats, "device": torch.cuda.get_device_name(0), "wall_ms": "medians; a device synchronisation on either side",
           "epoch_steps_through_the_trainer_ms": median(ab["train_steps"]), "fit_zinb_epoch_ms": median(ab["fit_zinb"]),
           "epoch_steps_all_ms": ab["train_steps"], "fit_zinb_all_ms": ab["fit_zinb"]}
    out["steps_over_fit_zinb"] = out["epoch_steps_through_the_trainer_ms"] / out["fit_zinb_epoch_ms"]
    t.consensus(dl, whole_set=False)
    t.validate(vl, full=True)
    out["consensus_pass_ms"] = median([wall_ms(lambda: t.consensus(dl, whole_set=False)) for _ in range(a.repeats)])
    out["validation_block_ms"] = median([wall_ms(lambda: t.validate(vl, full=True)) for _ in range(a.repeats)])
    with quiet:
        out["train_one_epoch_ms"] = median([wall_ms(lambda: t.train(dl, None, 1, good_enuf_consensus=2.0)) for _ in range(a.repeats)])
        out["train_one_epoch_with_validation_ms"] = median([wall_ms(lambda: t.train(dl, vl, 1, good_enuf_consensus=2.0))
                                                            for _ in range(a.repeats)])
    # eval_model: the ZINB model beside its MSE twin
    m = trainer("MSE")
    m.model.load_state_dict({k: v for k, v in t.model.state_dict().items() if not k.startswith(("fc11_p.", "fc11_r."))})
    ez, em = t.eval_model(el), m.eval_model(el)
    n = max(3, a.repeats // 2)
    out["eval_model"] = {"cells": NE, "batch": BE, "zinb_ms": median([wall_ms(lambda: t.eval_model(el)) for _ in range(n)]),
                         "mse_twin_ms": median([wall_ms(lambda: m.eval_model(el)) for _ in range(n)]),
                         "total_loss_rec_zinb": [float(v) for v in ez["total_loss_rec"]],
                         "total_loss_rec_mse_twin": [float(v) for v in em["total_loss_rec"]]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()

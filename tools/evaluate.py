"""Score a trained checkpoint as the reference's evaluation.py::main does: the average adjusted mutual information of every arm
against the cell types, and the consensus of the arms' labels (distributed_vae_amd.evaluation.evaluate).

    python tools/evaluate.py --model 'run/model/cpl_mixVAE_model_*' --data cells.npz --arms 3 --categories 92 \
        [--state-dim 2] [--latent-dim 10] [--fc-dim 100] [--batch-size 5000] [--out A3.npy]

--model  a checkpoint, or a glob pattern of which the one with the highest ``_epoch_<n>`` is taken (``parse_epoch``)
--data   a .npz, or a .npy holding a pickled dictionary, with the cells [N, D] under --x-key (default ``log1p``) and the
         one-hot cell types [N, F] under --targets-key (default ``c_onehot``): the reference's ``load_data`` keys
--out    where to ``np.save`` the result dictionary (as the reference does); it is always printed
"""
import argparse
import os
import sys

import numpy as np
import torch
from torch.utils.data import DataLoader, TensorDataset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import distributed_vae_amd  # noqa: F401,E402
from distributed_vae_amd.cpl_mixvae import cpl_mixVAE  # noqa: E402
from distributed_vae_amd.evaluation import evaluate  # noqa: E402


def load_cells(path, x_key, targets_key):
    data = np.load(path, allow_pickle=path.endswith(".npy"))
    if path.endswith(".npy"):
        data = data.item()
    return np.asarray(data[x_key], dtype=np.float32), np.asarray(data[targets_key])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--model", required=True)
    ap.add_argument("--data", required=True)
    ap.add_argument("--x-key", default="log1p")
    ap.add_argument("--targets-key", default="c_onehot")
    ap.add_argument("--arms", type=int, required=True)
    ap.add_argument("--categories", type=int, required=True)
    ap.add_argument("--state-dim", type=int, default=2)
    ap.add_argument("--latent-dim", type=int, default=10)
    ap.add_argument("--fc-dim", type=int, default=100)
    ap.add_argument("--batch-size", type=int, default=5000)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    x, targets = load_cells(args.data, args.x_key, args.targets_key)
    cpl = cpl_mixVAE(saving_folder="", device="cuda", save_flag=False)
    cpl.init_model(n_categories=args.categories, state_dim=args.state_dim, input_dim=x.shape[1], fc_dim=args.fc_dim,
                   lowD_dim=args.latent_dim, n_arm=args.arms)
    dl = DataLoader(TensorDataset(torch.from_numpy(x), torch.arange(len(x), dtype=torch.float32)), batch_size=args.batch_size,
                    shuffle=False)
    res = evaluate(cpl, args.model, dl, targets)
    if args.out:
        np.save(args.out, res)
    print(res)


if __name__ == "__main__":
    main()

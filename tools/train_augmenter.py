#!/usr/bin/env python
"""Train an augmenter on the device and write the ``aug_file`` the trainer loads (reference: dist/train_agumenter.py and
mmidas/augmentation/train.py, MSE mode; the discriminator is not built: it has no influence on the augmenter, see
``distributed_vae_amd.augmentation.train_augmenter``).

    python tools/train_augmenter.py --synthetic 2048 5032 --n_epoch 2 --saving-folder out/
    python tools/train_dp.py --aug_file out/augmenter.pth --genes 5032 --gpus 1 --n_epoch 2
"""
from __future__ import annotations

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 546


def parse(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--latent_dim", default=10, type=int, help="latent dimension")
    p.add_argument("--n_epoch", default=10000, type=int, help="number of epochs to train")
    p.add_argument("--batch_size", default=5000, type=int, help="batch size")
    p.add_argument("--lr", default=0.001, type=float, help="learning rate")
    p.add_argument("--ws", default=[1, 0.5, 0.1, 0.5], type=float, nargs=4, help="weights of the augmenter loss (only the fourth acts)")
    p.add_argument("--dim_noise", default=50, type=int, help="noise dimension")
    p.add_argument("--p_drop", default=0.5, type=float, help="input probability of dropout")
    p.add_argument("--loss_mode", default="MSE", type=str, help="MSE (ZINB is refused)")
    p.add_argument("--n_dim", default=500, type=int, help="width of the middle layers (the reference's fixed 500)")
    p.add_argument("--data", default="", type=str, help="dense float32 [cells, genes] .npy matrix (log1p counts)")
    p.add_argument("--synthetic", default=None, type=int, nargs=2, metavar=("N", "D"), help="N synthetic cells of D genes instead")
    p.add_argument("--saving-folder", dest="saving_folder", default=".", type=str, help="where augmenter.pth goes")
    p.add_argument("--resume", default="", type=str, help="continue from this augmenter.pth")
    p.add_argument("--device", default=0, type=int, help="GPU index")
    return p.parse_args(argv)


def main(argv=None) -> int:
    a = parse(argv)
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    import distributed_vae_amd  # noqa: F401
    from distributed_vae_amd.augmentation import Augmenter_smartseq, train_augmenter
    if not torch.cuda.is_available():
        raise SystemExit("no GPU (the HIP path has no CPU fallback)")
    dev = torch.device("cuda", a.device)
    if a.data:
        data = torch.from_numpy(np.load(a.data).astype(np.float32)).to(dev)
    elif a.synthetic:
        n, d = a.synthetic
        g = torch.Generator(device=dev).manual_seed(SEED)
        data = (torch.rand(n, d, generator=g, device=dev) < 0.2).float()
        data *= torch.randn(n, d, generator=g, device=dev).abs() * 3.0
    else:
        raise SystemExit("give --data FILE.npy or --synthetic N D")
    n, d = data.shape
    print(f"# cells: {n}, # genes: {d}", flush=True)
    folder = a.saving_folder.rstrip("/") + "/"
    os.makedirs(folder, exist_ok=True)
    parameters = {"batch_size": a.batch_size, "num_epochs": a.n_epoch, "learning_rate": a.lr, "alpha": 0.2, "num_z": a.latent_dim,
                  "num_n": a.dim_noise, "lambda": list(a.ws), "dataset_file": a.data, "mode": a.loss_mode, "initial_w": False,
                  "affine": False, "saving_path": folder, "save": True, "n_features": d}
    torch.manual_seed(SEED)
    netA = Augmenter_smartseq(noise_dim=a.dim_noise, latent_dim=a.latent_dim, input_dim=d, n_dim=a.n_dim, p_drop=a.p_drop)
    bs = min(a.batch_size, n)

    class Loader:       # shuffled full batches of the resident matrix (drop_last, as the reference's fixed-size labels need)
        def __len__(self):
            return n // bs

        def __iter__(self):
            perm = torch.randperm(n, device=dev)
            for i in range(n // bs):
                yield data[perm[i * bs:(i + 1) * bs]], None
    train_augmenter(netA, None, Loader(), parameters, dev, resume=a.resume or None)
    print(f"wrote {folder}augmenter.pth", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())

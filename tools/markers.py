"""Marker genes of the categories: the rank-sum test of every gene, each category against the rest, on the device
(distributed_vae_amd.utils.marker_analysis; cpl_mixVAE.category_markers).

    python tools/markers.py --synthetic 4096 512 8 [--top 5] [--out markers.npz]
    python tools/markers.py --model 'run/model/cpl_mixVAE_model_*' --data cells.npz --arms 2 --categories 92 \
        [--arm 0] [--state-dim 2] [--latent-dim 10] [--fc-dim 100] [--batch-size 5000] [--genes-key gene_id] [--top 20]

--synthetic N D K  log1p-like counts with 60 % zeros in which gene 3 + (D // K) k is raised in the cells of category k; the
         categories are the planted ones (no model), and the run fails unless every planted gene tops its category
--model  a checkpoint, or a glob pattern of which the one with the highest ``_epoch_<n>`` is taken; the categories are arm
         --arm's labels on the cells of --data (a .npz, or a .npy holding a pickled dictionary, the cells [N, D] under
         --x-key, default ``log1p``); at most 32768 cells, with --block-cells 1048576
--block-cells  ``auto`` (the blocked rank sums above 32768 cells) or a block size, a power of two in [128, 32768] (the
         blocked rank sums at any size); without it the one-call path and its cap
--out    where to ``np.savez`` the result: every array of the ``rank_sum_test`` dictionary, and ``top_genes`` [G, top]
"""
import argparse
import glob
import os
import sys

import numpy as np
import torch
from torch.utils.data import DataLoader, TensorDataset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import distributed_vae_amd  # noqa: F401,E402
from distributed_vae_amd.utils import marker_analysis as MA  # noqa: E402


def planted(n, D, K, seed=0):
    """(x float32 [n, D], labels int64 [n], the planted gene of every category)"""
    rng = np.random.default_rng(seed)
    counts = rng.poisson(3.0, size=(n, D)) * (rng.random((n, D)) >= 0.6)
    x = np.log1p(counts).astype(np.float32)
    labels = rng.integers(0, K, n).astype(np.int64)
    genes = 3 + (D // K) * np.arange(K)
    for k in range(K):
        x[labels == k, genes[k]] += np.float32(2.0)
    return x, labels, genes


def report(res, top, names=None):
    markers = res["markers"] if "markers" in res else MA.marker_genes(res, n_top=top, gene_names=names)
    for g, m in enumerate(markers):
        shown = ", ".join(f"{(m['names'][i] if m['names'] is not None else m['genes'][i])} (z {m['z'][i]:.1f}, "
                          f"q {m['pval_adj'][i]:.1e}, lfc {m['logfc'][i]:+.2f})" for i in range(len(m["genes"])))
        print(f"category {m['group']} ({int(res['n'][g])} cells): {shown}")
    return np.stack([np.pad(m["genes"], (0, top - len(m["genes"])), constant_values=-1) for m in markers])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--synthetic", type=int, nargs=3, metavar=("N", "D", "K"))
    ap.add_argument("--model", default="")
    ap.add_argument("--data", default="")
    ap.add_argument("--x-key", default="log1p")
    ap.add_argument("--genes-key", default="")
    ap.add_argument("--arms", type=int, default=2)
    ap.add_argument("--arm", type=int, default=0)
    ap.add_argument("--categories", type=int, default=0)
    ap.add_argument("--state-dim", type=int, default=2)
    ap.add_argument("--latent-dim", type=int, default=10)
    ap.add_argument("--fc-dim", type=int, default=100)
    ap.add_argument("--batch-size", type=int, default=5000)
    ap.add_argument("--eps", type=float, default=0.0)
    ap.add_argument("--top", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--block-cells", default=None, type=lambda v: v if v == "auto" else int(v))
    args = ap.parse_args()
    if args.synthetic:
        n, D, K = args.synthetic
        if not (K >= 2 and D >= K and 3 + (D // K) * (K - 1) < D and n >= 4 * K):
            ap.error("--synthetic needs K >= 2, D >= K, N >= 4 K and room for the last planted gene: 3 + (D // K) (K - 1) < D")
        x, labels, genes = planted(n, D, K)
        res = MA.rank_sum_test(x, labels, eps=args.eps, device="cuda", block_cells=args.block_cells)
        top = report(res, args.top)
        found = top[:, 0]
        print(f"planted genes {genes.tolist()}; top genes {found.tolist()}")
        if not np.array_equal(found, genes):
            raise SystemExit("the planted markers were NOT recovered")
        print("planted markers recovered")
    else:
        if not (args.model and args.data and args.categories):
            ap.error("give --synthetic N D K, or --model, --data and --categories")
        from distributed_vae_amd.cpl_mixvae import cpl_mixVAE
        from distributed_vae_amd.evaluation import parse_epoch
        data = np.load(args.data, allow_pickle=args.data.endswith(".npy"))
        if args.data.endswith(".npy"):
            data = data.item()
        x = np.asarray(data[args.x_key], dtype=np.float32)
        names = np.asarray(data[args.genes_key]) if args.genes_key else None
        model_file = args.model
        if glob.has_magic(model_file):
            found = glob.glob(model_file)
            if not found:
                raise FileNotFoundError(f"no checkpoint matches {model_file}")
            model_file = max(found, key=parse_epoch)
        cpl = cpl_mixVAE(saving_folder="", device="cuda", save_flag=False)
        cpl.init_model(n_categories=args.categories, state_dim=args.state_dim, input_dim=x.shape[1], fc_dim=args.fc_dim,
                       lowD_dim=args.latent_dim, n_arm=args.arms)
        cpl.load_model(model_file)
        dl = DataLoader(TensorDataset(torch.from_numpy(x), torch.arange(len(x), dtype=torch.float32)), batch_size=args.batch_size,
                        shuffle=False)
        res = cpl.category_markers(dl, arm=args.arm, n_top=args.top, eps=args.eps, block_cells=args.block_cells)
        if names is not None:
            res["markers"] = MA.marker_genes(res, n_top=args.top, gene_names=names)
        top = report(res, args.top, names)
    if args.out:
        np.savez(args.out, top_genes=top, **{k: v for k, v in res.items() if isinstance(v, np.ndarray)})
        print(f"wrote {args.out}")


if __name__ == "__main__":
    main()

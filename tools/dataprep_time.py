"""Time the data preparation at the Smart-seq shape on one GPU and write profiles/dataprep_time.json.

Seeded synthetic counts, 25 481 cells x 45 768 genes int32 with about 20 % non-zeros, dense and CSR, and the notebook's
selection of 5032 genes and 22 365 cells:

  * HIP-event medians of ``mmvae_cpm_dense`` and ``mmvae_cpm_csr`` alone (log-CPM to float32), with the selection and with
    one gene selected (then the launch is the norm pass and little else), the matrix bytes each moves over its time, next to
    the 6.3 TB/s a streaming kernel reaches on this part, and which pass binds;
  * end to end from host arrays (``logcpm(counts, genes=..., cells=..., out="torch", dtype=torch.float32)``), the upload
    listed separately;
  * the reference arithmetic on the same host, once: the numpy restatement (tests/dataprep_restatement.py) on the whole
    matrix plus the column and row selection and the float32 cast (``--no-host-reference`` skips it);
  * 64 sampled rows of the device result, the last one among them, against the host -- the matrix is 4.66 GB, so its byte
    offsets pass 2^32: the only place the 64-bit offsets are exercised;
  * ``gene_stats`` and ``reorder_genes`` on the 22 365 x 5032 float32 result.

    python tools/dataprep_time.py [--repeats R] [--no-host-reference] [--out profiles/dataprep_time.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import distributed_vae_amd  # noqa: F401,E402
import dataprep_restatement as DR  # noqa: E402
from distributed_vae_amd import _native as N  # noqa: E402
from distributed_vae_amd.utils import tools as T  # noqa: E402

NC, NG, SEL_C, SEL_G = 25481, 45768, 22365, 5032
HBM_COPY = 6.3e12
CHUNK = 2048


def _median_ms(fn, repeats):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        t.append(e0.elapsed_time(e1))
    t.sort()
    return t[len(t) // 2]


def _wall_s(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def to_csr_device(dense):
    """Canonical CSR of the dense device matrix, a chunk of rows at a time."""
    per_row, cols, vals = [], [], []
    for i in range(0, NC, CHUNK):
        piece = dense[i:i + CHUNK]
        keep = piece != 0
        per_row.append(keep.sum(dim=1))
        cols.append(keep.nonzero()[:, 1].to(torch.int32))
        vals.append(piece[keep])
    indptr = torch.zeros(NC + 1, dtype=torch.int64, device=dense.device)
    indptr[1:] = torch.cumsum(torch.cat(per_row), 0)
    return indptr, torch.cat(cols), torch.cat(vals)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--no-host-reference", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dataprep_time.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(546)
    dense = torch.empty(NC, NG, dtype=torch.int32, device=dev)
    for i in range(0, NC, CHUNK):
        m = min(CHUNK, NC - i)
        keep = torch.rand(m, NG, device=dev, generator=g) < 0.2
        dense[i:i + m] = torch.randint(1, 200, (m, NG), device=dev, generator=g, dtype=torch.int32) * keep
    dense[17] = 0                                                         # a zero row
    dense[NC - 1, NG - 1] = 7                                             # the matrix's very last element is stored
    indptr, indices, data = to_csr_device(dense)
    nnz = int(indices.numel())
    rng = np.random.default_rng(546)
    genes = rng.permutation(NG)[:SEL_G]
    others = np.setdiff1d(np.arange(NC), [17, NC - 1])
    cells = np.sort(np.concatenate([rng.choice(others, SEL_C - 2, replace=False), [17, NC - 1]]))   # the zero row and the last row
    n_sel = int(cells.size)
    rows_d = torch.from_numpy(cells).to(dev)
    genes_d = torch.from_numpy(genes.astype(np.int32)).to(dev)
    one_d = genes_d[:1].contiguous()
    inv = np.full(NG, -1, dtype=np.int32)
    inv[genes] = np.arange(SEL_G, dtype=np.int32)
    inv_d = torch.from_numpy(inv).to(dev)
    inv1 = np.full(NG, -1, dtype=np.int32)
    inv1[genes[0]] = 0
    inv1_d = torch.from_numpy(inv1).to(dev)
    nnz_sel = int((indptr[1:] - indptr[:-1])[rows_d].sum())
    res = {"shape": {"cells": NC, "genes": NG, "selected_cells": n_sel, "selected_genes": SEL_G, "nonzero_fraction": nnz / (NC * NG)},
           "repeats": args.repeats, "dense_matrix_bytes": NC * NG * 4, "csr_bytes": nnz * 8 + (NC + 1) * 8,
           "wide_loads": bool(N.cpm_wide(dense)), "hbm_streaming_bytes_per_s": HBM_COPY, "kernel": {}}

    def entry(ms, read_bytes, written_bytes):
        return {"ms": ms, "bytes_read": read_bytes, "bytes_written": written_bytes,
                "bytes_per_s": (read_bytes + written_bytes) / (ms * 1e-3),
                "fraction_of_6.3TBs": (read_bytes + written_bytes) / (ms * 1e-3) / HBM_COPY}

    row_bytes = n_sel * NG * 4
    out_bytes = n_sel * SEL_G * 4
    ms_full = _median_ms(lambda: N.cpm_dense(dense, rows_d, genes_d, 1e6, True, torch.float32), args.repeats)
    ms_one = _median_ms(lambda: N.cpm_dense(dense, rows_d, one_d, 1e6, True, torch.float32), args.repeats)
    res["kernel"]["cpm_dense"] = {"selection": entry(ms_full, row_bytes, out_bytes), "one_gene": entry(ms_one, row_bytes, n_sel * 4),
                                  "binds": "the norm pass (the stream of the selected rows)" if ms_one > 0.5 * ms_full
                                  else "the gather-and-log1p pass"}
    csr_read = nnz_sel * 8 + n_sel * 16
    ms_full = _median_ms(lambda: N.cpm_csr(indptr, indices, data, (NC, NG), inv_d, SEL_G, rows_d, 1e6, True, torch.float32), args.repeats)
    ms_one = _median_ms(lambda: N.cpm_csr(indptr, indices, data, (NC, NG), inv1_d, 1, rows_d, 1e6, True, torch.float32), args.repeats)
    res["kernel"]["cpm_csr"] = {"selection": entry(ms_full, csr_read, out_bytes), "one_gene": entry(ms_one, csr_read, n_sel * 4),
                                "binds": "the norm pass (the LDS windows of the dense row)" if ms_one > 0.5 * ms_full
                                else "the zeros and the scatter of the output"}

    # dense and CSR agree to the bit at this size too
    a = N.cpm_dense(dense, rows_d, genes_d, 1e6, True, torch.float32)
    b = N.cpm_csr(indptr, indices, data, (NC, NG), inv_d, SEL_G, rows_d, 1e6, True, torch.float32)
    res["dense_and_csr_bit_equal"] = bool(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]))
    # 64 sampled rows, the last among them, against the host
    pick = np.unique(np.concatenate([rng.choice(n_sel, 63, replace=False), [n_sel - 1]]))
    host_rows = dense[rows_d[torch.from_numpy(pick).to(dev)]].cpu().numpy()
    want, sums = DR.cpm(host_rows, 1e6, True, genes=genes)
    got = a[0][torch.from_numpy(pick).to(dev)].cpu().numpy()
    want32 = want.astype(np.float32)
    res["sampled_rows"] = {"rows": int(pick.size), "includes_last_row_of_the_matrix": bool(cells[pick[-1]] == NC - 1),
                           "largest_byte_offset": int((NC - 1) * NG * 4 + (NG - 1) * 4),
                           "norms_exact": bool(np.array_equal(a[1][torch.from_numpy(pick).to(dev)].cpu().numpy(), sums)),
                           "within_one_float32_ulp": bool((np.abs(got.astype(np.float64) - want32) <= np.spacing(want32)).all()),
                           "zeros_exact": bool(np.array_equal(got == 0, want == 0))}
    del a, b

    # end to end from host arrays
    t_dl, counts_h = _wall_s(lambda: dense.cpu().numpy())
    csr_h = (indptr.cpu().numpy(), indices.cpu().numpy(), data.cpu().numpy(), (NC, NG))
    t_up, _ = _wall_s(lambda: torch.from_numpy(counts_h).to(dev))
    t_up_csr, _ = _wall_s(lambda: [torch.from_numpy(x).to(dev) for x in csr_h[:3]])
    t_e2e, _ = _wall_s(lambda: T.logcpm(counts_h, genes=genes, cells=cells, out="torch", dtype=torch.float32))
    t_e2e_csr, _ = _wall_s(lambda: T.logcpm(csr_h, genes=genes, cells=cells, out="torch", dtype=torch.float32))
    t_res, x32 = _wall_s(lambda: T.logcpm(dense, genes=genes, cells=cells, out="torch", dtype=torch.float32))
    res["end_to_end_s"] = {"download_of_the_dense_matrix": t_dl, "dense_from_host": t_e2e, "dense_upload_alone": t_up, "csr_from_host": t_e2e_csr, "csr_upload_alone": t_up_csr,
                           "csr_includes": "the canonical-form check on the host", "dense_resident_on_device": t_res}
    del csr_h

    # the statistics on the prepared matrix
    ms_gs = _median_ms(lambda: N.gene_stats(x32, 0.1), args.repeats)
    t_ro, order = _wall_s(lambda: T.reorder_genes(x32))
    mat = n_sel * SEL_G * 4
    res["gene_stats"] = {"shape": [n_sel, SEL_G], "kernel_ms": ms_gs, "matrix_bytes_per_s": mat / (ms_gs * 1e-3),
                         "fraction_of_6.3TBs": mat / (ms_gs * 1e-3) / HBM_COPY,
                         "workspace_bytes": int(N.lib().mmvae_gene_stats_workspace_bytes(n_sel, SEL_G))}
    res["reorder_genes"] = {"wall_s": t_ro, "kept": int(order.size)}
    k_host = DR.counts_above(x32[:, :64].cpu().numpy(), 0.1)
    res["gene_stats"]["counts_exact_on_64_genes"] = bool(np.array_equal(N.gene_stats(x32, 0.1)[0][:64].cpu().numpy(), k_host))
    del x32
    torch.cuda.empty_cache()

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")

    res["host_reference_arithmetic"] = "not measured"
    write()                                                               # (the host pass below is long: keep what is measured)
    if not args.no_host_reference:
        t0 = time.perf_counter()
        full = DR.logcpm(counts_h)
        kept = full[:, genes][cells].astype(np.float32)
        dt = time.perf_counter() - t0
        res["host_reference_arithmetic"] = {"s": dt, "result_shape": list(kept.shape),
                                            "note": "numpy restatement of normalize + log1p on the whole matrix in float64, then the "
                                                    "column and row selection and the float32 cast, run once"}
        write()
    print(json.dumps(res))


if __name__ == "__main__":
    main()

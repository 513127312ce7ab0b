"""Build container only: run the REAL reference (oracle/ref_loader) encoder and intermed on a small model and commit what it
computed as the data-only fixture tests/golden/encode_a2.npz (tests/test_encode_cpu.py, tests/test_gpu_encode.py).

Holds, for the model of tools/gen_golden_decode.py (A = 2, D = 64, H = 16, L = 4, C = 6, S = 2; BatchNorm running statistics
randomised so that eval mode is not the identity), in fp64 and fp32:
  sd/<key>                 the state dict before any call (parameters and BatchNorm buffers, fp64)
  x                        the cells [N, D]
  <tag>/enc/x_low, c_prob  eval-mode encoder(x, a) per arm [A, N, L] / [A, N, C]
  im/y                     a recorded intermed input per arm [A, N, L + C]
  <tag>/im/mu, var         intermed(y[a], a) per arm [A, N, S]
  <tag>/tr/x_low, c_prob   training-mode encoder(x, a) per arm at x_drop = 0 (no random draw)
  <tag>/tr/sd/<key>        the BatchNorm buffers (running_mean, running_var, num_batches_tracked) after those calls

    python -m tools.gen_golden_encode
"""
import os

import numpy as np
import torch

from oracle import ref_loader as RL
from tools.gen_golden_decode import A, C, D, H, L, S, _model

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
N = 37


def main():
    ref = RL.load_reference_nn_model()
    g = torch.Generator().manual_seed(21)
    x = torch.relu(torch.randn(N, D, generator=g, dtype=torch.float64)) * 2
    y = torch.cat((torch.randn(A, N, L, generator=g, dtype=torch.float64),
                   torch.softmax(3 * torch.randn(A, N, C, generator=g, dtype=torch.float64), -1)), dim=-1)
    out = {"x": x.numpy(), "im/y": y.numpy(), "cfg": np.array([A, N, D, H, L, C, S], np.int64)}
    for tag, dtype in (("f64", torch.float64), ("f32", torch.float32)):
        old = torch.get_default_dtype()
        torch.set_default_dtype(dtype)
        try:
            m = _model(ref, dtype)
            if tag == "f64":
                sd64 = {k: v.clone() for k, v in m.state_dict().items()}
                for k, v in sd64.items():
                    out[f"sd/{k}"] = v.detach().cpu().numpy().copy()
            else:   # the same model, rounded (init draws differ between dtypes)
                m.load_state_dict({k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd64.items()})
            with torch.no_grad():
                enc = [m.encoder(x.to(dtype), a) for a in range(A)]
                out[f"{tag}/enc/x_low"] = np.stack([e[0].numpy() for e in enc]).astype(np.float64)
                out[f"{tag}/enc/c_prob"] = np.stack([e[1].numpy() for e in enc]).astype(np.float64)
                im = [m.intermed(y[a].to(dtype), a) for a in range(A)]
                out[f"{tag}/im/mu"] = np.stack([e[0].numpy() for e in im]).astype(np.float64)
                out[f"{tag}/im/var"] = np.stack([e[1].numpy() for e in im]).astype(np.float64)
                m.train()
                m.x_dp.p = 0.0
                tr = [m.encoder(x.to(dtype), a) for a in range(A)]
                out[f"{tag}/tr/x_low"] = np.stack([e[0].numpy() for e in tr]).astype(np.float64)
                out[f"{tag}/tr/c_prob"] = np.stack([e[1].numpy() for e in tr]).astype(np.float64)
                for k, v in m.state_dict().items():
                    if k.startswith("batch_"):
                        out[f"{tag}/tr/sd/{k}"] = v.detach().cpu().numpy().astype(np.float64 if v.is_floating_point() else np.int64)
        finally:
            torch.set_default_dtype(old)
    np.savez_compressed(os.path.join(GOLDEN, "encode_a2.npz"), **out)
    print({k: np.asarray(v).shape for k, v in out.items() if "sd/" not in k})


if __name__ == "__main__":
    main()

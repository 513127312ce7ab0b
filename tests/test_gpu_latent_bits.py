"""The latent kernels compute, bit for bit, what they computed at the commit tests/golden/latent_bits.npz was written at
(tools/latent_bits.py --write with that commit's library): the loss vector, the flat gradients, the BatchNorm running
statistics and the workspace arrays the kernels write, compared as SHA-256 digests of their raw bytes.  The cases
(tools/latent_bits.py CASES) cover both cell geometries, ragged last workgroups, every column-count edge, A = 1, 2, 3, 5,
soft and hard samples, state dropout, explicit and in-kernel noise, a category mask and the eval-mode forward."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("_latent_bits", os.path.join(ROOT, "tools", "latent_bits.py"))
LB = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(LB)


@pytest.fixture(scope="module")
def golden():
    return LB.load_golden()


def test_golden_covers_every_case(golden):
    assert sorted(golden) == sorted(LB.CASES)
    for case, arrs in golden.items():
        want = {"bn_running"} | {k for k, _, _ in LB.FWD}
        if LB.CASES[case][5] != "eval":
            want |= {"loss", "grad", "GMS", "GZC", "G5"}
        assert set(arrs) == want, case


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(LB.CASES))
def test_latent_bits(case, golden):
    got = LB.run_case(case)
    diff = sorted(k for k in set(golden[case]) | set(got) if golden[case].get(k) != got.get(k))
    assert not diff, f"{case}: not bit-identical to the golden digests: {diff}"

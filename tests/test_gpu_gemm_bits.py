"""The tile-engine GEMMs (k_x3_gemm, k_x3_small, k_bf16_gemm) compute, bit for bit, what they computed at the commit
tests/golden/gemm_bits.npz was written at (tools/gemm_bits.py --write with that commit's library): the loss vector, the
flat gradient, the BatchNorm running statistics and the workspace arrays R1 and DZ1 of one fused train step, compared as
SHA-256 digests of their raw bytes.  The cases (tools/gemm_bits.py CASES) cover one, two and three tiles along the cells
and along the genes with ragged last tiles and idle second groups, K tails of both operand orientations, K splits, the
keep-mask under in-kernel and explicit noise and its absence, the row-map instantiations, A = 1, 2, 3 and the bf16 engine (on the batch, through the row map, on its bf16 copy)."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("_gemm_bits", os.path.join(ROOT, "tools", "gemm_bits.py"))
GB = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(GB)


@pytest.fixture(scope="module")
def golden():
    return GB.load_golden()


def test_golden_covers_every_case(golden):
    assert sorted(golden) == sorted(GB.CASES)
    for case, arrs in golden.items():
        assert set(arrs) == GB.expected_keys(case), case


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(GB.CASES))
def test_gemm_bits(case, golden):
    got = GB.run_case(case)
    diff = sorted(k for k in set(golden[case]) | set(got) if golden[case].get(k) != got.get(k))
    assert not diff, f"{case}: not bit-identical to the golden digests: {diff}"

"""The chain kernels compute, bit for bit, what they computed at the commit tests/golden/chain_bits.npz was written at
(tools/chain_bits.py --write with that commit's library): the loss vector, the flat gradients, the BatchNorm running
statistics and the workspace arrays R2..R5, D6..D10, G1..G5, DZ1..DZ5, compared as SHA-256 digests of their raw bytes.
The cases (tools/chain_bits.py CASES) cover one ragged, one full + one ragged and two full + a 2-row block, A = 1, 2, 3, 5,
H = 100 and 128, the fp32x3 and the fp32 form (the latter through both switches that reach it), a training step, the
eval-mode encoder chain, a decode call, a pruned step, explicit and in-kernel noise."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("_chain_bits", os.path.join(ROOT, "tools", "chain_bits.py"))
CB = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(CB)


@pytest.fixture(scope="module")
def golden():
    return CB.load_golden()


def test_golden_covers_every_case(golden):
    assert sorted(golden) == sorted(CB.CASES)
    for case, arrs in golden.items():
        assert set(arrs) == CB.expected_keys(case), case


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CB.CASES))
def test_chain_bits(case, golden):
    got = CB.run_case(case)
    diff = sorted(k for k in set(golden[case]) | set(got) if golden[case].get(k) != got.get(k))
    assert not diff, f"{case}: not bit-identical to the golden digests: {diff}"

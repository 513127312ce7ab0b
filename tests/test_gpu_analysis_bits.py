"""The device analysis routines (silhouette, state_corr, group_moments, gauss_scores, gram, pca_project, cpm_dense, cpm_csr,
gene_stats) compute, bit for bit, what they computed at the commit tests/golden/analysis_bits.npz was written at
(tools/analysis_bits.py --write with that commit's library): every output tensor of every case, compared as SHA-256 digests
of the raw bytes.  The cases (tools/analysis_bits.py CASES) sit at the edges of the pieces these routines share: the segment
table (singleton, empty and multi-segment groups, both sides of the segment length, more than 256 groups, no offsets), the
clamped row-map read (a shuffled map with repeats) and the narrow and wide load forms."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("_analysis_bits", os.path.join(ROOT, "tools", "analysis_bits.py"))
AB = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(AB)


@pytest.fixture(scope="module")
def golden():
    return AB.load_golden()


def test_golden_covers_every_case(golden):
    gold, parent = golden
    assert len(parent) == 40 and set(parent) <= set("0123456789abcdef"), parent
    assert sorted(gold) == sorted(AB.CASES)
    for case, arrs in gold.items():
        assert set(arrs) == AB.expected_keys(case), case


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(AB.CASES))
def test_analysis_bits(case, golden):
    gold = golden[0][case]
    got = AB.run_case(case)
    diff = sorted(k for k in set(gold) | set(got) if gold.get(k) != got.get(k))
    assert not diff, f"{case}: not bit-identical to the golden digests: {diff}"

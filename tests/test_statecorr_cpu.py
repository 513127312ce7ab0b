"""CPU: the host side of the state-gene correlation (corr_analysis, cpl_mixVAE.state_gene_corr).  The two-pass fp64
restatement (tests/statecorr_restatement.py) against the reference's recorded returns (tests/golden/statecorr_kat.npz;
tools/gen_golden_statecorr.py), and on cases with known answers; the host-side contract of mmvae_state_corr: declared,
exported, ABI version unchanged, the workspace size, every bad argument refused before any device work; the public module
importable without scipy, and its refusals.

Bounds.  The restatement and scipy's float64 path both work in fp64 on the same values in the two-pass form; they differ in
the order of a few operations, which is what e_ref64 records (<= 1e-12 for every case, in fact below 1e-15).  The restatement
is compared with the recorded values at e_ref64 itself (it is the same computation that recorded it) plus 1e-15 for another
BLAS.  e_ref32, the distance of scipy's float32 path, must be below 1e-5."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import statecorr_restatement as SR  # noqa: E402
import distributed_vae_amd  # noqa: F401,E402
from distributed_vae_amd import _native as N  # noqa: E402

G = np.load(os.path.join(ROOT, "tests", "golden", "statecorr_kat.npz"))
CASES = [tuple(int(v) for v in row) for row in G["cases"]]
SLACK = 1e-15


# ---- 1. the fixture is what the generator promises -----------------------------------------------------------------------
def test_fixture_is_what_the_generator_promises():
    assert CASES == [(5, 1, 1), (6, 3, 1), (64, 9, 2), (300, 260, 2), (1100, 70, 3), (700, 40, 5)]
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "statecorr_kat.npz")) < 400 * 1024
    assert all(G[k].dtype != object for k in G.files)                       # arrays only
    assert "scipy" in str(G["source"])
    for k, (n, D, S) in enumerate(CASES):
        state, cell = G[f"c{k}/state"], G[f"c{k}/cell"]
        assert state.dtype == np.float32 and state.shape == (n, S) and np.isfinite(state).all()
        assert cell.dtype == np.float32 and cell.shape == (n, D) and np.isfinite(cell).all()
        assert np.array_equal(cell * 4096, np.round(cell * 4096)) and np.array_equal(state * 4096, np.round(state * 4096))
        for name in ("corr32", "corr64", "abs32", "abs64"):
            assert G[f"c{k}/{name}"].dtype == np.float64 and G[f"c{k}/{name}"].shape == (S, D)
        for name in ("gene32", "gene64"):
            assert G[f"c{k}/{name}"].dtype == np.int64 and G[f"c{k}/{name}"].shape == (S, D)
            assert all(sorted(row) == list(range(D)) for row in G[f"c{k}/{name}"])
        assert G[f"c{k}/nan"].dtype == bool and G[f"c{k}/zero"].dtype == bool
        assert 0 <= float(G[f"c{k}/e_ref64"]) <= 1e-12 and 0 <= float(G[f"c{k}/e_ref32"]) <= 1e-5
        if n > 8:
            assert 0.65 <= float((cell == 0).mean()) <= 0.8 and float((cell < 0).mean()) > 0.02
        z, four, five, const_x, const_s = (int(v) for v in G[f"c{k}/planted"])
        pos = (cell > 0).sum(axis=0)
        if z >= 0:
            assert pos[z] == 0 and pos[four] == 4 and pos[five] == 5
            assert G[f"c{k}/zero"][:, [z, four]].all() and not G[f"c{k}/zero"][:, five].any()
        if const_x >= 0:
            assert pos[const_x] > 4 and len(np.unique(cell[cell[:, const_x] > 0, const_x])) == 1
            assert G[f"c{k}/nan"][:, const_x].all()
            assert pos[const_s] > 4 and len(np.unique(state[cell[:, const_s] > 0, 0])) == 1
            assert G[f"c{k}/nan"][0, const_s] and not G[f"c{k}/nan"][1:, const_s].any()


# ---- 2. the restatement is the reference's arithmetic ----------------------------------------------------------------------
@pytest.mark.parametrize("k", range(6))
def test_restatement_equals_recorded_reference(k):
    """The reference alone (its float64 call) stays within the gate: the restatement reproduces it within e_ref64."""
    state, cell, e_ref = G[f"c{k}/state"].astype(np.float64), G[f"c{k}/cell"].astype(np.float64), float(G[f"c{k}/e_ref64"])
    r, cnt, kap = SR.state_corr(state, cell)
    got = np.abs(r[0])
    assert np.array_equal(np.isnan(got), G[f"c{k}/nan"]) and np.array_equal(got == 0, G[f"c{k}/zero"])
    fin = np.isfinite(got)
    err = float(np.abs(got - G[f"c{k}/abs64"])[fin].max())
    print(f"case {k}: worst |restatement - reference| {err:.2e}, e_ref64 {e_ref:.2e}")
    assert err <= e_ref + SLACK
    assert np.array_equal(cnt[0], (cell > 0).sum(axis=0))
    assert (kap[0][fin & (got != 0)] >= 1.0).all() and np.isinf(kap[0][~fin]).all()
    corr, gene = SR.corr_analysis(state, cell)
    for s in range(state.shape[1]):
        want = G[f"c{k}/corr64"][s]
        both = np.isfinite(want)
        assert np.array_equal(np.isnan(corr[s]), np.isnan(want)) and np.abs(corr[s] - want)[both].max() <= e_ref + SLACK
        assert np.array_equal(gene[s], np.argsort(got[s]))


def test_restatement_hand_cases():
    x = np.array([[1.0], [2.0], [3.0], [4.0], [5.0], [0.0], [-3.0]])
    s = np.array([[2.0, -1.0, 7.0]] * 7) * x + np.array([[0.0, 3.0, 0.0]])
    s[:, 2] = 7.0
    r, cnt, kap = SR.state_corr(s, x)
    assert cnt[0, 0] == 5 and r[0, 0, 0] == 1.0 and r[0, 1, 0] == -1.0 and np.isnan(r[0, 2, 0])
    assert kap[0, 0, 0] == 1.0 + 9.0 / 2.0                                  # both have mean^2 / var = 9 / 2 or 36 / 8
    r, cnt, _ = SR.state_corr(s[1:], x[1:])                                 # four expressing cells: 0 by rule
    assert cnt[0, 0] == 4 and not r.any()
    codes = np.array([0, 0, 0, 0, 0, 1, 1])
    r, cnt, _ = SR.state_corr(s, x, codes, 3)                               # groups: 5 cells, none expressing, empty
    assert list(cnt[:, 0]) == [5, 0, 0] and r[0, 0, 0] == 1.0 and not r[1:].any()
    assert np.array_equal(SR.tolerance(np.array([[7]]), np.array([[[2.0]]])), [[[8 * 8 * 2.0 * 2.0 ** -53]]])


# ---- 3. declared, exported, ABI unchanged; the workspace; the launch constants ---------------------------------------------
def _nseg(n, Gn):
    return Gn + n // N.STATECORR_SEG_ROWS


def _ws_bytes(n, D, S, Gn):
    return 8 * (_nseg(n, Gn) * (5 + 5 * S) * D + _nseg(n, Gn) + 1) + 4 * ((Gn + 2) // 2 * 2)


def test_entry_points_declared_exported_and_abi_unchanged():
    hdr = open(os.path.join(ROOT, "include", "mmvae.h")).read()
    assert re.search(r"\bint mmvae_state_corr\(", hdr) and re.search(r"\bsize_t mmvae_state_corr_workspace_bytes\(", hdr)
    assert re.search(r"\bint mmvae_debug_state_corr\(", hdr)
    for word in ("c <= 4", "min == max", "bit-identical", "CALLER'S", "INPUTS MUST BE FINITE",
                 "mmvae_state_corr_workspace_bytes(n, D, S, G)", "8 (c + 1) kappa 2^-53"):
        assert word in hdr, word
    src = open(os.path.join(ROOT, "distributed-vae_amd", "csrc", "api.hip")).read()
    assert "int mmvae_abi_version(void) { return 5; }" in src
    lib = N.lib()
    assert lib.mmvae_abi_version() == 5 == N.ABI_VERSION
    for name in ("mmvae_state_corr", "mmvae_state_corr_workspace_bytes", "mmvae_debug_state_corr"):
        assert hasattr(lib, name), name
    assert callable(N.state_corr)
    build = open(os.path.join(ROOT, "distributed-vae_amd", "build.py")).read()
    assert '"statecorr.hip"' in build


def test_workspace_bytes():
    ws = N.lib().mmvae_state_corr_workspace_bytes
    for n, D, S, Gn in ((1, 1, 1, 1), (255, 5, 1, 1), (256, 5, 1, 1), (257, 5, 2, 3), (22365, 5032, 2, 1), (22365, 5032, 2, 92),
                        (22365, 5032, 32, 92)):
        assert ws(n, D, S, Gn) == _ws_bytes(n, D, S, Gn), (n, D, S, Gn)
    assert _nseg(22365, 92) == 179 and ws(22365, 5032, 2, 92) < 110 * 2 ** 20     # the data set: 179 segments at most, 108 MB
    # grows monotonically in every argument
    base = (1000, 300, 2, 4)
    for i, bigger in enumerate(((1256, 300, 2, 4), (1000, 301, 2, 4), (1000, 300, 3, 4), (1000, 300, 2, 5))):
        assert ws(*bigger) > ws(*base), i
    sizes = [ws(n, 7, 2, 2) for n in range(1, 1100)]
    assert all(b >= a for a, b in zip(sizes, sizes[1:]))
    # 0 for what mmvae_state_corr refuses
    for bad in ((0, 5, 1, 1), (-1, 5, 1, 1), ((1 << 31) + 1, 5, 1, 1), (10, 0, 1, 1), (10, -1, 1, 1), (10, 5, 0, 1),
                (10, 5, -2, 1), (10, 5, 1, 0), (10, 5, 1, -1), (10, 5, 33, 1), (1 << 31, 1 << 20, 1, 1)):
        assert ws(*bad) == 0, bad
    assert ws(10, 5, 32, 1) == _ws_bytes(10, 5, 32, 1) and ws(1 << 31, 5, 1, 1) == _ws_bytes(1 << 31, 5, 1, 1)


def test_launch_constants_are_those_of_the_source():
    """The module attributes the GPU tests size their shapes by are the constants the kernels were built with."""
    hpp = open(os.path.join(ROOT, "distributed-vae_amd", "csrc", "common.hpp")).read()

    def const(name):
        return int(re.search(r"constexpr int " + name + r" = (\d+);", hpp).group(1))
    assert const("SC_SEG_ROWS") == N.STATECORR_SEG_ROWS == 256
    assert const("SC_TILE") == N.STATECORR_TILE == 256
    assert const("SC_MAX_S") == N.STATECORR_MAX_S == 32
    assert N.STATECORR_PATHS == {"auto": -1, "narrow": 0, "wide": 1}


# ---- 4. refusals on the host ------------------------------------------------------------------------------------------------
PTR = 0x1000     # fake device pointers: every case must be refused before anything dereferences them


def _call(data=PTR, ld=40, n_total=100, D=40, rows=PTR, state=PTR, lds=2, n=100, S=2, offsets=PTR, Gn=3, ws=PTR, ws_bytes=None,
          r=PTR, count=PTR, path=None):
    if ws_bytes is None:
        ok = 1 <= n <= 1 << 31 and D >= 1 and 1 <= S <= 32 and Gn >= 1
        ws_bytes = _ws_bytes(n, D, S, Gn) if ok else 1 << 40
    if path is None:
        return N.lib().mmvae_state_corr(data, ld, n_total, D, rows, state, lds, n, S, offsets, Gn, ws, ws_bytes, r, count, None)
    return N.lib().mmvae_debug_state_corr(data, ld, n_total, D, rows, state, lds, n, S, offsets, Gn, ws, ws_bytes, r, count,
                                          path, None)


BAD = [
    ("null_data", dict(data=None), -1), ("null_state", dict(state=None), -1), ("null_ws", dict(ws=None), -1),
    ("null_r", dict(r=None), -1), ("null_count", dict(count=None), -1),
    ("n0", dict(n=0), -1), ("n_neg", dict(n=-3), -1), ("n_past_2_31", dict(n=(1 << 31) + 1), -1),
    ("n_total0", dict(n_total=0), -1), ("no_rows_n_above_n_total", dict(rows=None, n=101), -1),
    ("D0", dict(D=0), -1), ("D_neg", dict(D=-1), -1), ("S0", dict(S=0), -1), ("S_neg", dict(S=-1), -1),
    ("G0", dict(Gn=0), -1), ("G_neg", dict(Gn=-1), -1),
    ("ld_below_D", dict(ld=39), -1), ("lds_below_S", dict(lds=1), -1), ("ws_misaligned", dict(ws=PTR + 4), -1),
    ("S33", dict(S=33, lds=33), -2), ("S33_ws_small", dict(S=33, lds=33, ws_bytes=8), -2),
    ("grid_too_large", dict(n=1 << 31, n_total=1 << 31, D=1 << 20, ld=1 << 20, ws_bytes=1 << 62), -2),
    ("ws_small", dict(ws_bytes=_ws_bytes(100, 40, 2, 3) - 1), -4),
    ("debug_path_2", dict(path=2), -1), ("debug_path_neg2", dict(path=-2), -1),
    ("debug_wide_on_odd_ld", dict(path=1, ld=41), -2), ("debug_wide_on_offset_base", dict(path=1, data=PTR + 4), -2),
]


@pytest.mark.parametrize("case,kw,rc", BAD, ids=[b[0] for b in BAD])
def test_state_corr_rejects_bad_arguments(case, kw, rc):
    assert _call(**kw) == rc, N.lib().mmvae_last_error_string()
    assert N.lib().mmvae_last_error_string()


def test_python_wrapper_has_no_cpu_fallback():
    import torch
    with pytest.raises(N.NativeError):
        N.state_corr(torch.zeros(5, 3), torch.zeros(5, 2))
    with pytest.raises(N.NativeError):
        N.state_corr(torch.zeros(5, 3), torch.zeros(5, 2), rows=torch.arange(5))


# ---- 5. the public module ---------------------------------------------------------------------------------------------------
def test_public_module_imports_without_scipy_or_pandas():
    code = ("import sys\n"
            "class Block:\n"
            "    def find_spec(self, name, path=None, target=None):\n"
            "        if name.split('.')[0] in ('scipy', 'pandas', 'sklearn'):\n"
            "            raise ImportError(name + ' is blocked')\n"
            "sys.meta_path.insert(0, Block())\n"
            f"sys.path.insert(0, {ROOT!r})\n"
            "import distributed_vae_amd\n"
            "from distributed_vae_amd.utils import tree_based_analysis as TA\n"
            "from distributed_vae_amd.cpl_mixvae import cpl_mixVAE\n"
            "assert callable(TA.corr_analysis) and callable(cpl_mixVAE.state_gene_corr)\n"
            "assert not hasattr(TA, 'get_merged_types') and 'get_merged_types' in TA.__doc__\n"
            "assert not any(m.split('.')[0] in ('scipy', 'pandas', 'sklearn') for m in sys.modules)\n"
            "print('ok')\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr
    from distributed_vae_amd.utils import tree_based_analysis as TA
    assert not re.search(r"^(import|from)\s+(scipy|pandas|sklearn)", open(TA.__file__).read(), flags=re.M)


def test_refusals_of_the_public_function():
    """Every refusal comes before any device work: these run without a GPU."""
    from distributed_vae_amd.utils import tree_based_analysis as TA
    rng = np.random.default_rng(0)
    state, cell = rng.normal(size=(6, 2)), rng.normal(size=(6, 3))
    with pytest.raises(ValueError, match="6 states for 5 cells"):
        TA.corr_analysis(state, cell[:5])
    with pytest.raises(ValueError, match="groups"):
        TA.corr_analysis(state, cell, groups=[0, 1, 0])
    with pytest.raises(ValueError, match="rows"):
        TA.corr_analysis(state, cell, rows=[0, 1, 2])
    with pytest.raises(ValueError, match="rows"):
        TA.corr_analysis(state, cell, rows=np.arange(6.0))
    with pytest.raises(IndexError):
        TA.corr_analysis(state, cell, rows=[0, 1, 2, 3, 4, 6])
    with pytest.raises(IndexError):
        TA.corr_analysis(state, cell, rows=[0, 1, 2, 3, 4, -1])
    for bad in (np.nan, np.inf):
        broken = cell.copy()
        broken[2, 1] = bad
        with pytest.raises(ValueError, match="NaN"):
            TA.corr_analysis(state, broken)
    with pytest.raises(ValueError, match="2-D"):
        TA.corr_analysis(state, cell[:, 0])

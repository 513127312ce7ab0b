"""CPU (no GPU): the host restatement of the noise contract (tests/noise_restatement.py) against Random123's known answers,
the field-width / threshold table of the input mask, and the counter layout's disjointness by enumeration.  Exact values
only: tests/test_gpu_noise.py then holds the device to this restatement bit for bit, which replaces any statistical check."""
from collections import Counter

import numpy as np
import pytest

from tests import noise_restatement as NR

# Random123 kat_vectors, philox4x32 10 rounds: (counter, key, output) -- the vectors of tests/test_host_cpu.py
KAT = [
    ([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
    ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
    ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0], [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]),
]


def test_restatement_reproduces_random123_vectors():
    for ctr, key, want in KAT:
        assert NR.philox4x32_10(ctr, key).tolist() == want
    # vectorised: a batch of counters under one key equals the calls one by one
    ctrs = np.array([[i, 7 * i, 0xFFFFFFFF - i, 1 << (i % 32)] for i in range(33)], dtype=np.uint64)
    got = NR.philox4x32_10(ctrs, KAT[2][1])
    assert got.shape == (33, 4) and got.dtype == np.uint32
    for i in range(33):
        assert got[i].tolist() == NR.philox4x32_10(ctrs[i], KAT[2][1]).tolist()


def test_key_and_step_words():
    assert NR.key_of(0x5EED0123456789) == (0x23456789, 0x005EED01)
    assert NR.key_of(2 ** 64 - 1) == (0xFFFFFFFF, 0xFFFFFFFF) and NR.key_of(2 ** 32) == (0, 1)
    assert NR.step_words(0, 0, 5) == (0, 5)
    assert NR.step_words(2, 3, 2 ** 32 + 5) == (11 ^ (1 << 8), 5)
    assert NR.step_words(7, 3, 2 ** 40) == (31 ^ (256 << 8), 0)


@pytest.mark.parametrize("p,m,x_thr", [(0.5, 1, 1), (0.25, 2, 3), (0.8125, 4, 3), (0.98828125, 8, 3), (0.3, 16, 45875),
                                        (0.0, 1, 2), (1.0, 1, 0),
                                        (1.0 - 2.0 ** -16, 16, 1),      # the finest keep probability: one value of 65536
                                        (2.0 ** -16, 16, 65535)])
def test_field_width_and_threshold_table(p, m, x_thr):
    assert NR.xmask_field(p)[:2] == (m, x_thr)
    # the field width is the smallest that holds the threshold, and the keep probability it realises is t16 / 65536
    _, thr, t16 = NR.xmask_field(p)
    assert thr << (16 - m) == t16 and (m == 1 or t16 % (1 << (16 - m // 2)) != 0)


def test_thresholds_take_the_float32_probability():
    # (0.3 is not a float32 either, but both its values give t16 = 45875.)  The float32 nearest to this p is
    # 0.7000045776367188 = 1 - 19660.5 / 65536, exactly on the rounding boundary: the double gives t16 = 19660, the float32
    # the library receives 19661
    p = 1.0 - 19660.4999999 / 65536.0
    assert float(np.float32(p)) != p
    t_double = int((1.0 - p) * 65536.0 + 0.5)
    t_float = int((1.0 - float(np.float32(p))) * 65536.0 + 0.5)
    assert t_double != t_float
    assert NR.xmask_field(p)[2] == t_float
    # state mask: thr32 = floor((1 - float32(p)) 2^32), saturated at both ends
    assert NR.state_keep_threshold(0.0) == 0xFFFFFFFF and NR.state_keep_threshold(1.0) == 0
    assert NR.state_keep_threshold(0.25) == 0xC0000000
    assert NR.state_keep_threshold(0.2) == int((1.0 - float(np.float32(0.2))) * 2.0 ** 32) != int(0.8 * 2.0 ** 32)
    assert NR.state_keep_threshold(2.0 ** -33) == 0xFFFFFFFF          # (1 - p) 2^32 >= 2^32 - 1: keep all
    assert NR.state_keep_threshold(2.0 ** -24) == 2 ** 32 - 256
    w = np.array([0, 0xBFFFFFFF, 0xC0000000, 0xFFFFFFFF], dtype=np.uint32)
    assert NR.state_keep(w, 0xC0000000).tolist() == [True, True, False, False]
    assert NR.state_keep(w, 0xFFFFFFFF).all() and not NR.state_keep(w, 0).any()
    d = NR.dump_noise(2, 5, 8, 3, 3, 0.0, 0.0, 9, 1)
    assert d["x_mask"].all() and d["s_mask"].all()
    d = NR.dump_noise(2, 5, 8, 3, 3, 1.0, 1.0, 9, 1)
    assert not d["x_mask"].any() and not d["s_mask"].any()


def test_uniform_is_the_top_24_bits():
    w = np.array([0, 0xFF, 0x100, 0x80000000, 0xFFFFFFFF], dtype=np.uint32)
    u = NR.u01(w)
    assert u.dtype == np.float32
    assert u.tolist() == [0.0, 0.0, 2.0 ** -24, 0.5, 1.0 - 2.0 ** -24]


def test_elements_take_their_word_of_their_group():
    """Element idx of a stream is word idx & 3 of the call whose counter is idx >> 2; element (row, col) of the mask is field
    col % (128 / m) of the call (col // (128 / m), row) -- spelled out one element at a time against the vectorised form."""
    seed, offset, arm = 0x5EED0123456789, 2 ** 32 + 5, 2
    key = NR.key_of(seed)
    words = NR.stream_words(arm, NR.KIND_GUMBEL, 23, seed, offset)
    for idx in (0, 1, 3, 4, 6, 21, 22):
        w2, w3 = NR.step_words(arm, NR.KIND_GUMBEL, offset)
        assert int(words[idx]) == int(NR.philox4x32_10([idx >> 2, 0, w2, w3], key)[idx & 3])
    B, D = 3, 70
    for p in (0.5, 0.25, 0.8125, 0.98828125, 0.3):
        m, thr, _ = NR.xmask_field(p)
        mask = NR.xmask(arm, B, D, p, seed, offset)
        assert mask.shape == (B, D) and mask.dtype == np.uint8
        w2, w3 = NR.step_words(arm, NR.KIND_XMASK, offset)
        epg = 128 // m
        for row, col in ((0, 0), (1, 31), (2, 32), (0, 63), (1, 64), (2, 69), (0, min(epg, D) - 1), (1, min(epg, D - 1))):
            out = NR.philox4x32_10([col // epg, row, w2, w3], key).tolist()
            big = out[0] | out[1] << 32 | out[2] << 64 | out[3] << 96
            field = (big >> ((col % epg) * m)) & ((1 << m) - 1)
            assert int(mask[row, col]) == int(field < thr), (p, row, col)


def test_state_changes_draws_are_the_state_stream_by_sample_then_cell():
    seed, offset = 77, 9
    u = NR.state_changes_draws(3, 7, 5, seed, offset)
    assert u.shape == (3, 7, 5) and u.dtype == np.float32
    for a in range(3):
        flat = NR.u01(NR.stream_words(a, NR.KIND_STATE, 35, seed, offset))
        assert np.array_equal(u[a].reshape(-1), flat)
    # the same stream as forward's state uniforms of that step: a traversal at an offset of its own shares nothing with a step
    d = NR.dump_noise(3, 5, 4, 2, 7, 0.5, 0.2, seed, offset)
    assert np.array_equal(d["u_state"].reshape(3, -1), u.reshape(3, -1))


OFFSETS = (1, 2, 2 ** 32, 2 ** 32 + 1)


@pytest.mark.parametrize("m,p", [(1, 0.5), (2, 0.25), (4, 0.8125), (8, 0.98828125), (16, 0.3)])
def test_counters_are_disjoint_over_kinds_arms_and_steps(m, p):
    """Every Philox call of four steps -- all four kinds, eight arms -- has a 128-bit counter of its own, so no two draws under
    one key share an output.  The layout guarantees this while arm * 4 + kind < 256 and step_hi < 2^24: `step_hi << 8` then
    neither leaves the word nor meets the stream bits, and (words 2, 3) identify (arm, kind, step) uniquely; past either
    limit two steps or two streams can meet (the second half of the test shows one such meeting)."""
    A, B, D, C, S = 8, 5, 150, 9, 3
    assert NR.xmask_field(p)[0] == m
    seen = Counter()
    n_calls = 0
    for offset in OFFSETS:
        for a in range(A):
            sets = [NR.xmask_counters(a, B, D, m, offset).reshape(-1, 4),
                    NR.stream_counters(a, NR.KIND_GUMBEL, B * C, offset),
                    NR.stream_counters(a, NR.KIND_STATE, B * S, offset),
                    NR.stream_counters(a, NR.KIND_SMASK, B * S, offset)]
            for c in sets:
                assert c.dtype == np.uint64 and int(c.max()) < 2 ** 32
                seen.update(map(tuple, c.tolist()))
                n_calls += len(c)
    groups = -(-D // (128 // m))
    assert n_calls == len(OFFSETS) * A * (B * groups + -(-B * C // 4) + 2 * -(-B * S // 4))
    assert len(seen) == n_calls and max(seen.values()) == 1
    # where the guarantee ends: step_hi = 2^24 shifts out of the word, so offset 2^56 + k draws what offset k draws
    assert NR.step_words(1, 2, 2 ** 56 + 3) == NR.step_words(1, 2, 3)
    # ... and a stream id of 256 (arm 64) would meet step_hi = 1 of stream 0
    assert NR.step_words(64, 0, 5) == NR.step_words(0, 0, 2 ** 32 + 5)
    assert NR.step_words(7, 3, 5) != NR.step_words(0, 0, 2 ** 32 + 5)

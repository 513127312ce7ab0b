"""Host restatement of the in-kernel noise contract (numpy only): what a kernel in Philox mode (mmvae_noise.mode == 1) must
draw, written from the contract's text -- the comments of csrc/common.hpp ("Philox4x32-10" .. make_xbits_range) and
make_noise_dev (csrc/rowwise.hip) -- in vectorised uint64 arithmetic, not from the device functions.

The contract:

  * Philox4x32-10 (Salmon et al., Random123), key = (seed low word, seed high word), step words = (offset low word,
    offset high word).  Every counter carries the step in words 2 and 3: word 3 = step_lo, word 2 = stream ^ (step_hi << 8)
    with stream = arm * 4 + kind, kind 0 the input mask, 1 the Gumbel uniforms, 2 the state uniforms, 3 the state mask.
  * Uniforms and the state mask: element idx of stream (arm, kind) is word idx & 3 of the call with counter words 0, 1 =
    the low and high word of g = idx >> 2.  idx = b * C + col (Gumbel), b * S + s (state uniforms and mask), samp * B + b
    (the traversal's state draws in state_changes).  u = (w >> 8) * 2^-24; state keep iff w < thr32,
    thr32 = floor((1 - p) * 2^32) saturated: >= 2^32 - 1 is 0xFFFFFFFF and means keep all, <= 0 is 0 (keep none).
  * Input mask: t16 = floor((1 - float32(p)) * 65536 + 0.5) clamped to [0, 65536]; a gene takes m in {1, 2, 4, 8, 16} random
    bits, the smallest m with t16 a multiple of 2^(16 - m), and is kept iff its m-bit field < x_thr = t16 >> (16 - m).  One call
    serves genes [cg * 128 / m, (cg + 1) * 128 / m) of a row: counter words 0, 1 = (cg, row); element i of the group owns
    bits [i m, (i + 1) m) of the 128-bit output, word 0 lowest.

The layout keeps the streams of one step and of different steps apart while arm * 4 + kind < 256 (A <= 64; the library
allows 8 arms) and step_hi < 2^24 (offset < 2^56): past either, `step_hi << 8` leaves the word or meets the stream bits.

The dropout probabilities reach the library as float32 (mmvae_hyper), so both thresholds are taken of float32(p).
"""
import numpy as np

KIND_XMASK, KIND_GUMBEL, KIND_STATE, KIND_SMASK = 0, 1, 2, 3
_LO = np.uint64(0xFFFFFFFF)
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)         # the two round multipliers
_W0, _W1 = 0x9E3779B9, 0xBB67AE85                                # the key schedule's Weyl increments


def philox4x32_10(counter, key):
    """counter: integer array [..., 4] of 32-bit words, key: two 32-bit words.  Returns uint32 [..., 4]."""
    c = np.atleast_2d(np.asarray(counter)).astype(np.uint64) & _LO
    c0, c1, c2, c3 = c[..., 0], c[..., 1], c[..., 2], c[..., 3]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2                              # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & _LO, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & _LO
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    out = np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)
    return out.reshape(np.shape(counter))


def key_of(seed):
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return seed & 0xFFFFFFFF, seed >> 32


def step_words(arm, kind, offset):
    """Counter words (2, 3) of stream (arm, kind) at step `offset`."""
    offset = int(offset) & 0xFFFFFFFFFFFFFFFF
    step_lo, step_hi = offset & 0xFFFFFFFF, offset >> 32
    return ((arm * 4 + kind) ^ ((step_hi << 8) & 0xFFFFFFFF)), step_lo


def stream_counters(arm, kind, n, offset):
    """The counters [ceil(n / 4), 4] that serve elements 0 .. n - 1 of a uniform / state-mask stream."""
    g = np.arange((n + 3) // 4, dtype=np.uint64)
    w2, w3 = step_words(arm, kind, offset)
    return np.stack([g & _LO, g >> np.uint64(32), np.full_like(g, w2), np.full_like(g, w3)], axis=-1)


def stream_words(arm, kind, n, seed, offset):
    """uint32 [n]: the random word of each element of the stream (element idx: word idx & 3 of group idx >> 2)."""
    return philox4x32_10(stream_counters(arm, kind, n, offset), key_of(seed)).reshape(-1)[:n]


def u01(w):
    """float32 in [0, 1): the top 24 bits of the word."""
    return (np.asarray(w, dtype=np.uint32) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def state_keep_threshold(p):
    k = (1.0 - float(np.float32(p))) * 4294967296.0
    if k >= 4294967295.0:
        return 0xFFFFFFFF
    return 0 if k <= 0.0 else int(k)


def state_keep(w, thr32):
    w = np.asarray(w, dtype=np.uint32)
    return np.ones(w.shape, dtype=bool) if thr32 == 0xFFFFFFFF else w < np.uint32(thr32)


def xmask_field(p):
    """(m, x_thr, t16) of input-dropout probability p."""
    k = (1.0 - float(np.float32(p))) * 65536.0 + 0.5
    t16 = 65536 if k >= 65536.0 else (0 if k <= 0.0 else int(k))
    m = next(m for m in (1, 2, 4, 8, 16) if t16 % (1 << (16 - m)) == 0)
    return m, t16 >> (16 - m), t16


def xmask_counters(arm, B, D, m, offset):
    """The counters [B, ceil(D / (128 / m)), 4] of arm `arm`'s input mask: (gene group, row, stream ^ step, step)."""
    epg = 128 // m
    cg, row = np.meshgrid(np.arange((D + epg - 1) // epg, dtype=np.uint64), np.arange(B, dtype=np.uint64))
    w2, w3 = step_words(arm, KIND_XMASK, offset)
    return np.stack([cg, row, np.full_like(cg, w2), np.full_like(cg, w3)], axis=-1)


def xmask(arm, B, D, p, seed, offset):
    """uint8 [B, D]: the keep-mask of arm `arm`."""
    m, x_thr, _ = xmask_field(p)
    w = philox4x32_10(xmask_counters(arm, B, D, m, offset), key_of(seed)).astype(np.uint64)       # [B, groups, 4]
    # the 32 / m fields of a word, lowest bits first; words in order: element i sits at bit i * m of the 128
    shifts = (np.arange(32 // m, dtype=np.uint64) * np.uint64(m))
    fields = (w[..., None] >> shifts) & np.uint64((1 << m) - 1)                                   # [B, groups, 4, 32 / m]
    return (fields.reshape(B, -1)[:, :D] < np.uint64(x_thr)).astype(np.uint8)


def dump_noise(A, B, D, C, S, x_drop, s_drop, seed, offset):
    """The four arrays of Engine.dump_noise: x_mask uint8 [A, B, D], u_gumbel float32 [A, B, C], u_state float32 [A, B, S],
    s_mask uint8 [A, B, S]."""
    thr32 = state_keep_threshold(s_drop)
    return {
        "x_mask": np.stack([xmask(a, B, D, x_drop, seed, offset) for a in range(A)]),
        "u_gumbel": np.stack([u01(stream_words(a, KIND_GUMBEL, B * C, seed, offset)).reshape(B, C) for a in range(A)]),
        "u_state": np.stack([u01(stream_words(a, KIND_STATE, B * S, seed, offset)).reshape(B, S) for a in range(A)]),
        "s_mask": np.stack([state_keep(stream_words(a, KIND_SMASK, B * S, seed, offset), thr32).reshape(B, S)
                            for a in range(A)]).astype(np.uint8),
    }


def state_changes_draws(A, n_samp, B, seed, offset):
    """float32 [A, n_samp, B]: the uniforms of mixVAE_model.state_changes (element samp * B + b of the arm's state stream)."""
    return np.stack([u01(stream_words(a, KIND_STATE, n_samp * B, seed, offset)).reshape(n_samp, B) for a in range(A)])

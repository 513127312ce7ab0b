"""Shapes of the augmenter-training tests: (NZ, Z, D, n_dim, B).

The step's launch plan has no switch of its own: every product goes to the planes x planes engine, whose tile and K split
follow from (M, N, K).  What differs between the cases is therefore what the engine sees: products inside one tile with one or
two K steps (case 0: no K split possible), odd widths and a batch that is no multiple of 32 (case 1: dW's K = 70 is five K
steps, the first size at which the engine may split K), tile edges crossed by D/5 = 260 and B = 300 with a K = 300 that is no
multiple of 16 (case 2: split dW products), and a batch one past a 256-row tile (case 3).  Which tile and split a product gets is the
engine's model's choice; FORCED below runs every tile shape and several K splits at a small shape, whatever the model would choose."""

CASES = [
    (6, 3, 52, 20, 16),
    (5, 2, 260, 45, 70),
    (50, 10, 1300, 500, 300),
    (4, 2, 520, 40, 257),
]
SMALL = CASES[:2]
# Forced engine choices (MMVAE_AUG_TILE = tile + 10 x KS; tiles 1 .. 4 = 256 x 256, 256 x 128, 128 x 128, 160 x 256), applied to every
# product of a step at FORCED_CASE, whose row counts (70, 260, 52, 45, 9, 5, 2) all fit the 160-row tile's padding: each tile without
# a split, and splits of 2, 3 and 8 (parts without a K step, splits that do not divide the accumulator tiles evenly).
FORCED_CASE = CASES[1]
FORCED = [1, 2, 3, 4, 21, 32, 23, 84]
PRODUCTION = (50, 10, 5032, 500, 5000)
P_DROP = 0.5


def seeds(case):
    """(state_dict seed, data seed, noise seed) of a case.  The small cases' seeds are chosen so that no float64 pre-ReLU value of
    the step lies within 1e-4 of zero (tests/test_augtrain_cpu.py checks it): every implementation takes the same decisions."""
    NZ, Z, D, n_dim, B = case
    if case == CASES[0]:
        return 11 + D, 23 + B, 1
    if case == CASES[1]:
        return 1, 1, 36
    return 11 + D, 23 + B, 37 + NZ + B

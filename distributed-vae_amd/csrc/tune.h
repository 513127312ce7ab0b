// Private: indices of mmvae_exec.tune (include/mmvae.h) -- switches between LIVE code paths (other shapes or engines take them
// anyway) for A/B timing and test hooks.  0 = production behaviour for every one of them.  MMVAE_TUNE_ENGINE
// (17) is public and defined in mmvae.h.  The Python binding translates environment variables into these (_native.TUNE_ENV); the
// library itself reads none.  Switches whose experiment is settled are gone with their code (round 4: where dW11 forks, extra
// LDS for dW11, small-layer products on the side stream, the coupling behind the dW11 fork, the join behind the last reduction,
// recorded fork events, the fc11 tensors' reduction on the main stream, smaller forward chain blocks, one wave per cell in the
// latent kernels, the one-launch encoder chains: numbers in DESIGN.md appendix, code of the last in tools/experiments/), the
// hot kernels' timing ablations and cycle stamps (results in profiles/, code in tools/experiments/), and the engine and path
// selections no test or benchmark ran (DESIGN.md appendix names the commit that still holds them).  Their indices stay unused.
#pragma once
enum {
    MMVAE_TUNE_AUG_TILE = 3,       // augmenter GEMMs: fp32 matrix instruction: tile 11 12 21 22 (1 = 64, 2 = 128); planes x planes engine:
                                   // 1 / 2 / 3 = 256 x 256 / 256 x 128 / 128 x 128 (+ 10 KS: K split)
    MMVAE_TUNE_COUPLE_SIDE = 13,   // fused step, where the coupling terms run: 0 = as a role of the decoder chain's launch from four arms up
                                   // and on the side stream below (api.hip make_plan), 1 = side stream always, 3 = role always
    // 17 MMVAE_TUNE_ENGINE: public (mmvae.h)
    MMVAE_TUNE_BN_PARTIALS = 19,   // BatchNorm batch sums through per-workgroup partial arrays instead of the accumulators
    MMVAE_TUNE_CHAIN_FP32 = 21,    // fp32x3 engine: the chain kernels' own GEMMs stay on the fp32 matrix instruction
};

// extern "C" surface of libmmvae_hip.so (see include/mmvae.h) and the per-step launch sequence.
#include "common.hpp"
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

namespace mmvae {

static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// Split factors are chosen so that each large kernel's grid fills the chip's resident-workgroup
// slots once (256 CUs x workgroups per CU that its registers / LDS admit) without spilling into a
// second, mostly empty round: e.g. 624 workgroups on 512 slots take two rounds, 468 take one.
Splits default_splits(const mmvae_dims& d, const mmvae_exec* ex) {
    int g_split[6] = {0, 0, 0, 0, 0, 0};
    if (ex) for (int i = 0; i < 6; ++i) g_split[i] = ex->split[i] > 0 && ex->split[i] <= 64 ? ex->split[i] : 0;
    constexpr int CUS = 256;
    // smallest split whose grid fills whole rounds of the resident slots to >= 93 % (else the best-filling one); an exact
    // fill one or two steps further is preferred.  With A = 5 a single round would leave a fifth of the chip idle (200 k
    // workgroups on 512 slots: k = 2 -> 78 %, k = 5 -> 98 % in two rounds; fc1 64 -> 53 us per arm); 720 workgroups on
    // 768 slots measured 12 % slower than 768 (small-layer dW GEMMs).
    auto fit = [](int base_blocks, int slots, int cap) {
        const int base = base_blocks > 0 ? base_blocks : 1;
        auto eff = [&](int k) { const int n = base * k; return (double)n / (double)(((n + slots - 1) / slots) * slots); };
        int pick = 1;
        double best = 0.0;
        for (int k = 1; k <= cap; ++k) {
            if (eff(k) >= 0.93) { pick = k; break; }
            if (eff(k) > best + 1e-9) { best = eff(k); pick = k; }
        }
        for (int k = pick + 1; k <= cap && k <= pick + 2; ++k)
            if (eff(k) >= 0.995) return k;
        return pick;
    };
    Splits s;
    const int nb128 = cdiv(d.B, 128), nb64 = cdiv(d.B, 64);
    const bool fastdims = fast_dims(d);
    // fc1 forward: fast kernel 128-row blocks, 3 workgroups / CU; general kernel 64-row blocks
    // (fc_dim 100: k_fc1_fwd_v3, two workgroups / CU)
    s.ks_fc1 = g_split[0] > 0 ? g_split[0] : (fastdims ? fit(nb128 * d.A, (d.H == 100 ? 2 : 3) * CUS, 16) : fit(nb64 * d.A, 4 * CUS, 16));
    s.ks_fc1 = min(s.ks_fc1, max(1, cdiv(d.D, 32)));
    // fc11 x_rec/loss/dZ11 kernel: 128-row blocks, 2 workgroups / CU (general fused kernel: 64-row blocks)
    s.ns_fc11 = g_split[1] > 0 ? g_split[1] : (fastdims ? fit(nb128 * d.A, 2 * CUS, 16) : fit(nb64 * d.A, 2 * CUS, 16));
    s.ns_fc11 = min(s.ns_fc11, max(1, cdiv(d.D, 64)));
    // dW1 / dW11: 128-gene tiles, 4 workgroups / CU
    s.ks_dw = g_split[2] > 0 ? g_split[2] : fit(cdiv(d.D, fastdims ? 128 : 64) * d.A, 4 * CUS, 16);
    s.ks_dw = min(s.ks_dw, max(1, cdiv(d.B, 32)));
    // dW11 runs on the side stream beside the latency-bound backward chain, which hides it: fewer, longer
    // workgroups (about 1.6 per CU) cost nothing there and halve the slabs the reduction has to read
    s.ks_dw11 = g_split[5] > 0 ? g_split[5] : fit(cdiv(d.D, 128) * d.A, 13 * CUS / 8, 16);
    s.ks_dw11 = min(s.ks_dw11, max(1, cdiv(d.B, 32)));
    if (!fastdims) s.ks_dw11 = s.ks_dw;
    s.ks_small = g_split[3] > 0 ? g_split[3] : fit(N_SMALL * d.A, 3 * CUS, 32);   // 3 workgroups / CU (136 VGPRs)
    s.ks_small = min(s.ks_small, max(1, cdiv(d.B, 32)));
    s.ks_gd10 = g_split[4] > 0 ? g_split[4] : fit(nb128 * d.A, (fastdims && d.H == 100 ? 2 : 3) * CUS, 16);   // fc_dim 100: k_gd10_v3, 2 / CU
    if (g_split[4] <= 0 && fastdims && d.H == 100) {
        // this is also k_fc11_zg's gene split, and that kernel fits one 256-cell workgroup per CU (152 KB of LDS): take
        // the smallest split whose grid fills whole rounds of the chip (A = 5: 2 -> 5, 200 -> 500 workgroups,
        // 609 -> 529 us; A = 2 keeps 6)
        const int wg = cdiv(d.B, 256) * d.A;
        int best = s.ks_gd10;
        double best_eff = 0.0;
        for (int ks = 1; ks <= 16; ++ks) {
            const int n = wg * ks;
            const double eff = (double)n / (double)(cdiv(n, CUS) * CUS);
            if (eff > best_eff + 0.02) { best_eff = eff; best = ks; }
            if (eff >= 0.93) { best = ks; break; }
        }
        s.ks_gd10 = best;
    }
    s.ks_gd10 = min(s.ks_gd10, max(1, cdiv(d.D, fastdims && d.H == 100 ? 64 : 32)));   // fc_dim 100: also k_fc11_zg's gene split
    // fp32x3 engine (gemm_bf16.hip): its kernels run ONE 512- or 256-thread workgroup per CU -- a pair of 128-row tiles
    // (fc1, dW1, dW11) or 128 cells (the fused fc11 kernel) -- so the splits fill 256 slots, not 512.  dW11 runs beside the
    // latency-bound backward chain, which needs CUs of its own (measured at A = 2: 873 us per step with the splits above,
    // 836 with these).
    if (ex && ex->tune[MMVAE_TUNE_ENGINE] == 2 && fastdims && x3_fc11_fits(d)) {
        const int pairs_b = cdiv(nb128, 2), pairs_d = cdiv(cdiv(d.D, 128), 2);
        if (g_split[0] <= 0) s.ks_fc1 = min(fit(pairs_b * d.A, CUS, 16), max(1, cdiv(d.D, 32)));
        if (g_split[4] <= 0) s.ks_gd10 = min(fit(nb128 * d.A, CUS, 16), max(1, cdiv(d.D, 64)));
        if (g_split[2] <= 0) s.ks_dw = min(fit(pairs_d * d.A, CUS, 16), max(1, cdiv(d.B, 32)));
        // (dW11: at most three eighths of the CUs -- its 120 KB of LDS leave a CU no room for a chain workgroup, and the
        // backward chain's 79 A workgroups should still find a CU each in ONE round: A = 2, 3 batch splits 768 us, 2: 757)
        // (workgroup count nearest to 96: measured best at A = 2 (2 splits), A = 3 (2) and A = 5 (1) while the chain kernels
        // ran their own GEMMs on the fp32 matrix instruction.  With those on the split engine too (chain.hip, X3) the chain
        // is 40 us shorter and dW11 has to keep up: nearest to 140 -- A = 2: 4 splits 707 us per step, 3: 720, 2: 728,
        // 5: 722; A = 3: 2 splits 931, 3: 940; A = 5: 1 split 1527, 2: 1530)
        if (g_split[5] <= 0) {
            const int nwg = max(1, pairs_d * d.A);
            const bool chain_x3 = chain_planes_fit(d) && !ex->tune[MMVAE_TUNE_CHAIN_FP32];
            const int target = chain_x3 ? 140 : 3 * CUS / 8;
            s.ks_dw11 = min(max(1, (target + nwg / 2) / nwg), max(1, cdiv(d.B, 32)));
        }
        if (g_split[3] <= 0) s.ks_small = min(fit(cdiv(N_SMALL * d.A, 2), CUS, 32), max(1, cdiv(d.B, 32)));   // k_x3_small: a pair of products per block
    }
    // the bf16 configuration runs its small-layer gradient products on k_x3_small too
    if (ex && ex->tune[MMVAE_TUNE_ENGINE] == 1 && fastdims && bf16_tiles_fit(d)) {
        if (g_split[3] <= 0) s.ks_small = min(fit(cdiv(N_SMALL * d.A, 2), CUS, 32), max(1, cdiv(d.B, 32)));
        // dW11 beside the backward chain: about 160 of its two-per-CU workgroups (A = 2: 5 splits 701 us per step, 3: 688, 2: 680)
        if (g_split[5] <= 0) {
            const int nwg = max(1, cdiv(d.D, 128) * d.A);
            s.ks_dw11 = min(max(1, (5 * CUS / 8 + nwg / 2) / nwg), max(1, cdiv(d.B, 32)));
        }
    }
    return s;
}

POff make_poff(const mmvae_dims& d) {
    POff p{};
    const int64_t D = d.D, H = d.H, L = d.L, C = d.C, S = d.S;
    const int64_t sizes[MMVAE_N_PARAM_TENSORS] = {
        H * D, H, H * H, H, H * H, H, H * H, H, L * H, L, C * L, C, S * (L + C), S * (L + C), S, S,
        L * (C + S), L, H * L, H, H * H, H, H * H, H, H * H, H, D * H, D};
    int64_t off = 0;
    for (int t = 0; t < MMVAE_N_PARAM_TENSORS; ++t) {
        // fc_sigma.w directly follows fc_mu.w, fc_sigma.b directly follows fc_mu.b: the state head is
        // one [2S, L+C] matrix for the kernels
        if (t != 13 && t != 15) off = cdiv64(off, 4) * 4;
        p.o[t] = off;
        off += sizes[t];
    }
    p.per_arm = cdiv64(off, 64) * 64;
    const int64_t bn[MMVAE_N_BN] = {H, H, H, H, L, S};
    off = 0;
    for (int i = 0; i < MMVAE_N_BN; ++i) {
        p.bn_mean[i] = off; off += bn[i];
        p.bn_var[i] = off; off += bn[i];
    }
    p.bn_per_arm = off;
    return p;
}

Layout make_layout(const mmvae_dims& d, const mmvae_exec* ex) {
    Layout L{};
    const int64_t A = d.A, B = d.B, D = d.D, H = d.H, Ld = d.L, C = d.C, S = d.S;
    L.nblk32 = cdiv(d.B, 32);
    L.nblk64 = cdiv(d.B, 64);
    L.nblkc = cdiv(d.B, CHAIN_ROWS);
    // cells per workgroup of the forward chain launches.  Measured at A = 2, B = 5000 (round 3): 64 cells (158 workgroups) 0.693 ms per
    // step, 48 (210) 0.692, 40 (250: one per CU) 0.695, 32 (314) 0.753 -- a chain launch is a latency chain of fixed costs (statistics
    // read, weight planes, barriers, the exchange), not of per-row work, so smaller blocks on the idle CUs buy nothing.
    L.chain_rows_fwd = CHAIN_ROWS;
    L.nblkf = cdiv(d.B, CHAIN_ROWS);
    L.nblkl = cdiv(d.B, LAT_ROWS);
    L.sp = default_splits(d, ex);
    int64_t off = 0;
    auto take = [&](int64_t n) { const int64_t o = off; off += cdiv64(n, 64) * 64; return o; };
    const int64_t nb = L.nblk32;
    for (int i = 0; i < 5; ++i) {
        const int64_t W = (i == 4) ? Ld : H;
        L.R[i] = take(A * B * W);
        L.bn_mean[i] = take(A * W);
        L.bn_rstd[i] = take(A * W);
        L.bn_part[i] = take(A * nb * 2 * W);
    }
    L.XLOW = take(A * B * Ld); L.CPROB = take(A * B * C); L.CC = take(A * B * C); L.YSOFT = take(A * B * C);
    L.CSMP = take(A * B * C); L.Y = take(A * B * (Ld + C)); L.MS = take(A * B * 2 * S); L.MU = take(A * B * S);
    L.LV = take(A * B * S); L.SS = take(A * B * S); L.ZIN = take(A * B * (C + S));
    for (int i = 0; i < 5; ++i) L.Dk[i] = take(A * B * (i == 0 ? Ld : H));
    L.c_part = take(A * nb * 2 * C); L.c_mean = take(A * C); L.c_iv = take(A * C);
    L.lat_part = take(A * nb * 2);
    L.fc1_slab = take((int64_t)L.sp.ks_fc1 * A * B * NP);
    L.n11 = (L.nblk64 + 2) * (max(L.sp.ns_fc11, L.sp.ks_gd10) + 1) + cdiv(d.D, 64);
    L.fc11_part = take(A * (int64_t)L.n11 * 2);
    L.acc = take((int64_t)ACC_NSETS * A * ACC_SET_FLOATS);   // directly behind fc11_part: one zero fill at the start of a forward pass
    L.acc_end = off;                                        // (the backward sets are the last ones: one zero fill at the start of a backward pass)
    L.GD10_slab = take((int64_t)max(L.sp.ns_fc11, L.sp.ks_gd10) * A * B * H);
    L.DZ11 = take(A * B * D);
    L.couple_part = take(nb * 2);
    L.T_part = take(nb * A * C); L.T = take(A * C);
    for (int i = 1; i <= 10; ++i) L.DZ[i] = take(A * B * ((i == 5 || i == 6) ? Ld : H));
    L.GZIN = take(A * B * (C + S)); L.GMS = take(A * B * 2 * S); L.GZC = take(A * B * C);
    for (int i = 1; i <= 5; ++i) {
        const int64_t W = (i == 5) ? Ld : H;
        L.G[i] = take(A * B * W);
        L.bnb_part[i] = take(A * (i == 5 ? (nb > cdiv(B, LAT_ROWS_BWD) ? nb : (int64_t)cdiv(B, LAT_ROWS_BWD)) : nb) * 2 * W);   // layer 5: the latent backward's partials
        L.bnb_sum[i] = take(A * 2 * W);
    }
    L.dw1_slab = take((int64_t)L.sp.ks_dw * A * H * D);
    L.dw11_slab = take((int64_t)max(L.sp.ks_dw, L.sp.ks_dw11) * A * D * DW11_LD);
    L.small_slab = take((int64_t)L.sp.ks_small * A * N_SMALL * NP * SMALL_LD);
    L.xbits = take(A * B * cdiv(d.D, 32));
    {   // slice planes (bf16: two per float)
        const int64_t Dk = cdiv64(D, 32) * 32, Dr = cdiv64(D, 128) * 128, Br = cdiv64(B, 256) * 256;
        L.pl_w1 = take(A * 3 * 128 * Dk / 2);
        L.pl_w11 = take(A * 3 * Dr * 128 / 2);
        L.pl_dz1 = take(A * 3 * Br * 128 / 2);
        L.pl_d10 = take(A * 3 * Br * 128 / 2);
        L.pl_small = take(A * (int64_t)PL_SMALL_SLOTS * 3 * 128 * 128 / 2);
    }
    L.rowmap = take(B + MAP_PAD);
    L.total = off;
    return L;
}

static int check_dims(const mmvae_dims* d) {
    if (!d) { set_error("dims is null"); return MMVAE_E_BADARG; }
    if (d->A < 1 || d->B < 1 || d->D < 1 || d->H < 1 || d->L < 1 || d->C < 1 || d->S < 1) {
        set_error("non-positive dimension (A=%d B=%d D=%d H=%d L=%d C=%d S=%d)",
                  d->A, d->B, d->D, d->H, d->L, d->C, d->S);
        return MMVAE_E_BADARG;
    }
    if (d->A > MMVAE_MAX_ARMS || d->H > 128 || d->C > 128 || d->L > 64 || 2 * d->S > 64 || d->L + d->C > 255 ||
        d->C + d->S > 255) {
        set_error("unsupported shape: need A<=%d, fc_dim<=128, n_categories<=128, lowD_dim<=64, state_dim<=32, "
                  "lowD+C<=255, C+S<=255 (got A=%d H=%d C=%d L=%d S=%d)",
                  MMVAE_MAX_ARMS, d->A, d->H, d->C, d->L, d->S);
        return MMVAE_E_UNSUPPORTED;
    }
    return 0;
}

static int make_ctx(Ctx& c, const mmvae_dims* d, const mmvae_hyper* h, void* ws, size_t ws_bytes, mmvae_exec* ex,
                    void* stream) {
    if (int rc = check_dims(d)) return rc;
    if (!h || !ws) { set_error("null hyper / workspace"); return MMVAE_E_BADARG; }
    if (int rc = check_gemm_engine(h->gemm_bf16)) return rc;
    if (h->training && d->B < 2) {   // a one-cell batch has no batch statistics; eval mode (running statistics) takes it
        set_error("training mode needs B >= 2 for the batch statistics (got B=%d)", d->B);
        return MMVAE_E_BADARG;
    }
    // the fixed-point batch-sum accumulators (common.hpp acc_add) hold 2^12 addends of the largest magnitude per column
    // without a carry between their slots; the producer with the fewest cells per workgroup is the latent backward kernel
    if (h->training && cdiv(d->B, ACC_MIN_PRODUCER_ROWS) > ACC_MAX_ADDENDS) {
        set_error("training mode takes at most %d cells per batch and rank (got B=%d): capacity of the exact batch-sum accumulators",
                  ACC_MAX_ADDENDS * ACC_MIN_PRODUCER_ROWS, d->B);
        return MMVAE_E_UNSUPPORTED;
    }
    c.d = *d;
    c.h = *h;
    if (h->cat_mask[0] | h->cat_mask[1] | h->cat_mask[2] | h->cat_mask[3]) {
        // bits beyond n_categories are ignored; at least one category must be kept
        uint32_t any = 0;
        for (int k = 0; k < d->C; ++k) any |= (h->cat_mask[k >> 5] >> (k & 31)) & 1u;
        if (!any) { set_error("cat_mask keeps none of the %d categories", d->C); return MMVAE_E_BADARG; }
    }
    c.ex_out = ex;
    if (ex) c.ex = *ex; else memset(&c.ex, 0, sizeof(c.ex));
    if (c.ex.side_stream) {
        for (int i = 0; i < MMVAE_N_EVENTS; ++i)
            if (!c.ex.ev[i]) { set_error("mmvae_exec: side_stream is set but ev[%d] is null", i); return MMVAE_E_BADARG; }
        if (c.ex.side_stream == stream) { set_error("mmvae_exec: side_stream must differ from the call's stream"); return MMVAE_E_BADARG; }
    }
    c.lay = make_layout(*d, &c.ex);
    c.po = make_poff(*d);
    if ((size_t)c.lay.total * sizeof(float) > ws_bytes) {
        set_error("workspace too small: need %zu bytes, got %zu", (size_t)c.lay.total * sizeof(float), ws_bytes);
        return MMVAE_E_WORKSPACE;
    }
    if (reinterpret_cast<uintptr_t>(ws) & 255) { set_error("workspace must be 256-byte aligned"); return MMVAE_E_BADARG; }
    c.ws = reinterpret_cast<float*>(ws);
    c.stream = reinterpret_cast<hipStream_t>(stream);
    return 0;
}

static int check_noise(const Ctx& c, const mmvae_noise* nz) {
    if (!nz) { set_error("noise descriptor is null"); return MMVAE_E_BADARG; }
    if (nz->mode == 0) {
        if (c.dropout() && !nz->x_mask) { set_error("explicit noise: x_mask is null"); return MMVAE_E_BADARG; }
        if (!c.h.eval_flag && !nz->u_gumbel) { set_error("explicit noise: u_gumbel is null"); return MMVAE_E_BADARG; }
        if (!nz->u_state) { set_error("explicit noise: u_state is null"); return MMVAE_E_BADARG; }
        if (c.h.training && c.h.s_drop > 0.f && !nz->s_mask) { set_error("explicit noise: s_mask is null"); return MMVAE_E_BADARG; }
    } else if (nz->mode != 1) {
        set_error("noise mode must be 0 (explicit) or 1 (philox)");
        return MMVAE_E_BADARG;
    }
    if (c.h.x_drop < 0.f || c.h.x_drop >= 1.f || c.h.s_drop < 0.f || c.h.s_drop >= 1.f) {
        set_error("dropout probabilities must be in [0,1)");
        return MMVAE_E_BADARG;
    }
    return 0;
}

static inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// The call's plan (common.hpp).  c.x_rows / c.x16 are set before; fc11_grad: fc11 runs for gradients without x_rec.
static void make_plan(Ctx& c, CallKind kind, const float* params, const float* x, int64_t xs, bool fc11_grad = true) {
    const mmvae_dims& d = c.d;
    const mmvae_hyper& h = c.h;
    const Layout& L = c.lay;
    Plan& p = c.plan;
    p = Plan{};
    p.kind = kind;
    const bool step = kind == CALL_STEP || kind == CALL_STEP_ROWS || kind == CALL_ZINB_STEP;
    const bool fwd = step || kind == CALL_FORWARD || kind == CALL_CLASSIFY || kind == CALL_TRAVERSE || kind == CALL_ENCODE;
    const bool dropout = c.dropout(), side = c.side() != nullptr;
    p.fast = fast_dims(d) && al16(params) && al16(x) && (xs & 3) == 0 && d.H >= 4 && (int64_t)d.B * d.D < ((int64_t)1 << 30);
    // engines of the five D x H products (mmvae_hyper.gemm_bf16: 1 bf16 operands, 2 fp32x3)
    const bool bf16_tiles = (h.gemm_bf16 == 1 || h.gemm_bf16 == 2) && bf16_tiles_fit(d);
    const bool x3 = h.gemm_bf16 == 2 && bf16_tiles_fit(d);
    p.big = !p.fast ? GEMM_GENERAL : x3 ? GEMM_X3 : bf16_tiles ? GEMM_BF16 : GEMM_FP32;
    p.small_x3 = bf16_tiles;   // (the bf16 configuration's small layers stay fp32-grade; on either path)
    // fp32x3: the fused train-step form of fc11 has its own kernel, the other forms run the fp32 matrix-instruction kernels.
    // At fc_dim 100 d(d10) is folded into the fc11 kernel (k_fc11_zg), whose gene split count equals the d(d10) kernel's so
    // that the decoder backward sums the same number of slabs whichever forward ran
    const bool slots = fc11_slots_fit(L, d.B);
    if (!p.fast) p.fc11 = FC11_GENERAL;
    else if (p.big == GEMM_X3 && fc11_grad && x3_fc11_fits(d) && slots) p.fc11 = FC11_X3;
    else if (p.big == GEMM_BF16) p.fc11 = FC11_BF16;
    else if (fc11_grad && d.H == 100 && (int64_t)cdiv(d.B, 256) * L.sp.ks_gd10 <= L.n11) p.fc11 = FC11_ZG;
    else p.fc11 = FC11_ZT;
    // (the ZINB step: mmvae_zinb_step_grads' one array, written behind the fc11 launch as slab 0)
    p.gd10_slabs = kind == CALL_ZINB_STEP ? 1 : p.fast ? L.sp.ks_gd10 : L.sp.ns_fc11;
    p.dw11_slabs = p.fast ? L.sp.ks_dw11 : L.sp.ks_dw;
    // the chain kernels' own GEMMs on the fp32x3 engine (also in the bf16 configuration: only its five D x H products round
    // their operands, everything else stays fp32-grade)
    p.chain_planes = p.fast && bf16_tiles && chain_planes_fit(d) && !c.tune(MMVAE_TUNE_CHAIN_FP32);
    p.lat_half = d.C <= 32 * LH_CPL && d.L <= 32 && 2 * d.S <= 32;
    // bf16 configuration on bf16 storage (mmvae_train_step_rows(data_bf16)): the NARROW operands of fc1 / dW1 (W1, dZ1) are
    // read as bf16 too -- slice 0 of the planes the fp32x3 engine uses -- instead of fp32 rounded by every block tile
    p.narrow = h.gemm_bf16 == 1 && c.x16 != nullptr && bf16_tiles_fit(d) && (d.D & 7) == 0;
    p.presplit = fwd && p.fast && (x3 || p.chain_planes);
    p.bwd_small_planes = kind == CALL_BACKWARD && p.chain_planes;   // (the fused step's forward pass has left them in place)
    p.d10_planes = x3;                                   // (these two also off the fast path, where no kernel reads them)
    p.dz1_in_apply = (x3 || p.narrow) && (d.H & 1) == 0;
    if (fwd && h.training) p.zero = p.presplit && dropout ? ZERO_PRESPLIT : p.fast && dropout ? ZERO_XBITS : ZERO_MEMSET;
    // what the row-indexed kernels take: the head launch builds the row map, the fused fc11 kernel of the fp32x3 or bf16 engine
    p.rowmap = kind == CALL_STEP_ROWS && p.zero == ZERO_PRESPLIT && slots && (p.fc11 == FC11_X3 || p.fc11 == FC11_BF16);
    p.dz11_bf16 = p.rowmap && c.x16 != nullptr && p.fc11 == FC11_BF16;
    // dW11 depends only on dZ11 and d10 (both final after forward): it runs on the side stream beside the backward chain, forked at
    // the START of the backward pass -- the later it starts, the more of it lands on the MFMA-bound dW1 (measured again in round 4,
    // profiles/r04_dw11_placement_sweep.txt: behind the decoder chain + 30 us per step, behind the latent backward + 15, not
    // forked + 75; fewer or more workgroups than the default split + 5 .. 10).
    p.dw11_side = (step || kind == CALL_BACKWARD) && p.fast && side;
    // The fused step on the fast path: the coupling terms AND the T sums of the latent backward (which need nothing but the
    // coupling kernel's output) run on the side stream beside the decoder chain and fc11; the loss scalars (which need
    // fc11's partials) follow dW11 on the side stream -- no fork between fc11 and the backward pass.
    p.loss_on_side = step && p.fast && side;
    // The coupling terms as a role of the decoder chain's launch (k_chain_fwd_couple: fp32x3 form, accumulator sets, 2 .. 5
    // arms; C <= 128 by check_dims).  Measured (A/B/A/B per arm count on one box, ms per step, role against side stream):
    // A = 2 0.674 / 0.672, A = 3 0.901 / 0.896, A = 5 1.479 / 1.489 -- the two bubbles it removes from the main stream show
    // in a rocprofv3 trace (5 - 6 us each) but not in the un-profiled step at two and three arms, where the combined launch
    // is 3 us longer than the chain's own (its grid has a third row of workgroups); at five arms the chain's 395 workgroups
    // already run in two rounds and the role fills the second.  So: the role from four arms up, the side stream below
    // (MMVAE_TUNE_COUPLE_SIDE: 1 side stream always, 3 role always).
    const int cs = c.tune(MMVAE_TUNE_COUPLE_SIDE);
    const bool role = p.loss_on_side && c.use_acc() && p.chain_planes && d.A >= 2 && d.A <= 5 && cs != 1 && (d.A >= 4 || cs == 3);
    p.couple = step && side ? (role ? COUPLE_IN_DEC : COUPLE_SIDE) : COUPLE_INLINE;
    // fork events ride on the kernels in front of the forks (the latent forward, the fused fc11 kernel): a recorded event is
    // a barrier packet of its own, 6 - 7 us of idle main stream (round 3: 686 -> 681 us per step)
    p.lat_fork_rides = p.couple == COUPLE_SIDE && p.lat_half;
    p.fc11_fork_rides = p.loss_on_side && (p.fc11 == FC11_X3 || p.fc11 == FC11_BF16);
    if (kind == CALL_DECODE) {
        // decode (`x` is x_rec, which the fast kernels store sixteen bytes at a time): the decoder chain as in a forward pass,
        // then fc11 for x_rec alone -- on the slice planes (fp32x3 within k_x3_fc11g's 112 columns, bf16), else on the fp32
        // matrix-instruction kernels in their output-only form.  Its planes come from one k_presplit launch of their own.
        if (!p.fast) p.fc11 = FC11_GENERAL;
        else if (p.big == GEMM_X3 && x3_fc11_fits(d)) p.fc11 = FC11_OUT_X3;
        else if (p.big == GEMM_BF16) p.fc11 = FC11_OUT_BF16;
        else p.fc11 = FC11_ZT;
        p.d10_planes = p.fc11 == FC11_OUT_X3 || p.fc11 == FC11_OUT_BF16;
        p.dec_planes = p.d10_planes || p.chain_planes;
    }
}

// Train step with a side stream: the coupling kernel needs only the latent block's outputs and the loss scalars only the
// coupling and fc11 partials, so both run on the side stream -- the coupling beside the decoder chain and fc11, the
// finalisation beside the d(d10) GEMM or dW11 (Plan::couple, loss_on_side).
// rode: the event rode on the kernel in front of the fork (Plan::lat_fork_rides / fc11_fork_rides, launch_k) -- only the side
// stream's wait is left
static int fork_to_side(const Ctx& c, int ev, bool rode = false) {
    if ((!rode && hipEventRecord(c.ev(ev), c.stream) != hipSuccess) || hipStreamWaitEvent(c.side(), c.ev(ev), 0) != hipSuccess) {
        set_error("stream fork failed");
        return MMVAE_E_LAUNCH;
    }
    return 0;
}
static int record_on_side(const Ctx& c, int ev) {
    if (hipEventRecord(c.ev(ev), c.side()) != hipSuccess) { set_error("event record failed"); return MMVAE_E_LAUNCH; }
    return 0;
}
static int join_from_side(const Ctx& c, int ev) {
    if (hipStreamWaitEvent(c.stream, c.ev(ev), 0) != hipSuccess) { set_error("stream join failed"); return MMVAE_E_LAUNCH; }
    return 0;
}

// The one dispatch level: the drivers pick each product's kernel family from the plan, the launchers launch their own file's
// kernels.  The three D x H GEMMs of the fast path (GEMM_FP32, GEMM_BF16 or GEMM_X3; GEMM_GENERAL: launch_fc1_fwd with its
// epilogue, launch_dw_big for both gradients) -- fc1 writes slabs that launch_fc1_epi sums:
static int fc1_gemm(const Ctx& c, const float* params, const float* x, int64_t xs) {
    return c.plan.big == GEMM_FP32 ? launch_fc1_fwd_fp32(c, params, x, xs) : launch_fc1_fwd_bf16(c, params, x, xs);
}
static int dw1(const Ctx& c, const float* x, int64_t xs) {
    return c.plan.big == GEMM_FP32 ? launch_dw1_fp32(c, x, xs) : launch_dw1_bf16(c, x, xs);
}
static int dw11(const Ctx& c) { return c.plan.big == GEMM_FP32 ? launch_dw11_fp32(c) : launch_dw11_bf16(c); }
static int fc1_forward(const Ctx& c, const mmvae_noise* nz, const float* params, const float* x, int64_t xs) {
    if (c.plan.big == GEMM_GENERAL) return launch_fc1_fwd(c, nz, params, x, xs);
    if (int rc = fc1_gemm(c, params, x, xs)) return rc;
    return launch_fc1_epi(c, params);
}
// fc11's main launch: x_rec / loss / dZ11 (where Plan::fc11_fork_rides, EV_FORK rides on it)
static int fc11_main(const Ctx& c, const float* params, const float* x, int64_t xs, float* x_rec, int need_grad) {
    switch (c.plan.fc11) {
        case FC11_GENERAL: return launch_fc11_fused(c, params, x, xs, x_rec, need_grad);
        case FC11_ZG: return launch_fc11_zg(c, params, x, xs, x_rec, need_grad);
        case FC11_ZT: return launch_fc11_zt(c, params, x, xs, x_rec, need_grad);
        case FC11_BF16: return launch_fc11_bf16(c, params, x, xs, x_rec, need_grad);
        case FC11_X3: return launch_fc11_x3(c, params, x, xs);
        default: set_error("internal: plan names fc11 family %d", (int)c.plan.fc11); return MMVAE_E_LAUNCH;
    }
}
// d(d10) = dZ11 W11 where it is a launch of its own
static int fc11_gd10(const Ctx& c, const float* params, float* x_rec, int need_grad) {
    if (!need_grad) return 0;
    switch (c.plan.fc11) {
        case FC11_ZT: return launch_gd10_fp32(c, params);
        case FC11_BF16: return x_rec ? launch_gd10_bf16(c, params) : 0;   // (without x_rec k_bf16_fc11g has written it)
        default: return 0;                                                // FC11_GENERAL, FC11_ZG, FC11_X3: out of the main launch
    }
}

static int do_forward(const Ctx& c, const mmvae_noise* nz, const float* params, float* bn_running, int64_t* nbt,
                      const float* x, int64_t xs, float* x_rec, int need_grad, float* loss_out = nullptr,
                      int32_t* labels = nullptr, const EncOut* enc = nullptr) {
    const Plan& p = c.plan;
    int rc;
    if ((p.zero == ZERO_MEMSET || p.zero == ZERO_XBITS) && (rc = launch_forward_zero(c, nz))) return rc;
    // fp32x3 / chain planes: slice planes of W1, [W11 | b11], the small layers (+ keep-mask, zero fill, row map: Plan::zero)
    if (p.presplit && (rc = launch_x3_planes(c, params, true, nz))) return rc;
    if ((rc = fc1_forward(c, nz, params, x, xs))) return rc;
    // batch statistics are recombined by the kernel that consumes each BatchNorm (no finalize launches);
    // eval mode copies the running statistics into the workspace instead
    if ((rc = launch_bn_eval_stats(c, bn_running))) return rc;
    if (!c.h.training) {
        if ((rc = launch_chain_fwd_enc_eval(c, params))) return rc;
    } else {
        for (int layer = 2; layer <= 5; ++layer)
            if ((rc = launch_chain_fwd_enc(c, layer, params, bn_running, nbt))) return rc;
    }
    if (p.kind == CALL_ENCODE) return launch_lat_enc(c, nz, params, bn_running, nbt, *enc, labels);   // mmvae_encode ends here
    if ((rc = launch_lat_fwd(c, nz, params, bn_running, nbt, labels))) return rc;   // (Plan::lat_fork_rides: EV_LAT rides on it)
    if (p.kind == CALL_CLASSIFY || p.kind == CALL_TRAVERSE) return 0;   // labels / the traversal's encoder: no decoder, no fc11
    Ctx cs = c;
    cs.stream = c.side();
    if (p.couple == COUPLE_SIDE) {
        if ((rc = fork_to_side(c, EV_LAT, p.lat_fork_rides))) return rc;
        if ((rc = launch_couple(cs))) return rc;
        if (p.loss_on_side) {
            if ((rc = launch_loss_finalize(cs, loss_out, 1))) return rc;
            if ((rc = record_on_side(c, EV_COUPLE))) return rc;
        }
    }
    // (fp32x3: it writes the slice planes of [d10 | 1] for fc11, dW11; COUPLE_IN_DEC: the coupling terms too)
    if ((rc = launch_chain_fwd_dec(c, params))) return rc;
    if (p.couple == COUPLE_SIDE && !p.loss_on_side && (rc = record_on_side(c, EV_COUPLE))) return rc;
    // loss_on_side: dW11 starts as soon as fc11 has finished -- EV_FORK rides on the fused fc11 kernel
    if ((rc = fc11_main(c, params, x, xs, x_rec, need_grad))) return rc;
    return fc11_gd10(c, params, x_rec, need_grad);
}

// decode and the traversal's decoder half: ZIN from `zb`, the decoder chain (eval mode: it has no BatchNorm), fc11 for x_rec
static int do_decode(const Ctx& c, const float* params, ZinBuild zb, const mmvae_noise* nz, float* x_rec) {
    int rc;
    if (c.plan.dec_planes && (rc = launch_dec_planes(c, params))) return rc;
    zb.zin = c.ws + c.lay.ZIN;
    if ((rc = launch_zin_build(zb, nz, c.h, c.stream))) return rc;
    if ((rc = launch_chain_fwd_dec(c, params))) return rc;
    switch (c.plan.fc11) {
        case FC11_GENERAL: return launch_fc11_fused_out(c, params, x_rec);
        case FC11_ZT: return launch_fc11_zt_out(c, params, x_rec);
        case FC11_OUT_BF16: case FC11_OUT_X3: return launch_fc11_out_bf16(c, x_rec);
        default: set_error("internal: decode plan names fc11 family %d", (int)c.plan.fc11); return MMVAE_E_LAUNCH;
    }
}

static int do_loss(const Ctx& c, float* loss_out) {
    int rc;
    if ((rc = launch_couple(c))) return rc;
    return launch_loss_finalize(c, loss_out);
}

// Plan::loss_on_side: the loss scalars (into loss_out) are still to be computed (the T sums are already on the side
// stream, EV_COUPLE) -- behind dW11 on the side stream
static int do_backward(const Ctx& c, const mmvae_noise* nz, const float* params, const float* x, int64_t xs,
                       float grad_scale, float* grads, const AdamHost* adam = nullptr, float* loss_out = nullptr) {
    const Plan& p = c.plan;
    int rc;
    // the ZINB step: d(d10) and fc11's dW and db (already in `grads`) are mmvae_zinb_step_grads': no dW11 GEMM (off the fast
    // path launch_dw_big still forms its slabs beside dW1; nothing reads them), no reduction of it
    const bool zinb = p.kind == CALL_ZINB_STEP;
    // dW11 on the side stream (Plan::dw11_side)
    const bool early = p.dw11_side && !adam && c.ex.early_grad_event != nullptr;
    const bool side_red = p.dw11_side && adam;
    if (c.ex_out) c.ex_out->early_recorded = 0;
    Ctx cs = c;
    cs.stream = c.side();
    if (p.dw11_side) {
        if ((rc = fork_to_side(c, EV_FORK, p.fc11_fork_rides))) return rc;
        if ((rc = dw11(cs))) return rc;
        if (early) {
            // data parallel: fc11.weight / fc11.bias (47 % of the parameters) are final here; reduce their slabs now
            // and tell the caller, who starts their all-reduce beside the rest of backward
            if ((rc = launch_reduce_grads(cs, grads, grad_scale, nullptr, 1))) return rc;
            if (hipEventRecord(reinterpret_cast<hipEvent_t>(c.ex.early_grad_event), c.side()) != hipSuccess) {
                set_error("event record failed");
                return MMVAE_E_LAUNCH;
            }
            if (c.ex_out) c.ex_out->early_recorded = 1;
        }
        if (side_red) {
            // fused Adam: fc11.weight / fc11.bias (47 % of the parameters) are reduced and updated here, behind their GEMM on
            // the side stream -- nothing reads W11 again in this step, and the side stream is idle from here to the join
            if ((rc = launch_reduce_grads(cs, grads, grad_scale, adam, 1))) return rc;
        }
        if (p.loss_on_side && (rc = launch_loss_finalize(cs, loss_out, 2))) return rc;
        if ((rc = record_on_side(c, EV_JOIN))) return rc;
    }
    if (p.bwd_small_planes && (rc = launch_x3_planes(c, params, false))) return rc;
    if ((rc = launch_chain_bwd_dec(c, params))) return rc;
    // T (sum of G log c, from the loss finalisation) is first needed here
    if (p.loss_on_side && p.couple == COUPLE_SIDE && (rc = join_from_side(c, EV_COUPLE))) return rc;
    if ((rc = launch_lat_bwd(c, nz, params))) return rc;
    for (int layer = 5; layer >= 2; --layer)
        if ((rc = launch_chain_bwd_enc(c, layer, params))) return rc;
    if ((rc = launch_bn_bwd_apply1(c))) return rc;
    if (p.big == GEMM_GENERAL) {
        if ((rc = launch_dw_big(c, nz, x, xs))) return rc;
    } else {
        if ((rc = dw1(c, x, xs))) return rc;
        if (!p.dw11_side && !zinb && (rc = dw11(c))) return rc;
    }
    if ((rc = launch_dw_small(c))) return rc;
    if (p.dw11_side && (rc = join_from_side(c, EV_JOIN))) return rc;
    return launch_reduce_grads(c, grads, grad_scale, adam, zinb || early || side_red ? 2 : 3);
}

}  // namespace mmvae

using namespace mmvae;

extern "C" {

int mmvae_abi_version(void) { return 5; }
const char* mmvae_last_error_string(void) { return g_err; }
int mmvae_check_dims(const mmvae_dims* d) { return check_dims(d); }

int mmvae_param_layout(const mmvae_dims* d, mmvae_param_layout_t* out) {
    if (int rc = check_dims(d)) return rc;
    if (!out) { set_error("out is null"); return MMVAE_E_BADARG; }
    const POff p = make_poff(*d);
    const int64_t D = d->D, H = d->H, L = d->L, C = d->C, S = d->S;
    const int64_t rows[MMVAE_N_PARAM_TENSORS] = {H, H, H, H, H, H, H, H, L, L, C, C, S, S, S, S, L, L, H, H, H, H, H, H, H, H, D, D};
    const int64_t cols[MMVAE_N_PARAM_TENSORS] = {D, 1, H, 1, H, 1, H, 1, H, 1, L, 1, L + C, L + C, 1, 1, C + S, 1, L, 1, H, 1, H, 1, H, 1, H, 1};
    out->per_arm = p.per_arm;
    for (int t = 0; t < MMVAE_N_PARAM_TENSORS; ++t) { out->offset[t] = p.o[t]; out->rows[t] = rows[t]; out->cols[t] = cols[t]; }
    out->bn_per_arm = p.bn_per_arm;
    const int64_t bn[MMVAE_N_BN] = {H, H, H, H, L, S};
    for (int i = 0; i < MMVAE_N_BN; ++i) { out->bn_mean_offset[i] = p.bn_mean[i]; out->bn_var_offset[i] = p.bn_var[i]; out->bn_dim[i] = bn[i]; }
    return 0;
}

size_t mmvae_workspace_bytes(const mmvae_dims* d, const mmvae_exec* ex) {
    if (check_dims(d)) return 0;
    return (size_t)make_layout(*d, ex).total * sizeof(float);
}

int64_t mmvae_ws_offset(const mmvae_dims* d, const mmvae_exec* ex, int id) {
    if (check_dims(d)) return -1;
    const Layout L = make_layout(*d, ex);
    switch (id) {
        case MMVAE_WS_X_LOW: return L.XLOW;
        case MMVAE_WS_C_PROB: return L.CPROB;
        case MMVAE_WS_C: return L.CC;
        case MMVAE_WS_C_SMP: return L.CSMP;
        case MMVAE_WS_S_MEAN: return L.MU;
        case MMVAE_WS_S_LOGVAR: return L.LV;
        case MMVAE_WS_S_SMP: return L.SS;
        case MMVAE_WS_Y_SOFT: return L.YSOFT;
        case MMVAE_WS_R1: return L.R[0];
        case MMVAE_WS_R2: return L.R[1];
        case MMVAE_WS_R3: return L.R[2];
        case MMVAE_WS_R4: return L.R[3];
        case MMVAE_WS_R5: return L.R[4];
        case MMVAE_WS_D6: return L.Dk[0];
        case MMVAE_WS_D7: return L.Dk[1];
        case MMVAE_WS_D8: return L.Dk[2];
        case MMVAE_WS_D9: return L.Dk[3];
        case MMVAE_WS_D10: return L.Dk[4];
        case MMVAE_WS_ZIN: return L.ZIN;
        case MMVAE_WS_DZ11: return L.DZ11;
        case MMVAE_WS_DZ1: return L.DZ[1];
        case MMVAE_WS_GZIN: return L.GZIN;
        case MMVAE_WS_GZC: return L.GZC;
        case MMVAE_WS_G5: return L.G[5];
        case MMVAE_WS_BN_MEAN1: return L.bn_mean[0];
        case MMVAE_WS_GD10_SLAB: return L.GD10_slab;
        case MMVAE_WS_G1: case MMVAE_WS_G2: case MMVAE_WS_G3: case MMVAE_WS_G4: return L.G[1 + id - MMVAE_WS_G1];
        case MMVAE_WS_DZ2: case MMVAE_WS_DZ3: case MMVAE_WS_DZ4: case MMVAE_WS_DZ5: return L.DZ[2 + id - MMVAE_WS_DZ2];
        default: set_error("unknown workspace id %d", id); return -1;
    }
}

int mmvae_splits(const mmvae_dims* d, const mmvae_exec* ex, int32_t out[6]) {
    if (int rc = check_dims(d)) return rc;
    if (!out) { set_error("out is null"); return MMVAE_E_BADARG; }
    const Splits s = default_splits(*d, ex);
    out[0] = s.ks_fc1; out[1] = s.ns_fc11; out[2] = s.ks_dw; out[3] = s.ks_small; out[4] = s.ks_gd10; out[5] = s.ks_dw11;
    return 0;
}

int mmvae_forward(const mmvae_dims* d, const mmvae_hyper* h, const mmvae_noise* nz, const float* params,
                  float* bn_running, int64_t* nbt, const float* x, int64_t x_arm_stride, float* x_rec, int need_grad,
                  void* ws, size_t ws_bytes, mmvae_exec* ex, void* stream) {
    Ctx c;
    if (int rc = make_ctx(c, d, h, ws, ws_bytes, ex, stream)) return rc;
    if (!params || !x) { set_error("null params / x"); return MMVAE_E_BADARG; }
    if (int rc = check_noise(c, nz)) return rc;
    if (need_grad && !h->training) { set_error("need_grad requires training mode (batch statistics)"); return MMVAE_E_UNSUPPORTED; }
    make_plan(c, CALL_FORWARD, params, x, x_arm_stride, need_grad && !x_rec);
    return do_forward(c, nz, params, bn_running, nbt, x, x_arm_stride, x_rec, need_grad);
}

int mmvae_loss(const mmvae_dims* d, const mmvae_hyper* h, void* ws, size_t ws_bytes, float* loss_out, mmvae_exec* ex,
               void* stream) {
    Ctx c;
    if (int rc = make_ctx(c, d, h, ws, ws_bytes, ex, stream)) return rc;
    if (!loss_out) { set_error("loss_out is null"); return MMVAE_E_BADARG; }
    make_plan(c, CALL_LOSS, nullptr, nullptr, 0);
    return do_loss(c, loss_out);
}

int mmvae_backward(const mmvae_dims* d, const mmvae_hyper* h, const mmvae_noise* nz, const float* params,
                   const float* x, int64_t x_arm_stride, float grad_scale, void* ws, size_t ws_bytes, float* grads,
                   mmvae_exec* ex, void* stream) {
    Ctx c;
    if (int rc = make_ctx(c, d, h, ws, ws_bytes, ex, stream)) return rc;
    if (!params || !x || !grads) { set_error("null params / x / grads"); return MMVAE_E_BADARG; }
    if (int rc = check_noise(c, nz)) return rc;
    if (!h->training) { set_error("backward requires training mode"); return MMVAE_E_UNSUPPORTED; }
    make_plan(c, CALL_BACKWARD, params, x, x_arm_stride);
    return do_backward(c, nz, params, x, x_arm_stride, grad_scale, grads);
}

int mmvae_adam_step(int64_t n, float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t step,
                    float lr, float beta1, float beta2, float adam_eps, float weight_decay, int decoupled,
                    void* stream) {
    if (n <= 0 || !params || !grads || !exp_avg || !exp_avg_sq || step < 1) {
        set_error("adam: bad argument");
        return MMVAE_E_BADARG;
    }
    return launch_adam(n, params, grads, exp_avg, exp_avg_sq, step, lr, beta1, beta2, adam_eps, weight_decay, decoupled,
                       reinterpret_cast<hipStream_t>(stream));
}

static int train_step_impl(Ctx& c, const mmvae_hyper* h, const mmvae_noise* nz, float* params,
                           float* bn_running, int64_t* nbt, const float* x, int64_t x_arm_stride,
                           float* grads, float* loss_out, int do_adam, float* exp_avg, float* exp_avg_sq, int64_t step,
                           float lr, float beta1, float beta2, float adam_eps, float weight_decay, int decoupled) {
    if (!params || !x || !grads || !loss_out) { set_error("null params / x / grads / loss_out"); return MMVAE_E_BADARG; }
    if (int rc = check_noise(c, nz)) return rc;
    if (!h->training) { set_error("train_step requires training mode"); return MMVAE_E_UNSUPPORTED; }
    const Plan& p = c.plan;
    int rc;
    if ((rc = do_forward(c, nz, params, bn_running, nbt, x, x_arm_stride, nullptr, 1, loss_out))) return rc;
    if (p.couple == COUPLE_SIDE && !p.loss_on_side) {   // general path: coupling done on the side, finalise here
        if ((rc = join_from_side(c, EV_COUPLE))) return rc;
        if ((rc = launch_loss_finalize(c, loss_out))) return rc;
    } else if (p.couple == COUPLE_INLINE && (rc = do_loss(c, loss_out))) {
        return rc;
    }
    if (do_adam) {
        // the Adam update rides on the slab reduction (alignment gaps of the flat buffers hold zeros and
        // need no update)
        if (!exp_avg || !exp_avg_sq || step < 1) { set_error("adam state missing"); return MMVAE_E_BADARG; }
        const AdamHost ah{params, exp_avg, exp_avg_sq, step, lr, beta1, beta2, adam_eps, weight_decay, decoupled};
        return do_backward(c, nz, params, x, x_arm_stride, 1.f, grads, &ah, loss_out);
    }
    return do_backward(c, nz, params, x, x_arm_stride, 1.f, grads, nullptr, loss_out);
}

int mmvae_train_step(const mmvae_dims* d, const mmvae_hyper* h, const mmvae_noise* nz, float* params,
                     float* bn_running, int64_t* nbt, const float* x, int64_t x_arm_stride, void* ws, size_t ws_bytes,
                     float* grads, float* loss_out, int do_adam, float* exp_avg, float* exp_avg_sq, int64_t step,
                     float lr, float beta1, float beta2, float adam_eps, float weight_decay, int decoupled,
                     mmvae_exec* ex, void* stream) {
    Ctx c;
    if (int rc = make_ctx(c, d, h, ws, ws_bytes, ex, stream)) return rc;
    make_plan(c, CALL_STEP, params, x, x_arm_stride);
    return train_step_impl(c, h, nz, params, bn_running, nbt, x, x_arm_stride, grads, loss_out, do_adam, exp_avg, exp_avg_sq, step,
                           lr, beta1, beta2, adam_eps, weight_decay, decoupled);
}

int mmvae_train_step_rows(const mmvae_dims* d, const mmvae_hyper* h, const mmvae_noise* nz, float* params,
                          float* bn_running, int64_t* nbt, const float* data, const uint16_t* data_bf16, int64_t ld, int64_t n_rows,
                          const int64_t* rows, void* ws, size_t ws_bytes, float* grads, float* loss_out, int do_adam, float* exp_avg,
                          float* exp_avg_sq, int64_t step, float lr, float beta1, float beta2, float adam_eps,
                          float weight_decay, int decoupled, mmvae_exec* ex, void* stream) {
    Ctx c;
    if (int rc = make_ctx(c, d, h, ws, ws_bytes, ex, stream)) return rc;
    if (!data || !rows || n_rows < 1 || ld < d->D) { set_error("train_step_rows: null data / rows, n_rows < 1 or ld < D"); return MMVAE_E_BADARG; }
    // what the row-indexed kernels take: the fp32x3 engine's fused step (its head launch builds the row map), 16-byte rows,
    // a matrix within reach of 32-bit byte offsets.  Everything else: gather the batch (mmvae_gather_rows) and call
    // mmvae_train_step.
    if ((ld & 3) || (reinterpret_cast<uintptr_t>(data) & 15) || n_rows * ld >= ((int64_t)1 << 30)) {
        set_error("train_step_rows: needs ld %% 4 == 0, 16-byte aligned data and n_rows * ld < 2^30 floats");
        return MMVAE_E_UNSUPPORTED;
    }
    c.x_rows = rows;
    c.x_ld = ld;
    c.x_nrows = n_rows;
    c.x16 = data_bf16;
    make_plan(c, CALL_STEP_ROWS, params, data, 0);
    if (!c.plan.rowmap) {
        set_error("train_step_rows: only the fused training step of the fp32x3 / bf16 engines reads the batch through a row map");
        return MMVAE_E_UNSUPPORTED;
    }
    // bf16 storage: the bf16 engine reads x from the copy and keeps dZ11 as bf16
    if (data_bf16 && (c.plan.big != GEMM_BF16 || (d->D & 7) || (ld & 7) || (reinterpret_cast<uintptr_t>(data_bf16) & 15))) {
        set_error("train_step_rows: data_bf16 needs the bf16 engine, D %% 8 == 0, ld %% 8 == 0 and a 16-byte aligned copy");
        return MMVAE_E_UNSUPPORTED;
    }
    return train_step_impl(c, h, nz, params, bn_running, nbt, data, 0, grads, loss_out, do_adam, exp_avg, exp_avg_sq, step,
                           lr, beta1, beta2, adam_eps, weight_decay, decoupled);
}

// ---- training under the ZINB likelihood: every argument is checked before the first launch
int mmvae_zinb_head_layout(const mmvae_dims* d, mmvae_zinb_head_layout_t* out) {
    if (int rc = check_dims(d)) return rc;
    if (!out) { set_error("out is null"); return MMVAE_E_BADARG; }
    const int64_t D = d->D, H = d->H;
    out->offset[0] = 0;                 // fc11_p.weight [D, H]
    out->offset[1] = D * H;             // fc11_p.bias [D]
    out->offset[2] = D * H + D;         // fc11_r.weight [D, H]
    out->offset[3] = 2 * D * H + D;     // fc11_r.bias [D]
    out->per_arm = 2 * (D * H + D);
    return 0;
}

// the ZINB kernels' workspace: mmvae_zinb_step_grads' (one arm's at a time; mmvae_zinb_nll's fits into its head), then the cell
// sums double [A][B], the gene sums double [D] (one arm's at a time) and zinb_loss of every arm, double [A]
struct ZinbWs { size_t grads, total; };
static ZinbWs zinb_step_ws(const mmvae_dims& d) {
    ZinbWs z{};
    if (zb_tiles(d.B, d.D) == 0 || zg_tiles(d.B, d.D, 0) == 0) return z;
    z.grads = zs_ws_bytes(d.B, d.D, d.H, 0);
    if (!z.grads) return ZinbWs{};
    z.total = bytes_or_0((unsigned __int128)z.grads + 8 * ((unsigned __int128)d.A * d.B + d.D + d.A));
    return z;
}

size_t mmvae_zinb_step_workspace_bytes(const mmvae_dims* d, const mmvae_exec* ex) {
    (void)ex;                           // (no size of it depends on the execution context)
    if (check_dims(d)) return 0;
    return zinb_step_ws(*d).total;
}

static int check_zinb_ws(const char* who, const mmvae_dims* d, double zinb_eps, const void* zws, size_t zws_bytes, ZinbWs& z) {
    if (!(zinb_eps >= 0.0 && zinb_eps < 1.0)) { set_error("%s: zinb_eps = %g outside [0, 1)", who, zinb_eps); return MMVAE_E_BADARG; }
    if (!zws || (reinterpret_cast<uintptr_t>(zws) & 7)) { set_error("%s: zws is null or not 8-byte aligned", who); return MMVAE_E_BADARG; }
    z = zinb_step_ws(*d);
    if (!z.total) { set_error("%s: B = %d, D = %d need more tiles of 64 x 64 than a grid holds", who, d->B, d->D); return MMVAE_E_UNSUPPORTED; }
    if (zws_bytes < z.total) { set_error("%s: zws too small: need %zu bytes, got %zu", who, z.total, zws_bytes); return MMVAE_E_WORKSPACE; }
    return 0;
}

// one arm's inputs of the ZINB kernels: D10 of the workspace, the arm's rows of x, fc11 of params and the two heads of heads_pr
static ZinbIn zinb_arm(const Ctx& c, int a, const float* params, const float* heads_pr, const float* x, int64_t xs, double eps, double scale) {
    const int64_t D = c.d.D, H = c.d.H;
    const float* P = params + (int64_t)a * c.po.per_arm;
    const float* Q = heads_pr + (int64_t)a * 2 * (D * H + D);
    return ZinbIn{c.ws + c.lay.Dk[4] + (int64_t)a * c.d.B * H, H, c.d.B, c.d.H, c.d.D,
                  {{P + c.po.o[26], Q, Q + D * H + D}, {P + c.po.o[27], Q + D * H, Q + 2 * D * H + D}},
                  x + (int64_t)a * xs, D, eps, scale, 7, 0};
}

int mmvae_zinb_train_step(const mmvae_dims* d, const mmvae_hyper* h, const mmvae_noise* nz, float* params, float* heads_pr,
                          float* bn_running, int64_t* nbt, const float* x, int64_t x_arm_stride, double zinb_eps, void* ws,
                          size_t ws_bytes, void* zws, size_t zws_bytes, float* grads, float* head_grads, float* loss_out, int do_adam,
                          float* exp_avg, float* exp_avg_sq, float* hp_exp_avg, float* hp_exp_avg_sq, int64_t step, float lr,
                          float beta1, float beta2, float adam_eps, float weight_decay, int decoupled, mmvae_exec* ex, void* stream) {
    const char* who = "zinb_train_step";
    Ctx c;
    if (int rc = make_ctx(c, d, h, ws, ws_bytes, ex, stream)) return rc;
    if (!params || !heads_pr || !x || !grads || !head_grads || !loss_out) {
        set_error("%s: null params / heads_pr / x / grads / head_grads / loss_out", who);
        return MMVAE_E_BADARG;
    }
    if (x_arm_stride < 0) { set_error("%s: negative arm stride", who); return MMVAE_E_BADARG; }
    if (int rc = check_noise(c, nz)) return rc;
    if (!h->training) { set_error("%s requires training mode", who); return MMVAE_E_UNSUPPORTED; }
    if (h->gemm_bf16 == 1) { set_error("%s: the bf16 engine is not offered (gemm_bf16 = 1)", who); return MMVAE_E_UNSUPPORTED; }
    if (h->cat_mask[0] | h->cat_mask[1] | h->cat_mask[2] | h->cat_mask[3]) {
        set_error("%s: a category mask (pruning) is not offered in training", who);
        return MMVAE_E_UNSUPPORTED;
    }
    ZinbWs z;
    if (int rc = check_zinb_ws(who, d, zinb_eps, zws, zws_bytes, z)) return rc;
    if (do_adam && (!exp_avg || !exp_avg_sq || !hp_exp_avg || !hp_exp_avg_sq || step < 1)) {
        set_error("%s: adam state missing", who);
        return MMVAE_E_BADARG;
    }
    // one stream: the ZINB kernels fill the chip, and nothing of the step is left to run beside the backward chain
    c.ex.side_stream = nullptr;
    c.ex.early_grad_event = nullptr;
    make_plan(c, CALL_ZINB_STEP, params, x, x_arm_stride);
    const int A = d->A, D = d->D, H = d->H;
    const int64_t B = d->B;
    char* zb = static_cast<char*>(zws);
    double* cell = reinterpret_cast<double*>(zb + z.grads);
    double* gene = cell + (int64_t)A * B;
    double* zrec = gene + D;
    int rc;
    // 1. the MSE step's forward, fc11 included: its launch leaves the partials of sum (relu(a_rec) - x)^2 that ll[a] is made of
    //    (its dZ11 and d(d10) slabs are not read)
    if ((rc = do_forward(c, nz, params, bn_running, nbt, x, x_arm_stride, nullptr, 1, loss_out))) return rc;
    // 2., 3. per arm, one pass over g: the heads' gradients into grads (fc11) and head_grads, d(d10) into slab 0
    const double scale = (double)(A > 1 ? A - 1 : 1) / ((double)B * (double)D);
    const int64_t hp_per_arm = 2 * ((int64_t)D * H + D);
    for (int a = 0; a < A; ++a) {
        float* G = grads + (int64_t)a * c.po.per_arm;
        float* HG = head_grads + (int64_t)a * hp_per_arm;
        const ZinbGradOut out{{G + c.po.o[26], HG, HG + (int64_t)D * H + D}, {G + c.po.o[27], HG + (int64_t)D * H, HG + 2 * (int64_t)D * H + D},
                              cell + (int64_t)a * B, gene, c.ws + c.lay.GD10_slab + (int64_t)a * B * H, H};
        if ((rc = launch_zinb_head_grads(zinb_arm(c, a, params, heads_pr, x, x_arm_stride, zinb_eps, scale), zb, out, c.stream))) return rc;
    }
    if ((rc = launch_zinb_rec(cell, A, B, D, zrec, c.stream))) return rc;
    if ((rc = launch_couple(c))) return rc;
    if ((rc = launch_loss_finalize(c, loss_out, 0, zrec))) return rc;
    // 4. the rest of the backward pass from slab 0
    if ((rc = do_backward(c, nz, params, x, x_arm_stride, 1.f, grads, nullptr, loss_out))) return rc;
    if (!do_adam) return 0;
    // (the alignment gaps of the flat buffers hold zeros in the parameters, the gradients and the moments, and keep them)
    if ((rc = launch_adam((int64_t)A * c.po.per_arm, params, grads, exp_avg, exp_avg_sq, step, lr, beta1, beta2, adam_eps, weight_decay,
                          decoupled, c.stream)))
        return rc;
    return launch_adam((int64_t)A * hp_per_arm, heads_pr, head_grads, hp_exp_avg, hp_exp_avg_sq, step, lr, beta1, beta2, adam_eps,
                       weight_decay, decoupled, c.stream);
}

int mmvae_zinb_objective(const mmvae_dims* d, const mmvae_hyper* h, const float* params, const float* heads_pr, const float* x,
                         int64_t x_arm_stride, double zinb_eps, void* ws, size_t ws_bytes, void* zws, size_t zws_bytes,
                         float* loss_out, mmvae_exec* ex, void* stream) {
    const char* who = "zinb_objective";
    Ctx c;
    if (int rc = make_ctx(c, d, h, ws, ws_bytes, ex, stream)) return rc;
    if (!params || !heads_pr || !x || !loss_out) { set_error("%s: null params / heads_pr / x / loss_out", who); return MMVAE_E_BADARG; }
    if (x_arm_stride < 0) { set_error("%s: negative arm stride", who); return MMVAE_E_BADARG; }
    ZinbWs z;
    if (int rc = check_zinb_ws(who, d, zinb_eps, zws, zws_bytes, z)) return rc;
    make_plan(c, CALL_LOSS, nullptr, nullptr, 0);
    const int A = d->A, D = d->D;
    const int64_t B = d->B;
    char* zb = static_cast<char*>(zws);
    double* cell = reinterpret_cast<double*>(zb + z.grads);
    double* gene = cell + (int64_t)A * B;
    double* zrec = gene + D;
    int rc;
    for (int a = 0; a < A; ++a) {
        if ((rc = launch_zinb_nll(zinb_arm(c, a, params, heads_pr, x, x_arm_stride, zinb_eps, 0.0), zb, cell + (int64_t)a * B, gene, c.stream)))
            return rc;
    }
    if ((rc = launch_zinb_rec(cell, A, B, D, zrec, c.stream))) return rc;
    if ((rc = launch_couple(c))) return rc;
    return launch_loss_finalize(c, loss_out, 0, zrec);
}

int mmvae_eval_classify(const mmvae_dims* d, const mmvae_hyper* h, const float* params, const float* bn_running,
                        const float* x, int64_t x_arm_stride, void* ws, size_t ws_bytes, int32_t* labels,
                        int64_t* counts, mmvae_exec* ex, void* stream) {
    Ctx c;
    if (int rc = make_ctx(c, d, h, ws, ws_bytes, ex, stream)) return rc;
    if (!params || !x || !bn_running || !labels) { set_error("null params / x / bn_running / labels"); return MMVAE_E_BADARG; }
    if (h->training || !h->eval_flag) { set_error("eval_classify needs training = 0 and eval_flag = 1"); return MMVAE_E_UNSUPPORTED; }
    int rc;
    // eval mode reads the running statistics (nothing is written to bn_running) and draws no Gumbel noise; the state
    // sample the latent kernel also produces does not enter c: it takes the Philox stream of seed 0
    mmvae_noise nzp{};
    nzp.mode = 1;
    make_plan(c, CALL_CLASSIFY, params, x, x_arm_stride);
    // the latent kernel's hard-sample argmax IS classify(c) in eval mode: the labels come out of it directly
    if ((rc = do_forward(c, &nzp, params, const_cast<float*>(bn_running), nullptr, x, x_arm_stride, nullptr, 0, nullptr, labels)))
        return rc;
    if (counts) return launch_confmat(labels, d->A, d->B, d->C, counts, c.stream);
    return 0;
}

// ---- decode / state traversal: every argument is checked before the first launch
static int check_decode_hyper(const mmvae_hyper* h) {
    if (!h) { set_error("hyper is null"); return MMVAE_E_BADARG; }
    if (int rc = check_gemm_engine(h->gemm_bf16)) return rc;
    return 0;
}

size_t mmvae_decode_workspace_bytes(const mmvae_dims* d, const mmvae_exec* ex) { return mmvae_workspace_bytes(d, ex); }

int mmvae_decode(const mmvae_dims* d, const mmvae_hyper* h, const float* params, const float* c, int64_t c_arm_stride,
                 const float* s, int64_t s_arm_stride, float* x_rec, void* ws, size_t ws_bytes, mmvae_exec* ex, void* stream) {
    if (int rc = check_dims(d)) return rc;
    if (int rc = check_decode_hyper(h)) return rc;
    if (!params || !c || !s || !x_rec) { set_error("decode: null params / c / s / x_rec"); return MMVAE_E_BADARG; }
    if (c_arm_stride < 0 || s_arm_stride < 0) { set_error("decode: negative arm stride"); return MMVAE_E_BADARG; }
    // the decoder has no BatchNorm: training mode differs from eval mode only by state dropout, which decode does not offer
    if (h->training != 0 && !(h->training == 1 && h->s_drop == 0.f)) {
        set_error("decode: state dropout (training mode with s_drop > 0) is not supported");
        return MMVAE_E_UNSUPPORTED;
    }
    mmvae_hyper he = *h;
    he.training = 0;
    Ctx cx;
    if (int rc = make_ctx(cx, d, &he, ws, ws_bytes, ex, stream)) return rc;
    make_plan(cx, CALL_DECODE, params, x_rec, 0);
    ZinBuild zb{};
    zb.A = d->A; zb.R = d->B; zb.C = d->C; zb.S = d->S; zb.L = d->L;
    zb.c = c; zb.c_arm = c_arm_stride; zb.s = s; zb.s_arm = s_arm_stride;
    return do_decode(cx, params, zb, nullptr, x_rec);
}

size_t mmvae_state_changes_workspace_bytes(const mmvae_dims* d, int n_samp, const mmvae_exec* ex) {
    if (check_dims(d) || n_samp < 1 || (int64_t)n_samp * d->B > INT32_MAX) return 0;
    mmvae_dims dd = *d;
    dd.B = n_samp * d->B;
    return mmvae_workspace_bytes(d, ex) + mmvae_workspace_bytes(&dd, ex);
}

int mmvae_state_changes(const mmvae_dims* d, const mmvae_hyper* h, const mmvae_noise* nz, const float* params,
                        const float* bn_running, const float* x, int d_s, int n_samp, float* x_rec, void* ws, size_t ws_bytes,
                        mmvae_exec* ex, void* stream) {
    if (int rc = check_dims(d)) return rc;
    if (int rc = check_decode_hyper(h)) return rc;
    if (!nz || !params || !bn_running || !x || !x_rec) {
        set_error("state_changes: null noise / params / bn_running / x / x_rec");
        return MMVAE_E_BADARG;
    }
    if (d_s < 0 || d_s >= d->S) { set_error("state_changes: d_s = %d outside [0, %d)", d_s, d->S); return MMVAE_E_BADARG; }
    if (n_samp < 1) { set_error("state_changes: n_samp = %d < 1", n_samp); return MMVAE_E_BADARG; }
    if (nz->mode != 0 && nz->mode != 1) { set_error("noise mode must be 0 (explicit) or 1 (philox)"); return MMVAE_E_BADARG; }
    if (nz->mode == 0 && !nz->u_state) { set_error("state_changes: explicit noise needs u_state [A, n_samp, B]"); return MMVAE_E_BADARG; }
    if (h->training) { set_error("state_changes needs eval mode (training = 0): the encoder reads the running statistics"); return MMVAE_E_UNSUPPORTED; }
    if ((int64_t)n_samp * d->B > INT32_MAX) { set_error("state_changes: n_samp * B beyond 2^31 rows"); return MMVAE_E_UNSUPPORTED; }
    mmvae_dims dd = *d;
    dd.B = n_samp * d->B;
    const size_t enc_bytes = mmvae_workspace_bytes(d, ex), dec_bytes = mmvae_workspace_bytes(&dd, ex);
    if (!ws) { set_error("null workspace"); return MMVAE_E_BADARG; }
    if (ws_bytes < enc_bytes + dec_bytes) {
        set_error("workspace too small: need %zu bytes, got %zu", enc_bytes + dec_bytes, ws_bytes);
        return MMVAE_E_WORKSPACE;
    }
    // encoder + latent block of forward(eval=True): c_smp is the hard straight-through sample of softmax(c_prob / tau) (no
    // category mask, no Gumbel noise: temp has no effect), mu and y = [x_low | c] stay in the first part of the workspace
    mmvae_hyper he = *h;
    he.training = 0; he.eval_flag = 1; he.hard = 1;
    for (int i = 0; i < 4; ++i) he.cat_mask[i] = 0;
    Ctx ce, cd;
    if (int rc = make_ctx(ce, d, &he, ws, enc_bytes, ex, stream)) return rc;
    if (int rc = make_ctx(cd, &dd, &he, reinterpret_cast<char*>(ws) + enc_bytes, dec_bytes, ex, stream)) return rc;
    make_plan(ce, CALL_TRAVERSE, params, x, 0);
    make_plan(cd, CALL_DECODE, params, x_rec, 0);
    mmvae_noise nzp{};   // (the latent kernel's own state sample is not used: Philox stream of seed 0, as eval_classify)
    nzp.mode = 1;
    int rc;
    if ((rc = do_forward(ce, &nzp, params, const_cast<float*>(bn_running), nullptr, x, 0, nullptr, 0))) return rc;
    ZinBuild zb{};
    zb.A = d->A; zb.R = dd.B; zb.C = d->C; zb.S = d->S; zb.L = d->L;
    zb.enc_ws = ce.ws; zb.csmp = ce.lay.CSMP; zb.y = ce.lay.Y; zb.mu = ce.lay.MU; zb.B = d->B; zb.d_s = d_s;
    zb.params = params; zb.per_arm = ce.po.per_arm; zb.o_wsig = ce.po.o[13]; zb.o_bsig = ce.po.o[15];
    zb.u = nz->mode == 0 ? nz->u_state : nullptr;
    return do_decode(cd, params, zb, nz, x_rec);
}

// ---- encode / intermed: every argument is checked before the first launch
size_t mmvae_encode_workspace_bytes(const mmvae_dims* d, const mmvae_exec* ex) { return mmvae_workspace_bytes(d, ex); }

int mmvae_encode(const mmvae_dims* d, const mmvae_hyper* h, const mmvae_noise* nz, const float* params, float* bn_running,
                 int64_t* nbt, const float* x, int64_t x_arm_stride, const mmvae_encode_out* out, int64_t out_row0,
                 int64_t out_rows, void* ws, size_t ws_bytes, mmvae_exec* ex, void* stream) {
    if (int rc = check_dims(d)) return rc;
    if (int rc = check_decode_hyper(h)) return rc;
    if (!params || !bn_running || !x || !out) { set_error("encode: null params / bn_running / x / out"); return MMVAE_E_BADARG; }
    if (x_arm_stride < 0) { set_error("encode: negative arm stride"); return MMVAE_E_BADARG; }
    const bool latent = out->c || out->c_smp || out->s_mean || out->s_logvar || out->labels || out->counts;
    if (!latent && !out->x_low && !out->c_prob) { set_error("encode: every output is null"); return MMVAE_E_BADARG; }
    if (out_row0 < 0 || out_rows < out_row0 + d->B) {
        set_error("encode: rows [%lld, %lld + %d) do not fit the %lld destination rows", (long long)out_row0, (long long)out_row0,
                  d->B, (long long)out_rows);
        return MMVAE_E_BADARG;
    }
    if (out->counts && d->A < 2) { set_error("encode: counts need at least two arms (got A=%d)", d->A); return MMVAE_E_BADARG; }
    if (h->training != 0 && h->training != 1) { set_error("encode: training must be 0 or 1"); return MMVAE_E_UNSUPPORTED; }
    if (h->training && latent) {
        set_error("encode: training mode offers the encoder outputs only (x_low, c_prob); mmvae_forward computes the latent block");
        return MMVAE_E_UNSUPPORTED;
    }
    if (!h->training && !h->eval_flag) { set_error("encode: eval mode needs eval_flag = 1 (the noise-free sample)"); return MMVAE_E_UNSUPPORTED; }
    mmvae_noise nzp{};   // eval mode draws nothing that reaches the outputs (the kernel's own state sample: Philox of seed 0, as
    nzp.mode = 1;        // eval_classify); training mode reads the dropout keep-mask only
    if (h->training) {
        if (!nz) { set_error("noise descriptor is null"); return MMVAE_E_BADARG; }
        if (nz->mode != 0 && nz->mode != 1) { set_error("noise mode must be 0 (explicit) or 1 (philox)"); return MMVAE_E_BADARG; }
        if (h->x_drop < 0.f || h->x_drop >= 1.f) { set_error("dropout probabilities must be in [0,1)"); return MMVAE_E_BADARG; }
        if (nz->mode == 0 && h->x_drop > 0.f && !nz->x_mask) { set_error("explicit noise: x_mask is null"); return MMVAE_E_BADARG; }
        nzp = *nz;
    }
    Ctx c;
    if (int rc = make_ctx(c, d, h, ws, ws_bytes, ex, stream)) return rc;
    make_plan(c, CALL_ENCODE, params, x, x_arm_stride);
    EncOut eo{out->x_low, out->c_prob, out->c, out->c_smp, out->s_mean, out->s_logvar, out->labels, out_row0, out_rows, !latent};
    // the confusion counts read compact [A, B] labels: the kernel leaves them in a region only a backward pass uses
    static_assert(sizeof(int32_t) == sizeof(float), "labels fit GZC's [A, B, C] floats");
    int32_t* labels_ab = out->counts ? reinterpret_cast<int32_t*>(c.ws + c.lay.GZC) : nullptr;
    if (int rc = do_forward(c, &nzp, params, bn_running, h->training ? nbt : nullptr, x, x_arm_stride, nullptr, 0, nullptr,
                            labels_ab, &eo))
        return rc;
    if (out->counts) return launch_confmat(labels_ab, d->A, d->B, d->C, out->counts, c.stream);
    return 0;
}

int mmvae_intermed(const mmvae_dims* d, const mmvae_hyper* h, const float* params, const float* y, int64_t y_arm_stride,
                   float* mu, float* var, void* stream) {
    if (int rc = check_dims(d)) return rc;
    if (int rc = check_decode_hyper(h)) return rc;
    if (!params || !y || !mu || !var) { set_error("intermed: null params / y / mu / var"); return MMVAE_E_BADARG; }
    if (y_arm_stride < 0) { set_error("intermed: negative arm stride"); return MMVAE_E_BADARG; }
    return launch_intermed(*d, make_poff(*d), params, y, y_arm_stride, mu, var, reinterpret_cast<hipStream_t>(stream));
}

// ---- pruning: every argument is checked before the launch
int mmvae_prune_apply(const mmvae_dims* d, const uint32_t cat_mask[4], float* params, float* grads, float* exp_avg,
                      float* exp_avg_sq, void* stream) {
    if (int rc = check_dims(d)) return rc;
    if (!cat_mask) { set_error("prune_apply: cat_mask is null"); return MMVAE_E_BADARG; }
    if (!params && !grads && !exp_avg && !exp_avg_sq) { set_error("prune_apply: every buffer is null"); return MMVAE_E_BADARG; }
    if (!(cat_mask[0] | cat_mask[1] | cat_mask[2] | cat_mask[3])) return 0;   // no mask: every category kept (mmvae_hyper.cat_mask)
    // bits beyond n_categories are ignored; at least one category must be kept (as make_ctx)
    uint32_t any = 0;
    for (int k = 0; k < d->C; ++k) any |= (cat_mask[k >> 5] >> (k & 31)) & 1u;
    if (!any) { set_error("cat_mask keeps none of the %d categories", d->C); return MMVAE_E_BADARG; }
    return launch_prune_apply(*d, make_poff(*d), cat_mask, params, grads, exp_avg, exp_avg_sq, reinterpret_cast<hipStream_t>(stream));
}

int mmvae_debug_stage(const mmvae_dims* d, const mmvae_hyper* h, const mmvae_noise* nz, int stage,
                      const float* params, const float* x, int64_t x_arm_stride, void* ws, size_t ws_bytes,
                      float* grads, mmvae_exec* ex, void* stream) {
    Ctx c;
    if (int rc = make_ctx(c, d, h, ws, ws_bytes, ex, stream)) return rc;
    if (!params || !x) { set_error("null params / x"); return MMVAE_E_BADARG; }
    if (int rc = check_noise(c, nz)) return rc;
    // a stage is replayed on the state a complete forward / backward pass of the same engine left behind: its slice planes
    // are in place, and no head launch of this call has zeroed anything
    make_plan(c, CALL_REPLAY, params, x, x_arm_stride);
    const bool fast = c.plan.fast;
    switch (stage) {
        case 0: return fc1_forward(c, nz, params, x, x_arm_stride);
        case 1:
            if (int rc = fc11_main(c, params, x, x_arm_stride, nullptr, 1)) return rc;
            return fc11_gd10(c, params, nullptr, 1);
        case 2:
            if (!fast) return launch_dw_big(c, nz, x, x_arm_stride);
            if (int rc = dw1(c, x, x_arm_stride)) return rc;
            return dw11(c);
        case 9: return launch_make_xbits(c, nz);
        case 20: return launch_chain_fwd_enc(c, 3, params, nullptr, nullptr);   // one encoder layer (fc3)
        case 21: return launch_chain_bwd_enc(c, 3, params);
        // single kernels of the fast path (per-kernel roofline timing)
        case 10: case 11: case 12: case 13: case 14:
            if (!fast) { set_error("stage %d needs the fast path", stage); return MMVAE_E_UNSUPPORTED; }
            if (stage == 10) return fc11_main(c, params, x, x_arm_stride, nullptr, 1);
            if (stage == 11) return fc11_gd10(c, params, nullptr, 1);   // (a launch only where d(d10) has one of its own: FC11_ZT)
            if (stage == 12) return dw1(c, x, x_arm_stride);
            if (stage == 13) return dw11(c);
            return fc1_gemm(c, params, x, x_arm_stride);
        case 3: return launch_dw_small(c);
        case 4: return launch_chain_fwd_dec(c, params);
        case 5: return launch_chain_bwd_dec(c, params);
        case 6: return launch_lat_fwd(c, nz, params, nullptr, nullptr);
        case 7: return launch_lat_bwd(c, nz, params);
        case 8: if (!grads) { set_error("grads is null"); return MMVAE_E_BADARG; } return launch_reduce_grads(c, grads, 1.f, nullptr);
        default: set_error("unknown stage %d", stage); return MMVAE_E_BADARG;
    }
}

int mmvae_debug_plan(const mmvae_dims* d, const mmvae_hyper* h, const mmvae_exec* ex, int call_kind, int params_align,
                     int x_align, int64_t x_arm_stride, int has_x16, int fc11_grad, int32_t out[MMVAE_PLAN_FIELDS]) {
    if (int rc = check_dims(d)) return rc;
    if (!h || !out) { set_error("null hyper / out"); return MMVAE_E_BADARG; }
    if (int rc = check_gemm_engine(h->gemm_bf16)) return rc;
    static_assert(MMVAE_CALL_STEP == CALL_STEP && MMVAE_CALL_STEP_ROWS == CALL_STEP_ROWS && MMVAE_CALL_FORWARD == CALL_FORWARD &&
                  MMVAE_CALL_BACKWARD == CALL_BACKWARD && MMVAE_CALL_LOSS == CALL_LOSS && MMVAE_CALL_CLASSIFY == CALL_CLASSIFY &&
                  MMVAE_CALL_REPLAY == CALL_REPLAY && MMVAE_CALL_DECODE == CALL_DECODE && MMVAE_CALL_TRAVERSE == CALL_TRAVERSE &&
                  MMVAE_CALL_ENCODE == CALL_ENCODE && MMVAE_CALL_ZINB_STEP == CALL_ZINB_STEP,
                  "MMVAE_CALL_* (include/mmvae.h) are the values of CallKind");
    if (call_kind < CALL_STEP || (call_kind > CALL_TRAVERSE && call_kind != CALL_ENCODE && call_kind != CALL_ZINB_STEP)) { set_error("unknown call kind %d", call_kind); return MMVAE_E_BADARG; }
    if (params_align < 0 || x_align < 0) { set_error("negative alignment"); return MMVAE_E_BADARG; }
    // what make_ctx gives make_plan to read -- dims, hyper, exec copy, layout -- without a workspace or a stream
    Ctx c{};
    c.d = *d;
    c.h = *h;
    // (as their entry points plan: decode and the traversal force eval mode, eval_classify accepts nothing else)
    if (call_kind == CALL_DECODE || call_kind == CALL_TRAVERSE || call_kind == CALL_CLASSIFY) c.h.training = 0;
    if (ex) c.ex = *ex; else memset(&c.ex, 0, sizeof(c.ex));
    if (call_kind == CALL_ZINB_STEP) c.ex.side_stream = nullptr;   // (mmvae_zinb_train_step runs on the call's stream alone)
    c.lay = make_layout(*d, &c.ex);
    c.po = make_poff(*d);
    // pointers that are never dereferenced: a 16-byte boundary plus the stated alignment's offset
    const uintptr_t base = 1u << 20;
    const float* params = reinterpret_cast<const float*>(base + (uintptr_t)(params_align & 15));
    const float* x = reinterpret_cast<const float*>(2 * base + (uintptr_t)(x_align & 15));
    if (has_x16 && call_kind == CALL_STEP_ROWS) c.x16 = reinterpret_cast<const unsigned short*>(3 * base);   // (no other call takes one)
    make_plan(c, (CallKind)call_kind, params, x, x_arm_stride, fc11_grad != 0);
    const Plan& p = c.plan;
    const int32_t v[] = {(int32_t)p.kind, p.fast, (int32_t)p.big, p.small_x3, (int32_t)p.fc11, p.gd10_slabs, p.dw11_slabs, p.chain_planes,
                         p.lat_half, p.narrow, p.presplit, p.bwd_small_planes, p.d10_planes, p.dz1_in_apply, p.dec_planes,
                         (int32_t)p.zero, p.rowmap, p.dz11_bf16, p.dw11_side, p.loss_on_side, (int32_t)p.couple, p.lat_fork_rides,
                         p.fc11_fork_rides};
    static_assert(sizeof(v) / sizeof(v[0]) == MMVAE_PLAN_FIELDS, "one value per field of Plan, in declaration order");
    for (int i = 0; i < MMVAE_PLAN_FIELDS; ++i) out[i] = v[i];
    return 0;
}

int mmvae_dump_noise(const mmvae_dims* d, const mmvae_hyper* h, const mmvae_noise* nz, uint8_t* x_mask,
                     float* u_gumbel, float* u_state, uint8_t* s_mask, void* stream) {
    if (int rc = check_dims(d)) return rc;
    if (!h || !nz) { set_error("null hyper / noise"); return MMVAE_E_BADARG; }
    return launch_dump_noise(*d, *h, nz, x_mask, u_gumbel, u_state, s_mask, reinterpret_cast<hipStream_t>(stream));
}

}  // extern "C"

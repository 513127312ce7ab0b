// C ABI (include/mmvae.h) of the evaluation and analysis routines: labels and consensus, mutual information, silhouette,
// state-gene correlation, the rank sums of the marker genes, k nearest neighbours, the Gaussian classifiers, the leaf merge, ZINB scoring and the ZINB heads' gradients, the count distributions, the random forest, PCA and data preparation.  Every argument is checked here, on the host,
// before any device work; the training step's entry points, the plan and set_error live in api.hip.
#include "common.hpp"

using namespace mmvae;

// ---- the checks the analysis entry points share.  who: the entry's name as its messages give it.  Each returns 0 or, after
// ---- set_error, the refusal's code; an entry lists its checks in the order that decides which refusal a doubly-bad call gets.
constexpr int64_t N_MAX = (int64_t)1 << 31;     // rows of one call at most

static int check_count(const char* who, const char* name, int64_t v, int64_t lo, int64_t hi) {
    if (v >= lo && v <= hi) return 0;
    set_error("%s: %s outside [%lld, %lld] (got %lld)", who, name, (long long)lo, (long long)hi, (long long)v);
    return MMVAE_E_BADARG;
}

// a count from 1 up (else a bad argument) that the kernels take up to cap (above: unsupported)
static int check_extent(const char* who, const char* name, int v, int cap) {
    if (int rc = check_count(who, name, v, 1, INT32_MAX)) return rc;
    if (v <= cap) return 0;
    set_error("%s: %s = %d above %d", who, name, v, cap);
    return MMVAE_E_UNSUPPORTED;
}

// n selected rows of a matrix of n_total: without a row map they are its first n
static int check_rowmap(const char* who, const int64_t* rows, int64_t n, int64_t n_total) {
    if (n_total < 1) { set_error("%s: n_total = %lld below 1", who, (long long)n_total); return MMVAE_E_BADARG; }
    if (rows || n <= n_total) return 0;
    set_error("%s: n = %lld rows of a matrix of %lld without a row map", who, (long long)n, (long long)n_total);
    return MMVAE_E_BADARG;
}

static int check_pitch(const char* who, const char* ldname, int64_t ld, const char* dname, int64_t d) {
    if (ld >= d) return 0;
    set_error("%s: %s = %lld below %s = %lld", who, ldname, (long long)ld, dname, (long long)d);
    return MMVAE_E_BADARG;
}

static int check_aligned(const char* who, const char* what, const void* p, size_t bytes) {
    if (reinterpret_cast<uintptr_t>(p) % bytes == 0) return 0;
    set_error("%s: %s %p not %zu-byte aligned", who, what, p, bytes);
    return MMVAE_E_BADARG;
}

static int check_ws(const char* who, size_t ws_bytes, size_t need) {
    if (ws_bytes >= need) return 0;
    set_error("%s: workspace of %zu bytes below the %zu needed", who, ws_bytes, need);
    return MMVAE_E_WORKSPACE;
}

// path: -1 the launcher's rule (the 16-byte loads where the base and the row pitch allow them), 0 the narrow loads, 1 the
// 16-byte loads
static int pick_wide(const char* who, int path, const void* base, int64_t ld, int elem_bytes, bool* wide) {
    if (int rc = check_count(who, "path", path, -1, 1)) return rc;
    const bool can = wide16(base, ld, elem_bytes);
    if (path == 1 && !can) {
        set_error("%s: path = 1 (16-byte loads) needs a 16-byte aligned base and a row pitch of whole 16 bytes (base %p, ld = %lld)",
                  who, base, (long long)ld);
        return MMVAE_E_UNSUPPORTED;
    }
    *wide = path < 0 ? can : path == 1;
    return 0;
}

extern "C" {

int mmvae_classify(const float* c_probs, int64_t n_cells, int C, int32_t* labels, void* stream) {
    if (!c_probs || !labels || n_cells <= 0 || C <= 0) { set_error("classify: bad argument"); return MMVAE_E_BADARG; }
    return launch_classify(c_probs, n_cells, C, labels, reinterpret_cast<hipStream_t>(stream));
}

int mmvae_confmat_accumulate(const int32_t* labels, int A, int64_t n, int C, int64_t* counts, void* stream) {
    if (!labels || !counts || A < 1 || A > MMVAE_MAX_ARMS || n <= 0 || C <= 0) {
        set_error("confmat_accumulate: bad argument");
        return MMVAE_E_BADARG;
    }
    return launch_confmat(labels, A, n, C, counts, reinterpret_cast<hipStream_t>(stream));
}

int mmvae_consensus(const int64_t* counts, int npairs, int C, double* cm_norm, double* consensus, void* stream) {
    if (!counts || !consensus || npairs < 1 || C < 1) { set_error("consensus: bad argument"); return MMVAE_E_BADARG; }
    if (C > 128) { set_error("consensus: C > 128 unsupported"); return MMVAE_E_UNSUPPORTED; }
    return launch_consensus(counts, npairs, C, cm_norm, consensus, reinterpret_cast<hipStream_t>(stream));
}

// every argument of mmvae_pair_stats is checked here, on the host, before any device work
static int pair_stats_args(const int32_t* labels, const float* probs, int n_arms_total, int64_t n, int C, const int32_t* pairs,
                           int n_pairs, const int64_t* counts, const int64_t* dist_acc) {
    if (!labels || !probs || !pairs || !counts || !dist_acc) { set_error("pair_stats: null pointer"); return MMVAE_E_BADARG; }
    if (C < 1 || C > 128) { set_error("pair_stats: C = %d outside [1, 128]", C); return MMVAE_E_BADARG; }
    if (n < 0 || n_pairs < 0) { set_error("pair_stats: negative n or n_pairs"); return MMVAE_E_BADARG; }
    if (n > ((int64_t)1 << 31)) { set_error("pair_stats: more than 2^31 cells in one call"); return MMVAE_E_BADARG; }
    if (n_arms_total < 1 || n_arms_total > 2 * MMVAE_MAX_ARMS) {
        set_error("pair_stats: n_arms_total = %d outside [1, %d]", n_arms_total, 2 * MMVAE_MAX_ARMS);
        return MMVAE_E_BADARG;
    }
    for (int64_t k = 0; k < 4 * (int64_t)n_pairs; ++k)
        if (pairs[k] < 0 || pairs[k] >= n_arms_total) {
            set_error("pair_stats: pairs[%lld][%d] = %d outside [0, %d)", (long long)(k / 4), (int)(k % 4), pairs[k], n_arms_total);
            return MMVAE_E_BADARG;
        }
    return 0;
}

int mmvae_pair_stats(const int32_t* labels, const float* probs, int n_arms_total, int64_t n, int C, const int32_t* pairs,
                     int n_pairs, int64_t* counts, int64_t* dist_acc, void* stream) {
    if (int rc = pair_stats_args(labels, probs, n_arms_total, n, C, pairs, n_pairs, counts, dist_acc)) return rc;
    if (n == 0 || n_pairs == 0) return 0;
    return launch_pair_stats(labels, probs, n, C, pairs, n_pairs, counts, dist_acc, -1, reinterpret_cast<hipStream_t>(stream));
}

int mmvae_debug_pair_stats(const int32_t* labels, const float* probs, int n_arms_total, int64_t n, int C, const int32_t* pairs,
                           int n_pairs, int64_t* counts, int64_t* dist_acc, int path, void* stream) {
    if (int rc = pair_stats_args(labels, probs, n_arms_total, n, C, pairs, n_pairs, counts, dist_acc)) return rc;
    if (path < -1 || path > 1) { set_error("debug_pair_stats: path %d outside {-1, 0, 1}", path); return MMVAE_E_BADARG; }
    if (n == 0 || n_pairs == 0) return 0;
    return launch_pair_stats(labels, probs, n, C, pairs, n_pairs, counts, dist_acc, path, reinterpret_cast<hipStream_t>(stream));
}

int mmvae_pair_stats_finish(const int64_t* counts, const int64_t* dist_acc, int n_pairs, int C, double* cm_norm, double* emp,
                            double* dist_norm, double* diag_mean, double* diag_min, void* stream) {
    if (!counts || !dist_acc || !cm_norm || !emp || !dist_norm || !diag_mean || !diag_min) {
        set_error("pair_stats_finish: null pointer");
        return MMVAE_E_BADARG;
    }
    if (C < 1 || C > 128) { set_error("pair_stats_finish: C = %d outside [1, 128]", C); return MMVAE_E_BADARG; }
    if (n_pairs < 0) { set_error("pair_stats_finish: negative n_pairs"); return MMVAE_E_BADARG; }
    if (n_pairs == 0) return 0;
    return launch_pair_finish(counts, dist_acc, n_pairs, C, cm_norm, emp, dist_norm, diag_mean, diag_min,
                              reinterpret_cast<hipStream_t>(stream));
}

// every argument of mmvae_mutinfo_counts is checked here, on the host, before any device work
static int mutinfo_counts_args(const int32_t* labels, int A, int64_t n, int C, const void* targets, int target_bytes, int64_t ldt,
                               int F, const int64_t* counts, const int64_t* t_sum, const int64_t* p_sum) {
    if (!labels || !targets || !counts || !t_sum || !p_sum) { set_error("mutinfo_counts: null pointer"); return MMVAE_E_BADARG; }
    if (A < 1 || A > MMVAE_MAX_ARMS) { set_error("mutinfo_counts: A = %d outside [1, %d]", A, MMVAE_MAX_ARMS); return MMVAE_E_BADARG; }
    if (C < 1 || C > 128) { set_error("mutinfo_counts: C = %d outside [1, 128]", C); return MMVAE_E_BADARG; }
    if (F < 1 || F > 4096) { set_error("mutinfo_counts: F = %d outside [1, 4096]", F); return MMVAE_E_BADARG; }
    if (n < 0 || n > ((int64_t)1 << 31)) { set_error("mutinfo_counts: n outside [0, 2^31]"); return MMVAE_E_BADARG; }
    if (ldt < F) { set_error("mutinfo_counts: ldt = %lld below F = %d", (long long)ldt, F); return MMVAE_E_BADARG; }
    if (target_bytes != 1 && target_bytes != 4) {
        set_error("mutinfo_counts: target_bytes = %d is neither 1 (uint8) nor 4 (int32)", target_bytes);
        return MMVAE_E_BADARG;
    }
    return 0;
}

int mmvae_mutinfo_counts(const int32_t* labels, int A, int64_t n, int C, const void* targets, int target_bytes, int64_t ldt, int F,
                         int64_t* counts, int64_t* t_sum, int64_t* p_sum, void* stream) {
    if (int rc = mutinfo_counts_args(labels, A, n, C, targets, target_bytes, ldt, F, counts, t_sum, p_sum)) return rc;
    if (n == 0) return 0;
    return launch_mi_counts(labels, A, n, C, targets, target_bytes, ldt, F, counts, t_sum, p_sum, -1,
                            reinterpret_cast<hipStream_t>(stream));
}

int mmvae_debug_mutinfo_counts(const int32_t* labels, int A, int64_t n, int C, const void* targets, int target_bytes, int64_t ldt,
                               int F, int64_t* counts, int64_t* t_sum, int64_t* p_sum, int path, void* stream) {
    if (int rc = mutinfo_counts_args(labels, A, n, C, targets, target_bytes, ldt, F, counts, t_sum, p_sum)) return rc;
    if (path < -1 || path > 1) { set_error("debug_mutinfo_counts: path %d outside {-1, 0, 1}", path); return MMVAE_E_BADARG; }
    if (n == 0) return 0;
    return launch_mi_counts(labels, A, n, C, targets, target_bytes, ldt, F, counts, t_sum, p_sum, path,
                            reinterpret_cast<hipStream_t>(stream));
}

size_t mmvae_ami_binary_workspace_bytes(int64_t N) {
    return N < 1 || N > ((int64_t)1 << 31) ? 0 : 2 * (size_t)(N + 1) * sizeof(double);
}

int mmvae_ami_binary(const int64_t* n11, const int64_t* t_sum, const int64_t* p_sum, int A, int F, int C, int64_t N, void* ws,
                     size_t ws_bytes, double* ami, void* stream) {
    if (!n11 || !t_sum || !p_sum || !ami) { set_error("ami_binary: null pointer"); return MMVAE_E_BADARG; }
    if (A < 0 || A > MMVAE_MAX_ARMS) { set_error("ami_binary: A = %d outside [0, %d]", A, MMVAE_MAX_ARMS); return MMVAE_E_BADARG; }
    if (C < 1 || C > 128) { set_error("ami_binary: C = %d outside [1, 128]", C); return MMVAE_E_BADARG; }
    if (F < 1 || F > 4096) { set_error("ami_binary: F = %d outside [1, 4096]", F); return MMVAE_E_BADARG; }
    if (N < 1 || N > ((int64_t)1 << 31)) { set_error("ami_binary: N outside [1, 2^31]"); return MMVAE_E_BADARG; }
    if (ws) {
        if (reinterpret_cast<uintptr_t>(ws) % sizeof(double)) { set_error("ami_binary: workspace not 8-byte aligned"); return MMVAE_E_BADARG; }
        if (ws_bytes < mmvae_ami_binary_workspace_bytes(N)) {
            set_error("ami_binary: workspace of %zu bytes below the %zu needed", ws_bytes, mmvae_ami_binary_workspace_bytes(N));
            return MMVAE_E_WORKSPACE;
        }
    }
    if (A == 0) return 0;
    return launch_ami_binary(n11, t_sum, p_sum, A, F, C, N, static_cast<double*>(ws), ami, reinterpret_cast<hipStream_t>(stream));
}

// ---- silhouette (silhouette.hip) ----
size_t mmvae_silhouette_workspace_bytes(int64_t n, int K) {
    if (n < 3 || n > N_MAX || K < 2 || K > n - 1) return 0;
    return seg_ws_bytes(nseg_max(n, K, SIL_SEG_COLS), n, K);
}

int mmvae_silhouette(const float* x_sorted, int64_t ld, int64_t n, int d, const int64_t* offsets, int K, const int64_t* perm, void* ws,
                     size_t ws_bytes, double* s, void* stream) {
    const char* who = "silhouette";
    if (!x_sorted || !offsets || !ws || !s) { set_error("%s: null pointer", who); return MMVAE_E_BADARG; }
    if (int rc = check_count(who, "n", n, 3, N_MAX)) return rc;
    if (int rc = check_count(who, "K", K, 2, n - 1)) return rc;
    if (int rc = check_count(who, "d", d, 1, INT32_MAX)) return rc;
    if (int rc = check_pitch(who, "ld", ld, "d", d)) return rc;
    if (int rc = check_aligned(who, "workspace", ws, sizeof(double))) return rc;
    if (d > SIL_MAX_D) { set_error("%s: d = %d above %d", who, d, SIL_MAX_D); return MMVAE_E_UNSUPPORTED; }
    const int64_t nseg = nseg_max(n, K, SIL_SEG_COLS);
    const size_t need = mmvae_silhouette_workspace_bytes(n, K);
    if (nseg > SIL_MAX_SEGMENTS || need == 0) {
        set_error("%s: K + n / %d = %lld segments above %lld", who, SIL_SEG_COLS, (long long)nseg, (long long)SIL_MAX_SEGMENTS);
        return MMVAE_E_UNSUPPORTED;
    }
    if (int rc = check_ws(who, ws_bytes, need)) return rc;
    return launch_silhouette(x_sorted, ld, n, d, offsets, K, perm, ws, s, reinterpret_cast<hipStream_t>(stream));
}

// ---- state-gene correlation (statecorr.hip) ----
// the most segments and the most workgroups of one grid that mmvae_state_corr launches; false where it refuses the shape
static bool sc_shape_ok(int64_t n, int D, int S, int G) {
    if (S > SC_MAX_S) return false;
    const unsigned __int128 tiles = (unsigned __int128)cdiv64(D, SC_TILE);
    return (unsigned __int128)nseg_max(n, G, SC_SEG_ROWS) * tiles <= (unsigned __int128)SC_MAX_BLOCKS &&
           (unsigned __int128)G * (unsigned __int128)cdiv64(D, 256) <= (unsigned __int128)SC_MAX_BLOCKS;
}

size_t mmvae_state_corr_workspace_bytes(int64_t n, int D, int S, int G) {
    if (n < 1 || n > N_MAX || D < 1 || S < 1 || G < 1 || !sc_shape_ok(n, D, S, G)) return 0;
    return seg_ws_bytes(nseg_max(n, G, SC_SEG_ROWS), (5 + 5 * (int64_t)S) * D, G);
}

static int state_corr_checked(const float* data, int64_t ld, int64_t n_total, int D, const int64_t* rows, const float* state,
                              int64_t lds, int64_t n, int S, const int64_t* offsets, int G, void* ws, size_t ws_bytes, double* r,
                              int64_t* count, int path, void* stream) {
    const char* who = "state_corr";
    if (!data || !state || !ws || !r || !count) { set_error("%s: null pointer", who); return MMVAE_E_BADARG; }
    if (int rc = check_count(who, "n", n, 1, N_MAX)) return rc;
    if (int rc = check_rowmap(who, rows, n, n_total)) return rc;
    if (int rc = check_count(who, "D", D, 1, INT32_MAX)) return rc;
    if (int rc = check_count(who, "S", S, 1, INT32_MAX)) return rc;
    if (int rc = check_count(who, "G", G, 1, INT32_MAX)) return rc;
    if (int rc = check_pitch(who, "ld", ld, "D", D)) return rc;
    if (int rc = check_pitch(who, "lds", lds, "S", S)) return rc;
    if (int rc = check_aligned(who, "workspace", ws, sizeof(double))) return rc;
    if (S > SC_MAX_S) { set_error("%s: S = %d above %d", who, S, SC_MAX_S); return MMVAE_E_UNSUPPORTED; }
    const size_t need = mmvae_state_corr_workspace_bytes(n, D, S, G);
    if (need == 0) {     // (the shape rule of sc_shape_ok, or a size no size_t holds)
        set_error("%s: n = %lld, D = %d, G = %d need a grid of more than %lld workgroups", who, (long long)n, D, G, (long long)SC_MAX_BLOCKS);
        return MMVAE_E_UNSUPPORTED;
    }
    if (int rc = check_ws(who, ws_bytes, need)) return rc;
    bool wide;
    if (int rc = pick_wide(who, path, data, ld, sizeof(float), &wide)) return rc;
    return launch_state_corr(data, ld, n_total, D, rows, state, lds, n, S, offsets, G, ws, r, count, wide,
                             reinterpret_cast<hipStream_t>(stream));
}

int mmvae_state_corr(const float* data, int64_t ld, int64_t n_total, int D, const int64_t* rows, const float* state, int64_t lds,
                     int64_t n, int S, const int64_t* offsets, int G, void* ws, size_t ws_bytes, double* r, int64_t* count,
                     void* stream) {
    return state_corr_checked(data, ld, n_total, D, rows, state, lds, n, S, offsets, G, ws, ws_bytes, r, count, -1, stream);
}

int mmvae_debug_state_corr(const float* data, int64_t ld, int64_t n_total, int D, const int64_t* rows, const float* state,
                           int64_t lds, int64_t n, int S, const int64_t* offsets, int G, void* ws, size_t ws_bytes, double* r,
                           int64_t* count, int path, void* stream) {
    return state_corr_checked(data, ld, n_total, D, rows, state, lds, n, S, offsets, G, ws, ws_bytes, r, count, path, stream);
}

// ---- rank sums of every gene (ranksum.hip) ----
size_t mmvae_rank_sum_workspace_bytes(int64_t n, int D, int G) {
    if (n < 1 || n > RS_MAX_N || D < 1 || G < 1 || G > RS_MAX_G) return 0;
    return ((size_t)(D < RS_CHUNK ? D : RS_CHUNK) * (size_t)n * sizeof(float) + 7) / 8 * 8;
}

// the checks both rank-sum entries begin with, up to eps.  cap: the entry's most cells; why: what those cells are the most of
static int rank_sum_args(const char* who, int cap, const char* why, const float* x, int64_t ldx, int64_t n_total, int D,
                         const int64_t* rows, int64_t n, const int64_t* offsets, int G, float eps, const void* ws,
                         const int64_t* rank_sum2, const int64_t* tie_term, const int64_t* n_pos, const double* sum) {
    if (!x || !offsets || !ws || !rank_sum2 || !tie_term || !n_pos || !sum) { set_error("%s: null pointer", who); return MMVAE_E_BADARG; }
    if (int rc = check_count(who, "n", n, 1, INT64_MAX)) return rc;
    if (n > cap) { set_error("%s: n = %lld cells above the %d %s", who, (long long)n, cap, why); return MMVAE_E_UNSUPPORTED; }
    if (int rc = check_rowmap(who, rows, n, n_total)) return rc;
    if (int rc = check_count(who, "D", D, 1, INT32_MAX)) return rc;
    if (int rc = check_extent(who, "G", G, RS_MAX_G)) return rc;
    if (int rc = check_pitch(who, "ldx", ldx, "D", D)) return rc;
    if (eps != eps) { set_error("%s: eps is a NaN", who); return MMVAE_E_BADARG; }
    return 0;
}

int mmvae_rank_sum(const float* x, int64_t ldx, int64_t n_total, int D, const int64_t* rows, int64_t n, const int64_t* offsets, int G,
                   float eps, void* ws, size_t ws_bytes, int64_t* rank_sum2, int64_t* tie_term, int64_t* n_pos, double* sum,
                   void* stream) {
    const char* who = "rank_sum";
    if (int rc = rank_sum_args(who, RS_MAX_N, "whose keys one workgroup's LDS holds", x, ldx, n_total, D, rows, n, offsets, G, eps, ws,
                               rank_sum2, tie_term, n_pos, sum))
        return rc;
    if (int rc = check_aligned(who, "workspace", ws, sizeof(double))) return rc;
    if (int rc = check_ws(who, ws_bytes, mmvae_rank_sum_workspace_bytes(n, D, G))) return rc;
    return launch_rank_sum(x, ldx, n_total, D, rows, (int)n, offsets, G, eps, ws, rank_sum2, tie_term, n_pos, sum,
                           reinterpret_cast<hipStream_t>(stream));
}

// block: 0 the default RS_MAX_N, else a power of two in [RSB_MIN_BLOCK, RS_MAX_N]; 0 for anything else
static int rsb_block(int block) {
    if (block == 0) return RS_MAX_N;
    return block >= RSB_MIN_BLOCK && block <= RS_MAX_N && (block & (block - 1)) == 0 ? block : 0;
}

size_t mmvae_rank_sum_blocked_workspace_bytes(int64_t n, int D, int G, int block) {
    if (n < 1 || n > RSB_MAX_N || D < 1 || G < 1 || G > RS_MAX_G || !rsb_block(block)) return 0;
    return ((size_t)rsb_chunk(n, D) * rsb_gene_bytes(n) + 7) / 8 * 8;
}

static int rank_sum_blocked_checked(const float* x, int64_t ldx, int64_t n_total, int D, const int64_t* rows, int64_t n,
                                    const int64_t* offsets, int G, float eps, int block, void* ws, size_t ws_bytes, int64_t* rank_sum2,
                                    int64_t* tie_term, int64_t* n_pos, double* sum, int form, int phases, void* stream) {
    const char* who = "rank_sum_blocked";
    if (int rc = rank_sum_args(who, RSB_MAX_N, "whose tie term an int64 holds", x, ldx, n_total, D, rows, n, offsets, G, eps, ws,
                               rank_sum2, tie_term, n_pos, sum))
        return rc;
    const int L = rsb_block(block);
    if (!L) {
        set_error("%s: block = %d is neither 0 nor a power of two in [%d, %d]", who, block, RSB_MIN_BLOCK, RS_MAX_N);
        return MMVAE_E_BADARG;
    }
    if (form < RSB_FORM_AUTO || form > RSB_FORM_IN_PLACE || phases < 0 || phases > 3) {
        set_error("%s: form = %d outside [-1, 1] or phases = %d outside [0, 3]", who, form, phases);
        return MMVAE_E_BADARG;
    }
    if (int rc = check_aligned(who, "workspace", ws, sizeof(double))) return rc;
    if (int rc = check_ws(who, ws_bytes, mmvae_rank_sum_blocked_workspace_bytes(n, D, G, block))) return rc;
    return launch_rank_sum_blocked(x, ldx, n_total, D, rows, (int)n, offsets, G, eps, L, ws, rank_sum2, tie_term, n_pos, sum, form, phases,
                                   reinterpret_cast<hipStream_t>(stream));
}

int mmvae_rank_sum_blocked(const float* x, int64_t ldx, int64_t n_total, int D, const int64_t* rows, int64_t n, const int64_t* offsets,
                           int G, float eps, int block, void* ws, size_t ws_bytes, int64_t* rank_sum2, int64_t* tie_term, int64_t* n_pos,
                           double* sum, void* stream) {
    return rank_sum_blocked_checked(x, ldx, n_total, D, rows, n, offsets, G, eps, block, ws, ws_bytes, rank_sum2, tie_term, n_pos, sum,
                                    RSB_FORM_AUTO, 0, stream);
}

int mmvae_debug_rank_sum_blocked(const float* x, int64_t ldx, int64_t n_total, int D, const int64_t* rows, int64_t n,
                                 const int64_t* offsets, int G, float eps, int block, void* ws, size_t ws_bytes, int64_t* rank_sum2,
                                 int64_t* tie_term, int64_t* n_pos, double* sum, int form, int phases, void* stream) {
    return rank_sum_blocked_checked(x, ldx, n_total, D, rows, n, offsets, G, eps, block, ws, ws_bytes, rank_sum2, tie_term, n_pos, sum,
                                    form, phases, stream);
}

// ---- k nearest neighbours (knn.hip) ----
size_t mmvae_knn_workspace_bytes(int64_t nq, int64_t nr, int d, int k) {
    if (nq < 1 || nq > KNN_MAX_N || nr < 1 || nr > KNN_MAX_N || d < 1 || d > KNN_MAX_D || k < 1 || k > KNN_MAX_K) return 0;
    return knn_ws_bytes(nq, nr, k, knn_seg_cols(nq, nr, k));
}

// what mmvae_knn and mmvae_knn_votes check alike, in their order: k, then `name` (d, n_classes), then nq and nr
static int knn_extents(const char* who, int k, const char* name, int v, int cap, int64_t nq, int64_t nr) {
    if (int rc = check_extent(who, "k", k, KNN_MAX_K)) return rc;
    if (int rc = check_extent(who, name, v, cap)) return rc;
    if (int rc = check_count(who, "nq", nq, 1, INT64_MAX)) return rc;
    if (int rc = check_count(who, "nr", nr, 1, INT64_MAX)) return rc;
    if (nq <= KNN_MAX_N && nr <= KNN_MAX_N) return 0;
    set_error("%s: nq = %lld, nr = %lld above %d", who, (long long)nq, (long long)nr, KNN_MAX_N);
    return MMVAE_E_UNSUPPORTED;
}

static int knn_checked(const float* q, int64_t ldq, int64_t nq, const float* r, int64_t ldr, int64_t nr, int d, int k,
                       const int32_t* qgroup, const int32_t* rgroup, void* ws, size_t ws_bytes, int32_t* idx, float* dist2,
                       int64_t seg_cols, int phases, void* stream) {
    const char* who = "knn";
    if (!q || !r || !ws || !idx || !dist2) { set_error("%s: null pointer", who); return MMVAE_E_BADARG; }
    if ((qgroup == nullptr) != (rgroup == nullptr)) {
        set_error("%s: qgroup and rgroup come together or not at all", who);
        return MMVAE_E_BADARG;
    }
    if (int rc = knn_extents(who, k, "d", d, KNN_MAX_D, nq, nr)) return rc;
    if (int rc = check_pitch(who, "ldq", ldq, "d", d)) return rc;
    if (int rc = check_pitch(who, "ldr", ldr, "d", d)) return rc;
    if (seg_cols < 0 || phases < KNN_PHASE_ALL || phases > KNN_PHASE_MERGE) {
        set_error("%s: seg_cols = %lld below 0 or phases = %d outside [0, 2]", who, (long long)seg_cols, phases);
        return MMVAE_E_BADARG;
    }
    if (int rc = check_aligned(who, "workspace", ws, sizeof(double))) return rc;
    if (seg_cols == 0) seg_cols = knn_seg_cols(nq, nr, k);
    const size_t need = knn_ws_bytes(nq, nr, k, seg_cols);
    if (need == 0 || need > KNN_WS_BYTES) {
        set_error("%s: segments of %lld columns need a workspace above %zu bytes", who, (long long)seg_cols, KNN_WS_BYTES);
        return MMVAE_E_UNSUPPORTED;
    }
    if (int rc = check_ws(who, ws_bytes, need)) return rc;
    return launch_knn(q, ldq, nq, r, ldr, nr, d, k, qgroup, rgroup, seg_cols, ws, idx, dist2, phases,
                      reinterpret_cast<hipStream_t>(stream));
}

int mmvae_knn(const float* q, int64_t ldq, int64_t nq, const float* r, int64_t ldr, int64_t nr, int d, int k, const int32_t* qgroup,
              const int32_t* rgroup, void* ws, size_t ws_bytes, int32_t* idx, float* dist2, void* stream) {
    return knn_checked(q, ldq, nq, r, ldr, nr, d, k, qgroup, rgroup, ws, ws_bytes, idx, dist2, 0, KNN_PHASE_ALL, stream);
}

int mmvae_debug_knn(const float* q, int64_t ldq, int64_t nq, const float* r, int64_t ldr, int64_t nr, int d, int k,
                    const int32_t* qgroup, const int32_t* rgroup, void* ws, size_t ws_bytes, int32_t* idx, float* dist2,
                    int64_t seg_cols, int phases, void* stream) {
    return knn_checked(q, ldq, nq, r, ldr, nr, d, k, qgroup, rgroup, ws, ws_bytes, idx, dist2, seg_cols, phases, stream);
}

int mmvae_knn_votes(const int32_t* idx, int64_t nq, int k, const int32_t* rlabel, int64_t nr, int n_classes, const int32_t* qlabel,
                    int32_t* pred, double* purity, int32_t* top2, void* stream) {
    const char* who = "knn_votes";
    if (!idx || !rlabel || !pred) { set_error("%s: null pointer", who); return MMVAE_E_BADARG; }
    if (purity && !qlabel) { set_error("%s: purity needs qlabel", who); return MMVAE_E_BADARG; }
    if (int rc = knn_extents(who, k, "n_classes", n_classes, KNN_MAX_CLASSES, nq, nr)) return rc;
    return launch_knn_votes(idx, nq, k, rlabel, nr, n_classes, qlabel, pred, purity, top2, reinterpret_cast<hipStream_t>(stream));
}

// ---- Gaussian classifiers (gaussclf.hip) ----
size_t mmvae_group_moments_workspace_bytes(int64_t n, int d, int G) {
    if (n < 1 || n > N_MAX || d < 1 || d > GC_MAX_D || G < 1 || G > GC_MAX_G) return 0;
    return seg_ws_bytes(nseg_max(n, G, GC_SEG_ROWS), d * (d + 3) / 2, G);
}

// dclass: -1 the launcher's rule (the first instance of GC_DC that holds d), 0 .. GC_N_DC - 1 that instance
static int group_moments_checked(const float* x, int64_t ld, int64_t n, int d, const int64_t* offsets, int G, const float* pivot,
                                 void* ws, size_t ws_bytes, double* s, double* M, int dclass, void* stream) {
    const char* who = "group_moments";
    if (!x || !offsets || !pivot || !ws || !s || !M) { set_error("%s: null pointer", who); return MMVAE_E_BADARG; }
    if (int rc = check_count(who, "n", n, 1, N_MAX)) return rc;
    if (int rc = check_count(who, "d", d, 1, INT32_MAX)) return rc;
    if (int rc = check_count(who, "G", G, 1, INT32_MAX)) return rc;
    if (int rc = check_pitch(who, "ld", ld, "d", d)) return rc;
    if (int rc = check_aligned(who, "workspace", ws, sizeof(double))) return rc;
    if (int rc = check_count(who, "dclass", dclass, -1, GC_N_DC - 1)) return rc;
    if (d > GC_MAX_D) { set_error("%s: d = %d above %d", who, d, GC_MAX_D); return MMVAE_E_UNSUPPORTED; }
    if (G > GC_MAX_G) { set_error("%s: G = %d above %d", who, G, GC_MAX_G); return MMVAE_E_UNSUPPORTED; }
    const size_t need = mmvae_group_moments_workspace_bytes(n, d, G);
    if (need == 0) { set_error("%s: n = %lld, d = %d, G = %d need a workspace size_t cannot hold", who, (long long)n, d, G); return MMVAE_E_UNSUPPORTED; }
    if (int rc = check_ws(who, ws_bytes, need)) return rc;
    if (dclass >= 0 && d > GC_DC[dclass]) {
        set_error("%s: the instance for d <= %d cannot run d = %d", who, GC_DC[dclass], d);
        return MMVAE_E_UNSUPPORTED;
    }
    return launch_group_moments(x, ld, n, d, offsets, G, pivot, ws, s, M, dclass < 0 ? gc_dclass(d) : dclass,
                                reinterpret_cast<hipStream_t>(stream));
}

int mmvae_group_moments(const float* x, int64_t ld, int64_t n, int d, const int64_t* offsets, int G, const float* pivot, void* ws,
                        size_t ws_bytes, double* s, double* M, void* stream) {
    return group_moments_checked(x, ld, n, d, offsets, G, pivot, ws, ws_bytes, s, M, -1, stream);
}

int mmvae_debug_group_moments(const float* x, int64_t ld, int64_t n, int d, const int64_t* offsets, int G, const float* pivot,
                              void* ws, size_t ws_bytes, double* s, double* M, int dclass, void* stream) {
    return group_moments_checked(x, ld, n, d, offsets, G, pivot, ws, ws_bytes, s, M, dclass, stream);
}

// the kernel keeps nothing between launches
size_t mmvae_gauss_scores_workspace_bytes(int64_t n, int d, int F, int K) {
    (void)n; (void)d; (void)F; (void)K;
    return 0;
}

int mmvae_gauss_scores(const float* x, int64_t ld, int64_t n, int d, const int32_t* model, int F, int K, const double* mu,
                       const double* W, const double* c0, const int64_t* perm, void* ws, size_t ws_bytes, int32_t* label,
                       double* best, double* second, double* scores, void* stream) {
    (void)ws_bytes;
    const char* who = "gauss_scores";
    if (!x || !model || !mu || !W || !c0 || !label || !best || !second) { set_error("%s: null pointer", who); return MMVAE_E_BADARG; }
    if (int rc = check_count(who, "n", n, 1, N_MAX)) return rc;
    if (int rc = check_count(who, "d", d, 1, INT32_MAX)) return rc;
    if (int rc = check_count(who, "F", F, 1, INT32_MAX)) return rc;
    if (int rc = check_count(who, "K", K, 1, INT32_MAX)) return rc;
    if (int rc = check_pitch(who, "ld", ld, "d", d)) return rc;
    if (int rc = check_aligned(who, "workspace", ws, sizeof(double))) return rc;     // (a null workspace is aligned)
    if (d > GC_MAX_D || K > GC_MAX_K || F > GC_MAX_F) {
        set_error("%s: d = %d, K = %d, F = %d above %d, %d, %d", who, d, K, F, GC_MAX_D, GC_MAX_K, GC_MAX_F);
        return MMVAE_E_UNSUPPORTED;
    }
    return launch_gauss_scores(x, ld, n, d, model, F, K, mu, W, c0, perm, label, best, second, scores,
                               reinterpret_cast<hipStream_t>(stream));
}

// ---- leaf posteriors merged up a tree (leafmerge.hip) ----
// the kernels keep nothing between launches
size_t mmvae_leaf_merge_workspace_bytes(int64_t n, int L, int T) {
    (void)n; (void)L; (void)T;
    return 0;
}

int mmvae_leaf_merge(double* p, int64_t ldp, int64_t n, int L, const int32_t* level_start, int T, const int32_t* start,
                     int64_t K_total, int K_max, const int32_t* leaf, int64_t nnz, void* ws, size_t ws_bytes, int32_t* label,
                     double* prob, double* second, double* merged, int K0, void* stream) {
    const char* who = "leaf_merge";
    if (!p || !level_start || !start || !leaf || !label || !prob) { set_error("%s: null pointer", who); return MMVAE_E_BADARG; }
    if (int rc = check_count(who, "n", n, 1, N_MAX)) return rc;
    if (int rc = check_count(who, "L", L, 1, INT32_MAX)) return rc;
    if (int rc = check_count(who, "T", T, 1, INT32_MAX)) return rc;
    if (int rc = check_count(who, "K_max", K_max, 1, INT32_MAX)) return rc;
    if (int rc = check_count(who, "K_total", K_total, 1, (int64_t)T * K_max)) return rc;
    if (int rc = check_count(who, "nnz", nnz, 0, INT64_MAX)) return rc;
    if (merged)
        if (int rc = check_count(who, "K0", K0, 1, K_max)) return rc;
    if (int rc = check_pitch(who, "ldp", ldp, "L", L)) return rc;
    if (int rc = check_aligned(who, "workspace", ws, sizeof(double))) return rc;     // (a null workspace is aligned)
    if (int rc = check_aligned(who, "p", p, sizeof(double))) return rc;
    if (int rc = check_aligned(who, "prob", prob, sizeof(double))) return rc;
    if (int rc = check_aligned(who, "second", second, sizeof(double))) return rc;
    if (int rc = check_aligned(who, "merged", merged, sizeof(double))) return rc;
    if (int rc = check_aligned(who, "label", label, sizeof(int32_t))) return rc;
    if (int rc = check_aligned(who, "level_start", level_start, sizeof(int32_t))) return rc;
    if (int rc = check_aligned(who, "start", start, sizeof(int32_t))) return rc;
    if (int rc = check_aligned(who, "leaf", leaf, sizeof(int32_t))) return rc;
    if (L > LM_MAX_L || K_max > LM_MAX_K || T > LM_MAX_T) {
        set_error("%s: L = %d, K_max = %d, T = %d above %d, %d, %d", who, L, K_max, T, LM_MAX_L, LM_MAX_K, LM_MAX_T);
        return MMVAE_E_UNSUPPORTED;
    }
    if (nnz > INT32_MAX) { set_error("%s: nnz = %lld at or above 2^31", who, (long long)nnz); return MMVAE_E_UNSUPPORTED; }
    if (int rc = check_ws(who, ws_bytes, mmvae_leaf_merge_workspace_bytes(n, L, T))) return rc;
    return launch_leaf_merge(p, ldp, n, L, level_start, T, start, (int)K_total, K_max, leaf, (int)nnz, label, prob, second, merged,
                             merged ? K0 : 0, reinterpret_cast<hipStream_t>(stream));
}

// ---- zero-inflated negative binomial inference (zinb.hip) ----
// what the three entries check alike: the extents, then the grid
static int zinb_extent(const char* who, int64_t N, int D) {
    if (int rc = check_count(who, "N", N, 1, N_MAX)) return rc;
    return check_count(who, "D", D, 1, INT32_MAX);
}

static int zinb_grid(const char* who, int64_t N, int D) {
    if (zb_tiles(N, D) > 0 && zb_ws_bytes(N, D) > 0) return 0;
    set_error("%s: N = %lld, D = %d need more than 2^31 - 1 tiles of 64 x 64", who, (long long)N, D);
    return MMVAE_E_UNSUPPORTED;
}

static int zinb_eps(const char* who, double eps) {
    if (eps >= 0.0 && eps < 1.0) return 0;
    set_error("%s: eps = %g outside [0, 1)", who, eps);
    return MMVAE_E_BADARG;
}

int mmvae_zinb_heads(const float* d10, int64_t ldh, int64_t N, int H, int D, const float* Wp, const float* bp, const float* Wr,
                     const float* br, float* x_p, float* x_r, int64_t ldo, void* stream) {
    const char* who = "zinb_heads";
    if (!d10 || !Wp || !bp || !Wr || !br || !x_p || !x_r) { set_error("%s: null pointer", who); return MMVAE_E_BADARG; }
    if (int rc = zinb_extent(who, N, D)) return rc;
    if (int rc = check_count(who, "H", H, 1, INT32_MAX)) return rc;
    if (int rc = check_pitch(who, "ldh", ldh, "H", H)) return rc;
    if (int rc = check_pitch(who, "ldo", ldo, "D", D)) return rc;
    if (H > ZB_MAX_H) { set_error("%s: H = %d above %d", who, H, ZB_MAX_H); return MMVAE_E_UNSUPPORTED; }
    if (int rc = zinb_grid(who, N, D)) return rc;
    return launch_zinb_heads(d10, ldh, N, H, D, Wp, bp, Wr, br, x_p, x_r, ldo, reinterpret_cast<hipStream_t>(stream));
}

size_t mmvae_zinb_nll_workspace_bytes(int64_t N, int D) {
    if (N < 1 || N > N_MAX || D < 1 || zb_tiles(N, D) == 0) return 0;
    return zb_ws_bytes(N, D);
}

size_t mmvae_zinb_terms_workspace_bytes(int64_t N, int D) { return mmvae_zinb_nll_workspace_bytes(N, D); }

int mmvae_zinb_nll(const float* d10, int64_t ldh, int64_t N, int H, int D, const float* W, const float* b, const float* Wp,
                   const float* bp, const float* Wr, const float* br, const float* X, int64_t ldx, double eps, void* ws,
                   size_t ws_bytes, double* cell_sum, double* gene_sum, void* stream) {
    const char* who = "zinb_nll";
    if (!d10 || !W || !b || !Wp || !bp || !Wr || !br || !X || !ws || !cell_sum || !gene_sum) {
        set_error("%s: null pointer", who);
        return MMVAE_E_BADARG;
    }
    if (int rc = zinb_extent(who, N, D)) return rc;
    if (int rc = check_count(who, "H", H, 1, INT32_MAX)) return rc;
    if (int rc = check_pitch(who, "ldh", ldh, "H", H)) return rc;
    if (int rc = check_pitch(who, "ldx", ldx, "D", D)) return rc;
    if (int rc = zinb_eps(who, eps)) return rc;
    if (int rc = check_aligned(who, "workspace", ws, sizeof(double))) return rc;
    if (H > ZB_MAX_H) { set_error("%s: H = %d above %d", who, H, ZB_MAX_H); return MMVAE_E_UNSUPPORTED; }
    if (int rc = zinb_grid(who, N, D)) return rc;
    if (int rc = check_ws(who, ws_bytes, mmvae_zinb_nll_workspace_bytes(N, D))) return rc;
    const ZinbIn in{d10, ldh, N, H, D, {{W, Wp, Wr}, {b, bp, br}}, X, ldx, eps, 0.0, 7, 0};
    return launch_zinb_nll(in, ws, cell_sum, gene_sum, reinterpret_cast<hipStream_t>(stream));
}

int mmvae_zinb_terms(const float* x_rec, int64_t ld_rec, const float* x_p, int64_t ld_p, const float* x_r, int64_t ld_r, const float* X,
                     int64_t ldx, int64_t N, int D, double eps, void* ws, size_t ws_bytes, double* cell_sum, double* gene_sum,
                     float* terms, int64_t ld_t, void* stream) {
    const char* who = "zinb_terms";
    if (!x_rec || !x_p || !x_r || !X || !ws || !cell_sum || !gene_sum) { set_error("%s: null pointer", who); return MMVAE_E_BADARG; }
    if (int rc = zinb_extent(who, N, D)) return rc;
    if (int rc = check_pitch(who, "ld_rec", ld_rec, "D", D)) return rc;
    if (int rc = check_pitch(who, "ld_p", ld_p, "D", D)) return rc;
    if (int rc = check_pitch(who, "ld_r", ld_r, "D", D)) return rc;
    if (int rc = check_pitch(who, "ldx", ldx, "D", D)) return rc;
    if (terms)
        if (int rc = check_pitch(who, "ld_t", ld_t, "D", D)) return rc;
    if (int rc = zinb_eps(who, eps)) return rc;
    if (int rc = check_aligned(who, "workspace", ws, sizeof(double))) return rc;
    if (int rc = zinb_grid(who, N, D)) return rc;
    if (int rc = check_ws(who, ws_bytes, mmvae_zinb_terms_workspace_bytes(N, D))) return rc;
    return launch_zinb_terms(x_rec, ld_rec, x_p, ld_p, x_r, ld_r, X, ldx, N, D, eps, ws, cell_sum, gene_sum, terms, ld_t,
                             reinterpret_cast<hipStream_t>(stream));
}

// ---- gradients of the ZINB term with respect to the heads (zinb_grad.hip) ----
static int zinb_scale(const char* who, double scale) {
    if (std::isfinite(scale)) return 0;
    set_error("%s: scale = %g is not finite", who, scale);
    return MMVAE_E_BADARG;
}

size_t mmvae_zinb_head_grads_workspace_bytes(int64_t N, int D, int H, int segments) {
    if (N < 1 || N > N_MAX || D < 1 || H < 1 || H > ZB_MAX_H || segments < 0 || zb_tiles(N, D) == 0 || zg_tiles(N, D, segments) == 0) return 0;
    return zg_ws_bytes(N, D, H, segments);
}

int mmvae_zinb_head_grads_segments(int64_t N, int D, int segments) {
    if (N < 1 || N > N_MAX || D < 1 || segments < 0) return 0;
    return zg_segments(N, D, segments, nullptr);
}

// What the three gradient entries check, in one order: `heads` for an entry that writes dW, db and the term's sums, `d10` for
// one that writes gd10; ws_fn is the entry's own workspace function.
static int zinb_grad_checks(const char* who, bool heads, bool d10, const ZinbIn& in, const void* ws, size_t ws_bytes,
                            size_t (*ws_fn)(int64_t, int, int, int), const ZinbGradOut& out) {
    const ZbHeads<3>& hd = in.hd;
    if (!in.d10 || !hd.W[0] || !hd.b[0] || !hd.W[1] || !hd.b[1] || !hd.W[2] || !hd.b[2] || !in.X || !ws ||
        (heads && (!out.cell_sum || !out.gene_sum)) || (d10 && !out.gd10)) {
        set_error("%s: null pointer", who);
        return MMVAE_E_BADARG;
    }
    if (int rc = check_count(who, "head_mask", in.mask, 1, 7)) return rc;
    for (int j = 0; heads && j < 3; ++j)
        if ((in.mask >> j & 1) && (!out.dW[j] || !out.db[j])) { set_error("%s: null pointer (a selected head's output)", who); return MMVAE_E_BADARG; }
    if (int rc = zinb_extent(who, in.N, in.D)) return rc;
    if (int rc = check_count(who, "H", in.H, 1, INT32_MAX)) return rc;
    if (int rc = check_count(who, "segments", in.segments, 0, INT32_MAX)) return rc;
    if (int rc = check_pitch(who, "ldh", in.ldh, "H", in.H)) return rc;
    if (int rc = check_pitch(who, "ldx", in.ldx, "D", in.D)) return rc;
    if (d10)
        if (int rc = check_pitch(who, "ldg", out.ldg, "H", in.H)) return rc;
    if (int rc = zinb_eps(who, in.eps)) return rc;
    if (int rc = zinb_scale(who, in.scale)) return rc;
    if (int rc = check_aligned(who, "workspace", ws, sizeof(double))) return rc;
    if (in.H > ZB_MAX_H) { set_error("%s: H = %d above %d", who, in.H, ZB_MAX_H); return MMVAE_E_UNSUPPORTED; }
    if (int rc = zinb_grid(who, in.N, in.D)) return rc;
    const size_t need = ws_fn(in.N, in.D, in.H, in.segments);
    if (need == 0) {
        set_error("%s: N = %lld, D = %d with %d segments need more than 2^31 - 1 workgroups", who, (long long)in.N, in.D, in.segments);
        return MMVAE_E_UNSUPPORTED;
    }
    return check_ws(who, ws_bytes, need);
}

int mmvae_zinb_head_grads(const float* d10, int64_t ldh, int64_t N, int H, int D, const float* W, const float* b, const float* Wp,
                          const float* bp, const float* Wr, const float* br, const float* X, int64_t ldx, double eps, double scale,
                          int head_mask, int segments, void* ws, size_t ws_bytes, float* dW, float* db, float* dWp, float* dbp,
                          float* dWr, float* dbr, double* cell_sum, double* gene_sum, void* stream) {
    const ZinbIn in{d10, ldh, N, H, D, {{W, Wp, Wr}, {b, bp, br}}, X, ldx, eps, scale, head_mask, segments};
    const ZinbGradOut out{{dW, dWp, dWr}, {db, dbp, dbr}, cell_sum, gene_sum, nullptr, 0};
    if (int rc = zinb_grad_checks("zinb_head_grads", true, false, in, ws, ws_bytes, mmvae_zinb_head_grads_workspace_bytes, out)) return rc;
    return launch_zinb_head_grads(in, ws, out, reinterpret_cast<hipStream_t>(stream));
}

// ---- the gradient with respect to d10, and the decoder trunk's backward (zinb_grad.hip, zinb_trunk.hip) ----
size_t mmvae_zinb_d10_grad_workspace_bytes(int64_t N, int D, int H, int segments) {
    if (N < 1 || N > N_MAX || D < 1 || H < 1 || H > ZB_MAX_H || segments < 0 || zb_tiles(N, D) == 0 || zd_tiles(N, D, segments) == 0) return 0;
    return zd_ws_bytes(N, D, H, segments);
}

int mmvae_zinb_d10_grad_segments(int64_t N, int D, int segments) {
    if (N < 1 || N > N_MAX || D < 1 || segments < 0) return 0;
    return zd_segments(N, D, segments, nullptr);
}

int mmvae_zinb_d10_grad(const float* d10, int64_t ldh, int64_t N, int H, int D, const float* W, const float* b, const float* Wp,
                        const float* bp, const float* Wr, const float* br, const float* X, int64_t ldx, double eps, double scale,
                        int head_mask, int segments, void* ws, size_t ws_bytes, float* gd10, int64_t ldg, void* stream) {
    const ZinbIn in{d10, ldh, N, H, D, {{W, Wp, Wr}, {b, bp, br}}, X, ldx, eps, scale, head_mask, segments};
    const ZinbGradOut out{{}, {}, nullptr, nullptr, gd10, ldg};
    if (int rc = zinb_grad_checks("zinb_d10_grad", false, true, in, ws, ws_bytes, mmvae_zinb_d10_grad_workspace_bytes, out)) return rc;
    return launch_zinb_d10_grad(in, ws, gd10, ldg, reinterpret_cast<hipStream_t>(stream));
}

// ---- the heads' gradients and gd10 in one pass over g (zinb_grad.hip, k_zg_step) ----
size_t mmvae_zinb_step_grads_workspace_bytes(int64_t N, int D, int H, int segments) {
    if (mmvae_zinb_head_grads_workspace_bytes(N, D, H, segments) == 0) return 0;
    return zs_ws_bytes(N, D, H, segments);
}

int mmvae_zinb_step_grads(const float* d10, int64_t ldh, int64_t N, int H, int D, const float* W, const float* b, const float* Wp,
                          const float* bp, const float* Wr, const float* br, const float* X, int64_t ldx, double eps, double scale,
                          int head_mask, int segments, void* ws, size_t ws_bytes, float* dW, float* db, float* dWp, float* dbp,
                          float* dWr, float* dbr, double* cell_sum, double* gene_sum, float* gd10, int64_t ldg, void* stream) {
    const ZinbIn in{d10, ldh, N, H, D, {{W, Wp, Wr}, {b, bp, br}}, X, ldx, eps, scale, head_mask, segments};
    const ZinbGradOut out{{dW, dWp, dWr}, {db, dbp, dbr}, cell_sum, gene_sum, gd10, ldg};
    if (int rc = zinb_grad_checks("zinb_step_grads", true, true, in, ws, ws_bytes, mmvae_zinb_step_grads_workspace_bytes, out)) return rc;
    return launch_zinb_head_grads(in, ws, out, reinterpret_cast<hipStream_t>(stream));
}

size_t mmvae_decoder_trunk_grads_workspace_bytes(int64_t N, int Z, int L, int H, int segments) {
    if (N < 1 || N > N_MAX || Z < 1 || L < 1 || L > TR_MAX_W || H < 1 || H > TR_MAX_W || segments < 0 || segments > TR_MAX_SEG) return 0;
    return tr_ws_bytes(N, Z, L, H, segments);
}

int mmvae_decoder_trunk_grads_segments(int64_t N, int segments) {
    if (N < 1 || N > N_MAX || segments < 0 || segments > TR_MAX_SEG) return 0;
    return tr_segments(N, segments, nullptr);
}

int mmvae_decoder_trunk_grads(int64_t N, int Z, int L, int H, const float* const* act, const int64_t* ld, const float* const* params,
                              const float* gd10, int64_t ldg, int segments, void* ws, size_t ws_bytes, float* const* grads, float* gzin,
                              int64_t ldgz, void* stream) {
    const char* who = "decoder_trunk_grads";
    if (!act || !ld || !params || !gd10 || !ws || !grads) { set_error("%s: null pointer", who); return MMVAE_E_BADARG; }
    for (int l = 0; l < 6; ++l)
        if (!act[l]) { set_error("%s: null pointer (activation %d of zin, d6 .. d10)", who, l); return MMVAE_E_BADARG; }
    for (int t = 0; t < 10; ++t)
        if (!params[t] || !grads[t]) { set_error("%s: null pointer (tensor %d of fc6.weight .. fc10.bias)", who, t); return MMVAE_E_BADARG; }
    if (int rc = check_count(who, "N", N, 1, N_MAX)) return rc;
    if (int rc = check_count(who, "Z", Z, 1, INT32_MAX)) return rc;
    if (int rc = check_count(who, "L", L, 1, INT32_MAX)) return rc;
    if (int rc = check_count(who, "H", H, 1, INT32_MAX)) return rc;
    if (int rc = check_count(who, "segments", segments, 0, TR_MAX_SEG)) return rc;
    const int width[6] = {Z, L, H, H, H, H};
    static const char* const names[6] = {"zin", "d6", "d7", "d8", "d9", "d10"};
    for (int l = 0; l < 6; ++l)
        if (int rc = check_pitch(who, names[l], ld[l], "its width", width[l])) return rc;
    if (int rc = check_pitch(who, "ldg", ldg, "H", H)) return rc;
    if (gzin)
        if (int rc = check_pitch(who, "ldgz", ldgz, "Z", Z)) return rc;
    if (int rc = check_aligned(who, "workspace", ws, sizeof(double))) return rc;
    if (H > TR_MAX_W || L > TR_MAX_W) { set_error("%s: H = %d, L = %d above %d", who, H, L, TR_MAX_W); return MMVAE_E_UNSUPPORTED; }
    const size_t need = mmvae_decoder_trunk_grads_workspace_bytes(N, Z, L, H, segments);
    if (need == 0) { set_error("%s: N = %lld, Z = %d, L = %d, H = %d: no size_t holds the workspace", who, (long long)N, Z, L, H); return MMVAE_E_UNSUPPORTED; }
    if (int rc = check_ws(who, ws_bytes, need)) return rc;
    const float* W[5];
    for (int l = 0; l < 5; ++l) W[l] = params[2 * l];
    return launch_decoder_trunk_grads(N, Z, L, H, act, ld, W, gd10, ldg, segments, ws, grads, gzin, ldgz, reinterpret_cast<hipStream_t>(stream));
}

int mmvae_zinb_terms_grad(const float* x_rec, int64_t ld_rec, const float* x_p, int64_t ld_p, const float* x_r, int64_t ld_r,
                          const float* X, int64_t ldx, int64_t N, int D, double eps, double scale, float* g_rec, float* g_p, float* g_r,
                          int64_t ld_g, void* stream) {
    const char* who = "zinb_terms_grad";
    if (!x_rec || !x_p || !x_r || !X || !g_rec || !g_p || !g_r) { set_error("%s: null pointer", who); return MMVAE_E_BADARG; }
    if (int rc = zinb_extent(who, N, D)) return rc;
    if (int rc = check_pitch(who, "ld_rec", ld_rec, "D", D)) return rc;
    if (int rc = check_pitch(who, "ld_p", ld_p, "D", D)) return rc;
    if (int rc = check_pitch(who, "ld_r", ld_r, "D", D)) return rc;
    if (int rc = check_pitch(who, "ldx", ldx, "D", D)) return rc;
    if (int rc = check_pitch(who, "ld_g", ld_g, "D", D)) return rc;
    if (int rc = zinb_eps(who, eps)) return rc;
    if (int rc = zinb_scale(who, scale)) return rc;
    if (int rc = zinb_grid(who, N, D)) return rc;
    return launch_zinb_terms_grad(x_rec, ld_rec, x_p, ld_p, x_r, ld_r, X, ldx, N, D, eps, scale, g_rec, g_p, g_r, ld_g,
                                  reinterpret_cast<hipStream_t>(stream));
}

int mmvae_debug_zinb_grad_host(int64_t n, const float* X, const float* a_rec, const float* a_p, const float* a_r, double eps, double* g,
                               double* term) {
    const char* who = "debug_zinb_grad_host";
    if (!X || !a_rec || !a_p || !a_r || !g) { set_error("%s: null pointer", who); return MMVAE_E_BADARG; }
    if (int rc = check_count(who, "n", n, 1, INT64_MAX)) return rc;
    if (int rc = zinb_eps(who, eps)) return rc;
    host_zinb_grad(n, X, a_rec, a_p, a_r, eps, g, term);
    return 0;
}

int mmvae_debug_digamma_host(int64_t n, const double* x, double* out) {
    const char* who = "debug_digamma_host";
    if (!x || !out) { set_error("%s: null pointer", who); return MMVAE_E_BADARG; }
    if (int rc = check_count(who, "n", n, 1, INT64_MAX)) return rc;
    host_digamma(n, x, out);
    return 0;
}

// ---- count distributions (countdist.hip) ----
// a pitch of 0 reads a vector [D] where vec_ok says so
static int cd_pitch(const char* who, const char* ldname, int64_t ld, int D, bool vec_ok) {
    if (vec_ok && ld == 0) return 0;
    return check_pitch(who, ldname, ld, "D", D);
}

static int count_logp_check(const char* who, const mmvae_count_logp_t* a) {
    if (!a) { set_error("%s: null pointer", who); return MMVAE_E_BADARG; }
    if (int rc = check_count(who, "kind", a->kind, 0, 2)) return rc;
    if (!a->x || !a->mu || !a->theta || (a->kind != 0 && !a->pi) || (a->kind == 2 && !a->mu2)) {
        set_error("%s: null pointer", who);
        return MMVAE_E_BADARG;
    }
    if (int rc = zinb_extent(who, a->N, a->D)) return rc;
    if (int rc = cd_pitch(who, "ldx", a->ldx, a->D, false)) return rc;
    if (int rc = cd_pitch(who, "ld_mu", a->ld_mu, a->D, false)) return rc;
    if (int rc = cd_pitch(who, "ld_theta", a->ld_theta, a->D, true)) return rc;
    if (a->kind != 0)
        if (int rc = cd_pitch(who, "ld_pi", a->ld_pi, a->D, false)) return rc;
    if (a->kind == 2) {
        if (int rc = cd_pitch(who, "ld_mu2", a->ld_mu2, a->D, false)) return rc;
        if (a->theta2)
            if (int rc = cd_pitch(who, "ld_theta2", a->ld_theta2, a->D, true)) return rc;
    }
    if (a->terms)
        if (int rc = cd_pitch(who, "ld_t", a->ld_t, a->D, false)) return rc;
    return zinb_eps(who, a->eps);
}

size_t mmvae_count_logp_workspace_bytes(int64_t N, int D) { return mmvae_zinb_nll_workspace_bytes(N, D); }

int mmvae_count_logp(const mmvae_count_logp_t* a, void* ws, size_t ws_bytes, void* stream) {
    const char* who = "count_logp";
    if (int rc = count_logp_check(who, a)) return rc;
    if (!a->cell_sum != !a->gene_sum) { set_error("%s: cell_sum and gene_sum come together", who); return MMVAE_E_BADARG; }
    if (!a->terms && !a->cell_sum) { set_error("%s: neither terms nor sums are wanted", who); return MMVAE_E_BADARG; }
    if (a->cell_sum) {
        if (!ws) { set_error("%s: null pointer", who); return MMVAE_E_BADARG; }
        if (int rc = check_aligned(who, "workspace", ws, sizeof(double))) return rc;
    }
    if (int rc = zinb_grid(who, a->N, a->D)) return rc;
    if (a->cell_sum)
        if (int rc = check_ws(who, ws_bytes, mmvae_count_logp_workspace_bytes(a->N, a->D))) return rc;
    return launch_count_logp(*a, ws, reinterpret_cast<hipStream_t>(stream));
}

int mmvae_debug_count_logp_host(const mmvae_count_logp_t* a) {
    const char* who = "debug_count_logp_host";
    if (int rc = count_logp_check(who, a)) return rc;
    if (!a->terms) { set_error("%s: null pointer", who); return MMVAE_E_BADARG; }
    host_count_logp(*a);
    return 0;
}

// what the draws check alike; heads_given: a, b and zi are read (mmvae_zinb_sample forms them itself)
static int count_sample_check(const char* who, const mmvae_count_sample_t* s, bool heads_given) {
    if (!s) { set_error("%s: null pointer", who); return MMVAE_E_BADARG; }
    if (int rc = check_count(who, "param", s->param, 0, 1)) return rc;
    if (int rc = check_count(who, "zi_kind", s->zi_kind, 0, 2)) return rc;
    const bool zi = s->param == 1 || s->zi_kind != 0;
    if (!s->out || !s->exhausted || (heads_given && (!s->a || !s->b || (zi && !s->zi)))) {
        set_error("%s: null pointer", who);
        return MMVAE_E_BADARG;
    }
    if (int rc = zinb_extent(who, s->N, s->D)) return rc;
    if (heads_given) {
        if (int rc = cd_pitch(who, "ld_a", s->ld_a, s->D, false)) return rc;
        if (int rc = cd_pitch(who, "ld_b", s->ld_b, s->D, s->param == 0)) return rc;
        if (zi)
            if (int rc = cd_pitch(who, "ld_zi", s->ld_zi, s->D, false)) return rc;
    }
    if (int rc = cd_pitch(who, "ld_out", s->ld_out, s->D, false)) return rc;
    if (s->cell0 < 0 || (unsigned __int128)((uint64_t)s->cell0 + (uint64_t)s->N) * (unsigned __int128)s->D >= ((unsigned __int128)1 << 63)) {
        set_error("%s: cell0 = %lld with N = %lld, D = %d leaves the 63-bit element index", who, (long long)s->cell0, (long long)s->N, s->D);
        return MMVAE_E_BADARG;
    }
    if (s->offset >> 56) { set_error("%s: offset = %llu not below 2^56", who, (unsigned long long)s->offset); return MMVAE_E_BADARG; }
    if (s->out_int32 && s->log1p) { set_error("%s: log1p needs the float32 output", who); return MMVAE_E_BADARG; }
    return s->param == 1 ? zinb_eps(who, s->eps) : 0;
}

int mmvae_count_sample(const mmvae_count_sample_t* s, void* stream) {
    if (int rc = count_sample_check("count_sample", s, true)) return rc;
    return launch_count_sample(*s, reinterpret_cast<hipStream_t>(stream));
}

int mmvae_debug_count_sample_host(const mmvae_count_sample_t* s) {
    if (int rc = count_sample_check("debug_count_sample_host", s, true)) return rc;
    host_count_sample(*s);
    return 0;
}

int mmvae_zinb_sample(const float* d10, int64_t ldh, int H, const float* W, const float* b, const float* Wp, const float* bp,
                      const float* Wr, const float* br, const mmvae_count_sample_t* s, void* stream) {
    const char* who = "zinb_sample";
    if (!d10 || !W || !b || !Wp || !bp || !Wr || !br) { set_error("%s: null pointer", who); return MMVAE_E_BADARG; }
    if (int rc = count_sample_check(who, s, false)) return rc;
    if (s->param != 1) { set_error("%s: param = %d, the heads' mapping (1) is the only one", who, s->param); return MMVAE_E_BADARG; }
    if (int rc = check_count(who, "H", H, 1, INT32_MAX)) return rc;
    if (int rc = check_pitch(who, "ldh", ldh, "H", H)) return rc;
    if (H > ZB_MAX_H) { set_error("%s: H = %d above %d", who, H, ZB_MAX_H); return MMVAE_E_UNSUPPORTED; }
    if (int rc = zinb_grid(who, s->N, s->D)) return rc;
    return launch_zinb_sample(d10, ldh, H, W, b, Wp, bp, Wr, br, *s, reinterpret_cast<hipStream_t>(stream));
}

// ---- random forest on 256-bin features (forest.hip) ----
size_t mmvae_forest_workspace_bytes(int64_t n, int d, int F, int K, int T) {
    if (n < 2 || n > RF_MAX_N || d < 1 || d > RF_MAX_D || F < 2 || F > RF_MAX_F || K < 2 || K > RF_MAX_K || T < 1 || T > RF_MAX_T)
        return 0;
    return rf_ws_bytes(n, F, K, T);
}

int mmvae_forest_cv(const uint8_t* bins, int64_t ld, int64_t n, int d, const int32_t* codes, const int32_t* fold, int K, int F, int T,
                    int mtry, uint64_t seed, void* ws, size_t ws_bytes, int32_t* label, int32_t* best, int32_t* second,
                    int32_t* votes, int32_t* tree_count, int32_t* tree_nodes, void* stream) {
    const char* who = "forest_cv";
    if (!bins || !codes || !fold || !ws || !label || !best || !second) { set_error("%s: null pointer", who); return MMVAE_E_BADARG; }
    if (!tree_count != !tree_nodes) { set_error("%s: tree_count and tree_nodes go together", who); return MMVAE_E_BADARG; }
    if (int rc = check_count(who, "n", n, 2, INT64_MAX)) return rc;
    if (int rc = check_count(who, "d", d, 1, INT32_MAX)) return rc;
    if (int rc = check_count(who, "K", K, 2, INT32_MAX)) return rc;
    if (int rc = check_count(who, "F", F, 2, INT32_MAX)) return rc;
    if (int rc = check_count(who, "T", T, 1, INT32_MAX)) return rc;
    if (int rc = check_count(who, "mtry", mtry, 1, d)) return rc;
    if (int rc = check_pitch(who, "ld", ld, "d", d)) return rc;
    if (int rc = check_aligned(who, "workspace", ws, 16)) return rc;
    if (n > RF_MAX_N || d > RF_MAX_D || K > RF_MAX_K || F > RF_MAX_F || T > RF_MAX_T) {
        set_error("%s: n = %lld, d = %d, K = %d, F = %d, T = %d above %lld, %d, %d, %d, %d", who, (long long)n, d, K, F, T,
                  (long long)RF_MAX_N, RF_MAX_D, RF_MAX_K, RF_MAX_F, RF_MAX_T);
        return MMVAE_E_UNSUPPORTED;
    }
    if (int rc = check_ws(who, ws_bytes, mmvae_forest_workspace_bytes(n, d, F, K, T))) return rc;
    return launch_forest(bins, ld, n, d, codes, fold, K, F, T, mtry, seed, ws, label, best, second, votes, tree_count, tree_nodes,
                         reinterpret_cast<hipStream_t>(stream));
}

// ---- principal components (pca.hip) ----
int mmvae_gram_segments(int64_t n, int D, int64_t* seg_rows) {
    if (n < 2 || n > N_MAX || D < 1 || D > GRAM_MAX_D) return 0;
    return gram_segments(n, D, seg_rows);
}

size_t mmvae_gram_workspace_bytes(int64_t n, int D) {
    const int nseg = mmvae_gram_segments(n, D, nullptr);
    if (nseg == 0) return 0;
    return sizeof(double) * ((size_t)(nseg - 1) * (size_t)D * (size_t)D + (size_t)nseg * (size_t)D);
}

static int gram_checked(const float* data, int64_t ld, int64_t n_total, const int64_t* rows, int64_t n, int D, const float* pivot,
                        void* ws, size_t ws_bytes, double* s, double* G, int cov, int path, void* stream) {
    const char* who = "gram";
    if (!data || !pivot || !ws || !s || !G) { set_error("%s: null pointer", who); return MMVAE_E_BADARG; }
    if (int rc = check_count(who, "n", n, 2, N_MAX)) return rc;
    if (int rc = check_rowmap(who, rows, n, n_total)) return rc;
    if (int rc = check_count(who, "D", D, 1, INT32_MAX)) return rc;
    if (int rc = check_pitch(who, "ld", ld, "D", D)) return rc;
    if (int rc = check_aligned(who, "workspace", ws, sizeof(double))) return rc;
    if (int rc = check_count(who, "cov", cov, 0, 1)) return rc;
    if (int rc = check_count(who, "path", path, -1, 1)) return rc;      // (before the limits below: a bad argument first)
    if (D > GRAM_MAX_D) { set_error("%s: D = %d above %d", who, D, GRAM_MAX_D); return MMVAE_E_UNSUPPORTED; }
    if (int rc = check_ws(who, ws_bytes, mmvae_gram_workspace_bytes(n, D))) return rc;
    bool wide;
    if (int rc = pick_wide(who, path, data, ld, sizeof(float), &wide)) return rc;
    return launch_gram(data, ld, n_total, rows, n, D, pivot, ws, s, G, cov, wide, reinterpret_cast<hipStream_t>(stream));
}

int mmvae_gram(const float* data, int64_t ld, int64_t n_total, const int64_t* rows, int64_t n, int D, const float* pivot, void* ws,
               size_t ws_bytes, double* s, double* G, int cov, void* stream) {
    return gram_checked(data, ld, n_total, rows, n, D, pivot, ws, ws_bytes, s, G, cov, -1, stream);
}

int mmvae_debug_gram(const float* data, int64_t ld, int64_t n_total, const int64_t* rows, int64_t n, int D, const float* pivot,
                     void* ws, size_t ws_bytes, double* s, double* G, int cov, int path, void* stream) {
    return gram_checked(data, ld, n_total, rows, n, D, pivot, ws, ws_bytes, s, G, cov, path, stream);
}

// the kernel keeps nothing between launches
size_t mmvae_symm_mul_workspace_bytes(int D, int b) {
    (void)D; (void)b;
    return 0;
}

int mmvae_symm_mul(const double* C, int64_t ldc, int D, const double* Q, int b, double* Y, void* stream) {
    const char* who = "symm_mul";
    if (!C || !Q || !Y) { set_error("%s: null pointer", who); return MMVAE_E_BADARG; }
    if (int rc = check_count(who, "D", D, 1, INT32_MAX)) return rc;
    if (int rc = check_count(who, "b", b, 1, INT32_MAX)) return rc;
    if (int rc = check_pitch(who, "ldc", ldc, "D", D)) return rc;
    if (D > GRAM_MAX_D || b > RM_CHUNK) { set_error("%s: D = %d, b = %d above %d, %d", who, D, b, GRAM_MAX_D, RM_CHUNK); return MMVAE_E_UNSUPPORTED; }
    return launch_symm_mul(C, ldc, D, Q, b, Y, reinterpret_cast<hipStream_t>(stream));
}

size_t mmvae_pca_project_workspace_bytes(int64_t n, int D, int k) {
    (void)n; (void)D; (void)k;
    return 0;
}

int mmvae_pca_project(const float* data, int64_t ld, int64_t n_total, const int64_t* rows, int64_t n, int D, const double* mean,
                      const double* V, int k, double* Z, void* stream) {
    const char* who = "pca_project";
    if (!data || !mean || !V || !Z) { set_error("%s: null pointer", who); return MMVAE_E_BADARG; }
    if (int rc = check_count(who, "n", n, 1, N_MAX)) return rc;
    if (int rc = check_rowmap(who, rows, n, n_total)) return rc;
    if (int rc = check_count(who, "D", D, 1, INT32_MAX)) return rc;
    if (int rc = check_count(who, "k", k, 1, INT32_MAX)) return rc;
    if (int rc = check_pitch(who, "ld", ld, "D", D)) return rc;
    if (k > RM_CHUNK) { set_error("%s: k = %d above %d", who, k, RM_CHUNK); return MMVAE_E_UNSUPPORTED; }
    return launch_pca_project(data, ld, n_total, rows, n, D, mean, V, k, Z, reinterpret_cast<hipStream_t>(stream));
}

// ---- data preparation (dataprep.hip) ----
static int cpm_vsize(int vtype) { return vtype == 2 ? 8 : 4; }

// what mmvae_cpm_dense and mmvae_cpm_csr check alike.  vtype 0 int32, 1 float, 2 double; otype 0 float, 1 double; mode 0
// normalise, 1 log1p
static int cpm_common_checked(const char* who, int vtype, int64_t n_total, int G, const int64_t* rows, int64_t n, int ng,
                              double scaler, int mode, const void* out, int otype, const double* norms) {
    if (!out || !norms) { set_error("%s: null pointer", who); return MMVAE_E_BADARG; }
    if (int rc = check_count(who, "value type", vtype, 0, 2)) return rc;
    if (int rc = check_count(who, "output type", otype, 0, 1)) return rc;
    if (int rc = check_count(who, "mode", mode, 0, 1)) return rc;
    if (int rc = check_count(who, "n", n, 1, N_MAX - 1)) return rc;
    if (int rc = check_rowmap(who, rows, n, n_total)) return rc;
    if (int rc = check_count(who, "G", G, 1, INT32_MAX)) return rc;
    if (int rc = check_count(who, "ng", ng, 1, INT32_MAX)) return rc;
    if (!(scaler == scaler) || scaler - scaler != 0.0) { set_error("%s: scaler = %g is not finite", who, scaler); return MMVAE_E_BADARG; }
    if (G > CPM_MAX_G || ng > CPM_MAX_G) { set_error("%s: G = %d, ng = %d above %d", who, G, ng, CPM_MAX_G); return MMVAE_E_UNSUPPORTED; }
    return 0;
}

static int cpm_dense_checked(const void* x, int vtype, int64_t ld, int64_t n_total, int G, const int64_t* rows, int64_t n,
                             const int32_t* genes, int ng, double scaler, int mode, void* out, int otype, double* norms, int path,
                             void* stream) {
    const char* who = "cpm_dense";
    if (!x) { set_error("%s: null pointer", who); return MMVAE_E_BADARG; }
    if (int rc = cpm_common_checked(who, vtype, n_total, G, rows, n, ng, scaler, mode, out, otype, norms)) return rc;
    if (int rc = check_pitch(who, "ld", ld, "G", G)) return rc;
    if (!genes && ng != G) { set_error("%s: ng = %d without a gene list must be G = %d", who, ng, G); return MMVAE_E_BADARG; }
    if (int rc = check_aligned(who, "x", x, cpm_vsize(vtype))) return rc;
    bool wide;
    if (int rc = pick_wide(who, path, x, ld, cpm_vsize(vtype), &wide)) return rc;
    return launch_cpm_dense(x, vtype, ld, n_total, G, rows, n, genes, ng, scaler, mode, out, otype, norms, wide,
                            reinterpret_cast<hipStream_t>(stream));
}

int mmvae_cpm_dense(const void* x, int vtype, int64_t ld, int64_t n_total, int G, const int64_t* rows, int64_t n, const int32_t* genes,
                    int ng, double scaler, int mode, void* out, int otype, double* norms, void* stream) {
    return cpm_dense_checked(x, vtype, ld, n_total, G, rows, n, genes, ng, scaler, mode, out, otype, norms, -1, stream);
}

int mmvae_debug_cpm_dense(const void* x, int vtype, int64_t ld, int64_t n_total, int G, const int64_t* rows, int64_t n,
                          const int32_t* genes, int ng, double scaler, int mode, void* out, int otype, double* norms, int path,
                          void* stream) {
    return cpm_dense_checked(x, vtype, ld, n_total, G, rows, n, genes, ng, scaler, mode, out, otype, norms, path, stream);
}

int mmvae_cpm_csr(const int64_t* indptr, const int32_t* indices, const void* data, int vtype, int64_t nnz, int64_t n_total, int G,
                  const int64_t* rows, int64_t n, const int32_t* inv, int ng, double scaler, int mode, void* out, int otype,
                  double* norms, void* stream) {
    const char* who = "cpm_csr";
    if (!indptr || !inv) { set_error("%s: null pointer", who); return MMVAE_E_BADARG; }
    if (int rc = check_count(who, "nnz", nnz, 0, INT64_MAX)) return rc;
    if (nnz > 0 && (!indices || !data)) { set_error("%s: null indices / data with nnz = %lld", who, (long long)nnz); return MMVAE_E_BADARG; }
    if (int rc = cpm_common_checked(who, vtype, n_total, G, rows, n, ng, scaler, mode, out, otype, norms)) return rc;
    if (int rc = check_count(who, "ng", ng, 1, G)) return rc;
    return launch_cpm_csr(indptr, indices, data, vtype, nnz, n_total, G, rows, n, inv, ng, scaler, mode, out, otype, norms,
                          reinterpret_cast<hipStream_t>(stream));
}

static bool gs_shape_ok(int64_t n, int D) {
    return (unsigned __int128)gs_nseg(n) * (unsigned __int128)cdiv64(D, GS_TILE) <= (unsigned __int128)GS_MAX_BLOCKS;
}

size_t mmvae_gene_stats_workspace_bytes(int64_t n, int D) {
    if (n < 1 || n > N_MAX || D < 1 || !gs_shape_ok(n, D)) return 0;
    return bytes_or_0((unsigned __int128)8 * 3 * (unsigned __int128)gs_nseg(n) * (unsigned __int128)D);
}

// vtype 1 float, 2 double
static int gene_stats_checked(const void* data, int vtype, int64_t ld, int64_t n_total, int D, const int64_t* rows, int64_t n,
                              double eps, void* ws, size_t ws_bytes, int64_t* n_above, double* mean, double* sd, int path,
                              void* stream) {
    const char* who = "gene_stats";
    if (!data || !ws || !n_above || !mean || !sd) { set_error("%s: null pointer", who); return MMVAE_E_BADARG; }
    if (int rc = check_count(who, "value type", vtype, 1, 2)) return rc;
    if (int rc = check_count(who, "n", n, 1, N_MAX)) return rc;
    if (int rc = check_rowmap(who, rows, n, n_total)) return rc;
    if (int rc = check_count(who, "D", D, 1, INT32_MAX)) return rc;
    if (int rc = check_pitch(who, "ld", ld, "D", D)) return rc;
    if (!(eps == eps)) { set_error("%s: eps is NaN", who); return MMVAE_E_BADARG; }
    if (int rc = check_aligned(who, "workspace", ws, sizeof(double))) return rc;
    if (int rc = check_aligned(who, "data", data, cpm_vsize(vtype))) return rc;
    if (int rc = check_count(who, "path", path, -1, 1)) return rc;      // (before the limits below: a bad argument first)
    const size_t need = mmvae_gene_stats_workspace_bytes(n, D);
    if (need == 0) {
        set_error("%s: n = %lld, D = %d need a grid of more than %lld workgroups", who, (long long)n, D, (long long)GS_MAX_BLOCKS);
        return MMVAE_E_UNSUPPORTED;
    }
    if (int rc = check_ws(who, ws_bytes, need)) return rc;
    bool wide;
    if (int rc = pick_wide(who, path, data, ld, cpm_vsize(vtype), &wide)) return rc;
    return launch_gene_stats(data, vtype, ld, n_total, D, rows, n, eps, ws, n_above, mean, sd, wide,
                             reinterpret_cast<hipStream_t>(stream));
}

int mmvae_gene_stats(const void* data, int vtype, int64_t ld, int64_t n_total, int D, const int64_t* rows, int64_t n, double eps,
                     void* ws, size_t ws_bytes, int64_t* n_above, double* mean, double* sd, void* stream) {
    return gene_stats_checked(data, vtype, ld, n_total, D, rows, n, eps, ws, ws_bytes, n_above, mean, sd, -1, stream);
}

int mmvae_debug_gene_stats(const void* data, int vtype, int64_t ld, int64_t n_total, int D, const int64_t* rows, int64_t n, double eps,
                           void* ws, size_t ws_bytes, int64_t* n_above, double* mean, double* sd, int path, void* stream) {
    return gene_stats_checked(data, vtype, ld, n_total, D, rows, n, eps, ws, ws_bytes, n_above, mean, sd, path, stream);
}

}  // extern "C"

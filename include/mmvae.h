/*
 * mmvae.h -- C ABI of the MI355X-native cpl-mixVAE train-step engine (libmmvae_hip.so).
 *
 * The reference (AllenInstitute/distributed-vae) has no FFI / operator layer: its hot path is
 * plain PyTorch.  This header is therefore the boundary the build
 * *introduces*; each entry point names the reference code it replaces:
 *
 *   mmvae_forward      mixVAE_model.forward          mmidas/nn_model.py:297-368
 *                      (encoder :263-269, double softmax :337, gumbel_softmax :430-493,
 *                       intermed :271-275, reparameterize :413-428, decoder :277-287)
 *   mmvae_loss         mixVAE_model.loss             mmidas/nn_model.py:495-598 (helpers :39-86)
 *   mmvae_backward     _loss.backward()              mmidas/cpl_mixvae.py:462 (autograd of the above)
 *   mmvae_adam_step    optimizer.step()              mmidas/cpl_mixvae.py:274,:463; train.py:144-147
 *   mmvae_train_step   the per-batch driver          mmidas/cpl_mixvae.py:434-463
 *   mmvae_eval_classify / mmvae_confmat_accumulate / mmvae_consensus
 *                      the per-epoch consensus loop  mmidas/cpl_mixvae.py:563-657, _utils.py:79-129
 *   mmvae_augment      netA(x.expand(A,-1,-1), True, 0.1)  mmidas/cpl_mixvae.py:422-423, augmentation/udagan.py:281-329
 *   mmvae_decode       mixVAE_model.decoder(c, s, arm)     mmidas/nn_model.py:277-287
 *   mmvae_state_changes  mixVAE_model.state_changes(x, d_s, temp, n_samp)  mmidas/nn_model.py:370-411
 *   mmvae_encode       mixVAE_model.encoder(x, arm) and the latent block of forward(eval=True)  mmidas/nn_model.py:263-269, :330-351
 *   mmvae_intermed     mixVAE_model.intermed(y, arm)       mmidas/nn_model.py:271-275
 *   mmvae_prune_apply  prune.custom_from_mask / prune.remove on fcc, fc_mu, fc_sigma, fc6  mmidas/cpl_mixvae.py:1124-1128, :1153-1161, :1396-1401
 *
 * Conventions
 *   - plain pointers and sizes only; every buffer is caller-owned DEVICE memory (fp32 unless
 *     noted); the library never allocates or frees device memory, creates no streams or events and keeps no
 *     global mutable state besides the last error string (thread-local).  Everything a call needs beyond its
 *     arguments -- the optional second stream, the events that fork and join it, split factors, experiment
 *     switches -- travels in a caller-owned mmvae_exec passed to the call; two engines never share any.
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*), re-entrant, with no
 *     hidden synchronisation.
 *   - return value: 0 = ok, <0 = error (MMVAE_E_*); mmvae_last_error_string() explains.
 *   - layouts are row-major.  Parameters live in ONE flat fp32 buffer, arm-major:
 *     params[a * per_arm + offset[t]], t indexing the 28 tensors listed at mmvae_param_layout;
 *     weights keep PyTorch's [out, in] layout so state_dict tensors are views of the buffer.
 */
#ifndef MMVAE_H
#define MMVAE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MMVAE_OK 0
#define MMVAE_E_BADARG (-1)      /* null pointer, non-positive size ...                       */
#define MMVAE_E_UNSUPPORTED (-2) /* shape outside the kernels' limits (see mmvae_check_dims)  */
#define MMVAE_E_LAUNCH (-3)      /* hipLaunch / runtime failure                               */
#define MMVAE_E_WORKSPACE (-4)   /* workspace too small                                       */

#define MMVAE_MAX_ARMS 8
#define MMVAE_N_PARAM_TENSORS 28
#define MMVAE_N_BN 6

/* A arms, B cells per batch (this rank), D genes, H fc_dim, L lowD_dim, C n_categories,
 * S state_dim  (mixVAE_model.__init__, nn_model.py:112-134). */
typedef struct mmvae_dims {
    int32_t A, B, D, H, L, C, S;
} mmvae_dims;

typedef struct mmvae_hyper {
    float tau;         /* nn_model.py:337                                   */
    float temp;        /* Gumbel-softmax temperature, :455                  */
    float beta;        /* KL weight, :551                                   */
    float lam;         /* coupling weight, :581                             */
    float eps;         /* self.eps, also the BatchNorm eps, :211            */
    float bn_momentum; /* :211                                              */
    float x_drop;      /* input dropout p, :165/:264                        */
    float s_drop;      /* state dropout p, :166/:278                        */
    int32_t hard;      /* straight-through one-hot sample, :486-493         */
    int32_t training;  /* module.training: batch-stat BN + dropout active   */
    int32_t eval_flag; /* forward(eval=True): no Gumbel noise, hard sample, :340-343 */
    int32_t gemm_bf16; /* engine of the five D x H GEMMs (fc1, fc11, d(d10), dW1, dW11):
                          0  fp32 operands on the fp32 matrix instruction (v_mfma_f32_32x32x2_f32: an exact fp32 FMA chain);
                          1  bf16 operands (rounded to nearest even on load), fp32 accumulation on the bf16 matrix pipe --
                             BASELINE.json's bf16 configuration;
                          2  "fp32x3": fp32 operands, each split EXACTLY into three bf16 slices (8 + 8 + 8 significand bits),
                             a product formed from six of the nine slice products on the bf16 matrix pipe with fp32
                             accumulation; what is dropped is <= 2^-26 of |a b|, below the fp32 rounding of the accumulation.
                             fp32-grade results at 6/64 of the matrix-pipe time of engine 0 (the Python binding's "fp32").
                          Every other computation and all parameters stay fp32 under all three.  Engines 1 and 2 need the
                          fast path (D % 4 == 0, fc_dim % 4 == 0, fc_dim <= 124; engine 2's fused fc11 kernel fc_dim <= 111),
                          else engine 0 runs.  Any other value: MMVAE_E_BADARG. */
    uint32_t cat_mask[4]; /* category subset of forward(mask=...) (nn_model.py:332-335, the pruning-time forward; eval_model passes
                          the categories whose fcc bias is non-zero, cpl_mixvae.py:1476-1478): bit k of the 128-bit mask set =
                          category k is kept; c = softmax(c_prob[:, kept] / tau) on the kept categories and 0 elsewhere.
                          All four words zero = no mask (every category kept). */
} mmvae_hyper;

/* Noise descriptor.  mode 0 = explicit buffers (parity tests; the reference's RNG stream cannot
 * be replayed on a GPU), mode 1 = in-kernel Philox4x32-10 keyed by (seed, offset), the
 * throughput mode.  Consumption order of the reference per arm: bernoulli[B,D] -> rand[B,C] ->
 * rand_like[B,S] -> bernoulli[B,S] iff s_drop>0. */
typedef struct mmvae_noise {
    int32_t mode;
    int32_t _pad;
    const uint8_t *x_mask;  /* [A,B,D] keep-mask (1 = keep), used iff training && x_drop>0 */
    const float *u_gumbel;  /* [A,B,C] U(0,1), used iff !eval_flag                         */
    const float *u_state;   /* [A,B,S] U(0,1) (uniform, as nn_model.py:427 draws it)       */
    const uint8_t *s_mask;  /* [A,B,S] keep-mask, used iff training && s_drop>0            */
    uint64_t seed;
    uint64_t offset;        /* advance by 1 per step                                       */
} mmvae_noise;


/* Caller-owned execution context (one per engine / workspace; NULL = defaults: single stream, automatic split
 * factors).  The library reads it during a call and writes only `early_recorded`.
 *   side_stream  optional second hipStream_t on the same device.  With it mmvae_backward / mmvae_train_step run the
 *                [dW11 | db11] GEMM, the coupling terms and the loss scalars beside the latency-bound chains of the main
 *                stream (fork / join by the events below).  The caller keeps stream and events alive while work that
 *                uses them is in flight.
 *   ev           MMVAE_N_EVENTS hipEvent_t (hipEventDisableTiming suffices), all non-NULL when side_stream is.  The library records
 *                them itself -- with hipEventRecord, or as the stop event of one of its own kernel launches (hipExtLaunchKernel):
 *                either way an event belongs to ONE engine and is not to be recorded or waited on by the caller while a call
 *                that uses it is in flight.
 *   early_grad_event  data-parallel overlap: when non-NULL (and side_stream is set), mmvae_backward and
 *                mmvae_train_step(do_adam == 0) reduce the gradients of fc11.weight / fc11.bias -- the last two
 *                tensors of every arm's segment of `grads`, 47 % of the parameters -- as soon as their GEMM has
 *                finished and record this event on the side stream, so the caller can start the all-reduce of those
 *                ranges while the rest of backward runs (replaces the reference's FSDP gradient traffic,
 *                train.py:140-143).  All other gradients are final when the call's work on `stream` is.
 *   early_recorded  out: 1 if the call recorded early_grad_event (it does not on shapes the fast kernels do not
 *                take, without a side stream, or with do_adam != 0): only then may the caller wait on it.
 *   split        split factors of the large GEMMs, 0 = automatic: 0 fc1 split-K, 1 fc11 column splits, 2 dW1 batch
 *                splits, 3 small-layer dW batch splits, 4 d(d10) gene splits, 5 dW11 batch splits.  They change the
 *                workspace layout: pass the same context to mmvae_workspace_bytes / mmvae_ws_offset.
 *   tune         MMVAE_TUNE_ENGINE below; the other entries are the implementation's experiment
 *                switches (0 = production behaviour).  The library reads no environment variables. */
#define MMVAE_N_EVENTS 8
#define MMVAE_N_TUNE 24
/* mmvae_exec.tune: 0 everywhere = production behaviour.  One entry is part of the interface: */
#define MMVAE_TUNE_ENGINE 17    /* the GEMM engine the caller is going to run (mmvae_hyper.gemm_bf16; 0 = not stated).
                                   The split factors of the workspace layout are chosen for the workgroup shapes of that
                                   engine; any engine runs correctly on any layout */
/* Every other index is an experiment switch of the implementation (A/B timing, test hooks), listed in the
 * library's private header distributed-vae_amd/csrc/tune.h; callers leave them 0. */
typedef struct mmvae_exec {
    void *side_stream;
    void *ev[MMVAE_N_EVENTS];
    void *early_grad_event;
    int32_t early_recorded;
    int32_t split[6];
    int32_t tune[MMVAE_N_TUNE];
} mmvae_exec;

/* Where things are, in floats.  Filled by mmvae_param_layout. Tensor order t = 0..27:
 *  0 fc1.w[H,D] 1 fc1.b 2 fc2.w[H,H] 3 fc2.b 4 fc3.w 5 fc3.b 6 fc4.w 7 fc4.b 8 fc5.w[L,H] 9 fc5.b
 * 10 fcc.w[C,L] 11 fcc.b 12 fc_mu.w[S,L+C] 13 fc_sigma.w[S,L+C] 14 fc_mu.b 15 fc_sigma.b
 * 16 fc6.w[L,C+S] 17 fc6.b 18 fc7.w[H,L] 19 fc7.b 20 fc8.w 21 fc8.b 22 fc9.w 23 fc9.b
 * 24 fc10.w 25 fc10.b 26 fc11.w[D,H] 27 fc11.b */
typedef struct mmvae_param_layout_t {
    int64_t per_arm;                          /* floats per arm (padded)            */
    int64_t offset[MMVAE_N_PARAM_TENSORS];    /* within one arm's segment           */
    int64_t rows[MMVAE_N_PARAM_TENSORS];      /* out features (or length for bias)  */
    int64_t cols[MMVAE_N_PARAM_TENSORS];      /* in features (1 for bias)           */
    /* BatchNorm running buffers: one flat fp32 buffer, arm-major; per arm
     * [mean_i, var_i] for batch_l1..batch_l5, batch_s (nn_model.py:208-255) */
    int64_t bn_per_arm;
    int64_t bn_mean_offset[MMVAE_N_BN];
    int64_t bn_var_offset[MMVAE_N_BN];
    int64_t bn_dim[MMVAE_N_BN];
} mmvae_param_layout_t;

/* Scalars written by mmvae_loss / mmvae_train_step into `loss_out` (device, fp32):
 *  [0] total  [1] loss_joint  [2] mean neg-joint-entropy  [3] mean simplex distance
 *  [4] mean l2 distance  then rec[A], kl[A], ll[A]   (the 9-tuple of nn_model.py:588-598). */
#define MMVAE_LOSS_TOTAL 0
#define MMVAE_LOSS_JOINT 1
#define MMVAE_LOSS_CENT 2
#define MMVAE_LOSS_CDIST 3
#define MMVAE_LOSS_CL2 4
#define MMVAE_LOSS_REC0 5
#define MMVAE_LOSS_FLOATS(A) (5 + 3 * (A))

/* Named workspace regions, for callers that return forward outputs as views and for tests that
 * localise a failing kernel.  All per-arm arrays are [A, B, width]. */
typedef enum mmvae_ws_id {
    MMVAE_WS_X_LOW = 0, /* [A,B,L]  BN5 output                (forward out 3) */
    MMVAE_WS_C_PROB,    /* [A,B,C]  softmax(fcc)              (forward out 9) */
    MMVAE_WS_C,         /* [A,B,C]  softmax(c_prob/tau)       (forward out 4) */
    MMVAE_WS_C_SMP,     /* [A,B,C]  Gumbel-softmax sample     (forward out 6) */
    MMVAE_WS_S_MEAN,    /* [A,B,S]                            (forward out 7) */
    MMVAE_WS_S_LOGVAR,  /* [A,B,S]                            (forward out 8) */
    MMVAE_WS_S_SMP,     /* [A,B,S]                            (forward out 5) */
    MMVAE_WS_Y_SOFT,    /* [A,B,C]  soft sample (== C_SMP unless hard) */
    MMVAE_WS_R1, MMVAE_WS_R2, MMVAE_WS_R3, MMVAE_WS_R4, /* [A,B,H] relu(fc_i), pre-BN */
    MMVAE_WS_R5,        /* [A,B,L] */
    MMVAE_WS_D6,        /* [A,B,L] */
    MMVAE_WS_D7, MMVAE_WS_D8, MMVAE_WS_D9, MMVAE_WS_D10, /* [A,B,H] */
    MMVAE_WS_ZIN,       /* [A,B,C+S] decoder input */
    MMVAE_WS_DZ11,      /* [A,B,D] d loss / d fc11 pre-activation */
    MMVAE_WS_DZ1,       /* [A,B,H] d loss / d fc1 pre-activation  */
    MMVAE_WS_GZIN,      /* [A,B,C+S] */
    MMVAE_WS_GZC,       /* [A,B,C]  d loss / d fcc output */
    MMVAE_WS_G5,        /* [A,B,L]  d loss / d x_low */
    MMVAE_WS_BN_MEAN1,  /* [A,H] batch mean of R1 (then BN_MEAN1+i for layer i+1) */
    MMVAE_WS_GD10_SLAB, /* [n_slab][A,B,H] gene-split partial sums of d loss / d d10 = dZ11 W11 (n_slab: mmvae_splits[4]) */
    MMVAE_WS_G1,        /* [A,B,H]  d loss / d BatchNorm1's output (then G1 + i for i < 4; G5 above)               */
    MMVAE_WS_G2, MMVAE_WS_G3, MMVAE_WS_G4,
    MMVAE_WS_DZ2,       /* [A,B,H]  d loss / d fc2's pre-activation (then DZ2 + i; DZ5 is [A,B,L])                 */
    MMVAE_WS_DZ3, MMVAE_WS_DZ4, MMVAE_WS_DZ5,
    MMVAE_WS_COUNT_
} mmvae_ws_id;

/* ---- queries (host only, no GPU needed) ------------------------------------------------- */
int mmvae_abi_version(void);
const char *mmvae_last_error_string(void);
/* 0 if the kernels support these dims (H,C<=128, L<=64, S<=32, L+C,C+S<=255, A<=MMVAE_MAX_ARMS).  Calls with
 * h->training != 0 additionally need 2 <= B <= 32768 (batch statistics; capacity of the exact batch-sum accumulators); eval
 * mode takes any batch from one cell up. */
int mmvae_check_dims(const mmvae_dims *d);
int mmvae_param_layout(const mmvae_dims *d, mmvae_param_layout_t *out);
/* bytes of caller-provided workspace that forward/loss/backward/train_step need */
size_t mmvae_workspace_bytes(const mmvae_dims *d, const mmvae_exec *ex);
/* offset (in floats) of a named region inside the workspace, or -1 */
int64_t mmvae_ws_offset(const mmvae_dims *d, const mmvae_exec *ex, int ws_id);
/* the split factors the layout uses for these dims and context, in the order of mmvae_exec.split (0 fc1 split-K, 1 fc11 column
 * splits, 2 dW1 batch splits, 3 small-layer dW batch splits, 4 d(d10) gene splits = slabs of MMVAE_WS_GD10_SLAB,
 * 5 dW11 batch splits) */
int mmvae_splits(const mmvae_dims *d, const mmvae_exec *ex, int32_t out[6]);

/* ---- compute (device pointers, asynchronous on stream) ----------------------------------- */

/* x: [B,D] shared by all arms when x_arm_stride == 0 (cpl_mixvae.py:425 x.expand(A,-1,-1)),
 * else arm a reads x + a*x_arm_stride (floats).
 * bn_running: flat running mean/var (updated in place when training); num_batches_tracked:
 * int64 [A*6] incremented when training (may be NULL).
 * x_rec: optional [A,B,D] output (forward out 0); NULL = do not materialise.
 * need_grad != 0 additionally stores what backward needs (dZ11, fc10-grad slabs).
 * All other forward outputs stay in `ws` (see mmvae_ws_offset). */
int mmvae_forward(const mmvae_dims *d, const mmvae_hyper *h, const mmvae_noise *nz,
                  const float *params, float *bn_running, int64_t *num_batches_tracked,
                  const float *x, int64_t x_arm_stride, float *x_rec, int need_grad,
                  void *ws, size_t ws_bytes, mmvae_exec *ex, void *stream);

/* Finishes the loss scalars from what forward left in ws.  Must follow mmvae_forward on the same
 * ws/stream. */
int mmvae_loss(const mmvae_dims *d, const mmvae_hyper *h, void *ws, size_t ws_bytes,
               float *loss_out, mmvae_exec *ex, void *stream);

/* Gradient of loss_out[0] * grad_scale w.r.t. every parameter into `grads` (flat, same layout
 * as params; fully overwritten).  Needs forward(need_grad=1) + loss on the same ws. */
int mmvae_backward(const mmvae_dims *d, const mmvae_hyper *h, const mmvae_noise *nz,
                   const float *params, const float *x, int64_t x_arm_stride, float grad_scale,
                   void *ws, size_t ws_bytes, float *grads, mmvae_exec *ex, void *stream);

/* torch.optim.Adam / AdamW semantics on a flat buffer of n floats. step >= 1. */
int mmvae_adam_step(int64_t n, float *params, const float *grads, float *exp_avg,
                    float *exp_avg_sq, int64_t step, float lr, float beta1, float beta2,
                    float adam_eps, float weight_decay, int decoupled, void *stream);

/* forward + loss + backward (+ Adam when do_adam) for one batch: cpl_mixvae.py:434-463.
 * With do_adam == 0 the caller all-reduces `grads` (data parallel) and then calls
 * mmvae_adam_step itself. */
int mmvae_train_step(const mmvae_dims *d, const mmvae_hyper *h, const mmvae_noise *nz,
                     float *params, float *bn_running, int64_t *num_batches_tracked,
                     const float *x, int64_t x_arm_stride, void *ws, size_t ws_bytes,
                     float *grads, float *loss_out, int do_adam, float *exp_avg,
                     float *exp_avg_sq, int64_t step, float lr, float beta1, float beta2,
                     float adam_eps, float weight_decay, int decoupled, mmvae_exec *ex, void *stream);

/* mmvae_train_step on a batch that is never materialised: cell b of the batch is row rows[b] of the resident cells x genes
 * matrix `data` ([n_rows, ld] fp32, ld >= D; rows: int64 [B] on the device, indices outside [0, n_rows) are clamped as
 * mmvae_gather_rows does), shared by all arms (x.expand).  Replaces the batch assembly of the reference's DataLoader
 * (mmidas/utils/dataloader.py:114-132: shuffled index batches collated into a fresh tensor, pinned, copied to the device) AND
 * the per-step row gather of mmvae_gather_rows: fc1, the fused fc11 kernel and dW1 read x through a row map (B 32-bit
 * offsets the step's head launch derives from `rows`), so a shuffled batch costs what a resident one does.  Bit-identical to
 * mmvae_gather_rows + mmvae_train_step.  Offered where it is built -- the fused training step of the fp32x3 and bf16 engines
 * (gemm_bf16 == 2 with fc_dim <= 111, or == 1; x_drop > 0), ld % 4 == 0, 16-byte aligned data, n_rows * ld < 2^30 floats --; otherwise
 * MMVAE_E_UNSUPPORTED: gather the batch and call mmvae_train_step.
 *
 * data_bf16 (optional, NULL = none; the bf16 engine only, BASELINE.json configs[2]): a bf16 copy of `data` with the same
 * shape and leading dimension (in elements), made once per data set by mmvae_to_bf16.  The engine rounds x to bf16 on its way
 * to the matrix pipe anyway; with the copy fc1, dW1 and the fused fc11 kernel read 2 bytes per cell and gene instead of 4, and
 * dZ11 travels from the fused kernel to the dW11 GEMM as bf16 (the values that GEMM takes in any case).  Same results as the
 * step on an fp32 matrix that holds the rounded values -- bit for bit --; against the unrounded matrix only the
 * reconstruction loss changes: it compares with the rounded x (within the configuration's 5e-2 gate).
 * Needs D % 8 == 0, ld % 8 == 0, a 16-byte aligned copy; MMVAE_E_UNSUPPORTED otherwise or with another engine. */
int mmvae_train_step_rows(const mmvae_dims *d, const mmvae_hyper *h, const mmvae_noise *nz, float *params,
                          float *bn_running, int64_t *num_batches_tracked, const float *data,
                          const uint16_t *data_bf16, int64_t ld,
                          int64_t n_rows, const int64_t *rows, void *ws, size_t ws_bytes, float *grads,
                          float *loss_out, int do_adam, float *exp_avg, float *exp_avg_sq, int64_t step, float lr,
                          float beta1, float beta2, float adam_eps, float weight_decay, int decoupled,
                          mmvae_exec *ex, void *stream);

/* ---- evaluation labels and between-arm consensus ----------------
 * Replaces the per-epoch host loop of mmidas/cpl_mixvae.py:563-657: eval-mode forward of every batch,
 * `classify` = argmax of c (mmidas/_utils.py:79-80), `compute_confmat` per arm pair (:84-95),
 * `confmat_normalize` (:98-100), `confmat_mean` (:128-129).
 *
 * mmvae_eval_classify: encoder + latent block of forward(eval=True) with the BatchNorm running statistics
 *   (h->training == 0, h->eval_flag == 1; no decoder, no fc11: the labels need c only), then
 *   labels[a*B + b] = argmax_k c[a][b][k] (first maximum on ties, as np.argmax).  labels: int32 [A,B].
 *   counts != NULL: additionally counts[pair][labels[a][b]][labels[a'][b]] += 1 for every arm pair a < a'
 *   in the order (0,1), (0,2) ... (A-2,A-1); counts: int64 [A(A-1)/2, C, C], zeroed by the caller before
 *   the first batch of an epoch.
 * mmvae_classify: the argmax alone on any [n_cells, C] fp32 matrix.
 * mmvae_confmat_accumulate: the counting alone, labels int32 [A, n].
 * mmvae_consensus: cm_norm[pair][i][j] = counts[pair][i][j] / max(rowsum_j, colsum_j) (0 where that is 0),
 *   consensus[pair] = mean_k cm_norm[pair][k][k]; fp64, numpy's summation order, C <= 128.
 *   cm_norm (double [npairs, C, C]) may be NULL; consensus: double [npairs]. */
int mmvae_eval_classify(const mmvae_dims *d, const mmvae_hyper *h, const float *params,
                        const float *bn_running, const float *x, int64_t x_arm_stride, void *ws,
                        size_t ws_bytes, int32_t *labels, int64_t *counts, mmvae_exec *ex, void *stream);
int mmvae_classify(const float *c_probs, int64_t n_cells, int C, int32_t *labels, void *stream);
int mmvae_confmat_accumulate(const int32_t *labels, int A, int64_t n, int C, int64_t *counts,
                             void *stream);
int mmvae_consensus(const int64_t *counts, int npairs, int C, double *cm_norm, double *consensus,
                    void *stream);

/* ---- cross-run evaluation (mmidas/_evals.py::evals2) ---------------------
 * evals2 fills, for every arm pair of two trained runs, a confusion matrix pm and a matrix emp of summed
 * probability distances with a host loop over the cells.  Here the labels and probabilities of both runs stay on
 * the device: T = the arms of run a followed by the arms of run b, labels int32 [T, n] (mmvae_encode's labels),
 * probs float [T, n, C] (mmvae_encode's c).
 *
 * mmvae_pair_stats: pairs is a HOST array int32 [n_pairs][4] = (lab1, prob1, lab2, prob2), arm indices into T (the
 *   reference's within-run loops take the second probability row from another arm than the second label row, so
 *   the four are separate).  For every pair p and cell i with i1 = labels[lab1][i], i2 = labels[lab2][i] both in
 *   [0, C) (other cells are skipped):
 *     counts[p][i1][i2] += 1                                                    int64 [n_pairs, C, C]
 *     dist[p][i1][i2]   += |(double)probs[prob1][i][i1] - (double)probs[prob2][i][i2]|
 *   dist_acc: int64 [n_pairs, C, C, 2], a fixed-point sum with resolution 2^-52 (slots hi, lo; value =
 *   (hi 2^32 + lo) 2^-52): every term is truncated by at most 2^-52, the adds are integer atomics, so the result is
 *   bit-identical from run to run and cannot overflow below 2^31 cells per call sequence.  A term outside [0, 2)
 *   (not a difference of probabilities; NaN, Inf) marks its matrix cell, which then reads back as NaN.  Both arrays
 *   are zeroed by the caller and a call ADDS to them, so a data set can be fed batch by batch.
 * mmvae_pair_stats_finish, per pair in fp64: smp[j] = max(row sum j, column sum j) of counts;
 *   cm_norm = counts / smp[j] along the last axis, 0 where smp[j] == 0 (mmvae_consensus's cm_norm, bit for bit);
 *   emp = the distance sums; dist_norm = emp / smp[j] by the same rule (all double [n_pairs, C, C]);
 *   diag_mean = mean of diag(cm_norm) in numpy's summation order, diag_min its minimum (double [n_pairs]).
 * Both check every argument on the host before any device work: MMVAE_E_BADARG for a null pointer, C outside
 *   [1, 128], n < 0 or n > 2^31, n_pairs < 0, n_arms_total outside [1, 2 MMVAE_MAX_ARMS], a pair index outside
 *   [0, n_arms_total).  n == 0 or n_pairs == 0: returns 0 without a launch.
 * mmvae_debug_pair_stats: mmvae_pair_stats with the kernel path named (-1 the launcher's rule, 0 the per-workgroup
 *   LDS histogram -- C <= 116, else MMVAE_E_UNSUPPORTED --, 1 the wave-combined global atomics); same results. */
int mmvae_pair_stats(const int32_t *labels, const float *probs, int n_arms_total, int64_t n, int C,
                     const int32_t *pairs, int n_pairs, int64_t *counts, int64_t *dist_acc, void *stream);
int mmvae_pair_stats_finish(const int64_t *counts, const int64_t *dist_acc, int n_pairs, int C,
                            double *cm_norm, double *emp, double *dist_norm, double *diag_mean,
                            double *diag_min, void *stream);
int mmvae_debug_pair_stats(const int32_t *labels, const float *probs, int n_arms_total, int64_t n, int C,
                           const int32_t *pairs, int n_pairs, int64_t *counts, int64_t *dist_acc, int path,
                           void *stream);

/* ---- mutual-information evaluation (evaluation.py::mutinfo) ---------------
 * mutinfo scores a model by sklearn's adjusted_mutual_info_score between every cell-type column f of the one-hot
 * targets and every cluster c, two binary labelings of the n cells per call.  Here one launch counts the
 * contingency of all (arm, f, c) and one launch evaluates all 2 x 2 adjusted-MI values from the counts.
 *
 * mmvae_mutinfo_counts: labels int32 [A, n] (mmvae_classify's argmax); targets a row-major 0/1 matrix [n, ldt] of
 *   which columns 0..F-1 are used, elements of target_bytes = 1 (uint8) or 4 (int32) bytes, non-zero = set.
 *   For every cell i and arm a with l = labels[a][i] in [0, C) (other labels are skipped):
 *     counts[a][f][l] += 1 for each f < F with targets[i][f] != 0        int64 [A, F, C]
 *     p_sum[a][l]     += 1                                                int64 [A, C]
 *   and t_sum[f] += 1 once per cell per set column, whatever the labels   int64 [F].
 *   Integer atomics: bit-identical from run to run.  The caller zeroes the three arrays and a call ADDS to them, so
 *   a data set can be fed batch by batch.  MMVAE_E_BADARG, before any device work, for a null pointer, A outside
 *   [1, MMVAE_MAX_ARMS], C outside [1, 128], F outside [1, 4096], n < 0 or n > 2^31, ldt < F, target_bytes not 1
 *   or 4.  n == 0: returns 0 without a launch.
 * mmvae_debug_mutinfo_counts: the same with the kernel path named: -1 the launcher's rule, 0 per-workgroup LDS
 *   histograms (F C + C + F <= 16384 counts, else MMVAE_E_UNSUPPORTED), 1 global atomics; same results.
 * mmvae_ami_binary: ami[a][f][c] (double [A, F, C]) = adjusted_mutual_info_score(u, v), average_method
 *   "arithmetic", of binary labelings u with t = t_sum[f] ones and v with p = p_sum[a][c] ones of N cells that share
 *   n11[a][f][c] ones, restated from the counts in fp64: contingency [[N-t-p+n11, p-n11], [t-n11, n11]]; both
 *   labelings single-valued 1.0, exactly one 0.0, else (MI - EMI) / (mean(H(u), H(v)) - EMI) with sklearn's clamps
 *   (numerator and denominator away from zero by 2^-52 keeping their sign, MI terms below 2^-52 dropped, MI clipped
 *   at 0) and EMI the sum of sklearn's _expected_mutual_info_fast.pyx.  p == 0 (c is no cluster) gives NaN, and so
 *   do counts that are no contingency table of N cells.  One wave per table with a fixed-order reduction:
 *   bit-identical from run to run.  ws: mmvae_ami_binary_workspace_bytes(N) = 2 (N + 1) doubles of device memory
 *   (0 for an N outside [1, 2^31]) for a table of lgamma(k + 1) and log(k) that a first small launch fills, or
 *   NULL: log-gamma and log are then evaluated per term (slower; no memory).  MMVAE_E_BADARG, before any device
 *   work, for a null n11 / t_sum / p_sum / ami, A outside [0, MMVAE_MAX_ARMS], C outside [1, 128], F outside
 *   [1, 4096], N outside [1, 2^31], a misaligned ws; MMVAE_E_WORKSPACE for a ws below the size.  A == 0 (no
 *   tables): returns 0 without a launch. */
int mmvae_mutinfo_counts(const int32_t *labels, int A, int64_t n, int C, const void *targets, int target_bytes,
                         int64_t ldt, int F, int64_t *counts, int64_t *t_sum, int64_t *p_sum, void *stream);
int mmvae_debug_mutinfo_counts(const int32_t *labels, int A, int64_t n, int C, const void *targets,
                               int target_bytes, int64_t ldt, int F, int64_t *counts, int64_t *t_sum,
                               int64_t *p_sum, int path, void *stream);
size_t mmvae_ami_binary_workspace_bytes(int64_t N);
int mmvae_ami_binary(const int64_t *n11, const int64_t *t_sum, const int64_t *p_sum, int A, int F, int C,
                     int64_t N, void *ws, size_t ws_bytes, double *ami, void *stream);

/* ---- silhouette samples (mmidas/utils/cluster_analysis.py: get_SilhScore, cluster_compare) ----
 * sklearn's silhouette_samples(X, labels, metric="euclidean") of n cells with points x_i in R^d and encoded labels
 * l_i in [0, K), cluster sizes f_k:
 *   S(i, k) = sum over the cells j with l_j = k of |x_i - x_j|_2
 *   a_i = S(i, l_i) / (f_{l_i} - 1)          (the cell itself adds an exact 0)
 *   b_i = min over k != l_i of S(i, k) / f_k
 *   s_i = (b_i - a_i) / max(a_i, b_i);  s_i = 0 when f_{l_i} = 1;  s_i = 0 when max(a_i, b_i) = 0
 * (sklearn reaches both zero rules through 0 / 0 and nan_to_num).
 *
 * mmvae_silhouette: x_sorted float32 row-major [n, ld], columns 0..d-1 used, the cells ordered by label, so that cluster
 *   k is the rows offsets[k] .. offsets[k + 1] - 1; offsets int64 [K + 1] on the device; perm int64 [n] on the device,
 *   perm[r] the caller's index of sorted row r, or NULL for the identity; s double [n] on the device, s[perm[r]] the
 *   value of sorted row r.  The host cannot read device memory without a synchronisation, so offsets that are not
 *   non-decreasing from offsets[0] = 0 to offsets[K] = n, and a perm that is no permutation of 0..n-1, are the CALLER'S
 *   CONTRACT: they give wrong values (no access outside the arrays).  An empty cluster is skipped.
 *   Arithmetic: every distance in fp32 in difference form (x_i - x_j per coordinate, the squares added by fma in
 *   coordinate order, a square root good to 1 ulp; no Gram expansion, hence no cancellation): relative error at most
 *   (d / 2 + 2) 2^-24 for finite inputs without overflow or denormal differences.  The sums S, the divisions, the minimum
 *   and s are fp64.  Nothing of size n x n exists: the sorted columns are cut into segments (whole clusters, a cluster of
 *   more than 512 columns into pieces of 512), a first launch builds that table, a second one adds every (row, segment)
 *   sum in column order and a third adds each cluster's segments in order and forms s.  No atomics, every sum in an order
 *   fixed by the inputs: bit-identical from run to run, and a row's value does not depend on the rows beside it.
 *   ws: mmvae_silhouette_workspace_bytes(n, K) bytes of device memory, 8-byte aligned: with m = K + n / 512 (the most
 *   segments there can be) m n doubles of partial sums, m + 1 int64 and K + 1 int32 of tables; 0 for an n or K that
 *   mmvae_silhouette refuses as a bad argument, or a size that size_t cannot hold.
 *   MMVAE_E_BADARG, before any device work, for a null x_sorted / offsets / ws / s, n < 3 or n > 2^31, K outside
 *   [2, n - 1], d < 1, ld < d, a misaligned ws; MMVAE_E_UNSUPPORTED for d > 128 or more than 2^23 possible segments;
 *   MMVAE_E_WORKSPACE for a ws below the size.  The launcher has one path (the d dispatch picks among instances of one
 *   kernel that give the same bits), so there is no debug entry. */
size_t mmvae_silhouette_workspace_bytes(int64_t n, int K);
int mmvae_silhouette(const float *x_sorted, int64_t ld, int64_t n, int d, const int64_t *offsets, int K,
                     const int64_t *perm /* NULL = identity */, void *ws, size_t ws_bytes, double *s, void *stream);

/* ---- state-gene correlation (mmidas/utils/tree_based_analysis.py: corr_analysis) ----
 * For every group g of cells, state dimension s and gene d, over the cells i of the group with x_id > 0, c of them:
 *   r = (sum x s - sum x sum s / c) / sqrt((sum x^2 - (sum x)^2 / c) (sum s^2 - (sum s)^2 / c)), clipped to [-1, 1]
 *   r = 0 exactly when c <= 4 (the reference's rule; a gene that is zero or negative in every cell has c = 0)
 *   r = NaN when x or s takes one value over those cells (min == max: scipy.stats.pearsonr's constant-input result)
 * which is scipy.stats.pearsonr(state[mask, s], cell[mask, d])[0] under the reference's mask and its `> 4` rule.
 *
 * mmvae_state_corr: data float32 row-major [n_total, ld], columns 0..D-1 used, read where it lies; rows int64 [n] on the
 *   device, the row of data of cell r, or NULL for the rows 0..n-1 (then n <= n_total); state float32 [n, lds], columns
 *   0..S-1 used, row r the state of cell rows[r]; offsets int64 [G + 1] on the device, group g the cells
 *   offsets[g] .. offsets[g + 1] - 1 (the cells ordered by group), or NULL for one group of all n cells (G = 1).
 *   r double [G, S, D] and count int64 [G, D] (the c above) on the device.
 *   The host cannot read device memory without a synchronisation, so offsets that are not non-decreasing from
 *   offsets[0] = 0 to offsets[G] = n and row indices outside [0, n_total) are the CALLER'S CONTRACT: every index derived
 *   from them is clamped, so they give wrong values and no access outside the arrays.  An empty group gives r = 0, c = 0.
 *   INPUTS MUST BE FINITE: a NaN or an infinity in data or state gives NaNs or wrong values (the mask x > 0 drops a NaN
 *   x, not a NaN state).
 *   Arithmetic: one pass over the matrix.  Counts are exact.  The five sums are fp64 sums of exact terms (a product of
 *   two fp32 values is exact in fp64) in row order within a segment, the segments of a group in order; with
 *   kappa = max over x and s of 1 + mean^2 / variance over the mask, |r - exact r on the same float32 values| <=
 *   8 (c + 1) kappa 2^-53 as long as that is small against 1 (DESIGN.md section 9e for the derivation).  Minima and
 *   maxima are exact, so the two special values are exact.
 *   The rows are cut into segments of at most 256 that never cross a group boundary; a wave owns one segment and 256
 *   consecutive genes (16-byte loads where data is 16-byte aligned and ld a multiple of 4, else one float at a time: the
 *   same lane-to-gene map and row order, hence the same bits), S states in passes of 4, 2 or 1; a last launch adds each
 *   group's segments in order.  No atomics: bit-identical from run to run, and group g's values are bit for bit those
 *   of a call on its cells alone.
 *   ws: mmvae_state_corr_workspace_bytes(n, D, S, G) bytes of device memory, 8-byte aligned: with m = G + n / 256 (the
 *   most segments there can be) m (5 + 5 S) D doubles of partial moments, m + 1 int64 and G + 1 int32 of tables; 0 for
 *   arguments that mmvae_state_corr refuses, or a size that size_t cannot hold.
 *   MMVAE_E_BADARG, before any device work, for a null data / state / ws / r / count, n < 1 or n > 2^31, n_total < 1,
 *   rows NULL with n > n_total, D < 1, S < 1, G < 1, ld < D, lds < S, a misaligned ws; MMVAE_E_UNSUPPORTED for S > 32 or a
 *   grid (m ceil(D / 256) or G ceil(D / 256) workgroups) of 2^31 or more; MMVAE_E_WORKSPACE for a ws below the size.
 * mmvae_debug_state_corr: the same with the load form named: path -1 the launcher's rule, 0 the narrow loads (any
 *   matrix), 1 the 16-byte loads (MMVAE_E_UNSUPPORTED where the base or ld does not allow them); same bits. */
size_t mmvae_state_corr_workspace_bytes(int64_t n, int D, int S, int G);
int mmvae_state_corr(const float *data, int64_t ld, int64_t n_total, int D, const int64_t *rows /* NULL = 0..n-1 */,
                     const float *state, int64_t lds, int64_t n, int S, const int64_t *offsets /* NULL = one group */,
                     int G, void *ws, size_t ws_bytes, double *r, int64_t *count, void *stream);
int mmvae_debug_state_corr(const float *data, int64_t ld, int64_t n_total, int D, const int64_t *rows,
                           const float *state, int64_t lds, int64_t n, int S, const int64_t *offsets, int G, void *ws,
                           size_t ws_bytes, double *r, int64_t *count, int path, void *stream);

/* ---- marker genes: the Wilcoxon rank-sum (Mann-Whitney) test of every gene, each group of cells against the rest
 * ---- (scipy.stats.mannwhitneyu, scanpy's rank_genes_groups(method="wilcoxon", tie_correct=True)) ----
 * For gene d the n selected cells' values are ranked among themselves, ties sharing the average rank.  With lo the number of
 * values < v and hi the number <= v, twice the mid-rank of a cell with value v is the integer lo + hi + 1, so
 *   rank_sum2[g, d] = sum over the cells of group g of (lo + hi + 1)          (twice the group's rank sum)
 *   tie_term[d]     = sum over the runs of equal values of t^3 - t            (t the length of a run)
 *   n_pos[g, d]     = the number of the group's cells with x > eps
 * are integers and EXACT; -0.0 and +0.0 are one value, -inf and +inf rank below and above every finite value.
 *   sum[g, d]       = the sum of the group's values in fp64, the terms exact, added in a fixed order
 * From these the caller forms U = rank_sum2 / 2 - n_g (n_g + 1) / 2 and the tie-corrected z (utils/marker_analysis.py).
 *
 * mmvae_rank_sum: x float32 row-major [n_total, ldx], columns 0..D-1 used, read where it lies; rows int64 [n] on the device,
 *   the row of x of cell r, or NULL for the rows 0..n-1 (then n <= n_total); offsets int64 [G + 1] on the device, group g the
 *   cells offsets[g] .. offsets[g + 1] - 1 (the cells ORDERED BY GROUP; an empty group is allowed and gives zeros).
 *   rank_sum2, n_pos int64 [G, D], tie_term int64 [D], sum double [G, D], on the device; every element is written
 *   (for offsets that keep the contract below).
 *   Offsets that are not non-decreasing from offsets[0] = 0 to offsets[G] = n and row indices outside [0, n_total) are the
 *   CALLER'S CONTRACT, as for mmvae_state_corr: every index derived from them is clamped, so they give wrong values and no
 *   access outside the arrays.  Under broken offsets the values are not only wrong: tie_term adds up the cells that lie in
 *   some group, so it is the gene's tie term only where the groups cover the cells 0..n-1 once; and where more than
 *   n / 1024 = 32 groups claim more than 1024 cells each (non-decreasing offsets cannot), the groups past the 32nd -- which
 *   ones is not determined -- get NO rank_sum2, n_pos and sum written and their cells are missing from tie_term.  NaN IS NOT CHECKED FOR: a gene that holds a NaN gets unspecified results (the other genes are
 *   not affected).  eps must not be a NaN.
 *   One workgroup owns one gene: its values become order-preserving 32-bit keys, are sorted in LDS, and every cell finds lo
 *   and hi by binary search.  The keys, padded to a power of two, are the LDS budget: 128 KiB of the 160 KiB a workgroup may
 *   declare hold MMVAE_RANKSUM_MAX_N = 32768 of them, and the G + 1 <= 4097 offsets lie beside them.  No floating-point
 *   atomics and no communication between workgroups: bit-identical from run to run, and a gene's results do not depend on
 *   which other genes the call holds.
 *   ws: mmvae_rank_sum_workspace_bytes(n, D, G) bytes of device memory, 8-byte aligned: the gene-major staging copy of a
 *   chunk of genes, min(D, 512) n floats (rounded up to whole 8 bytes); 0 for arguments that mmvae_rank_sum refuses.
 *   MMVAE_E_BADARG, before any device work, for a null x / offsets / ws / rank_sum2 / tie_term / n_pos / sum, n < 1,
 *   n_total < 1, rows NULL with n > n_total, D < 1, G < 1, ldx < D, a NaN eps, a misaligned ws; MMVAE_E_UNSUPPORTED for
 *   n > MMVAE_RANKSUM_MAX_N or G > 4096; MMVAE_E_WORKSPACE for a ws below the size. */
#define MMVAE_RANKSUM_KEY_LDS_BYTES (128 * 1024)                 /* of the 160 KiB of LDS one workgroup may declare */
#define MMVAE_RANKSUM_MAX_N (MMVAE_RANKSUM_KEY_LDS_BYTES / 4)    /* 32768 four-byte keys */
size_t mmvae_rank_sum_workspace_bytes(int64_t n, int D, int G);
int mmvae_rank_sum(const float *x, int64_t ldx, int64_t n_total, int D, const int64_t *rows /* NULL = 0..n-1 */, int64_t n,
                   const int64_t *offsets, int G, float eps, void *ws, size_t ws_bytes, int64_t *rank_sum2,
                   int64_t *tie_term, int64_t *n_pos, double *sum, void *stream);

/* ---- rank sums past 32768 cells: sorted blocks, cross-block ranks ----
 * mmvae_rank_sum_blocked: the arguments, the four outputs and their meaning are mmvae_rank_sum's; n may reach
 *   MMVAE_RANKSUM_BLOCKED_MAX_N = 2^20 = 1048576.  The n cells of a gene, in the call's order, are cut into ceil(n / L) blocks
 *   of L cells (the last one shorter, down to one cell), and every block's keys are sorted on their own.  For a cell with key k
 *     lo = the sum over the blocks b of #{keys of block b < k},   hi = the sum over the blocks b of #{keys of block b <= k}
 *   are the lo and hi of the whole column, so twice the mid-rank is again lo + hi + 1 and the cell adds t^2 - 1, t = hi - lo,
 *   to the tie term: every integer is mmvae_rank_sum's, whatever L is.  The groups' cells are then added in mmvae_rank_sum's
 *   order (a group of at most 1024 cells by one wave, a larger one by the workgroup of min(1024, P / 2) threads, P the power
 *   of two from 128 up that holds n), so for n <= MMVAE_RANKSUM_MAX_N all four outputs, the fp64 sum included, are
 *   bit-identical to mmvae_rank_sum's.  No floating-point atomics: bit-identical from run to run, and a gene's results do not
 *   depend on the other genes of the call.
 *   block: L; 0 = the default, MMVAE_RANKSUM_MAX_N; otherwise a power of two in [128, MMVAE_RANKSUM_MAX_N].
 *   The cap is what the number formats hold: a gene with every value tied has tie_term = n^3 - n < 2^60, an int64;
 *   lo + hi + 1 <= 2 n + 1 < 2^22 fits the uint32 kept per cell; a group's rank_sum2 stays below 2^42, so that U minus its mean
 *   is exact in fp64 on the host.
 *   Offsets that are not non-decreasing from 0 to n and row indices outside [0, n_total) are the CALLER'S CONTRACT as above:
 *   every index derived from them is clamped, so they give wrong values (tie_term is here that of all n cells) and no access
 *   outside the arrays; every output element is written.  NaN IS NOT CHECKED FOR: a gene that holds a NaN gets unspecified
 *   results, and every search stays inside its block.
 *   ws: mmvae_rank_sum_blocked_workspace_bytes(n, D, G, block) bytes of device memory, 8-byte aligned:
 *     gc (12 n + 8 ceil(n / 4096)) bytes rounded up to whole 8,   gc = min(D, 512, floor(2^32 / (12 n + 8 ceil(n / 4096))))
 *   -- for gc genes at a time the staged values, the sorted keys and lo + hi + 1 of every cell (4 bytes each) and one int64
 *   partial of the tie term per 4096 cells; at most 4 GiB at any allowed shape (gc = 341 at n = 2^20); 0 for arguments that
 *   mmvae_rank_sum_blocked refuses.
 *   The refusals are mmvae_rank_sum's, in its order, with MMVAE_E_UNSUPPORTED for n > MMVAE_RANKSUM_BLOCKED_MAX_N, and
 *   MMVAE_E_BADARG for a block that is neither 0 nor a power of two in [128, 32768].
 * mmvae_debug_rank_sum_blocked (tools/time_ranksum.py): form -1 the entry's choice, 0 every block's keys copied to LDS and
 *   searched there, 1 searched where they lie; the same bits.  phases 0 the whole call, 1 .. 3 only the staging copy / and the
 *   block sort / and the ranks of every chunk: a timing split that LEAVES THE OUTPUTS UNWRITTEN. */
#define MMVAE_RANKSUM_BLOCKED_MAX_N (1 << 20)
size_t mmvae_rank_sum_blocked_workspace_bytes(int64_t n, int D, int G, int block);
int mmvae_rank_sum_blocked(const float *x, int64_t ldx, int64_t n_total, int D, const int64_t *rows /* NULL = 0..n-1 */,
                           int64_t n, const int64_t *offsets, int G, float eps, int block, void *ws, size_t ws_bytes,
                           int64_t *rank_sum2, int64_t *tie_term, int64_t *n_pos, double *sum, void *stream);
int mmvae_debug_rank_sum_blocked(const float *x, int64_t ldx, int64_t n_total, int D, const int64_t *rows, int64_t n,
                                 const int64_t *offsets, int G, float eps, int block, void *ws, size_t ws_bytes,
                                 int64_t *rank_sum2, int64_t *tie_term, int64_t *n_pos, double *sum, int form, int phases,
                                 void *stream);

/* ---- k nearest neighbours, their votes and purity ----
 * For every query point q_i the k admitted reference points with the smallest squared Euclidean distance.
 *   q float32 row-major [nq, ldq] and r float32 row-major [nr, ldr], columns 0..d-1 used, both read where they lie;
 *   qgroup int32 [nq] and rgroup int32 [nr] on the device, both or neither: reference j is ADMITTED for query i iff no
 *   groups are given or rgroup[j] != qgroup[i] (no groups: a plain query; both = 0..n-1 on one set: the k-NN graph
 *   without the point itself; both = the fold of each cell: a test cell sees training cells only).
 *   The squared distance is fp32 in difference form: t = q_ic - r_jc rounded, acc = fma(t, t, acc) for c = 0 .. d-1 from
 *   +0.  Candidates are ordered by (the 32 bits of that float, then j), ascending -- a total order -- and
 *   idx int32 [nq, k], dist2 float32 [nq, k] hold the k smallest admitted candidates of every query in that order; where
 *   fewer than k are admitted the tail is idx = -1, dist2 = +inf.  Every element is written.  The result is a pure function
 *   of the inputs: bit-identical from run to run, independent of how the work is cut (seg_cols below) and, row by row, of the
 *   other queries of the call.  No atomics.  NaN IS NOT CHECKED FOR: a query or reference that holds one gets unspecified
 *   neighbours (indices stay inside [-1, nr)).
 *   ws: mmvae_knn_workspace_bytes(nq, nr, d, k) bytes of device memory, 8-byte aligned: the reference columns are cut into
 *   segments so that the chip is filled, and every (segment, query) keeps a sorted list of k 8-byte keys there, which a
 *   second launch merges; at most 2 GiB, 8 bytes where one segment is enough, 0 for arguments that mmvae_knn refuses.
 *   MMVAE_E_BADARG, before any device work, for a null q / r / ws / idx / dist2, one group array without the other, k, d,
 *   nq or nr below 1, ldq or ldr below d, a misaligned ws; MMVAE_E_UNSUPPORTED for k > 64, d > 128, nq or nr > 2^20;
 *   MMVAE_E_WORKSPACE for a ws below the size.
 * mmvae_debug_knn (tests, tools/time_knn.py): the same call with segments of seg_cols reference columns (0: the entry's own
 *   choice); ws then holds 8 ceil(nr / seg_cols) nq k bytes where that is more than one segment, and MMVAE_E_UNSUPPORTED
 *   where those exceed 2 GiB.  phases 0 the whole call, 1 the segment launch alone, 2 the merge alone (on the lists that an
 *   earlier call left in ws): a timing split; with more than one segment phase 1 LEAVES THE OUTPUTS UNWRITTEN.  The same bits
 *   for every seg_cols.
 * mmvae_knn_votes: idx int32 [nq, k] as above (entries outside [0, nr) are no neighbours), rlabel int32 [nr] with the
 *   reference points' labels in [0, n_classes) (a neighbour with another label is no neighbour) ->
 *   pred int32 [nq]: the label most of the row's valid neighbours carry, the SMALLEST such label on ties, -1 without a valid one;
 *   purity double [nq] (optional, needs qlabel int32 [nq]): valid neighbours with rlabel == qlabel[i] / valid neighbours,
 *   one fp64 division of two small integers, NaN without a valid neighbour;
 *   top2 int32 [nq, 2] (optional): the votes of pred and the most votes of any other label.
 *   Integer work only; deterministic.  MMVAE_E_BADARG for a null idx / rlabel / pred, purity without qlabel, nq, nr, k or
 *   n_classes below 1; MMVAE_E_UNSUPPORTED for k > 64, n_classes > 4096, nq or nr > 2^20. */
#define MMVAE_KNN_MAX_K 64
#define MMVAE_KNN_MAX_N (1 << 20)
size_t mmvae_knn_workspace_bytes(int64_t nq, int64_t nr, int d, int k);
int mmvae_knn(const float *q, int64_t ldq, int64_t nq, const float *r, int64_t ldr, int64_t nr, int d, int k,
              const int32_t *qgroup /* NULL with rgroup */, const int32_t *rgroup, void *ws, size_t ws_bytes, int32_t *idx,
              float *dist2, void *stream);
int mmvae_debug_knn(const float *q, int64_t ldq, int64_t nq, const float *r, int64_t ldr, int64_t nr, int d, int k,
                    const int32_t *qgroup, const int32_t *rgroup, void *ws, size_t ws_bytes, int32_t *idx, float *dist2,
                    int64_t seg_cols, int phases, void *stream);
int mmvae_knn_votes(const int32_t *idx, int64_t nq, int k, const int32_t *rlabel, int64_t nr, int n_classes,
                    const int32_t *qlabel /* or NULL */, int32_t *pred, double *purity /* or NULL */,
                    int32_t *top2 /* or NULL */, void *stream);

/* ---- Gaussian classifiers (mmidas/utils/cluster_analysis.py: QDA_classifier, LDA_classifier) ----
 * A Gaussian classifier under k-fold cross-validation scores a held-out cell x under class k of the model m fitted to the
 * other folds as
 *   score(x, k) = c0[m, k] - |W_mk^T (x - mu_mk)|^2 / 2,   label = the arg-max over k (the lowest index on ties)
 * with mu the class mean, W a factor of the inverse (regularised, or pooled) covariance and c0 the log prior minus half the
 * log determinant.  The host builds mu, W and c0 in fp64 from per-group moments; the two entries below are the dense part.
 *
 * mmvae_group_moments: x float32 row-major [n, ld], columns 0..d-1 used, the rows ordered by group; offsets int64 [G + 1]
 *   on the device, group g the rows offsets[g] .. offsets[g + 1] - 1; pivot float32 [d] on the device.  Per group, with
 *   t = (double)x - (double)pivot (one fp64 rounding, exact where the two exponents are close):
 *     s [G, d]               sum t
 *     M [G, d (d + 1) / 2]   sum t t^T, the upper triangle packed row by row: entry (i, j), i <= j, at
 *                            i d - i (i - 1) / 2 + j - i
 *   both double on the device; the counts are the offsets' differences.  All moments are about ONE pivot, so they add
 *   over groups: for a union of groups with N rows, mean = pivot + s / N and covariance = (M - s s^T / N) / (N - ddof).
 *   The host cannot read device memory without a synchronisation, so offsets that are not non-decreasing from
 *   offsets[0] = 0 to offsets[G] = n are the CALLER'S CONTRACT: every index derived from them is clamped, so they give
 *   wrong values and no access outside the arrays.  An empty group gives zeros.  INPUTS MUST BE FINITE.
 *   Arithmetic: each sum is one fp64 fma chain over the rows of a segment in row order (a product of two doubles is exact
 *   inside the fma), the segments of a group added in order.  Error of a covariance entry (u = 2^-53): every t carries
 *   one rounding, a chain of N terms at most N u times the sum of the terms' magnitudes, and by Cauchy-Schwarz
 *   sum |t_i t_j| <= N sqrt(m_i m_j) with m_i = var_i + (mean_i - pivot_i)^2 = kappa_i var_i; M_ij is then off by at most
 *   (N + 2) u N sqrt(m_i m_j), s_i s_j / N by at most (2 N + 5) u N sqrt(m_i m_j), and
 *     |cov_ij - exact cov_ij on the same float32 values| <= 4 (N + 2) kappa u sqrt(var_i var_j) N / (N - ddof),
 *     kappa = sqrt(kappa_i kappa_j),  kappa_i = 1 + (mean_i - pivot_i)^2 / var_i
 *   as long as that is small against 1; a pivot near the data's mean keeps kappa near 1.
 *   The rows are cut into segments of at most 256 that never cross a group boundary; a workgroup owns one segment and
 *   all d (d + 3) / 2 of its sums, staging 32 rows at a time in LDS as doubles; a last launch adds each group's segments in
 *   order.  No atomics: bit-identical from run to run, and group g's values are bit for bit those of a call on its rows
 *   alone.  Four instances of the segment kernel, for d <= 16, 32, 64, 128 (1, 3, 9, 33 sums a thread): the same chains,
 *   hence the same bits.
 *   ws: mmvae_group_moments_workspace_bytes(n, d, G) bytes of device memory, 8-byte aligned: with m = G + n / 256 (the
 *   most segments there can be) m d (d + 3) / 2 doubles of partial sums, m + 1 int64 and G + 1 int32 of tables; 0 for
 *   arguments that mmvae_group_moments refuses, or a size that size_t cannot hold.
 *   MMVAE_E_BADARG, before any device work, for a null x / offsets / pivot / ws / s / M, n < 1 or n > 2^31, d < 1, G < 1,
 *   ld < d, a misaligned ws; MMVAE_E_UNSUPPORTED for d > 128 or G > 2^20; MMVAE_E_WORKSPACE for a ws below the size.
 * mmvae_debug_group_moments: the same with the instance named: dclass -1 the launcher's rule (the first of 16, 32, 64,
 *   128 that holds d), 0..3 that instance (MMVAE_E_UNSUPPORTED where d is above it); same bits.
 *
 * mmvae_gauss_scores: x float32 row-major [n, ld], columns 0..d-1 used; model int32 [n] on the device, the model (fold)
 *   that scores cell r, in [0, F); mu double [F, K, d]; W double [F, K, d, d], W[m, k, j, c] the weight of coordinate j
 *   in column c; c0 double [F, K], -inf for a class that model m does not have; perm int64 [n] on the device, perm[r] the
 *   caller's index of row r, or NULL for the identity.  label int32 [n], best and second double [n] (the largest and the
 *   second largest score, -inf where there is none), scores double [n, K] or NULL: all on the device, entry perm[r] the
 *   value of row r.  The caller sorts the rows by model: a workgroup owns 64 consecutive cells (its waves, 16 at most,
 *   share them and split the classes into runs, merged in class order) and walks every model that one of its cells
 *   names, so sorted rows cost one walk a tile (two where a tile straddles two folds) and unsorted rows are slower, not
 *   wrong.  model values are clamped to [0, F - 1] and perm values to [0, n - 1]: a bad
 *   table gives wrong values and no access outside the arrays.
 *   Arithmetic: t_j = (double)x_j - mu_j; each inner product sum_j W[j, c] t_j one fp64 fma chain in coordinate order;
 *   the squares added by fma in column order; score = c0 - q / 2.  A column of W that is zero adds an exact 0, so a model of
 *   lower rank is its factor padded with zero columns.  A class with c0 = -inf scores exactly -inf (its mu and W are not
 *   read) and is never the label unless every class is -inf (label 0, as np.argmax).  Against the same formula summed in
 *   another order: |score - score'| <= (3 d + 4) u (sum_c (sum_j |W[j, c] t_j|)^2 + |c0|).  A cell's values do not depend
 *   on the cells beside it; bit-identical from run to run.  One kernel, no debug entry.
 *   ws: mmvae_gauss_scores_workspace_bytes(n, d, F, K) = 0 bytes: ws may be NULL.
 *   MMVAE_E_BADARG, before any device work, for a null x / model / mu / W / c0 / label / best / second, n < 1 or
 *   n > 2^31, d < 1, F < 1, K < 1, ld < d, a misaligned ws; MMVAE_E_UNSUPPORTED for d > 128, K > 4096 or F > 64. */
size_t mmvae_group_moments_workspace_bytes(int64_t n, int d, int G);
int mmvae_group_moments(const float *x, int64_t ld, int64_t n, int d, const int64_t *offsets, int G,
                        const float *pivot, void *ws, size_t ws_bytes, double *s, double *M, void *stream);
int mmvae_debug_group_moments(const float *x, int64_t ld, int64_t n, int d, const int64_t *offsets, int G,
                              const float *pivot, void *ws, size_t ws_bytes, double *s, double *M, int dclass,
                              void *stream);
size_t mmvae_gauss_scores_workspace_bytes(int64_t n, int d, int F, int K);
int mmvae_gauss_scores(const float *x, int64_t ld, int64_t n, int d, const int32_t *model, int F, int K,
                       const double *mu, const double *W, const double *c0, const int64_t *perm /* NULL = identity */,
                       void *ws /* may be NULL */, size_t ws_bytes, int32_t *label, double *best, double *second,
                       double *scores /* NULL = not wanted */, void *stream);

/* ---- leaf posteriors merged up a tree (mmidas/utils/analysis_tree_helpers.py: predict_leaf_gmm) ----
 * One Gaussian per leaf type scores a cell (mmvae_gauss_scores with c0 = log weight - log-determinant terms); the cell's
 * posterior over the L leaves is normalised in the log domain, and at every merge level of the dendrogram the posteriors
 * of the leaves under each label are added and the label with the largest sum is the prediction.
 *
 * mmvae_leaf_merge: p double [n, ldp] on the device, columns 0..L-1 used.  On entry the scores s of the cell under the L
 *   leaves, each finite or -inf (a leaf without a model); on return its posteriors.  The merge tables, int32 on the
 *   device, cover T levels: level_start [T + 1], level t the labels level_start[t] .. level_start[t + 1] - 1 of start;
 *   start [K_total + 1], label k the entries start[k] .. start[k + 1] - 1 of leaf; leaf [nnz] the leaves (columns of p) of
 *   one label after the other.  A label's list may be empty (its sum is exactly 0) and the lists of a level may overlap.
 *   K_max: the most labels of one level.  The host cannot read device memory without a synchronisation, so the tables'
 *   contents are the CALLER'S CONTRACT: level_start and start non-decreasing from 0 to K_total and nnz, at least one
 *   and at most K_max labels a level, leaves in [0, L).  Every index read from them is clamped to its array (a level's
 *   labels to the first K_max), so a bad table gives wrong values and no access outside the arrays; a level without
 *   labels gives label 0 and prob 0.
 *   Out, all on the device, entry [t, r] level t's value for cell r: label int32 [T, n] the index of the predicted label
 *   within its level; prob double [T, n] its sum; second double [T, n] or NULL, the largest sum among the level's other
 *   labels (equal to prob on a tie), 0 where the level has one label; merged double [n, K0] or NULL, every sum of level 0
 *   (K0 its number of labels; columns past the table's own count are 0).
 *   Arithmetic per cell, all fp64: m = max_l s_l (exact); e_l = exp(s_l - m); Z = sum_l e_l, lane j of a wave of 64 adding
 *   e_j, e_(j+64), ... in that order from 0.0, then z_j <- z_j + z_(j xor h) for h = 32, 16, 8, 4, 2, 1 (which is the
 *   pairwise tree that adds halves: z[0:32] + z[32:64], then [0:16] + [16:32], ...); p_l = e_l / Z, a correctly rounded
 *   division.  P_k = the p of label k's list added one by one in list order from 0.0, so that GIVEN THE POSTERIORS EVERY
 *   SUM IS DEFINED TO THE BIT; label = the lowest index of the largest P_k, as np.argmax, prob as np.max (a NaN is above
 *   every number).  Error of a posterior against exact arithmetic on the same scores (u = 2^-53): s_l - m carries one
 *   rounding, at most u |s_l - m| <= 745 u in the exponent wherever e_l is not below the normal range; the device exp is
 *   within 1 ulp (2 u); the L terms of Z, each within that and none negative, add to within (L + 2) u; the division adds
 *   u: |p_l - exact| <= (745 + L + 8) u p_l + 2^-1070, the last term for an e_l below 2^-1022 (denormal, or exactly 0
 *   from a spread above 745).  Two evaluations that form s_l - m alike (this one and tests/leafgmm_restatement.py) share
 *   that rounding and differ by at most (2 L + 12) u p_l + 2^-1070.
 *   A row of -inf only has s - m = NaN: NaN posteriors, NaN sums for every label with a leaf, label = the first of them
 *   (0 where label 0 has a leaf), prob NaN -- what the reference's 0 / 0 followed by np.argmax gives.  A NaN or +inf
 *   score gives a NaN row in the same way.
 *   No atomics and no value shared between cells: bit-identical from run to run and equal to a call on the cell alone.
 *   Levels do not build on each other: level t of a call is bit for bit a call with that level's table alone.
 *   Two launches: one wave a cell (normalise), one wave a (cell, level) with lane j on the labels j, j + 64, ... (merge).
 *   ws: mmvae_leaf_merge_workspace_bytes(n, L, T) = 0 bytes: ws may be NULL.
 *   MMVAE_E_BADARG, before any device work, for a null p / level_start / start / leaf / label / prob, n < 1 or n > 2^31,
 *   L < 1, T < 1, K_max < 1, K_total < 1 or K_total > T K_max, nnz < 0, K0 outside [1, K_max] where merged is given,
 *   ldp < L, a pointer not aligned to its element; MMVAE_E_UNSUPPORTED for L > 4096 (the limit of mmvae_gauss_scores),
 *   K_max > 4096, T > 4096 or nnz >= 2^31. */
size_t mmvae_leaf_merge_workspace_bytes(int64_t n, int L, int T);
int mmvae_leaf_merge(double *p, int64_t ldp, int64_t n, int L, const int32_t *level_start, int T, const int32_t *start,
                     int64_t K_total, int K_max, const int32_t *leaf, int64_t nnz, void *ws /* may be NULL */, size_t ws_bytes,
                     int32_t *label, double *prob, double *second /* NULL = not wanted */,
                     double *merged /* NULL = not wanted */, int K0, void *stream);

/* ---- zero-inflated negative binomial inference (mmidas/nn_model.py: decoder_zinb :289-295, zinb_loss :642-676; DESIGN.md
 * section 9k) ----
 * With h = d10, the decoder's last hidden layer [N, H]: x_rec = relu(fc11(h)), x_p = sigmoid(fc11_p(h)),
 * x_r = sigmoid(fc11_r(h)).  For one element with input X (the log1p matrix) and eps: k = exp(X) - 1, r = x_rec + eps,
 * p = (1 - eps)(x_p + eps), z = (1 - eps)(x_r + eps) and
 *   term = -log(z + (1 - z)(1 - p)^r)                                                          where X <= 0 (or X is NaN),
 *   term = -lgamma(k + r) + lgamma(r) - k log p - r log(1 - p) - log(1 - z), added in that order, where X > 0.
 * Only the selected branch is evaluated; the reference multiplies the other by an exact 0, which differs only where that
 * other branch is not finite.  zinb_loss is the mean of term over the elements.
 * All matrices are float32, row-major, on the device, with a row pitch in elements; weights [D, H] and biases [D] are
 * nn.Linear's, contiguous.  Every pre-activation is the k-ordered fp32 fma chain fma(h_{H-1}, w_{H-1}, ... fma(h_0, w_0, b))
 * of v_mfma_f32_32x32x2_f32 with the bias as C: |a - exact| <= (H + 2) 2^-24 (sum_k |w_k h_k| + |b|), and with
 * integer-valued operands whose sums stay below 2^24 it is exact.  Everything behind the fp32 pre-activation is fp64.
 *
 * mmvae_zinb_heads: x_p, x_r [N, ldo] from d10 [N, ldh] and the two layers.  sigmoid(a) = 1 / (1 + exp(-a)) in fp64,
 *   rounded once to float32: within 0.5 ulp + 2^-50 relative of the sigmoid of the fp32 pre-activation; with the bound
 *   above and the sigmoid's slope <= 1/4, |x - exact| <= (H + 2) 2^-26 (sum |w h| + |b|) + 2^-24 x.  One launch.
 *
 * mmvae_zinb_nll: the three heads of every 64 x 64 tile from d10 and the six arrays W, b (fc11), Wp, bp, Wr, br, the
 *   term of every element against X [N, ldx] in the epilogue; no head is written.  p and 1 - p come from the
 *   pre-activation a without a cancelling subtraction: e = exp(-|a|), s = 1 / (1 + e) or e / (1 + e),
 *   1 - p = (1 - eps)(1 - s) + eps^2; z and 1 - z alike; pow as exp(r log(1 - p)).  Out: cell_sum double [N] (over the
 *   genes) and gene_sum double [D] (over the cells).
 * mmvae_zinb_terms: the same sums from heads the caller gives (x_rec, x_p, x_r and X, four pitches); 1 - p and 1 - z are
 *   the fp64 differences.  terms float32 [N, ld_t] or NULL: every term, rounded once.
 *   Error of a term given its fp32 inputs: the fp64 evaluation, a few 2^-53 of M, the sum of the magnitudes of its
 *   addends -- far below what the fp32 pre-activations carry.
 *   Sums, both entries: a 32 x 32 sub-tile (cells 32 i .., genes 32 j ..) leaves for each cell the sum over its genes by
 *   the pairwise tree on the gene index (c <- c + c(g xor s), s = 16, 8, 4, 2, 1; genes past D count an exact 0) and for
 *   each gene the sum over its cells (rows (g & 3) + 8 (g >> 2) for g = 0..15 one by one from 0.0, the same for rows + 4,
 *   then the two added); a last launch adds the sub-tiles' partials in tile order from 0.0.  No floating-point atomics:
 *   bit-identical from run to run; a cell's cell_sum depends on that cell's rows of d10 and X alone, not on N or on the
 *   other cells of the call.
 *   ws: mmvae_zinb_nll_workspace_bytes(N, D) = mmvae_zinb_terms_workspace_bytes(N, D) = 8 (ceil(D / 32) N + ceil(N / 32) D)
 *   bytes of device memory, 8-byte aligned; 0 for arguments the entries refuse.
 * All three: MMVAE_E_BADARG, before any device work, for a null pointer (terms excepted), N < 1 or N > 2^31, D < 1, H < 1,
 *   a pitch below its width, eps outside [0, 1), a misaligned ws; MMVAE_E_UNSUPPORTED for H > 128 or more than 2^31 - 1
 *   tiles; MMVAE_E_WORKSPACE for a ws below the size.  Any N and D otherwise: no multiple is required. */
int mmvae_zinb_heads(const float *d10, int64_t ldh, int64_t N, int H, int D, const float *Wp, const float *bp,
                     const float *Wr, const float *br, float *x_p, float *x_r, int64_t ldo, void *stream);
size_t mmvae_zinb_nll_workspace_bytes(int64_t N, int D);
int mmvae_zinb_nll(const float *d10, int64_t ldh, int64_t N, int H, int D, const float *W, const float *b,
                   const float *Wp, const float *bp, const float *Wr, const float *br, const float *X, int64_t ldx,
                   double eps, void *ws, size_t ws_bytes, double *cell_sum, double *gene_sum, void *stream);
size_t mmvae_zinb_terms_workspace_bytes(int64_t N, int D);
int mmvae_zinb_terms(const float *x_rec, int64_t ld_rec, const float *x_p, int64_t ld_p, const float *x_r, int64_t ld_r,
                     const float *X, int64_t ldx, int64_t N, int D, double eps, void *ws, size_t ws_bytes,
                     double *cell_sum, double *gene_sum, float *terms /* NULL = not wanted */, int64_t ld_t,
                     void *stream);

/* ---- gradients of the ZINB term with respect to the decoder's three heads ----
 * Notation as above; a_rec, a_p, a_r are the heads' fp32 pre-activations (the fma chain of mmvae_zinb_nll, unchanged),
 * r = max(a_rec, 0) + eps, s = sigmoid(a), p = (1 - eps)(s_p + eps), z = (1 - eps)(s_r + eps), q = 1 - p, y = 1 - z.
 *   X > 0:   d/dr = -psi(k + r) + psi(r) - log q     d/dp = -k / p + r / q        d/dz = 1 / y
 *   X <= 0:  with w = q^r, u = z + y w:
 *            d/dr = -y w log q / u                    d/dp = y r w / (q u)         d/dz = expm1(r log q) / u
 * in fp64, only the selected branch; d r / d a_rec = [a_rec > 0], d p / d a_p = (1 - eps) s (1 - s) with s and 1 - s formed
 * from exp(-|a|) without a cancelling subtraction, z alike.  psi: the recurrence up to 10, the asymptotic series through
 * x^-14 from there on.
 *
 * mmvae_zinb_head_grads: with g_j[i, d] = d term / d a_j, for every head j whose bit of head_mask is set (1 fc11, 2 fc11_p,
 *   4 fc11_r):  dW_j[d, h] = scale sum_i g_j[i, d] d10[i, h] (float32 [D, H]),  db_j[d] = scale sum_i g_j[i, d]
 *   (float32 [D]); an unselected head's outputs may be NULL and are not written.  Also cell_sum [N] and gene_sum [D], the
 *   bits of mmvae_zinb_nll's.  Neither the N x D pre-activations nor g are written to memory: a workgroup owns 64 genes
 *   and a segment of the cells; per tile of 64 cells it forms the pre-activations, replaces them by g (fp64, rounded once
 *   to float32) and multiplies g^T into the cells' d10 on v_mfma_f32_32x32x2_f32, the cells in rising order.  A segment's
 *   dW is one float32 chain over its cells (db: an fp64 sum rounded once); the segments' partials are added in segment
 *   order in fp64, times scale,
 *   rounded once.  No atomics: bit-identical from run to run; a gene's row depends on that gene's column of X and its
 *   weights alone, not on D.
 *   segments: the number of cell segments asked for, 0 = the library's rule (about two workgroups a CU); the count used,
 *   mmvae_zinb_head_grads_segments(N, D, segments), is at most ceil(N / 64): every segment has ceil(ceil(N / 64) / segments) cell tiles, the last what is left.
 *   ws: mmvae_zinb_head_grads_workspace_bytes(N, D, H, segments) = mmvae_zinb_nll_workspace_bytes(N, D)
 *   + 4 S 3 D (H + 1) bytes (rounded up to whole 8) with S the count used, 8-byte aligned; 0 for arguments the entry
 *   refuses.
 * mmvae_zinb_terms_grad: g_rec, g_p, g_r float32 [N, ld_g] = scale x the gradient of the term with respect to the given
 *   heads x_rec, x_p, x_r (four pitches as mmvae_zinb_terms): r = x_rec + eps with no relu (the reference takes rec_x as
 *   given), d p / d x_p = d z / d x_r = 1 - eps; fp64, rounded once.  The heads are not checked: psi is defined here for
 *   a positive argument only (psi(0) = -inf; a negative argument, -inf or a NaN gives NaN, in at most ten steps of the
 *   recurrence), so where X > 0 and x_rec + eps <= 0 or x_rec is not a number g_rec is -inf, +inf or NaN as that
 *   arithmetic gives it, and x_p, x_r outside [0, 1] give what the logarithms and divisions of the table give (NaN or an
 *   infinity); such an element costs no more time than any other and touches no other element.
 * Refusals as mmvae_zinb_nll's; besides MMVAE_E_BADARG for head_mask outside [1, 7], a selected head's NULL output,
 *   segments < 0, a scale that is not finite.
 * mmvae_debug_zinb_grad_host, mmvae_debug_digamma_host: the element code on the host, no device work.  g double [3, n] =
 *   (g_rec, g_p, g_r) before the rounding, term double [n] or NULL, from float32 X, a_rec, a_p, a_r [n]; psi(x). */
size_t mmvae_zinb_head_grads_workspace_bytes(int64_t N, int D, int H, int segments);
int mmvae_zinb_head_grads_segments(int64_t N, int D, int segments);
int mmvae_zinb_head_grads(const float *d10, int64_t ldh, int64_t N, int H, int D, const float *W, const float *b,
                          const float *Wp, const float *bp, const float *Wr, const float *br, const float *X, int64_t ldx,
                          double eps, double scale, int head_mask, int segments, void *ws, size_t ws_bytes, float *dW,
                          float *db, float *dWp, float *dbp, float *dWr, float *dbr, double *cell_sum, double *gene_sum,
                          void *stream);
/* mmvae_zinb_d10_grad: gd10[i, h] = scale sum_{j in head_mask} sum_d g_j[i, d] W_j[d, h], float32
 *   [N, ldg], with g_j exactly as above.  The mirror of mmvae_zinb_head_grads: a workgroup owns 64 cells and a segment of
 *   the 64-gene tiles, which it walks in rising order; per tile it forms the pre-activations (the bits of mmvae_zinb_nll),
 *   replaces them by g (fp64, rounded once, an exact 0 past N or D) and multiplies g into the tile's rows of W_j on
 *   v_mfma_f32_32x32x2_f32.  A segment's gd10[i, h] is one float32 chain: gene tiles rising, within a tile the gene pairs
 *   rising, within a pair the selected heads in the order fc11, fc11_p, fc11_r; the segments' partials are added in segment
 *   order in fp64, times scale, rounded once.  Nothing N x D is written, no atomics: bit-identical from run to run, and with
 *   D and the segment count fixed a cell's row depends on that cell's rows of d10 and X and on the weights alone.  An
 *   unselected head's weights enter the pre-activations only.
 *   segments: the number of gene segments asked for, 0 = the library's rule (a grid of at most 512 workgroups: a constant,
 *   not read from the device); the count used, mmvae_zinb_d10_grad_segments(N, D, segments), is at most ceil(D / 64): every
 *   segment has ceil(ceil(D / 64) / segments) gene tiles, the last what is left.
 *   ws: mmvae_zinb_d10_grad_workspace_bytes(N, D, H, segments) = 4 S N H bytes (rounded up to whole 8), 8-byte aligned; 0
 *   for arguments the entry refuses.  Refusals as mmvae_zinb_head_grads'.
 * mmvae_decoder_trunk_grads: one arm's decoder trunk backward from gd10.  act / ld: the six activations zin [N, Z], d6
 *   [N, L], d7 .. d10 [N, H] as an eval forward or mmvae_decode leaves them, and their row pitches; params: the ten tensors
 *   fc6.weight, fc6.bias .. fc10.weight, fc10.bias in nn.Linear's layout (the biases are not read); grads: the ten float32
 *   gradients in that order, contiguous; gzin float32 [N, ldgz], the gradient with respect to the decoder's input, or NULL.
 *   The four arrays of pointers are host arrays.  dZ10 = gd10 [d10 > 0], G_l-1 = dZ_l W_l, dZ_l-1 = G_l-1 [d_l-1 > 0],
 *   dW_l = dZ_l^T in_l, db_l = sum_i dZ_l[i]: every product fp32 x fp32 exact in fp64, every sum an fp64 chain in a fixed
 *   order (the layer's fan-out rising; the cells rising within a cell segment, the segments' partials in segment order),
 *   rounded to float32 once where stored.  No atomics: bit-identical from run to run.
 *   segments: the cell segments of the dW launch, 0 = the library's rule (one per 512 cells, at most 32), at most 1024; the
 *   count used is mmvae_decoder_trunk_grads_segments(N, segments): whole chunks of 32 cells each.
 *   ws: mmvae_decoder_trunk_grads_workspace_bytes(N, Z, L, H, segments) = 4 N (L + 4 H) (whole 8) + 8 S P bytes with P the
 *   number of parameters of fc6 .. fc10, 8-byte aligned.
 *   MMVAE_E_BADARG for a null pointer (gzin excepted), N < 1 or N > 2^31, Z, L or H < 1, segments outside [0, 1024], a pitch
 *   below its width, a misaligned ws; MMVAE_E_UNSUPPORTED for H or L > 128; MMVAE_E_WORKSPACE for a ws below the size. */
size_t mmvae_zinb_d10_grad_workspace_bytes(int64_t N, int D, int H, int segments);
int mmvae_zinb_d10_grad_segments(int64_t N, int D, int segments);
int mmvae_zinb_d10_grad(const float *d10, int64_t ldh, int64_t N, int H, int D, const float *W, const float *b,
                        const float *Wp, const float *bp, const float *Wr, const float *br, const float *X, int64_t ldx,
                        double eps, double scale, int head_mask, int segments, void *ws, size_t ws_bytes, float *gd10,
                        int64_t ldg, void *stream);
/* mmvae_zinb_step_grads: mmvae_zinb_head_grads (at `segments` cell segments) and mmvae_zinb_d10_grad
 *   (at one segment a gene tile, segments = ceil(D / 64)) from ONE evaluation of g: k_zg_heads' walk, in which a tile's image
 *   of g, once multiplied (transposed) into d10 for dW, is also multiplied (M = cell, K = gene) into the 64 genes' rows of
 *   W_j; the 64 x H partials, [gene tile][cell][H] float32 in ws, are added in rising order of the gene tiles in fp64, scaled
 *   and rounded once.  The summation chains are the two entries': every output equals theirs bit for bit.
 *   ws: mmvae_zinb_step_grads_workspace_bytes(N, D, H, segments) = mmvae_zinb_head_grads_workspace_bytes(N, D, H, segments)
 *   + mmvae_zinb_d10_grad_workspace_bytes(N, D, H, ceil(D / 64)).  Refusals as the two entries'. */
size_t mmvae_zinb_step_grads_workspace_bytes(int64_t N, int D, int H, int segments);
int mmvae_zinb_step_grads(const float *d10, int64_t ldh, int64_t N, int H, int D, const float *W, const float *b,
                          const float *Wp, const float *bp, const float *Wr, const float *br, const float *X, int64_t ldx,
                          double eps, double scale, int head_mask, int segments, void *ws, size_t ws_bytes, float *dW,
                          float *db, float *dWp, float *dbp, float *dWr, float *dbr, double *cell_sum, double *gene_sum,
                          float *gd10, int64_t ldg, void *stream);
size_t mmvae_decoder_trunk_grads_workspace_bytes(int64_t N, int Z, int L, int H, int segments);
int mmvae_decoder_trunk_grads_segments(int64_t N, int segments);
int mmvae_decoder_trunk_grads(int64_t N, int Z, int L, int H, const float *const *act, const int64_t *ld,
                              const float *const *params, const float *gd10, int64_t ldg, int segments, void *ws,
                              size_t ws_bytes, float *const *grads, float *gzin /* NULL = not wanted */, int64_t ldgz,
                              void *stream);
int mmvae_zinb_terms_grad(const float *x_rec, int64_t ld_rec, const float *x_p, int64_t ld_p, const float *x_r,
                          int64_t ld_r, const float *X, int64_t ldx, int64_t N, int D, double eps, double scale,
                          float *g_rec, float *g_p, float *g_r, int64_t ld_g, void *stream);
int mmvae_debug_zinb_grad_host(int64_t n, const float *X, const float *a_rec, const float *a_p, const float *a_r,
                               double eps, double *g, double *term /* NULL = not wanted */);
int mmvae_debug_digamma_host(int64_t n, const double *x, double *out);

/* ---- training under the ZINB likelihood ----
 * The objective is the reference's loss() with the branch it left as `assert False` (mmidas/nn_model.py:547-549) taken
 * literally:  total = max(A - 1, 1) sum_a (zinb_loss(x_rec_a, x_p_a, x_r_a, x_a) + beta KL_a) + loss_joint, zinb_loss the mean
 * of the term over the B D elements of arm a as mmvae_zinb_nll evaluates it (zinb_eps: 1e-6 in the reference).  KL, entropy
 * and coupling terms are those of mmvae_train_step.
 *
 * The p and r heads live outside the 28-tensor flat layout, in a second flat float buffer heads_pr:
 *   [A][fc11_p.weight [D, H] | fc11_p.bias [D] | fc11_r.weight [D, H] | fc11_r.bias [D]], no padding;
 * mmvae_zinb_head_layout gives per_arm = 2 (D H + D) and the four offsets 0, D H, D H + D, 2 D H + D.  head_grads and the two
 * moment buffers hp_exp_avg, hp_exp_avg_sq have that shape.
 *
 * mmvae_zinb_train_step (call kind MMVAE_CALL_ZINB_STEP; needs h->training), on the call's stream alone (a side stream of
 * ex is not used):
 *   1. mmvae_train_step's forward pass, its fc11 launch included: the workspace's D10 and ZIN hold the step's activations,
 *      the BatchNorm running statistics and nbt are updated exactly as mmvae_train_step updates them, and the fc11 launch
 *      leaves the partial sums of (relu(a_rec) - x)^2 that ll[a] is made of (its dZ11 and d(d10) are not read);
 *   2., 3. per arm mmvae_zinb_step_grads (below: head_mask 7, segments 0) on D10 and x with scale = max(A - 1, 1) / (B D): what
 *      mmvae_zinb_head_grads gives for the three heads -- fc11's dW, db go to tensors 26 / 27 of grads, the other two heads'
 *      to head_grads -- and what mmvae_zinb_d10_grad gives at one segment a gene tile, written as the first slab of
 *      MMVAE_WS_GD10_SLAB, from one evaluation of g;
 *   4. the loss vector, then mmvae_train_step's backward pass from that one slab, without the dW11 GEMM: the other 26
 *      tensors of grads.
 * The ZINB kernels run on the fp32 matrix instruction; everything else on the engine h->gemm_bf16 states (0 or 2).
 * loss_out keeps the MMVAE_LOSS_* layout: rec[a] = zinb_loss of arm a (the fp64 per-cell sums added in a fixed order, divided
 * by B D, rounded once), total uses it; ll[a] keeps the reference's MSE-based expression (:542).
 * do_adam: mmvae_adam_step on params / grads / exp_avg / exp_avg_sq (A per_arm floats of mmvae_param_layout) and on heads_pr /
 * head_grads / hp_exp_avg / hp_exp_avg_sq, the same step; the alignment gaps of params, grads and the moments must hold
 * zeros (they then keep them).  do_adam == 0 leaves the gradients in grads / head_grads.
 * No atomics beyond those of mmvae_train_step's chains (the exact fixed-point batch sums): bit-identical from run to run.
 *   zws: mmvae_zinb_step_workspace_bytes(d, ex) = mmvae_zinb_step_grads_workspace_bytes(B, D, H, 0) + 8 (A B + D + A) bytes,
 *        8-byte aligned; 0 for dims the step refuses.
 * Refusals, all before the first launch: those of mmvae_train_step; MMVAE_E_UNSUPPORTED for eval mode, gemm_bf16 == 1 and a
 * non-zero cat_mask; MMVAE_E_BADARG for a NULL buffer, zinb_eps outside [0, 1), a negative arm stride, missing Adam state;
 * MMVAE_E_WORKSPACE for ws or zws below its size.
 *
 * mmvae_zinb_objective follows mmvae_forward on the same ws, in any mode, as mmvae_loss does: mmvae_zinb_nll per arm on D10,
 * then mmvae_loss's scalars with rec[a] = zinb_loss of arm a.  A cat_mask is allowed (eval). */
typedef struct {
    int64_t per_arm;        /* floats per arm: 2 (D H + D) */
    int64_t offset[4];      /* fc11_p.weight, fc11_p.bias, fc11_r.weight, fc11_r.bias */
} mmvae_zinb_head_layout_t;
int mmvae_zinb_head_layout(const mmvae_dims *d, mmvae_zinb_head_layout_t *out);
size_t mmvae_zinb_step_workspace_bytes(const mmvae_dims *d, const mmvae_exec *ex);
int mmvae_zinb_train_step(const mmvae_dims *d, const mmvae_hyper *h, const mmvae_noise *nz, float *params, float *heads_pr,
                          float *bn_running, int64_t *nbt, const float *x, int64_t x_arm_stride, double zinb_eps, void *ws,
                          size_t ws_bytes, void *zws, size_t zws_bytes, float *grads, float *head_grads, float *loss_out,
                          int do_adam, float *exp_avg, float *exp_avg_sq, float *hp_exp_avg, float *hp_exp_avg_sq,
                          int64_t step, float lr, float beta1, float beta2, float adam_eps, float weight_decay,
                          int decoupled, mmvae_exec *ex, void *stream);
int mmvae_zinb_objective(const mmvae_dims *d, const mmvae_hyper *h, const float *params, const float *heads_pr,
                         const float *x, int64_t x_arm_stride, double zinb_eps, void *ws, size_t ws_bytes, void *zws,
                         size_t zws_bytes, float *loss_out, mmvae_exec *ex, void *stream);

/* ---- count distributions (mmidas/utils/distributions.py) ----
 * The scVI-parameterised likelihoods of count data and one draw per element of NB / ZINB.  All matrices are float32 [N, D],
 * row-major, on the device, with a row pitch in elements; theta (and theta2) may be a vector [D], given with a pitch of 0.
 * Everything behind the float32 inputs is fp64.  With lt = log(theta + mu + eps), per element:
 *   kind 0, log_nb_positive:   theta (log(theta + eps) - lt) + x (log(mu + eps) - lt) + lgamma(x + theta) - lgamma(theta)
 *                              - lgamma(x + 1), added in that order;
 *   kind 1, log_zinb_positive: sp = softplus(-pi), ptl = -pi + theta (log(theta + eps) - lt);
 *                              x < eps: softplus(ptl) - sp;   x > eps: -sp + ptl + x (log(mu + eps) - lt) + lgamma(x + theta)
 *                              - lgamma(theta) - lgamma(x + 1);   x == eps: 0;   x NaN: NaN.  Only the selected branch is
 *                              evaluated; the reference multiplies the other by an exact 0, which differs only where that
 *                              other branch is not finite;
 *   kind 2, log_mixture_nb:    l1 = nb(x, mu, theta), l2 = nb(x, mu2, theta2 or theta), b = l2 - pi:
 *                              max(l1, b) + log1p(exp(-|l1 - b|)) - softplus(-pi).
 *   softplus(a) = max(a, 0) + log1p(exp(-|a|)): the reference's softplus switches to the identity above 20, which this does
 *   not.  Error of a term given its inputs: a few 2^-53 of the sum of the magnitudes of its addends, then one rounding to
 *   float32.
 * mmvae_count_logp.  Out, either or both: terms float32 [N, ld_t]; cell_sum double [N] and gene_sum double [D] (both or
 *   neither), by the tile scheme of mmvae_zinb_terms: 64 x 64 tiles, a partial per 32 x 32 sub-tile, the partials added in
 *   tile order.  No atomics: bit-identical from run to run, and a cell's sum depends on that cell's rows alone.
 *   ws: mmvae_count_logp_workspace_bytes(N, D) = mmvae_zinb_terms_workspace_bytes(N, D), needed for the sums only.
 *   MMVAE_E_BADARG for a null input that the kind needs, neither output, one sum without the other, N < 1 or N > 2^31,
 *   D < 1, a pitch below D (0 excepted for theta and theta2), eps outside [0, 1), a kind outside 0..2, a misaligned ws;
 *   MMVAE_E_UNSUPPORTED for more than 2^31 - 1 tiles; MMVAE_E_WORKSPACE for a ws below the size.
 * mmvae_debug_count_logp_host: the same element code on the host, every pointer host memory, terms only; no GPU call. */
typedef struct mmvae_count_logp {
    int kind;                               /* 0 NB, 1 ZINB, 2 NB mixture */
    int64_t N;
    int D;
    double eps;                             /* the reference's default: 1e-8 */
    const float *x; int64_t ldx;
    const float *mu; int64_t ld_mu;         /* mixture: mu_1 */
    const float *theta; int64_t ld_theta;   /* mixture: theta_1; pitch 0: a vector [D] */
    const float *pi; int64_t ld_pi;         /* ZINB: zero-inflation logits; mixture: mixture logits; NB: unused */
    const float *mu2; int64_t ld_mu2;       /* mixture only */
    const float *theta2; int64_t ld_theta2; /* mixture only; NULL = theta_1 */
    float *terms; int64_t ld_t;             /* NULL = not wanted */
    double *cell_sum; double *gene_sum;     /* NULL, NULL = not wanted */
} mmvae_count_logp_t;
size_t mmvae_count_logp_workspace_bytes(int64_t N, int D);
int mmvae_count_logp(const mmvae_count_logp_t *a, void *ws, size_t ws_bytes, void *stream);
int mmvae_debug_count_logp_host(const mmvae_count_logp_t *a);

/* mmvae_count_sample: one draw per element.  param 0: a = mu, b = theta (pitch 0: a vector [D]), zi by zi_kind: 0 none (NB),
 *   1 a logit, 2 a probability.  param 1: the model's heads a = x_rec, b = x_p, zi = x_r, mapped in fp64 under zinb_loss's
 *   eps guards: theta = x_rec + eps, p = (1 - eps)(x_p + eps), mu = theta p / (1 - p), z = (1 - eps)(x_r + eps).
 *   Steps: w ~ Gamma(shape theta, rate theta / mu); count ~ Poisson(min(w, 1e8)); ZINB: 0 where u <= z.  mu = 0 gives 0;
 *   mu < 0, theta <= 0, a parameter that is not finite or a NaN zi give NaN (int32 out: -1) before any loop.
 *   Out: float32 (log1p = 1: log1p of the count) or int32 (out_int32 = 1; log1p refused) [N, ld_out].
 *   Randomness: Philox4x32-10, key = seed.  The call for element i = (cell0 + row) D + gene, stage s (0 gamma, 1 boost,
 *   2 poisson, 3 inflation) and attempt t has the counter (i_lo, i_hi, (s + 4 t) ^ (offset_hi << 8), offset_lo);
 *   offset < 2^56.  Words to uniforms: u52(lo, hi) = (((hi << 32 | lo) >> 12) + 0.5) 2^-52, u32(w) = (w + 0.5) 2^-32.
 *     gamma, shape a >= 1 (Marsaglia-Tsang, d = a - 1/3, c = 1 / sqrt(9 d)), attempt t: n = sqrt(-2 log u52(w0, w1))
 *       cos(2 pi u32(w2)), y = c n; rejected if y <= -1; accepted if log u32(w3) < n^2 / 2 + d (3 log1p(y) - y (3 + y (3 + y)))
 *       with the value d (1 + y)^3.  theta < 1: shape theta + 1, times exp(log(u52 of (boost, 0)) / theta).
 *     poisson, lam < 10: u = u52 of (poisson, 0); k rises from 0 while u > the running cdf (p <- p lam / k), to 64 at most.
 *     poisson, lam >= 10: PTRS (Hoermann 1993), attempt t: U = u52(w0, w1) - 0.5, V = u52(w2, w3).
 *     inflation: u52 of (inflation, 0).
 *   A draw therefore depends on (seed, offset, i, its parameters) alone: batches with cell0 advancing equal the one call.
 *   Both rejection loops stop after 64 attempts and the inversion at k = 64; an element that gets there takes the gamma's
 *   mean (its shape) or floor(lam), and *exhausted (one int on the device, set by the call) counts such elements.
 *   MMVAE_E_BADARG for a null pointer that the mode needs, N < 1 or N > 2^31, D < 1, a pitch below D (0 excepted for
 *   param 0's b), cell0 < 0 or (cell0 + N) D >= 2^63, offset >= 2^56, eps outside [0, 1), log1p with out_int32, a param /
 *   zi_kind outside their values.
 * mmvae_zinb_sample: the three heads of every 64 x 64 tile from d10 [N, ldh] as mmvae_zinb_nll forms them, rounded to
 *   float32 as mmvae_zinb_heads and the decode write them, then param 1's mapping and draw in the epilogue: bit for bit
 *   mmvae_count_sample with param = 1 on the written heads.  Of *s it reads eps, N, D, cell0, seed, offset, out_int32, log1p,
 *   out, ld_out, exhausted.  Refusals as mmvae_zinb_nll's and mmvae_count_sample's.
 * mmvae_debug_count_sample_host: mmvae_count_sample's element code on the host, every pointer host memory; no GPU call. */
typedef struct mmvae_count_sample {
    int param;                              /* 0: (mu, theta[, zi]); 1: the heads (x_rec, x_p, x_r) */
    int zi_kind;                            /* param 0: 0 none, 1 logit, 2 probability */
    int64_t N;
    int D;
    int64_t cell0;                          /* the logical index of row 0 */
    double eps;                             /* param 1 only */
    uint64_t seed, offset;
    const float *a; int64_t ld_a;
    const float *b; int64_t ld_b;
    const float *zi; int64_t ld_zi;
    int out_int32, log1p;
    void *out; int64_t ld_out;
    int *exhausted;
} mmvae_count_sample_t;
int mmvae_count_sample(const mmvae_count_sample_t *s, void *stream);
int mmvae_zinb_sample(const float *d10, int64_t ldh, int H, const float *W, const float *b, const float *Wp,
                      const float *bp, const float *Wr, const float *br, const mmvae_count_sample_t *s, void *stream);
int mmvae_debug_count_sample_host(const mmvae_count_sample_t *s);

/* ---- random forest on 256-bin features (mmidas/utils/cluster_analysis.py: RF_classifier) ----
 * A forest under k-fold cross-validation on features quantised to 256 rank bins.  All arithmetic is integer up to one fp64
 * score per candidate split, so a tree is fixed by its inputs: bit-identical from run to run, independent of the order of
 * the LDS atomics (which only add integers), and the tree that tests/forest_restatement.py grows on the host.
 *
 * mmvae_forest_cv.  Inputs, all on the device: bins uint8 row-major [n, ld], columns 0..d-1 used; codes int32 [n] in [0, K);
 *   fold int32 [n] in [0, F).  T trees a fold, mtry in [1, d], a 64-bit seed.  Tree g = f T + t is trained on the n_f rows
 *   whose fold is not f, taken in ascending row order (train_rows).  codes are clamped to [0, K - 1] and fold values, where a
 *   row picks its trees, to [0, F - 1]: a bad table gives wrong values and no access outside the arrays.
 *   Bins are the caller's; the package's quantile_bins gives, per column, bin = (r 256) // n with r the rank of a value's first
 *   occurrence in the stably sorted column: equal values share a bin (-0.0 == 0.0), and with n <= 256 every distinct value
 *   has its own.  They are computed once over all n rows, without labels, and shared by every fold and tree.
 *   Randomness: philox4x32 (Philox4x32-10) with key = (seed's low word, seed's high word) and counter (i, g, node, stream);
 *   the training step's noise counters are another entry point with another key.  Stream 0, node 0, is the bootstrap:
 *   call i yields draws 4 i .. 4 i + 3 (its words in order), draw j picks row train_rows[(uint64(u_j) n_f) >> 32], n_f draws.
 *   Stream 1 is the feature order of node `node`: a lazy Fisher-Yates over 0 .. d - 1; step s swaps position s with
 *   s + ((uint64(u_s) (d - s)) >> 32), u_s word s & 3 of call i = s >> 2; the feature visited s-th is then at position s.
 *   Nodes: node 0 is the root; a node that splits allocates its children at the next two indices, left then right; nodes
 *   leave a stack onto which a split pushes right, then left -- so a node's index, which is the RNG's node field, is fixed
 *   by the inputs.  No depth cap: stack and tables are sized by n.
 *   Leaf: a node in which one class holds all rows, or in which, after all d features, none has two occupied bins.  Its
 *   class is the class with the most rows, the lowest code on ties.
 *   Split search: features in the drawn order; stop after mtry features once at least one candidate has been seen, else go
 *   on up to d (sklearn's rule).  For a feature, L_k(b) = the node's rows of class k with bin <= b, R_k = tot_k - L_k.  A
 *   candidate is an occupied bin b_lo that has a later occupied bin b_hi in the node.  SL2 = sum_k L_k^2 and SR2 = sum_k R_k^2
 *   are exact in uint64;  score = double(SL2) / double(nL) + double(SR2) / double(nR): two IEEE divisions and one addition,
 *   each rounded once, never contracted (n <= 2^24 keeps every operand an exact double).  Across features and bins a
 *   strictly larger score wins, so the first best in (visiting order, lowest b_lo) stands, and the node splits there
 *   whatever the gain (sklearn with min_impurity_decrease = 0).  thr = (b_lo + b_hi) >> 1; rows with bin <= thr go left:
 *   sklearn's midpoint between adjacent training values.  Only counts enter a tree; the rows of a node are nevertheless
 *   partitioned stably (left rows, then right rows, each in their order) between two index lists.
 *   Prediction: a row of fold f walks the T trees of fold f; each casts one hard vote, an integer; label = the class with the
 *   most votes, the lowest code on ties.  A class absent from a fold's training rows gets no votes in that fold.
 *   Outputs, on the device: label int32 [n]; best and second int32 [n], the votes of the label and the most votes among the
 *   other classes (0 where there are none); votes int32 [n, K] or NULL.  tree_count int32 [F T] and tree_nodes int32
 *   [F T, 2 n, 4], both or neither NULL: tree g has tree_count[g] <= 2 n_f - 1 nodes, node j = (feature, thr, left child,
 *   rows) for a split (the right child is left + 1) and (-1, class, 0, rows) for a leaf, rows the node's bootstrap rows;
 *   entries past the count are not written.  A fold that holds every row leaves its trees one leaf of class 0 and 0 rows.
 *   Departures from sklearn's RandomForestClassifier: 256 rank bins instead of exact thresholds; hard votes instead of
 *   averaged leaf distributions (equal where leaves are pure); Philox instead of MT19937 streams; the forest is seeded.
 *   Kernels: one workgroup of 256 threads grows one tree.  Per node and feature a uint32 histogram [present classes][256]
 *   in LDS (up to 128 KiB of dynamic LDS), filled by LDS integer atomics; a wave takes every fourth present class, a lane
 *   four consecutive bins (one 16-byte read, conflict-free) and the prefix is a wave scan; bin b's thread adds the waves'
 *   partial SL2, SR2 and nL, scores its candidate, and the workgroup takes the arg-max under the total order (score, then
 *   lowest bin).  Classes with no row in the node cost nothing, so small nodes are cheap on the one path there is (no
 *   debug entry).  Prediction: one launch a chunk, a wave a row, a lane a tree.  The trees are grown in chunks of launches
 *   of at most 2^30 bytes of per-tree tables (56 n + 4 bytes a tree, at least one tree); votes add across chunks.
 *   ws: mmvae_forest_workspace_bytes(n, d, F, K, T) bytes of device memory, 16-byte aligned: with c = min(F T,
 *   max(1, 2^30 // (56 n + 4))) trees a chunk, c (56 n + 4) + 4 n F + 4 n K + 4 F bytes rounded up to 16 (node tables, stacks
 *   and index lists of a chunk, the folds' training rows, the votes, the counts); 0 for arguments that mmvae_forest_cv
 *   refuses.  1.01 GiB at n = 22365, F = 10, K = 92, T = 100 (two chunks, of 857 and 143 trees).
 *   MMVAE_E_BADARG, before any device work, for a null bins / codes / fold / ws / label / best / second, one of tree_count /
 *   tree_nodes without the other, n < 2, d < 1, K < 2, F < 2, T < 1, mtry outside [1, d], ld < d, a misaligned ws;
 *   MMVAE_E_UNSUPPORTED for n > 2^24, d > 128, K > 128, F > 64 or T > 4096; MMVAE_E_WORKSPACE for a ws below the size. */
size_t mmvae_forest_workspace_bytes(int64_t n, int d, int F, int K, int T);
int mmvae_forest_cv(const uint8_t *bins, int64_t ld, int64_t n, int d, const int32_t *codes, const int32_t *fold, int K,
                    int F, int T, int mtry, uint64_t seed, void *ws, size_t ws_bytes, int32_t *label, int32_t *best,
                    int32_t *second, int32_t *votes /* NULL = not wanted */, int32_t *tree_count /* NULL = not wanted */,
                    int32_t *tree_nodes /* NULL = not wanted */, void *stream);

/* ---- principal components (mmidas/utils/cluster_analysis.py: cluster_compare's PCA) ----
 * The top-k principal subspace of an fp32 matrix needs three dense products: the covariance (once), the covariance times a
 * block of at most 64 vectors (once per step of a subspace iteration, which the host drives), and the centred data times the
 * components.  Everything is fp64 on the fp32 values; u = 2^-53.
 *
 * mmvae_gram: data float32 row-major [n_total, ld], columns 0..D-1 used, read where it lies; rows int64 [n] on the device,
 *   the row of data of sample r, or NULL for the rows 0..n-1 (then n <= n_total); pivot float32 [D] on the device.  With
 *   t = (double)x - (double)pivot (one fp64 rounding):
 *     s [D]      sum t over the n rows
 *     G [D, D]   sum t t^T, the full matrix, row pitch D; G[i, j] and G[j, i] are the same bits
 *   both double on the device.  cov = 0 leaves the raw moments about the pivot; cov = 1 turns G in place into the unbiased
 *   covariance (G - s s^T / n) / (n - 1); s is the same either way, and mean = pivot + s / n.  Any pivot is valid: it moves
 *   only kappa below.  Row indices outside [0, n_total) are the CALLER'S CONTRACT: they are clamped, so they give wrong
 *   values and no access outside the matrix.  INPUTS MUST BE FINITE.
 *   Arithmetic: only the 64 x 64 tiles with tile_i <= tile_j are computed, on v_mfma_f64_16x16x4_f64: the rows are staged
 *   32 at a time in LDS as the doubles t and every entry is a chain of MFMA steps of four rows in row order, each product
 *   exact before it is added.  Against the exact sum of the same t: |G_ij - exact| <= (n + 2) u sum_r |t_ri t_rj|, and for
 *   cov = 1 the bound derived for mmvae_group_moments above holds with N = n:
 *     |cov_ij - exact cov_ij on the same float32 values| <= 4 (n + 2) kappa u sqrt(var_i var_j) n / (n - 1).
 *   Where the upper-triangle tiles alone do not fill the chip (fewer than 256 of them: D <= 1408) and n > 256, the rows are
 *   cut into at most 3 segments -- of 256 rows while n <= 768, of ceil(n / 3) rounded up to a multiple of 32 beyond
 *   (mmvae_gram_segments returns their number and writes their length; 0 for arguments mmvae_gram refuses) -- a workgroup
 *   owns one tile of one segment, and a last launch adds the segments' tiles in segment order, mirrors the upper triangle
 *   into the lower and applies cov.  No atomics: bit-identical from run to run.  Launches: grid (T, T, segments), T =
 *   ceil(D / 64), 256 threads, 40 KiB of LDS (workgroups with tile_i > tile_j leave at once); then grid (ceil(D / 256), D).
 *   ws: mmvae_gram_workspace_bytes(n, D) bytes of device memory, 8-byte aligned: (segments - 1) D^2 doubles of partial
 *   matrices (the first segment's lands in G) and segments x D doubles of partial s: never more than twice the size of G
 *   plus 3 D doubles; 0 for arguments that mmvae_gram refuses.
 *   MMVAE_E_BADARG, before any device work, for a null data / pivot / ws / s / G, n < 2 or n > 2^31, n_total < 1, rows NULL
 *   with n > n_total, D < 1, ld < D, a misaligned ws, cov outside {0, 1}; MMVAE_E_UNSUPPORTED for D > 32768;
 *   MMVAE_E_WORKSPACE for a ws below the size.
 * mmvae_debug_gram: the same with the load form named: path -1 the launcher's rule, 0 one float at a time (any matrix),
 *   1 the 16-byte loads (MMVAE_E_UNSUPPORTED unless data is 16-byte aligned and ld a multiple of 4); same bits.
 *
 * mmvae_symm_mul: Y = C Q.  C double [D, ldc], columns 0..D-1 used (symmetric in its use here; the kernel reads every
 *   entry and does not rely on it); Q double [D, b] and Y double [D, b], row-major without padding, 1 <= b <= 64; all on the
 *   device.  Memory-bound: C is read once a call.  Y[i, c] is one fma chain over j = 0..D-1 in that order:
 *   |Y_ic - exact| <= (D + 1) u sum_j |C_ij Q_jc|; bit-identical from run to run.  A workgroup of 256 threads owns 16
 *   rows of C and stages 64 coordinates of them and of Q at a time (41 KiB of LDS); grid ceil(D / 16).
 *   ws: none; mmvae_symm_mul_workspace_bytes is 0.
 *   MMVAE_E_BADARG, before any device work, for a null C / Q / Y, D < 1, b < 1, ldc < D; MMVAE_E_UNSUPPORTED for
 *   D > 32768 or b > 64.
 *
 * mmvae_pca_project: Z = ((double)x - mean) V.  data, ld, n_total, rows, n, D as for mmvae_gram (n >= 1 here); mean double
 *   [D], V double [D, k] and Z double [n, k], row-major without padding, 1 <= k <= 64; all on the device.  Row r of Z is
 *   the sample rows[r].  t_j = (double)x_j - mean_j carries one rounding and Z[r, c] is one fma chain over j = 0..D-1 in
 *   that order: |Z_rc - exact on the same t| <= (D + 2) u sum_j |t_j V_jc|.  A row's values do not depend on the rows
 *   beside it; bit-identical from run to run.  The same kernel as mmvae_symm_mul: 16 rows a workgroup, grid ceil(n / 16).
 *   ws: none; mmvae_pca_project_workspace_bytes is 0.
 *   MMVAE_E_BADARG, before any device work, for a null data / mean / V / Z, n < 1 or n > 2^31, n_total < 1, rows NULL with
 *   n > n_total, D < 1, k < 1, ld < D; MMVAE_E_UNSUPPORTED for k > 64. */
size_t mmvae_gram_workspace_bytes(int64_t n, int D);
int mmvae_gram_segments(int64_t n, int D, int64_t *seg_rows /* may be NULL */);
int mmvae_gram(const float *data, int64_t ld, int64_t n_total, const int64_t *rows /* NULL = 0..n-1 */, int64_t n, int D,
               const float *pivot, void *ws, size_t ws_bytes, double *s, double *G, int cov, void *stream);
int mmvae_debug_gram(const float *data, int64_t ld, int64_t n_total, const int64_t *rows, int64_t n, int D,
                     const float *pivot, void *ws, size_t ws_bytes, double *s, double *G, int cov, int path, void *stream);
size_t mmvae_symm_mul_workspace_bytes(int D, int b);
int mmvae_symm_mul(const double *C, int64_t ldc, int D, const double *Q, int b, double *Y, void *stream);
size_t mmvae_pca_project_workspace_bytes(int64_t n, int D, int k);
int mmvae_pca_project(const float *data, int64_t ld, int64_t n_total, const int64_t *rows /* NULL = 0..n-1 */, int64_t n,
                      int D, const double *mean, const double *V, int k, double *Z, void *stream);

/* ---- data preparation (mmidas/utils/tools.py: normalize_cellxgene, logcpm, reorder_genes) ----
 * The reference normalises a cell x gene count matrix with sklearn's normalize(x, axis=1, norm="l1") and takes
 * np.log1p(. * scaler).  For the selected row r' (row rows[r'] of the matrix) and the selected gene j (column genes[j]):
 *   norm = sum |x| over ALL G genes of the row, 1 where that is 0
 *   out[r', j] = x / norm * scaler             (mode 0; scaler 1 gives the normalised matrix)
 *   out[r', j] = log1p(x / norm * scaler)      (mode 1)
 * the division, the product and log1p one IEEE double operation each, nothing contracted; x = 0 gives exactly 0; a float
 * output is that double rounded once.  norms[r'] is the sum itself (0 for a zero row).  Value types (vtype): 0 int32,
 * 1 float, 2 double; output types (otype): 0 float, 1 double.  An int32 row is summed in int64, exactly; a float or double
 * row in fp64 in an order that depends on G alone: the row as 16-byte pieces, piece p to thread p mod 256 of the row's
 * workgroup, a piece's values added in column order, a thread's pieces in order, the 256 sums by a fixed tree.  No atomics:
 * bit-identical from run to run.  A NaN or an infinity in a row shows in its norm, which the caller can test; the rows'
 * other values are then meaningless.
 *
 * mmvae_cpm_dense: x row-major [n_total, ld] of the value type, columns 0..G-1 used, read where it lies; rows int64 [n] on
 *   the device or NULL for the rows 0..n-1 (then n <= n_total); genes int32 [ng] on the device or NULL for all G columns
 *   in order (then ng = G).  out [n, ng] of the output type, row pitch ng, and norms double [n], on the device.  Only the
 *   selected rows are read and only the selected columns are written.  Row indices outside [0, n_total) and gene indices
 *   outside [0, G) are the CALLER'S CONTRACT: they are clamped, so they give wrong values and no access outside the
 *   arrays.  All element offsets are 64-bit.  16-byte loads where x is 16-byte aligned and the row pitch a whole number of
 *   16 bytes, else one value at a time: the same map and order, hence the same bits.
 *   MMVAE_E_BADARG, before any device work, for a null x / out / norms, a vtype, otype or mode outside its range, n < 1 or
 *   n >= 2^31, n_total < 1, rows NULL with n > n_total, G < 1, ng < 1, ld < G, genes NULL with ng != G, a scaler that is
 *   not finite, a misaligned x; MMVAE_E_UNSUPPORTED for G or ng above 2^20.
 * mmvae_debug_cpm_dense: the same with the load form named: path -1 the launcher's rule, 0 the narrow loads (any matrix),
 *   1 the 16-byte loads (MMVAE_E_UNSUPPORTED where the base or ld does not allow them); same bits.
 * mmvae_cpm_csr: the same matrix as CSR: indptr int64 [n_total + 1], indices int32 [nnz] and data [nnz] of the value
 *   type, on the device; the indices of every row strictly increasing (canonical CSR: the CALLER'S CONTRACT).  inv int32
 *   [G] on the device: the output column of gene g, or -1 for a gene that is not selected (ng <= G).  The library writes
 *   the zeros of out itself.  The row's norm is summed in mmvae_cpm_dense's order (windows of 4096 columns of the dense
 *   row are rebuilt in LDS), so out and norms are bit for bit those of mmvae_cpm_dense on the dense matrix.  Every position
 *   read from indptr is clamped to [0, nnz]; an entry whose column is outside [0, G) is never used or written; an inv
 *   value outside [0, ng) is not written: a table that breaks the contract gives wrong values and no access outside the
 *   arrays.  An empty row gives a zero row.  MMVAE_E_BADARG as above, and for a null indptr / inv, nnz < 0, null indices
 *   or data with nnz > 0, ng > G.
 *
 * mmvae_gene_stats: data float (vtype 1) or double (vtype 2) row-major [n_total, ld], columns 0..D-1 used, read where it
 *   lies; rows as above.  Per gene d over the n selected rows: n_above int64 [D], the number of rows with x > eps, eps
 *   rounded to the value type first (numpy's comparison of a float32 array with a Python float), exact; mean and sd double
 *   [D], the mean and the population standard deviation from fp64 moments about the pivot p_d = x[rows[0], d]:
 *   mean = p + s1 / n, sd = sqrt(max(0, (s2 - s1 s1 / n) / n)) with s1 = sum (x - p), s2 = sum (x - p)^2.  The rows are
 *   cut into segments of 256; a wave owns one segment and 256 consecutive genes (16-byte loads where data is 16-byte
 *   aligned and the row pitch a whole number of 16 bytes, else one value at a time: same bits) and adds its rows in
 *   order; a last launch adds the segments in order.  No atomics: bit-identical from run to run, and a call with a row map
 *   gives the bits of a call on those rows alone.  With kappa = 1 + (mean - p)^2 / var, mean and sd are within
 *   (n + 2) kappa 2^-53 sd of the exact values on the same inputs, and the rounding of the value's own representation
 *   (DESIGN.md section 9h).  INPUTS MUST BE FINITE.
 *   ws: mmvae_gene_stats_workspace_bytes(n, D) = 8 * 3 * ceil(n / 256) * D bytes of device memory, 8-byte aligned; 0 for
 *   arguments that mmvae_gene_stats refuses, or a size that size_t cannot hold.
 *   MMVAE_E_BADARG, before any device work, for a null data / ws / n_above / mean / sd, a vtype outside [1, 2], n < 1 or
 *   n > 2^31, n_total < 1, rows NULL with n > n_total, D < 1, ld < D, a NaN eps, a misaligned ws or data;
 *   MMVAE_E_UNSUPPORTED for a grid (ceil(n / 256) ceil(D / 256) workgroups) of 2^31 or more; MMVAE_E_WORKSPACE for a ws
 *   below the size.
 * mmvae_debug_gene_stats: the same with the load form named, as mmvae_debug_cpm_dense. */
int mmvae_cpm_dense(const void *x, int vtype, int64_t ld, int64_t n_total, int G, const int64_t *rows /* NULL = 0..n-1 */,
                    int64_t n, const int32_t *genes /* NULL = 0..G-1 */, int ng, double scaler, int mode, void *out,
                    int otype, double *norms, void *stream);
int mmvae_debug_cpm_dense(const void *x, int vtype, int64_t ld, int64_t n_total, int G, const int64_t *rows, int64_t n,
                          const int32_t *genes, int ng, double scaler, int mode, void *out, int otype, double *norms,
                          int path, void *stream);
int mmvae_cpm_csr(const int64_t *indptr, const int32_t *indices, const void *data, int vtype, int64_t nnz, int64_t n_total,
                  int G, const int64_t *rows /* NULL = 0..n-1 */, int64_t n, const int32_t *inv, int ng, double scaler,
                  int mode, void *out, int otype, double *norms, void *stream);
size_t mmvae_gene_stats_workspace_bytes(int64_t n, int D);
int mmvae_gene_stats(const void *data, int vtype, int64_t ld, int64_t n_total, int D, const int64_t *rows /* NULL = 0..n-1 */,
                     int64_t n, double eps, void *ws, size_t ws_bytes, int64_t *n_above, double *mean, double *sd,
                     void *stream);
int mmvae_debug_gene_stats(const void *data, int vtype, int64_t ld, int64_t n_total, int D, const int64_t *rows, int64_t n,
                           double eps, void *ws, size_t ws_bytes, int64_t *n_above, double *mean, double *sd, int path,
                           void *stream);

/* ---- augmenter forward in the training loop ----------------------
 * Replaces `self.netA(x.expand(A,-1,-1), True, 0.1)[1]` (mmidas/cpl_mixvae.py:422-423; netA.eval(), :184), i.e.
 * Augmenter_smartseq.forward in eval mode (mmidas/augmentation/udagan.py:281-329, reparam_trick
 * mmidas/augmentation/aug_utils.py:51-65): Linear + BatchNorm1d(running statistics) + ReLU stacks around a
 * noise-conditioned Gaussian bottleneck.  D input_dim, N1 = D / 5, N3 = n_dim, N5 = n_dim / 5, Z latent_dim,
 * NZ noise_dim (udagan.py:218-279); A arms x B cells per call. */
typedef struct mmvae_aug_dims {
    int32_t A, B, D, N1, N3, N5, Z, NZ;
} mmvae_aug_dims;

/* Device pointers to the module's tensors, PyTorch layouts ([out, in] weights, contiguous). */
typedef struct mmvae_aug_tensors {
    const float *w[11], *b[11];            /* fc1 .. fc11 (fc5.weight is [N5, N3 + NZ])                   */
    const float *bn_mean[10], *bn_var[10]; /* batch_fc1 .. batch_fc10 running_mean / running_var          */
    const float *w_mu, *b_mu, *w_sigma, *b_sigma, *bn_mu_mean, *bn_mu_var; /* fc_mu, fc_sigma, batch_fc_mu */
    const float *noise_w;                  /* noise.weight [NZ, NZ] (no bias)                             */
    const float *bnz_weight, *bnz_bias, *bnz_mean, *bnz_var; /* bnz: affine BatchNorm1d, eps 1e-5        */
} mmvae_aug_tensors;

/* floats of the packed-weights buffer / bytes of workspace (shared_x: the arms share x) */
size_t mmvae_aug_packed_floats(const mmvae_aug_dims *d);
size_t mmvae_aug_workspace_bytes(const mmvae_aug_dims *d, int shared_x);
/* Once per set of weights: rows padded to 16 bytes, BatchNorm folded into per-column (scale, shift). */
int mmvae_aug_pack(const mmvae_aug_dims *d, const mmvae_aug_tensors *t, float *packed, void *stream);
/* x: [B,D] shared by the arms (x_arm_stride == 0, as x.expand) or [A,B,D] contiguous (x_arm_stride == B*D).
 * z0: [A,B,NZ] and eps: [A,B,Z] standard-normal draws (the reference's torch.randn / randn_like); scale: the
 * noise scale (0.1 in the trainer).  Outputs: s_out [A,B,Z] (forward out 0), x_aug [A,B,D] (forward out 1),
 * ready as the per-arm input of mmvae_train_step (x_arm_stride = B*D).  gemm_bf16 (0 / 1 / 2 as mmvae_hyper.gemm_bf16): != 0: the ten large Linear layers
 * take bf16 operands with fp32 accumulation (BASELINE.json's bf16 configuration); the latent block, the folded
 * BatchNorm / ReLU epilogues and all stored activations stay fp32. */
int mmvae_augment(const mmvae_aug_dims *d, const float *packed, const float *x, int64_t x_arm_stride,
                  const float *z0, const float *eps, float scale, void *ws, size_t ws_bytes, float *s_out,
                  float *x_aug, int gemm_bf16, const mmvae_exec *ex, void *stream);

/* The same forward on a batch that is ROWS OF A RESIDENT MATRIX, never assembled (the augmented counterpart of
 * mmvae_train_step_rows; the reference gathers the batch in its DataLoader, mmidas/utils/dataloader.py:114-132, and hands it to
 * netA, cpl_mixvae.py:418-423): the matrix is kept as the GEMM engine's tiled bf16 slice planes -- made ONCE per data set by
 * mmvae_tp_planes (n_planes 3: the three exact slices of the fp32x3 engine, gemm_bf16 = 2; 1: the matrix rounded to bf16,
 * gemm_bf16 = 1; mmvae_tp_planes_bytes of ZERO-FILLED device memory, 0 for unsupported arguments: K % 4 == 0, a plane --
 * n_rows rounded up to 256 x K rounded up to 16 x 2 bytes -- below 4 GB) -- and the first
 * layer's loads take the batch's rows out of it through `rows` (int64 [B] on the device, clamped to the matrix).  The arms
 * share x (as x.expand).  Same results, bit for bit, as mmvae_augment on the gathered batch.  MMVAE_E_UNSUPPORTED for
 * gemm_bf16 = 0 (the fp32 matrix-instruction engine has no planes). */
size_t mmvae_tp_planes_bytes(int64_t n_rows, int32_t K, int32_t n_planes);
int mmvae_tp_planes(const float *src, int64_t ld, int64_t n_rows, int32_t K, int32_t n_planes, uint16_t *dst,
                    void *stream);
int mmvae_augment_rows(const mmvae_aug_dims *d, const float *packed, const uint16_t *x_planes, int64_t n_rows,
                       int32_t n_planes, const int64_t *rows, const float *z0, const float *eps, float scale,
                       void *ws, size_t ws_bytes, float *s_out, float *x_aug, int gemm_bf16,
                       const mmvae_exec *ex, void *stream);

/* ---- augmenter training (mmidas/augmentation/train.py:10-157 in MSE mode) ----------------------
 * The training-mode forward of Augmenter_smartseq (udagan.py:311-329: dropout, batch-statistic BatchNorm with running-statistic
 * updates) and one step of the reference's train_augmenter, of which only weight * mse_loss(x_aug, x) has a gradient with
 * respect to the augmenter.  One arm (d->A == 1: the non-batched forward), d->B >= 2.
 * Linear layers l = 0..13: fc1..fc11, fc_mu, fc_sigma, noise (no bias: b_off = -1).  BatchNorms i = 0..11: batch_fc1..batch_fc10,
 * batch_fc_mu, bnz.  params / grads / the Adam moments: flat fp32 buffers of `total` floats in the order of
 * Augmenter_smartseq.parameters(), PyTorch layouts, alignment gaps that hold zeros; running: flat fp32 buffer of run_total floats
 * (rm_off / rv_off); nbt: int64 [12] num_batches_tracked.  act_off[i]: where the workspace keeps y^_i = the normalised
 * pre-activation of fc(i+1) ([B, rows] contiguous; h_i = relu(y^_i)) after a forward or a step. */
typedef struct mmvae_aug_train_layout {
    int64_t w_off[14], b_off[14], rows[14], cols[14];
    int64_t bnz_w_off, bnz_b_off, total;
    int64_t rm_off[12], rv_off[12], bn_n[12], run_total;
    int64_t act_off[10];
} mmvae_aug_train_layout;
int mmvae_aug_param_layout(const mmvae_aug_dims *d, mmvae_aug_train_layout *out);
size_t mmvae_aug_train_workspace_bytes(const mmvae_aug_dims *d);
/* x [B,D]; mask: uint8 [B,D] dropout keep-mask (kept entries are scaled by 1 / (1 - p_drop)); z0 [B,NZ], eps [B,Z] standard
 * normal draws.  Writes s_out [B,Z], x_aug [B,D]; updates running (unbiased variance; momentum 0.01, bnz 0.1) and nbt. */
int mmvae_aug_train_forward(const mmvae_aug_dims *d, float *params, float *running, int64_t *nbt, const float *x,
                            const uint8_t *mask, float p_drop, const float *z0, const float *eps, float scale, void *ws,
                            size_t ws_bytes, float *s_out, float *x_aug, const mmvae_exec *ex, void *stream);
/* [statistics pass: a forward with stat_mask / stat_z0 / stat_eps when stat_mask != NULL], forward, the gradient of
 * weight * mean((x_aug - x)^2) with respect to all 29 tensors into grads, Adam (mmvae_adam_step on the flat buffers) when
 * do_adam.  loss_out: 3 doubles on the device: mse, the count of elements with (x_aug > 1e-3) != (x > 1e-4), and
 * (mse + 100 count / (B D)) / 2.  No atomics: bit-identical from run to run. */
int mmvae_aug_train_step(const mmvae_aug_dims *d, float *params, float *running, int64_t *nbt, const float *x,
                         const uint8_t *mask, float p_drop, const float *z0, const float *eps, const uint8_t *stat_mask,
                         const float *stat_z0, const float *stat_eps, float scale, float weight, void *ws, size_t ws_bytes,
                         float *grads, float *s_out, float *x_aug, double *loss_out, int do_adam, float *exp_avg,
                         float *exp_avg_sq, int64_t step, float lr, float beta1, float beta2, float adam_eps,
                         float weight_decay, const mmvae_exec *ex, void *stream);

/* ---- device-resident data path ------------------------------------
 * out[i, :] = data[idx[i], :], i < n: the batch assembly of the reference's DataLoader
 * (mmidas/utils/dataloader.py:114-132: shuffled index batches collated from a host TensorDataset, pinned, copied to
 * the device) as one row gather in HBM.  data: [n_rows, ld] fp32 with ld >= D; idx: int64 [n] on the device
 * (out-of-range indices are clamped; the host loader validates them); out: [n, D] contiguous. */
int mmvae_gather_rows(const float *data, int64_t ld, int64_t n_rows, const int64_t *idx, int64_t n, int32_t D,
                      float *out, void *stream);
/* dst[r, c] = bf16(src[r, c]) (round to nearest even), r < n_rows, whole rows of ld elements: the bf16 copy of a resident
 * matrix for mmvae_train_step_rows(data_bf16).  src: [n_rows, ld] fp32, ld % 4 == 0, 16-byte aligned; dst: [n_rows, ld]
 * 2-byte elements. */
int mmvae_to_bf16(const float *src, int64_t ld, int64_t n_rows, int32_t D, uint16_t *dst, void *stream);
/* ---- data-parallel gradient exchange (SURVEY.md sections 8b / 8e) ------------------------------------------------------
 * ONE RCCL all-reduce (average) of the flat fp32 gradient buffer per step, issued by the library on the stream the step
 * runs on (stream-ordered behind mmvae_train_step(do_adam = 0), in front of mmvae_adam_step; no host synchronisation, no
 * second stream).  Replaces the reference's FSDP gradient traffic (train.py:140-143; the bring-up of
 * mmidas/_dist_utils.py:12-55 for this collective).  RCCL is resolved at run time (librccl.so.1): without it these entry
 * points return MMVAE_E_UNSUPPORTED and everything else works.  One process per GPU:
 *   rank 0:      mmvae_dp_unique_id(id)         and hands the 128 bytes to every rank (any channel: a file, a store, MPI)
 *   every rank:  mmvae_dp_init(id, rank, world_size, &comm)      on its device (collective: returns when all have called)
 *   per step:    mmvae_allreduce_grads(comm, grads, n, stream)   in place; every rank with the same n
 *   at the end:  mmvae_dp_destroy(comm)
 * The communicator is caller-owned; the library keeps nothing but the resolved RCCL entry points. */
#define MMVAE_DP_ID_BYTES 128
int mmvae_dp_unique_id(uint8_t id[MMVAE_DP_ID_BYTES]);
int mmvae_dp_init(const uint8_t id[MMVAE_DP_ID_BYTES], int rank, int world_size, void **comm);
int mmvae_allreduce_grads(void *comm, float *grads, int64_t n, void *stream);
int mmvae_dp_destroy(void *comm);

/* ---- decoding a chosen latent code, continuous-state traversal ---------------------------------------------------
 * mmvae_decode: the decoder of every arm on N = d->B rows of the caller's code: x_rec = relu(fc11(relu(fc10(...relu(fc6([c | s]))...))))
 *   (mixVAE_model.decoder, nn_model.py:277-287).  c: [A,N,C], arm a at c + a * c_arm_stride (floats), rows contiguous;
 *   s: [A,N,S] likewise; x_rec: [A,N,D].  One arm of the model: A = 1 and params + a * per_arm.  State dropout is the
 *   identity: h->training == 0, or == 1 with s_drop == 0 (both compute the same: the decoder has no BatchNorm); anything else
 *   MMVAE_E_UNSUPPORTED.  Any N from 1 up (no training-batch cap).  fc11 reads no x and computes no loss: on engine 2 (within
 *   fc_dim + 1 <= 112) and engine 1 it runs from the decoder's bf16 slice planes (engine 1: W11, b11 and d10 rounded to bf16),
 *   otherwise on the fp32 matrix instruction with the forward pass's arithmetic (engine 0: x_rec of a forward, bit for bit).
 *   Workspace: mmvae_decode_workspace_bytes(d, ex) == mmvae_workspace_bytes(d, ex) with d->B = N; the regions of mmvae_ws_offset
 *   for these dims hold the decoder's activations (MMVAE_WS_ZIN, MMVAE_WS_D6 .. D10) afterwards.
 * mmvae_state_changes: the continuous traversal of mixVAE_model.state_changes (nn_model.py:370-411) for d->B cells, eval mode
 *   only (h->training == 0, else MMVAE_E_UNSUPPORTED).  x: [B,D] shared by the arms; bn_running: the running statistics.
 *   Per arm: the eval-mode encoder and latent block (c = the hard straight-through sample of softmax(c_prob / tau), no category
 *   mask; temp has no effect), mu and v = sigmoid(fc_sigma(y)); for sample i < n_samp and cell b the decoder input is
 *   [c_b | s] with s = mu_b except s[d_s] = u[a][i][b] * sqrt(exp(log(v[d_s]))) + mu_b[d_s].  u ~ U(0,1): nz->mode 0 reads
 *   nz->u_state as [A, n_samp, B]; mode 1 draws it from Philox (seed, offset).  x_rec: [A, n_samp, B, D] in sample order
 *   (the reference's reordering of the samples is the caller's).  Workspace: mmvae_state_changes_workspace_bytes =
 *   mmvae_workspace_bytes(d) + mmvae_workspace_bytes(d with B = n_samp * B), the encoder's part first.
 * Both check every argument before any device work: MMVAE_E_BADARG for null pointers, n_samp < 1, d_s outside [0, S), a
 * gemm_bf16 outside {0, 1, 2} and dims mmvae_check_dims rejects as such; MMVAE_E_UNSUPPORTED for shapes outside its limits. */
size_t mmvae_decode_workspace_bytes(const mmvae_dims *d, const mmvae_exec *ex);
int mmvae_decode(const mmvae_dims *d, const mmvae_hyper *h, const float *params, const float *c, int64_t c_arm_stride,
                 const float *s, int64_t s_arm_stride, float *x_rec, void *ws, size_t ws_bytes, mmvae_exec *ex, void *stream);
size_t mmvae_state_changes_workspace_bytes(const mmvae_dims *d, int n_samp, const mmvae_exec *ex);
int mmvae_state_changes(const mmvae_dims *d, const mmvae_hyper *h, const mmvae_noise *nz, const float *params,
                        const float *bn_running, const float *x, int d_s, int n_samp, float *x_rec, void *ws, size_t ws_bytes,
                        mmvae_exec *ex, void *stream);

/* ---- the encoder and the latent block alone: latents of a data set without the decoder -------------------------------
 * mmvae_encode: what a forward pass computes up to the latent block -- fc1 .. fc5 with their BatchNorms, fcc and the first
 *   softmax, and in eval mode the second softmax, the noise-free hard sample and the state head -- for d->B cells of every arm,
 *   with the kernels of mmvae_forward (its outputs, bit for bit); no decoder chain, no fc11, no x_rec.  x, x_arm_stride, params,
 *   bn_running, num_batches_tracked: as mmvae_forward takes them.  `out` names the arrays wanted; each pointer may be NULL, not
 *   all of them.  Cell b of arm a is written to row a * out_rows + out_row0 + b of every array, so the chunks of a data set
 *   land in [A, out_rows, .] arrays directly (out_rows >= out_row0 + B; rows outside [out_row0, out_row0 + B) are not touched).
 *   Eval mode (h->training == 0, h->eval_flag == 1; nz may be NULL): running statistics, no dropout, any B >= 1 (no training
 *   batch cap), num_batches_tracked may be NULL, nothing is written to bn_running.  With only x_low / c_prob asked for the
 *   latent kernel returns behind the first softmax.
 *   Training mode (h->training == 1): the encoder half of a training mmvae_forward -- dropout from nz (only x_mask is read),
 *   batch statistics, the momentum update of bn_running and the increment of num_batches_tracked for BatchNorm 1 .. 5 -- and
 *   x_low / c_prob only: any other output MMVAE_E_UNSUPPORTED (mmvae_forward is the call for those); 2 <= B <= the batch cap.
 *   One arm of the model: A = 1 with params + a * per_arm, bn_running + a * bn_per_arm, num_batches_tracked + a * MMVAE_N_BN.
 *   Workspace: mmvae_encode_workspace_bytes(d, ex) == mmvae_workspace_bytes(d, ex), 256-byte aligned; afterwards the regions of
 *   mmvae_ws_offset hold the encoder's activations (MMVAE_WS_R1 .. R5, X_LOW) and, unless only x_low / c_prob were asked
 *   for, the latent block's (C_PROB, C, C_SMP, S_MEAN, S_LOGVAR); with counts, MMVAE_WS_GZC holds the [A, B] labels.
 * mmvae_intermed: mu = fc_mu(y), var = sigmoid(fc_sigma(y)) (the log with eps is forward's, nn_model.py:350) for N = d->B
 *   rows per arm.  y: [A,N,L+C], arm a at y + a * y_arm_stride (floats), rows contiguous; mu, var: [A,N,S].  Any N >= 1; reads
 *   no BatchNorm (training and eval compute the same), needs no workspace.  One arm: A = 1 and params + a * per_arm.
 * Both check every argument before any device work: MMVAE_E_BADARG for null required pointers, every output NULL,
 * out_row0 < 0 or out_rows < out_row0 + B, counts with A < 2, a gemm_bf16 outside {0, 1, 2}, a negative arm stride and dims
 * mmvae_check_dims rejects as such; MMVAE_E_UNSUPPORTED for shapes outside its limits. */
typedef struct mmvae_encode_out {
    float *x_low;     /* [A,out_rows,L]  low-dimensional representation, BatchNorm5's output                       */
    float *c_prob;    /* [A,out_rows,C]  softmax(fcc(x_low)): the second value of mixVAE_model.encoder             */
    float *c;         /* [A,out_rows,C]  softmax(c_prob / tau) on the categories h->cat_mask keeps, 0 elsewhere    */
    float *c_smp;     /* [A,out_rows,C]  eval: the noise-free hard sample                                          */
    float *s_mean;    /* [A,out_rows,S]                                                                            */
    float *s_logvar;  /* [A,out_rows,S]  log(sigmoid(fc_sigma(y)) + eps)                                           */
    int32_t *labels;  /* [A,out_rows]    argmax of c (first maximum on ties)                                       */
    int64_t *counts;  /* [A(A-1)/2,C,C]  += this call's between-arm confusion counts, as mmvae_eval_classify       */
} mmvae_encode_out;
size_t mmvae_encode_workspace_bytes(const mmvae_dims *d, const mmvae_exec *ex);
int mmvae_encode(const mmvae_dims *d, const mmvae_hyper *h, const mmvae_noise *nz, const float *params, float *bn_running,
                 int64_t *num_batches_tracked, const float *x, int64_t x_arm_stride, const mmvae_encode_out *out,
                 int64_t out_row0, int64_t out_rows, void *ws, size_t ws_bytes, mmvae_exec *ex, void *stream);
int mmvae_intermed(const mmvae_dims *d, const mmvae_hyper *h, const float *params, const float *y, int64_t y_arm_stride,
                   float *mu, float *var, void *stream);

/* ---- the pruning phase: parameters of switched-off categories held at zero ------------------------------------------
 * mmvae_prune_apply: for every arm and every category k < d->C whose bit of cat_mask is clear (bit k set = kept, as
 *   mmvae_hyper.cat_mask; bits at or above C are ignored), writes +0.0f to fcc.weight[k, :], fcc.bias[k],
 *   fc_mu.weight[:, L + k], fc_sigma.weight[:, L + k] and fc6.weight[:, k] of each given flat buffer of the parameter layout
 *   (params, grads, exp_avg, exp_avg_sq: [A * per_arm] floats; any may be NULL and is skipped) -- the five masks of the
 *   reference's pruning loop (mmidas/cpl_mixvae.py:1124-1128), which it applies through torch.nn.utils.prune.custom_from_mask
 *   (:1153-1161).  No other element is written, alignment gaps included.  One launch for all arms and buffers, asynchronous
 *   on `stream`.  Behind mmvae_train_step(do_adam = 1, the same cat_mask in the hyper-parameters) on the step's stream, with
 *   all four buffers, the effective weights are torch's weight_orig * mask after every step; the Adam moments of pruned
 *   entries are held at 0 (torch keeps decaying remnants there, which never reach an effective weight).  The step has joined
 *   its side stream by the time it returns, so stream order is enough.
 * All four words zero = nothing is pruned: returns 0 without a launch.  MMVAE_E_BADARG before any launch: null dims or
 * cat_mask, all four buffers NULL, a mask that keeps none of the C categories. */
int mmvae_prune_apply(const mmvae_dims *d, const uint32_t cat_mask[4], float *params, float *grads, float *exp_avg,
                      float *exp_avg_sq, void *stream);

/* Writes the noise the Philox mode (nz->mode == 1) would use, in explicit-buffer form, so a test
 * can replay a Philox step through mode 0.  Any output pointer may be NULL. */
int mmvae_dump_noise(const mmvae_dims *d, const mmvae_hyper *h, const mmvae_noise *nz,
                     uint8_t *x_mask, float *u_gumbel, float *u_state, uint8_t *s_mask,
                     void *stream);

/* Launches ONE stage of the step on an already prepared workspace (mmvae_forward(need_grad=1) +
 * mmvae_loss [+ mmvae_backward] must have run on it): for per-kernel timing with HIP events and for
 * rocprof runs.  Stages: 0 fc1 forward (split-K GEMM + epilogue), 1 fused fc11 (x_rec GEMM + loss +
 * dZ11 + d(d10) GEMM), 2 dW1 and dW11 GEMMs, 3 batched small-layer dW GEMM, 4 decoder chain forward,
 * 5 decoder chain backward, 6 latent forward, 7 latent backward, 8 gradient slab reduction (grads),
 * 9 dropout keep-mask bit image; single kernels of the fast path: 10 fc11 x_rec/loss/dZ11, 11 d(d10) GEMM,
 * 12 dW1 GEMM, 13 [dW11|db11] GEMM, 14 fc1 GEMM without its epilogue. */
int mmvae_debug_stage(const mmvae_dims *d, const mmvae_hyper *h, const mmvae_noise *nz, int stage,
                      const float *params, const float *x, int64_t x_arm_stride, void *ws,
                      size_t ws_bytes, float *grads, mmvae_exec *ex, void *stream);

/* Host only (no workspace, stream or device call): the per-call plan -- which kernel family, zero fill, stream
 * placement and plane set a call with these arguments would take -- written as MMVAE_PLAN_FIELDS int32 values in the
 * declaration order of `Plan` (csrc/common.hpp: kind, fast, big, small_x3, fc11, gd10_slabs, dw11_slabs, chain_planes,
 * lat_half, narrow, presplit, bwd_small_planes, d10_planes, dz1_in_apply, dec_planes, zero, rowmap, dz11_bf16,
 * dw11_side, loss_on_side, couple, lat_fork_rides, fc11_fork_rides; enumerators by value, bools 0 / 1).  It runs the
 * library's own planner on the dims, the hyper-parameters and a copy of `ex` (null: zeros; a non-null side_stream
 * counts as "has a side stream", its events are not looked at), for the tests that pin every switch point of it.
 *   call_kind      MMVAE_CALL_*: the entry point (STEP mmvae_train_step, STEP_ROWS mmvae_train_step_rows, ...).  DECODE,
 *                  TRAVERSE and CLASSIFY are planned in eval mode (h->training is ignored), as their entry points run;
 *                  ENCODE (mmvae_encode) in the mode h->training states: CLASSIFY's choices in eval mode, the forward half
 *                  of FORWARD's in training mode.
 *   params_align   alignment in bytes of the flat parameter pointer: 16 or more means 16-byte aligned, 4 or 8 a pointer
 *                  that many bytes past a 16-byte boundary.
 *   x_align        the same for x (for DECODE: x_rec).
 *   x_arm_stride   as passed to the entry point (floats).
 *   has_x16        STEP_ROWS only (ignored otherwise): a bf16 copy of the matrix is given.
 *   fc11_grad      mmvae_forward: need_grad && !x_rec (every other entry point: 1). */
#define MMVAE_PLAN_FIELDS 23
#define MMVAE_CALL_STEP 0
#define MMVAE_CALL_STEP_ROWS 1
#define MMVAE_CALL_FORWARD 2
#define MMVAE_CALL_BACKWARD 3
#define MMVAE_CALL_LOSS 4
#define MMVAE_CALL_CLASSIFY 5
#define MMVAE_CALL_REPLAY 6
#define MMVAE_CALL_DECODE 7
#define MMVAE_CALL_TRAVERSE 8
#define MMVAE_CALL_ENCODE 10   /* (9 is not a call kind: mmvae_debug_plan refuses it as unknown, as it always has) */
#define MMVAE_CALL_ZINB_STEP 11   /* mmvae_zinb_train_step: planned without a side stream whatever ex states; gd10_slabs is 1 */
int mmvae_debug_plan(const mmvae_dims *d, const mmvae_hyper *h, const mmvae_exec *ex, int call_kind,
                     int params_align, int x_align, int64_t x_arm_stride, int has_x16, int fc11_grad,
                     int32_t out[MMVAE_PLAN_FIELDS]);

#ifdef __cplusplus
}
#endif
#endif /* MMVAE_H */

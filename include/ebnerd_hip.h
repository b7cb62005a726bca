/*
 * ebnerd_hip.h -- C ABI of the MI355X (gfx950) NRMS / NRMSDocVec hot path.
 *
 * The reference (ebanalyse/ebnerd-benchmark) has no FFI: its hot path is Python
 * calling TensorFlow ops.  This header is the boundary a maintainer would bind
 * instead (ctypes stub in INTEGRATION.md).  Every entry point names the reference
 * interface it replaces (paths relative to src/ebrec/models/newsrec/).
 *
 * Conventions
 *   - all pointers are DEVICE pointers owned by the caller (e.g. torch tensors'
 *     data_ptr()); all matrices are row-major fp32 unless stated otherwise;
 *   - `stream` is a hipStream_t passed as void*; calls only ENQUEUE work on it and
 *     return immediately (no host sync, no allocation -> hipGraph-capturable);
 *   - return 0 on success, a positive hipError_t from the launch, or a negative
 *     EBN_ERR_* argument code (the host layer raises on non-zero);
 *   - no global mutable state: re-entrant, callable from several host threads on
 *     different streams;
 *   - step-dependent scalars (Adam step size, dropout keys) live in a DEVICE
 *     `ebn_step_state` so a captured graph replays with fresh values.
 */
#ifndef EBNERD_HIP_H
#define EBNERD_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EBN_ABI_VERSION 1

#define EBN_OK 0
#define EBN_ERR_BAD_ARG (-1)     /* null pointer / negative size */
#define EBN_ERR_UNSUPPORTED (-2) /* shape outside what the kernels are built for */
#define EBN_ERR_ALIGN (-3)       /* pointer or leading dimension not 16-byte friendly */

typedef void* ebn_stream_t;

/* Dropout call sites (keys in ebn_step_state.drop_key). nrms.py:136 / nrms.py:154 /
 * nrms_docvec.py:124 (site EBN_SITE_MLP0 + layer). */
#define EBN_SITE_NEWS_IN 0
#define EBN_SITE_NEWS_ATT 1
#define EBN_SITE_MLP0 8
#define EBN_N_SITES 12

/* 64-byte device-resident per-step state. */
typedef struct ebn_step_state {
  uint32_t step;       /* optimizer step t, 1-based after the first advance */
  uint32_t seed;       /* model seed (NRMSModel(seed=...), nrms.py:33) */
  float adam_alpha;    /* lr*sqrt(1-b2^t)/(1-b1^t), refreshed by ebn_step_advance */
  float lr;            /* current learning rate (ReduceLROnPlateau rewrites it) */
  uint32_t drop_key[EBN_N_SITES];
} ebn_step_state;

int ebn_abi_version(void);
const char* ebn_error_string(int code);
/* Kernel launches this library has enqueued in this process so far (captured ones included: a launch recorded into a hipGraph counts
 * once, at capture).  Diagnostics: bench.py reports `launches_per_step` as the difference around one eager step.  No reference
 * counterpart (Keras' train_function, nrms.py:92-99 compile + fit, hides its op launches).                                          */
int64_t ebn_launch_count(void);

/* step++ ; adam_alpha and the dropout keys for the new step. One tiny kernel. */
int ebn_step_advance(ebn_step_state* st, double beta1, double beta2, ebn_stream_t stream);

/* ---- a1  tf.keras.layers.Embedding (nrms.py:125-134) ---------------------------
 * out[r,:] = table[ids[r],:] (* inverted-dropout multiplier of nrms.py:136 when
 * drop_p > 0 and st != NULL).  ids outside [0,V) write a zero row and set *oob_flag
 * (may be NULL) to 1: the host layer turns that into an IndexError.               */
int ebn_gather_rows_f32(const int32_t* ids, const float* table, float* out, int64_t n_tok,
                        int32_t D, int64_t V, const ebn_step_state* st, int32_t site,
                        float drop_p, int32_t* oob_flag, ebn_stream_t stream);

/* ---- a13  device-side batch assembly (dataloader.py:169-179: lookup_article_matrix[article rows]) ----------
 * ids_out[r*T + t] = token_matrix[art_idx[r]*T + t]: the loader ships B*(H+C) article-row numbers per step
 * instead of B*(H+C)*T token ids; row 0 of the matrix is the "unknown / padded article" title.  Integer copy,
 * bit-exact.  art_idx outside [0, n_rows) writes zeros and sets *oob_flag (may be NULL).                       */
int ebn_expand_titles_i32(const int32_t* art_idx, const int32_t* token_matrix, int32_t* ids_out,
                          int64_t n_titles, int32_t T, int64_t n_rows, int32_t* oob_flag,
                          ebn_stream_t stream);

/* Backward of a1: dTable[ids[r],:] += dX[r,:] * dropout multiplier. dTable must be
 * zeroed by the caller (dense gradient, Keras-Adam dense semantics).   */
int ebn_embedding_grad_scatter_f32(const int32_t* ids, const float* dX, float* dTable,
                                   int64_t n_tok, int32_t D, int64_t V,
                                   const ebn_step_state* st, int32_t site, float drop_p,
                                   ebn_stream_t stream);

/* Deterministic form of the same backward: gradients are accumulated as 2^40-scaled 64-bit integers (integer
 * atomics are associative, so the result does not depend on the order in which duplicate tokens arrive -- hot rows
 * such as token 0 of padded history get the same bits every run), then ebn_fixed_to_f32 converts the accumulator
 * to the fp32 dense gradient and zeroes it for the next step.  Resolution 9e-13; |sum| must stay below 2^23 -- a single
 * term >= 2^21 (or NaN) or an accumulated |sum| >= 2^22 sets *range_flag (may be NULL) to 1 instead of wrapping silently:
 * the host layer raises FloatingPointError.                                                                       */
int ebn_embedding_grad_scatter_fixed(const int32_t* ids, const float* dX, int64_t* acc, int64_t n_tok,
                                     int32_t D, int64_t V, const ebn_step_state* st, int32_t site,
                                     float drop_p, int32_t* range_flag, ebn_stream_t stream);
/* ebn_embedding_grad_scatter_fixed combines the duplicates among each run of 64 consecutive tokens before they reach the
 * atomics (one atomic per distinct id, column and run: padded titles and Zipfian tokens hammer table row 0 -- reference
 * _behaviors.py:647-654, dataloader.py:43).  This is the plain form, one atomic per non-zero gradient element: same sums
 * bit for bit (wrapping integer addition is associative), kept as the validation / A-B form.                              */
int ebn_embedding_grad_scatter_fixed_atomic(const int32_t* ids, const float* dX, int64_t* acc, int64_t n_tok,
                                            int32_t D, int64_t V, const ebn_step_state* st, int32_t site,
                                            float drop_p, int32_t* range_flag, ebn_stream_t stream);
int ebn_fixed_to_f32(int64_t* acc, float* out, int64_t n, int32_t* range_flag, ebn_stream_t stream);
/* ebn_fixed_to_f32 + ebn_adam_keras_step_f32 in one pass over the table: the gradient is read from the accumulator
 * (which is re-zeroed), never materialised -- the single-GPU step of a trainable table (nrms.py:129 trainable=True with
 * Keras' dense moment decay).  Same arithmetic as the two calls in sequence.                           */
int ebn_adam_keras_step_fixed_f32(float* theta, int64_t* acc, float* m, float* v, int64_t n, const ebn_step_state* st,
                                  double beta1, double beta2, double eps, float grad_scale, int32_t* range_flag,
                                  ebn_stream_t stream);

/* ---- an OPT-IN second precision of the projection matmuls (layers.py:214-226 and their weight gradient): fp32-accurate
 * GEMM on the bf16 matrix pipe.  Each fp32 operand element is split exactly into three bf16 values (8 + 8 + 8 significand
 * bits) and the product keeps the six leading cross terms, each a bf16 MFMA with fp32 accumulation; the dropped terms are
 * below 2^-23 of |a.b| per product, i.e. below the rounding of the fp32 accumulation itself.  Same argument meaning as
 * ebn_gemm_f32 (all four layouts, alpha / beta, leading dimensions); `workspace`: ebn_gemm_split_workspace_bytes(M, N, K) bytes,
 * 16-byte aligned (the bf16 planes of both operands + deterministic split-K partials).  The exact-fp32 kernels stay the default
 * everywhere; ebn_gemm_f32_prec selects by `precision` (0 = exact fp32, 1 = bf16x6 split).                               */
int64_t ebn_gemm_split_workspace_bytes(int64_t M, int64_t N, int64_t K);
int ebn_gemm_f32_split(int32_t transA, int32_t transB, int64_t M, int64_t N, int64_t K, float alpha, const float* A,
                       int64_t lda, const float* B, int64_t ldb, float beta, float* C, int64_t ldc, void* workspace,
                       int64_t workspace_bytes, ebn_stream_t stream);
/* The pieces ebn_gemm_f32_split is made of, for callers that keep an operand's planes across calls or have a producer write
 * them directly.  A plane set = the three bf16 planes of one operand as [plane][K/8][rows][8] (rows padded to 256, K to 16,
 * zero-filled: ebn_planes_bytes(rows, K) bytes, 16-byte aligned) -- `rows` is the operand's non-contracted extent (M or N).
 *   ebn_split_planes_f32         src fp32 row-major [rows][K] (trans = 0) or [K][rows] (trans = 1, transposed on the way)
 *   ebn_gather_split_planes_f32  the training step's Embedding + Dropout (nrms.py:125-136) in split precision: token r's row
 *                                table[ids[r]] with the dropout stream of ebn_gather_rows_f32 (same mask bit for bit), written as
 *                                planes in BOTH orientations -- planes_n (rows = tokens, K = D: the A operand of X.Wqkv) and
 *                                planes_t (rows = D, K = tokens: the A operand of X^T.dQKV) -- instead of the fp32 X
 *   ebn_gemm_planes_f32          C[M,N] = alpha * A.B^T + beta * C from two plane sets (A: rows M, B: rows N, same K);
 *                                workspace: ebn_gemm_planes_workspace_floats(M, N, K) floats (deterministic split-K partials) */
int64_t ebn_planes_bytes(int64_t rows, int64_t K);
int ebn_split_planes_f32(const float* src, int64_t ld, int64_t rows, int64_t K, int32_t trans, void* planes,
                         ebn_stream_t stream);
int ebn_gather_split_planes_f32(const int32_t* ids, const float* table, int64_t n_rows, int32_t D, int64_t V,
                                const ebn_step_state* st, int32_t site, float drop_p, int32_t* oob_flag, void* planes_n,
                                void* planes_t, ebn_stream_t stream);
int64_t ebn_gemm_planes_workspace_floats(int64_t M, int64_t N, int64_t K);
int ebn_gemm_planes_f32(const void* a_planes, int64_t M, const void* b_planes, int64_t N, int64_t K, float alpha, float beta,
                        float* C, int64_t ldc, float* workspace, int64_t workspace_floats, ebn_stream_t stream);
int64_t ebn_gemm_prec_workspace_bytes(int64_t M, int64_t N, int64_t K, int32_t precision);
int ebn_gemm_f32_prec(int32_t transA, int32_t transB, int64_t M, int64_t N, int64_t K, float alpha, const float* A,
                      int64_t lda, const float* B, int64_t ldb, float beta, float* C, int64_t ldc, void* workspace,
                      int64_t workspace_bytes, int32_t precision, ebn_stream_t stream);

/* ---- row-sharded Embedding (BASELINE.json configs[4]; no reference counterpart: nrms.py:125-134 keeps one table on
 * one device) -- device-side plan of a lookup into a table whose rows are split over `world` ranks (rank o owns the
 * block [o*per, (o+1)*per), per = ceil(V/world); or, cyclic != 0, the ids = o mod world).  Dedups the n_tok local ids
 * and lays the distinct ones out in FIXED-CAPACITY per-owner request lists, so the two exchanges of a lookup are
 * equal-split all-to-alls with host-known sizes (no host sync, hipGraph-capturable):
 *   slot_rows[o*cap + j]  owner-local row number of the j-th distinct id wanted from owner o (ascending), -1 = padding
 *                         (what ebn_gather_rows_f32 / ebn_embedding_grad_scatter_f32 take as `ids` on the owner's side)
 *   inv[t]                o*cap + j of token t: its row in the received (world*cap, D) buffer; -1 for an id outside [0,V)
 *   counts[0..world)      distinct ids wanted from each owner;  counts[world] = 1 when a list overflowed `cap` (ids were
 *                         dropped: the caller must fail the step);  counts[world+1] = 1 when an id was out of range.
 *                         The two flag words are STICKY (only ever raised here; the caller zeroes them before the first
 *                         call and whenever it has read them), so one host read per epoch sees every step's overflow
 * `workspace`: ebn_shard_plan_workspace_ints(V, world) int32 of scratch.  Integer work only, deterministic.          */
int64_t ebn_shard_plan_workspace_ints(int64_t V, int32_t world);
int ebn_shard_plan_i32(const int32_t* ids, int64_t n_tok, int64_t V, int32_t world, int32_t cyclic, int64_t cap,
                       int32_t* workspace, int32_t* slot_rows, int32_t* inv, int32_t* counts, ebn_stream_t stream);

/* ---- K.dot / Dense matmuls (layers.py:65,214,220,226; nrms_docvec.py:116,130) ----
 * C[M,N] = alpha * op(A)[M,K] * op(B)[K,N] + beta * C, exact-fp32 MFMA
 * (v_mfma_f32_32x32x2_f32). transA=0: A is [M,K] (lda>=K); transA=1: A is [K,M].
 * transB=0: B is [K,N]; transB=1: B is [N,K].                                      */
int ebn_gemm_f32(int32_t transA, int32_t transB, int64_t M, int64_t N, int64_t K, float alpha,
                 const float* A, int64_t lda, const float* B, int64_t ldb, float beta, float* C,
                 int64_t ldc, ebn_stream_t stream);
/* Same, with a caller-owned scratch buffer that enables deterministic split-K for skinny
 * outputs (weight gradients: M,N ~ 1e3, K = all tokens of the batch).
 * ebn_gemm_workspace_floats() returns the size the planner can use for (M,N,K).
 * NOTE: which kernel family runs DEPENDS on the scratch given: with no / too little of it a skinny product runs unsplit on
 * the block tiles (or the 32 x 32 small-output tiles), with enough of it as split-K slices or -- transposed-A, small output,
 * K >= 4096 -- as the K-chunked 16 x 16-block kernel (csrc/ebn_gemm_direct.hip), whose slices ebn_gemm_workspace_floats()
 * already covers.  Results agree to fp32 summation order; callers that need bit-identical reruns keep the size fixed.  */
int64_t ebn_gemm_workspace_floats(int64_t M, int64_t N, int64_t K);
/* The plan the launcher will use for (M,N,K) with `workspace_floats` of scratch: block tile bm x bn (128x128, 64x64 or
 * the tall 256x64 that removes column padding / last-turn idling, e.g. N = 1200) and the split-K factor.  Diagnostic:
 * lets bench.py and profiler summaries name the kernel instantiation that runs.                                    */
int ebn_gemm_plan(int64_t M, int64_t N, int64_t K, int64_t workspace_floats, int32_t* bm, int32_t* bn, int32_t* splits);
int ebn_gemm_f32_ws(int32_t transA, int32_t transB, int64_t M, int64_t N, int64_t K, float alpha,
                    const float* A, int64_t lda, const float* B, int64_t ldb, float beta, float* C,
                    int64_t ldc, float* workspace, int64_t workspace_floats, ebn_stream_t stream);

/* The product WITHOUT its combining pass: alpha * op(A).op(B) is left in `workspace` as *n_parts dense [M][N] slices whose sum it
 * is -- the deterministic split-K partials of a weight-gradient GEMM (K.dot backward, layers.py:65,214-226), or the product
 * itself as one slice when the plan does not split K.  ebn_grad_finish_f32 (EBN_FINISH_SPLITK job) sums them, together with the
 * other small finishing passes of the step, in one launch.  workspace: ebn_gemm_partials_workspace_floats(M, N, K) floats
 * (with fewer, down to M * N, the plan settles for fewer slices); *n_parts is a HOST out-parameter, known when the call returns. */
int64_t ebn_gemm_partials_workspace_floats(int64_t M, int64_t N, int64_t K);
int ebn_gemm_f32_partials(int32_t transA, int32_t transB, int64_t M, int64_t N, int64_t K, float alpha, const float* A,
                          int64_t lda, const float* B, int64_t ldb, float* workspace, int64_t workspace_floats,
                          int32_t* n_parts, ebn_stream_t stream);

/* ---- the finishing passes of a training step's backward as ONE launch ----------------------------------------------------
 * Second stages of deterministic reductions their producers left out (see ebn_gemm_f32_partials, ebn_attpool_bwd_dpre_f32,
 * ebn_user_head_train_f32); same summation order as the stand-alone passes, hence the same bits.  `jobs` is a HOST array (copied
 * into the launch).  kind EBN_FINISH_SPLITK: out0[r * ld + c] = sum_z partials[z][r][c] (+ beta * out0), z < n_parts, r < rows,
 * c < cols.  EBN_FINISH_COLRED: partials [n_parts][2][cols] -> out0[c] = scale * sum_p partials[p][0][c], out1 likewise with
 * [p][1][c] (accumulated into when beta != 0).  EBN_FINISH_HEAD: partials [rows][2][cols] -> out0 = d(q), out1 = d(b) summed
 * over the rows in a fixed order, loss_out[0] = sum(loss_rows[0 .. rows)).  Jobs get consecutive block ranges in list order and
 * blocks are dispatched in order: list the latency-bound jobs (COLRED, HEAD: a few blocks, long chains) before the bulk sums.   */
#define EBN_FINISH_SPLITK 0
#define EBN_FINISH_COLRED 1
#define EBN_FINISH_HEAD 2
#define EBN_FINISH_MAX_JOBS 6
typedef struct {
  int32_t kind;
  int32_t n_parts;
  int64_t rows, cols;
  const float* partials;
  float* out0;
  float* out1;
  int64_t ld;
  float beta, scale;
  const float* loss_rows;
  float* loss_out;
} ebn_finish_job;
int ebn_grad_finish_f32(const ebn_finish_job* jobs, int32_t n_jobs, ebn_stream_t stream);

/* ONE-RANK steps: the same finishing launch with the optimizer inside (nrms.py:69-80; with world > 1 the gradient all-reduce sits
 * between the gradients and Adam: ebn_grad_finish_f32 + ebn_adam_keras_step_f32 stay).  theta / grad / m / v: the flat parameter,
 * gradient and Adam-moment buffers (identical offsets, numel floats each); every out0 / out1 of `jobs` must point into `grad`.
 * Keras-form Adam (the arithmetic of ebn_adam_keras_step_f32, element by element) is applied to each gradient element a job finishes,
 * by the thread that has just written it, and -- in blocks behind the jobs' -- to the `rest` ranges (offset, length in floats) of the
 * flat buffers: the parameters whose gradients earlier launches of the step wrote complete.  Together the jobs' outputs and the rest
 * ranges must cover every parameter exactly once (the caller's contract; nothing checks it).                                      */
#define EBN_ADAM_FLAT_MAX_REST 12
typedef struct ebn_adam_flat {
  float* theta;
  const float* grad;
  float* m;
  float* v;
  int64_t numel;
  double beta1, beta2, eps;
  float grad_scale;
  int32_t n_rest;
  int64_t rest_off[EBN_ADAM_FLAT_MAX_REST];
  int64_t rest_len[EBN_ADAM_FLAT_MAX_REST];
} ebn_adam_flat;
int ebn_grad_finish_adam_f32(const ebn_finish_job* jobs, int32_t n_jobs, const ebn_adam_flat* adam, const ebn_step_state* st,
                             ebn_stream_t stream);

/* Same again; `site` is accepted and ignored (rounds 1-4 used it to label the kernel instantiation of the encoders' Q|K|V
 * projection for per-kernel profiler summaries; the instantiations it doubled are gone).                        */
int ebn_gemm_f32_site(int32_t transA, int32_t transB, int64_t M, int64_t N, int64_t K, float alpha,
                      const float* A, int64_t lda, const float* B, int64_t ldb, float beta, float* C,
                      int64_t ldc, float* workspace, int64_t workspace_floats, int32_t site,
                      ebn_stream_t stream);

/* ---- a3/a6  SelfAttention core (layers.py:231-252) -------------------------------
 * qkv [n_seq*L, ld_qkv] holds Q | K | V in column blocks [0,E) [E,2E) [2E,3E), E=h*d.
 * out[n,j,a*d+c] = sum_i softmax_j'(Q_i.K_j'/sqrt(d))[i,j] * V[i,c]   (P^T V, line 249)
 * times the dropout multiplier of nrms.py:154 when drop_p > 0.
 * Supported: L <= 256, d <= 32 (MFMA kernels for L <= 32 and d in {16, 20, 32}; VALU/LDS kernels otherwise);
 * EBN_ERR_UNSUPPORTED beyond.                                                        */
int ebn_attn_fwd_f32(const float* qkv, int64_t ld_qkv, float* out, int64_t ld_out, int64_t n_seq,
                     int32_t L, int32_t h, int32_t d, const ebn_step_state* st, int32_t site,
                     float drop_p, ebn_stream_t stream);
/* dqkv (same layout as qkv) from d(out); the dropout multiplier is re-derived.     */
int ebn_attn_bwd_f32(const float* qkv, int64_t ld_qkv, const float* dout, int64_t ld_dout,
                     float* dqkv, int64_t ld_dqkv, int64_t n_seq, int32_t L, int32_t h, int32_t d,
                     const ebn_step_state* st, int32_t site, float drop_p, ebn_stream_t stream);
/* The same backward when the attention output fed an AttLayer2 pooling (layers.py:79-81): the pooling term of d(Y),
 * pool_w[n*L + l] * pool_dout[n, :], is added to `dout` on the fly, so the GEMM that produces dout = dpre.W^T needs no
 * rank-1 epilogue.  MFMA path only (ebn_attn_bwd_pooled_supported(L, d), 16-byte aligned operands, ld % 4 == 0):
 * EBN_ERR_UNSUPPORTED otherwise -- callers then use ebn_gemm_f32_rank1 + ebn_attn_bwd_f32.                            */
int ebn_attn_bwd_pooled_f32(const float* qkv, int64_t ld_qkv, const float* dout, int64_t ld_dout, const float* pool_w,
                            const float* pool_dout, int64_t ld_pool, float* dqkv, int64_t ld_dqkv, int64_t n_seq,
                            int32_t L, int32_t h, int32_t d, const ebn_step_state* st, int32_t site, float drop_p,
                            ebn_stream_t stream);
int ebn_attn_bwd_pooled_supported(int32_t L, int32_t d);

/* C[M,N] = alpha * A[M,K] * B[N,K]^T + row_scale[m] * seq_rows[m / L, n]   (C overwritten; A row-major, B stored [N,K]).
 * The d(x) of AttLayer2 in one pass: dpre.W^T (backward of K.dot(x, W), layers.py:65) plus w[n,l]*dout[n,:] (backward of
 * the weighted sum, layers.py:79-81) -- the rank-1 term is added in the GEMM epilogue instead of being written by
 * ebn_attpool_bwd_pool_f32 and read back through beta = 1.  workspace as for ebn_gemm_f32_ws(0, 1, M, N, K).       */
int ebn_gemm_f32_rank1(int64_t M, int64_t N, int64_t K, float alpha, const float* A, int64_t lda, const float* B,
                       int64_t ldb, float* C, int64_t ldc, const float* row_scale, const float* seq_rows,
                       int64_t ld_seq, int32_t L, float* workspace, int64_t workspace_floats, ebn_stream_t stream);

/* Both gradient GEMMs of Y[R,N_out] = X[R,K_in] . W[K_in,N_out] (K.dot at layers.py:65,214,220,226; Dense at
 * nrms_docvec.py:116,130 -- what tf.GradientTape emits for a MatMul):
 *   dW[K_in,N_out] = X^T . dY + beta_w * dW          dX[R,K_in] = dY . W^T          (all row-major)
 * They are independent of each other; when both are small-output shapes with 16-byte-aligned operands they run as ONE
 * launch (each alone leaves half of the chip idle and costs a launch of the step's dependent chain), otherwise as two
 * ebn_gemm_f32_ws calls.  dW, dX must not alias the inputs; workspace as for the larger of the two plain calls.        */
int ebn_dense_bwd_pair_f32(int64_t R, int64_t K_in, int64_t N_out, const float* X, int64_t ldx, const float* dY,
                           int64_t lddy, const float* W, int64_t ldw, float beta_w, float* dW, int64_t lddw, float* dX,
                           int64_t lddx, float* workspace, int64_t workspace_floats, ebn_stream_t stream);

/* C[M,N] = max(A[M,K] * B[K,N] + bias[n], 0): tf.keras.layers.Dense(units, activation="relu") forward
 * (nrms_docvec.py:116-119,130; nrms.py:143-146) in one pass -- bias and ReLU ride in the GEMM epilogue (or in its
 * split-K reduce) instead of a separate element-wise launch.  workspace as for ebn_gemm_f32_ws(0, 0, M, N, K).    */
int ebn_dense_relu_fwd_f32(int64_t M, int64_t N, int64_t K, const float* A, int64_t lda, const float* B, int64_t ldb,
                           const float* bias, float* C, int64_t ldc, float* workspace, int64_t workspace_floats,
                           ebn_stream_t stream);

/* ---- a4/a7  AttLayer2 (layers.py:55-81) after the x.W matmul ----------------------
 * fwd: U <- tanh(U + b) in place ([R,A], R = n_seq*L); e = U.q; a = exp(e);
 *      w = a/(sum_l a + 1e-7); out[n,:] = sum_l w[n,l] X[n,l,:].                    */
int ebn_attpool_fwd_f32(float* U, const float* b, const float* q, const float* X, float* out,
                        float* w, int64_t n_seq, int32_t L, int32_t E, int32_t A,
                        ebn_stream_t stream);
/* bwd step 1: dX[n,l,:] = w[n,l]*dout[n,:]; de[n,l] = w (dw - sum w dw), dw = dout.X.
 * dX may be NULL: only de is produced (the caller adds the dX term with ebn_gemm_f32_rank1). */
int ebn_attpool_bwd_pool_f32(const float* X, const float* w, const float* dout, float* dX,
                             float* de, int64_t n_seq, int32_t L, int32_t E,
                             ebn_stream_t stream);
/* bwd step 2: dq[k] = sum_r de[r] U[r,k]; U <- dpre = de*q*(1-U^2) in place;
 * db[k] = sum_r dpre[r,k].  `partials` is scratch of ebn_attpool_partials_len(R, A)
 * floats; dq/db are ACCUMULATED into when accumulate != 0 (else overwritten).
 * dq == db == NULL: only the row-block partials are written -- their sum is left to ebn_grad_finish_f32
 * (EBN_FINISH_COLRED job: partials, n_parts = ebn_attpool_partials_len(R, A) / (2 A) row blocks, cols = A).  */
int64_t ebn_attpool_partials_len(int64_t R, int32_t A);
int ebn_attpool_bwd_dpre_f32(float* U, const float* q, const float* de, float* dq, float* db,
                             float* partials, int64_t R, int32_t A, int32_t accumulate,
                             ebn_stream_t stream);
/* ---- stage level: SelfAttention + AttLayer2 over a batch of sequences -----------------
 * The news encoder after its embedding gather (nrms.py:137-156, L = title_size,
 * Din = word_emb_dim) and the user encoder after TimeDistributed(news encoder)
 * (nrms.py:108-111, L = history_size, Din = E) are the same stage:
 *   QKV = X.Wqkv ; Y = drop(P^T V) ; U = tanh(Y.W + b) ; w = exp(U.q)/(sum+1e-7) ; out = sum w Y
 * Wqkv is [Din, 3E] = WQ | WK | WV side by side (layers.py:155-172 have no bias).
 * All activation buffers are caller-allocated and are what the backward needs.          */
typedef struct ebn_encoder_dims {
  int64_t n_seq; /* sequences in this call */
  int32_t L;     /* sequence length */
  int32_t Din;   /* input feature width */
  int32_t h, d;  /* heads, head width; E = h*d */
  int32_t A;     /* attention_hidden_dim */
  int32_t drop_site; /* EBN_SITE_* of the dropout after self-attention, or -1 */
  float drop_p;
} ebn_encoder_dims;

typedef struct ebn_encoder_params {
  const float* Wqkv; /* [Din, 3E] */
  const float* W;    /* [E, A]  */
  const float* b;    /* [A]     */
  const float* q;    /* [A]     */
} ebn_encoder_params;

typedef struct ebn_encoder_acts {
  const float* X; /* [R, Din] input rows, R = n_seq*L */
  float* QKV;     /* [R, 3E] */
  float* Y;       /* [R, E]  (after dropout) */
  float* U;       /* [R, A]  tanh output */
  float* w;       /* [R]     attention weights */
  float* out;     /* [n_seq, E] */
} ebn_encoder_acts;

typedef struct ebn_encoder_grads {
  float* dWqkv; /* [Din, 3E] */
  float* dW;    /* [E, A] */
  float* db;    /* [A] */
  float* dq;    /* [A] */
} ebn_encoder_grads;

typedef struct ebn_encoder_scratch {
  float* dY;    /* [R, E]  */
  float* dQKV;  /* [R, 3E] */
  float* de;    /* [R]     */
  float* partials;        /* ebn_attpool_partials_len(R, A) floats */
  float* gemm_ws;         /* split-K scratch, may be NULL */
  int64_t gemm_ws_floats;
} ebn_encoder_scratch;

/* scratch may be NULL; when given, its gemm_ws lets the two projection GEMMs of a SMALL batch of sequences
 * (the user encoder: B*H rows) use split-K to fill the chip (only gemm_ws / gemm_ws_floats are read).    */
int ebn_encoder_fwd_f32(const ebn_encoder_dims* dims, const ebn_encoder_params* params,
                        const ebn_encoder_acts* acts, const ebn_encoder_scratch* scratch,
                        const ebn_step_state* st, ebn_stream_t stream);
/* ebn_encoder_fwd_f32 of the news encoder in INFERENCE mode with the embedding gather fused into the projection
 * (nrms.py:125-139 without the training-only Dropout of :136): row r of the projection's A operand is table[ids[r], :],
 * fetched table -> LDS -> MFMA; X (a->X) is neither read nor written.  ids outside [0, table_rows) read row 0 and set
 * *oob_flag (may be NULL).  EBN_ERR_UNSUPPORTED (nothing launched) when the shape is outside the fused kernel's
 * (fewer than 256 token rows, unaligned operands, a table of 4 GB or more): the caller gathers and calls ebn_encoder_fwd_f32. */
int ebn_encoder_fwd_gather_f32(const ebn_encoder_dims* dims, const ebn_encoder_params* params, const ebn_encoder_acts* acts,
                               const ebn_encoder_scratch* scratch, const int32_t* ids, const float* table, int64_t table_rows,
                               int32_t* oob_flag, ebn_stream_t stream);
/* The fused product by itself: C (M, N) = table[ids[0..M), :] (K columns, leading dimension ldt) . B (K, N).  Same contract. */
int ebn_gemm_f32_rowmap(const int32_t* ids, int64_t table_rows, int64_t M, int64_t N, int64_t K, const float* table,
                        int64_t ldt, const float* B, int64_t ldb, float* C, int64_t ldc, int32_t* oob_flag, ebn_stream_t stream);

/* dout [n_seq, E] -> parameter gradients (accumulated when accumulate != 0) and, when dX is
 * non-NULL, dX [R, Din] (overwritten).  acts->U is consumed (overwritten with d(pre-tanh)). */
int ebn_encoder_bwd_f32(const ebn_encoder_dims* dims, const ebn_encoder_params* params,
                        const ebn_encoder_acts* acts, const float* dout,
                        const ebn_encoder_grads* grads, const ebn_encoder_scratch* scratch,
                        float* dX, int32_t accumulate, const ebn_step_state* st,
                        ebn_stream_t stream);

/* The user encoder and the scorer of a TRAINING step in one call: ebn_encoder_fwd_f32 on the B sequences of L news vectors
 * (nrms.py:108-111), Dot + softmax + compiled loss (nrms.py:201-202, 56-67) against cand [B*C, E] / labels [B*C], and the
 * backward of both into dcand [B*C, E], dX [B*L, Din] (the history news vectors) and the user encoder's weight gradients
 * (overwritten).  When ebn_user_head_supported(L, C, E, A) and ebn_attn_bwd_pooled_supported(L, d) hold and
 * `head_partials` (ebn_user_head_partials_len(B, A) floats) is given, everything between the two GEMM groups is
 * ebn_user_head_train_f32 -- one launch instead of six; otherwise ebn_encoder_fwd_f32 + ebn_score_loss_train_f32 +
 * ebn_encoder_bwd_f32 run as they are.  a->out receives the user vectors, duser [B, E] their gradient.              */
int ebn_user_stage_train_f32(const ebn_encoder_dims* dims, const ebn_encoder_params* p, const ebn_encoder_acts* a,
                             const float* cand, const float* labels, float* scores, float* probs, float* loss_rows,
                             float* loss_out, float* dcand, float* duser, const ebn_encoder_grads* g,
                             const ebn_encoder_scratch* s, float* head_partials, float* dX, int32_t C, int32_t loss_kind,
                             float inv_batch, const ebn_step_state* st, ebn_stream_t stream);

/* ---- a8/a9  Dot + softmax/sigmoid + loss (nrms.py:201-205, 56-67) ------------------
 * scores[b,c] = cand[b,c,:].user[b,:]; probs = softmax_c (mode 0) or sigmoid (mode 1). */
int ebn_score_fwd_f32(const float* cand, const float* user, float* scores, float* probs,
                      int64_t B, int32_t C, int32_t E, int32_t mode, ebn_stream_t stream);
/* loss_kind 0: categorical CE on the softmax logits; 1: log_loss as sigmoid CE on the same logits
 * ([KERAS-SEMANTICS] _keras_logits path); 2: log_loss as binary CE on the softmax OUTPUTS clipped to
 * [1e-7, 1-1e-7], -(y log(p^+1e-7) + (1-y) log(1-p^+1e-7)) (SURVEY.md A.5's reading of nrms.py:54,61-62; Keras
 * binary_crossentropy(from_logits=False) on a tensor without cached logits).  Writes loss_rows[b] (already divided so that
 * sum_b loss_rows = batch loss), dscores, dcand[b,c,:], duser[b,:].                   */
int ebn_score_loss_bwd_f32(const float* cand, const float* user, const float* scores,
                           const float* labels, float* loss_rows, float* dcand, float* duser,
                           int64_t B, int32_t C, int32_t E, int32_t loss_kind, float inv_batch,
                           ebn_stream_t stream);
/* Training step: ebn_score_fwd_f32 (softmax mode) + ebn_score_loss_bwd_f32 as ONE launch (same arithmetic), followed by the
 * batch loss loss_out[0] = sum(loss_rows).  nrms.py:201-202 + nrms.py:56-67 and their backward.                      */
int ebn_score_loss_train_f32(const float* cand, const float* user, const float* labels, float* scores, float* probs,
                             float* loss_rows, float* loss_out, float* dcand, float* duser, int64_t B, int32_t C,
                             int32_t E, int32_t loss_kind, float inv_batch, ebn_stream_t stream);
/* The head of a TRAINING step in one launch (+ a small fixed-order reduction): everything between the user encoder's two
 * GEMM groups, all of it local to one impression --
 *   user AttLayer2 after its x.W matmul: U <- tanh(U + b), w = exp(U.q) / (sum + 1e-7), user = sum_l w_l X_l (layers.py:65-81)
 *   -> scores = cand . user, probs = softmax (nrms.py:201-202) -> compiled loss and d(scores) (nrms.py:56-67; loss_kind as above)
 *   -> dcand = ds (x) user, duser = sum_c ds_c cand_c -> AttLayer2 backward: de = w (dw - sum w dw), dw_l = duser . X_l,
 *      U <- d(pre-tanh) = de q (1 - tanh^2), dq = sum de tanh, db = sum d(pre-tanh)
 * i.e. ebn_attpool_fwd_f32 + ebn_score_loss_train_f32 + ebn_attpool_bwd_pool_f32 + ebn_attpool_bwd_dpre_f32 of the USER
 * encoder (same formulas; six links of the step's dependent launch chain become two).  One workgroup per impression keeps
 * its L x A, L x E and C x E rows in LDS: ebn_user_head_supported(L, C, E, A) says whether they fit (E, A multiples of 4;
 * history_size 50 at E = 400, A = 200 does).  U [B*L, A], X [B*L, E], cand / dcand [B*C, E], labels / scores / probs [B*C],
 * w / de [B*L], user / duser [B, E], loss_rows [B], loss_out [1] = sum(loss_rows), dq / db [A] (overwritten),
 * partials: ebn_user_head_partials_len(B, A) floats of scratch.  16-byte aligned pointers.
 * dq == db == NULL: the fixed-order reduction is left to ebn_grad_finish_f32 (EBN_FINISH_HEAD job: partials, rows = B, cols = A,
 * loss_rows -> loss_out); loss_out is not written by this call then.                                                       */
int ebn_user_head_supported(int32_t L, int32_t C, int32_t E, int32_t A);
int64_t ebn_user_head_partials_len(int64_t B, int32_t A);
int ebn_user_head_train_f32(float* U, const float* b, const float* q, const float* X, const float* cand, const float* labels,
                            float* w, float* user, float* scores, float* probs, float* loss_rows, float* loss_out,
                            float* dcand, float* duser, float* de, float* dq, float* db, float* partials, int64_t B,
                            int32_t L, int32_t C, int32_t E, int32_t A, int32_t loss_kind, float inv_batch,
                            ebn_stream_t stream);
/* Streaming AUC of compile(metrics=["AUC"]) (ebnerd_nrms.py:244-248; tf.keras.metrics.AUC defaults): every (label,
 * prediction) pair of a batch goes into pos_hist / neg_hist [n_thresholds + 1] at bucket = number of thresholds strictly
 * below the prediction (`thresholds`: ascending float64 on the device).  Integer atomics: order-independent.           */
int ebn_auc_hist_f32(const float* probs, const float* labels, int64_t n, const double* thresholds, int32_t n_thresholds,
                     int64_t* pos_hist, int64_t* neg_hist, ebn_stream_t stream);
/* ragged scoring for the eval path (dataloader.py:94-107 + nrms.py:204-205):
 * out[p] = act(user[u_idx[p],:] . news[n_idx[p],:]), act = sigmoid (mode 1) or id (0). */
int ebn_pair_score_f32(const float* user, const float* news, const int32_t* u_idx,
                       const int32_t* n_idx, float* out, int64_t n_pairs, int32_t E, int32_t mode,
                       ebn_stream_t stream);

/* ---- a10  tf.keras.optimizers.Adam (nrms.py:69-80), Keras update form -------------
 * m += (g-m)(1-b1); v += (g^2-v)(1-b2); theta -= alpha_t * m/(sqrt(v)+eps), dense over
 * n elements; g is multiplied by grad_scale first (1/world_size after an all-reduce sum).
 * Betas are doubles so that (1-beta) is formed as Keras forms it (Python floats), then cast. */
int ebn_adam_keras_step_f32(float* theta, const float* g, float* m, float* v, int64_t n,
                            const ebn_step_state* st, double beta1, double beta2, double eps,
                            float grad_scale, ebn_stream_t stream);

/* ---- small dense helpers used by the DocVec encoder (nrms_docvec.py:113-135) ------- */
/* Y = relu(X + bias) row-wise, in place allowed (Dense(relu)).                        */
int ebn_bias_relu_f32(const float* X, const float* bias, float* Y, int64_t R, int32_t Ccols,
                      ebn_stream_t stream);
/* dX = dY * (Y > 0); dbias[c] = sum_r dX[r,c] (partials scratch: ebn_colsum_partials_len). */
int64_t ebn_colsum_partials_len(int64_t R, int32_t Ccols);
int ebn_bias_relu_bwd_f32(const float* Y, const float* dY, float* dX, float* dbias,
                          float* partials, int64_t R, int32_t Ccols, int32_t accumulate,
                          ebn_stream_t stream);
/* BatchNormalization(axis=-1, momentum .99, eps 1e-3) over the R rows of one call site.
 * training != 0: batch statistics (biased var), saved to mean_out/istd_out, moving stats
 * updated in place; else moving statistics.  Optional fused dropout (site, drop_p) with
 * flat element offset elem_offset.                                                     */
int ebn_batchnorm_fwd_f32(const float* X, const float* gamma, const float* beta,
                          float* moving_mean, float* moving_var, float* Y, float* xhat,
                          float* mean_out, float* istd_out, float* partials, int64_t R,
                          int32_t Ccols, int32_t training, const ebn_step_state* st,
                          int32_t site, float drop_p, int64_t elem_offset,
                          ebn_stream_t stream);
int ebn_batchnorm_bwd_f32(const float* dY, const float* xhat, const float* gamma,
                          const float* istd, float* dX, float* dgamma, float* dbeta,
                          float* partials, int64_t R, int32_t Ccols, int32_t training,
                          int32_t accumulate, const ebn_step_state* st, int32_t site,
                          float drop_p, int64_t elem_offset, ebn_stream_t stream);
/* The two TimeDistributed call sites of a TRAINING step in one launch each way (rows [0,R0) = history block, [R0,R0+R1)
 * = candidate block of one row block; R0 + R1 <= 1024, else EBN_ERR_UNSUPPORTED and the caller uses the per-site entry
 * points): forward = two ebn_batchnorm_fwd_f32 (own batch statistics, two moving-average updates, history first; the
 * dropout stream is indexed by the element's position in the whole block); backward = two ebn_batchnorm_bwd_f32 with
 * dgamma/dbeta summed over the sites, followed by ebn_bias_relu_bwd_f32 of the Dense(relu) in front (relu_out = that
 * Dense's output): dX = d(pre-activation), dbias = its column sums.  nrms_docvec.py:116-124, nrms.py:143-152.          */
int ebn_batchnorm2_fwd_f32(const float* X, const float* gamma, const float* beta, float* moving_mean, float* moving_var,
                           float* Y, float* xhat, float* mean_out0, float* istd_out0, float* mean_out1, float* istd_out1,
                           int64_t R0, int64_t R1, int32_t Ccols, const ebn_step_state* st, int32_t site, float drop_p,
                           ebn_stream_t stream);
int ebn_batchnorm2_relu_bwd_f32(const float* dY, const float* xhat, const float* relu_out, const float* gamma,
                                const float* istd0, const float* istd1, float* dX, float* dgamma, float* dbeta,
                                float* dbias, int64_t R0, int64_t R1, int32_t Ccols, const ebn_step_state* st, int32_t site,
                                float drop_p, ebn_stream_t stream);

/* ---- a11 as ONE launch per Dense layer and direction (nrms_docvec.py:113-135, training step) ------------------------
 * x -> [Dense(u_l, relu, l2) -> BatchNormalization -> Dropout] x n_layers -> Dense(e_out, relu) over the rows of the two
 * TimeDistributed call sites (rows [0,n0) = history block, [n0,n0+n1) = candidate block: own batch statistics and one
 * moving-average update each, history first; nrms_docvec.py:88-90,176-178).  BatchNormalization, Dropout and the ReLU
 * backward never run as passes of their own: the matmul in front leaves per-tile column partials, the matmul behind
 * combines them and transforms its A operand on the way into LDS (csrc/ebn_docvec.hip).  Same arithmetic as
 * ebn_dense_relu_fwd_f32 + ebn_batchnorm2_fwd_f32 / ebn_batchnorm2_relu_bwd_f32 + ebn_bias_relu_bwd_f32 up to fp32
 * rounding (the column sums are order-independent 64-bit fixed-point accumulations of per-tile sums, the batch variance
 * is E[x^2] - mean^2 in float64 from them, not two-pass over the block): bitwise reproducible run to run.
 *
 * All pointers device, matrices dense row-major.  X0, W[], R[], Xn[], NE, dNE, dY[], dP[] and stat are accessed as 16-byte vectors
 * or 64-bit words and must be 16-byte aligned: EBN_ERR_ALIGN otherwise (the per-column vectors b, gamma, beta, the moving statistics,
 * ggamma and gbeta only 4-byte).  A NULL among the pointers a call uses is EBN_ERR_BAD_ARG, a shape outside ebn_dvn_supported
 * EBN_ERR_UNSUPPORTED.  Both calls validate EVERYTHING in front of their first launch: a refused call has launched nothing and
 * written nothing, `stat` included.  W[l] is (d_l, u_l) with d_0 = din, W[n_layers] the
 * output kernel (u_last, e_out); b[l] likewise.  Forward writes R[l] = relu(Dense_l), Xn[l] = Dropout(BN(R[l])), NE, the
 * batch statistics (inside `stat`) and the moving statistics.  Backward reads dNE and writes dY[l] = d(Xn[l]) with the
 * dropout mask applied, dP[l] = d(pre-activation of Dense l) for l = 0..n_layers (the B operands of the weight gradients
 * W[l]' = Xn[l-1]^T . dP[l], bias gradient = column sums of dP[l]: ebn_gemm_tn_group_f32), ggamma / gbeta, and adds
 * l2 * sum_l sum(W[l]^2), l < n_layers, to loss[0] (loss may be NULL; the 2*l2*W term of the kernel gradients is the
 * l2_W option of ebn_gemm_tn_group_f32).
 * ebn_dvn_supported: 1 <= n_layers <= 4, widths multiples of 4, hidden widths <= 1024.
 * `stat`: ebn_dvn_stat_floats(args) floats, 16-byte aligned, ZERO before the first forward call, then owned by the two
 * calls: it must survive from the forward to the backward call of a step, and every forward call must be followed by the
 * backward call of the same step before the next forward (the accumulators inside are re-zeroed by the step's own
 * launches: the backward ones by the first forward launch, the forward ones by the last backward launch).  After a step
 * that ran only half way the caller zeroes `stat` again.                                                               */
#define EBN_DVN_MAX_LAYERS 4
typedef struct ebn_dvn_args {
  int32_t n_layers, din, e_out;
  int32_t units[EBN_DVN_MAX_LAYERS];
  int32_t n0, n1;
  float drop_p, l2;
  const float* W[EBN_DVN_MAX_LAYERS + 1];
  const float* b[EBN_DVN_MAX_LAYERS + 1];
  const float* gamma[EBN_DVN_MAX_LAYERS];
  const float* beta[EBN_DVN_MAX_LAYERS];
  float* moving_mean[EBN_DVN_MAX_LAYERS];
  float* moving_var[EBN_DVN_MAX_LAYERS];
  const float* X0;
  float* R[EBN_DVN_MAX_LAYERS];
  float* Xn[EBN_DVN_MAX_LAYERS];
  float* NE;
  float* stat;
  const float* dNE;
  float* dY[EBN_DVN_MAX_LAYERS];
  float* dP[EBN_DVN_MAX_LAYERS + 1];
  float* ggamma[EBN_DVN_MAX_LAYERS];
  float* gbeta[EBN_DVN_MAX_LAYERS];
  float* loss;
  int32_t* range_flag; /* may be NULL.  Set to 1 (never cleared) when a tile's column sum is not finite or leaves the range of the
                          fixed-point accumulators: the statistics of that step are invalid, the run has diverged               */
} ebn_dvn_args;
int ebn_dvn_supported(const ebn_dvn_args* args);
int64_t ebn_dvn_stat_floats(const ebn_dvn_args* args);
int ebn_dvn_fwd_train_f32(const ebn_dvn_args* args, const ebn_step_state* st, ebn_stream_t stream);
int ebn_dvn_bwd_f32(const ebn_dvn_args* args, const ebn_step_state* st, ebn_stream_t stream);

/* The prologue of an NRMSDocVec training step on a device-resident batch of article-row numbers (dataloader.py:169-179,
 * lookup_article_matrix[rows]) as ONE launch: ebn_step_advance (st may be NULL: no advance) + the label copy (n_labels floats) +
 * X0[r,:] = matrix[idx[r],:] for the n0 + n1 rows of the (up to two) index segments idx0 | idx1 -- what ebn_copy3_advance +
 * ebn_gather_rows_f32 do in two.  Rows outside [0, n_rows) write zeros and set *oob_flag (may be NULL).  din % 4 == 0.
 * An empty segment may be NULL; n0 = n1 = 0 (both NULL) copies the labels, advances the step state and writes nothing else.  */
int ebn_docvec_stage_gather_f32(const int32_t* idx0, int64_t n0, const int32_t* idx1, int64_t n1, const float* labels_src,
                                float* labels_dst, int64_t n_labels, const float* matrix, int64_t n_rows, int32_t din, float* X0,
                                int32_t* oob_flag, ebn_step_state* st, double beta1, double beta2, ebn_stream_t stream);

/* Up to EBN_TN_GROUP_MAX independent weight-gradient products C_i (M_i, N_i) = A_i^T . B_i (A_i (K_i, M_i), B_i (K_i, N_i),
 * all row-major) in ONE launch of 32x32 small-output tiles -- the Dense kernel gradients of a step (nrms_docvec.py:116-134
 * backward; the user encoder's K.dot gradients of layers.py:65,214-226), each too small to fill the chip alone.  Options per
 * problem: colsum (N_i floats) = column sums of B_i over K_i (the bias gradient of the same Dense layer, taken from the B
 * tiles as they pass); l2_W (M_i, N_i, leading dimension ldc) adds two_lambda * l2_W to C_i (kernel_regularizer=l2).
 * 16-byte aligned operands, extents and leading dimensions multiples of 4; EBN_ERR_UNSUPPORTED otherwise.              */
#define EBN_TN_GROUP_MAX 8
typedef struct ebn_tn_problem {
  int64_t M, N, K;
  const float* A;
  int64_t lda;
  const float* B;
  int64_t ldb;
  float* C;
  int64_t ldc;
  float* colsum;
  const float* l2_W;
  float two_lambda;
} ebn_tn_problem;
int ebn_gemm_tn_group_f32(const ebn_tn_problem* problems, int32_t n, ebn_stream_t stream);

/* The closing launch of a ONE-RANK NRMSDocVec training step (nrms_docvec.py:99-188 backward + nrms.py:69-80): the Dense weight
 * gradients of ebn_gemm_tn_group_f32 (`problems`: every C_i / colsum_i must lie inside the flat gradient buffer `grad`) and, dealt over
 * the same workgroups instead of launches of their own, (1) Keras-form Adam -- in the epilogue of the tile that has just produced a
 * gradient element, and element-wise over the `rest` ranges (offset, length in floats) of the flat buffers, i.e. every parameter no
 * tile owns; theta / grad / m / v are the flat parameter, gradient and moment buffers with identical offsets, `numel` floats each --
 * (2) the user head's finishing sums (ebn_user_head_train_f32 called with dq == db == NULL leaves `head_partials`, `loss_rows`):
 * d(q), d(b) over the B impressions and loss_out[0] = sum(loss_rows) + l2 * sum_l sum(W[l]^2) (ebn_dvn_bwd_f32 called with
 * args->loss == NULL leaves the L2 term to this call), then Adam on d(q) / d(b).  Same arithmetic, element by element, as
 * ebn_gemm_tn_group_f32 + ebn_user_head_train_f32's finishing pass + ebn_adam_keras_step_f32 (one Adam element, ebn_adam_flat.h: the
 * same bits).  Any tile count: a group with fewer tiles than the head's ceil(2A / 256) + 1 finishing blocks launches the difference as
 * workgroups without a tile.  With world > 1 the gradient all-reduce sits between the gradients and Adam: the separate calls stay.      */
#define EBN_DVN_FINALE_MAX_REST 12
typedef struct ebn_dvn_finale {
  float* theta;
  const float* grad;
  float* m;
  float* v;
  int64_t numel;
  double beta1, beta2, eps;
  float grad_scale;
  int32_t n_rest;
  int64_t rest_off[EBN_DVN_FINALE_MAX_REST];
  int64_t rest_len[EBN_DVN_FINALE_MAX_REST];
  const float* head_partials;
  int64_t B;
  int32_t A;
  float* dq;
  float* db;
  const float* loss_rows;
  float* loss_out;
} ebn_dvn_finale;
int ebn_dvn_finale_f32(const ebn_dvn_args* args, const ebn_tn_problem* problems, int32_t n, const ebn_dvn_finale* fin,
                       const ebn_step_state* st, ebn_stream_t stream);

/* ---- NPA (npa.py:120-136 news encoder, layers.py:312-339 PersonalizedAttentivePooling) -------------------------------------
 * Dropout sites of an NPA training step (keys in ebn_step_state.drop_key): Dropout(p) after the Conv1D (npa.py:129), the 0.2
 * Dropout at the input of the news-level pooling (layers.py:324) and of the user-level pooling. */
#define EBN_SITE_NPA_CONV 2
#define EBN_SITE_NPA_NEWS_PAP 3
#define EBN_SITE_NPA_USER_PAP 4

/* Conv1D(F, window, activation="relu", padding="same") + Dropout(p) + the pooling's Dropout(0.2) (npa.py:120-129, layers.py:324)
 * as an implicit GEMM on the exact-fp32 MFMA: X [n_titles*T, E] are the gathered (dropped-out) tokens, titles of T rows
 * contiguous; W [window*E, F] is the Keras kernel (window, E, F) flattened, bias [F].  "same" padding: (window-1)/2 rows on
 * the left, the rest on the right, taps outside a title read zero (no im2col image, no padded copy of X).
 *   Vd[r, f] = relu(sum_{j,e} X[r + j - (window-1)/2, e] W[j*E + e, f] + bias[f]) * drop(conv_site, conv_p) * drop(pap_site, pap_p)
 * with the dropout stream of ebn_gather_rows_f32 at element index r*F + f (st == NULL or p == 0: no dropout).  Vd is the only
 * activation the backward needs.  E % 4 == 0, F % 4 == 0, window <= 15, X / W 16-byte aligned (EBN_ERR_UNSUPPORTED /
 * EBN_ERR_ALIGN otherwise).                                                                                                    */
int ebn_conv1d_fwd_f32(const float* X, const float* W, const float* bias, float* Vd, int64_t n_titles, int32_t T, int32_t E,
                       int32_t F, int32_t window, const ebn_step_state* st, int32_t conv_site, float conv_p, int32_t pap_site,
                       float pap_p, ebn_stream_t stream);
/* Backward-data of the same: dX [n_titles*T, E] (overwritten) = the transposed convolution (taps reversed) of
 * dY' = d(pre-activation), which is derived on the fly from the forward's Vd and its gradient dVd [n_titles*T, F]:
 * dY' = dVd / ((1 - conv_p)(1 - pap_p)) where Vd > 0 and 0 elsewhere (Vd > 0 iff the ReLU passed and both masks kept).
 * conv_p / pap_p as given to the forward (st == NULL: no dropout was applied).  Same shape rules; dVd / Vd / W aligned.      */
int ebn_conv1d_bwd_data_f32(const float* dVd, const float* Vd, const float* W, float* dX, int64_t n_titles, int32_t T, int32_t E,
                            int32_t F, int32_t window, const ebn_step_state* st, float conv_p, float pap_p, ebn_stream_t stream);
/* Backward-weight: partials [splits][window*E + 1][F] = deterministic split-K slices (over the token rows) of
 * [dW ; db] = [A(X)^T ; 1^T] . dY' -- rows 0 .. window*E-1 the kernel gradient, row window*E the bias gradient.  Their sum is
 * left to ebn_grad_finish_f32 (EBN_FINISH_SPLITK job: n_parts = splits, rows = window*E + 1, cols = F), i.e. the gradient is
 * the same bits for the same `splits` on every run.  ebn_conv1d_wgrad_splits: the split count the library suggests for the
 * shape (1..64); ebn_conv1d_wgrad_workspace_floats: the size of `partials` for a split count (0 for an invalid problem).     */
int ebn_conv1d_wgrad_splits(int64_t n_titles, int32_t T, int32_t E, int32_t F, int32_t window);
int64_t ebn_conv1d_wgrad_workspace_floats(int64_t n_titles, int32_t T, int32_t E, int32_t F, int32_t window, int32_t splits);
int ebn_conv1d_bwd_weight_f32(const float* X, const float* dVd, const float* Vd, float* partials, int32_t splits, int64_t n_titles,
                              int32_t T, int32_t E, int32_t F, int32_t window, const ebn_step_state* st, float conv_p, float pap_p,
                              ebn_stream_t stream);

/* PersonalizedAttentivePooling after its Dense(A) matmul (layers.py:324-336), one workgroup per sequence n of L rows:
 *   U <- tanh(U + ba) in place ([n_seq*L, A], U = Vd.Wa from ebn_gemm_f32);  s_l = Q[q_idx[n]] . U_l  (Q [n_q, A]: the query
 *   Dense of each impression, npa.py:134 / :99; q_idx a DEVICE int32 [n_seq], rows outside [0, n_q) read row 0);
 *   w = softmax_l(s) (max-subtracted, no +1e-7);  out[n] = sum_l w_l V_l  (V [n_seq*L, F], out [n_seq, F], w [n_seq*L]).
 * out_d (may be NULL): out_d[n] = Dropout(drop_p, site)(out[n]) for n < n_drop (element index n*F + f) -- the 0.2 input
 * dropout of the NEXT pooling (the user encoder's, layers.py:324), written in the same pass.  L <= 256, F <= 4096.        */
int ebn_pap_fwd_f32(float* U, const float* ba, const float* Q, const int32_t* q_idx, int64_t n_q, const float* V, float* out,
                    float* w, float* out_d, int64_t n_drop, int64_t n_seq, int32_t L, int32_t F, int32_t A,
                    const ebn_step_state* st, int32_t site, float drop_p, ebn_stream_t stream);
/* Its backward.  dout [n_seq, F]: rows n < n_drop are first multiplied IN PLACE by the dropout multiplier of (site, drop_p)
 * (the backward of out_d); then dw_l = dout . V_l, ds = w (dw - sum w dw), dq [n_seq, A] = sum_l ds_l U_l (one row per
 * SEQUENCE: ebn_pap_dq_reduce_f32 sums them per query row), U <- d(pre-tanh) = ds q (1 - U^2) in place, and, when dV is not
 * NULL, dV [n_seq*L, F] = w (x) dout (the pooling's direct term; the term through Wa is dpre.Wa^T -- callers that fold both
 * into one pass pass NULL and use ebn_gemm_f32_rank1).                                                                    */
int ebn_pap_bwd_f32(float* U, const float* Q, const int32_t* q_idx, int64_t n_q, const float* V, const float* w, float* dout,
                    float* dV, float* dq, int64_t n_drop, int64_t n_seq, int32_t L, int32_t F, int32_t A,
                    const ebn_step_state* st, int32_t site, float drop_p, ebn_stream_t stream);
/* dQ[i] = sum of dq[n] over the sequences n with q_idx[n] == i, in ascending n (fixed order, no atomics): the per-impression
 * gradient of the query when every impression's H + C titles share its query (npa.py:99-103,185-190).                      */
int ebn_pap_dq_reduce_f32(const float* dq, const int32_t* q_idx, int64_t n_seq, float* dQ, int64_t n_q, int32_t A,
                          ebn_stream_t stream);

/* ---- LSTUR (lstur.py:56-144 user and news encoders, layers.py:55-81 AttLayer2, layers.py:273-309 Compute/OverwriteMasking) ---
 * The news encoder reuses ebn_conv1d_* (Dropout(p) at site EBN_SITE_NPA_CONV, the pooling dropout passed as p = 0) and the
 * AttLayer2 backward (ebn_attpool_bwd_pool_f32 / ebn_attpool_bwd_dpre_f32, linear in w: masked rows get zero gradients).
 *
 * AttLayer2 under the title encoder's mask (lstur.py:136-141): ebn_attpool_fwd_f32 with the token ids [n_seq*L] of the rows:
 *   U <- tanh(U + b) in place;  m_l = (ids_l != 0) && any(X_l != 0)  (OverwriteMasking by token != 0, then Masking());
 *   a_l = m_l exp(U_l . q) (no max-subtraction);  w_l = a_l / (sum a + 1e-7);  out = sum_l w_l X_l.
 * A masked row gets w_l == 0 exactly; a title of padding only gets out == 0.  X is the conv output Vd (not zeroed at
 * padding: the mask covers those rows).                                                                                       */
int ebn_attpool_masked_fwd_f32(float* U, const float* b, const float* q, const float* X, const int32_t* ids, float* out,
                               float* w, int64_t n_seq, int32_t L, int32_t E, int32_t A, ebn_stream_t stream);
/* Masked Keras GRU recurrence (lstur.py:81-104; TF2 GRU defaults: reset_after=True, sigmoid / tanh), B sequences of H steps,
 * enqueued as one launch per step on `stream` (no allocation, no sync: capturable).
 *   gx [B*H, 3U] = X . kernel (one ebn_gemm_f32 beforehand; row b*H + t), X [B*H, F] the history news vectors, Wrec [U, 3U] the
 *   recurrent kernel, bias [2, 3U] (row 0 input, row 1 recurrent); column blocks [z | r | h] throughout.
 *   z = sig(gx_z + b_z + h.Wrec_z + b'_z), r = sig(... r ...), n = tanh(gx_h + b_h + r (h.Wrec_h + b'_h)), h' = z h + (1-z) n;
 *   step t of sequence b is masked (Masking(0.0): h' = h) iff X[b*H + t] is all zero -- derived in the kernel.
 * h0 [B, U] or NULL (zeros).  Out: Hs [H+1, B, U] time-major with Hs[0] = h0 (Hs[H] is the output), act [H, B, 4U] =
 * z | r | n | (h.Wrec_h + b'_h) per step (zeros on masked steps).  F % 4 == 0, U % 4 == 0, H <= 4096, X / Wrec / h0 / Hs
 * 16-byte aligned.                                                                                                            */
int ebn_gru_fwd_f32(const float* gx, const float* X, const float* Wrec, const float* bias, const float* h0, float* Hs,
                    float* act, int64_t B, int32_t H, int32_t F, int32_t U, ebn_stream_t stream);
/* Its backward in reverse time (H + 1 launches): dhH [B, U] = dL/dHs[H] (not modified).  Out: dgx [B*H, 3U] = dL/d(gx + b)
 * (row b*H + t), dgh [H, B, 3U] = dL/d(h.Wrec + b') -- both zero rows on masked steps -- and dh0 [B, U] = dL/dh0 (a masked
 * step passes dh through unchanged).  The weight gradients follow on the GEMMs: dWrec = Hs[0:H]^T . dgh (K = H*B),
 * dkernel = X^T . dgx, dX = dgx . kernel^T, the bias rows are the column sums of dgx and dgh.  Same shape rules; dh0 must not
 * alias dhH; X / Wrec / dgh 16-byte aligned.                                                                                  */
int ebn_gru_bwd_f32(const float* dhH, const float* X, const float* Wrec, const float* Hs, const float* act, float* dgx,
                    float* dgh, float* dh0, int64_t B, int32_t H, int32_t F, int32_t U, ebn_stream_t stream);

/* The same recurrence for scorer.predict over a once-encoded article catalogue (lstur.py:81-104,191-200 with the news encoder
 * taken out of the per-batch work): gx_all [n_rows, 3U] = news_all . kernel of EVERY catalogue row (one ebn_gemm_f32 per predict),
 * live_all [n_rows] int32 = any(news_all[row] != 0) (the Masking(0.0) predicate of ebn_gru_fwd_f32, per article), his_idx [B, H]
 * int32 catalogue rows.  Step t of sequence b reads gx_all[his_idx[b, t]] and is masked when live_all says so; one launch per step,
 * the grid, tile GEMM and gate epilogue of ebn_gru_fwd_f32 (bit-equal to its Hs[H] on the gathered rows).  h moves between h_work
 * and h_out [B, U] (distinct, neither may be h0); the last step writes h_out.  Nothing is kept for a backward pass.  h0 [B, U] or
 * NULL (zeros).  A row number outside [0, n_rows) sets *oob_flag (may be NULL), is never used as an address and masks the step.
 * U % 4 == 0, H <= 4096, Wrec / h0 / h_work / h_out 16-byte aligned.                                                          */
int ebn_gru_infer_indexed_f32(const float* gx_all, const int32_t* live_all, int64_t n_rows, const int32_t* his_idx,
                              const float* Wrec, const float* bias, const float* h0, float* h_work, float* h_out, int64_t B,
                              int32_t H, int32_t U, int32_t* oob_flag, ebn_stream_t stream);

/* ---- NAML (naml.py news encoder: title / body / vert / subvert views, layers.py:55-81 AttLayer2 over the views) -------------
 * Title and body run ebn_gather_rows_f32 -> ebn_conv1d_fwd_f32 (pooling dropout p = 0) -> ebn_attpool_fwd_f32, with their own
 * weights and the shared word table; the title at sites EBN_SITE_NEWS_IN / EBN_SITE_NPA_CONV, the body at the two sites below.
 * The four views of an article are stacked view-major, Vw [n_views, N, F] (view v of article n at row v*N + n).           */
#define EBN_SITE_NAML_BODY_IN 5
#define EBN_SITE_NAML_BODY_CONV 6

/* Both categorical views (naml.py _build_vertencoder / _build_subvertencoder) in one launch, view i = 0, 1:
 *   out_i[n, f] = relu(sum_k table_i[ids_i[n], k] Wb_i[k, f] + Wb_i[K_i, f])   (n < N, f < F; out_i [N, F], e.g. Vw[2], Vw[3])
 * table_i [rows_i, K_i] the Embedding, Wb_i [K_i + 1, F] the Dense kernel rows then its bias row.  K_i <= 256, any value (no
 * multiple-of-4 rule; the contraction runs on the VALU, k ascending).  An id outside [0, rows_i) reads a zero row and sets
 * *oob_flag (may be NULL) to 1.  No alignment requirement.                                                                   */
int ebn_naml_catview_fwd_f32(const int32_t* ids0, const float* table0, int64_t rows0, int32_t K0, const float* Wb0,
                             float* out0, const int32_t* ids1, const float* table1, int64_t rows1, int32_t K1,
                             const float* Wb1, float* out1, int64_t N, int32_t F, int32_t* oob_flag, ebn_stream_t stream);
/* Its backward from dout_i [N, F] and the forward's out_i (ReLU gate out > 0): dWb_i [K_i + 1, F] (kernel rows, then the bias
 * row) and the dense table gradient dtable_i [rows_i, K_i] (rows no id names get 0; ids outside the table contribute
 * nothing), all overwritten.  Two launches: per slice of 32 articles the partial [dW ; db] and de = dY.W^T, then the slices
 * summed in ascending order and, for each table row, the de of the articles naming it in ascending article order -- no
 * atomics, the same bits on every run.  partials: ebn_naml_catview_partials_len(N, K0, K1, F) floats of scratch.            */
int64_t ebn_naml_catview_partials_len(int64_t N, int32_t K0, int32_t K1, int32_t F);
int ebn_naml_catview_bwd_f32(const int32_t* ids0, const float* table0, int64_t rows0, int32_t K0, const float* Wb0,
                             const float* out0, const float* dout0, float* dWb0, float* dtable0, const int32_t* ids1,
                             const float* table1, int64_t rows1, int32_t K1, const float* Wb1, const float* out1,
                             const float* dout1, float* dWb1, float* dtable1, float* partials, int64_t partials_len,
                             int64_t N, int32_t F, ebn_stream_t stream);
/* AttLayer2 over the n_views (<= 8) strided rows of each article, one wave per article (the view-level attention of naml.py):
 *   U <- tanh(U + b) in place ([n_views*N, A], U = Vw.Wa from one ebn_gemm_f32 over the n_views*N rows);
 *   a_v = exp(U_v . q) (no max-subtraction);  w_v = a_v / (sum_v a + 1e-7) -> w [n_views, N];  news [N, F] = sum_v w_v Vw[v, n]. */
int ebn_naml_viewatt_fwd_f32(float* U, const float* b, const float* q, const float* Vw, float* w, float* news, int64_t N,
                             int32_t n_views, int32_t F, int32_t A, ebn_stream_t stream);
/* Its backward's direct part from dnews [N, F]: dVw[v, n] = w_v dnews_n (overwritten; must not alias Vw) and
 * de [n_views, N] = w_v (dw_v - sum_u w_u dw_u), dw_v = dnews_n . Vw[v, n].  The rest is row-order agnostic and reuses
 * ebn_attpool_bwd_dpre_f32 over the n_views*N rows (dpre, dq, db) and ebn_gemm_f32 (dWa = Vw^T.dpre, dVw += dpre.Wa^T).      */
int ebn_naml_viewatt_bwd_f32(const float* Vw, const float* w, const float* dnews, float* dVw, float* de, int64_t N,
                             int32_t n_views, int32_t F, ebn_stream_t stream);

/* ---- Fastformer (reference models/fastformer/fastformer.py; PyTorch, BERT-style blocks around additive attention) ---------------
 * The Linear layers run on ebn_gemm_f32 (torch's [out, in] weights through transB = 1); these entry points are everything between
 * them.  Exact fp32, fixed summation orders, no float atomics.  Dropout: the counter stream of ebn_step_advance's keys, but the
 * key of a call site is passed BY VALUE (`drop_key`; drop_p = 0 disables it): this model's 1 + 2 * layers sites do not live in
 * ebn_step_state.  The mask of element (r, c) is that of flat index r * D + c.
 *
 * bias + dropout + residual + LayerNorm over R rows of D <= 1024 columns:
 *   mode 0 (SequenceFastformerEncoder.forward): Y = drop(LN(X + bias + res)), res [D] one row broadcast to every row;
 *   mode 1 (BertSelfOutput / BertOutput):       Y = LN(drop(X + bias) + res), res [R, D];
 *   LN(z) = gamma * xhat + beta, xhat = (z - mean) / sqrt(var + eps), biased variance.  xhat [R, D] and rstd [R] are what the
 *   backward needs (both may be NULL: inference).  Y may alias X.                                                           */
int ebn_ff_ln_fwd_f32(const float* X, const float* bias, const float* res, const float* gamma, const float* beta, float eps,
                      int32_t mode, uint32_t drop_key, float drop_p, float* Y, float* xhat, float* rstd, int64_t R, int32_t D,
                      ebn_stream_t stream);
/* Its backward from dY: dX [R, D] = dL/dX; mode 1 also dres [R, D] = dL/dres.  The column sums are left as *n_parts (a HOST
 * out-parameter) partials [n_parts][3][D] = dgamma | dbeta | dbias for ebn_ff_colsum_finish_f32 (stride = width = 3 * D); in mode 0
 * the gradient of the broadcast row equals dbias.  partials: ebn_ff_ln_partials_len(R, D) floats.                        */
int64_t ebn_ff_ln_partials_len(int64_t R, int32_t D);
int ebn_ff_ln_bwd_f32(const float* dY, const float* xhat, const float* rstd, const float* gamma, int32_t mode, uint32_t drop_key,
                      float drop_p, float* dX, float* dres, float* partials, int32_t* n_parts, int64_t R, int32_t D,
                      ebn_stream_t stream);
/* out[i] = sum_p partials[p * stride + i], i < width: four interleaved chains of ascending p, combined (0 + 1) + (2 + 3).  */
int ebn_ff_colsum_finish_f32(const float* partials, int64_t n_parts, int64_t stride, int64_t width, float* out,
                             ebn_stream_t stream);
/* BertIntermediate after its GEMM: Y = gelu(X + bias), erf form, [R, C]; backward dX = dY * gelu'(X + bias) recomputed from the
 * saved pre-activation X, dbias [C] its column sum (two launches; partials: ebn_colsum_partials_len(R, C) floats).        */
int ebn_ff_gelu_fwd_f32(const float* X, const float* bias, float* Y, int64_t R, int32_t C, ebn_stream_t stream);
int ebn_ff_gelu_bwd_f32(const float* X, const float* bias, const float* dY, float* dX, float* dbias, float* partials, int64_t R,
                        int32_t C, ebn_stream_t stream);
/* AttentionPooling (fastformer.py) after att_fc1's GEMM, n_seq sequences of L <= 4096 rows, one workgroup per sequence:
 *   U [n_seq*L, D] <- tanh(U + b1) in place;  a_l = exp(U_l . w2 + b2[0]) * mask[n, l] (no max-subtraction);
 *   w_l = a_l / (sum_l a + 1e-8) -> w [n_seq, L];  out [n_seq, D] = sum_l w_l X_l;  sinv [n_seq] = 1 / (sum a + 1e-8).
 * A sequence whose mask is all zero gets w == 0 and out == 0 exactly.  Not ebn_attpool_fwd_f32 (1e-7, no b2, no mask).     */
int ebn_ff_pool_fwd_f32(float* U, const float* b1, const float* w2, const float* b2, const float* X, const float* mask, float* out,
                        float* w, float* sinv, int64_t n_seq, int32_t L, int32_t D, ebn_stream_t stream);
/* Its backward's direct part from dout [n_seq, D]: dX [n_seq*L, D] = w_l dout (overwritten), de [n_seq*L] = w_l (dw_l - s) with
 * dw_l = dout . X_l, s = sum_l w_l dw_l, and db2n [n_seq] = the sequence's share of d(b2) = sum_l de_l in its closed form
 * s * 1e-8 * sinv (the literal sum is pure cancellation).  The rest is ebn_attpool_bwd_dpre_f32 over the rows (q = w2) and GEMMs. */
int ebn_ff_pool_bwd_f32(const float* X, const float* w, const float* sinv, const float* dout, float* dX, float* de, float* db2n,
                        int64_t n_seq, int32_t L, int32_t D, ebn_stream_t stream);
/* Head: score[n] = sigmoid(user[n] . W[0:D] + cand[n] . W[D:2D] + b[0]); backward from dscore [N]: duser, dcand [N, D],
 * dW [2D] (n ascending), db [1].                                                                                              */
int ebn_ff_head_fwd_f32(const float* user, const float* cand, const float* W, const float* b, float* score, int64_t N, int32_t D,
                        ebn_stream_t stream);
int ebn_ff_head_bwd_f32(const float* user, const float* cand, const float* W, const float* score, const float* dscore, float* duser,
                        float* dcand, float* dW, float* db, int64_t N, int32_t D, ebn_stream_t stream);
/* FastSelfAttention between its Linear layers, one workgroup per sequence of T tokens.  Q, K [n_seq*T, D] arrive as x.Wq^T, x.Wk^T
 * and leave with their biases added (mixed_query_layer / mixed_key_layer, kept for the backward).  hs = D / heads:
 *   a_h = softmax_t((Q_t . Wqa_h + bqa_h) / sqrt(hs) + (1 - mask_t) * -10000)  -- Wqa [heads, D]: every head reads the WHOLE row;
 *   pq = per-head sum_t a_h[t] Q_t (on the head's columns);  KP = K * pq;  b_h likewise from KP with Wka, bka;  pk = sum_t b_h[t] KP_t;
 *   AO [n_seq*T, D] = pk * Q (the input of `transform`);  SV0 (may be NULL) = Q + btr, the buffer transform's GEMM accumulates
 *   into (beta = 1) for "+ mixed_query_layer".  Saved: qw, kw [n_seq, heads, T], pq, pk [n_seq, D].
 * Shape rules: D % heads == 0 (else EBN_ERR_BAD_ARG); D % 4 == 0, D <= 1024, heads * D <= 4096, T <= 4096 and
 * 4 * (T * (D + 4) + 6 * D + heads * T + T) bytes of LDS <= 64 KiB forward, 4 * (T * (D + 4) + 4 * D + 4 * heads * T) backward
 * (EBN_ERR_UNSUPPORTED); Q, K, AO, SV0 and the weights 16-byte aligned.                                                       */
int ebn_ff_attn_fwd_f32(float* Q, float* K, const float* bq, const float* bk, const float* btr, const float* Wqa, const float* bqa,
                        const float* Wka, const float* bka, const float* mask, float* AO, float* SV0, float* qw, float* kw,
                        float* pq, float* pk, int64_t n_seq, int32_t T, int32_t D, int32_t heads, ebn_stream_t stream);
/* Its backward from dAO and (may be NULL) dSV, the gradient reaching Q through SV0: dQ, dK [n_seq*T, D] and *n_parts (HOST
 * out-parameter, <= 256) per-workgroup partials [n_parts][2 * heads * D + 3 * D] = dWqa | dWka | colsum(dQ) | colsum(dK) |
 * colsum(dSV) (= d(query.bias), d(key.bias), d(transform.bias)) for ebn_ff_colsum_finish_f32.  Workgroup g walks the sequences
 * g, g + n_parts, ... in ascending order.  The logit biases bqa / bka have identically zero gradients (a softmax does not see a
 * shift) and are not computed.  partials: ebn_ff_attn_partials_len(n_seq, D, heads) floats.                                  */
int64_t ebn_ff_attn_partials_len(int64_t n_seq, int32_t D, int32_t heads);
/* The shape rules above as a pure host query: EBN_OK, or the code ebn_ff_attn_fwd_f32 (and, with_backward != 0, ebn_ff_attn_bwd_f32,
 * whose LDS bound is the tighter one) would return.  The module asks it before the first launch of a training step.              */
int ebn_ff_attn_supported(int32_t T, int32_t D, int32_t heads, int32_t with_backward);
int ebn_ff_attn_bwd_f32(const float* Q, const float* K, const float* Wqa, const float* Wka, const float* qw, const float* kw,
                        const float* pq, const float* pk, const float* dAO, const float* dSV, float* dQ, float* dK, float* partials,
                        int32_t* n_parts, int64_t n_seq, int32_t T, int32_t D, int32_t heads, ebn_stream_t stream);
/* The streamed pair (csrc/ebn_fastformer_streamed.hip): the same operation for shapes the pair above refuses -- hidden 768 / 12
 * heads, hidden 1024 / 16 heads, hundreds of tokens.  Nothing T x D is kept in LDS: a token row lives in the registers of the wave
 * that works on it and Q, K are re-read from global memory.  ebn_ff_attn_streamed_fwd_f32 takes the arguments of
 * ebn_ff_attn_fwd_f32 and leaves the same tensors, the biased Q and K included.
 * Shape rules: D % heads == 0 (else EBN_ERR_BAD_ARG); D % 4 == 0, D <= 1024, T <= 4096, any heads <= D (heads * D is not bounded),
 * and 4 * (heads * T + T + 2 * D) bytes of LDS <= 64 KiB forward, 4 * (2 * heads * T + 4 * D) backward (EBN_ERR_UNSUPPORTED):
 * T <= 1142 forward and T <= 554 backward at D = 768, 12 heads.  Q, K, AO, SV0, kp and the weights 16-byte aligned.
 * ebn_ff_attn_streamed_supported is the pure host query of these rules, as ebn_ff_attn_supported is of the resident pair's.    */
int ebn_ff_attn_streamed_supported(int32_t T, int32_t D, int32_t heads, int32_t with_backward);
int ebn_ff_attn_streamed_fwd_f32(float* Q, float* K, const float* bq, const float* bk, const float* btr, const float* Wqa,
                                 const float* bqa, const float* Wka, const float* bka, const float* mask, float* AO, float* SV0,
                                 float* qw, float* kw, float* pq, float* pk, int64_t n_seq, int32_t T, int32_t D, int32_t heads,
                                 ebn_stream_t stream);
/* Its backward: dQ, dK as above; *n_parts (HOST out-parameter, <= 256) per-workgroup partials [n_parts][3 * D] = colsum(dQ) |
 * colsum(dK) | colsum(dSV) for ebn_ff_colsum_finish_f32 (workgroup g walks the sequences g, g + n_parts, ...).  The logit-weight
 * gradients are NOT formed here: the kernel writes d1, d2 [n_seq*T, heads], the gradients of the query / key logits behind their
 * softmax backwards, and kp [n_seq*T, D] = K * pq, and the caller computes
 *   dWqa [heads, D] = inv * d1^T . Q,   dWka = inv * d2^T . kp,   inv = 1 / sqrt(D / heads)
 * with ebn_gemm_f32_ws(transA = 1, transB = 0, heads, D, n_seq*T, inv, ...).  Sizes in floats: partials
 * ebn_ff_attn_streamed_partials_len(n_seq, D), d1 and d2 ebn_ff_attn_streamed_dlogits_len(n_seq, T, heads) each, kp
 * ebn_ff_attn_streamed_kp_len(n_seq, T, D); every element of all four is written.                                                */
int64_t ebn_ff_attn_streamed_partials_len(int64_t n_seq, int32_t D);
int64_t ebn_ff_attn_streamed_dlogits_len(int64_t n_seq, int32_t T, int32_t heads);
int64_t ebn_ff_attn_streamed_kp_len(int64_t n_seq, int32_t T, int32_t D);
int ebn_ff_attn_streamed_bwd_f32(const float* Q, const float* K, const float* Wqa, const float* Wka, const float* qw,
                                 const float* kw, const float* pq, const float* pk, const float* dAO, const float* dSV, float* dQ,
                                 float* dK, float* d1, float* d2, float* kp, float* partials, int32_t* n_parts, int64_t n_seq,
                                 int32_t T, int32_t D, int32_t heads, ebn_stream_t stream);

/* ---- Fastformer_wu (reference models/fastformer/fastformer_wu.py): the positional encoder and the class head ---------------------
 * StandardFastformerEncoder.forward's embedding block (fastformer_wu.py:216-224: position_ids = arange(n_tokens), embeddings =
 * dropout(LayerNorm(input_embs + position_embeddings))) over n_seq sequences of T tokens, D <= 1024 columns; row r = n * T + t:
 *   Y [n_seq*T, D] = drop(LN(X + bias + pos[r % T])),  pos [>= T, D]: only rows < T are read.
 * bias [D] may be NULL (the stand-alone encoder has none; Fastformer_wu folds embedding_transform.bias in, fastformer_wu.py:267).
 * LN, eps, drop_key / drop_p, xhat [n_seq*T, D] and rstd [n_seq*T] (both may be NULL) as ebn_ff_ln_fwd_f32 mode 0; Y may alias X.
 * The backward is ebn_ff_ln_bwd_f32 mode 0 (dX and the dgamma | dbeta | dbias partials); the position rows' gradient is the sum of
 * dX over the sequences, dpos[t] = sum_n dX[n, t] = ebn_ff_colsum_finish_f32(dX, n_seq, T * D, T * D, dpos).                       */
int ebn_ff_ln_pos_fwd_f32(const float* X, const float* bias, const float* pos, const float* gamma, const float* beta, float eps,
                          uint32_t drop_key, float drop_p, float* Y, float* xhat, float* rstd, int64_t n_seq, int32_t T, int32_t D,
                          ebn_stream_t stream);
/* Fastformer_wu.forward's head (fastformer_wu.py:269-270: score = output_layer(text_vec); loss = CrossEntropyLoss()(score, targets)),
 * 1 <= C <= 64 classes, D <= 1024 (else EBN_ERR_UNSUPPORTED), one wave per row, two launches:
 *   logits [N, C] = X [N, D] . W[C, D]^T + b;  prob [N, C] = softmax(logits) with the row maximum subtracted (kept for the backward);
 *   rowloss [N] = log(sum_c exp(l_c - m)) + m - l_y;  loss[0] = (sum_n rowloss[n]) / N: 256 interleaved chains of ascending n, then a
 *   fixed halving tree.  targets [N] int64.  A target outside [0, C) sets flag[0] = 1 (the caller zeroes it), its row contributes
 *   nothing to the sum (N still divides it) and, in the backward, no loss gradient.  No ignore_index, no class weights.            */
int ebn_ff_cls_fwd_f32(const float* X, const float* W, const float* b, const int64_t* targets, float* logits, float* prob,
                       float* rowloss, float* loss, int32_t* flag, int64_t N, int32_t D, int32_t C, ebn_stream_t stream);
/* Its backward from dloss (a DEVICE scalar; NULL = 0) and dscore [N, C] (NULL = 0):
 *   dlogits = dloss[0] / N * (prob - onehot(target)) + dscore;  dX [N, D] = dlogits . W (c ascending).
 * dW [C, D] and db [C] are left as *n_parts (a HOST out-parameter, <= 128) per-workgroup partials [n_parts][C * D + C] = dW | db for
 * ebn_ff_colsum_finish_f32 (stride = width = C * D + C); workgroup g adds its rows in ascending order.  partials:
 * ebn_ff_cls_partials_len(N, D, C) floats.                                                                                        */
int64_t ebn_ff_cls_partials_len(int64_t N, int32_t D, int32_t C);
int ebn_ff_cls_bwd_f32(const float* X, const float* W, const float* prob, const int64_t* targets, const float* dloss,
                       const float* dscore, float* dX, float* partials, int32_t* n_parts, int64_t N, int32_t D, int32_t C,
                       ebn_stream_t stream);

/* Step prologue: copy up to three device buffers (history ids, candidate ids, labels of a batch handed over as device
 * tensors -- the inputs of nrms.py:170-176) into the step's static buffers with ONE launch; n_i in bytes, multiples
 * of 4; a NULL source or n_i = 0 skips that pair.                                                                   */
int ebn_copy3(const void* s0, void* d0, int64_t n0, const void* s1, void* d1, int64_t n1, const void* s2, void* d2,
              int64_t n2, ebn_stream_t stream);
/* The same copy with ebn_step_advance folded in (the staging launch of a training step on a device-resident batch). */
int ebn_copy3_advance(const void* s0, void* d0, int64_t n0, const void* s1, void* d1, int64_t n1, const void* s2,
                      void* d2, int64_t n2, ebn_step_state* st, double beta1, double beta2, ebn_stream_t stream);

/* y = a*x + y over n elements (L2 kernel-regulariser gradient, gradient accumulation). */
int ebn_axpy_f32(float a, const float* x, float* y, int64_t n, ebn_stream_t stream);
/* kernel_regularizer=l2(lambda) of one Dense kernel in a single pass (nrms_docvec.py:119-121, nrms.py:146-148):
 * gW += 2*lambda*W and loss[0] += lambda*sum(W^2); `partials` = scratch of at least 256 floats
 * (ebn_colsum_partials_len never returns less).                                                            */
int ebn_l2_reg_f32(const float* W, float* gW, int64_t n, float lambda, float* partials, float* loss,
                   ebn_stream_t stream);
/* The same for up to four Dense kernels with two launches in total (NULL W_i / n_i = 0 skips a slot): gW_i += 2*lambda*W_i,
 * loss[0] += lambda * sum_i sum(W_i^2); `partials` = scratch of at least 1024 floats.                                 */
int ebn_l2_reg4_f32(const float* W0, float* g0, int64_t n0, const float* W1, float* g1, int64_t n1, const float* W2,
                    float* g2, int64_t n2, const float* W3, float* g3, int64_t n3, float lambda, float* partials,
                    float* loss, ebn_stream_t stream);
/* out[0] (+)= scale * sum(x[0..n)) -- deterministic single-block reduction.            */
int ebn_sum_f32(const float* x, int64_t n, float scale, float* out, int32_t accumulate,
                ebn_stream_t stream);
/* out[0] (+)= scale * sum(x^2).                                                         */
int ebn_sumsq_f32(const float* x, int64_t n, float scale, float* out, int32_t accumulate,
                  ebn_stream_t stream);

/* ---- beyond-accuracy list metrics (paths relative to src/ebrec/evaluation/) ------------------------------------------
 * Lists are int32 ROW numbers of a device table + int64 CSR offsets [n_lists + 1] into an id array of n_ids entries.  A row
 * number < 0 or >= n_rows is a MISSING id (get_keys_in_dict, utils.py:155-169): the kernels skip it and never form an address
 * from it; a list whose offsets leave [0, n_ids] or run backwards is treated as empty.  Any list length is legal, 0 included.
 * All results are fp32; "undefined" is NaN exactly where the reference returns NaN.  D is any positive width (16-byte loads
 * when D % 4 == 0 and the table is 16-byte aligned, 4-byte loads otherwise).                                                 */
/* dst[r] = src[r] / sqrt(sum src[r]^2); a zero row is divided by 1 and stays zero -- sklearn's normalize inside the
 * cosine_distances the reference passes as pairwise_distance_function (beyond_accuracy.py:3,60).  dst may be src.          */
int ebn_ba_unit_rows_f32(const float* src, float* dst, int64_t n_rows, int64_t D, ebn_stream_t stream);
/* IntralistDiversity.__call__ (beyond_accuracy.py:81-96) + intralist_diversity (metrics/_beyond_accuracy.py:45-52) over UNIT
 * rows: out[l] = sum over positions i != j of clip(1 - u_i . u_j, 0, 2) / (n (n - 1)), n = valid ids of the list (a repeated id
 * counts once per position); NaN when n < 2.  form 0: lists of at most 10 positions run one wave per list with the rows in
 * registers, longer ones one workgroup per list over LDS tiles; form 1: every list takes the tiled form (the test hook that
 * compares the two).                                                                                                         */
int ebn_ba_intralist_f32(const float* unit, int64_t n_rows, int64_t D, const int32_t* ids, int64_t n_ids, const int64_t* offsets,
                         int64_t n_lists, int32_t form, float* out, ebn_stream_t stream);
/* Serendipity.__call__ (beyond_accuracy.py:405-427) + serendipity (metrics/_beyond_accuracy.py:91-94): out[l] = mean over all
 * n x m pairs (recommendation i of list l, history item j of list l) of clip(1 - u_i . u_j, 0, 2) -- no diagonal is zeroed, the
 * two sides are different arrays; NaN when either side has no valid id.  form 0: a pair whose shorter side has at most 10
 * positions runs one wave per pair with that side's rows in registers (D % 4 == 0, D <= 1024, 16-byte aligned table; otherwise,
 * and for every other pair, one workgroup per pair over LDS tiles); form 1: every pair takes the tiled form.                   */
int ebn_ba_cross_f32(const float* unit, int64_t n_rows, int64_t D, const int32_t* ids_r, int64_t n_ids_r, const int64_t* off_r,
                     const int32_t* ids_h, int64_t n_ids_h, const int64_t* off_h, int64_t n_lists, int32_t form, float* out,
                     ebn_stream_t stream);
/* The candidates' distance matrix of IntralistDiversity._candidate_diversity (beyond_accuracy.py:130-154), built once:
 * out [m, m], out[i, j] = clip(1 - u_ids[i] . u_ids[j], 0, 2), exactly 0 where i == j, NaN where either id is missing.
 * m <= 16 * 65535 (EBN_ERR_UNSUPPORTED beyond).                                                                              */
int ebn_ba_pairdist_f32(const float* unit, int64_t n_rows, int64_t D, const int32_t* ids, int64_t m, float* out, ebn_stream_t stream);
/* Sentiment.__call__ (beyond_accuracy.py:295-302; transform 0: mean of values[id]) and Novelty.__call__ + novelty
 * (beyond_accuracy.py:479-486, metrics/_beyond_accuracy.py:165; transform 1: mean of -log2(values[id])); NaN on a list without a
 * valid id.                                                                                                                  */
int ebn_ba_list_mean_f32(const float* values, int64_t n_rows, const int32_t* ids, int64_t n_ids, const int64_t* offsets,
                         int64_t n_lists, int32_t transform, float* out, ebn_stream_t stream);
/* The per-combination diversities of _candidate_diversity (beyond_accuracy.py:139-154): subsets [n_subsets, k] int32 indices into
 * the m x m matrix of ebn_ba_pairdist_f32, out[s] = sum over a != b of dist[s_a, s_b] / (k' (k' - 1)), k' = indices inside
 * [0, m) (others are skipped); NaN when k' < 2.  Minimum and maximum are taken by the caller.                                 */
int ebn_ba_subset_sums_f32(const float* dist, int64_t m, const int32_t* subsets, int64_t k, int64_t n_subsets, float* out,
                           ebn_stream_t stream);

/* ---- per-impression ranking metrics over ragged lists (paths relative to src/ebrec/) ----------------------------------------
 * Lists are a flat score array (score_kind EBN_RM_F32 or EBN_RM_F64; scores are COMPARED in that type, unrounded), a flat uint8
 * label array (0 / non-zero) and int64 CSR offsets [n_lists + 1] into both (n_items entries each, n_items <= 2^31 - 257).  A list
 * whose offsets leave [0, n_items] or run backwards is treated as empty; any length is legal, 0 and 1 included.  A candidate's rank
 * comes from counting, rank_i = 1 + #{j : s_j > s_i} + #{j < i : s_j == s_i}; everything after the comparisons is fp64.
 * Per-list flag byte: bit 0 "tie-ambiguous" = two EQUAL scores of the list carry DIFFERENT labels (the only case in which
 * mrr / ndcg depend on the order inside a tie group, which on the host is the order of an unstable argsort); bit 1 = the list
 * holds a non-finite score.  The caller recomputes flagged lists on the host.
 * form 0: a list of at most 16 candidates runs in a 16-lane group (four lists per wave), one of at most 64 in one wave, a longer one
 * with a whole workgroup over an LDS copy of the list (at most 1024 candidates) or over 1024-candidate tiles re-read from global
 * memory; form 1: every list takes the last, general form (the test hook that compares the forms).                              */
#define EBN_RM_MAX_SLOTS 16
#define EBN_RM_F32 0
#define EBN_RM_F64 1
#define EBN_RM_AUC 0      /* roc_auc_score (metrics/_sklearn.py): (#{pos > neg} + #{pos == neg} / 2) / (n_pos n_neg)                 */
#define EBN_RM_MRR 1      /* mrr_score (metrics/_ranking.py:152-155): sum y_i / rank_i / n_pos                                        */
#define EBN_RM_NDCG 2     /* ndcg_score (:121-123), param = k: gains 2^y - 1, discounts log2(rank + 1), ranks <= min(k, n)            */
#define EBN_RM_LOGLOSS 3  /* LogLossScore (metrics_protocols.py:99): scores clipped to [10e-12, 1 - 10e-12]                           */
#define EBN_RM_RMSE 4     /* sqrt(mean (y - s)^2)                                                                                     */
#define EBN_RM_ACCURACY 5 /* param = threshold: mean((s >= threshold) == y)                                                           */
#define EBN_RM_F1 6       /* param = threshold: 2 tp / (2 tp + fp + fn) of s >= threshold, 0.0 on a zero denominator                  */
/* Bytes of the workspace ebn_rank_metrics needs for n_lists lists (one partial per slot and workgroup; 0 for n_lists outside
 * [0, 2^31 - 1]).                                                                                                              */
int64_t ebn_rank_metrics_workspace_bytes(int64_t n_lists);
/* MetricEvaluator.evaluate (evaluation/metrics_protocols.py:141-217) for up to EBN_RM_MAX_SLOTS metrics in one pass.  slot_kind /
 * slot_param are DEVICE arrays of n_slots entries (an unknown kind gives NaN).  Outputs, all on the device:
 *   sums [n_slots] fp64: the sum of the slot's per-list values over the lists that are left to the device -- a list with flag bit 1
 *     adds to no sum, one with bit 0 to no mrr / ndcg sum, a one-class list to no auc / logloss sum (there the host raises); any
 *     other NaN value (mrr / ndcg of a list without a positive, rmse / accuracy of an empty list) is added, as np.mean would;
 *   flags [n_lists]; counters [3] = lists with one class only (empty ones included), with bit 0, with bit 1;
 *   per_list (may be NULL) [n_slots, n_lists] fp64: every list's value, NaN where the host functions give NaN or raise.
 * Sums are taken in a fixed order (lane tree, one running sum per lane group, 16 per workgroup, a closing launch over the
 * workgroups): no floating-point atomics, two runs give the same bits.  workspace: 16-byte aligned device memory.               */
int ebn_rank_metrics(const void* scores, int32_t score_kind, const uint8_t* labels, int64_t n_items, const int64_t* offsets,
                     int64_t n_lists, const int32_t* slot_kind, const double* slot_param, int32_t n_slots, int32_t form, double* sums,
                     uint8_t* flags, int64_t* counters, double* per_list, void* workspace, int64_t workspace_bytes,
                     ebn_stream_t stream);
/* rank_predictions_by_score (utils/_python.py:41-59) of every list: ranks [n_items] int32, 1 for the highest score.  A list with
 * ANY two equal scores (flag bit 0) or a non-finite score (bit 1) is left to the host: its ranks are written as 0.               */
int ebn_list_ranks(const void* scores, int32_t score_kind, int64_t n_items, const int64_t* offsets, int64_t n_lists, int32_t form,
                   int32_t* ranks, uint8_t* flags, ebn_stream_t stream);

/* ---- scoring from a once-encoded article catalogue (naml.py user encoder + scorer: AttLayer2 layers.py:55-81, Dot + sigmoid) ---
 * The NAML user encoder is an UNMASKED AttLayer2 over the history's news vectors: the logit of a history item,
 * a = exp(tanh(x.W + b).q) (layers.py:69-75, no max-subtraction), depends on the article alone -- one scalar per catalogue row.
 * a[r] = exp(sum_k tanh(U[r, k] + b[k]) q[k]) for the pre-activations U [n_rows, A] = news_all . W (one ebn_gemm_f32); U is not
 * modified.  The arithmetic of ebn_attpool_fwd_f32's logit.                                                                    */
int ebn_att_logit_rows_f32(const float* U, const float* b, const float* q, float* a, int64_t n_rows, int32_t A,
                           ebn_stream_t stream);
/* The user stage and the scorer of one eval batch in one launch (layers.py:75-80 + naml.py scorer: sigmoid(news(pred_one) . user)):
 * one workgroup per impression i of B,
 *   w_l = a_all[his_idx[i, l]] / (sum_l a_all[his_idx[i, l]] + 1e-7),  user_i = sum_l w_l news_all[his_idx[i, l]]  (kept on chip),
 *   scores[p] = act(user_i . news_all[cand_idx[p]]) for p in [offsets[i], offsets[i + 1]),  act = sigmoid (mode 1) or id (0).
 * news_all [n_rows, F], a_all [n_rows], his_idx [B, H] int32, cand_idx [n_cand] int32 with int64 CSR offsets [B + 1] (an
 * impression's candidates are contiguous), user [B, F] optional (NULL: not written).  Any candidate count per impression, 0
 * included; H <= 2048, F % 4 == 0, F <= 8192, news_all / user 16-byte aligned.  A row number outside [0, n_rows) sets *oob_flag
 * (may be NULL) and is never used as an address: a history item of that kind is skipped, a candidate of that kind scores act(0);
 * an offsets pair that runs backwards or leaves [0, n_cand] makes that impression's list empty.  Fixed summation order.          */
int ebn_indexed_attpool_score_f32(const float* news_all, const float* a_all, int64_t n_rows, const int32_t* his_idx,
                                  const int32_t* cand_idx, const int64_t* offsets, int64_t n_cand, float* scores, float* user,
                                  int32_t* oob_flag, int64_t B, int32_t H, int32_t F, int32_t mode, ebn_stream_t stream);

/* ---- NPA from a once-encoded catalogue (npa.py:120-136 news encoder, layers.py:312-339 PersonalizedAttentivePooling) ----------
 * The personalised news vector depends on the user only through the logits q . Ua_l: per catalogue row the conv output
 * Vd [L, F] and the attention keys Ua = tanh(Vd.Wa + ba) [L, A] are kept, and a (query, article) pair is pooled from them.
 * U <- tanh(U + ba[k]) in place for U [n_rows, A] (the pre-activations Vd.Wa of ebn_gemm_f32): pap_fwd's expression (layers.py:333),
 * so the stored bits are those ebn_pap_fwd_f32 leaves in U.                                                                     */
int ebn_bias_tanh_rows_f32(float* U, const float* ba, int64_t n_rows, int32_t A, ebn_stream_t stream);
/* One workgroup per sequence n of n_seq, row = row_idx[n] (DEVICE int32), q = Q[q_idx[n]] (Q [n_q, A], q_idx as ebn_pap_fwd_f32:
 * an index outside [0, n_q) reads row 0):
 *   s_l = q . Ua_all[row, l];  w = softmax_l(s) (max-subtracted, layers.py:334-335);  pooled = sum_l w_l Vd_all[row, l]
 *   out[n] = pooled (out [n_seq, F], may be NULL);  scores[n] = act(pooled . users[q_idx[n]]) (users [n_q, F]; scores may be NULL,
 *   it needs users; act = sigmoid (mode 1) or id (0); npa.py:188-199 scorer) -- with scores alone the vector never reaches memory.
 * Same operations in the same order as ebn_pap_fwd_f32: given the same Ua and Vd bits, out is bit-equal to that kernel's on
 * the gathered rows.  Nothing is modified in place; w is not kept; no dropout (inference).  Ua_all [n_rows, L, A], Vd_all
 * [n_rows, L, F], offsets are 64-bit.  A row outside [0, n_rows) sets *oob_flag (may be NULL) and is never used as an address:
 * its out row is zeros, its score act(0).  L <= 256, F <= 4096, F % 4 == 0, Ua_all / Vd_all / out 16-byte aligned.               */
int ebn_pap_indexed_f32(const float* Ua_all, const float* Vd_all, int64_t n_rows, const int32_t* row_idx, const float* Q,
                        const int32_t* q_idx, int64_t n_q, float* out, const float* users, float* scores, int32_t mode,
                        int32_t* oob_flag, int64_t n_seq, int32_t L, int32_t F, int32_t A, ebn_stream_t stream);

/* ---- top-N recommendation from an encoded catalogue (examples/beyond_accuracy/make_beyond_accuracy.ipynb, cell "Your Model":
 * every beyond-accuracy user's top-N out of one shared candidate list; scorers of nrms.py / nrms_docvec.py / lstur.py / naml.py:
 * act(user . news)) ---------------------------------------------------------------------------------------------------------------
 * score[u, c] = users[u, :] . news_all[cand_rows[c], :] in exact fp32 (MFMA fma chain), never written out: each user keeps its best
 * k in the order (score descending, candidate position ascending).  users [U, F], news_all [n_rows, F]; cand_rows [M] rows of
 * news_all, or NULL = rows 0 .. n_rows - 1 (then M == n_rows); duplicate rows are distinct candidates.  exclude [U, X] (or NULL):
 * candidate c is skipped for user u when cand_rows[c] equals any of exclude[u, :]; entries outside [0, n_rows) match nothing (-1 is
 * the padding).  A cand_rows entry outside [0, n_rows) is never turned into an address: it is skipped and sets flags[0]; a NaN score
 * never enters a list and sets flags[1]; +-inf rank like numbers.  flags [2] is only ever SET (the caller zeroes it and may let it
 * accumulate over calls).  out_pos [U, k]: position in cand_rows (the row number when cand_rows is NULL), -1 in the empty trailing
 * slots of a user with fewer than k admissible candidates; out_score [U, k]: the raw dot product (mode 0) or its sigmoid (mode 1,
 * applied to the kept values only; ranking is always on the raw value), -inf in empty slots.
 * Limits: 1 <= k <= 64, 0 <= X <= 256, F % 4 == 0, 4 <= F <= 8192 (EBN_ERR_UNSUPPORTED), users / news_all 16-byte aligned
 * (EBN_ERR_ALIGN).  U == 0: nothing to do; M == 0: the outputs are filled as empty.
 * The grid is 128-user tiles x n_splits ranges of 128-candidate tiles (n_splits 0 = ebn_topk_auto_splits; clamped to the number of
 * candidate tiles and to 64).  More than one range: each writes a partial list to the workspace (16-byte aligned, at least
 * ebn_topk_workspace_bytes(U, k, n_splits) bytes, else EBN_ERR_BAD_ARG) and a second launch merges them in the same total order.
 * No atomics; the result is bit-identical for every n_splits and from run to run.                                                 */
/* Bytes of workspace for n_splits >= 1 candidate ranges (a nominal 16 for one range, which needs none); 0 for sizes outside the
 * limits.  Pure host query.                                                                                                       */
int64_t ebn_topk_workspace_bytes(int64_t n_users, int32_t k, int32_t n_splits);
/* The number of candidate ranges n_splits = 0 stands for: 1 once the user tiles alone give a few hundred workgroups.  Pure host
 * query, >= 1.                                                                                                                    */
int ebn_topk_auto_splits(int64_t n_users, int64_t n_cand);
int ebn_topk_score_f32(const float* users, const float* news_all, int64_t n_rows, const int32_t* cand_rows, int64_t M,
                       const int32_t* exclude, int32_t X, int32_t k, int32_t mode, int32_t n_splits, int32_t* out_pos,
                       float* out_score, int32_t* flags, void* workspace, int64_t workspace_bytes, int64_t U, int32_t F,
                       ebn_stream_t stream);
/* The same with a window of candidate positions per user (freshness: candidates sorted by publish time, an impression's admissible
 * articles are one range).  window [U, 2] int32 on the DEVICE, (lo_u, hi_u) = window[u]: user u may receive position c only when
 * max(lo_u, 0) <= c < min(hi_u, M); lo_u >= hi_u after clamping gives an empty list (-1 / -inf).  Inside a window everything is
 * ebn_topk_score_f32's: the total order, exclude, cand_rows == NULL, duplicate rows, mode, the limits, the alignment and argument
 * codes (all checked on the host before anything is launched: a failing call writes nothing), U == 0, M == 0, the workspace
 * (ebn_topk_workspace_bytes) and n_splits (0 = ebn_topk_auto_splits).  window == NULL is EBN_ERR_BAD_ARG: the unwindowed call is
 * ebn_topk_score_f32.  A score's bits are those ebn_topk_score_f32 gives the same (user, candidate row) pair (the same fma chain);
 * a list depends neither on n_splits, nor on the run, nor on which other users share the launch.
 * A 128-user workgroup visits only the 128-candidate tiles that meet the union of its users' windows (its tiles, not the
 * catalogue's, are what n_splits divides), so users sorted by lo cost in proportion to the window, not to M.  Hence the flags:
 * flags[1] is set only by a NaN score of a pair inside that user's window -- a NaN outside it is never looked at.  flags[0] is set
 * when a cand_rows entry outside [0, n_rows) lies in the window of at least one user, and is not set when no such entry lies in
 * [min lo, max hi) over all users; for an entry in between -- inside that span but in no user's window -- EITHER value may come
 * back: it is seen iff it lies between the lowest lo and the highest hi of one 128-user workgroup.                               */
int ebn_topk_score_window_f32(const float* users, const float* news_all, int64_t n_rows, const int32_t* cand_rows, int64_t M,
                              const int32_t* window, const int32_t* exclude, int32_t X, int32_t k, int32_t mode, int32_t n_splits,
                              int32_t* out_pos, float* out_score, int32_t* flags, void* workspace, int64_t workspace_bytes,
                              int64_t U, int32_t F, ebn_stream_t stream);

/* ---- full-catalogue rank of one target candidate per user (the accuracy side of the same workflow,
 * examples/beyond_accuracy/make_beyond_accuracy.ipynb, cell "Your Model": where the clicked article stands among all candidates the
 * top-N is drawn from -- hit-rate@k, MRR and nDCG@k over the candidate list; scorers as above: act(user . news)) ---------------------
 * Everything not said here is ebn_topk_score_window_f32's contract: the operands and cand_rows == NULL, duplicate rows being distinct
 * candidates, exclude [U, X] matching by catalogue row, the clamping of window [U, 2], the limits (F % 4 == 0, 4 <= F <= 8192,
 * X <= 256: EBN_ERR_UNSUPPORTED; users / news_all 16-byte aligned: EBN_ERR_ALIGN), the argument codes (all checked on the host before
 * anything is launched: a failing call writes nothing), U == 0 (nothing to do), n_splits (0 = ebn_topk_auto_splits; the ranges
 * divide the tiles a workgroup's windows meet) and flags[0] / flags[1], including the either-value clause for a row outside the
 * table that lies inside a workgroup's span but in nobody's window.  window == NULL: no windows, every position is inside.
 * s(u, c) = users[u, :] . news_all[cand_rows[c], :] has the BITS ebn_topk_score_f32 gives the same (user row, catalogue row) pair:
 * the same v_mfma_f32_32x32x2_f32 fma chain in the same k order.  Position c is admissible for user u when it lies in u's clamped
 * window, cand_rows[c] lies in [0, n_rows) and is not in exclude[u, :], and s(u, c) is not NaN.  target_pos [U] int32 on the DEVICE
 * (required, EBN_ERR_BAD_ARG): the position of the user's target in the candidate list; < 0: no target; >= M: no target and
 * flags[0] is set.  With t = s(u, target_pos[u]):
 *   out_count[u] = the number of admissible positions
 *   out_rank[u]  = 1 + #{admissible c != target : s(u, c) > t or (s(u, c) == t and c < target_pos[u])} -- the target's index + 1 in
 *                  the total order of ebn_topk_score_f32 (score descending, then position ascending; +-inf rank like numbers) --
 *                  or 0 when there is no target or the target position is itself not admissible (a NaN t inside the window also
 *                  sets flags[1], a target row outside the table inside the window flags[0])
 *   out_score[u] = t (mode 0) or sigmoid(t) (mode 1) when out_rank[u] > 0, else -inf
 * M == 0: rank 0, count 0, score -inf.  The three outputs depend neither on n_splits, nor on the run, nor on which other users
 * share the launch.  More than one range of candidates: each writes its two partial counts per user to the workspace (16-byte
 * aligned, at least ebn_target_rank_workspace_bytes(U, n_splits) bytes, else EBN_ERR_BAD_ARG) and a second launch adds them --
 * integer sums, the order is free; no atomics on global memory.                                                                   */
/* Bytes of workspace for n_splits >= 1 candidate ranges (a nominal 16 for one range, which needs none); 0 for sizes outside the
 * limits, never negative.  Pure host query.                                                                                       */
int64_t ebn_target_rank_workspace_bytes(int64_t n_users, int32_t n_splits);
int ebn_target_rank_f32(const float* users, const float* news_all, int64_t n_rows, const int32_t* cand_rows, int64_t M,
                        const int32_t* target_pos, const int32_t* window, const int32_t* exclude, int32_t X, int32_t mode,
                        int32_t n_splits, int32_t* out_rank, int32_t* out_count, float* out_score, int32_t* flags, void* workspace,
                        int64_t workspace_bytes, int64_t U, int32_t F, ebn_stream_t stream);

/* ---- top-N recommendation for NPA from the once-encoded catalogue (the same workflow for npa.py: its news vector depends on the
 * user -- layers.py:312-339 PersonalizedAttentivePooling -- so there is no [n_rows, F] catalogue for ebn_topk_score_f32) ------------
 * Per user u and candidate row = cand_rows[c], from what NPAEngine.encode_catalogue keeps (Ua_all [n_rows, L, A] tanh'd attention
 * keys, Vd_all [n_rows, L, F] conv outputs) and the user stage gives (Q [U, A] news-level queries, users [U, F] user vectors):
 *   s_l = Q[u, :] . Ua_all[row, l, :];  w = softmax_l(s) (max-subtracted, layers.py:334-335; no masking: every token counts)
 *   score[u, c] = sum_l w_l (users[u, :] . Vd_all[row, l, :])     ( = pooled(u, row) . users[u], npa.py:188-199 scorer)
 * Both dot products in exact fp32 (MFMA fma chains in a fixed k order); neither the [U, M, L] logits and dots nor the [U, M] scores
 * are written out: each user keeps its best k in the order (score descending, candidate position ascending).  A pair's score bits
 * depend only on that user's two rows and that catalogue row's data -- not on the candidate's position, U, M, n_splits or the run.
 * NOT bit-equal to ebn_pap_indexed_f32's score, which pools first and dots second (both are within rounding of the same value).
 * cand_rows [M] rows of the catalogue, or NULL = rows 0 .. n_rows - 1 (then M == n_rows); duplicate rows are distinct candidates
 * (with bit-equal scores).  exclude [U, X] (or NULL): candidate c is skipped for user u when cand_rows[c] equals any of
 * exclude[u, :]; entries outside [0, n_rows) match nothing (-1 is the padding).  A cand_rows entry outside [0, n_rows) is never
 * turned into an address: it is skipped and sets flags[0]; a NaN score never enters a list and sets flags[1]; +-inf rank like
 * numbers.  flags [2] is only ever SET (the caller zeroes it and may let it accumulate over calls).  out_pos [U, k]: position in
 * cand_rows (the row number when cand_rows is NULL), -1 in the empty trailing slots of a user with fewer than k admissible
 * candidates; out_score [U, k]: the raw score (mode 0) or its sigmoid (mode 1, applied to the kept values only; ranking is always
 * on the raw value), -inf in empty slots.  All offsets are 64-bit.
 * Limits: 1 <= k <= 64, 0 <= X <= 256, 1 <= L <= 64, A % 4 == 0, 4 <= A <= 1024, F % 4 == 0, 4 <= F <= 4096 (EBN_ERR_UNSUPPORTED),
 * users / Q / Ua_all / Vd_all 16-byte aligned (EBN_ERR_ALIGN), NULL pointers or negative sizes EBN_ERR_BAD_ARG; all checked on the
 * host before anything is launched, a failing call writes nothing.  U == 0: nothing to do; M == 0: the outputs are filled as empty.
 * L is padded inside the kernel to the 32-row tile only (32, or 64 for L > 32): padded tokens get weight 0 and are never read.
 * The grid is 128-user tiles x n_splits ranges of candidate steps (4 candidates a step for L <= 32, 2 above; n_splits 0 =
 * ebn_npa_topk_auto_splits; clamped to the number of steps and to 64).  More than one range: each writes a partial list to the
 * workspace -- the layout of ebn_topk_score_f32: 16-byte aligned, at least ebn_topk_workspace_bytes(U, k, n_splits) bytes, else
 * EBN_ERR_BAD_ARG -- and a second launch merges them in the same total order.  No atomics; the result is bit-identical for every
 * n_splits and from run to run.                                                                                                    */
/* The number of candidate ranges n_splits = 0 stands for.  Pure host query, >= 1.                                                  */
int ebn_npa_topk_auto_splits(int64_t n_users, int64_t n_cand, int32_t L);
int ebn_npa_topk_score_f32(const float* users, const float* Q, const float* Ua_all, const float* Vd_all, int64_t n_rows,
                           const int32_t* cand_rows, int64_t M, const int32_t* exclude, int32_t X, int32_t k, int32_t mode,
                           int32_t n_splits, int32_t* out_pos, float* out_score, int32_t* flags, void* workspace,
                           int64_t workspace_bytes, int64_t U, int32_t L, int32_t F, int32_t A, ebn_stream_t stream);
/* The same with a window of candidate positions per user: what ebn_topk_score_window_f32 is to ebn_topk_score_f32.  window [U, 2]
 * int32 on the DEVICE, (lo_u, hi_u) = window[u]: user u may receive position c only when max(lo_u, 0) <= c < min(hi_u, M);
 * lo_u >= hi_u after clamping gives an empty list (-1 / -inf).  window == NULL is EBN_ERR_BAD_ARG: the unwindowed call is
 * ebn_npa_topk_score_f32.
 * ebn_npa_topk_score_f32's inside a window: the operands and the pair score, the total order, exclude, cand_rows == NULL, duplicate
 * rows, mode, padded tokens, the limits, the alignment and argument codes (all checked on the host before anything is launched: a
 * failing call writes nothing), U == 0 (nothing to do), M == 0 (the outputs are filled as empty), the workspace
 * (ebn_topk_workspace_bytes) and n_splits (0 = ebn_npa_topk_auto_splits(U, M, L); clamped to the catalogue's steps and to 64).  A
 * score's bits are those ebn_npa_topk_score_f32 gives the same (user rows, catalogue row) pair: the same fma chains, in-lane
 * reduction order, cross-half add and division; a list depends neither on n_splits, nor on the run, nor on which other users share
 * the launch.
 * ebn_topk_score_window_f32's: a 128-user workgroup visits only the candidate steps (4 candidates for L <= 32, 2 above) that meet the
 * union of its users' windows -- its steps, not the catalogue's, are what n_splits divides -- so users sorted by lo cost in
 * proportion to the window, not to M.  Hence the flags: flags[1] is set only by a NaN score of a pair inside that user's window -- a
 * NaN outside it is never looked at.  flags[0] is set when a cand_rows entry outside [0, n_rows) lies in the window of at least one
 * user, and is not set when no such entry lies in [min lo, max hi) over all users; for an entry in between -- inside that span but
 * in no user's window -- EITHER value may come back: it is seen iff it lies between the lowest lo and the highest hi of one
 * 128-user workgroup.                                                                                                              */
int ebn_npa_topk_score_window_f32(const float* users, const float* Q, const float* Ua_all, const float* Vd_all, int64_t n_rows,
                                  const int32_t* cand_rows, int64_t M, const int32_t* window, const int32_t* exclude, int32_t X,
                                  int32_t k, int32_t mode, int32_t n_splits, int32_t* out_pos, float* out_score, int32_t* flags,
                                  void* workspace, int64_t workspace_bytes, int64_t U, int32_t L, int32_t F, int32_t A,
                                  ebn_stream_t stream);

/* ---- full-catalogue rank of one target candidate per user for NPA (the accuracy side of the same workflow for npa.py: where the
 * clicked article stands among all candidates NPA's top-N is drawn from) --------------------------------------------------------------
 * The counting form of ebn_npa_topk_score_f32, as ebn_target_rank_f32 is the counting form of ebn_topk_score_f32.  Everything not
 * said here is one of those two contracts.
 * ebn_npa_topk_score_f32's: the operands (users [U, F], Q [U, A], Ua_all [n_rows, L, A], Vd_all [n_rows, L, F]) and the pair score,
 * cand_rows == NULL, duplicate rows being distinct candidates, exclude [U, X] matching by catalogue row (-1 and rows past the table
 * match nothing), padded tokens (weight 0, never read), the limits (1 <= L <= 64, A % 4 == 0, 4 <= A <= 1024, F % 4 == 0,
 * 4 <= F <= 4096, X <= 256: EBN_ERR_UNSUPPORTED; users / Q / Ua_all / Vd_all 16-byte aligned: EBN_ERR_ALIGN) and the steps n_splits
 * divides (0 = ebn_npa_topk_auto_splits(U, M, L); with windows: the steps a workgroup's windows meet).
 * ebn_target_rank_f32's: target_pos [U] (required; < 0: no target; >= M: no target and flags[0]), window [U, 2] and its clamping
 * (NULL: every position is inside), out_rank / out_count / out_score and mode, M == 0 (rank 0, count 0, score -inf), flags[0] and
 * flags[1] including the either-value clause for a row outside the table that lies inside a workgroup's span but in nobody's
 * window, the argument codes (all checked on the host before anything is launched: a failing call writes nothing), U == 0 (nothing
 * to do), no atomics on global memory.
 * s(u, c) and the target's score t have the BITS ebn_npa_topk_score_f32 gives the same (user rows, catalogue row) pair: the same fma
 * chains, in-lane reduction order, cross-half add and division.  Position c is admissible for user u when it lies in u's clamped
 * window, cand_rows[c] lies in [0, n_rows) and is not in exclude[u, :], and s(u, c) is not NaN.  out_count[u] is the number of
 * admissible positions; out_rank[u] is 1 + the number of admissible positions ahead of the target in ebn_npa_topk_score_f32's order
 * (score descending, then position ascending), or 0 when the target is absent or inadmissible.  So out_rank[u] = r <= k holds
 * exactly when ebn_npa_topk_score_f32 with the same exclude and k has the target at index r - 1, and out_score[u] is then that
 * slot's score, bit for bit.  The three outputs depend neither on n_splits, nor on the run, nor on which other users share the launch.
 * Three launches: a target pass (t [U] into the workspace), the walk (two partial counts per user and range into the workspace), a
 * small one that adds them and writes the outputs.  So ONE range needs the workspace too: 16-byte aligned, at least
 * ebn_npa_target_rank_workspace_bytes(U, n_splits) bytes (n_splits 0: that of ebn_npa_topk_auto_splits), else EBN_ERR_BAD_ARG.      */
/* Bytes of workspace for n_splits >= 1 candidate ranges; 0 for sizes outside the limits, never negative.  Pure host query.         */
int64_t ebn_npa_target_rank_workspace_bytes(int64_t n_users, int32_t n_splits);
int ebn_npa_target_rank_f32(const float* users, const float* Q, const float* Ua_all, const float* Vd_all, int64_t n_rows,
                            const int32_t* cand_rows, int64_t M, const int32_t* target_pos, const int32_t* window,
                            const int32_t* exclude, int32_t X, int32_t mode, int32_t n_splits,
                            int32_t* out_rank, int32_t* out_count, float* out_score, int32_t* flags,
                            void* workspace, int64_t workspace_bytes, int64_t U, int32_t L, int32_t F, int32_t A,
                            ebn_stream_t stream);

/* ---- MMR re-ranking of a relevance pool (greedy Maximal Marginal Relevance over the distance of IntralistDiversity,
 * beyond_accuracy.py:81-96: the list a top-N of ebn_topk_score_f32 with k = P becomes when relevance is traded against diversity) ---
 * Per user u of U: P pool entries, relevance pool_rel[u, i] and row pool_rows[u, i] of the UNIT table unit [n_rows, D] (what
 * ebn_ba_unit_rows_f32 leaves).  An entry is ABSENT when its row is outside [0, n_rows) (-1 is the padding of a short list and sets
 * nothing, any other such row sets flags[0]) or its relevance is not finite (-inf is the padding, NaN and +inf set flags[1]); an
 * absent entry's row is never turned into an address.  d(i, j) = fminf(fmaxf(1 - u_i . u_j, 0), 2), the dot product in exact fp32 (one
 * MFMA fma chain over D in a fixed order); a NaN dot product between two present entries gives d = 0 and sets flags[1].
 * Round 0 picks the present entry with the largest relevance (obj = rel); round t >= 1 picks, among the present entries not yet
 * picked, the largest obj_i = lam * rel_i + (1 - lam) * min over picked j of d(i, j).  Larger obj first, equal obj to the smaller pool
 * index.  The rounds end after k picks or when nothing is left; lam = 1 gives the relevance order of the pool, which need not
 * arrive sorted.  out_sel [U, k]: the pool INDEX of each pick, -1 in the empty trailing slots; out_obj [U, k] (may be NULL): its
 * objective, -inf in empty slots.  flags [2] is only ever SET (the caller zeroes it and may let it accumulate over calls).
 * Limits: 1 <= P <= 64, 1 <= k <= 64 (k > P is legal: the lists come back short), D % 4 == 0, 4 <= D <= 8192 (EBN_ERR_UNSUPPORTED);
 * lam outside [0, 1] or NaN: EBN_ERR_BAD_ARG; unit 16-byte aligned (EBN_ERR_ALIGN).  U == 0: nothing to do.  A failing call writes
 * nothing.  One workgroup per user (two users when P <= 32), no atomics: a user's output bits depend neither on U nor on the users
 * that share its launch, and two runs give the same bits.                                                                       */
int ebn_mmr_rerank_f32(const float* unit, int64_t n_rows, int32_t D, const int32_t* pool_rows, const float* pool_rel, int32_t P,
                       int32_t k, float lam, int32_t* out_sel, float* out_obj, int32_t* flags, int64_t U, ebn_stream_t stream);

/* ---- DPP re-ranking of a relevance pool (greedy MAP inference of a determinantal point process, Chen, Zhang, Zhou, NeurIPS 2018:
 * where MMR looks at a pick's NEAREST earlier pick, DPP scores the list jointly through log det of its similarity matrix) ----------
 * The arguments, the pool, ABSENT entries, the flags, the limits and the error codes are those of ebn_mmr_rerank_f32, and so is
 * d(i, j) = fminf(fmaxf(1 - u_i . u_j, 0), 2), the dot product in exact fp32 (one MFMA fma chain over D in a fixed order); a NaN dot
 * product between two present entries -- an entry with itself included, the diagonal is used here -- gives d = 0 and sets flags[1].
 * An absent entry's row is never turned into an address.
 * Similarity S(i, j) = 1 - d(i, j) / 2: (1 + cos) / 2 for unit rows, positive semi-definite, in [0, 1], monotone in the cosine,
 * the diagonal AS COMPUTED (1 up to rounding for a unit row, 1/2 for a zero row).  State per entry: d2_i, the conditional variance
 * of i given the picks, initially S(i, i), and a Cholesky row c_i[0..t).  EPS = 1e-4f.
 * Round t = 0, 1, ... picks, among the present entries not yet picked, the largest
 *   obj_i = lam * rel_i + (1 - lam) * logf(fmaxf(d2_i, EPS))
 * (lam * rel_i is the marginal gain of lam * sum rel + (1 - lam) * log det S_Y).  Larger obj first, equal obj to the smaller pool
 * index.  After picking j: if d2_j <= EPS the pick is degenerate (already spanned by the picks) and nothing is updated but
 * c_i[t] = 0; otherwise, for every present unpicked i,
 *   e_i = (S(j, i) - sum_{s<t} c_j[s] c_i[s]) / sqrtf(d2_j),   c_i[t] = e_i,   d2_i -= e_i * e_i,
 * the sum over s ascending in ONE fma chain.  The rounds end after k picks or when nothing is left.  A pool whose rank is below k
 * still gives full-length lists: spanned entries are clamped at EPS, not dropped, and then order by relevance.  lam = 1 gives the
 * relevance order of the pool (which need not arrive sorted) with out_obj = rel.  out_sel [U, k]: the pool INDEX of each pick, -1
 * in the empty trailing slots; out_obj [U, k] (may be NULL): its objective, -inf in empty slots.  flags [2] is only ever SET.
 * Limits: 1 <= P <= 64, 1 <= k <= 64 (k > P is legal: the lists come back short), D % 4 == 0, 4 <= D <= 8192 (EBN_ERR_UNSUPPORTED);
 * lam outside [0, 1] or NaN: EBN_ERR_BAD_ARG; unit 16-byte aligned (EBN_ERR_ALIGN).  U == 0: nothing to do.  A failing call writes
 * nothing.  One workgroup per user (two users when P <= 32), one wave of it running the rounds with the Cholesky rows in LDS, no
 * atomics: a user's output bits depend neither on U nor on the users that share its launch, and two runs give the same bits.   */
int ebn_dpp_rerank_f32(const float* unit, int64_t n_rows, int32_t D, const int32_t* pool_rows, const float* pool_rel, int32_t P,
                       int32_t k, float lam, int32_t* out_sel, float* out_obj, int32_t* flags, int64_t U, ebn_stream_t stream);

/* ---- calibrated re-ranking of a relevance pool (Steck, RecSys 2018: the greedy list whose label distribution stays close, in KL
 * divergence, to a target distribution -- what Distribution, beyond_accuracy.py:158-209, reports over category / sentiment_label /
 * topics in examples/beyond_accuracy/make_beyond_accuracy.ipynb) -----------------------------------------------------------------
 * LABEL TABLE W [n_rows, C] float32, one row per article: W[r, c] >= 0 is the share of label c in article r -- a one-hot row for a
 * single-valued attribute, 1 / len on each distinct label of a list-valued one, a zero row for no label (a legal pick that only
 * dilutes the list).
 *
 * ebn_label_target_f32: the history target.  hist_rows [U, H] rows of W, hist_w [H] one weight per history SLOT (decay weights) or
 * NULL = all ones.  target[u, c] = sum_h w_h W[hist_rows[u, h], c] / sum_h w_h over the slots whose row lies in [0, n_rows), each
 * label summed in slot order; a row of -1 is the padding and sets nothing, any other row outside the table sets flags[0]; such a
 * row is never turned into an address.  No valid slot, or a weight sum that is not > 0, gives a zero row.  target [U, C] is
 * written whole.  Limits: 1 <= C <= 128, 1 <= H <= 256 -- the X limit of ebn_topk_score_f32, so a caller can pass the history it
 * excludes by (EBN_ERR_UNSUPPORTED); U or n_rows outside [0, 2^31 - 1]: EBN_ERR_BAD_ARG.  U == 0: nothing to do.  A failing call
 * writes nothing.  flags [2] is only ever SET.  One wave per user, no atomics.                                                    */
int ebn_label_target_f32(const float* W, int64_t n_rows, int32_t C, const int32_t* hist_rows, int32_t H, const float* hist_w,
                         float* target, int32_t* flags, int64_t U, ebn_stream_t stream);
/* ebn_calibrated_rerank_f32.  Per user u of U: P pool entries, relevance pool_rel[u, i] and row pool_rows[u, i] of W, under the
 * contract of ebn_mmr_rerank_f32: an entry is ABSENT when its row is outside [0, n_rows) (-1 is the padding and sets nothing, any
 * other such row sets flags[0]) or its relevance is not finite (-inf is the padding, NaN and +inf set flags[1]); an absent entry's
 * row is never turned into an address.  The target p is target[u * target_stride + c]: target_stride = C gives a row per user,
 * 0 ONE row for all users.  A target entry that is negative or not finite counts as 0 and sets flags[1]; the target is used as
 * given, NOT renormalised; an all-zero target (an empty history) makes the calibration term 0 for every entry.
 * After the picks I, with S_c = sum over j in I of W[row_j, c], n = |I|, q~_c = (1 - alpha) S_c / n + alpha p_c and
 * KL(I) = sum over c with p_c > 0 of p_c logf(p_c / q~_c), EVERY round (round 0 too, unlike MMR) picks, among the present entries
 * not yet picked, the largest obj_i = lam * rel_i - (1 - lam) * KL(I + {i}).  Larger obj first, equal obj to the smaller pool index;
 * two entries with the same label row get the same KL bits.  The rounds end after k picks or when nothing is left; lam = 1 gives
 * the relevance order of the pool (which need not arrive sorted) with out_obj = rel.  out_sel [U, k]: the pool INDEX of each pick,
 * -1 in the empty trailing slots; out_obj [U, k] (may be NULL): its objective, -inf in empty slots.  flags [2] is only ever SET
 * (the caller zeroes it and may let it accumulate over calls).
 * Limits: 1 <= P <= 64, 1 <= k <= 64 (k > P is legal: the lists come back short), 1 <= C <= 128 (EBN_ERR_UNSUPPORTED).  Why 128:
 * a user's label rows stay in LDS for all k rounds, and with P = 64 they are 64 x 129 floats = 32 KiB of the CU's 160 KiB --
 * four users per CU; a wider label set would leave a CU to fewer waves than it has SIMDs.  lam outside [0, 1], alpha outside
 * (0, 1), NaN in either, target_stride not in {0, C}, U or n_rows outside [0, 2^31 - 1]: EBN_ERR_BAD_ARG.  U == 0: nothing to do.
 * A failing call writes nothing.  One wave per user, no atomics: a user's output bits depend neither on U nor on the users that
 * share its launch, and two runs give the same bits.                                                                            */
int ebn_calibrated_rerank_f32(const float* W, int64_t n_rows, int32_t C, const int32_t* pool_rows, const float* pool_rel, int32_t P,
                              const float* target, int64_t target_stride, int32_t k, float lam, float alpha, int32_t* out_sel,
                              float* out_obj, int32_t* flags, int64_t U, ebn_stream_t stream);

/* ---- Poisson bootstrap of per-item metric columns (no reference counterpart: the interval and the paired test behind every mean
 * MetricEvaluator and rank_metrics report; Hanley and MacGibbon 2006, Chamandy et al. 2012 for the Poisson form) --------------------
 * Resample b gives item i the weight w(i, b) ~ Poisson(1) of a counter-based stream, all arithmetic in uint32, lowbias32 the mixer
 * of the dropout stream:
 *   k   = lowbias32(seed ^ 0x9E3779B9)
 *   a_i = lowbias32(key_i ^ k)                key_i = keys[i], or first_key + i when keys is NULL
 *   r_b = lowbias32((b * 0x9E3779B9) ^ ~k)    b = first_resample + row
 *   u   = lowbias32(a_i + r_b)
 *   w   = #{ j : u >= C_j },  C_j = floor(2^32 P(W <= j)) for W ~ Poisson(1), j = 0 .. 11 (EBN_BS_THRESHOLDS; the 13th threshold
 *         would be 2^32 - 1, so w <= 12)
 * Items with the same key (a dense cluster code: a user) get the same weight in every resample -- the cluster bootstrap.  The weight
 * is a function of (seed, key, b) alone, so resamples [first_resample, first_resample + n_resamples) are those rows of any larger
 * call, and two disjoint item sets with global keys ADD to their union (sums within rounding, weight_sums exactly).
 *   sums [n_resamples, n_cols] fp64 = sum_i w(i, b) values[c * ld + i];  weight_sums [n_resamples] int64 = sum_i w(i, b), exact.
 * values [n_cols, ld] fp64 on the device, ld >= n_items; only entries i < n_items of a column are read.  A non-finite value makes
 * its column's sums NaN (0 * inf): the host layer rejects such input.
 * Grid: EBN_BS_RESAMPLES resamples per workgroup (two per lane) x up to 512 contiguous item ranges, each a whole number of
 * EBN_BS_TILE-item tiles staged through LDS (a_i and the column values, read back as broadcasts); the ranges depend on n_items ONLY.
 * A lane adds its items in ascending order, one fma(w, x, acc) per column; every range writes its partials to the workspace and a
 * closing launch adds the ranges in ascending order.  No floating-point atomics: two runs give the same bits; a column's bits do
 * not depend on which other columns share the call, nor a resample's on which other resamples do.
 * 1 <= n_cols <= EBN_BS_MAX_COLS (EBN_ERR_UNSUPPORTED above); n_items in [0, 2^31 - 257] (0: all sums are 0), n_resamples in
 * [0, 2^31 - 1] (0: nothing to do), first_resample >= 0 and first_resample + n_resamples <= 2^32, ld >= n_items, NULL values / sums /
 * weight_sums / workspace, a workspace that is not 16-byte aligned or smaller than the query: EBN_ERR_BAD_ARG.  All checked on the
 * host before anything is launched.                                                                                               */
#define EBN_BS_MAX_COLS 16
#define EBN_BS_TILE 256      /* items of one LDS tile; an item range is a whole number of tiles */
#define EBN_BS_RESAMPLES 512 /* resamples per workgroup */
#define EBN_BS_MAX_WEIGHT 12
#define EBN_BS_THRESHOLDS                                                                                                     \
  {1580030168u, 3160060337u, 3950075421u, 4213413783u, 4279248373u, 4292415291u, 4294609777u, 4294923276u, 4294962463u, 4294966817u, \
   4294967252u, 4294967292u}
/* Bytes of workspace: ranges(n_items) * n_resamples * (n_cols + 1) * 8; 0 for extents outside the limits above, INT64_MAX when the
 * product does not fit.  Pure host query.                                                                                          */
int64_t ebn_poisson_bootstrap_workspace_bytes(int64_t n_items, int64_t n_resamples, int32_t n_cols);
int ebn_poisson_bootstrap_f64(const double* values, int64_t ld, int64_t n_items, int32_t n_cols, const uint32_t* keys,
                              uint32_t first_key, uint32_t seed, int64_t first_resample, int64_t n_resamples, double* sums,
                              int64_t* weight_sums, void* workspace, int64_t workspace_bytes, ebn_stream_t stream);

/* ---- trailing-window event counts: time-aware popularity (the baseline beside examples/baseline/ebnerd_feat_baselines.py of the
 * reference, whose total_pageviews / total_inviews lookups count over the whole dataset and so see every impression's future) ------
 * EVENTS: the events (clicks, in-views) of article row r are event_times[row_offsets[r] .. row_offsets[r + 1]), ascending int64
 * times in any unit, equal times allowed; row_offsets [n_rows + 1] int64, a row holds fewer than 2^31 events.
 * ITEMS: item i of n_items (an in-view article of an impression) asks for row item_rows[i] and belongs to list l with
 * list_offsets[l] <= i < list_offsets[l + 1] (list_offsets [n_lists + 1] int64 ascending, list_offsets[0] = 0,
 * list_offsets[n_lists] >= n_items; empty lists anywhere); its query time is t = list_times[l].
 *   counts[w * ld + i] = #{ e in row item_rows[i] : t - max_age_w <= e < t - min_age }      w < n_windows, i < n_items, int32
 * The interval is HALF-OPEN AT THE TOP: with min_age = 0 an event at the impression's own time is not counted, so an index that
 * holds the evaluated impressions' own clicks does not leak them into their scores.  (Freshness, ebn_topk_score_window_f32's host
 * side, admits  t - max_age <= p <= t - min_age, closed: an article published at the impression's instant may be shown.)
 * t - max_age and t - min_age SATURATE at INT64_MIN, they do not wrap; max_age = EBN_WC_UNBOUNDED: the window has no lower end.
 * A window whose max_age <= min_age counts 0.  The windows may come in any order, with duplicates; unused max_age arguments
 * (w >= n_windows) are ignored.  They are passed BY VALUE, not as an array: every pointer of this ABI is a device pointer, the
 * ages must be checked (and sorted) on the host, and as kernel arguments they cost no upload and no load.
 * An item_rows[i] outside [0, n_rows) counts 0 in every window and reads nothing (-1 is the host layer's "unknown article").
 * Only counts[w * ld + i] for i < n_items, w < n_windows is written; nothing of the inputs past their extents is read.
 * One lane per item, 256-item workgroups: one upper_bound over list_offsets per workgroup, its next 256 list boundaries staged in
 * LDS; per item one lower_bound for t - min_age over the row, then one per window inside [previous result, that position), the
 * windows visited in descending max_age; the two searches over the whole row (the upper end, the longest bounded window) share one
 * loop.  All compares and indices int64.  No atomics, no workspace: two runs give the same bits.
 * n_windows outside [1, EBN_WC_MAX_WINDOWS], ld < n_items, n_items / n_lists / n_rows outside [0, 2^31 - 1], min_age < 0, a
 * max_age_w < 0 (w < n_windows), n_items > 0 with n_lists = 0, NULL item_rows / list_offsets / list_times / counts with n_items > 0,
 * NULL event_times / row_offsets with n_items > 0 and n_rows > 0: EBN_ERR_BAD_ARG.  n_items == 0: nothing to do.  All checked on the
 * host before the launch: a failing call writes nothing.                                                                          */
#define EBN_WC_MAX_WINDOWS 8
#define EBN_WC_UNBOUNDED INT64_MAX /* a max_age: the window has no lower end */
int ebn_window_counts_i32(const int64_t* event_times, const int64_t* row_offsets, int64_t n_rows, const int32_t* item_rows,
                          int64_t n_items, const int64_t* list_offsets, const int64_t* list_times, int64_t n_lists,
                          int32_t n_windows, int64_t max_age0, int64_t max_age1, int64_t max_age2, int64_t max_age3,
                          int64_t max_age4, int64_t max_age5, int64_t max_age6, int64_t max_age7, int64_t min_age,
                          int32_t* counts, int64_t ld, ebn_stream_t stream);

/* ---- content-similarity baselines: "recommend what looks like what this user read", from the document vectors alone (the reference
 * has no content baseline; the float64 brute force of tests/content_cases.py is the yardstick) ------------------------------------
 * TABLE: table [n_rows, D] fp32 at row stride ld >= D.  The kernels use the rows AS THEY ARE: the host passes unit rows (what
 * ebn_ba_unit_rows_f32 leaves), so the dots are cosines.  16-byte loads are used only where the pointer and ld allow them; the bits
 * of the results do not depend on ld or on the alignment.  D <= EBN_CS_MAX_D.
 * HISTORIES: history u of n_hists (one per USER, shared by all of the user's impressions) holds the entries
 * [hist_offsets[u], hist_offsets[u + 1]) of hist_rows [n_hist_items] int32, oldest first; hist_offsets [n_hists + 1] int64
 * ascending from 0 to at most n_hist_items.  Entry j weighs hist_weights[j] (finite and >= 0: the host's guarantee; used as it is),
 * or 1 when hist_weights is NULL.
 * LISTS: list l of n_lists (an impression) holds the items [cand_offsets[l], cand_offsets[l + 1]) of cand_rows [n_cand_items] int32
 * (cand_offsets [n_lists + 1] int64 ascending from 0 to n_cand_items; empty lists anywhere) and reads history
 * u(l) = list_hist ? list_hist[l] : l.
 * An entry or item whose row is outside [0, n_rows) is ABSENT (-1 is the host layer's "unknown article"): its row is never turned
 * into an address.  Columns >= D of a row and of a profile are never read, nothing of the other operands past its extent is read,
 * and only the outputs named below are written.
 *   ebn_cs_profiles_f32:         profiles[u * ldp + k] = p_k / ||p||,  p = sum over the present entries j of history u of
 *                                w_j * table[hist_rows[j], :];  a ZERO row when no entry is present or ||p|| is 0.  k < D, u < n_hists.
 *   ebn_cs_centroid_scores_f32:  scores[i] = profiles[u(l), :] . table[cand_rows[i], :] for item i of list l; 0 when the item is
 *                                absent or u(l) is outside [0, n_hists).  profiles [n_hists, D] at row stride ldp.
 *   ebn_cs_nearest_scores_f32:   scores[i] = max over the present entries j of history u(l) of w_j * (table[hist_rows[j], :] .
 *                                table[cand_rows[i], :]); 0 when the item is absent, u(l) is outside [0, n_hists) or the history
 *                                has no present entry.
 * profiles: one workgroup per history, its 4 waves take the entries round-robin, partial sums added through LDS in wave order, one
 * division per element.  centroid: one wave per list, the profile row in registers, one 64-lane sum per item, coalesced stores.
 * nearest: one workgroup per list, 16 candidate rows per LDS tile (16 * ceil(D / 256) * 1 KiB of dynamic LDS, 64 KiB at the most),
 * each wave streams its share of the history rows once per tile and keeps a running max per candidate.  Lane ownership of the
 * columns and every summation order are fixed.  No atomics, no workspace: two runs give the same bits.
 * D < 1, ld < D, ldp < D, any of n_rows / D / ld / ldp / n_hists / n_hist_items / n_lists / n_cand_items outside [0, 2^31 - 1],
 * n_cand_items > 0 with n_lists = 0, n_hist_items > 0 with n_hists = 0: EBN_ERR_BAD_ARG; then D > EBN_CS_MAX_D: EBN_ERR_UNSUPPORTED.
 * Nothing to do (EBN_OK, no launch): n_hists == 0 for the profiles, n_cand_items == 0 for the scores.  Otherwise a NULL among the
 * pointers the call needs is EBN_ERR_BAD_ARG; hist_weights and list_hist may be NULL, table may be NULL with n_rows == 0 (every
 * entry is absent), hist_rows with n_hist_items == 0, profiles (an input) and hist_offsets of the score calls with n_hists == 0.
 * All checked on the host before the launch: a failing call writes nothing.                                                         */
#define EBN_CS_MAX_D 1024
int ebn_cs_profiles_f32(const float* table, int64_t n_rows, int64_t D, int64_t ld, const int32_t* hist_rows, const float* hist_weights,
                        const int64_t* hist_offsets, int64_t n_hists, int64_t n_hist_items, float* profiles, int64_t ldp,
                        ebn_stream_t stream);
int ebn_cs_centroid_scores_f32(const float* table, int64_t n_rows, int64_t D, int64_t ld, const float* profiles, int64_t n_hists,
                               int64_t ldp, const int32_t* list_hist, const int32_t* cand_rows, const int64_t* cand_offsets,
                               int64_t n_lists, int64_t n_cand_items, float* scores, ebn_stream_t stream);
int ebn_cs_nearest_scores_f32(const float* table, int64_t n_rows, int64_t D, int64_t ld, const int32_t* hist_rows,
                              const float* hist_weights, const int64_t* hist_offsets, int64_t n_hists, int64_t n_hist_items,
                              const int32_t* list_hist, const int32_t* cand_rows, const int64_t* cand_offsets, int64_t n_lists,
                              int64_t n_cand_items, float* scores, ebn_stream_t stream);

/* ---- co-visitation baseline: "recommend what other readers of the same articles went on to read", item-to-item collaborative
 * filtering over click sequences (the reference has no such baseline; the plain-Python brute force of tests/covisit_cases.py is the
 * yardstick) -------------------------------------------------------------------------------------------------------------------
 * SEQUENCES: sequence s of n_seqs (one user's clicks, oldest first) holds the entries [seq_offsets[s], seq_offsets[s + 1]) of
 * seq_rows [n_entries] int32; seq_offsets [n_seqs + 1] int64 ascending from 0 to at most n_entries, empty sequences anywhere.  An
 * entry at or past seq_offsets[n_seqs] belongs to no sequence.
 *   ebn_cv_pair_keys_i64: with G = max_gap and K = symmetric ? 2 G : G, for entry i of sequence s and g = 1 .. G, j = i + g:
 *     keys[i * K + g - 1]     = seq_rows[j] * n_rows + seq_rows[i]   matrix row = the article clicked LATER, column = the one before it
 *     keys[i * K + G + g - 1] = seq_rows[i] * n_rows + seq_rows[j]   (symmetric only: the mirrored pair)
 *   when j < seq_offsets[s + 1], both rows lie in [0, n_rows) and the rows differ; EBN_CV_NO_PAIR otherwise, and for every slot of an
 *   entry without a sequence.  All n_entries * K slots are written and nothing else; seq_rows is read inside [0, n_entries) only.
 *   One lane per entry, 256-entry workgroups: the sequence of an entry is found as ebn_window_counts_i32 finds an item's list (one
 *   uniform search per workgroup, 256 staged boundaries in LDS, a fallback search behind a run of empty sequences); the slots of a
 *   workgroup leave as consecutive 8-byte stores.
 *   n_seqs / n_entries / n_rows outside [0, 2^31 - 1], max_gap < 1, with n_entries > 0 a NULL seq_rows / seq_offsets / keys or
 *   n_seqs == 0: EBN_ERR_BAD_ARG; then max_gap > EBN_CV_MAX_GAP: EBN_ERR_UNSUPPORTED; then n_entries == 0: nothing to do (EBN_OK, no
 *   launch).  symmetric: 0 or not 0.
 * MATRIX: CSR over n_rows rows: row r holds the columns cols[indptr[r] .. indptr[r + 1]) int32, STRICTLY ASCENDING, with the values
 * vals[...] fp32; indptr [n_rows + 1] int64, nnz entries.  S[c, h] is the stored value, 0 where nothing is stored.
 * HISTORIES and LISTS: as for ebn_cs_nearest_scores_f32 above (hist_rows / hist_weights / hist_offsets, list_hist, cand_rows /
 * cand_offsets); an entry or item whose row is outside [0, n_rows) is ABSENT; an entry that occurs twice counts twice.
 *   ebn_cv_scores_f32: for item i of list l, c = cand_rows[i], u = list_hist ? list_hist[l] : l:
 *     mode 0 (sum)  scores[i] = sum over the present entries j of history u of w_j * S[c, hist_rows[j]]
 *     mode 1 (max)  scores[i] = max over the same entries of w_j * S[c, hist_rows[j]]
 *   exactly 0.0f when the item is absent, u is outside [0, n_hists) or history u has no present entry.  All n_cand_items scores
 *   are written and nothing else.  Whatever cols holds, cols and vals are read only at positions inside
 *   [indptr[c], indptr[c + 1]) intersected with [0, nnz); the history extents are clamped to [0, n_hist_items] in the same way.
 *   256-item workgroups: one lane per item finds its list, history extent and matrix row extent; then one wave per item, 4 items
 *   per round: lane s takes the history entries s, s + 64, ... in order and binary-searches each present one in the row's columns;
 *   a butterfly over the 64 lanes (xor 32 .. 1) adds or maximises the partials.  Each product and each add rounds once, the order
 *   is fixed, no atomics, no workspace: two runs give the same bits.
 *   n_rows / nnz / n_hists / n_hist_items / n_lists / n_cand_items outside [0, 2^31 - 1], mode outside {0, 1}, n_cand_items > 0 with
 *   n_lists = 0, n_hist_items > 0 with n_hists = 0: EBN_ERR_BAD_ARG.  n_cand_items == 0: nothing to do (EBN_OK, no launch).  Otherwise
 *   a NULL among the pointers the call needs is EBN_ERR_BAD_ARG; hist_weights and list_hist may be NULL, indptr with n_rows == 0,
 *   cols and vals with nnz == 0, hist_offsets with n_hists == 0, hist_rows with n_hist_items == 0 (zeros in one launch).
 * All checked on the host before the launch: a failing call writes nothing.                                                         */
#define EBN_CV_MAX_GAP 64
#define EBN_CV_NO_PAIR INT64_MAX /* a key slot without a pair; sorts behind every key */
int ebn_cv_pair_keys_i64(const int32_t* seq_rows, const int64_t* seq_offsets, int64_t n_seqs, int64_t n_entries, int64_t n_rows,
                         int32_t max_gap, int32_t symmetric, int64_t* keys, ebn_stream_t stream);
int ebn_cv_scores_f32(const int64_t* indptr, const int32_t* cols, const float* vals, int64_t n_rows, int64_t nnz,
                      const int32_t* hist_rows, const float* hist_weights, const int64_t* hist_offsets, int64_t n_hists,
                      int64_t n_hist_items, const int32_t* list_hist, const int32_t* cand_rows, const int64_t* cand_offsets,
                      int64_t n_lists, int64_t n_cand_items, int32_t mode, float* scores, ebn_stream_t stream);

/* ---- co-visitation top-N lists and clicked-article ranks over the whole catalogue (csrc/ebn_covisit_topk.hip; the plain-Python
 * brute force of tests/covisit_topn_cases.py is the yardstick): what ebn_topk_score_window_f32 and ebn_target_rank_f32 are to the
 * dense scorers, for the sparse score of ebn_cv_scores_f32 ------------------------------------------------------------------------
 * Everything not said here is ebn_cv_scores_f32's (the CSR operand rules, the clamping of offsets to [0, nnz] and [0, n_hist_items],
 * ABSENT entries, repeated entries counting twice) and ebn_topk_score_window_f32's (window [U, 2] and its clamping to [0, M),
 * exclude [U, X] matching by catalogue row with -1 matching nothing, the total order, flags [2] only ever SET, all argument checks
 * on the host before anything is launched: a failing call writes nothing).
 * MATRIX: T, the TRANSPOSE of the fitted matrix, as CSR: t_indptr [n_rows + 1] int64, t_cols [nnz] int32 STRICTLY ASCENDING per row,
 * t_vals [nnz] fp32: row h of T holds every catalogue row c with a stored S[c, h], and the value.
 * HISTORIES: hist_rows / hist_weights (NULL: every weight 1) / hist_offsets over n_hists histories and n_hist_items entries; user u
 * of U uses history user_hist ? user_hist[u] : u, an index outside [0, n_hists) is a user without history.
 * POSITIONS: cand_pos [n_rows] int32 or NULL: the candidate position of catalogue row r; negative: the row is no candidate; NULL:
 * position = row (then M == n_rows, else EBN_ERR_BAD_ARG).  A value >= M is skipped and sets flags[0] when some user touches the
 * row.  Positions of distinct rows are distinct: the host's guarantee.
 * SCORE: row c is TOUCHED by user u when at least one present entry j of u's history has a stored S[c, hist_rows[j]] (a stored 0.0
 * counts).  With p_j = w_j * S[c, hist_rows[j]]: the score starts as the first touching entry's p_j; every later touching entry, in
 * history order, does acc = acc + p_j (mode 0) or acc = (p_j > acc or p_j is NaN) ? p_j : acc (mode 1).  Every product and every
 * add rounds once to fp32 (no fused multiply-add).  A score's bits depend on that user's history and that row's stored values
 * only: not on U, M, n_splits, the run or the other users of the launch.  No floating-point atomics.
 * ADMISSIBLE: row c for user u when it is touched, cand_pos[c] lies in [0, M) and in u's clamped window, c is not in exclude[u, :]
 * and the score is not NaN.  A NaN score of a touched row that is admissible otherwise sets flags[1]; +-inf rank like numbers.  An
 * untouched row never enters a list; a touched row with a negative score does.
 *   ebn_cv_topk_f32: out_pos [U, k] / out_score [U, k]: each user's best k admissible rows as (position, score), score descending,
 *     then position ascending; -1 / -inf in the empty trailing slots.  1 <= k <= 64.
 *   ebn_cv_target_rank_f32: target_pos [U] int32 on the DEVICE (required).  out_rank / out_count / out_score as ebn_target_rank_f32
 *     defines them, over this admissible set; the rank is 0 (score -inf) when there is no target (< 0; >= M also sets flags[0]),
 *     the position belongs to no row, or the target's row is untouched or not admissible (a NaN t of a row admissible otherwise
 *     sets flags[1]).  t has the bits ebn_cv_topk_f32 gives the same (user, row) pair.
 * One 256-thread workgroup per (user, split) walks ranges of ebn_cv_topk_range() catalogue rows, an fp32 tile and two bits per row
 * in LDS (34 KiB): per present history entry the segment of T's row inside the range (two binary searches), the threads stride
 * over it, one barrier between entries.  n_splits: 0 = ebn_cv_topk_auto_splits(U, n_rows); clamped to the number of ranges and to
 * 64.  More than one split: partial lists in the layout of ebn_topk_workspace_bytes (ebn_cv_topk_workspace_bytes gives the same
 * number) merged by a second launch; partial counts ([2, n_splits, U] int32, then [U] fp32) added by a second launch.  The
 * workspace is 16-byte aligned (else EBN_ERR_ALIGN) and at least that large (else, or NULL: EBN_ERR_BAD_ARG).  Results are
 * bit-identical for every n_splits and from run to run.
 * Any of n_rows / nnz / n_hists / n_hist_items / M / U outside [0, 2^31 - 1], X < 0, n_splits < 0, workspace_bytes < 0, mode
 * outside {0, 1}, n_hist_items > 0 with n_hists = 0, cand_pos NULL with M != n_rows: EBN_ERR_BAD_ARG; then k outside [1, 64] or
 * X > 256: EBN_ERR_UNSUPPORTED; then U == 0: nothing to do (EBN_OK, no launch); then a NULL output, flags or target_pos:
 * EBN_ERR_BAD_ARG; then n_rows == 0, nnz == 0 or M == 0: empty outputs in one launch (-1 / -inf; rank 0, count 0, -inf, and
 * flags[0] for a target position >= M); then a NULL t_indptr / t_cols / t_vals, hist_offsets with n_hists > 0 or hist_rows with
 * n_hist_items > 0: EBN_ERR_BAD_ARG.  hist_weights, user_hist, cand_pos, window and exclude (then X counts as 0) may be NULL.      */
/* The catalogue rows one LDS tile covers.  Pure host query.                                                                        */
int64_t ebn_cv_topk_range(void);
/* The number of row ranges n_splits = 0 stands for: 1 once the users alone give about 16 384 workgroups.  Pure host query, >= 1.  */
int ebn_cv_topk_auto_splits(int64_t n_users, int64_t n_rows);
/* Bytes of workspace for n_splits >= 1 (a nominal 16 where none is needed: one split, and for the rank call no cand_pos); 0 for
 * sizes outside the limits.  n_positions: M when the rank call gets a cand_pos, else 0 -- the call first writes the inverse of
 * cand_pos, [M] int32, into the workspace (one launch over the rows, once per call), so that a target's row is one load and not
 * a search.  Pure host queries.                                                                                                    */
int64_t ebn_cv_topk_workspace_bytes(int64_t n_users, int32_t k, int32_t n_splits);
int64_t ebn_cv_target_rank_workspace_bytes(int64_t n_users, int32_t n_splits, int64_t n_positions);
int ebn_cv_topk_f32(const int64_t* t_indptr, const int32_t* t_cols, const float* t_vals, int64_t n_rows, int64_t nnz,
                    const int32_t* hist_rows, const float* hist_weights, const int64_t* hist_offsets, int64_t n_hists,
                    int64_t n_hist_items, const int32_t* user_hist, const int32_t* cand_pos, int64_t M, const int32_t* window,
                    const int32_t* exclude, int32_t X, int32_t k, int32_t mode, int32_t n_splits, int32_t* out_pos, float* out_score,
                    int32_t* flags, void* workspace, int64_t workspace_bytes, int64_t U, ebn_stream_t stream);
int ebn_cv_target_rank_f32(const int64_t* t_indptr, const int32_t* t_cols, const float* t_vals, int64_t n_rows, int64_t nnz,
                           const int32_t* hist_rows, const float* hist_weights, const int64_t* hist_offsets, int64_t n_hists,
                           int64_t n_hist_items, const int32_t* user_hist, const int32_t* cand_pos, int64_t M, const int32_t* target_pos,
                           const int32_t* window, const int32_t* exclude, int32_t X, int32_t mode, int32_t n_splits, int32_t* out_rank,
                           int32_t* out_count, float* out_score, int32_t* flags, void* workspace, int64_t workspace_bytes, int64_t U,
                           ebn_stream_t stream);

/* ---- implicit-feedback ALS baseline (Hu, Koren, Volinsky 2008): latent-factor collaborative filtering, one half-sweep per call (the
 * reference has no such baseline; the float64 brute force of tests/als_cases.py is the yardstick) ----------------------------------
 * FIXED SIDE: fixed [n_fixed, F] fp32 at row stride ld >= F, used as it is; gram [F, F] at row stride ldg >= F is fixed^T fixed,
 * computed by the caller (ebn_gemm_f32_ws with transA = 1); only its lower triangle i >= j is read.
 * ROWS: CSR over n_solve rows: row r holds the entries [indptr[r], indptr[r + 1]) clamped to [0, nnz] of cols [nnz] int32 and
 * conf [nnz] fp32 (a_k >= 0: the host's guarantee; used as it is); indptr [n_solve + 1] int64.  An entry whose column is outside
 * [0, n_fixed) is ABSENT: it adds nothing and its column is never turned into an address.  Entries are used AS GIVEN: a repeated
 * column counts twice -- the host layer combines duplicates (summing their confidences) before the call.
 *   ebn_als_solve_f32: out[r * ldo + 0 .. F) = x_r, the solution of
 *       (gram + reg I + sum_k a_k y_k y_k^T) x_r = sum_k (1 + a_k) y_k,     y_k = fixed[cols[k], :], a_k = conf[k],
 *     over the present entries k of row r.  A row without a present entry gets exact +0.0 and no factorisation.  If a Cholesky
 *     pivot is not > 0 (NaN included) the WHOLE output row is NaN (the host layer raises on it).  All n_solve * F outputs are
 *     written and nothing else; columns >= F of fixed, gram and out are never read or written.
 *     LONG ROWS: with row_parts [n_solve + 1] int64 non-NULL, n_parts > 0 and row_parts[r] < row_parts[r + 1] (both clamped to
 *     [0, n_parts]) the kernel adds the parts [row_parts[r], row_parts[r + 1]) of `partials` in ascending order INSTEAD of walking
 *     the row's entries (such a row is always factorised).  row_parts is ignored when n_parts == 0.
 *   ebn_als_partials_f32: part p of n_parts covers the entries [part_begin[p], part_end[p]) clamped to [0, nnz] and writes
 *     partials[p * F (F + 1) + ...]: first the FULL symmetric matrix sum_k a_k y_k y_k^T as F * F floats, row-major (element (i, j)
 *     and (j, i) hold the same bits; the solve reads i >= j), then the F floats sum_k (1 + a_k) y_k.  All n_parts * F (F + 1)
 *     floats are written and nothing else.  The host cuts only rows longer than its split_len into parts of at most split_len
 *     entries: short rows never touch the workspace.
 * One workgroup per row / part, a G x G grid of threads: 256 threads (G = 16) for F > 32, one wave (G = 8) for F <= 32.  A lives in
 * registers (thread (ty, tx) owns the elements (ty + G a, tx + G b) of the blocks a >= b; F is rounded up to G, 2 G, 4 G or 8 G), the
 * entries are staged 16 at a time as a [16, F] tile in LDS and taken in their order, a right-looking Cholesky runs on the
 * registers with one column of L passing through LDS per step (two barriers a step), wave 0 does the two triangular solves.  Every product, add, fused multiply-add,
 * correctly rounded sqrtf and division happens in one fixed order: no atomics, two runs and every placement give the same bits,
 * and the bits do not depend on ld / ldg / ldo or on alignment (16-byte loads are used only where fixed and ld allow them).
 * LDS: 4 (FB (FB + 1) + 18 FB + 72) bytes for FB = F rounded up: 73.8 KiB at 128 (two workgroups per CU), 21.0 KiB at 64.
 * Any of n_fixed / F / ld / ldg / ldo / n_solve / nnz / n_parts outside [0, 2^31 - 1], F < 1, ld < F, ldg < F, ldo < F, reg not
 * finite or not > 0, n_parts > 0 with NULL partials, a NULL among the pointers the call needs: EBN_ERR_BAD_ARG; then
 * F > EBN_ALS_MAX_F: EBN_ERR_UNSUPPORTED.  Nothing to do (EBN_OK, no launch): n_solve == 0, or n_parts == 0 for the partials
 * call.  cols / conf may be NULL with nnz == 0 and fixed with n_fixed == 0 or nnz == 0 (every entry is absent: zeros in one
 * launch); row_parts may be NULL.  All checked on the host before the launch: a failing call launches and writes nothing.         */
#define EBN_ALS_MAX_F 128
int ebn_als_solve_f32(const float* fixed, int64_t n_fixed, int64_t F, int64_t ld, const float* gram, int64_t ldg,
                      const int64_t* indptr, const int32_t* cols, const float* conf, int64_t n_solve, int64_t nnz, float reg,
                      const int64_t* row_parts, const float* partials, int64_t n_parts, float* out, int64_t ldo,
                      ebn_stream_t stream);
int ebn_als_partials_f32(const float* fixed, int64_t n_fixed, int64_t F, int64_t ld, const int32_t* cols, const float* conf,
                         int64_t nnz, const int64_t* part_begin, const int64_t* part_end, int64_t n_parts, float* partials,
                         ebn_stream_t stream);

/* ---- score blending over ragged lists (the reference has no such step; the plain-Python brute force of tests/blend_cases.py is the
 * yardstick; host layer: ebrec/models/ensemble.py) -------------------------------------------------------------------------------
 * SOURCES: scores [M, n_items], source-major, 1 <= M <= EBN_BL_MAX_SOURCES, all fp32 (score_kind EBN_RM_F32) or all fp64
 * (EBN_RM_F64); compared and transformed in that type, unrounded.  All sources share one CSR offsets [n_lists + 1] int64; the
 * conventions are those of ebn_rank_metrics: n_items <= 2^31 - 257, any list length (0 and 1 included), a list whose offsets leave
 * [0, n_items] or run backwards is empty.  kinds [M] int32, params [M] fp64 and weights [M] fp64 are DEVICE arrays.
 * TRANSFORMS: the feature of item i in a list of n, all arithmetic after the load in fp64, rounded once to fp32:
 *   EBN_BL_RAW     s_i
 *   EBN_BL_ZSCORE  (s_i - mean) / sd, two-pass population sd; 0 for every item when sd == 0 or max == min
 *   EBN_BL_MINMAX  (s_i - min) / (max - min); 0 when max == min
 *   EBN_BL_RANK    (n - r_i) / (n - 1) with the mid-rank r_i = 1 + #{s_j > s_i} + 0.5 #{j != i: s_j == s_i}; 0 when n == 1
 *   EBN_BL_RRF     1 / (param + r_i)
 *   any other kind: NaN.  mean and the sum of squares are summed over the list's items in ascending order.
 * A list in which source m holds a non-finite score gets bit 1 (value 2) of flags[l] and NaN features in row m (RAW copies the
 * scores through); flags[l] is written for every list, 0 otherwise.
 *   ebn_blend_features_f32: features [M, n_items] fp32.  Every item of a well-formed list is written in every row, nothing else.
 *   ebn_blend_combine_f64: out[i] = sum_m weights[m] * (double) feature_m,i, m ascending, of the SAME fp32-rounded features, with
 *     no [M, n_items] intermediate; NaN for every item of a flagged list.
 *   ebn_blend_sums_f64: over features [M, n_items] fp32 and labels [n_items] uint8 (non-zero = positive), at weights w, for list l
 *       z = w . f (m ascending), p = softmax(z) with the maximum subtracted, t_i = y_i / n_pos, log p_i = (z_i - max) - log S,
 *       loss_l = -(sum_i y_i log p_i) / n_pos,  g_l = sum_i (p_i - t_i) f_i,  u = sum_i p_i f_i,
 *       H_l = sum_i p_i (f_i - u)(f_i - u)^T  (the centred form: positive semi-definite to rounding for features of any size);
 *     sums [1 + M + M (M + 1) / 2] = the sum over the used lists of loss, g, and the upper triangle of H row-major (a <= b).
 *     Skipped: one-class lists (no positive or no negative; empty lists included), then lists with a feature that is not finite.
 *     counters [3] int64 = lists used, one-class, with such a feature.  n_lists == 0 writes zeros (one launch).
 * FORMS: a 16-lane group per list of up to 16 items, half a wave up to 32, a wave up to 64, the workgroup beyond; form = 1 forces
 * the workgroup form for every list (test hook), any other value but 0: EBN_ERR_BAD_ARG.  Every floating-point sum is taken in ONE
 * order whatever the form (items ascending inside a list; lists ascending inside 16 slots per workgroup, slots ascending,
 * workgroups through a closing launch), without atomics and without contraction: two runs, both forms and every placement give
 * the same bits.
 * M outside [1, 16], n_items outside [0, 2^31 - 257], n_lists outside [0, 2^31 - 1], an unknown score_kind, a NULL among the
 * pointers (scores / features / labels / out may be NULL with n_items == 0; offsets and the workspace of the sums call with
 * n_lists == 0), a workspace that is not 16-byte aligned or smaller than the query: EBN_ERR_BAD_ARG.  All checked on the host
 * before the launch: a failing call launches and writes nothing.  n_lists == 0: nothing to do for features / combine.            */
#define EBN_BL_MAX_SOURCES 16
#define EBN_BL_RAW 0
#define EBN_BL_ZSCORE 1
#define EBN_BL_MINMAX 2
#define EBN_BL_RANK 3
#define EBN_BL_RRF 4
int ebn_blend_features_f32(const void* scores, int32_t score_kind, int32_t M, int64_t n_items, const int64_t* offsets, int64_t n_lists,
                           const int32_t* kinds, const double* params, int32_t form, float* features, uint8_t* flags,
                           ebn_stream_t stream);
int ebn_blend_combine_f64(const void* scores, int32_t score_kind, int32_t M, int64_t n_items, const int64_t* offsets, int64_t n_lists,
                          const int32_t* kinds, const double* params, const double* weights, int32_t form, double* out, uint8_t* flags,
                          ebn_stream_t stream);
/* Bytes of the workspace ebn_blend_sums_f64 needs (one partial per entry and workgroup); 0 for n_lists or M outside their ranges.
 * Pure host query.                                                                                                              */
int64_t ebn_blend_sums_workspace_bytes(int64_t n_lists, int32_t M);
int ebn_blend_sums_f64(const float* features, const uint8_t* labels, int32_t M, int64_t n_items, const int64_t* offsets, int64_t n_lists,
                       const double* weights, int32_t form, double* sums, int64_t* counters, void* workspace, int64_t workspace_bytes,
                       ebn_stream_t stream);

/* ---- history-kNN baseline (S-KNN / V-SKNN, Jannach & Ludewig 2017): neighbourhood collaborative filtering over whole click
 * sequences, "find the readers whose sequences look most like this one, and recommend what they read" (the reference has no such
 * baseline; the plain-Python brute force of tests/knn_cases.py is the yardstick; host layer: ebrec/models/baselines/knn.py) ------
 * FITTED DATA: n_seqs training sequences over n_rows catalogue rows; the host orders them by recency: sequence id s ASCENDS from
 * the oldest to the most recent.  Two CSR structures:
 *   POSTINGS  p_indptr [n_rows + 1] int64, p_seqs [nnz_p] int32 STRICTLY ASCENDING per row: the distinct sequences that hold the row
 *   SETS      s_indptr [n_seqs + 1] int64, s_items [nnz_s] int32 STRICTLY ASCENDING per sequence: its distinct rows
 * Every extent read from p_indptr / s_indptr / hist_offsets is clamped to its array ([0, nnz_p], [0, nnz_s], [0, n_hist_items])
 * before use, an extent that runs backwards is empty, and an id read from p_seqs addresses nothing before it is checked against
 * its range: whatever the arrays hold, nothing outside them is read.
 * QUERY: history u of n_hists holds the entries [hist_offsets[u], hist_offsets[u + 1]) of hist_rows [n_hist_items] int32 with the
 * weights hist_weights (NULL: every weight 1; finite: the host's guarantee).  An entry whose row is outside [0, n_rows) is ABSENT.
 * The query's ITEMS are its distinct present rows; an item has the weight of its LAST occurrence, and the items are ordered by
 * the position of that occurrence.  hist_self [n_hists] int32 or NULL: a sequence id never to be used (the user's own training
 * sequence), or -1.
 * CANDIDATES: the union is every sequence other than hist_self[u] that holds at least one item; the candidates are its
 * sample_size LARGEST ids (the most recent possible neighbours).  A candidate s that lies in the posting row of item i lies among
 * the last sample_size + 1 entries of that row: fewer than sample_size members of the union are larger than s, and the only id
 * the row can hold beyond them is hist_self.  So only that TAIL of every posting row is read, and what follows is exact.
 * SIMILARITY: dot(u, s) = the fp32 sum of the weights of the items that s holds, IN ITEM ORDER: the first one assigns, every
 * later one adds and rounds once.  sim = dot * seq_scale[s], one fp32 multiply; seq_scale [n_seqs] NULL: sim = dot.  (The host
 * passes 1 / sqrt(|set(s)|) for the cosine; the query's own norm is the same for all of its candidates and is left out.)
 *   ebn_knn_neighbours_f32: out_seq [n_hists, k] int32 / out_sim [n_hists, k] fp32: the best k candidates of every history, sim
 *     descending, then id DESCENDING (the more recent one first); -1 / -inf in the slots past the last candidate.  All
 *     2 n_hists k outputs are written and nothing else.  The order of a NaN sim is not defined (finite weights and scales give
 *     none).  One 256-thread workgroup per history walks ranges of ebn_knn_range() sequence ids from the most recent downwards
 *     -- an fp32 sum and a touched bit per id in LDS, the tails cut to the range by two binary searches per item, one barrier
 *     between items, the next range starting at the largest id a tail still holds -- until sample_size candidates are counted
 *     from the top; the pairs are sorted in LDS (bitonic).  No floating-point atomics, one fixed order: two runs give the same
 *     bits.  The last-occurrence scan costs (entries)^2 / 256 compares per history.  A history of at most 256 entries pays it
 *     ONCE and keeps what it staged (each range then cuts off what it took of a tail); a longer history is staged again, chunk
 *     by chunk, in EVERY visited range (up to n_seqs / ebn_knn_range() of them), scan and both searches included: meant for
 *     click histories, not for lists of 10^5 entries.
 *     n_rows / nnz_p / n_seqs / n_hists / n_hist_items outside [0, 2^31 - 1], sample_size < 1, k < 1, k > sample_size,
 *     n_hist_items > 0 with n_hists = 0, with n_hists > 0 a NULL hist_offsets / out_seq / out_sim, p_indptr (n_rows > 0), p_seqs
 *     (nnz_p > 0) or hist_rows (n_hist_items > 0): EBN_ERR_BAD_ARG; then k > EBN_KNN_MAX_K or sample_size > EBN_KNN_MAX_SAMPLE:
 *     EBN_ERR_UNSUPPORTED; then n_hists == 0: nothing to do (EBN_OK, no launch).  seq_scale, hist_weights and hist_self may be
 *     NULL; n_rows == 0 or nnz_p == 0 gives -1 / -inf everywhere in one launch.  sample_size > 2048 needs more than 64 KiB of
 *     LDS: a device that refuses the function attribute for it gives EBN_ERR_UNSUPPORTED, nothing launched.
 *   ebn_knn_scores_f32: nbr_seq / nbr_sim [n_hists, k] as the call above leaves them.  For item i of list l, c = cand_rows[i],
 *     u = list_hist ? list_hist[l] : l (lists as for ebn_cv_scores_f32):
 *       scores[i] = item_scale[c] * sum over the n with 0 <= nbr_seq[u, n] < n_seqs and c in set(nbr_seq[u, n]) of nbr_sim[u, n]
 *     item_scale [n_rows] NULL: 1.  Exactly +0.0f when the item is absent (c outside [0, n_rows)), u is outside [0, n_hists) or
 *     history u has no neighbour.  All n_cand_items scores are written and nothing else.  256-item workgroups: one lane per item
 *     finds its list and history; then one wave per item: lane s takes the neighbours s, s + 64, ..., binary-searches c in the
 *     neighbour's set and adds the sim at a hit; a butterfly (xor 32 .. 1) folds the lanes.  The order of the sum is the
 *     kernel's own and fixed; no atomics, no workspace: two runs give the same bits.
 *     n_seqs / nnz_s / n_rows / n_hists / n_lists / n_cand_items outside [0, 2^31 - 1], k < 1, n_cand_items > 0 with n_lists = 0,
 *     with n_cand_items > 0 a NULL cand_rows / cand_offsets / scores, s_indptr (n_seqs > 0), s_items (nnz_s > 0) or nbr_seq /
 *     nbr_sim (n_hists > 0): EBN_ERR_BAD_ARG; then k > EBN_KNN_MAX_K: EBN_ERR_UNSUPPORTED; then n_cand_items == 0: nothing to do
 *     (EBN_OK, no launch).  item_scale and list_hist may be NULL.
 * All checked on the host before the launch: a failing call launches and writes nothing.                                          */
#define EBN_KNN_MAX_K 512
#define EBN_KNN_MAX_SAMPLE 4096 /* 1 <= k <= sample_size */
/* The sequence ids one LDS tile of the neighbour kernel covers.  Pure host query.                                                  */
int64_t ebn_knn_range(void);
int ebn_knn_neighbours_f32(const int64_t* p_indptr, const int32_t* p_seqs, int64_t n_rows, int64_t nnz_p, int64_t n_seqs,
                           const float* seq_scale, const int32_t* hist_rows, const float* hist_weights, const int64_t* hist_offsets,
                           int64_t n_hists, int64_t n_hist_items, const int32_t* hist_self, int32_t sample_size, int32_t k,
                           int32_t* out_seq, float* out_sim, ebn_stream_t stream);
int ebn_knn_scores_f32(const int64_t* s_indptr, const int32_t* s_items, int64_t n_seqs, int64_t nnz_s, int64_t n_rows,
                       const float* item_scale, const int32_t* nbr_seq, const float* nbr_sim, int64_t n_hists, int32_t k,
                       const int32_t* list_hist, const int32_t* cand_rows, const int64_t* cand_offsets, int64_t n_lists,
                       int64_t n_cand_items, float* scores, ebn_stream_t stream);

/* ---- history-kNN top-N lists and clicked-article ranks over the whole catalogue (csrc/ebn_knn_topk.hip, ebn_knn_tile.h; the
 * plain-Python brute force of tests/knn_topn_cases.py is the yardstick): what ebn_cv_topk_f32 and ebn_cv_target_rank_f32 are to the
 * co-visitation matrix, for the score of ebn_knn_scores_f32 -----------------------------------------------------------------------
 * Everything not said here is ebn_cv_topk_f32's / ebn_cv_target_rank_f32's: user_hist, cand_pos and M, window [U, 2] and its
 * clamping, exclude [U, X] matching by catalogue row, the total order, flags [2] only ever SET, target_pos, the rank / count / score
 * outputs, n_splits and the workspace layouts, all argument checks on the host before anything is launched.
 * SETS: s_indptr [n_seqs + 1] int64 / s_items [nnz_s] int32 of the fitted index, as ebn_knn_scores_f32 takes them: the rows of a set
 * are distinct and ASCENDING.  Every extent read from s_indptr is clamped to [0, nnz_s] (end < begin: empty); every row read from
 * s_items is checked against the rows of the tile in hand before it addresses anything.  item_scale [n_rows] fp32 or NULL.
 * NEIGHBOURS: nbr_seq / nbr_sim [n_hists, k_nbr] as ebn_knn_neighbours_f32 leaves them, 1 <= k_nbr <= EBN_KNN_MAX_K; user u of U
 * uses row user_hist ? user_hist[u] : u, an index outside [0, n_hists) is a user without neighbours.  A sequence id outside
 * [0, n_seqs) is an ABSENT neighbour.
 * SCORE: row c is TOUCHED by user u when the set of at least one present neighbour holds it.  The neighbour slots are walked in
 * list order j = 0 .. k_nbr - 1: the first touching neighbour assigns acc = sim_j, every later one does acc = acc + sim_j, each add
 * rounding once to fp32; then score = item_scale ? acc * item_scale[c] (one rounding) : acc.  A sequence listed twice counts
 * twice.  No floating-point atomics.  A score's bits depend on that user's neighbour row and the sets only: not on U, M, n_splits,
 * the run or the other users of the launch.
 * ADMISSIBLE: row c for user u when it is touched, cand_pos[c] lies in [0, M) and in u's clamped window, c is not in exclude[u, :]
 * and the score is not NaN.  A NaN score of a row that is admissible otherwise sets flags[1]; a touched row with cand_pos[c] >= M
 * sets flags[0].  An untouched row never enters a list; a touched row with score 0 or below does.
 *   ebn_knn_topk_f32: out_pos [U, k] / out_score [U, k]: each user's best k admissible rows as (position, score), score descending,
 *     then position ascending; -1 / -inf in the empty trailing slots.  1 <= k <= 64.
 *   ebn_knn_target_rank_f32: target_pos [U] int32 on the DEVICE (required); out_rank / out_count / out_score as
 *     ebn_target_rank_f32 defines them over this admissible set; rank 0 (score -inf) when there is no target (< 0; >= M also sets
 *     flags[0]), the position belongs to no row, or the target's row is untouched or not admissible.  The target's score has the
 *     bits ebn_knn_topk_f32 gives the same (user, row) pair.
 * One 256-thread workgroup per (user, split) stages the neighbour row in LDS once and walks ranges of ebn_knn_topk_range() catalogue
 * rows; every wave owns a quarter of the range as a private fp32 tile with two bits per row, cuts all sets to it with one lane per
 * neighbour and applies the neighbours with a segment in list order: no workgroup barrier inside the walk (42 KiB of LDS).
 * Results are bit-identical for every n_splits and from run to run.
 * Any of n_seqs / nnz_s / n_rows / n_hists / M / U outside [0, 2^31 - 1], X < 0, n_splits < 0, workspace_bytes < 0, k_nbr < 1,
 * cand_pos NULL with M != n_rows: EBN_ERR_BAD_ARG; then k outside [1, 64], X > 256 or k_nbr > EBN_KNN_MAX_K: EBN_ERR_UNSUPPORTED;
 * then U == 0: nothing to do (EBN_OK, no launch); then a NULL output, flags or target_pos: EBN_ERR_BAD_ARG; then n_rows == 0,
 * n_seqs == 0, nnz_s == 0 or M == 0: empty outputs in one launch (-1 / -inf; rank 0, count 0, -inf, and flags[0] for a target
 * position >= M); then a NULL s_indptr / s_items, or nbr_seq / nbr_sim with n_hists > 0: EBN_ERR_BAD_ARG; then the workspace
 * (too small or NULL: EBN_ERR_BAD_ARG; not 16-byte aligned: EBN_ERR_ALIGN).  item_scale, user_hist, cand_pos, window and exclude
 * (then X counts as 0) may be NULL.                                                                                                */
/* The catalogue rows one range covers (four wave tiles).  Pure host query.                                                          */
int64_t ebn_knn_topk_range(void);
/* The number of row ranges n_splits = 0 stands for: 1 once the users alone give about 2 048 workgroups.  Pure host query, >= 1.   */
int ebn_knn_topk_auto_splits(int64_t n_users, int64_t n_rows);
/* Bytes of workspace for n_splits >= 1, as ebn_cv_topk_workspace_bytes / ebn_cv_target_rank_workspace_bytes give them (a nominal
 * 16 where none is needed; 0 for sizes outside the limits; n_positions: M when the rank call gets a cand_pos, else 0).  Pure host
 * queries.                                                                                                                          */
int64_t ebn_knn_topk_workspace_bytes(int64_t n_users, int32_t k, int32_t n_splits);
int64_t ebn_knn_target_rank_workspace_bytes(int64_t n_users, int32_t n_splits, int64_t n_positions);
int ebn_knn_topk_f32(const int64_t* s_indptr, const int32_t* s_items, int64_t n_seqs, int64_t nnz_s, int64_t n_rows,
                     const float* item_scale, const int32_t* nbr_seq, const float* nbr_sim, int64_t n_hists, int32_t k_nbr,
                     const int32_t* user_hist, const int32_t* cand_pos, int64_t M, const int32_t* window, const int32_t* exclude,
                     int32_t X, int32_t k, int32_t n_splits, int32_t* out_pos, float* out_score, int32_t* flags, void* workspace,
                     int64_t workspace_bytes, int64_t U, ebn_stream_t stream);
int ebn_knn_target_rank_f32(const int64_t* s_indptr, const int32_t* s_items, int64_t n_seqs, int64_t nnz_s, int64_t n_rows,
                            const float* item_scale, const int32_t* nbr_seq, const float* nbr_sim, int64_t n_hists, int32_t k_nbr,
                            const int32_t* user_hist, const int32_t* cand_pos, int64_t M, const int32_t* target_pos,
                            const int32_t* window, const int32_t* exclude, int32_t X, int32_t n_splits, int32_t* out_rank,
                            int32_t* out_count, float* out_score, int32_t* flags, void* workspace, int64_t workspace_bytes, int64_t U,
                            ebn_stream_t stream);

/* ---- EASE^R baseline (Steck, "Embarrassingly Shallow Autoencoders for Sparse Data", WWW 2019): the item-to-item ridge regression in
 * closed form (the reference has no such baseline; the float64 brute force of tests/ease_cases.py is the yardstick; host layer:
 * ebrec/models/baselines/ease.py; kernels: csrc/ebn_ease.hip) ---------------------------------------------------------------------
 * With X [users, n] binary (item i occurs in user u's sequence):  G = X^T X (co-click counts, item counts on the diagonal),
 * A = G + reg I,  P = A^{-1},  B[i, j] = -P[i, j] / P[j, j] for i != j, B[j, j] = 0.  The score of candidate c for a history
 * h_1 .. h_m with weights w is sum_j w_j B[h_j, c] (x^T B: B is not symmetric).  One entry point per stage:
 *   ebn_ease_gram_i32: CSR over n_users rows: row u holds the entries [indptr[u], indptr[u + 1]) clamped to [0, nnz] of cols [nnz]
 *     int32, taken AS GIVEN (the host layer makes them ascending and distinct; a repeated column counts as often as it pairs); an
 *     entry outside [0, n_items) is skipped and never turned into an address.  G int32 [n_items, ldg]: the call zeroes the LOWER
 *     triangle (j <= i) itself, then adds 1 to G[max(a, b), min(a, b)] for every pair of positions p >= q of a row whose columns
 *     a, b are present, with INTEGER global atomics: integer sums commute, two runs give the same bits.  The upper triangle and the
 *     columns >= n_items are never written.  One 256-thread workgroup per row; a row of m entries costs m (m + 1) / 2 atomics
 *     spread over its threads; m is not capped.
 *     n_users / nnz / n_items / ldg outside [0, 2^31 - 1], ldg < n_items, a NULL G (n_items > 0), indptr (n_users > 0) or cols
 *     (nnz > 0): EBN_ERR_BAD_ARG; then n_items > EBN_EASE_MAX_ITEMS: EBN_ERR_UNSUPPORTED; then n_items == 0: nothing to do (EBN_OK,
 *     no launch).  n_users == 0 or nnz == 0: zeros in one launch.
 *   ebn_ease_system_f32: A[i, j] = A[j, i] = (float) G[max(i, j), min(i, j)] for i, j < n, plus reg on the diagonal (one fp32 add);
 *     only the lower triangle of G is read, only columns < n of A are written.  *flag (device int32, only ever SET: the caller
 *     zeroes it) becomes 1 when a count read exceeds 2^24, where it is no longer exact in fp32.
 *     n / ldg / lda outside [0, 2^31 - 1], ldg < n, lda < n, reg not finite, with n > 0 a NULL G / A / flag: EBN_ERR_BAD_ARG; then
 *     n > EBN_EASE_MAX_ITEMS: EBN_ERR_UNSUPPORTED; then n == 0: EBN_OK, no launch.
 *   ebn_ease_invert_f32: A [n, n] at row stride lda, symmetric positive definite (only its lower triangle is read), is overwritten
 *     by the full symmetric A^{-1}: (i, j) and (j, i) hold the same bits; columns >= n are never read or written.  A host loop of
 *     launches on `stream`, no synchronisation and no host read in between: (1) blocked right-looking Cholesky with block size
 *     NB = ebn_ease_block(): a one-workgroup kernel factorises the NB x NB diagonal block in LDS (fixed order, correctly rounded
 *     sqrtf and division) and inverts its triangular factor in the same launch, W_k = L_kk^{-1}; the panel below, L_ik = A_ik W_k^T,
 *     and the trailing update A_22 -= L_21 L_21^T (column strips starting at the diagonal) run on ebn_gemm_f32; (2) Z = L^{-1} by
 *     block forward substitution with the same W_k and GEMMs; (3) P = Z^T Z by GEMMs over column strips, then mirrored.  No
 *     floating-point atomics and no split-K: two runs give the same bits.  n need not be a multiple of NB.
 *     info (device int32) is WRITTEN: 0 = ok, k + 1 = the first pivot (global index k) that was not > 0, NaN included.  After such
 *     a pivot the remaining launches still run and A holds NaN-filled garbage; nothing faults and nothing waits for the host (the
 *     host layer raises FloatingPointError).  work: ebn_ease_workspace_floats(n) floats, written before they are read; 16-byte
 *     alignment of A / work and lda % 4 == 0, n % 4 == 0 let the GEMMs use their vector loads (the bits then depend on it, as
 *     ebn_gemm_f32's do).
 *     n / lda outside [0, 2^31 - 1], lda < n, a NULL A / work / info: EBN_ERR_BAD_ARG; then n > EBN_EASE_MAX_ITEMS or work_floats
 *     below the query: EBN_ERR_UNSUPPORTED; then n == 0: EBN_OK, no launch.
 *   ebn_ease_invert_nb_f32: the same with the block size given, nb in {32, 64, 128} (else EBN_ERR_BAD_ARG, with the first group):
 *     the measurement hook behind the choice of ebn_ease_block() (tools/ease_probe.py).  The workspace query covers every nb.
 *   ebn_ease_weights_f32: B[i, j] = -(P[i, j] / P[j, j]) for i != j (correctly rounded division), exact +0.0 on the diagonal;
 *     n * n elements are written and nothing else.  B == P (in place) is allowed: the first launch writes the off-diagonal
 *     elements and only reads the diagonal, the second writes the diagonal.
 *     n / ldp / ldb outside [0, 2^31 - 1], ldp < n, ldb < n, with n > 0 a NULL P / B: EBN_ERR_BAD_ARG; then
 *     n > EBN_EASE_MAX_ITEMS: EBN_ERR_UNSUPPORTED; then n == 0: EBN_OK, no launch.
 *   ebn_ease_scores_f32: B [n_items, ldb] fp32; histories and lists as for ebn_cv_scores_f32 (hist_rows / hist_weights /
 *     hist_offsets, list_hist, cand_rows / cand_offsets; extents clamped to [0, n_hist_items]; an entry or item whose row is
 *     outside [0, n_items) is ABSENT; an entry that occurs twice counts twice).  For item i of list l, c = cand_rows[i],
 *     u = list_hist ? list_hist[l] : l:
 *       scores[i] = sum over the present entries j of history u of w_j * B[hist_rows[j], c]          (w_j = 1 with hist_weights NULL)
 *     exactly +0.0f when the item is absent, u is outside [0, n_hists) or history u has no present entry.  All n_cand_items scores
 *     are written and nothing else.  256-item workgroups: one lane per item finds its list and history; then one wave per item:
 *     lane s takes the entries s, s + 64, ... in order (one fused multiply-add each; a plain add without weights), a butterfly
 *     (xor 32 .. 1) folds the lanes.  The order is fixed, no atomics, no workspace: two runs give the same bits.
 *     n_items / ldb / n_hists / n_hist_items / n_lists / n_cand_items outside [0, 2^31 - 1], ldb < n_items, n_cand_items > 0 with
 *     n_lists = 0, n_hist_items > 0 with n_hists = 0: EBN_ERR_BAD_ARG; then n_cand_items == 0: nothing to do (EBN_OK, no launch);
 *     then a NULL cand_rows / cand_offsets / scores, B (n_items > 0), hist_offsets (n_hists > 0) or hist_rows (n_hist_items > 0):
 *     EBN_ERR_BAD_ARG.  hist_weights and list_hist may be NULL.
 * All checked on the host before the launch: a failing call launches and writes nothing.                                          */
#define EBN_EASE_MAX_ITEMS 32768
/* The block size NB of ebn_ease_invert_f32.  Pure host query.                                                                      */
int ebn_ease_block(void);
/* Floats of workspace for ebn_ease_invert_f32 / ebn_ease_invert_nb_f32 (about n^2 + 256 n); 0 for n outside [0, EBN_EASE_MAX_ITEMS].
 * Pure host query.                                                                                                                 */
int64_t ebn_ease_workspace_floats(int64_t n);
int ebn_ease_gram_i32(const int64_t* indptr, const int32_t* cols, int64_t n_users, int64_t nnz, int64_t n_items, int32_t* G,
                      int64_t ldg, ebn_stream_t stream);
int ebn_ease_system_f32(const int32_t* G, int64_t ldg, int64_t n, float reg, float* A, int64_t lda, int32_t* flag,
                        ebn_stream_t stream);
int ebn_ease_invert_f32(float* A, int64_t lda, int64_t n, float* work, int64_t work_floats, int32_t* info, ebn_stream_t stream);
int ebn_ease_invert_nb_f32(float* A, int64_t lda, int64_t n, float* work, int64_t work_floats, int32_t* info, int32_t nb,
                           ebn_stream_t stream);
int ebn_ease_weights_f32(const float* P, int64_t ldp, int64_t n, float* B, int64_t ldb, ebn_stream_t stream);
int ebn_ease_scores_f32(const float* B, int64_t n_items, int64_t ldb, const int32_t* hist_rows, const float* hist_weights,
                        const int64_t* hist_offsets, int64_t n_hists, int64_t n_hist_items, const int32_t* list_hist,
                        const int32_t* cand_rows, const int64_t* cand_offsets, int64_t n_lists, int64_t n_cand_items, float* scores,
                        ebn_stream_t stream);

/* ---- EASE top-N lists and clicked-article ranks over the whole catalogue (csrc/ebn_ease_topk.hip; the plain-Python brute force of
 * tests/ease_topn_cases.py is the yardstick): what ebn_cv_topk_f32 and ebn_cv_target_rank_f32 are to the co-visitation matrix, for
 * the DENSE row sums of EASE -------------------------------------------------------------------------------------------------------
 * Everything not said here is ebn_cv_topk_f32's / ebn_cv_target_rank_f32's: the history operands and their clamping to
 * [0, n_hist_items], ABSENT entries (a row outside [0, n_rows): it adds nothing and is never turned into an address), a repeated
 * entry counting twice, user_hist, cand_pos [n_rows] (negative: no candidate; NULL: position = row, then M == n_rows; >= M: skipped
 * and flags[0] set), window [U, 2] and exclude [U, X] by catalogue row, the total order (score descending, then position
 * ascending) with -1 / -inf in the empty trailing slots, flags [2] only ever SET, the outputs of the rank call, the workspace
 * rules, all argument checks on the host before anything is launched: a failing call writes nothing.
 * MATRIX: B [n_rows, ldb] fp32, row-major, any ldb >= n_rows and any alignment: the weights of ebn_ease_weights_f32.  Only the
 * columns < n_rows of a row are read.
 * SCORE: column c is scored for user u when u's history has at least one present entry -- B is dense, there is no "touched"
 * notion: every column of such a user has a score, a user without a present entry has none (an empty list; rank 0, count 0,
 * score -inf).  With p_j = w_j * B[hist_rows[j], c] (hist_weights NULL: the stored value itself): the score starts as the first
 * present entry's p_j; every later present entry, in history order, does acc = acc + p_j.  Every product and every add rounds
 * once to fp32 (no fused multiply-add).  A score's bits depend on that user's history and that column of B only: not on U, M,
 * n_splits, ldb, the alignment of B (16-byte loads or 4-byte loads: the same operations), the run or the other users of the
 * launch.  No floating-point atomics.  This chain is NOT the lane-strided fma order of ebn_ease_scores_f32: predict and recommend
 * agree to rounding (two fp32 summation orders of the same rounded products), not in bits.
 * ADMISSIBLE: column c for user u when it is scored, cand_pos[c] lies in [0, M) and in u's clamped window, c is not in
 * exclude[u, :] and the score is not NaN.  A NaN score that is admissible otherwise sets flags[1]; +-inf rank like numbers.  A
 * position >= M sets flags[0] when some user with a present entry walks the column.
 *   ebn_ease_topk_f32: out_pos [U, k] / out_score [U, k], 1 <= k <= 64.
 *   ebn_ease_target_rank_f32: target_pos [U] int32 on the DEVICE (required); t has the bits ebn_ease_topk_f32 gives the same
 *     (user, column) pair.
 * One 256-thread workgroup per (user, split) walks ranges of ebn_ease_topk_range() columns: every thread keeps the sums of its
 * own columns of the range in registers and reads, per present history entry, its 16 bytes of each of its groups of four columns
 * of that row of B, several rows' loads in flight; the present entries of the history are staged once in LDS (256 at a time, in
 * order).  Selection per wave in registers, the four lists merged by wave 0; the rank call evaluates the target column's chain
 * first (one load per entry, folded in history order) and counts in the same walk.  n_splits: 0 =
 * ebn_ease_topk_auto_splits(U, n_rows); clamped to the number of ranges and to 64; partial lists / counts in the workspace
 * layouts of ebn_cv_topk_f32 / ebn_cv_target_rank_f32, merged / added by a second launch.  Results are bit-identical for every
 * n_splits and from run to run.
 * Any of n_rows / ldb / n_hists / n_hist_items / M / U outside [0, 2^31 - 1], X < 0, n_splits < 0, workspace_bytes < 0,
 * ldb < n_rows, n_hist_items > 0 with n_hists = 0, cand_pos NULL with M != n_rows: EBN_ERR_BAD_ARG; then k outside [1, 64],
 * X > 256 or n_rows > EBN_EASE_MAX_ITEMS: EBN_ERR_UNSUPPORTED; then U == 0: nothing to do (EBN_OK, no launch); then a NULL output,
 * flags or target_pos: EBN_ERR_BAD_ARG; then n_rows == 0 or M == 0: empty outputs in one launch (-1 / -inf; rank 0, count 0,
 * -inf, and flags[0] for a target position >= M); then a NULL B, hist_offsets with n_hists > 0 or hist_rows with
 * n_hist_items > 0: EBN_ERR_BAD_ARG; then the workspace (NULL or too small: EBN_ERR_BAD_ARG; not 16-byte aligned: EBN_ERR_ALIGN).
 * hist_weights, user_hist, cand_pos, window and exclude (then X counts as 0) may be NULL.                                         */
/* The catalogue columns one pass of a workgroup covers.  Pure host query.                                                          */
int64_t ebn_ease_topk_range(void);
/* The number of column ranges n_splits = 0 stands for: 1 once the users alone give about 16 384 workgroups.  Pure host query, >= 1. */
int ebn_ease_topk_auto_splits(int64_t n_users, int64_t n_rows);
/* Bytes of workspace for n_splits >= 1, as ebn_cv_topk_workspace_bytes / ebn_cv_target_rank_workspace_bytes give them (a nominal
 * 16 where none is needed; 0 for sizes outside the limits; n_positions: M when the rank call gets a cand_pos, else 0).  Pure host
 * queries.                                                                                                                          */
int64_t ebn_ease_topk_workspace_bytes(int64_t n_users, int32_t k, int32_t n_splits);
int64_t ebn_ease_target_rank_workspace_bytes(int64_t n_users, int32_t n_splits, int64_t n_positions);
int ebn_ease_topk_f32(const float* B, int64_t n_rows, int64_t ldb, const int32_t* hist_rows, const float* hist_weights,
                      const int64_t* hist_offsets, int64_t n_hists, int64_t n_hist_items, const int32_t* user_hist,
                      const int32_t* cand_pos, int64_t M, const int32_t* window, const int32_t* exclude, int32_t X, int32_t k,
                      int32_t n_splits, int32_t* out_pos, float* out_score, int32_t* flags, void* workspace, int64_t workspace_bytes,
                      int64_t U, ebn_stream_t stream);
int ebn_ease_target_rank_f32(const float* B, int64_t n_rows, int64_t ldb, const int32_t* hist_rows, const float* hist_weights,
                             const int64_t* hist_offsets, int64_t n_hists, int64_t n_hist_items, const int32_t* user_hist,
                             const int32_t* cand_pos, int64_t M, const int32_t* target_pos, const int32_t* window,
                             const int32_t* exclude, int32_t X, int32_t n_splits, int32_t* out_rank, int32_t* out_count,
                             float* out_score, int32_t* flags, void* workspace, int64_t workspace_bytes, int64_t U,
                             ebn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* EBNERD_HIP_H */

/* taco_hip.h -- C ABI of libtaco_hip.so, the MI355X (gfx950) implementation of the Tacotron acoustic-model
 * hot path of barronalex/Tacotron (models/tacotron.py + models/ops.py).
 *
 * The reference has NO FFI / plugin boundary (it is a pure-Python TF-1.2 graph), so every entry
 * point below cites the reference function whose arithmetic it replaces.  Conventions:
 *   - every function returns int: 0 = ok, negative = TACO_E* (never throws, never exits);
 *     taco_last_error_string() describes the last failure on the calling thread;
 *   - all pointers except `shape`/tables are DEVICE pointers, contiguous row-major, fp32 unless stated;
 *   - one call = stream-ordered enqueues on `stream` (a hipStream_t passed as void*); no allocation, no
 *     host synchronisation, no ownership transfer.  The caller supplies parameters, inputs, outputs and a
 *     workspace of taco_workspace_bytes() bytes;
 *   - tensors are batch-major (B, T, C); weights use the reference's TF variable layouts
 *     (dense kernel (in,out); conv1d kernel (k,Cin,Cout); GRUCell gates kernel (Cin+H,2H) r-then-u ...).
 */
#ifndef TACO_HIP_H
#define TACO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

#define TACO_VERSION 120

#define TACO_OK 0
#define TACO_EINVAL (-1)   /* bad argument / unsupported shape   */
#define TACO_ELAUNCH (-2)  /* HIP launch or runtime error        */
#define TACO_ENOTFOUND (-3)

/* activation codes for taco_conv_gemm */
#define TACO_ACT_NONE 0
#define TACO_ACT_RELU 1
#define TACO_ACT_SIGMOID 2
#define TACO_ACT_TANH 3

/* Problem shape.  Model widths (embed 256, prenet 256/128, CBHG 128, attention/decoder 256, 80 mels, 1025 bins,
 * K=16/8 conv banks) are the reference's Config constants (tacotron.py:12-33, 131, 147) and are compiled in. */
typedef struct TacoShape {
  int32_t B;   /* batch (Config.batch_size = 32)                                    */
  int32_t Tt;  /* padded text length                                               */
  int32_t Td;  /* decoder steps = Config.max_decode_iter (tacotron.py:13)          */
  int32_t r;   /* mel frames per decoder step (audio.r, audio.py:15-17)            */
  int32_t V;   /* vocab_size (train.py:22)                                         */
  int32_t S;   /* num_speakers (tacotron.py:23); <= 1 = single speaker, no speaker path */
} TacoShape;

/* One row of the parameter / workspace tables. */
typedef struct TacoTensorInfo {
  char name[64];
  int64_t offset; /* in floats from the base pointer */
  int64_t size;   /* in floats                      */
  int32_t ndim;
  int32_t dims[4];
} TacoTensorInfo;

int taco_version(void);
const char* taco_last_error_string(void);

/* ---- parameter layout: one flat fp32 buffer, TF variable order (tacotron.py:107-154 graph order) ---------- */
int64_t taco_param_count(const TacoShape* shape);
/* Fills up to `cap` rows; returns the number of tensors (or negative error). */
int taco_param_table(const TacoShape* shape, TacoTensorInfo* rows, int cap);

/* ---- workspace ------------------------------------------------------------------------------------------ */
/* Bytes needed by taco_forward / taco_backward / taco_infer for `shape` (train != 0 includes backward stashes). */
int64_t taco_workspace_bytes(const TacoShape* shape, int train);
/* Named intermediate tensors inside the workspace (for parity tests / debugging). */
int taco_workspace_table(const TacoShape* shape, int train, TacoTensorInfo* rows, int cap);

/* ---- op level ------------------------------------------------------------------------------------------- */
/* C[m, n] = post( act( sum_{tap<taps} sum_{k<K} A[row(m,tap), k] * W[tap][k][n] + bias[n] ) )
 *   row(m,tap): m = b*T + t  ->  t' = t + tap - pad_l ; zero row unless 0 <= t' < T   ('same' conv1d, ops.py:54-60;
 *   taps = 1, pad_l = 0 is tf.layers.dense, tacotron.py:40-43).
 *   post(y) = (keep ? y * keep[m,n] * 2 : y) * scale[n] + shift[n] + residual[m,n]   (each optional / nullable)
 *   scale and shift are independent: either alone applies (scale alone: y * scale[n]; shift alone: y + shift[n]).
 *   Cpre (nullable) receives the value before scale/shift/residual.  W tap stride is K*ldw floats.
 *   Pitches: A lda, W ldw, residual ldr, C ldc; Cpre has no pitch argument of its own and is written with the pitch of C
 *   (element (m, n) at Cpre[m * ldc + n]); keep is dense, one byte per element, read at keep[m * N + n].  No pointer needs more
 *   than its type's alignment: 16-byte aligned operands with pitches and K, N multiples of 4 only select the vector forms. */
int taco_conv_gemm(const float* A, int lda, const float* W, int ldw, const float* bias, const float* scale,
                   const float* shift, const float* residual, int ldr, const uint8_t* keep, float* C, int ldc,
                   float* Cpre, int M, int N, int K, int taps, int T, int pad_l, int act, void* stream);

/* Same contract (without the post() part), run the way the library runs the tall-skinny CBHG projections: the (tap, k) sum is
 * cut into chunks that become independent workgroups writing partial slabs (scratch `slabs`, `slab_floats` floats), summed in a
 * fixed order by a second pass -- deterministic, no atomics.  Exposed for parity tests and tuning. */
/* debug: only the eligible NN launches whose running index falls in [lo, hi) use gemm2.hip's kernel (bisecting a divergence);
 * returns the number of eligible (non-pooled) launches seen since the previous call and restarts the count */
int taco_debug_gemm2_window(int lo, int hi);
/* Pre-split weight images (round 6; csrc/kernels.h "weight images"): the bf16 plane image of a weight tensor W (taps, K, N; row pitch
 * ldw) that gemm2.hip's NN kernel reads instead of splitting W in registers.  The model-level entry points build the images of
 * their own weights themselves (into the workspace) and drop them from the table when they return; this is the op-level door
 * for parity tests and tools.  Op-level calls see only images registered here, and those stay until the next W == NULL call or
 * the next model-level call (which empties this thread's table on entry).
 *   W == NULL: clears this host thread's table, returns the number of launches that ran the image form since the previous such
 *   call (all threads).   img == NULL: returns the bytes image(W) needs.
 *   otherwise: registers image(W) at img (16-byte aligned, img_bytes >= that size) and enqueues its build on `stream`; the
 *   following taco_conv_gemm / taco_debug_conv_gemm_* calls of this thread whose weight pointer, pitch, taps, K equal W's and whose
 *   N <= N run the image form.  Replaces nothing in the reference (TF holds fp32 kernels only; models/ops.py:54-60,80-86). */
int64_t taco_debug_weight_image(const float* W, int ldw, int taps, int K, int N, void* img, int64_t img_bytes, void* stream);
/* debug / test aid: dense layer with weight rows zero-padded to nld loadable columns (the final 256 -> 1025 layer's form) */
int taco_debug_conv_gemm_nld(const float* A, int lda, const float* W, int ldw, int nld, const float* bias, float* C, int ldc, int M,
                             int N, int K, int act, void* stream);
int taco_debug_conv_gemm_ksplit(const float* A, int lda, const float* W, int ldw, const float* bias, float* C, int ldc, int M,
                                int N, int K, int taps, int T, int pad_l, int act, float* slabs, int64_t slab_floats,
                                void* stream);

/* dW[tap][k][n] (+)= sum_m A[row(m,tap), k] * dY[m, n]   (weight gradient of the op above; accumulate != 0 adds) */
int taco_gemm_tn(const float* A, int lda, const float* dY, int ldy, float* dW, int ldw, int M, int N, int K, int taps,
                 int T, int pad_l, int accumulate, void* stream);

/* Reference GEMM on scalar FMAs (debug aid for the MFMA kernels; same contract as taco_conv_gemm without post). */
int taco_debug_gemm_naive(const float* A, int lda, const float* W, int ldw, const float* bias, float* C, int ldc,
                          int M, int N, int K, int taps, int T, int pad_l, int act, void* stream);

/* Bidirectional GRU(128) over the full padded length (ops.py:117-128; tf.nn.bidirectional_dynamic_rnn without
 * sequence_length).  x (B,T,128); weights in TF GRUCell layout: wg (256,256), bg (256), wc (256,128), bc (128) per
 * direction.  out (B,T,256) = concat(fw,bw).  ruc (B,T,768) receives r,u,c for both directions (nullable).
 * xg (B,T,768) is scratch for the hoisted input projections. */
int taco_bigru_fwd(const float* x, const float* wg_fw, const float* bg_fw, const float* wc_fw, const float* bc_fw,
                   const float* wg_bw, const float* bg_bw, const float* wc_bw, const float* bc_bw, float* xg,
                   float* out, float* ruc, int B, int T, void* stream);

/* ---- op-level debug doors of the CBHG tail (tests/test_gpu_cbhg_tail.py) ------------------------------------
 * Thin wrappers over the launches the model makes for the bi-GRU recurrences (bigru.hip), the highway stacks (highway.hip) and
 * the encoder pre_net (prenet.hip), so that a test can place every operand itself.  All tensors fp32, dense and row-major.  A null
 * operand that is not marked nullable, a size out of range, or an output whose bytes meet those of any other operand returns
 * TACO_EINVAL with a message that names the argument, before anything is enqueued.  Outputs arrive with arbitrary contents; no
 * call writes a byte outside the extents given here.  TACO_VERSION did not change with these entry points: detect them by the
 * symbol.
 *
 * taco_debug_bigru_rec_fwd: the forward recurrence of both directions without the x-side projection.
 *   xg (B,T,768): per direction d the pre-activations [x.Wg_x + bg (256: r | u) | x.Wc_x + bc (128)] at columns [384 d, 384 d + 384);
 *   wg_* (256,256), wc_* (256,128): the GRUCell kernels in TF layout, of which rows [128, 256) (the h side) are read;
 *   h0 (B,128) initial state of both directions, nullable (zeros).
 *   out (B,T,256) = [fw | bw]; ruc (B,T,768), nullable: per direction [r | u | c] at columns [384 d, 384 d + 384).
 * taco_debug_bigru_bwd: the backward recurrence (BPTT) of both directions.
 *   dout (B,T,256) gradient of out; out, ruc as the forward call wrote them; h0 as given to it (nullable);
 *   wghT_* (256,128) = Wg[128:, :]^T, wchT_* (128,128) = Wc[128:, :]^T (the layout of BiGruBwdWeights, csrc/kernels.h).
 *   dxg (B,T,768) gradient of xg; rh (B,T,256) = r * h_prev per direction; dh0 (2,B,128), nullable: gradient of h0 per direction. */
int taco_debug_bigru_rec_fwd(const float* xg, const float* wg_fw, const float* wc_fw, const float* wg_bw, const float* wc_bw,
                             const float* h0, float* out, float* ruc, int B, int T, void* stream);
int taco_debug_bigru_bwd(const float* dout, const float* out, const float* ruc, const float* wghT_fw, const float* wchT_fw,
                         const float* wghT_bw, const float* wchT_bw, const float* h0, float* dxg, float* rh, float* dh0, int B, int T,
                         void* stream);
/* taco_debug_highway_stack_fwd / _bwd: the fields of HighwayStackArgs / HighwayStackBwdArgs (csrc/kernels.h).  Every `const*`
 * argument is a table of 4 pointers, one per layer, of which entries [0, nl) are read; nl in [1, 4].
 *   forward : x (M,128); wt, wh (128,128), bt, bh (128) per layer; y[l] (M,128) the layer's output; th, nullable as a table:
 *             th[l] (M,256) = [T | H].  Adapter form (wa != NULL; nl == 4, T divides M): wa[l] (128,128), rowb[l] (M / T,128),
 *             hx[l] (M,128) = y[l-1] . wa[l] + rowb[l][m / T], the input of the layer's gates.
 *   backward: g (M,128) gradient of y[nl-1]; wT[l] (256,128) = [Wt^T ; Wh^T]; th[l] as the forward wrote it; x[l] (M,128) the input of
 *             layer l's gates (plain: x, y[0], ..; adapter form: hx[l]); dth[l] (M,256) gradient of the pre-activations of [T | H];
 *             gout (M,128) gradient of x.  Adapter form (waT != NULL; nl == 4): waT[l] (128,128) = wa[l]^T, dhx[l] (M,128) gradient
 *             of hx[l]. */
int taco_debug_highway_stack_fwd(const float* x, const float* const* wt, const float* const* bt, const float* const* wh,
                                 const float* const* bh, float* const* th, float* const* y, const float* const* wa,
                                 const float* const* rowb, float* const* hx, int M, int nl, int T, void* stream);
int taco_debug_highway_stack_bwd(const float* g, const float* const* wT, const float* const* th, const float* const* x,
                                 float* const* dth, float* gout, const float* const* waT, float* const* dhx, int M, int nl, void* stream);
/* taco_debug_prenet_fwd / _bwd: the fields of PrenetArgs (csrc/kernels.h).  keep1 (M,256), keep2 (M,128): uint8 0 / 1 keep masks of
 * the two dropout layers, both nullable (no dropout; a kept unit is scaled by 2).
 *   forward : x (M,256); w1 (256,256), b1 (256), w2 (256,128), b2 (128) (biases nullable); y1 (M,256), y2 (M,128) after ReLU and dropout.
 *   backward: dy2 (M,128) gradient of y2; w2T (128,256) = w2^T, w1T (256,256) = w1^T; y1_in, y2_in the forward's y1, y2;
 *             dz2 (M,128), dz1 (M,256) gradients of the two pre-activations; dx (M,256) gradient of x. */
int taco_debug_prenet_fwd(const float* x, const float* w1, const float* b1, const float* w2, const float* b2, const uint8_t* keep1,
                          const uint8_t* keep2, float* y1, float* y2, int M, void* stream);
int taco_debug_prenet_bwd(const float* dy2, const float* w2T, const float* w1T, const uint8_t* keep1, const uint8_t* keep2,
                          const float* y1_in, const float* y2_in, float* dz2, float* dz1, float* dx, int M, void* stream);

/* ---- op-level debug doors of the GEMM forms only the model reaches (tests/test_gpu_gemm_forms.py) ------------
 * Thin wrappers over the launches model.hip makes for the CBHG's conv bank and the decoder's `d keys` product: each builds its
 * ConvGemmProblem / GemmTnArgs (csrc/kernels.h) exactly as cbhg_fwd, cbhg_bwd and taco_backward build theirs; no kernel of their own.
 * All tensors fp32, row-major, (rows, cols) with the row pitch given (element (m, n) at p[m * ld + n]; operands without a pitch
 * argument are dense).  Conventions of the CBHG-tail doors above: a null operand that is not nullable, a size out of range
 * (rows <= 2^22, columns <= 2^14, T must divide M) or an output whose bytes meet those of another operand returns TACO_EINVAL
 * with a message naming the argument, before anything is enqueued; where the library itself would fall back to another form a
 * door returns TACO_ENOTFOUND with nothing enqueued, so that a test can tell which form ran.  TACO_VERSION did not change with these
 * entry points: detect them by the symbol.
 *
 * taco_debug_conv_bank_pool_fwd: the conv bank with the pooled epilogue (ConvGemmProblem::pool == 1), F problems of ONE launch.
 *   Filter f = 1..F: 'same' conv of width f (pad_l = (f - 1) / 2) of x (M, K; lda) with W[f-1] (f, K, N) dense, bias[f-1] (N, nullable),
 *   ReLU -> bank[:, (f-1) N ..] (nullable: not stored); z = bank * scale * scale_mul + shift (scale, shift (F N));
 *   pool[m] = max(z[m], z[m+1]) inside a sequence of T rows, z[m] on its last row.  pool, bank (M, F N; ldc).
 *   TACO_ENOTFOUND where cbhg_fwd runs the convolutions and taco_debug_bn_maxpool_fwd's launch as two passes (gemm2.hip does not take
 *   the batch: TACO_GEMM2_MIN_TILES, the float4 contract of csrc/gemm2.hip pool_contract).
 * taco_debug_conv_gemm_pool_bwd: one problem with pool == 2: dy = sum_tap shift_tap(A) . W[tap] (A (M, K; lda), W (taps, K, N; ldw)) is
 *   d(pooled); with z = pool_x * scale * scale_mul + shift (pool_x (M, N; ldc) the stored bank activations, scale, shift (N)):
 *   dz[m] = [last row of its sequence or z[m] >= z[m+1]] dy[m] + [not the first and z[m] > z[m-1]] dy[m-1],
 *   C[m] = (pool_x[m] > 0) dz[m] scale scale_mul (C (M, N; ldc)), dgamma[n] += sum_m dz pool_x scale_mul, dbeta[n] += sum_m dz (both (N),
 *   ACCUMULATED into).  TACO_ENOTFOUND where cbhg_bwd takes the two-pass form (TACO_DETERMINISTIC=1, or as above).
 * taco_debug_bn_maxpool_fwd / _bwd: the two-pass twins (elementwise.hip), dense (B T, C), C % 4 == 0, scale_mul = 1 / sqrt(1 + 1e-3)
 *   fixed: y = pool(x gamma scale_mul + beta); dx, dgamma (+=), dbeta (+=) as C, dgamma, dbeta above with dy given.
 * taco_debug_bank_gather: the conv bank's input gradient as ONE reduction (ConvGemmProblem::bank_filters) cut into S chunks of the
 *   (tap, 32-deep k-tile) sequence, each into its own slab, then the slab sum: dx_out (M, N; ldc) += sum_f convT_f(dbank[:, (f-1) K ..])
 *   + residual (M, N; ldr; nullable).  dbank (M, F K; lda); WT[f-1] (f, K, N) dense, the transposed kernel of width f whose tap j reads
 *   the rows shifted by j - ((f - 1) - (f - 1) / 2); slabs: scratch of slab_floats floats.  pad_l as cbhg_bwd passes it,
 *   (F - 1) - (F - 1) / 2.  TACO_ENOTFOUND (nothing written) where cbhg_bwd falls back to the atomic batch below: S < 2, WT[f] not
 *   contiguous behind WT[f-1], N % 4 != 0, K % 32 != 0, fewer than ceil(nit / ceil(nit / S)) M N slab floats, another pad_l, operands
 *   off the float4 contract.
 * taco_debug_conv_gemm_batch_atomic: that fall-back -- the F transposed convolutions as F problems of one launch adding into
 *   dx_out with fp32 atomics (atomic_out), the residual on the f = 1 problem.  dx_out must hold what the sum is added to.
 * taco_debug_conv_gemm_rowbias: C (M, N; ldc) = A (M, K; lda) . W (K, N; ldw) + rowb[m / T] with rowb (M / T, N; bias_stride): the
 *   per-sequence bias of the speaker sites (ConvGemmProblem::bias_stride).
 * taco_debug_gemm_tn_group: n <= 26 weight gradients W[i] (taps, K, N; ldw) += shift(A[i])^T . Y[i] as one launch_gemm_tn_batch call
 *   (every argument a table of n entries); dbias (nullable as a table and per entry): dbias[i][n] += sum_m Y[i][m][n].
 * taco_debug_gemm_tn_strided: `batch` problems of one launch, member z at A + z strideA, Y + z strideY, W + z strideW (floats),
 *   accumulated into W; taps = 1 (the decoder's d keys product: M = T = Td, K = Tt, pad_l = 1). */
int taco_debug_conv_bank_pool_fwd(const float* x, int lda, const float* const* W, const float* const* bias, const float* scale,
                                  const float* shift, float scale_mul, float* pool, float* bank, int ldc, int M, int T, int F, int N, int K,
                                  void* stream);
int taco_debug_conv_gemm_pool_bwd(const float* A, int lda, const float* W, int ldw, const float* pool_x, const float* scale,
                                  const float* shift, float scale_mul, float* C, int ldc, float* dgamma, float* dbeta, int M, int N, int K,
                                  int taps, int T, int pad_l, void* stream);
int taco_debug_bn_maxpool_fwd(const float* x, const float* gamma, const float* beta, float* y, int B, int T, int C, void* stream);
int taco_debug_bn_maxpool_bwd(const float* x, const float* gamma, const float* beta, const float* dy, float* dx, float* dgamma,
                              float* dbeta, int B, int T, int C, void* stream);
int taco_debug_bank_gather(const float* dbank, int lda, const float* const* WT, const float* residual, int ldr, float* dx_out, int ldc,
                           float* slabs, int64_t slab_floats, int M, int T, int F, int K, int N, int pad_l, int S, void* stream);
int taco_debug_conv_gemm_batch_atomic(const float* dbank, int lda, const float* const* WT, const float* residual, int ldr, float* dx_out,
                                      int ldc, int M, int T, int F, int K, int N, void* stream);
int taco_debug_conv_gemm_rowbias(const float* A, int lda, const float* W, int ldw, const float* rowb, int bias_stride, float* C, int ldc,
                                 int M, int T, int N, int K, void* stream);
int taco_debug_gemm_tn_group(int n, const float* const* A, const int* lda, const float* const* Y, const int* ldy, float* const* W,
                             const int* ldw, float* const* dbias, const int* M, const int* N, const int* K, const int* taps,
                             const int* T, const int* pad_l, void* stream);
int taco_debug_gemm_tn_strided(const float* A, int lda, int64_t strideA, const float* Y, int ldy, int64_t strideY, float* W, int ldw,
                               int64_t strideW, int M, int N, int K, int T, int pad_l, int batch, void* stream);

/* ---- op-level debug doors of the train step's glue kernels (tests/test_gpu_glue_ops.py) ----------------------
 * The memory-bound passes of csrc/elementwise.hip between the GEMMs and the recurrences, each door one launch_* of that file with
 * the caller's stream; no kernel of their own, no launch added to any product path.  Conventions of the doors above: fp32,
 * row-major, dense unless a pitch is given; a null operand that is not nullable, a size out of range (rows <= 2^22, columns
 * <= 2^14, flat counts < 2^31) or an output whose bytes meet another operand's returns TACO_EINVAL with a message naming the
 * argument, before anything is enqueued.  TACO_DETERMINISTIC=1 is read on every call, as in the train step.  Detect by the symbol.
 *
 * taco_debug_embedding: out (rows, width) = table (V, width) [clamp(ids, 0, V - 1)]; width % 4 == 0 (the model: 256 and 16).
 * taco_debug_embedding_bwd: dtable[v] += sum of the rows of dout (rows, width) whose clamped id is v; width % 4 == 0, <= 1024.
 *   min(32, ceil(rows / 256)) row segments that meet in fp32 atomics; ONE segment, plain adds, under TACO_DETERMINISTIC=1.
 * taco_debug_highway_combine: th (M, 256) = [T | H], x, y (M, 128): y = H T + x (1 - T).
 * taco_debug_highway_combine_bwd: dth (M, 256) = [dy (H - x) T (1 - T) | H > 0 ? dy T : 0], dx = dy (1 - T).
 * taco_debug_act_bwd: dz = dy act'(y) over n elements, y the stored OUTPUT of the activation (RELU: y > 0 ? dy : 0; SIGMOID:
 *   dy y (1 - y); TANH: dy (1 - y y)); keep (n bytes, nullable): dz = keep ? 2 dz : 0.  dz == dy (in place) is allowed.
 * taco_debug_affine_act_bwd: pre, dy, dz (M, N), rs = 1 / sqrt(1 + 1e-3): dgamma[n] += sum_m dy pre rs, dbeta[n] += sum_m dy (fp32
 *   atomics, one per row chunk; one chunk under TACO_DETERMINISTIC=1), dz = dy gamma rs, 0 where act == TACO_ACT_RELU and
 *   !(pre > 0); act NONE or RELU.
 * taco_debug_colsum_batched: out (B, N) = sum over t < T of x ((B T), N; ld); overwritten.
 * taco_debug_mask_rows: y (B, T, C) = x where t < len[b], else 0; C % 4 == 0.
 * taco_debug_center_rows: n = clamp(len[b], 1, T): out[b, s] = x[b, s] - mean over s' < n of x[b, s'] for s < n, else 0; C % 4 == 0.
 * taco_debug_mask_pos: in place g[r][c] = y[r][c] > 0 ? scale g[r][c] : 0 for c < cols; g (rows, cols; ldg), y (rows, cols; ldy).
 * taco_debug_zero_tail_rows: rows t >= len[b] of x0 (B, Td, C0) and, when given, x1 (B, Td, C1) become 0 in place.
 * taco_debug_add: y = a + b over n elements.
 * taco_debug_l1_loss: the loss as taco_forward forms it.  Term i = 0, 1 (a_i, b_i (M_i, N_i); both null: the term is 0):
 *   parts[512 i ..] = 512 block partials of sum |a - b| (blocks without rows write 0), grad_i (M_i, N_i; ldg_i; nullable) =
 *   sign(a - b), 0 at a == b and in the pad columns [N_i, ldg_i); then loss[1], loss[2] = ordered sums of the partials, loss[0] =
 *   their sum, out (3, nullable) = {loss[0], loss[1], loss[2]}.  parts holds 1024 floats, loss 3.
 * taco_debug_transpose_batch: n <= 96 jobs of one launch: out[i] (taps, N, K; ldo) = the transposes of in[i] (taps, K, N; ldi) with
 *   the taps REVERSED (out tap t = in tap taps - 1 - t).  ldi / ldo: null tables or 0 = dense; a pitched job has taps == 1.
 * taco_debug_sumsq: out[0 .. 256) = per-block partial sums of x[i]^2 over n elements (x 16-byte aligned); taco_clip_adam_step adds
 *   them in order and takes the root. */
int taco_debug_embedding(const float* table, const int32_t* ids, float* out, int rows, int V, int width, void* stream);
int taco_debug_embedding_bwd(const float* dout, const int32_t* ids, float* dtable, int rows, int V, int width, void* stream);
int taco_debug_highway_combine(const float* th, const float* x, float* y, int M, void* stream);
int taco_debug_highway_combine_bwd(const float* th, const float* x, const float* dy, float* dth, float* dx, int M, void* stream);
int taco_debug_act_bwd(const float* y, const float* dy, const uint8_t* keep, float* dz, int64_t n, int act, void* stream);
int taco_debug_affine_act_bwd(const float* pre, const float* gamma, const float* dy, float* dz, float* dgamma, float* dbeta, int M,
                              int N, int act, void* stream);
int taco_debug_colsum_batched(const float* x, int ld, float* out, int B, int T, int N, void* stream);
int taco_debug_mask_rows(const float* x, const int32_t* len, float* y, int B, int T, int C, void* stream);
int taco_debug_center_rows(const float* x, const int32_t* len, float* out, int B, int T, int C, void* stream);
int taco_debug_mask_pos(float* g, int ldg, const float* y, int ldy, int rows, int cols, float scale, void* stream);
int taco_debug_zero_tail_rows(float* x0, int C0, float* x1, int C1, const int32_t* len, int B, int Td, void* stream);
int taco_debug_add(const float* a, const float* b, float* y, int64_t n, void* stream);
int taco_debug_l1_loss(const float* a0, const float* b0, float* grad0, int ldg0, int M0, int N0, const float* a1, const float* b1,
                       float* grad1, int ldg1, int M1, int N1, float* parts, float* loss, float* out, void* stream);
int taco_debug_transpose_batch(int n, const float* const* in, float* const* out, const int* taps, const int* K, const int* N,
                               const int* ldi, const int* ldo, void* stream);
int taco_debug_sumsq(const float* x, int64_t n, float* out, void* stream);

/* ---- model level ---------------------------------------------------------------------------------------- */
/* Tacotron.inference with train=True (tacotron.py:107-154) + add_loss_op (tacotron.py:156-165).
 *   text (B,Tt) int32; text_length (B) int32; mel (B,Td,80r); stft (B,Td,1025r);
 *   speaker (B) int32 speaker ids, used (and required) only when shape->S > 1 (tacotron.py:117-124, ops.py:101-115);
 *   masks (uint8 0/1, nullable = no dropout / no sampling):
 *     enc_keep1 (B,Tt,256), enc_keep2 (B,Tt,128)  encoder pre_net dropout keep masks (tacotron.py:128)
 *     dec_keep1 (B,Td,256), dec_keep2 (B,Td,128)  decoder pre_net dropout keep masks (tacotron.py:64-71)
 *     sample (Td,B): 1 => step t+1 of row b is fed cell_output[t] (ScheduledOutputTrainingHelper, tacotron.py:84-85)
 *   outputs: seq2seq_output (B,Td,80r), output (B,Td,1025r), alignments (B,Td,Tt), loss[3] = {total, seq2seq, output}. */
int taco_forward(const TacoShape* shape, const float* params, const int32_t* text, const int32_t* text_length,
                 const int32_t* speaker, const float* mel, const float* stft, const uint8_t* enc_keep1, const uint8_t* enc_keep2,
                 const uint8_t* dec_keep1, const uint8_t* dec_keep2, const uint8_t* sample, float* seq2seq_output,
                 float* output, float* alignments, float* loss, void* workspace, void* stream);

/* Gradient of loss w.r.t. every parameter (opt.compute_gradients, tacotron.py:172), after taco_forward on the same
 * workspace with the same PARAMETERS, inputs and masks (taco_forward also leaves the transposed weight copies the
 * backward pass reads in the workspace).  seq2seq_output and alignments are the tensors taco_forward produced.
 * grads has taco_param_count floats and is overwritten. */
int taco_backward(const TacoShape* shape, const float* params, const int32_t* text, const int32_t* text_length,
                  const int32_t* speaker, const float* seq2seq_output, const float* alignments, const uint8_t* enc_keep1,
                  const uint8_t* enc_keep2, const uint8_t* dec_keep1, const uint8_t* dec_keep2, const uint8_t* sample,
                  float* grads, void* workspace, void* stream);

/* Tacotron.inference with train=False (test.py:29, ops.InferenceHelper ops.py:5-25): zeros first frame, feeds back
 * its own output, always Td steps, no dropout.  mel/stft/loss absent. */
int taco_infer(const TacoShape* shape, const float* params, const int32_t* text, const int32_t* text_length,
               const int32_t* speaker,
               float* seq2seq_output, float* output, float* alignments, void* workspace, void* stream);

/* Inference end detection (no reference counterpart: the reference always decodes Td steps and Tacotron 1 has no stop token; the
 * signal is the attention reaching the last characters and staying there).  All three parameters are integers, so that the device
 * and a host restatement agree exactly.  For row b with text length L (clamped to 1..Tt) and alignments a[t, :] of step t:
 *   target = max(0, L - 1 - end_offset);  a_t = first index of the maximum of a[t, 0:Tt] (lowest index on ties, as np.argmax);
 *   run_t = (a_t >= target) ? run_{t-1} + 1 : 0, run_{-1} = 0;  t* = the first t with run_t >= hold and t + 1 >= min_steps;
 *   len_b = min(Td, 4 ceil((t* + 1) / 4)), or Td if there is no such t.
 * len_b is a multiple of 4 steps (or Td) because the r-frame layout (audio.reshape_frames, audio.py:22-35) interleaves blocks of
 * 4 decoder steps: cut inside a block, the chronological frames of taco_denorm_unframe would have holes.
 * Valid rules: end_offset >= 0, hold >= 1, min_steps >= 1 (min_steps = Td + 1 is valid and never fires).  `reserved`: 0. */
typedef struct TacoStopRule {
  int32_t end_offset;
  int32_t hold;
  int32_t min_steps;
  int32_t reserved;
} TacoStopRule;

/* Tacotron inference as taco_infer, with the end detection above.  Same workspace (train = 0) and output shapes; rule is a HOST
 * pointer, lengths (B) int32 a device pointer that receives len_b.
 *   - rows t < len_b of seq2seq_output and alignments are bit-identical to what taco_infer computes from the same inputs;
 *   - rows t >= len_b of seq2seq_output, alignments and output are exactly 0;
 *   - output is the post-net and final dense of the zero-filled seq2seq_output over all Td steps (the post-net's convolutions and
 *     backward GRU reach past len_b), cleared from len_b on.
 * The default decoder (decoder3.hip) evaluates the rule inside its step loop: each cluster of rows stops after the step of its
 * longest row.  decoder.hip (taco_decoder_mode 2, and shapes decoder3.hip does not cover) decodes all Td steps and the rule then
 * runs over its alignments: the same results, no time saved.  A NULL rule or lengths, or a rule outside the valid range, returns
 * TACO_EINVAL before anything is enqueued.  Graph-capturable, as taco_infer. */
int taco_infer_stop(const TacoShape* shape, const float* params, const int32_t* text, const int32_t* text_length,
                    const int32_t* speaker, const TacoStopRule* rule, float* seq2seq_output, float* output, float* alignments,
                    int32_t* lengths, void* workspace, void* stream);

/* Alignment scores: per utterance, how the attention read its text (the role of the attention picture the reference sends to
 * TensorBoard, train.py:92-103 and test.py:60-69, as numbers that stay on the device).  Built on the stop rule's argmax walk.
 *   alignments  (B, Td, Tt) as taco_forward, taco_infer or taco_infer_stop write them
 *   text_length (B) int32;  steps (B) int32 on the DEVICE, or NULL: the `lengths` of taco_infer_stop;  max_jump >= 0
 *   counts (B, 6) int32 and means (B, 2) fp32, both required
 * For row b:  L = clamp(text_length[b], 1, Tt);  n = Td when steps is NULL, else clamp(steps[b], 0, Td).  For every scored step
 * t < n, a_t is the lowest index s < Tt at which a[t, s] equals the maximum of the step's non-NaN elements, and 0 when every
 * element is NaN -- for a step without NaN the stop rule's a_t, lowest index on ties -- and p_t = a[t, a_t].
 *   counts[b] = { n,
 *                 end       = max_t a_t, 0 when n == 0,
 *                 pad_steps = #{t : a_t >= L},
 *                 back      = #{1 <= t < n : a_t < a_{t-1}},
 *                 skip      = #{1 <= t < n : a_t > a_{t-1} + max_jump},
 *                 covered   = #{s < L : a_t == s for some t < n} }
 *   means[b]  = { focus    = (1 / n) sum_t p_t,
 *                 pad_mass = (1 / n) sum_t sum_{s >= L} a[t, s] },  both 0 when n == 0
 * The means are fp32 sums in a fixed order (the same arguments give the same bits); a NaN among their terms makes them NaN,
 * the counts are defined for any input.  Rows t >= n and every other row's data have no influence on row b.
 * One launch of B workgroups, each keeping its row's a_t in LDS: no workspace, no allocation, no host synchronisation, no
 * workgroup waits for another one; graph-capturable.  Nothing outside counts and means is written; alignments needs the
 * alignment of a float only (16-byte loads are used when Tt % 4 == 0 and the base allows).  The LDS record holds
 * TACO_ALIGNMENT_MAX_TD steps and the bitmap behind `covered` TACO_ALIGNMENT_MAX_TT characters.  NULL alignments / text_length /
 * counts / means, B, Td or Tt <= 0, max_jump < 0, Td > TACO_ALIGNMENT_MAX_TD or Tt > TACO_ALIGNMENT_MAX_TT return TACO_EINVAL before
 * anything is enqueued.  TACO_VERSION did not change with this entry point: detect it by the symbol. */
#define TACO_ALIGNMENT_MAX_TD 16384
#define TACO_ALIGNMENT_MAX_TT 16384
int taco_alignment_scores(const float* alignments, const int32_t* text_length, const int32_t* steps, int max_jump,
                          int32_t* counts, float* means, int B, int Td, int Tt, void* stream);

/* Alignment path: per utterance, the best MONOTONE path through the attention matrix -- which character each decoder step speaks,
 * and from it how many steps each character lasts.  taco_alignment_scores' argmax walk may go back and skip; a timing cannot be
 * read off it.  No counterpart in the reference.
 *   alignments, text_length, steps: exactly as taco_alignment_scores takes them (steps on the DEVICE, or NULL)
 *   1 <= max_jump <= TACO_ALIGN_PATH_MAX_JUMP: how many characters a step may advance
 *   path (B, Td) int32, dur (B, Tt) int32, counts (B, 3) int32, mass (B) fp32: all required, every element of each is written
 *   workspace: taco_alignment_path_workspace_bytes(B, Td, Tt) bytes, arbitrary contents (NULL allowed when that is 0)
 * For row b:  L = clamp(text_length[b], 1, Tt);  n = Td when steps is NULL, else clamp(steps[b], 0, Td);  J = max_jump.  The
 * criterion is the attention MASS on the path, not its log-probability: a sum of fp32 values, one addition per cell, so a NumPy
 * float32 restatement gives the same bits, and the exactly-zero rows behind a stop need no floor.
 *   1. weights       w(t, s) = a[t, s] if a[t, s] > 0, else +0 (NaN, negative values and -0 give +0)
 *   2. start         the path starts on character 0:  Q(0, 0) = w(0, 0)
 *   3. reachability  cell (t, s) is reachable iff s <= min(L - 1, J t)
 *   4. recurrence    for a reachable cell with t >= 1 the predecessor is (t-1, s-d), d the SMALLEST d in 0 .. min(J, s) at which
 *                    Q(t-1, s-d) is largest among the reachable candidates;  Q(t, s) = w(t, s) + Q(t-1, s-d), one fp32 addition
 *                    rounded to nearest even
 *   5. end           free: e = the lowest s at which Q(n-1, s) is largest;  mass[b] = Q(n-1, e)
 *   6. path          path[b, n-1] = e,  path[b, t-1] = path[b, t] - d(t, path[b, t]);  path[b, t] = -1 for t >= n
 *   7. durations     dur[b, s] = #{t < n : path[b, t] == s} for every s < Tt (0 for skipped characters, for s > e and for s >= L)
 *   8. counts        counts[b] = { n, e, skipped = #{s <= e : dur[b, s] == 0} }
 *   9. empty row     n == 0: path all -1, dur all 0, counts {0, 0, 0}, mass +0
 * Defined for every input, +inf included (no NaN arises from sums of non-negative values).  Steps t >= n, characters s >= L and
 * every other row's data have no influence on row b; the same arguments give the same bits.
 * One launch of B workgroups: no allocation, no host synchronisation, no workgroup waits for another one; graph-capturable.
 * Nothing outside path / dur / counts / mass / workspace is written; alignments needs the alignment of a float only.  The
 * workspace holds the direction table (a byte per cell) of the shapes whose table does not fit LDS; it is 0 bytes for Tt <= 256
 * at the decoder lengths the product uses.  Any of the five required pointers NULL, a NULL workspace where one is needed, B, Td
 * or Tt <= 0, Td > TACO_ALIGN_PATH_MAX_TD, Tt > TACO_ALIGN_PATH_MAX_TT or max_jump outside 1 .. TACO_ALIGN_PATH_MAX_JUMP return
 * TACO_EINVAL before anything is enqueued; the size function returns TACO_EINVAL for the same shapes.  TACO_VERSION did not
 * change with these entry points: detect them by the symbol. */
#define TACO_ALIGN_PATH_MAX_TD   16384
#define TACO_ALIGN_PATH_MAX_TT   4096
#define TACO_ALIGN_PATH_MAX_JUMP 15
int64_t taco_alignment_path_workspace_bytes(int B, int Td, int Tt);
int taco_alignment_path(const float* alignments, const int32_t* text_length, const int32_t* steps, int max_jump,
                        int32_t* path, int32_t* dur, int32_t* counts, float* mass, void* workspace,
                        int B, int Td, int Tt, void* stream);

/* ---- held-out evaluation: frame distance over a dynamic-time-warping path ------------------------------------------------- */
/* Frames in use: x (B, F, C) chronological frames (taco_denorm_unframe's spec).  n[b] = 1 + the last f with x[b, f, c] > floor for
 * some c, and 0 when there is none; a NaN compares false.  The corpus pads every recording with frames of exactly log(1e-8) and
 * stores no frame count, so the recorded length is read off the frames.  One launch of B workgroups, no workspace, no allocation,
 * no host synchronisation; graph-capturable.  NULL x / n or B, F, C <= 0 return TACO_EINVAL before anything is enqueued. */
int taco_frames_active(const float* x, float floor, int32_t* n, int B, int F, int C, void* stream);

/* Dynamic time warping of two frame sequences per batch row (the warp behind mel-cepstral distortion, MCD-DTW).
 *   a (B, Fa, C), b (B, Fb, C) fp32 chronological frames;  na, nb (B) int32 on the DEVICE, or NULL: Fa / Fb; used clamped to
 *   [0, Fa] / [0, Fb];  basis (K, C) fp32, or NULL: K == C and the coefficients are the channels themselves;
 *   cost (B) fp32 and steps (B) int32, both required;  workspace: taco_frame_dtw_workspace_bytes(B, Fa, Fb, K) bytes, arbitrary
 *   contents (NULL allowed when that is 0).
 * Exact semantics -- every operation below is ONE fp32 operation rounded to nearest even, nothing is fused, denormals are kept, so a
 * NumPy float32 restatement gives the same bits:
 *   1. coefficients  u[i, k] = sum_c basis[k, c] * a[b, i, c]: acc = +0, then for c = 0 .. C-1 acc = acc + (basis[k, c] * a[b, i, c]);
 *      v[j, k] likewise from b.  With basis NULL u[i, k] = a[b, i, k].
 *   2. local distance  d(i, j) = sqrt(s), s = +0, then for k = 0 .. K-1  t = u[i, k] - v[j, k];  s = s + (t * t);  sqrt correctly rounded.
 *   3. recurrence  D[0][0] = d(0, 0), N[0][0] = 1.  Otherwise the predecessor is the candidate of smallest D among (i-1, j-1),
 *      (i-1, j), (i, j-1), those inside the table only; on equal D the earliest in that order wins;
 *      D[i][j] = D[pred] + d(i, j), N[i][j] = N[pred] + 1.
 *   4. results  cost[b] = D[na-1][nb-1], steps[b] = N[na-1][nb-1] (the cells on the chosen path); both 0 when na == 0 or nb == 0.
 * Frames i >= na and j >= nb and every other row's data have no influence on row b.  With non-finite inputs the results are
 * unspecified, but the launch ends and writes nothing outside cost / steps / workspace.
 * One launch, a workgroup per row walking the anti-diagonals i + j = const with the three live diagonals of (D, N) in LDS; the
 * coefficients are computed once per row, into LDS where they fit beside the diagonals (160 KiB) and else into the row's slice of
 * `workspace`.  The Fa x Fb table is never materialised.  No allocation, no host synchronisation, no workgroup waits for another
 * one; graph-capturable; the same arguments give the same bits.
 * The warping path itself: taco_frame_dtw_path below (it needs a direction table in the workspace; this entry point keeps none).
 * NOT provided: a Sakoe-Chiba band (every cell is visited).
 * NULL a / b / cost / steps, B, Fa, Fb, C or K <= 0, basis == NULL with K != C, K > TACO_DTW_MAX_K, C > TACO_DTW_MAX_C, Fa or Fb >
 * TACO_DTW_MAX_FRAMES, or a NULL workspace where one is needed return TACO_EINVAL before anything is enqueued; the size function
 * returns TACO_EINVAL for the same shapes.  TACO_VERSION did not change with these entry points: detect them by the symbol. */
#define TACO_DTW_MAX_FRAMES 1024
#define TACO_DTW_MAX_K 32
#define TACO_DTW_MAX_C 128
int64_t taco_frame_dtw_workspace_bytes(int B, int Fa, int Fb, int K);
int taco_frame_dtw(const float* a, const int32_t* na, const float* b, const int32_t* nb, const float* basis, float* cost,
                   int32_t* steps, void* workspace, int B, int Fa, int Fb, int C, int K, void* stream);

/* The same warp with its path.  a, na, b, nb, basis, cost, steps: exactly as taco_frame_dtw takes them, with the same limits;
 * steps 1-4 above with the same tie order, and cost / steps have the same BITS as taco_frame_dtw's on the same inputs.
 *   path_a, path_b (B, P) int32, P = Fa + Fb - 1, both required: entries t = 0 .. steps[b]-1 of row b hold the cells (i_t, j_t) of
 *   the chosen path in chronological order -- (i_0, j_0) = (0, 0), the last one (na-1, nb-1), (i_{t-1}, j_{t-1}) the predecessor
 *   step 3 chose for (i_t, j_t) -- and entries t >= steps[b] hold -1 (the whole row when na or nb is 0).  Every element of both
 *   is written.
 *   workspace: taco_frame_dtw_path_workspace_bytes(B, Fa, Fb, K) bytes, required (never 0), 4-byte aligned, arbitrary contents:
 *   the coefficients where taco_frame_dtw keeps them there, then per row a direction table of one byte per cell, stored by
 *   anti-diagonal: (Fa + Fb - 1) Fa bytes a row (253 KiB at 360 x 360, 2 MiB at 1024 x 1024).
 * One launch, a workgroup per row: the walk of taco_frame_dtw storing one direction byte per cell, then the path read off the table
 * backwards by one lane (one dependent load per step), each entry written in its final place, while the whole workgroup fills the
 * tails.  Measured on an MI355X (profiles/frame_dtw_path_timing.json): 1.09 x the cost-only call at 32 x 360 x 360, K = 13, 1.12 x
 * at 32 x 1000 x 1000; 0.17 us per step of the backtrack.  No allocation, no host synchronisation, no workgroup waits for another
 * one; graph-capturable; the same arguments give the same bits.  Nothing outside cost / steps / path_a / path_b / workspace is
 * written, also with non-finite inputs (whose results are unspecified).  No Sakoe-Chiba band.
 * Every refusal of taco_frame_dtw, NULL path_a / path_b and a NULL workspace return TACO_EINVAL (message "frame_dtw_path: ...")
 * before anything is enqueued; the size function returns TACO_EINVAL for the shapes taco_frame_dtw_workspace_bytes refuses.
 * TACO_VERSION did not change with these entry points: detect them by the symbol. */
int64_t taco_frame_dtw_path_workspace_bytes(int B, int Fa, int Fb, int K);
int taco_frame_dtw_path(const float* a, const int32_t* na, const float* b, const int32_t* nb, const float* basis, float* cost,
                        int32_t* steps, int32_t* path_a, int32_t* path_b, void* workspace, int B, int Fa, int Fb, int C, int K,
                        void* stream);

/* add_train_op (tacotron.py:167-185): global-norm clip (cap_grads) then TF-form Adam, in place.
 *   step = global_step after this update (1-based).  scratch: >= 256 floats.  gnorm_out[0] receives ||g||. */
int taco_clip_adam_step(float* params, const float* grads, float* m, float* v, int64_t n, float lr, float cap,
                        int64_t step, float* scratch, float* gnorm_out, void* stream);

/* Same, guarded: err_words (nullable) points at the two int32 decoder error words of the workspace (tensor "dec.err" of
 * taco_workspace_table: [0] forward, [1] backward).  The persistent decoder kernels exchange data between workgroups with
 * bounded spins; a time-out (workgroups not co-resident on a busy GPU) sets a word and the launch drains with garbage
 * gradients.  When either word is non-zero the update is skipped and gnorm_out[0] = -1.  The words are STICKY: only
 * taco_clear_error resets them (call it once on a fresh workspace, and after handling an error).
 * scratch: >= 256 floats (per-block partial sums of squares, summed in a fixed order: the norm is reproducible). */
int taco_clip_adam_step_guarded(float* params, const float* grads, float* m, float* v, int64_t n, float lr, float cap,
                                int64_t step, float* scratch, float* gnorm_out, const int32_t* err_words, void* stream);
int taco_clear_error(const TacoShape* shape, int train, void* workspace, void* stream);

/* Process-wide decoder mode.  The default persistent decoder kernels (decoder3.hip) exchange data between the 32 workgroups of
 * a cluster through granules that are published with WORKGROUP-scope stores and read with L1-bypassing agent-scope loads when
 * the whole cluster sits on one XCD (verified at kernel start from HW_REG_XCC_ID).  That is faster than the placement-
 * independent agent-scope form (0.21 vs 0.37 us per hop) but leans on gfx942 / gfx950 implementation behaviour: a write-through
 * L1 and one L2 per XCD shared by its CUs.  Granules are epoch-tagged, so a stale read can only delay or time out, never
 * corrupt; a time-out sets the sticky error word (taco_clip_adam_step_guarded).
 *   mode 0 (default)  decoder3.hip, XCD-local exchange where placement allows
 *   mode 1            decoder3.hip, agent-scope exchange only (environment TACO_DEC_V3_AGENT=1)
 *   mode 2            decoder.hip (round-1/2 kernels: one cluster of 8-16 workgroups per batch row; environment TACO_DEC_V3=0)
 * taco_decoder_mode(mode) sets the mode (mode < 0: query only) and returns the previous one.  The Python host escalates
 * 0 -> 1 -> 2 when Tacotron.check() finds an error word set, so a box where the fast form misbehaves degrades instead of
 * skipping every update. */
int taco_decoder_mode(int mode);

/* ---- data-parallel overlap (no reference counterpart: train.py:24 is a single Session) ---------------- */
/* The flat gradient buffer becomes final in FIVE contiguous segments, in this order during taco_backward:
 *   segment 4 = [bounds[4], bounds[5])  post-net CBHG + final dense   (final before the decoder BPTT; ANNOUNCED right after it)
 *   segment 3 = [bounds[3], bounds[4])  attention memory layer + decoder
 *   segment 2 = [bounds[2], bounds[3])  encoder CBHG without its conv bank: projections, highways, bi-GRU
 *   segment 1 = [bounds[1], bounds[2])  encoder conv bank   (behind its grouped weight-gradient launch, the last big one of the pass)
 *   segment 0 = [bounds[0], bounds[1])  embedding(s) + encoder pre_net   (end of taco_backward)
 * taco_grad_segments fills bounds[6] (float offsets) and returns 5 (version 117 and earlier: four segments, the conv bank in
 * segment 0).  taco_wait_grad_segment makes `stream` wait (device
 * side, hipStreamWaitEvent) until segment `seg` of the most recent taco_backward enqueued by the calling thread on the
 * current device is final, so an all-reduce enqueued on `stream` afterwards overlaps the rest of the backward pass.
 * Segment 4 is announced AFTER the decoder BPTT kernel although it is final before it: that kernel is a persistent launch
 * whose 256 workgroups must all be co-resident (one per CU), so no collective is ever allowed to compete with it for CUs;
 * segments 4 and 3 (13.7 MB) travel under the encoder backward, segment 2 (4.7 MB) under the encoder conv-bank gradients,
 * segment 1 (8.9 MB) under the step's tail (bank input gradient, pre_net chain, embedding scatter: ~0.1 ms), and only
 * segment 0 (0.5 MB) is exposed in full. */
int taco_grad_segments(const TacoShape* shape, int64_t* bounds);
int taco_wait_grad_segment(int seg, void* stream);
/* Communication-kernel stand-in for the co-residency tests (tests/test_gpu_dist.py): `blocks` workgroups x `threads` threads, `lds_bytes` of LDS each, spinning
 * for `usec` microseconds.  Does no work. */
int taco_debug_spin(int blocks, int threads, int lds_bytes, int usec, void* stream);

/* Shader-clock probe: one 512-thread workgroup per CU, every wave a chain of `iters` dependent FMAs; out3[0] = elapsed shader
 * cycles, out3[1] = elapsed ticks of the constant 100 MHz counter of workgroup 0 (device int64[3]).  cycles / (ticks * 10 ns) =
 * the clock the chip sustains under a chip-wide latency-bound load, which is what the persistent decoder / bi-GRU kernels scale
 * with (boxes of one pool were measured ~10 % apart on those kernels). */
int taco_debug_clock_probe(long long* out3, int iters, void* stream);

/* Fabric probe: the latencies the persistent decoder / bi-GRU kernels wait on, measured on the box at hand (bench.py `box`).
 * One launch of 64 small workgroups; out32 (device int64[32], zeroed by the caller) receives, in ticks of the 100 MHz counter,
 * the total of `iters` round trips of a granule ping-pong between two workgroups of ONE XCD with workgroup-scope stores [0]
 * (decoder3.hip's exchange) and agent-scope stores [1], between two XCDs [2] (decoder.hip's exchange), of `iters` dependent loads
 * that hit the L2 [3] / agent-scope loads of cold lines anywhere in the scratch buffer [4], and the time
 * one workgroup needs to stream 8 MB [5]; [6] = iters, [7] = ok bits, [8 + b] = XCC id of workgroup b < 24.
 * gran4k: 4 KiB of zeroed device memory; scratch: zeroed device memory, scratch_bytes >= 32 MiB.  No counterpart in the reference. */
int taco_debug_fabric_probe(long long* out32, void* gran4k, const void* scratch, long long scratch_bytes, int iters, void* stream);

/* ---- spectrogram boundary ---------------------------------------------------------------------------- */
/* test.py:64 `out * stft_std + stft_mean` followed by audio.reshape_frames(forward=False) (audio.py:29-35), on the device.
 *   output (B, Td, r*C) as produced by taco_infer (C = 1025 linear bins, or 80 for mel frames); stft_mean / stft_std (r*C)
 *   spec  (B, F, C), nullable: chronological, de-normalised log-magnitude frames, F = (Td / 4) * 4 * r
 *   mag_t (B, C, F), nullable: exp(spec) transposed -- the matrix audio.invert_spectrogram (audio.py:69-72) gives Griffin-Lim */
int taco_denorm_unframe(const float* output, const float* stft_mean, const float* stft_std, float* spec, float* mag_t,
                        int B, int Td, int r, int C, void* stream);

/* Speaking rate at synthesis (no reference counterpart: the reference speaks at the rate its model learned).  Between
 * taco_denorm_unframe and Griffin-Lim an utterance is a magnitude matrix with no phase attached; resampling it along the frame axis
 * changes the duration, and Griffin-Lim then finds phases consistent with the new length, so the pitch does not move.
 *   mag_t  (B, C, F) fp32 and out (B, C, Fo) fp32, the frame index contiguous (the layout of taco_denorm_unframe's mag_t)
 *   frames (B) int32 on the DEVICE, or NULL: F_b = clamp(frames[b] * frames_per_unit, 0, F), the product formed in 64 bits; NULL:
 *          F_b = F.  frames_per_unit >= 1 is required either way (pass r with the lengths of taco_infer_stop)
 *   step_q (B) int32 on the DEVICE, or NULL: the source frames advanced per output frame in units of 2^-16 -- the rate as an
 *          integer, so that the device and a NumPy restatement agree exactly (the choice TacoStopRule made).  Used as
 *          s_b = clamp(step_q[b], TACO_STRETCH_MIN_STEP, TACO_STRETCH_MAX_STEP); NULL: TACO_STRETCH_ONE.  The host reads nothing
 *          from frames or step_q
 *   frames_out (B) int32, required
 * Per row b, exactly:
 *   Fo_b = 0 when F_b == 0, else min(Fo, ((F_b - 1) << 16) / s_b + 1) in integer division;  frames_out[b] = Fo_b
 *   for j < Fo_b: p = j * s_b, i = p >> 16, w = float(p & 0xFFFF) * 2^-16 (exact in fp32)
 *     w == 0: out[b, k, j] = mag_t[b, k, i] bit for bit, and element i + 1 is NOT read (the last output frame can sit exactly on
 *             source frame F_b - 1)
 *     else:   out[b, k, j] = a + (w * (c - a)), a = mag_t[b, k, i], c = mag_t[b, k, i + 1]: one fp32 subtraction, one multiply and
 *             one addition, each rounded to nearest even, nothing contracted into an FMA -- NumPy float32 gives the same bits.  The
 *             formula for Fo_b guarantees i + 1 <= F_b - 1 here
 *   out[b, k, j] = 0 exactly for Fo_b <= j < Fo
 *   - every element of out and frames_out is written and nothing outside them, for any F, Fo and any alignment of mag_t and out
 *     (one form: 4-byte accesses, 256 contiguous bytes per wave; two forms with 16-byte stores measured no faster and were deleted);
 *   - with s_b = TACO_STRETCH_ONE and Fo >= F_b the first F_b columns are a bit-identical copy;
 *   - columns t >= F_b of mag_t and every other row's data have no influence on row b (they may hold NaN);
 *   - row b of a B-row call equals a B = 1, F = F_b call on a contiguous copy of the row's first F_b columns;
 *   - no atomics: the same arguments give the same bits.
 * One launch of B x ceil(C / 16) x ceil(Fo / 256) workgroups, no workspace, no allocation, no host synchronisation, no workgroup
 * waits for another one: graph-capturable, and a replay follows whatever frames and step_q hold at replay time.  NULL mag_t / out /
 * frames_out, out overlapping mag_t, B, C, F or Fo <= 0, F or Fo > TACO_STRETCH_MAX_FRAMES and frames_per_unit < 1 return
 * TACO_EINVAL, with a message that names the argument, before anything is enqueued.  TACO_VERSION did not change with this entry
 * point: detect it by the symbol.
 * Not here: interpolation of log-magnitudes or of mel frames (a rate that varies inside an utterance: taco_frames_stretch_curve).  Nobody has listened to the result: the
 * limits 0.25 and 4 are bounds of the arithmetic ((frame << 16) and j * s_b stay inside 31 bits), not recommendations. */
#define TACO_STRETCH_ONE        65536     /* step_q of rate 1 */
#define TACO_STRETCH_MIN_STEP   16384     /* rate 0.25: four times slower */
#define TACO_STRETCH_MAX_STEP   262144    /* rate 4 */
#define TACO_STRETCH_MAX_FRAMES 8192      /* F and Fo; keeps (frame << 16) inside 31 bits */
int taco_frames_stretch(const float* mag_t, const int32_t* frames, int frames_per_unit, const int32_t* step_q,
                        float* out, int32_t* frames_out, int B, int C, int F, int Fo, void* stream);

/* Pitch at synthesis (no reference counterpart), the second prosody control beside the speaking rate and in the same place: between
 * taco_denorm_unframe and Griffin-Lim, where a frame is magnitudes without phases.  A warp of the bin axis alone would move the
 * formants with the pitch, so each frame's log-magnitudes are split into a smooth log-envelope (the low quefrencies of the cepstrum)
 * and a log-excitation (the rest, which carries the harmonics); the excitation alone is warped and put back under the unmoved
 * envelope, and Griffin-Lim then finds phases for the harmonics it is given.
 *   mag_t  (B, C, F) fp32 and out (B, C, F) fp32, the frame index contiguous (the layout of taco_denorm_unframe's mag_t);
 *          C - 1 a power of two, 8 <= C - 1 <= 1024; N = 2 (C - 1).  Production: C = 1025; the small C keep tests cheap
 *   frames, frames_per_unit: as taco_frames_stretch: F_b = clamp(frames[b] * frames_per_unit, 0, F), NULL: F_b = F
 *   step_q (B) int32 on the DEVICE, or NULL: source bins advanced per output bin in units of 2^-16 = 65536 / ratio, ratio =
 *          2^(semitones / 12); used as s_b = clamp(step_q[b], TACO_PITCH_MIN_STEP, TACO_PITCH_MAX_STEP); NULL: TACO_PITCH_ONE.
 *          The host reads nothing from frames or step_q
 *   lifter Q, 1 <= Q <= min(TACO_PITCH_MAX_LIFTER, (C - 1) / 2): the quefrencies 0 .. Q make the envelope (rectangular lifter)
 * For frame f < F_b of row b, m[k] = mag_t[b, k, f], in real numbers:
 *   L[k] = log(max(m[k], TACO_PITCH_FLOOR))                                        (the front end's own epsilon)
 *   c[n] = (L[0] + (-1)^n L[C-1] + 2 sum_{k=1..C-2} L[k] cos(2 pi n k / N)) / N,  n = 0 .. Q  (cepstrum of the even extension)
 *   E[k] = c[0] + 2 sum_{n=1..Q} c[n] cos(2 pi n k / N);   R[k] = L[k] - E[k]
 *   p = k * s_b, i = p >> 16, w = (p & 0xFFFF) 2^-16:  R'[k] = R[i] + w (R[i+1] - R[i]) for i < C - 1;  R[C-1] for i == C - 1 and
 *   w == 0;  0 beyond the top bin (there the output is the envelope alone)
 *   out[b, k, f] = exp(E[k] + R'[k])
 * computed in fp32 (logf, expf, a cosine table from cospif, the two cosine products as ordered fmaf chains in a fixed order) and
 * held by the tests to an fp64 restatement within a tolerance sized from a float32 restatement (tests/pitch_ref.py).  Exactly:
 *   - a row with s_b == TACO_PITCH_ONE is copied: out[b, k, f] = mag_t[b, k, f] bit for bit for f < F_b, no log / exp round trip;
 *   - out[b, k, f] = +0 for F_b <= f < F;
 *   - every element of out is written and nothing outside it, for any F and any 4-byte alignment of mag_t and out;
 *   - columns f >= F_b, every other row and every other frame have no influence on a frame (they may hold NaN); a non-finite value
 *     inside a frame leaves unspecified values in that frame only;
 *   - the bits of a frame depend on its own C bins, s_b and Q alone -- not on B, F, its position f or the buffers' alignment; no
 *     atomics; the same arguments give the same bits.
 * One launch of B x ceil(F / 32) workgroups, no workspace, no allocation, no host synchronisation, no workgroup waits for another
 * one: graph-capturable, and a replay follows whatever frames and step_q hold at replay time.  NULL mag_t / out, out overlapping
 * mag_t, B or F <= 0, F > TACO_STRETCH_MAX_FRAMES, C - 1 not a power of two in 8 .. 1024, lifter out of range and
 * frames_per_unit < 1 return TACO_EINVAL, with a message that names the argument, before anything is enqueued.  TACO_VERSION did
 * not change with this entry point: detect it by the symbol.
 * Not here: a tapered or caller-supplied lifter, mel frames (a pitch contour inside an utterance: taco_frames_pitch_curve).  Nobody has listened to the
 * result: the default lifter of the Python layer (32: quefrencies up to 2 ms at 16 kHz) is untuned, and the limits of +-12
 * semitones are bounds of the arithmetic (k * s_b <= 2^27), not recommendations. */
#define TACO_PITCH_ONE        65536     /* step_q of 0 semitones */
#define TACO_PITCH_MIN_STEP   32768     /* +12 semitones */
#define TACO_PITCH_MAX_STEP   131072    /* -12 semitones */
#define TACO_PITCH_MAX_LIFTER 64
#define TACO_PITCH_FLOOR      1e-8f     /* audio.py:59 */
int taco_frames_pitch(const float* mag_t, const int32_t* frames, int frames_per_unit, const int32_t* step_q, int lifter,
                      float* out, int B, int C, int F, void* stream);

/* Timbre at synthesis (no reference counterpart), the dual of taco_frames_pitch in the same place: the envelope (the formants, the
 * apparent vocal-tract length) moves along the bin axis and the harmonics stay where they are.  Every argument exactly as
 * taco_frames_pitch: mag_t, out (B, C, F) fp32 with the frame index contiguous, C - 1 a power of two in 8 .. 1024; frames,
 * frames_per_unit and F_b; step_q (B) int32 on the DEVICE or NULL, s_b = clamp(step_q[b], TACO_PITCH_MIN_STEP, TACO_PITCH_MAX_STEP),
 * NULL: TACO_PITCH_ONE, step_q = 65536 / ratio with ratio = 2^(semitones / 12) -- a ratio above 1 moves the formants UP; lifter Q in
 * 1 .. min(TACO_PITCH_MAX_LIFTER, (C - 1) / 2).  The host reads nothing from frames or step_q.
 * For frame f < F_b of row b, m[k] = mag_t[b, k, f], in real numbers:
 *   L[k], c[n] (n = 0 .. Q), E[k]          exactly as taco_frames_pitch defines them (floor TACO_PITCH_FLOOR, rectangular lifter)
 *   p = k * s_b, i = p >> 16, w = (p & 0xFFFF) 2^-16
 *   E'[k] = E[i] + w (E[i+1] - E[i])       for i < C - 1;  E[C-1] otherwise (the envelope is held beyond the top bin)
 *   y[k]  = m[k] exp(E'[k] - E[k])         (m, not max(m, floor): a zero bin stays exactly zero)
 *   P0 = sum_k m[k]^2, P1 = sum_k y[k]^2   (plain sums, k = 0 .. C - 1);  g = sqrt(P0 / P1), and 1 when P1 == 0
 *   out[b, k, f] = y[k] g
 * so the log-excitation L - E of every bin at or above the floor is unchanged, the envelope is the input's read at k / ratio, and
 * the frame energy is the input's, as in taco_frames_sharpen.  Computed in fp32 with the cepstrum and envelope chains of
 * taco_frames_pitch (the same fp32 cepstra and envelope) and held to an fp64 restatement (tests/formant_ref.py).  Exactly:
 *   - a row with s_b == TACO_PITCH_ONE is copied bit for bit for f < F_b, no log / exp round trip;
 *   - out[b, k, f] = +0 for F_b <= f < F;
 *   - every element of out is written and nothing outside it, for any 4-byte alignment of mag_t and out;
 *   - columns behind F_b, other rows and other frames have no influence on a frame (they may hold NaN);
 *   - the bits of a frame depend on its own C bins, s_b and Q alone -- not on B, F, its position or the buffers' alignment; no
 *     atomics; the same arguments give the same bits; row b of a B-row call equals the call on that row alone.
 * One launch of B x ceil(F / 32) workgroups, no workspace, no allocation, no host synchronisation: graph-capturable, and a replay
 * follows whatever frames and step_q hold at replay time.  The refusals of taco_frames_pitch: NULL mag_t / out, out overlapping
 * mag_t, a bad B, C, F or frames_per_unit and lifter out of range return TACO_EINVAL with a message that names the argument, before
 * anything is enqueued.  TACO_VERSION did not change with this entry point: detect it by the symbol.
 * Not here: a per-frame or per-word formant curve, a fused pitch + formant launch that shares one cepstrum, mel frames, a tapered
 * lifter.  Nobody has listened to the result: the default lifter of the Python layer (32) is untuned, and the limits of +-12
 * semitones are those of taco_frames_pitch's arithmetic, not recommendations. */
int taco_frames_formant(const float* mag_t, const int32_t* frames, int frames_per_unit, const int32_t* step_q, int lifter,
                        float* out, int B, int C, int F, void* stream);

/* Prosody inside an utterance (no reference counterpart): the two controls above with one value per FRAME instead of one per row, and
 * the gather that makes such curves from per-character values along the path of taco_alignment_path -- which decoder step speaks
 * which character is the anchor a per-word rate or pitch needs.  Each is one or two plain launches on the caller's stream: no
 * workspace, no allocation, no atomics, nothing read back by the host, graph-capturable, and a replay follows whatever the device
 * buffers hold at replay time.  Refusals return TACO_EINVAL with a message that names the argument, before anything is enqueued.
 * TACO_VERSION did not change with these entry points: detect them by the symbol.
 *
 * taco_path_curve: per-character values -> a per-frame curve.
 *   path   (B, Td) int32 as taco_alignment_path writes it (-1 behind the row's steps); values (B, Tt) int32; both on the DEVICE
 *   curve  (B, Td * frames_per_step) int32, every element written:
 *          curve[b, t * frames_per_step + u] = values[b, path[b, t]] when 0 <= path[b, t] < Tt, else `fill`
 *   A pure gather, exact; no clamping -- the consumers clamp.  One launch.  Any NULL pointer, B, Td, Tt or frames_per_step < 1 and
 *   Td * frames_per_step > TACO_STRETCH_MAX_FRAMES are refused.
 *
 * taco_frames_stretch_curve: a rate that varies along the utterance.  mag_t, frames, frames_per_unit, out, frames_out, B, C, F, Fo and
 * F_b exactly as taco_frames_stretch.
 *   dur_q (B, F) int32 on the DEVICE, or NULL: the output frames source frame i lasts, in units of 2^-16 -- the inverse sense of
 *          step_q, because durations add and steps do not.  Used as d_i = clamp(dur_q[b, i], TACO_STRETCH_MIN_STEP,
 *          TACO_STRETCH_MAX_STEP) (16384: rate 4; 262144: rate 0.25); NULL: 65536 everywhere.  Never read by the host
 *   src   (B, Fo) int32, required: the time map, an OUTPUT (the timings place word boundaries in the stretched audio with it)
 * Per row b, all in integers:
 *   D_0 = 0, D_{i+1} = D_i + d_i  (D reaches 2^31 at F = 8192 with every d_i = 262144: unsigned 32 bits hold it, signed do not)
 *   Fo_b = 0 when F_b == 0, else min(Fo, (D_{F_b - 1} >> 16) + 1);  frames_out[b] = Fo_b
 *   for j < Fo_b: q = j << 16, i = the largest index <= F_b - 1 with D_i <= q, wq = ((q - D_i) << 16) / d_i in 64-bit integer
 *     division (0 <= wq < 65536), w = wq 2^-16;  src[b, j] = (i << 16) | wq
 *     wq == 0: out[b, k, j] = mag_t[b, k, i] bit for bit, and frame i + 1 is NOT read
 *     else:    out[b, k, j] = a + (w * (c - a)), a = mag_t[b, k, i], c = mag_t[b, k, i + 1]: the three separately rounded fp32
 *              operations of taco_frames_stretch
 *   src[b, j] = -1 and out[b, k, j] = +0 for Fo_b <= j < Fo
 * Fo_b's formula gives q <= D_{F_b - 1}: i = F_b - 1 occurs only with wq == 0, and nothing behind a row's end is read.  src rises
 * strictly along a row.  With a constant d of 16384, 32768, 65536, 131072 or 262144 the map, Fo_b and hence every bit of out equal
 * taco_frames_stretch at step 262144, 131072, 65536, 32768, 16384; other constants quantise the weight differently and no equality is
 * claimed.  The guarantees of taco_frames_stretch carry over: every element of out, frames_out and src is written and nothing
 * outside them, any 4-byte alignment, columns behind F_b and other rows have no influence (they may hold NaN), row b of a B-row
 * call equals the call on that row alone.  Two launches: the map (one workgroup per row: the scan of d in LDS, a binary search and
 * the one division per output frame), then taco_frames_stretch's gather reading positions from src.  The refusals of
 * taco_frames_stretch, and NULL src.
 *
 * taco_frames_pitch_curve: a pitch contour.  Everything as taco_frames_pitch, but
 *   step_q (B, F) int32 on the DEVICE, or NULL: frame f of row b uses s = clamp(step_q[b, f], TACO_PITCH_MIN_STEP,
 *          TACO_PITCH_MAX_STEP); NULL: TACO_PITCH_ONE
 * and because the bits of a frame depend on its own C bins, its step and Q alone: frame f has exactly the bits of the same frame in a
 * taco_frames_pitch call whose row step is s; a frame at TACO_PITCH_ONE is its input bit for bit, also next to shifted frames (no
 * log / exp round trip); +0 behind F_b.  One launch, the kernel of taco_frames_pitch with the step per lane; the lifter path
 * depends on Q alone.
 *
 * Not here: ramps across word boundaries (a word's characters share one value, the curve steps at its edges), long prompts split
 * into pieces (--long: the pieces re-index words), mel frames.  Nobody has listened to the result. */
int taco_path_curve(const int32_t* path, const int32_t* values, int frames_per_step, int32_t fill, int32_t* curve, int B, int Td,
                    int Tt, void* stream);
int taco_frames_stretch_curve(const float* mag_t, const int32_t* frames, int frames_per_unit, const int32_t* dur_q, float* out,
                              int32_t* frames_out, int32_t* src, int B, int C, int F, int Fo, void* stream);
int taco_frames_pitch_curve(const float* mag_t, const int32_t* frames, int frames_per_unit, const int32_t* step_q, int lifter,
                            float* out, int B, int C, int F, void* stream);

/* Spectral sharpening at synthesis and the raw material of the global variance (no reference counterpart).  Magnitudes trained under an
 * L1 loss and handed to Griffin-Lim have over-smoothed envelopes: formant peaks too low, valleys filled in.  The measure is the global
 * variance (GV): the variance over an utterance's frames of each cepstral coefficient, predicted against recorded.  The cure is a
 * cepstral post-filter: the envelope's low quefrencies scaled by 1 + beta at unchanged frame energy.
 *
 * taco_frames_sharpen: the post-filter, in the place of taco_frames_pitch (between taco_denorm_unframe and Griffin-Lim; the driver
 * runs it first, in front of pitch, stretch and F0).
 *   mag_t, out, frames, frames_per_unit, B, C, F and F_b exactly as taco_frames_pitch
 *   beta   in [TACO_SHARPEN_MIN_BETA, TACO_SHARPEN_MAX_BETA]; one value for the whole call
 *   lifter Q, TACO_SHARPEN_FIRST <= Q <= min(TACO_PITCH_MAX_LIFTER, (C - 1) / 2): the quefrencies 2 .. Q are scaled (rectangular)
 * For frame f < F_b of row b, m[k] = mag_t[b, k, f], in real numbers:
 *   L[k]  = log(max(m[k], TACO_PITCH_FLOOR))
 *   c[n]  = the cepstrum taco_frames_pitch defines, n = 0 .. Q
 *   D[k]  = 2 beta sum_{n = 2 .. Q} c[n] cos(2 pi n k / N),  N = 2 (C - 1)
 *   y[k]  = m[k] exp(D[k])                                      (m, not max(m, floor): a zero bin stays zero)
 *   P0 = sum_k m[k]^2, P1 = sum_k y[k]^2 (k = 0 .. C - 1, plain sums);  g = sqrt(P0 / P1), and 1 when P1 == 0
 *   out[b, k, f] = y[k] g
 * so that, for bins at or above the floor, the cepstrum of out has c'[n] = (1 + beta) c[n] for 2 <= n <= Q, c'[1] = c[1], c'[n] = c[n]
 * for n > Q, and sum out^2 = sum m^2.  Computed in fp32 with the chains of taco_frames_pitch and held to an fp64 restatement
 * (tests/sharpen_ref.py).  Exactly:
 *   - beta == 0 copies the live frames bit for bit, with no log or exp;
 *   - out[b, k, f] = +0 for F_b <= f < F;
 *   - every element of out is written and nothing outside it, for any 4-byte alignment;
 *   - columns behind F_b, other rows and other frames have no influence on a frame (they may hold NaN);
 *   - the bits of a frame depend on its own bins, beta and Q alone -- not on B, F, its position or the buffers' alignment; no
 *     atomics; the same arguments give the same bits.
 * One launch, no workspace, no allocation, no host synchronisation, graph-capturable; a replay follows `frames` on the device.  NULL
 * mag_t / out, out overlapping mag_t, a bad B, C, F or frames_per_unit, lifter out of range, and beta NaN or outside its range return
 * TACO_EINVAL with a message that names the argument, before anything is enqueued.
 *
 * taco_frames_cepstats: per row the sums over the live frames of every cepstral coefficient and of its square.
 *   sums   (B, Q + 1, 2) fp64, at any 4-byte alignment: sums[b, n, 0] = sum_{f < F_b} c[n][f], sums[b, n, 1] = sum_{f < F_b} c[n][f]^2,
 *          the c[n][f] being the fp32 cepstra of taco_frames_sharpen's first stage (the same chains), added in fp64 in a fixed order
 *   count  (B) int32: count[b] = F_b.  A row with F_b == 0 gives zeros
 *   workspace: taco_frames_cepstats_workspace_bytes(B, C, F, lifter) bytes at any alignment, with any contents
 * Frame tiles are reduced in parallel into per-tile partials in the workspace and a second launch folds them in tile order: no
 * atomics, the same arguments give the same bits, a row does not depend on its neighbours or on columns behind F_b.  No allocation,
 * no host synchronisation, graph-capturable.  The refusals of taco_frames_sharpen without beta and out, and NULL sums, count or
 * workspace; the size function returns TACO_EINVAL for the same B, C, F and lifter.  The variance of coefficient n over a row is
 * sums[b, n, 1] / count - (sums[b, n, 0] / count)^2, formed by the caller in fp64.
 *
 * TACO_VERSION did not change with these entry points: detect them by the symbol.
 * Not here: a per-row or per-frame beta, a tapered lifter, mel frames.  Nobody has listened to the result: the Python layer's
 * defaults (lifter 32) are untuned, and the cepstra are this model's linear-frequency ones -- a GV ratio from them is comparable
 * between checkpoints here, not with published mel-cepstral GV figures. */
#define TACO_SHARPEN_FIRST    2       /* quefrencies 0 (level) and 1 (tilt) are never scaled */
#define TACO_SHARPEN_MIN_BETA -1.0f   /* removes quefrencies 2 .. Q: used by tests to make an over-smoothed input */
#define TACO_SHARPEN_MAX_BETA 1.0f
int taco_frames_sharpen(const float* mag_t, const int32_t* frames, int frames_per_unit, float beta, int lifter, float* out, int B,
                        int C, int F, void* stream);
int64_t taco_frames_cepstats_workspace_bytes(int B, int C, int F, int lifter);
int taco_frames_cepstats(const float* mag_t, const int32_t* frames, int frames_per_unit, int lifter, double* sums, int32_t* count,
                         void* workspace, int B, int C, int F, void* stream);

/* F0 tracker (no reference counterpart): the per-frame pitch of magnitude frames, measured where the two prosody controls above
 * run -- the instrument that stands in for listening to them.  By Wiener-Khinchin the cosine transform of a frame's power spectrum is
 * the autocorrelation of the windowed frame, so no waveform, phase or vocoder run is needed: the same call serves the model's output,
 * the frames behind taco_frames_pitch / taco_frames_stretch and a corpus' recorded stft targets.
 *   mag_t  (B, C, F) fp32, the frame index contiguous; C - 1 a power of two, 8 <= C - 1 <= 1024; N = 2 (C - 1)
 *   frames, frames_per_unit: as taco_frames_pitch: F_b = clamp(frames[b] * frames_per_unit, 0, F), NULL: F_b = F; never read by the host
 *   weight (C) fp32 or NULL (all ones): a weight per bin of the power spectrum (the Python layer undoes the features' pre-emphasis
 *          with it; it can also band-limit)
 *   gain   (L) fp32 or NULL (all ones), L = lag_max - lag_min + 3: gain[j] multiplies lag lag_min - 1 + j (the Python layer passes
 *          the inverse of the analysis window's own autocorrelation: Boersma's correction)
 *   2 <= lag_min <= lag_max <= C - 2 and L <= TACO_F0_MAX_LAGS; 0 < ratio <= 1; threshold any number
 *   period (B, F), strength (B, F) fp32: required; acf (B, L, F) fp32 or NULL
 * For frame f < F_b of row b, m[k] = mag_t[b, k, f], u[0] = u[C-1] = 1 and u[k] = 2 otherwise, in real numbers:
 *   p[k] = u[k] weight[k] m[k]^2;   r0 = sum_k p[k];   r[n] = sum_k p[k] cos(2 pi n k / N), n = lag_min - 1 .. lag_max + 1
 *   r0 > 0 false (zero, underflowed, NaN): the frame is unvoiced, period = strength = +0 and its acf column is +0.  Otherwise
 *   y[n] = (r[n] / r0) gain[n - lag_min + 1];   acf[b, j, f] = y[lag_min - 1 + j]
 * computed in fp32 (a cosine table from cospif; the product on v_mfma_f32_32x32x2_f32, one ordered chain over the bin pairs per
 * lag and frame) and held by the tests to an fp64
 * restatement within a tolerance sized from a float32 restatement (tests/f0_ref.py).  The pick is EXACT: every operation below is one
 * fp32 operation rounded to nearest even on the fp32 values y that acf holds, nothing contracted, so a NumPy float32 restatement
 * applied to the device's own acf gives the device's period and strength bit for bit:
 *   candidates: the n in [lag_min, lag_max] with y[n] > y[n-1] and y[n] >= y[n+1]; none: unvoiced
 *   g = the largest candidate value; n* = the smallest candidate with y[n] >= ratio * g (the bias towards short lags suppresses
 *   octave-down errors); y[n*] >= threshold false: unvoiced
 *   a = y[n*-1] - y[n*+1], t = y[n*] + y[n*], d = (y[n*-1] - t) + y[n*+1];  delta = 0 when d == 0, else (0.5f * a) / d correctly
 *   rounded and clamped to [-0.5, 0.5];  period = float(n*) + delta in samples (F0 = sr / period is the host's to form);
 *   strength = y[n*] (it may exceed 1 with a gain)
 * Further:
 *   - period, strength and acf are +0 for F_b <= f < F;
 *   - every element of the outputs is written and nothing outside them, for any F and any 4-byte alignment;
 *   - columns f >= F_b, every other row and every other frame have no influence on a frame (they may hold NaN); a non-finite value
 *     inside a frame leaves unspecified values in that frame's outputs only;
 *   - the bits of a frame depend on its own C bins and the arguments alone -- not on B, F, its position f or the buffers'
 *     alignment; no atomics; with acf == NULL period and strength have the bits of the call with it.
 * One launch of B x ceil(F / 32) workgroups, no workspace, no allocation, no host synchronisation, no workgroup waits for another
 * one: graph-capturable, and a replay follows whatever frames holds at replay time.  NULL mag_t / period / strength, an output
 * overlapping mag_t, B or F <= 0, F > TACO_STRETCH_MAX_FRAMES, C - 1 not a power of two in 8 .. 1024, lags out of range, ratio
 * outside (0, 1] or NaN, a NaN threshold and frames_per_unit < 1 return TACO_EINVAL, with a message that names the argument, before
 * anything is enqueued.  TACO_VERSION did not change with this entry point: detect it by the symbol.
 * Not here: F0 from mel frames.  Smoothing across frames is taco_f0_viterbi below, which reads the acf this call writes.  The Python
 * layer's ratio 0.9 and threshold 0.3 are untuned. */
#define TACO_F0_MAX_LAGS 512
int taco_frames_f0(const float* mag_t, const int32_t* frames, int frames_per_unit, const float* weight, const float* gain,
                   int lag_min, int lag_max, float ratio, float threshold, float* period, float* strength, float* acf,
                   int B, int C, int F, void* stream);

/* Statistics of a pitch track: a frame counts when f < F_b and period[b, f] > 0 -- with `other` (B, F) given, other[b, f] > 0 too.
 *   x_f = log2(period[b, f]) without other;  x_f = log2(other[b, f]) - log2(period[b, f]) with it: the octaves by which period's
 *   pitch lies above other's (12 x the mean: semitones)
 *   stats (B, 3) fp32 = (the count as a float, the mean of x, the population standard deviation of x); the last two 0 at count 0
 * fp32, one workgroup per row, two passes in a fixed order (the sum, then the squares around the mean): no atomics, no workspace,
 * graph-capturable; frames / frames_per_unit as above.  NULL period / stats, B or F <= 0, F > TACO_STRETCH_MAX_FRAMES and
 * frames_per_unit < 1 return TACO_EINVAL before anything is enqueued.  Detect it by the symbol. */
int taco_f0_stats(const float* period, const float* other, const int32_t* frames, int frames_per_unit, float* stats, int B, int F,
                  void* stream);

/* The intonation range of an utterance (no reference counterpart): a tracked pitch contour -> the per-frame step curve
 * taco_frames_pitch_curve consumes, which multiplies every frame's distance from the row's own pitch level, in octaves, by k --
 * the cure for the flattened intonation of an L1-trained model that taco_f0_stats' deviation measures.
 *   period  (B, F) fp32 as taco_frames_f0 / taco_f0_viterbi write it; a frame is voiced when f < F_b and period[b, f] > 0
 *   frames, frames_per_unit: as taco_frames_f0 (F_b = clamp(frames[b] * frames_per_unit, 0, F) in 64 bits, NULL: F); never read by the host
 *   scale_q (B) int32 on the device or NULL (65536): k_b = clamp(scale_q[b], 0, 4 * 65536) * 2^-16; 0 flattens the contour to the
 *           row's level, 65536 is neutral, 98304 widens every excursion by 1.5
 *   base_q  (B, F) int32 on the device or NULL (TACO_PITCH_ONE): a step curve to compose with (a broadcast pitch, a prosody curve),
 *           used as clamp(base, TACO_PITCH_MIN_STEP, TACO_PITCH_MAX_STEP)
 *   smooth  = W, 0 <= W <= TACO_F0_RANGE_MAX_SMOOTH;  limit in octaves, 0 < limit <= 1: the ceiling on the excursion change of one
 *           frame, so that an octave error of the tracker cannot be amplified without bound
 *   step_q  (B, F) int32: the output;  stats (B, 3) fp32 or NULL: exactly what taco_f0_stats(period, NULL, ...) writes for the row
 * Per row, with x_f = log2f(period[b, f]) on voiced frames, fp32, every step one rounded operation, nothing contracted:
 *   1. count, c (the mean) and the deviation are THE BITS of taco_f0_stats: one device function, both kernels.  count == 0: every
 *      frame f < F_b gets clamp(base), or TACO_PITCH_ONE without a base
 *   2. d_f = x_f - c on voiced frames
 *   3. an unvoiced frame f with p the nearest voiced frame before it and n the nearest one after it: t = float(f - p) / float(n - p),
 *      d_f = d_p + t * (d_n - d_p); with only one of them: that neighbour's value.  The search runs in integers.
 *   4. s_f = (sum_{j = -W .. W} (W + 1 - |j|) * d[clamp(f + j, 0, F_b - 1)]) / (W + 1)^2, summed in the order j = -W .. W from +0
 *   5. e_f = clamp((k_b - 1) * s_f, -limit, limit)
 *   6. with a base: e_f += log2f(float(clamp(base)) * 2^-16)
 *   7. step_q[b, f] = clamp((int)rintf(65536 * exp2f(e_f)), TACO_PITCH_MIN_STEP, TACO_PITCH_MAX_STEP)
 *   8. step_q[b, f] = TACO_PITCH_ONE for F_b <= f < F
 * The sign follows from the units: a longer period is a lower pitch and step = 65536 / ratio, so step = 65536 * 2^((k - 1)(x - c))
 * multiplies the frame's distance from the level by k.  tests/f0_range_ref.py restates this in float64 and float32; the device is
 * held to the former within a bar sized from the latter.  Further:
 *   - a row with scale_q == 65536 gives clamp(base), or TACO_PITCH_ONE, bit for bit on every frame f < F_b: no log, no exp;
 *   - every element of step_q, and of stats when given, is written and nothing outside them, for any 4-byte alignment;
 *   - columns f >= F_b and other rows have no influence (they may hold NaN): row b of a B-row call equals the call on it alone;
 *   - no atomics: the same arguments give the same bits.
 * One launch of B workgroups, no workspace, no allocation, no host synchronisation: graph-capturable, and a replay follows
 * whatever frames, scale_q, base_q and period hold at replay time.  NULL period / step_q, step_q overlapping period or base_q, B or
 * F <= 0, F > TACO_STRETCH_MAX_FRAMES, frames_per_unit < 1, smooth outside 0 .. 8 and a limit that is NaN or outside (0, 1] return
 * TACO_EINVAL, with a message that names the argument, before anything is enqueued.  TACO_VERSION did not change with this entry
 * point: detect it by the symbol.
 * The Python layer's smooth = 2 and limit = 0.5 are UNTUNED: nobody has listened.  Measured on one MI355X at 32 rows of 360 | 720 |
 * 8192 frames (profiles/f0_range_timing.json): 6.0 | 7.3 | 44.2 us with W = 2 and a base = 1.62 | 1.77 | 2.84 x taco_f0_stats on
 * the same period in the same run, 0.02 | 0.013 % of the Griffin-Lim call behind the chain; the factor at 8192 frames is an open
 * item.  Not here: a per-word range, a target range in semitones
 * instead of a factor, an energy contour, mel frames. */
#define TACO_F0_RANGE_MAX_SMOOTH 8
int taco_f0_range_curve(const float* period, const int32_t* frames, int frames_per_unit, const int32_t* scale_q, const int32_t* base_q,
                        int smooth, float limit, int32_t* step_q, float* stats, int B, int F, void* stream);

/* A pitch track smoothed across frames (no reference counterpart): up to K candidates per frame out of the acf taco_frames_f0 writes,
 * and per frame one of them, or "unvoiced", chosen by the best path under a cost for pitch jumps and one for voiced / unvoiced
 * switches (Boersma 1993) -- the cure for the octave flips and single-frame voicing drops of a pick that decides every frame alone.
 *   acf    (B, L, F) fp32 as taco_frames_f0 writes it, L = lag_max - lag_min + 3, row j the lag lag_min - 1 + j; any 4-byte alignment
 *   frames, frames_per_unit: as taco_frames_f0 (F_b = clamp(frames[b] * frames_per_unit, 0, F) in 64 bits, NULL: F); never read by the host
 *   bias   (L) fp32 or NULL (zeros): subtracted from a candidate's height (Boersma's octave cost; the Python layer makes it)
 *   lg     (L) fp32, required: the caller's log2 of the lag of every row -- the device takes no logarithm
 *   1 <= K <= TACO_F0_MAX_CAND voiced candidates kept per frame; slot K is the unvoiced state
 *   period, strength (B, F) fp32 with the meaning of taco_frames_f0's; counts (B, 4) int32; score (B) fp32: all required, every
 *   element written;  workspace: taco_f0_viterbi_workspace_bytes(B, L, F, K) bytes, arbitrary contents
 * EXACT rules, every arithmetic step one fp32 operation rounded to nearest even, nothing contracted, per row b over its frames
 * f < F_b with y[i] = acf[b, i, f] (tests/f0_viterbi_ref.py restates them in NumPy float32 and gives the device's bits):
 *   1. candidates: the rows 1 <= i <= L - 2 with y[i] > y[i-1] and y[i] >= y[i+1] (a NaN is never one); v(i) = y[i] - bias[i], and
 *      v(i) = y[i] without an operation when bias is NULL
 *   2. kept: the K first under "larger v first, smaller i on equal v", sorted by ascending i into slots 0 .. k_f - 1; the slots
 *      k_f .. K - 1 are absent (v = -inf); slot K has v = threshold
 *   3. T(p -> c) between slots of consecutive frames: both voiced: jump_cost * |lg[i_p] - lg[i_c]| (one subtraction, its absolute
 *      value, one product); exactly one of them slot K: switch_cost; both slot K: +0
 *   4. E(0, c) = v_c;  E(f, c) = max_p (D(f-1, p) - T(p -> c)) + v_c, the predecessor the lowest p of the largest difference (a
 *      strict > from p = 0 on);  m_f = max_c E(f, c);  D(f, c) = E(f, c) - m_f
 *   5. s(F_b - 1) = the lowest c of the largest D(F_b - 1, c);  s(f - 1) = the recorded predecessor of s(f)
 *   6. a frame on a voiced slot with row i: period = float(lag_min - 1 + i) + delta with taco_frames_f0's parabola on y (a, t, d and
 *      the clamp as above), strength = y[i]; a frame on slot K and every frame f >= F_b: +0 and +0;  score[b] = m_0 + m_1 + ...
 *      summed in frame order, +0 for an empty row
 *   7. counts[b] = { F_b, voiced = #{f : s(f) < K}, moved = #{f : s(f) != the lowest slot of the frame's largest local score v},
 *      switches = #{f >= 1 : exactly one of s(f-1), s(f) is K} }; four zeros at F_b = 0
 *   8. hence with jump_cost = switch_cost = 0 and bias NULL period and strength have the bits of taco_frames_f0 at ratio = 1 and
 *      the same threshold, and moved = 0
 * Frames f >= F_b and every other row have no influence on a row (they may hold NaN); a non-finite value among a row's first F_b
 * columns leaves unspecified values in that row's outputs only -- the launch still ends and nothing outside the outputs and the
 * workspace is written.  No float atomics: the same arguments give the same bits.  Two launches (B x ceil(F / 32) workgroups for the
 * candidates, B for the paths), no allocation, no host synchronisation, no workgroup waits for another one: graph-capturable, and a
 * replay follows whatever frames holds at replay time.  NULL acf / lg / period / strength / counts / score / workspace, an output
 * overlapping acf, B or F <= 0, F > TACO_STRETCH_MAX_FRAMES, lags outside 2 <= lag_min <= lag_max or L > TACO_F0_MAX_LAGS, K outside
 * 1 .. TACO_F0_MAX_CAND, a NaN or infinite threshold, a negative, NaN or infinite jump_cost or switch_cost and frames_per_unit < 1
 * return TACO_EINVAL, with a message "f0_viterbi: ..." that names the argument, before anything is enqueued; the size function
 * returns TACO_EINVAL for the same shapes.  TACO_VERSION did not change with this entry point: detect it by the symbol.
 * Not here: the candidates formed inside taco_frames_f0's kernel (which would save the acf round trip), Boersma's silence term in
 * the unvoiced score, tuned costs (the Python layer's are Praat's, untuned). */
#define TACO_F0_MAX_CAND 15
int64_t taco_f0_viterbi_workspace_bytes(int B, int L, int F, int K);
int taco_f0_viterbi(const float* acf, const int32_t* frames, int frames_per_unit, const float* bias, const float* lg, int lag_min,
                    int lag_max, int K, float threshold, float jump_cost, float switch_cost, float* period, float* strength,
                    int32_t* counts, float* score, void* workspace, int B, int F, void* stream);

/* F0 error along a warping path: the frame-by-frame companions of MCD (F0 RMSE, voicing decision error, gross pitch error).
 *   period_a (B, Fa), period_b (B, Fb) fp32 periods as taco_frames_f0 writes them (0: unvoiced);  path_a, path_b (B, P) int32,
 *   P = Fa + Fb - 1, and steps (B) int32 as taco_frame_dtw_path writes them;  gross fp32 > 1 (1.2 is usual)
 * steps[b] is used clamped to [0, P].  For t < steps[b] with i = path_a[b, t] in [0, Fa) and j = path_b[b, t] in [0, Fb) -- any
 * other entry is skipped and nothing is read for it -- pa = period_a[b, i], pb = period_b[b, j]:
 *   counts (B, 5) int32 = { cells visited, both voiced (pa > 0 && pb > 0), a only, b only, gross errors among the both-voiced cells:
 *                           pa > gross * pb || pb > gross * pa, each product ONE rounded fp32 multiply (a NumPy float32
 *                           restatement gives the count exactly) }
 *   means (B, 2) fp32 = { mean, root mean square } of x = log2(pb) - log2(pa) over the both-voiced cells: the octaves by which a's
 *                       pitch lies above b's (x 1200: cents; the RMS x 1200 is the F0 RMSE in cents); both +0 without such a cell
 * x is formed in double and rounded once to fp32; the sums of x and x x are fp32, in a fixed order (the same arguments give the
 * same bits).  One workgroup per row, no atomics, no workspace, no
 * allocation, no host synchronisation; graph-capturable.  Nothing outside counts and means is written.  NULL pointers, B, Fa or
 * Fb <= 0, Fa or Fb > TACO_DTW_MAX_FRAMES, gross <= 1 or NaN return TACO_EINVAL (message "path_f0_scores: ...") before anything is
 * enqueued.  Detect it by the symbol. */
int taco_path_f0_scores(const float* period_a, const float* period_b, const int32_t* path_a, const int32_t* path_b,
                        const int32_t* steps, float gross, int32_t* counts, float* means, int B, int Fa, int Fb, void* stream);

/* ---- corpus boundary ----------------------------------------------------------------------------------------------------- */
/* The batch gather of the training corpus with the reference's target standardisation (data_input.py:55-65
 * `(x - mean) / std`, which the reference applies to the whole corpus on the host) fused in: the inverse of
 * taco_denorm_unframe's affine map.  The corpus stays in memory as preprocess stores it.
 *   src    (N, row): N utterances of row = Td * C values; fp16 when src_fp16 != 0, else fp32
 *   index  (B) int64 on the DEVICE, or NULL: identity (row b of src; needs B <= N)
 *   mean, std (C) fp32; the column of element e of an utterance is e % C.  Both NULL: a pure gather / widening, bit-equal to
 *          the conversion.  Exactly one NULL is TACO_EINVAL
 *   out    (B, row) fp32:  out[b, e] = (float(src[index[b], e]) - mean[e % C]) / std[e % C], one IEEE fp32 subtraction and one
 *          correctly rounded fp32 division (no reciprocal multiply) -- NumPy's (x.astype(float32) - mean) / std bit for bit
 *   n_bad  int32 on the device, or NULL.  A row whose index is outside [0, N) reads nothing, is written as zeros and adds one to
 *          *n_bad, which the call zeroes on `stream` first
 * Right for every base alignment the element types allow and every row and C: the host picks, per call, the widest access
 * V in {8 (fp16 only), 4, 2, 1} elements with row % V == 0, src a multiple of V elements and out a multiple of min(V, 4) floats
 * (V = 8: 16-byte loads, two 16-byte stores).  One launch of B x ceil(row / (1024 V)) workgroups; no allocation, no host
 * synchronisation, no workgroup waits for another one: graph-capturable.  NULL src / out, N, B, row or C <= 0, row % C != 0,
 * index == NULL with B > N, or out overlapping src return TACO_EINVAL before anything is enqueued.  TACO_VERSION did not change
 * with this entry point: detect it by the symbol. */
int taco_corpus_batch(const void* src, int src_fp16, const int64_t* index, const float* mean, const float* std, float* out,
                      int32_t* n_bad, int64_t N, int B, int64_t row, int C, void* stream);

/* ---- vocoder ---------------------------------------------------------------------------------------------- */
/* audio.griffinlim (audio.py:77-97) with the reference's constants compiled in (n_fft 2048, win_length 1200, hop_length 300,
 * periodic Hann, librosa center=True framing): n_iter rounds of istft -> stft keeping the given magnitudes, then a final istft.
 *   mag_t  (B, 1025, F)  linear magnitudes (taco_denorm_unframe's mag_t)
 *   phase0 (B, 1025, F)  initial phase angles in radians (the reference draws 2 pi U[0,1), audio.py:81; caller supplied here so
 *                        that results are reproducible)
 *   wave   (B, 300 (F - 1)) output samples
 *   workspace: taco_griffinlim_workspace_bytes(B, F) bytes.  Hand-written 2048-point FFT, no vendor library. */
int64_t taco_griffinlim_workspace_bytes(int B, int F);   /* F >= 5 frames (as taco_griffinlim), else TACO_EINVAL */
int taco_griffinlim(const float* mag_t, const float* phase0, float* wave, void* workspace, int B, int F, int n_iter, void* stream);

/* Griffin-Lim per utterance (no reference counterpart: the reference vocodes one prompt at a time, test.py:64).  As
 * taco_griffinlim, but row b is vocoded over its own first F_b = min(F, frames[b] * frames_per_unit) frames -- columns
 * 0 .. F_b - 1 of its (1025, F) matrices -- so that a batch that ended per row (the lengths of taco_infer_stop) gives every
 * prompt the Griffin-Lim of that prompt alone, and the frames past a row's end cost no FFT.
 *   mag_t  (B, 1025, F), wave (B, 300 (F - 1)) as above; the row pitch stays F
 *   frames (B) int32 on the DEVICE; frames_per_unit >= 1: pass r with the lengths of taco_infer_stop (decoder steps), 1 with
 *          frame counts
 *   phase0 (B, 1025, F) initial angles in radians, or NULL: the phases then come from the device.  Element (b, k, t) has index
 *          i = (b * 1025 + k) * F + t, h = splitmix64(seed * 0xD1342543DE82EF95 + i) in 64-bit wrap-around arithmetic (the mixing
 *          of taco_fill_bernoulli), u = h >> 40 (24 bits), and the unit phasor is (cos, sin) of 2 pi u / 2^24, formed with
 *          sincospif of 2 u / 2^24 (exact in fp32).  All integers: a host restatement gives the same u.  seed is ignored when
 *          phase0 is given
 *   - samples [0, 300 (F_b - 1)) of row b are bit-identical to what taco_griffinlim writes for B = 1, F = F_b from that row's
 *     first F_b columns (copied contiguous) and the same phases; the samples from 300 (F_b - 1) on are exactly 0;
 *   - a row with F_b < 5 (frames[b] <= 0 included; the centre padding needs more than 1024 samples) is all zeros and does no FFT
 *     work;
 *   - columns t >= F_b of mag_t and phase0 have no influence on anything (they may hold NaN).
 * The host reads nothing from frames and does not synchronise: graph-capturable, and a replay follows whatever frames holds at
 * replay time.  workspace: taco_griffinlim_rows_workspace_bytes bytes (one window sum-of-squares table per row: it depends on
 * F_b at the tail).  NULL mag_t / frames / wave / workspace, B <= 0, F < 5, n_iter < 0 or frames_per_unit < 1 return TACO_EINVAL
 * before anything is enqueued.  TACO_VERSION did not change with these two entry points: detect them by the symbol. */
int64_t taco_griffinlim_rows_workspace_bytes(int B, int F);     /* B > 0, F >= 5, else TACO_EINVAL */
int taco_griffinlim_rows(const float* mag_t, const float* phase0, uint64_t seed, const int32_t* frames,
                         int frames_per_unit, float* wave, void* workspace, int B, int F, int n_iter, void* stream);

/* Fast Griffin-Lim with a convergence readout (no reference counterpart beyond the loss audio.py:90-92 prints when verbose).
 * The momentum update of Perraudin, Balazs and Sondergaard, "A fast Griffin-Lim algorithm" (WASPAA 2013).  Round
 * i = 0 .. n_iter - 1, with M = |mag_t| and angles_0 from phase0 / the seed:
 *     t_i = STFT(ISTFT(M * angles_i))                        (one round of the plain algorithm)
 *     c_i = t_i for i = 0, else t_i + momentum * (t_i - t_{i-1})     per bin, complex, fp32
 *     angles_{i+1} = c_i / |c_i|, and (1, 0) where c_i = 0
 * and the waveform is ISTFT(M * angles_{n_iter}).  librosa's griffinlim(momentum = a) forms t_i - a / (1 + a) t_{i-1}, which is
 * c_i / (1 + a): a positive factor per bin, so the phases are the same.  momentum = 0 is the plain algorithm.
 *   mag_t, phase0 (nullable: device counter-hash phases from seed), wave, frames_per_unit, B, F, n_iter: exactly as for the
 *          per-utterance entry point above
 *   frames (B) int32 on the DEVICE, or NULL: every row then has F frames (one window table for the batch, as the plain entry
 *          point); frames_per_unit is ignored then but must still be >= 1
 *   momentum 0 <= momentum < 1
 *   conv   (B, n_iter + 1) device floats, or NULL.  conv[b, i] = || |t_i| - M ||_F / || M ||_F over row b's own F_b frames x 1025
 *          bins for i < n_iter (conv[b, 0] is that of the initial phases), and conv[b, n_iter] is the same quantity for
 *          angles_{n_iter}: the spectral convergence of the RETURNED waveform (the STFT of the overlap-added signal that is written
 *          out; one more analysis pass, run only when conv is given).  A row with F_b = 0 or || M || = 0 gets zeros.  Every element
 *          is written
 *   - momentum = 0: wave is bit-identical to the per-utterance entry point with the same arguments (frames given) and to the plain
 *     one (frames NULL, phase0 given); n_iter <= 1: wave does not depend on momentum; wave does not depend on whether conv is given;
 *   - the per-row contract above holds for every momentum, for wave and for row b of conv: bit-identical to a B = 1, F = F_b call
 *     on that row's first F_b columns; zeros behind 300 (F_b - 1) samples; no FFT work for F_b < 5; columns t >= F_b may hold NaN;
 *   - no atomics: the same arguments give the same bits in wave and conv.
 * No allocation, no host synchronisation, nothing read from frames on the host: graph-capturable.  workspace:
 * taco_griffinlim_fast_workspace_bytes bytes, 8-byte aligned, arbitrary contents (the per-utterance layout, a second spectrum
 * (B, F, 1025, 2) and the readout's partial sums; independent of n_iter).  NULL mag_t / wave / workspace, B <= 0, F < 5, n_iter < 0,
 * frames_per_unit < 1, momentum < 0, >= 1 or NaN return TACO_EINVAL before anything is enqueued.  TACO_VERSION did not change with
 * these two entry points: detect them by the symbol. */
int64_t taco_griffinlim_fast_workspace_bytes(int B, int F);      /* B > 0, F >= 5, else TACO_EINVAL */
int taco_griffinlim_fast(const float* mag_t, const float* phase0, uint64_t seed, const int32_t* frames, int frames_per_unit,
                         float momentum, float* wave, float* conv, void* workspace, int B, int F, int n_iter, void* stream);

/* Initial phases read off the magnitudes (no reference counterpart: the reference draws them at random, audio.py:81): single-pass
 * spectrogram inversion (Beauregard, Harish and Wyse, "Single pass spectrogram inversion", DSP 2015).  Every spectral peak of a frame
 * is taken as a sinusoid: its frequency is refined by a parabola through three bins, its phase is advanced by hop x frequency from
 * the previous frame, and the bins of its lobe are locked to it.  The result is the phase0 of the three Griffin-Lim entry points above.
 *   mag_t  (B, 1025, F) fp32 magnitudes (taco_denorm_unframe's mag_t, or what the pitch / stretch calls made of it)
 *   frames, frames_per_unit: as for the calls above (F_b = clamp(frames[b] * frames_per_unit, 0, F) in 64 bits, NULL: F); never read
 *          by the host
 *   phase0 (B, 1025, F) fp32 radians in [0, 2 pi), every element written;  workspace: taco_phase_estimate_workspace_bytes(B, F)
 *          bytes, 4-byte aligned, arbitrary contents
 * EXACT rules.  Only fp32 subtraction, multiplication, one IEEE division and integers, nothing contracted: a restatement in NumPy
 * float32 / uint32 (tests/phase_estimate_ref.py) gives the device's bits.  K = 1025 bins, N = 2048, hop = 300; per row b and frame
 * t < F_b, m[j] = |mag_t[b, j, t]|; acc[0 .. K-1] one unsigned 32-bit accumulator per bin and row, the phase at the centre of the
 * frame in turns x 2^32, wrapping modulo 2^32, all zero in front of frame 0:
 *   1. peaks: bin j is a peak when 1 <= j <= K - 2, m[j] > m[j-1] and m[j] >= m[j+1]
 *   2. offset of a peak j, with a = m[j-1], b = m[j], c = m[j+1]: den = (a - 2 b) + c; p = 0 when den == 0, else
 *      (0.5 (a - c)) / den clamped to [-0.5, 0.5]; q = (int) rint(p x 65536)
 *   3. advance: adv[j] = (300 x (j x 65536 + q)) << 5 modulo 2^32 -- hop (j + p) / N turns in Q32 (300 x 2^32 / (2048 x 65536) =
 *      300 x 32), in wrapping unsigned arithmetic, never in float
 *   4. owner: left[j] the largest peak index <= j, right[j] the smallest peak index > j, either may be absent;
 *      own[j] = right[j] when j < K - 1 and m[j+1] > m[j], else left[j] (a peak owns itself).  A bin whose owner is absent has none:
 *      every bin of a frame without peaks, the bins left of the first peak that do not rise, the bins that rise into bin K - 1
 *   5. update, all bins at once from the previous frame's accumulators: acc'[j] = acc[own[j]] + adv[own[j]] modulo 2^32 when j has
 *      an owner, else acc'[j] = acc[j]
 *   6. output: u = ((acc'[j] + (j << 31)) mod 2^32) >> 8; phase0[b, j, t] = (float) u x (2 pi / 2^24), one rounded fp32 product with
 *      the fp32 constant.  The half turn per bin stands for the analysis window being centred in its 2048-sample frame
 *   - phase0[b, :, t >= F_b] is exactly +0; columns t >= F_b of mag_t have no influence on anything (they may hold NaN);
 *   - row b of a B-row call is bit-identical to a B = 1, F = F_b call on a contiguous copy of its first F_b columns;
 *   - no atomics: the same arguments give the same bits; nothing is written outside phase0 and the workspace;
 *   - a non-finite magnitude inside F_b does not fault; that row's phases are then unspecified.
 * Two launches (B x ceil(F / 16) workgroups for peaks, owners and advances, B workgroups for the chain across frames), no
 * allocation, no host synchronisation, no workgroup waits for another one: graph-capturable, and a replay follows whatever frames
 * holds at replay time.  NULL mag_t / phase0 / workspace, B or F <= 0, frames_per_unit < 1 and phase0 overlapping mag_t return
 * TACO_EINVAL, with a message "phase_estimate: ..." that names the argument, before anything is enqueued; the size function returns
 * TACO_EINVAL for B or F <= 0.  TACO_VERSION did not change with these two entry points: detect them by the symbol.
 * Not here: a parabola through log-magnitudes (better on stationary tones, but the device's logf is not NumPy's log: it would give
 * up the bit-exact rule above). */
int64_t taco_phase_estimate_workspace_bytes(int B, int F);       /* B > 0, F > 0, else TACO_EINVAL */
int taco_phase_estimate(const float* mag_t, const int32_t* frames, int frames_per_unit, float* phase0, void* workspace, int B, int F,
                        void* stream);

/* Waveform finishing (no reference counterpart: the reference writes the pre-emphasised Griffin-Lim signal as it is,
 * audio.py:67-74).  Undoes the front end's pre-emphasis, optionally cuts leading / trailing silence by the front end's energy
 * rule, and emits fp32 samples and / or PCM16 by write_wav's rule, so that what leaves the device is finished audio.
 *   wave    (B, L) fp32: what the three Griffin-Lim entry points write, L = 300 (F - 1)
 *   samples (B) int32 on the DEVICE, or NULL: n_b = clamp(samples[b], 0, L); NULL: n_b = L.  The host reads nothing from it
 *   deemphasis  a in [0, 1);  trim_top_db >= 0 (0: no trim)
 *   out     (B, L) fp32, nullable;  pcm (B, L) int16, nullable; at least one of the two
 *   bounds  (B, 2) int32 and peak (B) fp32, both required
 * Per row b, in this order:
 *   1. de-emphasis  y[0] = x[0], y[n] = x[n] + a y[n-1] for n < n_b: the inverse of e[n] = y[n] - a y[n-1].  a == 0 gives y = x
 *      bit for bit.  Evaluated as a scan of the maps c -> a c + x[n] over chunks of 2048 samples at fixed positions of the row;
 *      the lag-k term a^k x[n-k] passes through at most 2k + 16 roundings, so
 *      |y - y_exact|[n] <= 2^-24 (16 S[n] + 2 T[n]) to first order, S[n] = |x[n]| + a S[n-1], T[n] = a (T[n-1] + S[n-1])
 *   2. trim (trim_top_db > 0)  mean squares of frames of 2048 samples at hop 512 over y[0 : n_b] reflect-padded by 1024
 *      (1 + n_b / 512 frames); a frame is kept when 10 log10(max(1e-10, ms)) - 10 log10(max(1e-10, max ms)) > -trim_top_db;
 *      s_b = 512 first, e_b = min(n_b, 512 (last + 1)) -- librosa.effects.trim as taco_audio_features applies it with 60 dB.  An
 *      all-zero row is all 0 dB and is not trimmed.  trim_top_db == 0: [s_b, e_b) = [0, n_b); n_b == 0: [0, 0).
 *      bounds[b] = (s_b, e_b)
 *   3. peak[b] = max |y[n]| over [s_b, e_b) (exact); 0 for an empty range
 *   4. out[b, i] = y[s_b + i] for i < e_b - s_b, exactly 0 behind;  pcm[b, i] = (int16) trunc(v * 32767.0f) with
 *      v = peak_b > 1 ? y / peak_b : y -- one IEEE fp32 division, one rounded fp32 multiply (no contraction) -- and 0 behind
 *   - every element of out, pcm, bounds and peak is written and nothing outside them; the workspace may hold arbitrary bytes;
 *   - no atomics: the same arguments give the same bits;
 *   - row b of a B-row call is bit-identical to a B = 1, L = n_b call on a contiguous copy of x[b, 0 : n_b] (n_b >= 1): bounds,
 *     peak and the first n_b elements of out and pcm;
 *   - samples x[b, n >= n_b] have no influence on anything (they may hold NaN); non-finite samples inside n_b do not fault, the
 *     row's values are then unspecified.
 * No allocation, no host synchronisation, no workgroup waits for another one: one stream-ordered enqueue, graph-capturable.
 * workspace: taco_wave_finish_workspace_bytes bytes (y, the chunk aggregates, block maxima and frame energies).  NULL wave /
 * bounds / peak / workspace, out and pcm both NULL, out == wave, B <= 0, L <= 0, deemphasis < 0, >= 1 or NaN, trim_top_db < 0 or
 * NaN return TACO_EINVAL before anything is enqueued.  TACO_VERSION did not change with these two entry points: detect them by the
 * symbol. */
int64_t taco_wave_finish_workspace_bytes(int B, int L);          /* B > 0, L > 0, else TACO_EINVAL */
int taco_wave_finish(const float* wave, const int32_t* samples, float deemphasis, float trim_top_db, float* out, int16_t* pcm,
                     int32_t* bounds, float* peak, void* workspace, int B, int L, void* stream);

/* Joining the finished pieces of long prompts (no reference counterpart: the reference cannot speak a line of more than 140
 * characters).  A long prompt is cut on the host where a speaker would pause (tacotron_amd.data.split_prompt), its pieces are
 * synthesised as rows of ordinary batches and finished by taco_wave_finish; this entry point puts the finished pieces of every
 * prompt together -- silence between them, a short linear ramp at every interior edge -- and emits one fp32 row and / or one PCM16
 * row per prompt, scaled by the PROMPT'S peak.
 *   pieces  (N, pitch) fp32, pitch >= L: row i holds piece i from index 0 -- the `out` of taco_wave_finish, already shifted by its
 *           trim start
 *   bounds  (N, 2) int32 on the DEVICE: the `bounds` of taco_wave_finish as written; len_i = clamp(bounds[i][1] - bounds[i][0], 0, L).
 *           The host reads nothing from it
 *   first   (P + 1) int32 in HOST memory: the pieces of prompt p are rows first[p] .. first[p+1] - 1 (checked: first[0] == 0,
 *           non-decreasing, first[P] == N; a prompt may have no pieces; copied into the workspace on `stream`)
 *   gap     (N) int32 in HOST memory: samples of silence behind piece i (checked >= 0, copied likewise; ignored for the last piece
 *           of a prompt)
 *   fade    >= 0: the length in samples of the linear ramp at every interior edge
 *   out     (P, Lj) fp32, nullable;  pcm (P, Lj) int16, nullable; at least one of the two
 *   offsets (N) int32, total (P) int32 and peak (P) fp32, all required
 * Per prompt p, with o running from 0 and o += len_i + gap_i behind each piece (64-bit):
 *   1. offsets[i] = min(o, Lj);  total[p] = min(Lj, o_last + len_last), 0 for a prompt without pieces
 *   2. f_i = min(fade, len_i / 2) (integer division: the two ramps of a piece never meet; len_i <= 1 has none) and
 *      w(k) = (k + 0.5) / f_i -- one rounded fp32 addition, one IEEE fp32 division.  Sample n of piece i is x w(n) for n < f_i when i
 *      is not the first piece of its prompt, x w(len_i - 1 - n) for n >= len_i - f_i when i is not the last one -- one rounded fp32
 *      multiply (no contraction) -- and x bit for bit otherwise; fade == 0 copies every sample
 *   3. the sample goes to out[p, o_i + n] when that index is below Lj; gaps are exactly 0, and so is everything from total[p] to Lj
 *   4. peak[p] = max |v| over [0, total[p]) (exact); 0 for an empty range
 *   5. pcm[p, j] = (int16) trunc(v' * 32767.0f) with v' = peak_p > 1 ? v / peak_p : v: taco_wave_finish's rule with the prompt's peak.
 *      The pieces are joined at their fp32 amplitudes; the per-piece peaks of taco_wave_finish play no part
 *   - every element of out, pcm, offsets, total and peak is written and nothing outside them, for any Lj and any alignment of out
 *     and pcm (16-byte / 8-byte stores where the row's address allows, scalar ones at a row's two edges);
 *   - pieces[i, n >= len_i] has no influence on anything (it may hold NaN); the workspace may hold arbitrary bytes;
 *   - no atomics: the same arguments give the same bits;
 *   - prompt p of a P-prompt call is bit-identical to a P = 1 call on its own pieces.
 * No allocation, no host synchronisation, no workgroup waits for another one; everything is ordered on `stream`.  workspace:
 * taco_wave_join_workspace_bytes bytes (the joined fp32 rows when out is NULL, the tile maxima, the copies of first and gap).  NULL
 * pieces / bounds / first / gap / offsets / total / peak / workspace, out and pcm both NULL, out overlapping pieces, N, P, L or
 * Lj <= 0, pitch < L, fade < 0, a first that does not start at 0, decreases or does not end at N, and a negative gap return
 * TACO_EINVAL before anything is enqueued.  TACO_VERSION did not change with these two entry points: detect them by the symbol. */
int64_t taco_wave_join_workspace_bytes(int N, int P, int Lj);      /* N, P, Lj > 0, else TACO_EINVAL */
int taco_wave_join(const float* pieces, int64_t pitch, const int32_t* bounds, const int32_t* first, const int32_t* gap, int fade,
                   float* out, int16_t* pcm, int32_t* offsets, int32_t* total, float* peak, void* workspace,
                   int N, int P, int L, int Lj, void* stream);

/* Loudness (no reference counterpart: the reference writes whatever level the checkpoint produced).  Measures the integrated
 * loudness of finished rows by ITU-R BS.1770 -- K-weighting, 400 ms blocks at 75 % overlap, an absolute and a relative gate -- and
 * optionally emits the rows at a target loudness under a ceiling on the sample peak, as fp32 and / or PCM16.
 *
 * taco_k_weighting is a HOST function (no GPU call): coef = b0 b1 b2 a1 a2 of the shelf, then b0 b1 b2 a1 a2 of the high-pass, in
 * fp64, for sr a multiple of 10 with 8000 <= sr <= 48000 (else TACO_EINVAL; NULL coef likewise):
 *   shelf      f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196, K = tan(pi f0 / sr), Vh = 10^(G/20),
 *              Vb = Vh^0.4996667741545416, a0 = 1 + K/Q + K^2, b = [(Vh + Vb K/Q + K^2)/a0, 2 (K^2 - Vh)/a0, (Vh - Vb K/Q + K^2)/a0],
 *              a1 = 2 (K^2 - 1)/a0, a2 = (1 - K/Q + K^2)/a0
 *   high-pass  f0 = 38.13547087602444, Q = 0.5003270373238773, K = tan(pi f0 / sr), d = 1 + K/Q + K^2, b = [1, -2, 1],
 *              a1 = 2 (K^2 - 1)/d, a2 = (1 - K/Q + K^2)/d
 * which is the standard's table at 48 kHz.  The device uses these values rounded once to fp32.
 *
 * taco_wave_loudness:
 *   wave    (B, L) fp32, contiguous: the rows taco_wave_finish writes to `out`, or the rows taco_wave_join writes
 *   samples (B) int32 on the DEVICE, or NULL: n_b = clamp(samples[b], 0, L); NULL: n_b = L.  The host reads nothing from it
 *   sr      as for taco_k_weighting;  target_lufs in [-70, 0];  ceiling in (0, 1], on |sample|
 *   out     (B, L) fp32, nullable;  pcm (B, L) int16, nullable.  With both NULL the call measures only and neither target_lufs nor
 *           ceiling is looked at
 *   loud    (B, 4) fp32 = (I, M, g, peak_out) and blocks (B, 4) int32 = (nb, blocks past the absolute gate, blocks past both
 *           gates, limited), both required
 * Per row b, in this order:
 *   1. K-weighting  y = highpass(shelf(x[0 : n_b])) from a zero state, each biquad in the transposed direct form II in fused
 *      multiply-adds: u = b0 x + s1; s1 = -a1 u + (b1 x + s2); s2 = -a2 u + b2 x; y = u + t1; t1 = -a1' y + (-2 u + t2);
 *      t2 = -a2' y + u.  With S = (s1, s2, t1, t2) a sample is S -> M S + v x for a constant 4 x 4 matrix M, so k samples are
 *      S -> M^k S + R.  Evaluated as a scan of these maps over chunks of TACO_LOUD_CHUNK = 2048 samples at fixed positions of the
 *      row, a thread owning 8 consecutive samples: the thread's run from a zero state; a scan over the 64 lanes of a wave in steps of
 *      1, 2, ..., 32 lanes (X_l += M^(8 d) X_(l-d)); the four waves of a chunk in order with M^512; the state that enters chunk c by
 *      the same scan over the chunks' end states, 64 chunks at a time in order, in steps of 1, 2, ..., 32 chunks with M^(2048 d), the
 *      state that enters a group of 64 folded into its first chunk's end state with M^2048; the state entering the wave folded into
 *      lane 0's end state (with M^8) and the lane scan once more -- all of this in
 *      fp64, with the fp32 coefficients widened and the powers of M formed from them on the host in fp64 by repeated squaring
 *      (nothing assumes that a power is negligible); the state that enters a thread's run is then rounded to fp32 once and the
 *      thread's run AGAIN from it, in fp32 by the recursion above, yields y.  The fp64 part is there because the high-pass has a
 *      double pole at radius 0.985 to 0.995: fp32 runs from a zero state leave 1e-3 of a constant input in y at 48 kHz
 *   2. hops and blocks  H = sr / 10, nh = n_b / H.  h_k = the sum of the rounded fp32 squares y^2 over hop k: 64 partial sums, partial
 *      l adding samples l, l + 64, ... of the hop in that order, then a fixed tree over the 64.  nh >= 4: nb = nh - 3 blocks,
 *      z_j = (((h_j + h_j+1) + h_j+2) + h_j+3) / (4 H), one IEEE division.  1 <= n_b < 4 H: ONE block over all samples,
 *      z_0 = sum(y^2) / n_b (the same 64-way sum over [0, n_b)) -- a stated deviation from BS.1770, which leaves a signal shorter
 *      than 400 ms unmeasured.  n_b == 0: no block
 *   3. gates, in the power domain (no logarithm takes part in a decision): block j passes the absolute gate when z_j > Z_ABS = the
 *      fp32 value of 10^((-70 + 0.691)/10); with m_A the mean of those (256 partial sums, partial t adding blocks t, t + 256, ...,
 *      a fixed tree, one division by the count), it passes the relative gate when also z_j > 0.1f m_A; z_I = the mean of the
 *      blocks past both, summed likewise
 *   4. readings  I = -0.691 + 10 log10(z_I), -inf when no block passes; M = -0.691 + 10 log10(max_j z_j), -inf without a block or
 *      with z = 0; both formed in fp64 from the fp32 means and rounded once
 *   5. gain (only with out or pcm)  peak_in = max |x| over [0, n_b), exact.  g = 10^((target_lufs - I)/20) (fp64, rounded once);
 *      when the fp32 product peak_in g > ceiling: g = ceiling / peak_in (one IEEE fp32 division), limited = 1.  g = 1, limited = 0
 *      when I is -inf or peak_in is 0.  out[b, n] = x[n] g, one rounded fp32 multiply, no contraction; peak_out = max |out| (exact:
 *      it is the rounded product peak_in g);  pcm[b, n] = (int16) trunc(v * 32767.0f) with v = out clamped to [-1, 1] first.
 *      Everything from n_b to L is exactly 0 in out and pcm.  Measure-only: g = 1, limited = 0, peak_out = peak_in
 *   - every element of out, pcm, loud and blocks is written and nothing outside them, for any L and any alignment of out and pcm
 *     (16-byte / 8-byte stores where the row's address allows, scalar ones at a row's two edges); the workspace may hold arbitrary
 *     bytes;
 *   - no atomics: the same arguments give the same bits;
 *   - row b of a B-row call is bit-identical to a B = 1, L = n_b call on a contiguous copy of x[b, 0 : n_b] (n_b >= 1);
 *   - x[b, n >= n_b] has no influence on anything (it may hold NaN); non-finite samples inside n_b do not fault, the row's values
 *     are then unspecified;
 *   - out may alias wave (out == wave): the map is elementwise and nothing is shifted, unlike taco_wave_finish.
 * No allocation, no host synchronisation, no workgroup waits for another one: graph-capturable, and a replay follows whatever
 * samples holds at replay time.  Five to seven launches.  workspace: taco_wave_loudness_workspace_bytes bytes, 16-byte aligned (y, the
 * chunks' end states, carries and maxima, the hop sums).  NULL wave / loud / blocks / workspace, B <= 0, L <= 0, an sr that taco_k_weighting refuses and -- with out
 * or pcm -- target_lufs outside [-70, 0] or NaN, ceiling outside (0, 1] or NaN return TACO_EINVAL, with a message
 * "wave_loudness: ...", before anything is enqueued; the size function returns TACO_EINVAL for the same shapes.  TACO_VERSION did not
 * change with these entry points: detect them by the symbol.
 * Not here: loudness range and short-term loudness, more than one channel.  True-peak (oversampled) limiting is taco_wave_limit,
 * below: this call's own ceiling stays what it was, on the sample peak and by the whole row's gain. */
#define TACO_LOUD_CHUNK 2048
int taco_k_weighting(int sr, double coef[10]);
int64_t taco_wave_loudness_workspace_bytes(int B, int L, int sr);   /* B > 0, L > 0, sr as above, else TACO_EINVAL */
int taco_wave_loudness(const float* wave, const int32_t* samples, int sr, float target_lufs, float ceiling, float* out, int16_t* pcm,
                       float* loud, int32_t* blocks, void* workspace, int B, int L, void* stream);

/* True-peak meter and look-ahead limiter (no reference counterpart).  taco_wave_loudness reaches its ceiling by holding the whole
 * row's gain down, and its ceiling is on the sample peak.  taco_wave_limit applies the gain G_b the caller asks for and pulls down
 * only the neighbourhood of a peak, with the ceiling on the TRUE peak: the largest of the samples and of P - 1 interpolated phases
 * between them.  There is no recursion in it -- an interpolating FIR, a sliding minimum, a smoothing FIR -- and every value is ONE
 * rounded fp32 operation in a stated order with no contraction (no fused multiply-add), so a NumPy float32 restatement gives the
 * same bits (tests/limiter_ref.py).
 *   wave    (B, L) fp32, contiguous
 *   samples (B) int32 on the DEVICE, or NULL: n_b = clamp(samples[b], 0, L); NULL: n_b = L.  The host reads nothing from it
 *   gain    (B) fp32 on the DEVICE, or NULL: G_b = gain[b]; a value that is not a finite positive number counts as 1; NULL: 1
 *   ceiling in (0, 1], on the true peak
 *   taps    (P - 1, T) fp32 on the device: phases 1 .. P - 1 of the interpolator; P in 1..8, T even in 2..32.  P = 1: a sample-peak
 *           limiter, taps is not looked at.  (tacotron_amd.lib.true_peak_taps: a Kaiser-windowed sinc, each phase normalised)
 *   window  (2 W + 1) fp32 on the device: non-negative smoothing weights; W in 0..512 is the look-ahead in samples
 *   out     (B, L) fp32, nullable, may be wave itself (else it may not overlap wave);  pcm (B, L) int16, nullable
 *   peaks   (B, 4) fp32 = (tp_in, G, g_min, peak_out);  counts (B, 2) int32 = (n_b, samples with s < 1); both required
 * Per row, with x = 0 outside [0, n_b):
 *   1. envelope  for p = 1 .. P - 1: v_p[n] = sum_{j = 0 .. T - 1} taps[p - 1][j] x[n - (T/2 - 1) + j], accumulated from 0 in order of
 *      j as acc = fl(acc + fl(t x));  e[n] = max(|x[n]|, |v_1[n]|, ...): phase 0 is the sample itself;  tp_in = max_n e[n] over
 *      [0, n_b), 0 for an empty row
 *   2. required gain  ge = fl(G e[n]);  r[n] = fl(ceiling / ge) when ge > ceiling, else exactly 1;  r = 1 outside [0, n_b)
 *   3. look-ahead  m[i] = min r[j] over |j - i| <= W
 *   4. smoothing  d[n] = sum_{k = 0 .. 2W} fl(window[k] fl(1 - m[n - W + k])), accumulated from 0 in order of k;
 *      s[n] = min(fl(1 - d[n]), r[n]).  s is exactly 1 wherever no sample within 2 W needs limiting, and s <= r makes the bound exact
 *   5. emit  out[n] = fl(fl(G x[n]) s[n]);  pcm = (int16) trunc(v * 32767.0f) with v = out clamped to [-1, 1] first (the rule of
 *      taco_wave_loudness);  everything from n_b to L is exactly 0;  g_min = min s (1 for an empty row), peak_out = max |out|.
 *      |out| <= ceiling (1 + 2^-22): |fl(G x)| <= ge, and fl(ge fl(ceiling / ge)) carries two roundings
 *   6. measure only (out and pcm both NULL): step 1 alone.  peaks = (tp_in, 1, 1, max |x|), counts = (n_b, 0); gain, ceiling, window
 *      and W are not looked at.  This is the dBTP meter
 * The contract is that of taco_wave_loudness: every element of out, pcm, peaks and counts is written and nothing outside them, for
 * any L and any alignment of out and pcm (16-byte / 8-byte stores where the address allows, scalar ones at the edges of a chunk of
 * TACO_LIMIT_CHUNK = 2048 samples); the workspace may hold arbitrary bytes and needs the alignment of a float; no atomics: the same
 * arguments give the same bits; row b of a B-row call is bit-identical to the B = 1, L = n_b call on a copy of its samples;
 * x[b, n >= n_b] has no influence on anything (it may hold NaN); non-finite samples inside n_b do not fault, the row's values are
 * then unspecified.  No allocation, no host synchronisation, no workgroup waits for another one: graph-capturable, and a replay
 * follows whatever samples and gain hold at replay time.  Two launches; three when out is the wave (the samples either side of every
 * chunk are copied into the workspace first, so that no workgroup reads what its neighbour overwrites).  NULL wave / peaks /
 * counts / workspace, B <= 0 or > 65535, L <= 0, P or T out of range, T odd, NULL taps with P > 1 and -- with out or pcm -- W out
 * of range, NULL window, ceiling outside (0, 1] or NaN return TACO_EINVAL, with a message "wave_limit: ...", before anything is
 * enqueued; the size function returns TACO_EINVAL for B <= 0, L <= 0 and W out of range.  TACO_VERSION did not change with this
 * entry point: detect it by the symbol.
 * Not here: a recursive (attack / release) limiter, oversampled output, more than one channel. */
#define TACO_LIMIT_CHUNK 2048
int64_t taco_wave_limit_workspace_bytes(int B, int L, int W);   /* B > 0, L > 0, W in 0..512, else TACO_EINVAL */
int taco_wave_limit(const float* wave, const int32_t* samples, const float* gain, float ceiling, const float* taps, int P, int T,
                    const float* window, int W, float* out, int16_t* pcm, float* peaks, int32_t* counts, void* workspace, int B, int L,
                    void* stream);

/* ---- feature front end (preprocess.py) ------------------------------------------------------------------------------- */
/* audio.process_audio (audio.py:38-65) for a batch of waveforms, the reference's constants compiled in (n_fft 2048, win_length
 * 1200, hop_length 300, pre-emphasis 0.97, log(|.| + 1e-8), 80 mels): librosa.effects.trim (0.6 form: frame mean squares at
 * 2048 / 512, top_db 60) -> dropped when longer than max_len, else zero-padded to max_len -> pre-emphasis -> librosa.stft
 * (center=True) -> log magnitudes and log |mel_basis @ stft| (the complex STFT, as melspectrogram(S=stft) computes) -> the
 * r-frame layout of audio.reshape_frames.
 *   wave      (B, L) fp32 samples; row b holds wave_len[b] of them
 *   wave_len  (B) int32 in HOST memory, 1 <= wave_len[b] <= L (checked; copied into the workspace on `stream`)
 *   mel_basis (80, 1025) fp32 filterbank (tacotron_amd.audio.mel_basis: librosa.filters.mel(22050, 2048, 80))
 *   mel       (B, Td, 80 r), stft (B, Td, 1025 r): fp32, or fp16 (round to nearest even of the same fp32 values) when
 *             out_fp16 = 1; Td = (F / 4r) * 4 with F = 1 + max_len / 300.  Rows of dropped utterances are zero
 *   bounds    (B, 2) int32: the trim [start, end) in samples of the input row
 *   kept      (B) int32: 1 = end - start <= max_len, 0 = dropped (the reference's `return None, None`)
 *   workspace taco_audio_features_workspace_bytes(B, L) bytes
 * max_len: a multiple of 300 above 1024 giving at least 4r frames (the reference: 108000); r in 1..5.  Bit-reproducible (no
 * atomics).  Bad arguments return TACO_EINVAL before anything is enqueued. */
int64_t taco_audio_features_workspace_bytes(int B, int L);   /* B, L > 0, else TACO_EINVAL */
int taco_audio_features(const float* wave, const int* wave_len, const float* mel_basis, void* mel, void* stft, int* bounds,
                        int* kept, void* workspace, int B, int L, int max_len, int r, int out_fp16, void* stream);

/* PCM decode and resampling, the stage in front of taco_audio_features: the role of librosa.load(fname, mono=True, sr=sr)
 * (audio.py:39) from the bytes of the WAV data chunk on.  librosa resamples with resampy's 'kaiser_best' windowed sinc; the host
 * (tacotron_amd.audio.resample_filter) evaluates that filter once per rate pair as a polyphase table and this entry point applies it.
 *   pcm     (B, row_bytes) bytes: row b holds little-endian PCM frames as they sit in the file, channels interleaved; one format
 *           per call: width in 1..4 bytes per sample (8-bit unsigned, 16 / 24 / 32-bit signed), channels in 1..8
 *   rows    (B, 2) int32 on the DEVICE: (n_orig_b, n_calc_b), the row's input frames and the outputs to compute.  The host reads
 *           nothing from it and derives no length: librosa's are n_calc = int(n_orig ratio), row length int(ceil(n_orig ratio)).
 *           Used as n_orig_b clamped to [0, row_bytes / (width channels)], n_calc_b clamped to [0, L]
 *   taps    (Q, n_left + n_right) fp32: row p serves the outputs t with (t P) % Q == p; its first n_left entries multiply
 *           x[nn], x[nn - 1], ..., the other n_right multiply x[nn + 1], x[nn + 2], ..., nn = (t P) / Q (64-bit product); rows with
 *           fewer taps are zero-padded.  P / Q = input rate / output rate
 *   wave    (B, L) fp32
 * Per row b:
 *   - decode: sample = (u - 128) / 128 (8-bit), float(v) 2^-(bits - 1) with the int -> float conversion rounded to nearest even
 *     (16 / 32-bit), sign-extended v times 2^-23 (24-bit); mono = the fp32 sum over the channels divided by their count in one IEEE
 *     division, the sum in channel order (8 channels: the balanced tree of NumPy's 8-accumulator block) -- the bits of
 *     x.reshape(-1, channels).mean(axis=1, dtype=float32), i.e. of tacotron_amd.audio.load_wav.  The mono signal x exists in LDS only
 *   - P == Q is decode-only: wave[b, t] = x[t] for t < min(n_orig_b, n_calc_b); taps is not read and may be NULL
 *   - otherwise wave[b, t] for t < n_calc_b is the sum over the taps of row (t P) % Q, in signal order (x[nn - n_left + 1] first,
 *     x[nn + n_right] last), with x = 0 outside [0, n_orig_b): fp32 taps, one fp32 fused multiply-add chain per output
 *   - wave[b, t] = 0 exactly for n_calc_b <= t < L (min(n_orig_b, n_calc_b) when decode-only); every element of wave is written
 *     and nothing outside it
 *   - bytes of row b behind n_orig_b frames have no influence
 *   - no atomics: the same arguments give the same bits; row b of a B-row call is bit-identical to a B = 1 call on that row
 * A workgroup computes TACO_WAVE_RESAMPLE_TILE consecutive outputs of one row from an LDS copy of the frames they read.  No
 * workspace, no allocation, no host synchronisation, no workgroup waits for another one: one stream-ordered enqueue,
 * graph-capturable.  NULL pcm / rows / wave, NULL taps with P != Q, width outside 1..4, channels outside 1..8, P, Q, n_left or
 * n_right < 1, B <= 0 or > 65535, L <= 0, row_bytes <= 0 or not a multiple of width channels, and a P / Q and tap count whose tile
 * does not fit 64 KiB of LDS (((TILE - 1) P / Q + 1 + n_left + n_right) floats; Q == 1: rounded up to a multiple of P, plus the taps)
 * return TACO_EINVAL before anything is enqueued.  TACO_VERSION did not change with this entry point: detect it by the symbol. */
#define TACO_WAVE_RESAMPLE_TILE 1024
int taco_wave_resample(const uint8_t* pcm, int64_t row_bytes, int width, int channels, const int32_t* rows, const float* taps,
                       int P, int Q, int n_left, int n_right, float* wave, int B, int L, void* stream);

/* Bernoulli(p_keep) bytes from a counter-based hash RNG (replaces TF's dropout / Bernoulli sampler state). */
int taco_fill_bernoulli(uint8_t* out, int64_t n, float p_one, uint64_t seed, void* stream);

/* ---- training monitor (monitor.hip) -------------------------------------------------------------------------------- */
/* Statistics and a histogram of each of n segments of ONE fp32 buffer, in one call: what the reference's tf.summary.histogram
 * sites (models/tacotron.py:129,139,152, models/ops.py:73-130) show of eight activations, here for any named row of
 * taco_workspace_table and for every tensor of taco_param_table in the parameter, gradient and Adam buffers.
 *   base      fp32 on the device, 16-byte aligned; segment i is the floats [offset_i, offset_i + size_i) of it
 *   counts    (n, 6) int64: size, finite, NaN, +Inf, -Inf, exact zeros (+0 and -0)
 *   moments   (n, 5) fp64 over the FINITE elements: sum, sumsq, min, max, absmax.  min, max and absmax are the fp32 values widened
 *             (exact; -0 orders below +0); a square is formed in fp64 from the fp32 value (48 bits of product: exact) and only the
 *             sums round.  With no finite element the row is 0, 0, +inf, -inf, 0
 *   hist      (n, NB) int64: the finite elements in sign-symmetric logarithmic buckets, by integer arithmetic on the bits alone:
 *             u = bits(x) & 0x7fffffff, k = u >> (23 - s), s = sub_bits in 0..3;  lo = (127 + e_lo) << s,
 *             hi = ((127 + e_hi + 1) << s) - 1;  m = 0 when k < lo (zeros, subnormals, everything below 2^e_lo), else
 *             m = min(k, hi) - lo + 1 (the top bucket takes everything from its lower edge up);  Nm = (e_hi - e_lo + 1) << s,
 *             NB = 2 Nm + 1;  the bin is Nm for m = 0, Nm + m for a positive and Nm - m for a negative value.
 *             -126 <= e_lo <= e_hi <= 127; 2^s buckets per octave
 * The segments are static for a model, so the work list is a PLAN the host builds once:
 *   taco_tensor_stats_plan_bytes(segments, n)   bytes of the blob for `segments` = (n, 2) int64 in HOST memory, (offset, size) in
 *             floats; TACO_EINVAL for NULL, n outside 1..TACO_STATS_MAX_SEGMENTS, a negative offset or size
 *   taco_tensor_stats_plan(segments, n, base_floats, plan, plan_bytes, &n_items)   writes the blob into HOST memory: a 32-byte header
 *             (4 int64: a tag, n, n_items, base_floats), the segments with their first work item and chunk count, then the work
 *             items (segment, chunk).  A segment that is not inside [0, base_floats) is refused.  The caller copies the blob to the
 *             device (8-byte aligned) and keeps the header
 *   taco_tensor_stats_workspace_bytes(n, n_items, NB)   bytes of the workspace (8-byte aligned): one record and one histogram row
 *             of NB 32-bit counts per work item
 *   taco_tensor_stats(base, plan_dev, plan_header, n, n_items, e_lo, e_hi, sub_bits, counts, moments, hist, workspace, stream)
 *             plan_dev the blob on the device, plan_header its first 32 bytes in HOST memory -- all the call reads on the host; the
 *             descriptors and the work list are read on the device only
 * ORDER OF THE SUMS.  Segment i is laid on positions p = (offset_i & 3) + j, j the element's index in the segment: position 0 is the
 * 16-byte boundary at or below the segment's first float.  Chunk c is the positions [c C, (c + 1) C), C = TACO_STATS_CHUNK; a work
 * item is one chunk and belongs to one wave.  Within a chunk, partial l of 64 adds the elements of the position groups
 * [4 g, 4 g + 4) with g mod 64 == l in increasing position (a group inside the segment is one 16-byte load, a segment's two edge
 * groups scalar loads of its own floats only); the 64 partials meet in the tree v_l += v_(l + 32), then 16, 8, 4, 2, 1.  The chunks'
 * sums meet 64 at a time in chunk order by the same tree (absent chunks count as +0), and the tiles are added to a running total
 * in order.  All of it in fp64, nothing fused but the exact square into its sum.  The cut and the order follow from (offset_i,
 * size_i) alone, never from a neighbour.
 * HISTOGRAM FORM: partial-and-fold.  A wave counts into a histogram of its own in LDS (integer adds); the waves of a workgroup that
 * hold consecutive chunks of one segment add theirs and write one row of 32-bit counts into the workspace, and the second launch
 * adds the rows of a segment as integers -- exact in any order.  No float atomics, no global atomics, no memset.
 *   - every element of counts, moments and hist is written and nothing outside them; the workspace may hold arbitrary bytes;
 *   - floats of base outside every segment are never read and may hold NaN; segments may overlap, may be empty and may start at
 *     any float offset;
 *   - the same arguments give the same bits, and the row of segment i is bit-identical to a call with that segment alone.
 * No allocation, no host synchronisation, no workgroup waits for another one: two stream-ordered launches, graph-capturable.
 * NULL pointers, n outside 1..TACO_STATS_MAX_SEGMENTS, a negative n_items, a bad exponent range or sub_bits, a header that does not
 * carry the tag, n and n_items, a base that is not 16-byte aligned and a plan_dev or workspace that is not 8-byte aligned return
 * TACO_EINVAL, with a message "tensor_stats: ...", before anything is enqueued; the size functions return TACO_EINVAL.  TACO_VERSION
 * did not change with these entry points: detect them by the symbol.
 * Not here: quantiles, per-row (batch element) statistics, fp16 / bf16 buffers. */
#define TACO_STATS_CHUNK        8192    /* C: positions per work item */
#define TACO_STATS_MAX_SEGMENTS 4096
#define TACO_STATS_MAX_BINS     4065    /* NB of e_lo = -126, e_hi = 127, sub_bits = 3 */
int64_t taco_tensor_stats_plan_bytes(const int64_t* segments, int n);
int taco_tensor_stats_plan(const int64_t* segments, int n, int64_t base_floats, void* plan, int64_t plan_bytes, int32_t* n_items);
int64_t taco_tensor_stats_workspace_bytes(int n, int n_items, int NB);
int taco_tensor_stats(const float* base, const void* plan_dev, const void* plan_header, int n, int n_items, int e_lo, int e_hi,
                      int sub_bits, int64_t* counts, double* moments, int64_t* hist, void* workspace, void* stream);

/* ---- weight averaging (ema.hip) ------------------------------------------------------------------------------------ */
/* Exponential moving average of the parameters, tf.train.ExponentialMovingAverage's `shadow -= (1 - decay) (shadow - var)`; no
 * counterpart in the reference, which decodes from the weights as the last minibatch left them.  One pass over two flat fp32
 * buffers of n floats, enqueued behind taco_clip_adam_step_guarded on the step's stream.
 *   ema, params   n floats each on the device, at ANY float alignment (16-byte loads and stores when both are 16-byte aligned, else
 *                 float by float; the result is the same bits either way); they may not overlap
 *   w             1 - decay of THIS update, in [0, 1], from the host: the kernel holds no schedule (the num_updates warm-up
 *                 min(decay, (1 + k) / (10 + k)) is the caller's)
 * THE UPDATE is three separately rounded fp32 operations per element, in this order, nothing fused:
 *   d = params[i] - ema[i];   t = w * d;   ema[i] = ema[i] + t
 * so ema holds the same bits as a NumPy float32 restatement.  (w = 1 does not make ema a copy of params: e + (p - e) is not p in
 * fp32.  Start an average as a copy.)
 * THE GUARD is taco_clip_adam_step_guarded's: err_words (nullable) are the decoder kernels' two error words; when either is non-zero
 * ema is neither read nor written -- a skipped Adam update is not averaged in as if it had happened -- and stats, if given, reads
 * (-1, -1, 0).
 *   stats         nullable; 3 doubles on the device, 8-byte aligned:
 *                 [0] sum of (double)d (double)d, d the fp32 difference above: the squared distance of the live weights from the
 *                     average BEFORE this update;  [1] sum of (double)params[i]^2;  [2] 1 when the update was applied.
 *                 The squares of fp32 values are exact in fp64, so only the order of the additions rounds: per thread in the order
 *                 the thread meets its elements, the 64 lanes of a wave in the tree v_l += v_(l + 32), 16, 8, 4, 2, 1, the waves of a
 *                 workgroup in sequence, one pair of partials per workgroup into the workspace; a second launch of one workgroup adds
 *                 the partials in a fixed order.  The grid follows from n, the alignment and the device's CU count alone
 *   workspace     taco_param_ema_workspace_bytes(n) bytes, 8-byte aligned, arbitrary contents; needed with stats only
 *   - no atomics: the same call on the same inputs gives the same bits;
 *   - the bits of ema do not depend on whether stats is given; with stats == NULL the reduction and the second launch are skipped
 *     and workspace may be NULL;
 *   - nothing is written outside ema, stats and the workspace.
 * No allocation, no host synchronisation, no workgroup waits for another one: one or two stream-ordered launches, graph-capturable.
 * NULL ema or params, n <= 0, w outside [0, 1] or NaN, ema overlapping params, stats without a workspace and a stats or workspace that
 * is not 8-byte aligned return TACO_EINVAL, with a message "param_ema: ...", before anything is enqueued; the size function returns
 * TACO_EINVAL for n <= 0 and needs no device.  TACO_VERSION did not change with these two entry points: detect them by the symbol.
 * Not here: the average inside the Adam kernel (one read of params less; that kernel's bits are pinned), averaging across
 * checkpoint files, fp16 / bf16 buffers, moving statistics of batch norm (the model's BN keeps none). */
int64_t taco_param_ema_workspace_bytes(int64_t n);            /* n > 0, else TACO_EINVAL; needs no device */
int taco_param_ema(float* ema, const float* params, int64_t n, float w, const int32_t* err_words,
                   double* stats, void* workspace, void* stream);

/* ---- measurement --------------------------------------------------------------------------------------------- */
/* Launch-level timing with hipEventRecord pairs on the launch stream (rings of 4096 event pairs per category; no
 * synchronisation at record time).  Categories: 0 = persistent decoder forward kernel, 1 = decoder backward kernel,
 * 2 = MFMA GEMM family (conv_gemm / gemm_tn / fused highway stack launches), 3 = bi-GRU recurrences.
 * taco_profile_enable(mask): bit c switches category c on (mask 0 = off); bit 4 (16) additionally keeps ALL work on the caller's
 * stream (no side stream) while set, so that a category-2 pass times every GEMM launch by itself.
 * taco_profile_read2 synchronises on the recorded events, writes up to `cap` elapsed times (milliseconds) and the
 * algorithmic FLOPs of each launch (2 M N K taps) to the HOST arrays, oldest first, clears the ring, returns the count.
 * Launches that overlap on two streams are each timed by their own events (their times then sum to more than the wall). */
int taco_profile_enable(int mask);
/* Workgroups per cluster the most recent decoder forward (which = 0) / backward (1) launch of this process ran with:
 * 32 on the default path (decoder3.hip: 8 clusters x 32 workgroups, each cluster owning up to 4 batch rows); on the fallback
 * path (decoder.hip: one cluster per batch row) 8 in training and up to 16 at inference, fewer when B * width workgroups
 * would not be co-resident. */
int taco_debug_last_cluster(int which);
/* Labels of the launches currently in ring `which` (what each timed launch was: kernel family and shape), one line per
 * launch, oldest first, into the HOST buffer; returns the number of launches.  Call BEFORE taco_profile_read2 (which clears). */
int taco_debug_profile_labels(int which, char* buf, int cap);
int taco_profile_read(int which, float* ms, int cap);
int taco_profile_read2(int which, float* ms, double* flops, int cap);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* TACO_HIP_H */

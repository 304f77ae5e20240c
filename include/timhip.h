/*
 * timhip.h — C ABI of libtimhip.so: the MI355X (gfx950) implementation of the
 * TIM (time_interval_machine) encoder hot path, forward and backward.
 *
 * Drop-in boundary.  Each stage entry point replaces the
 * torch.nn call chain the reference runs for that stage:
 *
 *   timhip_layer_{fwd,bwd}     <- TransformerEncoderLayer.forward over nn.MultiheadAttention
 *                                 .../models/helpers/transformers.py:92-111 with the mask of
 *                                 recognition/.../models/tim.py:161-166 (det tim.py:320-325,384-389)
 *   timhip_gemm_nt, timhip_wgrad <- nn.Linear forward / input-gradient / weight-gradient:
 *                                 tim.py:66-74 (time MLP), encodings.py:21-26,140-153 (embedders),
 *                                 head.py:8-15 (CLS heads), det head.py:99-114 (regression heads)
 *   timhip_layernorm_{fwd,bwd} <- nn.LayerNorm (+ the ReLU/GELU in front of it) tim.py:72-73,
 *                                 encodings.py:23-25
 *   timhip_time_l1_{fwd,bwd}   <- the K=2 first Linear+ReLU of TIM.time_mlp, tim.py:67-68
 *   timhip_assemble_{fwd,bwd}  <- *FeatureEncoding.forward concat/add/dropout, encodings.py:190-250
 *   timhip_gather_rows / _scatter_rows_add <- the tail slicing of *CLSHead.forward, head.py:18-36
 *   timhip_cast_weight         <- (no reference counterpart) operand-dtype working copies of the
 *                                 fp32 master weights, plain and transposed, once per optimizer step.
 *
 * Conventions
 *   - Plain C: pointers and sizes only.  Every device buffer is allocated and owned by the caller;
 *     the library never allocates device memory and keeps no pointer after the call returns
 *     (re-entrant; forward is called from the Python main thread and backward from PyTorch's
 *     autograd thread).  Exceptions, all opt-in: two process-wide switches - the dropout salt
 *     pointer registered by timhip_dropout_salt() (HIP-graph replay) and the measurement hooks
 *     timhip_gemm_timing_start/stop() (bench.py) - and timhip_softnms_1d(), which synchronises its
 *     stream once (it returns the number of kept segments to the host).
 *   - State that a captured step must redraw lives in caller-owned 64-bit device counters which the drawing kernel itself
 *     advances: the mixup set counter, the batch sampler's iteration counter and the DRLoc draw counter
 *     (timhip_mixup_draw, timhip_sampler_draw, timhip_drloc_draw below).
 *   - All work is enqueued on the `stream` argument (a hipStream_t passed as void*).
 *   - Return value: 0 on success, a negative TIMHIP_E* code otherwise (timhip_strerror()).
 *     No exception crosses the ABI.
 *   - Layout: batch-first.  A window is S = F + Q token rows (F feature tokens first, then Q query
 *     tokens); activations are row-major [B*S, E].  "Operand dtype" T is bf16 for
 *     TIMHIP_PREC_BF16, fp16 for TIMHIP_PREC_F16 and fp32 for TIMHIP_PREC_FP32 / _BF16X3 (which splits on the fly).  Operand matrices are K-contiguous
 *     with a leading dimension that is a multiple of 64 elements, zero padded.
 */
#ifndef TIMHIP_H
#define TIMHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TIMHIP_VERSION 6   /* 6, additive (no layout or signature change, so no new number): timhip_attention_weights, timhip_stack_infer_maps, timhip_stack_infer_maps_workspace_bytes, timhip_rec_{accumulate,finalize,counts}, timhip_det_candidates_{count,emit}, timhip_stack_infer, timhip_stack_infer_workspace_bytes, timhip_attention_fwd_rows, TIMHIP_EPI_GELU_T, lse = NULL in timhip_attention_fwd; 6 (round 6): timhip_timing_stop_families; 5 (round 5): timhip_assemble_{fwd,bwd}_p (token / modality vectors by pointer), timhip_dx_init_slabs, timhip_det_side_loss_{fwd,bwd}, timhip_sigmoid_bwd_rows, timhip_time_l1_fwd_split3, timhip_gather_split3_ranges, TIMHIP_EPI_RELU_SPLIT3_T, timhip_layernorm_{fwd,bwd}2, timhip_cast_rows_pair; 4 (round 4): 8-word timhip_grad_scale block + non-finite flag, TIMHIP_DESC_STREAM16*, timhip_dx_init, timhip_reload_env */

enum {
  TIMHIP_OK = 0,
  TIMHIP_EINVAL = -1,       /* null pointer / bad descriptor field */
  TIMHIP_EUNSUPPORTED = -2, /* shape outside what the kernels handle */
  TIMHIP_EWORKSPACE = -3,   /* workspace too small */
  TIMHIP_ELAUNCH = -4,      /* hipGetLastError() reported a launch failure */
  TIMHIP_EALIGN = -5        /* pointer or leading dimension not aligned */
};

/* TIMHIP_PREC_F16: fp16 MFMA operands (v_mfma_f32_32x32x16_f16: the bf16 rate, 3 more mantissa bits), fp32 accumulation -
 * the arithmetic of the reference's own GPU recipe (torch.cuda.amp fp16 autocast, recognition/scripts/train.py:82,197).
 * Gradient operands are stored multiplied by a power of two (TimDesc.grad_scale; the weight-gradient outputs undo it). */
enum { TIMHIP_PREC_BF16 = 0, TIMHIP_PREC_BF16X3 = 1, TIMHIP_PREC_FP32 = 2, TIMHIP_PREC_F16 = 3 };

/* epilogue selector of the generic GEMM entry point (unit tests, heads) */
enum {
  TIMHIP_EPI_STORE_T = 0,   /* out0(T)   = acc + bias */
  TIMHIP_EPI_RELU_T = 1,    /* out0(T)   = relu(acc + bias) */
  TIMHIP_EPI_STORE_F32 = 2, /* out0(f32) = acc + bias */
  TIMHIP_EPI_GELU_DROP_T2 = 3, /* out1(T) = acc+bias ; out0(T) = drop(gelu(out1)) */
  TIMHIP_EPI_DROP_RES_F32 = 4, /* out0(f32) = res + drop(acc + bias) */
  TIMHIP_EPI_ADD_F32 = 5,   /* out0(f32) = acc + res (res may be null) */
  TIMHIP_EPI_DGELU_T = 6,   /* out0(T)   = acc * dropmask * gelu'(aux(T)) */
  TIMHIP_EPI_DRELU_T = 7,   /* out0(T)   = acc * (aux(T) > 0) */
  TIMHIP_EPI_ATOMIC_F32 = 8,/* out0(f32) += acc (split-K weight gradients) */
  TIMHIP_EPI_SIGMOID_F32 = 9,/* out0(f32) = sigmoid(acc + bias) */
  TIMHIP_EPI_DRELU_F32IN_T = 10,/* out0(T) = acc * (aux(f32) > 0) */
  TIMHIP_EPI_GELU_DROP_G2 = 11, /* u = acc+bias ; out0(T) = dropmask * gelu(u) ; out1(T) = dropmask * gelu'(u): the factor the
                                   backward multiplies with, so that its epilogue (TIMHIP_EPI_MULAUX_T) needs no erf / exp and
                                   no second look at the dropout mask */
  TIMHIP_EPI_MULAUX_T = 12,     /* out0(T) = acc * aux(T) */
  TIMHIP_EPI_RELU_SPLIT3_T = 13,/* v = relu(acc + bias) as the split operand [hi | lo | hi]: out0(T)[m, n] = T(v), [m, ld1 + n] = T(v - hi),
                                   [m, 2 ld1 + n] = T(v); ld1 = the block width (a multiple of 64), ld0 = the row stride (3 ld1) - what
                                   timhip_split3_many (mode 0, relu) makes of the fp32 output, without the round trip (time MLP) */
  TIMHIP_EPI_GELU_T = 14        /* out0(T) = gelu(acc + bias): linear1 of an evaluation forward - no out1, no mask, no dropout; the bits
                                   TIMHIP_EPI_GELU_DROP_G2 writes to out0 at p_drop = 0, from the same kernels at the same shapes */
};

/* Shape of one call.  M = B*S rows flow through the encoder. */
typedef struct TimDesc {
  int32_t B;         /* windows in this batch */
  int32_t S;         /* tokens per window = F + Q */
  int32_t F;         /* feature tokens per window (keys every token may attend to) */
  int32_t d;         /* d_model */
  int32_t E;         /* transformer width = 2*d_model */
  int32_t H;         /* heads */
  int32_t FF;        /* feed-forward width */
  int32_t precision; /* TIMHIP_PREC_* */
  float p_drop;      /* encoder dropout probability; 0 => evaluation mode */
  uint64_t seed;     /* Philox key for this step */
  int32_t layer;     /* layer index (part of the Philox stream id) */
  int32_t reserved;  /* flags: TIMHIP_DESC_* (0 by default) */
  const float* grad_scale; /* backward of TIMHIP_PREC_F16: device {S, 1/S} as timhip_grad_scale writes them (NULL: S = 1).
                              fp16 gradient operands (the T copies LayerNorm-backward writes, and everything the data chain
                              derives from them) are stored multiplied by S; the fp32 gradient stream, the weight, bias
                              and LayerNorm-parameter gradients are true-scale.  Ignored by the other precisions' forward */
} TimDesc;
/* TimDesc.reserved flags */
#define TIMHIP_DESC_ATTN_FP32 1        /* run the attention in fp32 arithmetic (reference kernels) */
#define TIMHIP_DESC_ATTN_BWD_ONE_KERNEL 2 /* accepted and ignored: the single-kernel backward was removed; the fused and two-kernel
                                             forms give the same result */
#define TIMHIP_DESC_WGRAD_OVERWRITE 4  /* bf16 only: timhip_layer_bwd_split / _bwd_weights[_pair] WRITE the weight and bias gradients of the four
                                          Linears (dW = ..., not +=): those buffers need no zero fill and are not read */
#define TIMHIP_DESC_WGRAD_SEPARATE 8   /* bf16 only: four timhip_wgrad launches per layer instead of the grouped one (A/B knob) */
#define TIMHIP_DESC_OUTPROJ_SPLIT 16   /* forward, 16-bit precisions: TimLayerParams.out_w is a [E, ld >= 2E] SPLIT copy of the out-projection
                                          weight, column blocks [hi | lo | ...] as timhip_split3_many(mode 0) writes them; the
                                          out-projection runs over K = 2E with the attention output read twice (TimEpi.a_wrap_k):
                                          its weight's fp16 rounding error - the same for every token, hence not averaged out by
                                          the attention - was the largest single term of the fp16 mode's logit error (DESIGN.md
                                          section 6).  out_wt (the backward's operand) stays the plain transposed copy. */
#define TIMHIP_DESC_INPROJ_SPLIT 32    /* the same for in_w ([3E, ld >= 2E]), l1_w ([FF, ld >= 2E]) and l2_w ([E, ld >= 2FF]): with all four */
#define TIMHIP_DESC_L1_SPLIT 64        /* set every forward GEMM of the layer carries its weight to ~22 bits at twice the matrix */
#define TIMHIP_DESC_L2_SPLIT 128       /* work (an opt-in margin mode, tim_amd: TIM_AMD_SPLIT_LAYER_WEIGHTS=all); default: out only */
/* Backward of TIMHIP_PREC_F16 (grad_scale set), timhip_layer_bwd_split / _data_split: the RESIDUAL part of the gradient stream in
 * the operand dtype, times the gradient scale - like its branch parts (dx_*_add) and the gradient operands - instead of fp32.
 *   STREAM16      inside the layer (between the two LayerNorm-backward launches);
 *   STREAM16_IN   dx_out points at a T [M, E] matrix (what the layer above wrote under STREAM16_OUT), not at floats;
 *   STREAM16_OUT  dx_in is written as such a T matrix (requires dx_in_add: the layer below adds the two as it reads).
 * 120 instead of 160 MB per LayerNorm-backward launch at C2a; parameter gradients move by <= 1.5e-3 of their largest element. */
#define TIMHIP_DESC_STREAM16 0x10000
#define TIMHIP_DESC_STREAM16_IN 0x20000
#define TIMHIP_DESC_STREAM16_OUT 0x40000
/* ABI 6: the layer's saved block carries the keep-bits of its attention dropout (TIMHIP_SAVED_ATTN_KEEP_BITS), drawn ahead of the
 * layer by timhip_attn_keep_bits(): the attention forward and the fused attention backward read them instead of running Philox
 * for every (row, key) in both directions.  Set on the forward AND the backward desc of a step, or on neither. */
#define TIMHIP_DESC_ATTN_KEEP_BITS 0x80000

/* One encoder layer.  *_op are operand-dtype working copies made by timhip_prepare_weights:
 * w (as stored, [N,K]) and wt (transposed, [K,N]).  Biases and LayerNorm parameters are the
 * fp32 master tensors. */
typedef struct TimLayerParams {
  const void *in_w, *in_wt;   /* [3E,E] / [E,3E]   self_attn.in_proj_weight */
  const void *out_w, *out_wt; /* [E,E]             self_attn.out_proj.weight */
  const void *l1_w, *l1_wt;   /* [FF,E] / [E,FF]   linear1.weight */
  const void *l2_w, *l2_wt;   /* [E,FF] / [FF,E]   linear2.weight */
  const float *in_b, *out_b, *l1_b, *l2_b;
  const float *n1_w, *n1_b, *n2_w, *n2_b;
} TimLayerParams;

/* fp32 gradient accumulators, same shapes as the master parameters (+=). */
typedef struct TimLayerGrads {
  float *in_w, *in_b, *out_w, *out_b, *l1_w, *l1_b, *l2_w, *l2_b;
  float *n1_w, *n1_b, *n2_w, *n2_b;
  /* optional (NULL = reduce inside the layer call): timhip_layer_ln_partial_bytes() bytes that receive the per-block partial
   * sums of the two LayerNorm parameter gradients (norm2 first, then norm1) INSTEAD of adding them into n*_w / n*_b; the
   * caller reduces the partials of all its layers with one timhip_ln_partials_reduce launch (12 small launches -> 1) */
  float* ln_partials;
} TimLayerGrads;
size_t timhip_layer_ln_partial_bytes(const TimDesc* d);
/* dgamma[i] += column sums of set i's gamma partials, dbeta[i] likewise: nsets sets laid out back to back, each as written by one
 * LayerNorm backward over `rows` rows of `cols` columns; dgamma / dbeta: HOST arrays of nsets device pointers (<= 16) */
int timhip_ln_partials_reduce(const float* partials, int nsets, int rows, int cols, float* const* dgamma,
                              float* const* dbeta, void* stream);

int timhip_version(void);
/* The launchers' A/B knobs (TIMHIP_* environment variables, tim_amd/csrc/common.h: TimKnobs) are read once, at the first
 * launch.  Test hook: read them again after changing the environment inside a process. */
void timhip_reload_env(void);
/* ABI 6 (tests / tools): the row tile of the eight-phase NT kernel (gemm_nt_p8_kernel: 256 x 256 / 320 x 256 tiles for the shapes
 * that run more than one round of 160 x 256 tiles) a plain timhip_gemm_nt launch of this epilogue and shape takes - 8 (256 rows),
 * 10 (320 rows) or 0 (another kernel); follows TIMHIP_GEMM_P8 (0 off, 1 by shape, 8 / 10 forced). */
int timhip_gemm_p8_choice(int epi, int M, int N, int K);
/* bit 0: the library was built with TUNING=1 (carries the measured-slower kernel variants and the ablation hooks) */
int timhip_build_flags(void);
const char* timhip_strerror(int code);

/* bytes of the per-layer saved-for-backward block and of the scratch workspace */
size_t timhip_layer_saved_bytes(const TimDesc* d);
size_t timhip_layer_workspace_bytes(const TimDesc* d);
/* Test hook: byte offset and size of one field of the saved block (opaque to the product's host code).  Fields: the packed
 * in-projection output qkv [M,3E] (T), the attention output o [M,E] (T), the pre-norm sums y1 / y2 [M,E] fp32, the operand copy
 * of norm1's output x1 [M,E] (T), the FFN hidden activations h [M,FF] (T: dropmask * gelu(linear1)), and the FFN dropout
 * keep-bits [M, FF/8] bytes that LayerNorm-1 draws (bit c%8 of byte [r*FF/8 + c/8] = element (r,c) kept; only written when
 * p_drop > 0). */
enum { TIMHIP_SAVED_QKV = 0, TIMHIP_SAVED_O = 1, TIMHIP_SAVED_Y1 = 2, TIMHIP_SAVED_X1T = 3, TIMHIP_SAVED_H = 4,
       TIMHIP_SAVED_Y2 = 5, TIMHIP_SAVED_FFN_KEEP_BITS = 6, TIMHIP_SAVED_ATTN_KEEP_BITS = 7 };
int timhip_layer_saved_field(const TimDesc* d, int field, size_t* offset, size_t* bytes);

/* ---------------------------------------------------------------- weights ---- */
/* dst[rows, ld] (T) = cast(src[rows, cols] fp32), zero padded to ld columns.
 * transpose != 0: dst[cols, ld] = src^T.  ld % 64 == 0. */
int timhip_cast_weight(int precision, const float* src, int rows, int cols, void* dst, int ld,
                       int transpose, void* stream);

/* both operand copies of one fp32 weight [rows, cols] in a single pass:
 * plain[rows, ldp] = cast(src), tr[cols, ldt] = cast(src^T), zero padded; ldp, ldt multiples of 64 */
int timhip_cast_weight_both(int precision, const float* src, int rows, int cols, void* plain, int ldp,
                            void* tr, int ldt, void* stream);

/* the same for n weights in one launch (the refresh of every operand copy after an optimizer step);
 * items is a HOST array, copied into the kernel arguments */
typedef struct TimCastItem {
  const float* src; /* fp32 master [rows, cols], 16-byte aligned */
  void* plain;      /* [rows, ldp] */
  void* tr;         /* [cols, ldt] */
  int32_t rows, cols, ldp, ldt;
} TimCastItem;
int timhip_cast_weights(int precision, const TimCastItem* items, int n, void* stream);

/* ---------------------------------------------------------------- optimizer step ---- */
/* The tail of a training iteration - clip_grad_norm_ -> AdamW -> operand copies of the updated weights (the reference's
 * recognition/scripts/train.py:351-363) - as device-side passes over a table of parameters.  Every scalar that changes from
 * step to step lives in a STATE BLOCK in device memory (TIMHIP_OPT_STATE_WORDS 32-bit words, zero before the first step
 * except the learning rate), never in a launch argument, so a captured step replays correctly:
 *   [STEP]  uint32  updates applied so far (t of the bias corrections)          [LR]       float  learning rate (input)
 *   [NORM]  float   total gradient norm of the latest step, before clipping     [COEF]     float  min(1, max_norm / (norm + 1e-6))
 *   [FOUND_INF] uint32  1: the latest step was skipped                          [SKIPPED]  uint32 steps skipped so far
 *   [BC1]   float   1 - beta1^t                                                 [BC2_SQRT] float  sqrt(1 - beta2^t)
 * One step = timhip_optim_norm over every table that shares the clip, ONE timhip_optim_finish, timhip_optim_update per table. */
enum { TIMHIP_OPT_STEP = 0, TIMHIP_OPT_LR = 1, TIMHIP_OPT_NORM = 2, TIMHIP_OPT_COEF = 3, TIMHIP_OPT_FOUND_INF = 4,
       TIMHIP_OPT_SKIPPED = 5, TIMHIP_OPT_BC1 = 6, TIMHIP_OPT_BC2_SQRT = 7 };
#define TIMHIP_OPT_STATE_WORDS 8

typedef struct TimOptItem {
  float* p;       /* fp32 master [rows, cols], contiguous (a 1-D tensor: rows = 1); any 4-byte aligned start */
  const float* g; /* its gradient, same shape; read, never rescaled in memory (the clip lives in [COEF]) */
  float* m;       /* exp_avg */
  float* v;       /* exp_avg_sq */
  void* plain;    /* operand-dtype copy [rows, ldp] of the updated master, or NULL; plain and tr are given together */
  void* tr;       /* ... and its transpose [cols, ldt] (TimCastItem's meaning: 16-byte aligned, ldp / ldt multiples of 64) */
  int32_t rows, cols, ldp, ldt;
} TimOptItem;

/* Number of partial sums (doubles) timhip_optim_norm writes for this table, or a TIMHIP_E* code (< 0).  items: HOST array,
 * any length (the launches take it 48 items at a time in their kernel arguments). */
int timhip_optim_norm_partials(const TimOptItem* items, int n);

/* partials[0 .. timhip_optim_norm_partials(items, n)) = per-block sums of g^2 over the table.  No atomics: the result depends
 * on the table alone. */
int timhip_optim_norm(const TimOptItem* items, int n, double* partials, void* stream);

/* One block finishes the step's scalars: norm = sqrt(sum of the partials, fixed order); found_inf = the norm is inf / nan, or
 * any of the n_flags <= 32 device words flags[i] is non-zero (HOST array of device pointers: the out[4] words of the backward's
 * timhip_grad_scale blocks); coef as above (max_norm <= 0: no clipping, the norm is still reported).  Then, for each of the
 * n_states <= 8 state blocks (HOST array of device pointers; beta1 / beta2: HOST arrays, one pair per block): NORM, COEF,
 * FOUND_INF are written, and either SKIPPED += 1 (found_inf) or STEP += 1 with BC1 / BC2_SQRT of the new step. */
int timhip_optim_finish(const double* partials, int n_partials, const uint32_t* const* flags, int n_flags, float max_norm,
                        float* const* states, const double* beta1, const double* beta2, int n_states, void* stream);

/* AdamW on g * COEF, torch's arithmetic in fp32, with lr and the bias corrections read from `state`:
 *   p *= 1 - lr * weight_decay;  m = beta1 m + (1 - beta1) g;  v = beta2 v + (1 - beta2) g g;
 *   p -= (lr / BC1) * m / (sqrt(v) / BC2_SQRT + eps)
 * Returns at once, touching nothing, when state[FOUND_INF] is set.  Items with copies: the block that updates a 64 x 64 tile
 * also writes plain[r, c] and tr[c, r] = the updated value in the operand dtype of `precision` - the bits timhip_cast_weights
 * would produce from the updated master; padding columns (c >= cols, r >= rows) are left as they are. */
int timhip_optim_update(int precision, const TimOptItem* items, int n, const float* state, double beta1, double beta2,
                        double eps, double weight_decay, void* stream);

/* ---------------------------------------------------------------- generic ops (also unit-test hooks) */
typedef struct TimEpi {
  void* out0;
  void* out1;
  const float* bias;
  const float* res;
  const void* aux;
  int32_t ld0, ld1, ldres, ldaux;
  float p_drop;
  uint32_t site;   /* Philox stream id of the dropout site */
  uint64_t seed;
  const void* mask; /* optional: the site's keep-bits drawn ahead of time (bit c%8 of byte [r*ldmask + c/8] = element (r,c)
                       kept; what timhip_layer_fwd has LayerNorm-1 write for the FFN dropout).  NULL: drawn in the epilogue */
  int32_t ldmask;   /* row stride of mask in bytes */
  int32_t reserved; /* 0, or the operand replication factor of a split-operand product (3 for timhip_split3_many operands):
                       only divides the FLOP count the timing hooks attribute to the launch */
  /* TIMHIP_EPI_DROP_RES_F32 only, optional: the residual is LayerNorm(res).  res then holds the PRE-norm fp32 rows, ln_stats
   * the (mean, rstd) pair of every row as timhip_layernorm_fwd writes them, ln_w / ln_b the affine parameters; the epilogue
   * normalises what it reads, so the normalised fp32 rows need not exist in memory.  NULL: res is used as it is. */
  const float* ln_stats;
  const float* ln_w;
  const float* ln_b;
  /* optional device scalar: the accumulators are multiplied by *acc_scale before the epilogue (NULL = 1).  TIMHIP_PREC_F16
   * keeps its gradient OPERANDS multiplied by a power of two S (timhip_grad_scale); an input-gradient GEMM whose result joins
   * the fp32 gradient stream (TIMHIP_EPI_ADD_F32) passes 1/S here. */
  const float* acc_scale;
  /* optional (0 = off): the A operand has only a_wrap_k columns and is read TWICE along the contraction, K = 2 * a_wrap_k
   * (a multiple of 64; lda >= a_wrap_k): C = [A | A] B^T.  With B = [w_hi | w_lo] (the first two column blocks of a
   * timhip_split3_many mode-0 copy of an fp32 weight) the product carries the weight to ~22 bits at twice the matrix work and
   * no extra activation traffic - what TIMHIP_DESC_OUTPROJ_SPLIT uses.  16-bit precisions only. */
  int32_t a_wrap_k;
  int32_t reserved2;
} TimEpi;

/* n <= 6 independent small problems with the same epilogue as ONE launch (bf16; TIMHIP_EPI_STORE_F32, _ADD_F32, _STORE_T,
 * _RELU_T): what the classification heads use - four under-filled GEMMs each way (head.py:17-38).  items is a HOST array. */
typedef struct TimGemmItem {
  const void* A; const void* B;
  int32_t lda, ldb, M, N, K, reserved;   /* reserved: as TimEpi.reserved */
  TimEpi e;
} TimGemmItem;
int timhip_gemm_nt_group(int precision, int epi, const TimGemmItem* items, int n, void* stream);

/* C[M,N] = A[M,K] * B[N,K]^T through epilogue `epi` (TIMHIP_EPI_*).  A, B operand dtype,
 * lda/ldb multiples of 64 and >= K.  splitk > 1 only with TIMHIP_EPI_ATOMIC_F32. */
int timhip_gemm_nt(int precision, int epi, const void* A, int lda, const void* B, int ldb, int M,
                   int N, int K, const TimEpi* e, int splitk, void* stream);

/* dst[cols, ld] (T) = src[rows, lds]^T (T); pad columns rows..ld are zeroed.  */
int timhip_transpose(int precision, const void* src, int rows, int cols, int lds, void* dst, int ld,
                     void* stream);

/* out[n] += sum_m src[m, n]  (T source of row stride ld >= cols, fp32 accumulate): bias gradients.  ACCUMULATED: every block of 64
 * rows ends in one float atomicAdd per column, so `out` keeps what it held (the caller zeroes it for a plain sum) and the order of
 * the additions - the last bits of the result - is not fixed. */
int timhip_colsum(int precision, const void* src, int rows, int cols, int ld, float* out,
                  void* stream);

/* Split operands: src_i [rows_i, cols_i] fp32 (row stride lds_i) -> dst_i [rows_i, ldd_i] (T = bf16 / fp16), ldd_i = 3 * block
 * width, block width = cols_i rounded up to a multiple of 64 (zero padded).  With hi = T(x), lo = T(x - hi) the three column
 * blocks are [hi | lo | hi] (mode 0: activations; relu != 0 applies max(x, 0) first) or [hi | hi | lo] (mode 1: weights), so a
 * 16-bit NT GEMM of a mode-0 matrix with a mode-1 matrix over K = ldd computes x w^T to ~22 bits (x_hi w_hi + x_lo w_hi +
 * x_hi w_lo).  count <= 6 matrices per launch; HOST arrays.  What TIMHIP_PREC_F16 models use for the time MLP and the
 * classification heads (the two small sites that dominate the 16-bit error budget). */
int timhip_split3_many(int precision, int count, const float* const* src, const int* rows, const int* cols, const int* lds,
                       void* const* dst, const int* ldd, int mode, int relu, void* stream);

/* Data-parallel gradient exchange (tim_amd/dp.py; replaces the DistributedDataParallel wrap of models/build.py:58-63): after
 * the all-to-all, recv [world][per] (bf16 if wire_bf16 else fp32) holds this rank's chunk of every rank's bucket;
 * out[per] (same dtype) = scale * sum over ranks, accumulated in fp32.  per % 4 == 0, 16-byte aligned buffers. */
int timhip_dp_reduce(int wire_bf16, const void* recv, int world, long long per, float scale, void* out, void* stream);

/* Gradient scale of the fp16 mode.  fp16 has 5 exponent bits: gradient operands would underflow (the reference's GPU recipe
 * wraps its step in a GradScaler for that reason, recognition/scripts/train.py:82,355-363).  Here the scale is chosen per
 * backward pass ON THE DEVICE from the cotangents entering it: S = 2^floor(log2(target / max|cot|)), out[0] = S,
 * out[1] = 1/S (S = 1 when every cotangent is 0).  cot / counts: HOST arrays of n <= 8 device pointers / element counts;
 * out: 8 floats in device memory, out[2..7] zero before the first call (out[2..3] scratch, left zero).  One launch, no host sync.
 *
 * NON-FINITE WATCH (out[4], read as uint32): every entry point below that takes `out_scale` expects NULL or &out[1] of such a
 * block, multiplies what it writes by out[1] = 1/S, and ORs 1 into out[4] when a FINAL fp32 gradient it writes is inf or nan
 * (timhip_wgrad, timhip_wgrad_group, timhip_time_l1_bwd - every weight / bias gradient of the fp16 backward).  An overflow of
 * a 16-bit gradient operand anywhere in the chain reaches every weight gradient upstream of it, so the flag is what the
 * reference's GradScaler inf check computes (recognition/scripts/train.py:351,357-363: skip the step, halve the scale)
 * without a pass over the gradients and without a host synchronisation until somebody reads the word. */
int timhip_grad_scale(const float* const* cot, const long long* counts, int n, float target, float* out, void* stream);

/* fp32 -> T with optional dropout (p_drop > 0) and zero padding to ld; scale: optional device scalar multiplied in */
int timhip_cast_rows(int precision, const float* src, int rows, int cols, int lds, void* dst, int ld,
                     float p_drop, uint64_t seed, uint32_t site, const float* scale, void* stream);
/* timhip_cast_rows for TWO contiguous fp32 matrices with the same row count in one launch of the same kernel (the two embedders'
 * inputs: widths cols[i], operand rows of stride ld[i], dropout site sites[i]; same masks as two timhip_cast_rows calls) */
int timhip_cast_rows_pair(int precision, const float* const* src, const int* cols, void* const* dst, const int* ld, int rows,
                          float p_drop, uint64_t seed, const uint32_t* sites, void* stream);

/* LayerNorm over the last dim of act(y): x = LN(act(y)) * w + b.
 * act: 0 none, 1 relu, 2 gelu(erf).  Writes x_f32 (may be null, row stride ldx, column
 * offset already applied by the caller), x_T (may be null, ld ldt) and stats[rows,2]=(mean,rstd).
 * p_drop>0 applies (sequence) dropout to the outputs. */
int timhip_layernorm_fwd(int precision, const float* y, int rows, int cols, int ldy, int act,
                         const float* w, const float* b, float* x_f32, int ldx, void* x_T, int ldt,
                         float* stats, void* stream);
/* dy = LN'(dx) (through act'); dgamma += , dbeta +=.  dy_f32 (may be null) and
 * dy_T = dropmask(site) * dy (may be null). */
int timhip_layernorm_bwd(int precision, const float* dx, int lddx, const float* y, int ldy,
                         const float* stats, int rows, int cols, int act, const float* w,
                         float* dy_f32, int lddy, void* dy_T, int ldt, float p_drop, uint64_t seed,
                         uint32_t site, float* dgamma, float* dbeta, const float* t_scale, void* stream);
/* Two LayerNorms of the same width and activation over STACKED rows in one launch (round 5: the two modality embedders,
 * encodings.py:21-26): rows [0, split_row) use (w, b), rows from split_row on (w2, b2); in the backward the parameter gradients of
 * the two halves go to (dgamma, dbeta) and (dgamma2, dbeta2) - accumulated, the caller zeroes them - and split_row must be a
 * multiple of 16 (a block of the backward owns 16 consecutive rows).  Everything else as timhip_layernorm_fwd / _bwd. */
int timhip_layernorm_fwd2(int precision, const float* y, int rows, int cols, int ldy, int act, const float* w, const float* b,
                          int split_row, const float* w2, const float* b2, float* x_f32, int ldx, void* x_T, int ldt, float* stats,
                          void* stream);
int timhip_layernorm_bwd2(int precision, const float* dx, int lddx, const float* y, int ldy, const float* stats, int rows, int cols,
                          int act, const float* w, int split_row, const float* w2, float* dy_f32, int lddy, void* dy_T, int ldt,
                          float* dgamma, float* dbeta, float* dgamma2, float* dbeta2, const float* t_scale, void* stream);

/* structured attention over qkv[B*S, 3E] (T): token i attends to the F feature tokens and to
 * itself.  o[B*S,E] (T), lse[B,H,S] fp32 (only the backward reads it: NULL skips the store). */
int timhip_attention_fwd(const TimDesc* d, const void* qkv, void* o, float* lse, void* stream);
/* The same for the token rows s0 <= s < S of every window only, written compactly: o_rows[b * (S - s0) + (s - s0), :] (T).  Keys
 * and values still come from the full qkv; no lse, no dropout (d->p_drop must be 0: TIMHIP_EINVAL).  Every row goes through the
 * arithmetic of the full kernel in the same key order - the rows of o_rows equal rows s0 .. S - 1 of timhip_attention_fwd's o
 * bit for bit; 32-row blocks that lie wholly below s0 are not run.  With s0 = F: the query rows, all the last layer of an
 * evaluation forward needs once nobody reads `feats` (timhip_stack_infer, tail_only). */
int timhip_attention_fwd_rows(const TimDesc* d, const void* qkv, int s0, void* o_rows, void* stream);
/* Query rows against keys and values kept elsewhere (evaluation only; d->p_drop must be 0: TIMHIP_EINVAL).  d: B = G groups, S = Q
 * rows per group, F = keys per window, E, H.  qkv_q [G Q, 3E] (T): q | own k | own v of the query rows.  kv: the K columns of row 0
 * of window 0; V lies E elements behind K in the same row; ldkv: row pitch in elements (>= 2E); wrows: rows from one window to the
 * next (>= F); W: windows.  A compact cache is ldkv = 2E, wrows = F; the qkv of timhip_attention_fwd is read in place with
 * kv = qkv + E, ldkv = 3E, wrows = S.  widx (device, G ints; NULL: group g reads window g, G == W required - else TIMHIP_EINVAL).
 * Every row runs the softmax over the F keys of window widx[g] plus its own key: o[g Q + i, :] = sum_j p_j V_j + p_self v_own -
 * the arithmetic of timhip_attention_fwd's kernels (one shared body), so the rows equal that call's query rows bit for bit on
 * equal inputs: the matrix-core kernel for 16-bit precisions and the shapes it is built for, the fp32-arithmetic kernel for
 * everything else (fp32 / bf16x3 included: there the equal bits are those of timhip_attention_fwd under TIMHIP_DESC_ATTN_FP32).
 * A widx[g] outside [0, W): nothing is read through it and the group's o rows are quiet NaNs. */
int timhip_attention_query_fwd(const TimDesc* d, const void* qkv_q, const void* kv, int ldkv, int wrows, int W, const int* widx,
                               void* o, void* stream);
/* The attention WEIGHTS of those rows - what the reference's TransformerEncoder.forward returns beside its output (transformers.py:
 * 45-48: nn.MultiheadAttention's head-averaged softmax weights) and the kernels above keep in registers.  A token attends to the F
 * feature tokens and to itself, so a row has F + 1 entries: w[b * (S - s0) + (s - s0), j] (fp32, row pitch ld >= F + 1 floats;
 * columns past F are not written) = the mean over the heads, in ascending head order, of softmax_j(scale q[b,h,s] . k[b,h,key(j)]),
 * key(j) = j for j < F; column F = the token's own key for query rows (s >= F) and exact 0.0f for feature rows, whose own key is
 * one of the F.  per_head != 0: no mean, w is [B, H, S - s0, ld].  Keys come from the full qkv (the matrix timhip_attention_fwd
 * reads); the softmax is computed here, no lse is read.  No dropout: d->p_drop must be 0 (the reference's weights under dropout
 * are a mask, not a map).  A row's arithmetic depends on neither B nor s0: the same window gives the same bits alone or in any
 * batch, on every run (no atomics).  16-bit precisions run Q K^T on the matrix cores for the shapes timhip_attention_fwd does;
 * every other shape, the fp32-storage modes and TIMHIP_DESC_ATTN_FP32 run one fp32-arithmetic kernel (F <= 192, else
 * TIMHIP_EUNSUPPORTED).  Checked before any launch: NULL d / qkv / w, a bad descriptor, p_drop != 0, s0 outside [0, S),
 * ld < F + 1 - TIMHIP_EINVAL; w not float-aligned (qkv not element-aligned) - TIMHIP_EALIGN. */
int timhip_attention_weights(const TimDesc* d, const void* qkv, int s0, int per_head, float* w, int ld, void* stream);
/* The attention weights of query rows against keys kept elsewhere: timhip_attention_weights for the rows and the key source of
 * timhip_attention_query_fwd.  d, qkv_q, kv, ldkv, wrows, W, widx: as there (B = G groups, S = Q rows per group, F = keys per
 * window; only the K columns of the cache are read).  w[g Q + i, j] (fp32, row pitch ld >= F + 1 floats; columns past F are not
 * written), 0 <= j <= F: the mean over the heads, in ascending head order, of softmax_j(scale q . k_key(j)), key(j) = key j of
 * window widx[g] for j < F, column F the row's own key.  per_head != 0: no mean, w is [G, H, Q, ld].  The kernels are
 * timhip_attention_weights' own bodies with another key source (lane pair per row on the matrix cores for the head widths and
 * key-block counts timhip_attention_fwd covers, under the alignment timhip_attention_query_fwd asks of its matrix-core route;
 * a wave per row in fp32 arithmetic for every other shape, the fp32-storage modes and TIMHIP_DESC_ATTN_FP32), so on equal q and
 * K values the rows equal timhip_attention_weights' query rows (s0 = F) bit for bit - on every row whose largest raw score m
 * has |m scale log2(e)| < 2^30; rows beyond that (raw scores near the largest finite bf16 / fp32 value, where the rounding error
 * of that product is no exponent exp2 can take and timhip_attention_weights is not finite) use exp2((score - m) scale log2(e))
 * and stay finite.  No atomics: a row's bits depend on neither
 * G, nor the row's place in a block, nor the other groups of the launch.  A widx[g] outside [0, W): nothing is read through it
 * and columns 0 .. F of the group's rows are quiet NaNs.  Checked before any launch: NULL d / qkv_q / kv / w, a bad descriptor,
 * p_drop != 0, W <= 0, NULL widx with G != W, ld < F + 1, ldkv < 2E, wrows < F - TIMHIP_EINVAL; F > 192 - TIMHIP_EUNSUPPORTED; w
 * not float-aligned, qkv_q / kv not element-aligned - TIMHIP_EALIGN. */
int timhip_attention_query_weights(const TimDesc* d, const void* qkv_q, const void* kv, int ldkv, int wrows, int W,
                                   const int* widx, int per_head, float* w, int ld, void* stream);
/* ABI 6: keep-bits of the attention dropout of `nlayers` encoder layers in ONE launch, written into the layers' saved blocks
 * (saved[l] = the block timhip_layer_fwd of layer l will fill; field TIMHIP_SAVED_ATTN_KEEP_BITS: per (window, head, token row)
 * two 64-bit words, word g bit 4 c + t = key 8 c + 4 g + t kept, keys 0 .. 127 - the order in which the MFMA attention
 * kernels' lanes own keys).  The same Philox stream as the kernels' own draws (seed d->seed, site of layer l, element
 * ((b H + h) S + s) LP + key, LP = F + 1 rounded up to 8): results are bit-identical with and without the flag.
 * TIMHIP_EUNSUPPORTED (the caller leaves TIMHIP_DESC_ATTN_KEEP_BITS off): everything but 16-bit precisions with 128-wide heads and
 * 97 .. 128 feature keys (the geometry whose kernels read the bits), and evaluation mode (p_drop = 0). */
int timhip_attn_keep_bits(const TimDesc* d, int nlayers, void* const* saved, void* stream);
/* Backward of timhip_attention_fwd: dqkv[B*S, 3E] (T) from d_o[B*S, E] (T), with the forward's qkv, o and lse.  16-bit precisions run
 * the matrix-core kernels (fused, or rows + keys through the workspace) for head widths 128 / 64 / 32 with E a multiple of 8 and
 * B * H <= 65535; every other shape - a 16-bit backward with B * H > 65535 included - runs the fp32-arithmetic kernel, as under
 * TIMHIP_DESC_ATTN_FP32.  workspace: timhip_attention_bwd_workspace_bytes (TIMHIP_EWORKSPACE if smaller). */
int timhip_attention_bwd(const TimDesc* d, const void* qkv, const void* o, const float* lse,
                         const void* d_o, void* dqkv, void* workspace, size_t workspace_bytes,
                         void* stream);
size_t timhip_attention_bwd_workspace_bytes(const TimDesc* d);
/* timhip_attention_bwd handed the keep-bits of the layer's attention dropout (timhip_attn_keep_bits' words, [B * H * S][2], 16-byte
 * aligned; NULL: exactly timhip_attention_bwd), as the layer backward hands them to it: the fused kernels of the geometry that call
 * serves read the bits instead of drawing the mask themselves; every other kernel ignores them.  The same results, bit for bit. */
int timhip_attention_bwd_keep_bits(const TimDesc* d, const void* qkv, const void* o, const float* lse, const void* d_o, void* dqkv,
                                   void* workspace, size_t workspace_bytes, const void* keep_bits, void* stream);

/* dW[Nout,Kout] += dY[M,Nout]^T X[M,Kout] and (db != NULL) db[Nout] += colsum(dY): weight/bias
 * gradients of one nn.Linear.  workspace (timhip_wgrad_workspace_bytes) holds the transposed
 * operand copies and the split-K fp32 partial slabs. */
size_t timhip_wgrad_workspace_bytes(int precision, int Nout, int Kout, int M);
int timhip_wgrad(int precision, const void* dY, int ldy, int Nout, const void* X, int ldx, int Kout,
                 int M, float* dW, float* db, void* workspace, size_t workspace_bytes, const float* out_scale, void* stream);

/* The same for n <= 8 Linear layers that share M (the four of one encoder layer), as ONE launch: their tile lists are
 * concatenated and the number of splits of the contraction is chosen for the total - at E = 1024, FF = 2048 the layer has
 * exactly 512 tiles = the chip's 512 block slots, the contraction is not split and dW / db are written directly, with no
 * partial slabs and no reduce.  accumulate = 0 writes dW / db instead of adding to them.  bf16 operands only (the fp32 and
 * bf16x3 modes go through timhip_wgrad); every Nout*Kout must be a multiple of 4.  items is a HOST array, copied into the
 * kernel arguments.  workspace may be NULL when timhip_wgrad_group_workspace_bytes returns 0.
 * Alignment, one rule for every kernel the group may run on (the plain tiles, the ping-pong grid, the eight-phase grid): ldy and
 * ldx multiples of 8 elements, dY, X and dW 16-byte aligned - otherwise TIMHIP_EALIGN.  The whole group is checked on the host
 * BEFORE any launch: a refused group has written nothing, whichever item was at fault.  A group that one of the tiled grids
 * cannot address (M * ld * 2 bytes >= 2^32) runs on the plain tiles instead of being refused. */
typedef struct TimWgradItem {
  const void* dY;   /* [M, ldy] */
  const void* X;    /* [M, ldx] */
  float* dW;        /* [Nout, Kout] */
  float* db;        /* [Nout] or NULL */
  int32_t ldy, ldx, Nout, Kout;
} TimWgradItem;
size_t timhip_wgrad_group_workspace_bytes(int precision, const TimWgradItem* items, int n, int M);
int timhip_wgrad_group(int precision, const TimWgradItem* items, int n, int M, int accumulate, void* workspace,
                       size_t workspace_bytes, const float* out_scale, void* stream);

/* dx[r,c] = g[r,c] * keep-mask/(1-p): backward of the feature dropout applied by timhip_cast_rows */
int timhip_dropout_rows_bwd(const float* g, int rows, int cols, int ldg, float* dx, int ldx,
                            float p_drop, uint64_t seed, uint32_t site, void* stream);

/* time MLP layer 1 (K = 2, tim.py:67): h[r,j] = relu(t[r,0] w[j,0] + t[r,1] w[j,1] + b[j]) (T, ld) */
int timhip_time_l1_fwd(int precision, const float* times, int rows, int d, const float* w,
                       const float* b, void* h, int ld, void* stream);
/* The same with the row written as the split operand [hi | lo | hi] of the fp32 value (three 16-bit column blocks of width ld, a
 * multiple of 64; row stride 3 ld; 16-bit modes): what timhip_split3_many (mode 0) makes of the fp32 output, without the fp32
 * round trip and the second launch. */
int timhip_time_l1_fwd_split3(int precision, const float* times, int rows, int d, const float* w, const float* b, void* h3,
                              int ld, void* stream);
/* dh: gradient w.r.t. the pre-activation of layer 1 (T).  dw[d,2] +=, db[d] +=, dt[rows,2] = (may be NULL) */
int timhip_time_l1_bwd(int precision, const float* times, int rows, int d, const float* w,
                       const void* dh, int ld, float* dw, float* db, float* dt, const float* out_scale, void* stream);

/* keep-mask (1/0 bytes) of a dropout site, as the kernels generate it: test hook.  Element (r, c) has linear index
 * r * cols + c; one Philox-4x32-7 call (key = seed, stream = site, counter = index / 8) decides 8 consecutive elements by its
 * eight 16-bit halves: kept iff halfword >= floor(p * 65536). */
int timhip_dropout_mask(uint64_t seed, uint32_t site, float p, int rows, int cols, uint8_t* out,
                        void* stream);

/* Graph-safe dropout.  Every entry point that takes a `seed` passes it to its kernels by value, so a step captured in a
 * HIP graph would replay the masks of the captured step.  After timhip_dropout_salt(p) (p: one 64-bit word in device
 * memory, owned by the caller, alive while registered) every dropout kernel launched from this library draws with
 * seed + *p, read on the device when the kernel runs: bump the word between replays (or with a node inside the graph) and
 * forward and backward of one replay still agree.  NULL restores plain launch-time seeds.  Process-wide (one process per
 * GPU).  The reference has no counterpart: torch's CUDA-graph-safe Philox offsets play this role there. */
int timhip_dropout_salt(const unsigned long long* dev_salt);

/* ---------------------------------------------------------------- stages ---- */
/* One post-norm encoder layer.  x_in (fp32 [M,E]) and x_in_T (T [M,E]) are the layer input,
 * x_out / x_out_T the output.  `saved` (timhip_layer_saved_bytes) is read back by the backward.
 * x_out may be NULL when nobody reads the fp32 output rows (the next layer then runs timhip_layer_fwd_chained).
 * workspace / workspace_bytes are not used any more (kept for binary compatibility). */
int timhip_layer_fwd(const TimDesc* d, const TimLayerParams* w, const float* x_in,
                     const void* x_in_T, float* x_out, void* x_out_T, void* saved, void* workspace,
                     size_t workspace_bytes, void* stream);
/* The same for a layer that follows another one of the same shape: its fp32 input rows are not read from memory but
 * recomputed where they are needed (the residual of the out-projection epilogue) as LayerNorm-2 of the previous layer's
 * pre-norm rows, taken from prev_saved with prev_w's norm2 parameters; x_in_T is still the previous layer's x_out_T.
 * Together with x_out = NULL on the inner layers the fp32 stream between layers never exists in memory. */
int timhip_layer_fwd_chained(const TimDesc* d, const TimLayerParams* w, const TimLayerParams* prev_w,
                             const void* prev_saved, const void* x_in_T, float* x_out, void* x_out_T, void* saved,
                             void* stream);
/* Evaluation forward of a whole stack of `nlayers` post-norm layers of one shape, out of ONE arena whose size does not depend on
 * nlayers (at most timhip_layer_saved_bytes plus one fp32 and one operand-dtype [B S, E] row buffer): per layer the launches of
 * timhip_layer_fwd / timhip_layer_fwd_chained in evaluation arithmetic (d->p_drop must be 0: TIMHIP_EINVAL), minus the stores
 * only a backward reads - attention without lse, linear1 through TIMHIP_EPI_GELU_T.  The TIMHIP_DESC_*_SPLIT flags of
 * d->reserved are honoured as there.  layers[l]: the parameters of layer l.  x_in (fp32) / x_in_T (T): the [B S, E] input rows.
 *   tail_only = 0: x_out (fp32, may be NULL) and x_out_T (T) are [B S, E] - the values timhip_layer_fwd of the last layer writes.
 *   tail_only = 1: the last layer runs its in-projection on all rows and everything behind it on the B (S - F) query rows only
 *     (timhip_attention_fwd_rows with s0 = F; the residual rows gathered): x_out / x_out_T are compact, [B (S - F), E], row
 *     b (S - F) + (s - F) = token s of window b.  A token's row depends on the feature rows' keys and values and on itself,
 *     so these are the rows tail_only = 0 computes, up to the tiles the GEMMs pick at the smaller row count.  S == F: TIMHIP_EINVAL.
 * TIMHIP_EWORKSPACE when workspace_bytes < timhip_stack_infer_workspace_bytes(d, nlayers, tail_only).  Launches only: one stream,
 * no events - capturable as a linear graph. */
size_t timhip_stack_infer_workspace_bytes(const TimDesc* d, int nlayers, int tail_only);
int timhip_stack_infer(const TimDesc* d, int nlayers, const TimLayerParams* layers, const float* x_in, const void* x_in_T,
                       float* x_out, void* x_out_T, int tail_only, void* workspace, size_t workspace_bytes, void* stream);
/* timhip_stack_infer that also writes attention maps: behind layer l's launches, while that layer's qkv is live in the arena,
 * timhip_attention_weights (mean over heads, rows maps_s0 .. S - 1, row pitch ld) into maps[l].  maps: a HOST array of nlayers
 * device pointers, read during the call only; NULL entries are skipped.  With tail_only = 1 the last layer still computes qkv on
 * all rows, so maps_s0 = F (the query rows) and maps_s0 = 0 both work there.  The arena is timhip_stack_infer's, whatever
 * the number of maps: the maps are the caller's buffers.  x_out / x_out_T are timhip_stack_infer's bit for bit (the same launches
 * in the same order; the weights kernels only read).  Launches only, one stream, no events, no host reads of device memory:
 * capturable as a linear graph.  maps == NULL, maps_s0 outside [0, S), ld < F + 1: TIMHIP_EINVAL; a map that is not float-aligned:
 * TIMHIP_EALIGN - all before the first launch. */
size_t timhip_stack_infer_maps_workspace_bytes(const TimDesc* d, int nlayers, int tail_only);
int timhip_stack_infer_maps(const TimDesc* d, int nlayers, const TimLayerParams* layers, const float* x_in, const void* x_in_T,
                            float* x_out, void* x_out_T, int tail_only, float* const* maps, int maps_s0, int ld,
                            void* workspace, size_t workspace_bytes, void* stream);
/* ---- encode a window once, query it many times (evaluation only) ----
 * Under TIM's mask the feature rows of a window never read a query row, and a query row reads the F feature rows' keys and values
 * plus its own: the stack can run on the feature rows alone, keep every layer's K | V columns, and later run any number of query
 * rows against them.
 *
 * timhip_stack_encode: timhip_stack_infer (tail_only = 0) on feature rows only - d: B = W windows, S = F.  x_in / x_in_T: the
 * [W F, E] assembled feature rows.  Behind layer l's launches the K | V columns of its qkv are copied (one pitched device copy per
 * layer: 2/3 of qkv read and written) into cache + l * W F 2E elements: cache is [nlayers][W F][2 E] in the operand dtype,
 * timhip_window_cache_bytes(d, nlayers) bytes (0 for a descriptor the call refuses), 16-byte aligned (TIMHIP_EALIGN).
 * feats_out (fp32 [W F, E], may be NULL): the last layer's output rows - the `feats` of a full forward.  S != F, NULL cache:
 * TIMHIP_EINVAL.  workspace: timhip_stack_infer_workspace_bytes(d, nlayers, 0).
 *
 * timhip_stack_query: all nlayers layers on query rows only - d: B = G groups, S = Q query rows per group, F = the cached keys per
 * window (Q < F is fine).  Group g reads window widx[g] of the W cached ones (widx: device, G entries; NULL: window g, G == W
 * required).  Per layer: in-projection of the G Q rows (q | own k | own v), timhip_attention_query_fwd against cache block l,
 * out-projection + residual, LayerNorm, FFN, LayerNorm as timhip_stack_infer chains them.  xq_in / xq_in_T: the [G Q, E] assembled
 * query rows; xq_out (fp32, may be NULL) / xq_out_T (T): the last layer's rows - what a full forward computes for these tokens, up
 * to the tiles the GEMMs pick at this row count.  workspace: timhip_stack_query_workspace_bytes(d, nlayers), one layer's arena for
 * G Q rows.  Refused before the first launch: NULL pointers, p_drop != 0, W <= 0, NULL widx with G != W - TIMHIP_EINVAL; F > 192 -
 * TIMHIP_EUNSUPPORTED; a short workspace - TIMHIP_EWORKSPACE.  An entry of widx outside [0, W) is not an error the host can see:
 * that group's rows come out as NaN and nothing is read through the index (timhip_attention_query_fwd).
 * Both: launches and device copies only, one stream, no events, no allocation - capturable as a linear graph. */
size_t timhip_window_cache_bytes(const TimDesc* d, int nlayers);
int timhip_stack_encode(const TimDesc* d, int nlayers, const TimLayerParams* layers, const float* x_in, const void* x_in_T,
                        float* feats_out, void* cache, void* workspace, size_t workspace_bytes, void* stream);
size_t timhip_stack_query_workspace_bytes(const TimDesc* d, int nlayers);
int timhip_stack_query(const TimDesc* d, int nlayers, const TimLayerParams* layers, const void* cache, int W, const int* widx,
                       const float* xq_in, const void* xq_in_T, float* xq_out, void* xq_out_T, void* workspace,
                       size_t workspace_bytes, void* stream);
/* timhip_stack_query that also writes attention maps: behind layer l's launches, while that layer's in-projection of the query
 * rows (q | own k | own v) is live in the arena, timhip_attention_query_weights against cache block l into maps[l] - [G Q, ld]
 * fp32, or [G, H, Q, ld] with per_head != 0.  maps: a HOST array of nlayers device pointers, read during the call only; NULL
 * entries are skipped.  xq_out / xq_out_T are timhip_stack_query's bit for bit (the same launches in the same order; the weights
 * kernels only read).  The arena is timhip_stack_query's, the maps are the caller's buffers.  Launches only, one stream, no
 * events, no host read of device memory: capturable as a linear graph.  timhip_stack_query's refusals, and maps == NULL,
 * ld < F + 1: TIMHIP_EINVAL; a map that is not float-aligned: TIMHIP_EALIGN - all before the first launch. */
size_t timhip_stack_query_maps_workspace_bytes(const TimDesc* d, int nlayers);
int timhip_stack_query_maps(const TimDesc* d, int nlayers, const TimLayerParams* layers, const void* cache, int W, const int* widx,
                            const float* xq_in, const void* xq_in_T, float* xq_out, void* xq_out_T, float* const* maps,
                            int per_head, int ld, void* workspace, size_t workspace_bytes, void* stream);
/* dx_out: gradient w.r.t. the layer output (fp32 [M,E]).  dx_in: gradient w.r.t. the
 * layer input (fp32 [M,E]).  Parameter gradients are accumulated (+=) into *g.
 * This is timhip_layer_bwd_split (below: the form tim_amd calls) with dx_out_add = dx_in_add = NULL. */
int timhip_layer_bwd(const TimDesc* d, const TimLayerParams* w, const void* x_in_T,
                     const void* saved, float* dx_out, float* dx_in, const TimLayerGrads* g,
                     void* workspace, size_t workspace_bytes, void* stream);

/* Two-stream form of the layer backward.  The data chain (LayerNorm / GELU / attention backward and
 * the input-gradient GEMMs) produces dx_in and leaves the four gradient operands df, du, da, dqkv in
 * `dy` (timhip_layer_dy_bytes); the weight-gradient part consumes `dy` and the saved activations and
 * may be enqueued on a second stream so that it overlaps the data chain of the next layer
 * (the caller orders the two streams with events).  LayerNorm gradients are written by the data chain,
 * all other parameter gradients by the weights part.  timhip_layer_bwd_data is timhip_layer_bwd_data_split (below: the form
 * tim_amd calls) with dx_out_add = dx_in_add = NULL. */
size_t timhip_layer_dy_bytes(const TimDesc* d);
size_t timhip_layer_data_workspace_bytes(const TimDesc* d);
size_t timhip_layer_wgrad_workspace_bytes(const TimDesc* d);
int timhip_layer_bwd_data(const TimDesc* d, const TimLayerParams* w, const void* saved, float* dx_out,
                          float* dx_in, void* dy, const TimLayerGrads* g, void* workspace,
                          size_t workspace_bytes, void* stream);
int timhip_layer_bwd_weights(const TimDesc* d, const void* x_in_T, const void* saved, const void* dy,
                             const TimLayerGrads* g, void* workspace, size_t workspace_bytes,
                             void* stream);
/* Round 6: the weight gradients of TWO layers (a, b: the arguments of timhip_layer_bwd_weights for each) as one grouped launch.
 * A C2a layer's four products (transformers.py:73,102,107 under autograd) are 128 tiles of 256 x 256: two layers fill the 256
 * CUs with one tile each, every block running the whole contraction.  timhip_layer_wgrad_pair_wins(d) = 1 when that is the
 * case for this descriptor - then a host defers a layer's weight gradients until its neighbour's data chain has run (each
 * layer's `dy` block and saved activations stay untouched until the pair call) - 0 otherwise (pairing gains nothing; the pair
 * call may then return TIMHIP_EWORKSPACE, its workspace being sized for one layer). */
int timhip_layer_bwd_weights_pair(const TimDesc* d, const void* x_in_T_a, const void* saved_a, const void* dy_a,
                                  const TimLayerGrads* ga, const void* x_in_T_b, const void* saved_b, const void* dy_b,
                                  const TimLayerGrads* gb, void* workspace, size_t workspace_bytes, void* stream);
int timhip_layer_wgrad_pair_wins(const TimDesc* d);

/* Split gradient stream between layers (optional, what tim_amd/functional.py uses inside the stack).  The gradient of a layer
 * boundary travels as an fp32 part plus an operand-dtype part: dx = dx_f32 + (1/S) * dx_add, S the fp16 gradient scale of
 * TimDesc.grad_scale (1 in the other modes).  dx_out_add (may be NULL: the gradient entering the stack is plain fp32) is added
 * by the layer's norm2 backward as it reads its input; with dx_in_add != NULL the layer leaves its input gradient in the same
 * split form - dx_in receives norm1's fp32 output gradient, dx_in_add [M,E] (T) the in-projection's input-gradient product -
 * for the next call's dx_out / dx_out_add; with dx_in_add == NULL dx_in is the complete fp32 gradient (as timhip_layer_bwd).
 * Inside the layer the FFN branch's input gradient is handed to norm1's backward the same way.  The "+ residual" epilogues of
 * the two N = E input-gradient GEMMs disappear: they store 2 bytes per element instead of reading 4 and writing 4.  dx_out is
 * NOT clobbered by these forms. */
int timhip_layer_bwd_split(const TimDesc* d, const TimLayerParams* w, const void* x_in_T, const void* saved, const float* dx_out,
                           const void* dx_out_add, float* dx_in, void* dx_in_add, const TimLayerGrads* g, void* workspace,
                           size_t workspace_bytes, void* stream);
int timhip_layer_bwd_data_split(const TimDesc* d, const TimLayerParams* w, const void* saved, const float* dx_out,
                                const void* dx_out_add, float* dx_in, void* dx_in_add, void* dy, const TimLayerGrads* g,
                                void* workspace, size_t workspace_bytes, void* stream);

/* ---- front end --------------------------------------------------------------
 * The time MLP (tim.py:66-74), the modality embedders and the sequence assembly
 * (encodings.py:41-75,102-121,181-251) are sequenced by the host mirror
 * (tim_amd/functional.py) from the generic entry points above plus the two below. */

/* Sequence assembly (encodings.py:190-250): token row s of every window is described by
 * rows[s]: x[b,s,:d] = (kind 0: e0[b,src] | kind 2: e1[b,src] | kind 1: cls[src]),
 * x[b,s,d:] = te[b,te_row], + mod[mod] over all 2d columns (mod < 0: none), then sequence
 * dropout; writes the fp32 residual stream and its operand-dtype copy. */
typedef struct TimSeqRow {
  int32_t kind;
  int32_t src;
  int32_t te_row;
  int32_t mod;
} TimSeqRow;
int timhip_assemble_fwd(int precision, const TimSeqRow* rows /*device, [S]*/, int B, int S, int d,
                        const float* e0, const float* e1, int n_e_rows, const float* cls,
                        const float* te, int T, const float* mod, float p_seq_drop, uint64_t seed,
                        uint32_t site, float* x, void* x_T, void* stream);
/* d_e0 / d_e1 (either may be NULL) are WRITTEN: row (b, src) of every feature row the table names, no other row is touched.
 * d_te (may be NULL) is WRITTEN in full, [B, T, d]: the sum over the token rows that read time row t, in table order, no atomics -
 * zero for a time row no token row reads; the caller need not clear it.  d_cls and d_mod are ACCUMULATED (+=, float atomics, the
 * order of the additions is not fixed): the caller zeroes them, or passes a gradient that is to be added to. */
int timhip_assemble_bwd(const TimSeqRow* rows, int B, int S, int d, const float* dx, int n_e_rows,
                        int T, float p_seq_drop, uint64_t seed, uint32_t site, float* d_e0,
                        float* d_e1, float* d_cls, float* d_te, float* d_mod, void* stream);

/* The same with the CLS token vectors (ncls <= 8, [d] each) and the modality vectors (nmod <= 4, [2 d] each) given by pointer:
 * host arrays of device pointers, 16-byte aligned - the separate nn.Parameters of encodings.py:29-35,158-175 as they lie (and, in
 * the backward, their gradient views: accumulated into, zeroed by the caller; a NULL entry of a gradient table means that
 * gradient is not wanted - the forward refuses NULL or misaligned entries with TIMHIP_EALIGN before it launches).  Saves the two concatenations of a forward and
 * the copy back of a backward. */
int timhip_assemble_fwd_p(int precision, const TimSeqRow* rows, int B, int S, int d, const float* e0, const float* e1,
                          int n_e_rows, const float* const* cls, int ncls, const float* te, int T, const float* const* mod,
                          int nmod, float p_seq_drop, uint64_t seed, uint32_t site, float* x, void* x_T, void* stream);
int timhip_assemble_bwd_p(const TimSeqRow* rows, int B, int S, int d, const float* dx, int n_e_rows, int T,
                          float p_seq_drop, uint64_t seed, uint32_t site, float* d_e0, float* d_e1, float* const* d_cls, int ncls,
                          float* d_te, float* const* d_mod, int nmod, void* stream);

/* ---- heads ------------------------------------------------------------------ */
/* rows_T[B*n, E] (T) = x_T[b, s0 + i, :] for i < n : gathers the query rows a head reads (any E > 0; E % 4 == 0 moves 4 elements
 * per access - with TIMHIP_PREC_FP32 as the element type also the fp32 rows and [rows, 2] statistics of the evaluation tail) */
int timhip_gather_rows(int precision, const void* x_T, int B, int S, int E, int s0, int n,
                       void* rows_T, void* stream);
/* dx[b, s0+i, :] += d_rows[b*n+i, :]  (fp32; E % 4 == 0) */
int timhip_scatter_rows_add(const float* d_rows, int B, int S, int E, int s0, int n, float* dx,
                            void* stream);
/* The same moves for up to 6 token ranges in one launch (the four classification heads; the two entry points above are the
 * one-range calls of these kernels; E % 4 == 0, B > 0; the ranges of a scatter must be DISJOINT - heads that share token rows,
 * as in the detection model, go into separate launches), and the fp32 -> operand-dtype
 * cast of several cotangent matrices (dst[i] is [rows[i], ld[i]], zero padded beyond cols[i]) in one launch. */
int timhip_gather_ranges(int precision, const void* x_T, int B, int S, int E, int count, const int* s0, const int* n,
                         void* const* rows_T, void* stream);
/* rows3_T[i][b * n[i] + j, 0 .. 3 E) = the fp32 row x[b, s0[i] + j, :] as the split operand [hi | lo | hi] (three 16-bit column
 * blocks of width E, a multiple of 64; 16-bit modes): timhip_gather_ranges on the fp32 rows + timhip_split3_many (mode 0) in one
 * launch - how the fp16 mode feeds its classification heads (count 1 .. 6 ranges) */
int timhip_gather_split3_ranges(int precision, const float* x, int B, int S, int E, int count, const int* s0, const int* n,
                                void* const* rows3_T, void* stream);
/* dx[B,S,E] (fp32, the gradient entering the last encoder layer) written in one pass: rows s < F <- feats_cot[b,s,:] (NULL: 0),
 * rows of the count <= 6 DISJOINT token ranges [s0[i], s0[i] + n[i]) (s0[i] >= F) <- d_rows[i][b*n[i] + j,:], every other row 0. */
int timhip_dx_init(int B, int S, int F, int E, const float* feats_cot, int count, const int* s0, const int* n,
                   const float* const* d_rows, float* dx, void* stream);
/* dst[rows, ld] (operand dtype, zero padded beyond cols) = scale * grad_out * y * (1 - y): the backward of a sigmoid output layer
 * (the regression heads of det head.py:95-163) written as the operand rows of the gradient GEMMs; scale: device scalar or NULL */
int timhip_sigmoid_bwd_rows(int precision, const float* grad_out, const float* y, int rows, int cols, void* dst, int ld,
                            const float* scale, void* stream);
/* ... with range i given as nslab[i] (1 .. 16; NULL: 1 each) consecutive [B n[i], E] slabs at d_rows[i] that are added up on the
 * way: the input-gradient product of a head with a long contraction (3806 action classes) runs as several column chunks of the
 * contraction side by side, each into its own slab (tim_amd/functional.py: the 240 blocks of that product ran 60 contraction
 * steps each while the other heads' blocks had finished after 2 - 5). */
int timhip_dx_init_slabs(int B, int S, int F, int E, const float* feats_cot, int count, const int* s0, const int* n,
                         const float* const* d_rows, const int* nslab, float* dx, void* stream);
int timhip_scatter_ranges_add(int B, int S, int E, int count, const int* s0, const int* n,
                              const float* const* d_rows, float* dx, void* stream);
int timhip_cast_rows_many(int precision, int count, const float* const* src, const int* rows, const int* cols,
                          void* const* dst, const int* ld, const float* scale, void* stream);

/* ---------------------------------------------------------------- detection query labelling */
/* TIM.label_queries of the detection model (detection/time_interval_machine/models/tim.py:214-270, with get_query_ious
 * :186-212): every query [b, q] is matched to the ground-truth segment of window b with the largest 1-D IoU (first maximum,
 * as torch.argmax; all intervals of a window are first shifted by |min(0, earliest segment start)|).  queries [B,Nq,2] and
 * segs [B,Ng,2] fp32, labels [B,Ng,NL] int64.  Writes targets [B*Nq,2] (the matched - shifted - segment, +inf for queries whose
 * best IoU is < iou_threshold), ious [B*Nq] and qlabels [B*Nq,NL] (-1 for those negatives).  fp32 results are the
 * reference's bit for bit. */
int timhip_label_queries(const float* queries, const float* segs, const int64_t* labels, int B, int Nq, int Ng, int NL,
                         float iou_threshold, float* targets, float* ious, int64_t* qlabels, void* stream);
/* The label-smoothed one-hot classification targets of TIM.assign_positive_labels (tim.py:157-184) for label column `col`
 * of qlabels [rows, ld]: out[r, c] = (c == label) ? on : base for c < n (a label of -1 leaves the row at `base`).  The caller
 * passes on = fp32(fp32(smoothing) + base), base = fp32((1 - smoothing) / (n + 1)), the two values the reference's expression
 * takes.  out [rows, n] fp32, 16-byte aligned. */
int timhip_smooth_one_hot(const int64_t* qlabels, int ld, int col, int64_t rows, int n, float on, float base, float* out,
                          void* stream);

/* ---------------------------------------------------------------- loss tail of the training step */
/* Label-smoothed cross entropy under mixup, as recognition/scripts/train.py:46-49,218-316 applies it through
 * utils/mixup.py:24-39:  loss = lam * mean_{r: ta[r] != -1} CE(logits[r], ta[r]) + (1-lam) * mean_{r: tb[r] != -1}
 * CE(logits[r], tb[r]),  CE with label smoothing `smoothing` (torch.nn.CrossEntropyLoss(label_smoothing, ignore_index=-1)).
 * target_b may be NULL (plain criterion, lam = 1).  stats [rows,4] and accum [4] are scratch kept for the backward;
 * loss is a device scalar.  dlogits = grad_out[0] * d loss / d logits (grad_out: device scalar or NULL = 1).
 * logits is [rows, C] with row pitch ld >= C, dlogits [rows, C] with row pitch ldd >= C (elements; columns from C on are neither
 * read nor written); no alignment beyond that of a float.  rows >= 1, 0 <= smoothing < 1, else TIMHIP_EINVAL.  A target outside
 * [0, C) is ignored like -1; a side without a valid row contributes 0 and its rows get no gradient.  stats[r] = (logsumexp,
 * mean, CE_a or -1, CE_b or -1), accum = (sum_a, n_a, sum_b, n_b); no atomics: two calls give the same bits. */
int timhip_ce_mixup_fwd(const float* logits, int rows, int C, int ld, const int64_t* target_a, const int64_t* target_b,
                        float lam, float smoothing, float* stats, float* accum, float* loss, void* stream);
int timhip_ce_mixup_bwd(const float* logits, int rows, int C, int ld, const int64_t* target_a, const int64_t* target_b,
                        float lam, float smoothing, const float* stats, const float* accum, const float* grad_out,
                        float* dlogits, int ldd, void* stream);

/* DRLoc sample collection (models/helpers/losses/drloc.py:11-15,24-26,37-39): out[(b*m+i), 0:D] = x1[b, pos1[b,i], :],
 * out[.., D:2D] = x2[b, pos2[b,i], :], cast to the operand dtype ([n*m, ld] GEMM operand of drloc_mlp.0).
 * x1, x2: fp32 [n, l, D] views with element strides (batch_stride, row_stride, 1).  The scatter adds the gradient
 * of that operand back: dx1[b, pos1[b,i], :] += d_pts[(b*m+i), 0:D] (fp32 atomics; positions repeat).
 * gather: D, ld, batch_stride and row_stride are multiples of 4, ld >= 2D (else TIMHIP_EINVAL); x1, x2 and out are 16-byte
 * aligned (else TIMHIP_EALIGN); columns of out from 2D on are not written; x1 and x2 may overlap or coincide.  scatter: d_pts has
 * row pitch ldg >= 2D; dx1 / dx2 are accumulated onto (not zeroed) and may overlap or coincide; no alignment rule.  Positions must
 * lie in [0, l): they are not checked. */
int timhip_drloc_gather(int precision, const float* x1, const float* x2, int64_t batch_stride, int64_t row_stride,
                        int n, int l, int D, const int64_t* pos1, const int64_t* pos2, int m, void* out, int ld,
                        void* stream);
int timhip_drloc_scatter_add(const float* d_pts, int ldg, float* dx1, float* dx2, int64_t batch_stride,
                             int64_t row_stride, int n, int l, int D, const int64_t* pos1, const int64_t* pos2, int m,
                             void* stream);

/* The same cross entropy with lam read from DEVICE memory (a mixup state that a captured step redraws, below): the arguments,
 * the launches and the bits of timhip_ce_mixup_fwd / _bwd called with the float lam[0] holds when the forward's kernel runs.
 * accum is [8] here: words 0-3 as above, word 4 = the lam the forward used; the backward reads THAT copy (it takes no lam),
 * so a state redrawn between forward and backward does not reach it.  lam NULL: TIMHIP_EINVAL. */
int timhip_ce_mixup_fwd_dev(const float* logits, int rows, int C, int ld, const int64_t* target_a, const int64_t* target_b,
                            const float* lam, float smoothing, float* stats, float* accum, float* loss, void* stream);
int timhip_ce_mixup_bwd_dev(const float* logits, int rows, int C, int ld, const int64_t* target_a, const int64_t* target_b,
                            float smoothing, const float* stats, const float* accum, const float* grad_out,
                            float* dlogits, int ldd, void* stream);

/* ---------------------------------------------------------------- mixup of the inputs on the device (utils/mixup.py:4-22) */
/* Draw: n independent mixup sets in one launch, nothing on the host taking part.  lam float[n]; perm, inv int32[n * B] with
 * inv[s * B + perm[s * B + b]] == b.  counter: one 64-bit word in device memory, the number of sets drawn so far; the kernel
 * reads it (c) and stores c + n (one thread, after every thread has read it), so the k-th set of a seed is the same bits
 * whether its launch is eager or the k-th replay of a captured graph.  Set s of the launch is draw number D = c + s.
 *   randomness  philox4x32_7 (csrc/common.h) with key = seed, site = SITE_MIXUP (8) and Philox counter (D << 24) | j, block
 *               j = 0, 1, ... of four 32-bit words; D counts modulo 2^40.  The dropout salt is NOT added: a draw does not depend on
 *               how many encoder forwards ran in between.
 *   lam         ~ Beta(alpha, alpha), sampled exactly (up to the 2^-32 grid of a uniform u = (word + 0.5) / 2^32) by rejection,
 *               in double precision, rounded to float at the end:
 *                 alpha < 1   Johnk: X = u0^(1/alpha), Y = u1^(1/alpha) from words 0, 1 of block j = trial; accepted when
 *                             X + Y <= 1; lam = X / (X + Y).  At most 64 trials; a trial is rejected with probability
 *                             1 - Gamma(alpha+1)^2 / Gamma(2 alpha+1) <= 1/2, so the bound is hit with probability <= 2^-64
 *                             per draw; lam is then 0.5.
 *                 alpha >= 1  lam = G1 / (G1 + G2), two Marsaglia-Tsang Gamma(alpha) variates: d = alpha - 1/3, c = 1/sqrt(9d),
 *                             x = sqrt(-2 ln u0) cos(2 pi u1), v = (1 + c x)^3, accepted when v > 0 and
 *                             ln u2 < x^2/2 + d - d v + d ln v; G = d v.  G1 reads blocks 0..31, G2 blocks 32..63 (words
 *                             0, 1, 2 of block = trial).  A trial is rejected with probability < 0.06 for every alpha >= 1, so
 *                             32 trials all fail with probability < 1e-39 per variate; the variate is then d.
 *               alpha <= 0: lam = 1 (utils/mixup.py:6) and the permutation is still drawn.  Supported:
 *               TIMHIP_MIXUP_ALPHA_MIN <= alpha <= TIMHIP_MIXUP_ALPHA_MAX (below it u^(1/alpha) leaves the double range); any
 *               other positive alpha, or NaN: TIMHIP_EINVAL.
 *   perm        Fisher-Yates from the identity, i = B-1 .. 1: j = (uint64(r) * (i + 1)) >> 32, swap(perm[i], perm[j]); r = word
 *               i & 3 of block 256 + (i >> 2).  Integer arithmetic only: a CPU restatement gives the same bits.  j is not
 *               exactly uniform on 0..i: each value's probability is off by at most 2^-32, a total bias of at most B / 2^32
 *               per swap.
 * 1 <= B <= 2^20, 1 <= n <= 65536, else TIMHIP_EINVAL.  One thread per set, one block: a few microseconds at n = 1. */
#define TIMHIP_MIXUP_ALPHA_MIN 0.05f
#define TIMHIP_MIXUP_ALPHA_MAX 16.0f
#define TIMHIP_MIXUP_MAX_TENSORS 4
int timhip_mixup_draw(uint64_t seed, uint64_t* counter, float alpha, int B, int n, float* lam, int32_t* perm, int32_t* inv,
                      void* stream);

/* Apply: dst_t[b] = lam * src_t[b] + (1 - lam) * src_t[index[b]] for nt <= TIMHIP_MIXUP_MAX_TENSORS tensors in one launch;
 * b = 0..B-1, item b of tensor t being the contiguous slab of elems[t] >= 1 elements at element offset b * elems[t].
 * src, dst, elems, dtype: HOST arrays of nt entries; dtype[t] = TIMHIP_PREC_FP32, _F16 or _BF16 is the STORAGE type of src_t
 * and dst_t (anything else: TIMHIP_EINVAL); the arithmetic is fp32 - two rounded products, one rounded sum, no fused
 * multiply-add - and the result is rounded once to the storage type.  lam: device float; index: device int32[B] with entries
 * in [0, B) (not checked).  dst_t must not overlap any src.  The backward of the mix is the same call on the output gradients
 * with the inverse permutation as index.  Pointers need the alignment of their element only: items whose three slabs are
 * 16-byte aligned move as 16-byte accesses, the tail of an item (elems not a multiple of 16 bytes) and items off that
 * alignment element by element.  Byte-bound: two reads and one write per element. */
int timhip_mixup_apply(int nt, const void* const* src, void* const* dst, const int64_t* elems, const int32_t* dtype, int B,
                       const float* lam, const int32_t* index, void* stream);

/* ---------------------------------------------------------------- detection losses */
/* sigmoid focal loss (detection models/helpers/losses/sigmoid.py:5-52) under get_loss(.., weights, reduction="sum")
 * (losses/loss.py:5-14):  loss_sum = sum_{r: valid[r]} w[r] * sum_c focal(logits[r,c], targets[r,c]);  targets are the
 * smoothed one-hot floats of det tim.py:157-184; row_weights / row_valid may be NULL; loss_elem (optional, [rows,C])
 * receives the weighted per-element terms (reduction "none").  bwd: dlogits = grad_out[0] * d loss_sum / d logits.
 * logits, targets, loss_elem and dlogits are dense [rows, C] (no pitch argument), float aligned; rows with row_valid == 0 give
 * exactly 0 in loss_elem and dlogits.  alpha < 0: no alpha weighting; any gamma >= 0 (gamma == 2 takes a multiply instead of powf;
 * where 1 - p_t is 0 the gradient's second term is its limit 0).  rows == 0: loss_sum is zeroed, nothing else is written.
 * loss_sum is joined with one atomic per block: its last bits depend on the order. */
int timhip_focal_loss_fwd(const float* logits, const float* targets, int rows, int C, const float* row_weights,
                          const uint8_t* row_valid, float alpha, float gamma, float* loss_sum, float* loss_elem,
                          void* stream);
int timhip_focal_loss_bwd(const float* logits, const float* targets, int rows, int C, const float* row_weights,
                          const uint8_t* row_valid, float alpha, float gamma, const float* grad_out, float* dlogits,
                          void* stream);
/* 1-D centre-offset DIoU loss (losses/iou.py:4-65), summed over the valid rows; offsets are [n,2] = (left, right).
 * loss_sum and/or dpred (= grad_out[0] * d loss / d pred) are produced when non-NULL; both NULL is TIMHIP_EINVAL; n == 0 zeroes
 * loss_sum and writes nothing else.  Dense [n,2] arrays, float aligned; rows with row_valid == 0 give 0.  The gradient follows the
 * compiled TorchScript form of the reference: min / max pass a gradient under strict comparison only (nothing to the tied side of
 * an exact tie), clamp(min=eps) where its input >= eps. */
int timhip_diou_1d(const float* pred_offsets, const float* target_offsets, int n, const uint8_t* row_valid, float eps,
                   const float* grad_out, float* loss_sum, float* dpred, void* stream);
/* One modality side of the detection training loss (det scripts/train.py:222-349) with the row flags derived where they are used:
 * valid_cls = iou >= 0, row weight = iou < iou_threshold ? 1 : iou, positive = offsets[r, 0] != inf; the nheads <= 4 classification
 * heads' focal sums, the DIoU sum of the positive rows and their count in one pass each, then
 *   normaliser <- momentum * normaliser + (1 - momentum) * max(positives, 1)      (device scalar, in / out)
 *   loss = focal / (nheads * normaliser) + (positives > 0 ? lambda_reg * DIoU / normaliser : 0)
 * block (device float[8], out) = {loss, focal sum, DIoU sum, positives, normaliser used, 0, 0, 0}; the backward reads it.
 * logits / targets / dlogits: host arrays of device pointers, dense [rows, C[k]] each; dlogits[k] may be NULL, dreg may be NULL.
 * 1 <= nheads <= 4, and with rows > 0 every head that is read (forward: all; backward: those with dlogits[k] != NULL) has logits[k],
 * targets[k] and C[k] >= 1, else TIMHIP_EINVAL; every argument is checked before the first launch, so a refused call writes nothing.
 * Rows with iou < 0 get exactly 0 in every dlogits[k], non-positive rows exactly 0 in dreg (same tie / clamp rule as
 * timhip_diou_1d).  grad_out: device scalar or NULL = 1.  All arrays float aligned; block is 8 floats, all of them written. */
int timhip_det_side_loss_fwd(const float* const* logits, const float* const* targets, const int* C, int nheads, int rows,
                             const float* iou, const float* offsets, const float* reg_pred, float iou_threshold, float alpha,
                             float gamma, float eps, float lambda_reg, float momentum, float* normaliser, float* block,
                             void* stream);
/* The same forward with sums that do not depend on the order in which blocks finish (additive to ABI 6).  timhip_det_side_loss_fwd
 * adds the partial sums of its blocks and waves onto block[1..3] with float atomics: the loss of one input differs in its last place
 * from run to run.  Here every block (focal launches) and every wave (rows launch) stores its sum in a slot of `partials` (device
 * float[TIMHIP_DET_SIDE_PARTIALS], caller-owned scratch, contents undefined afterwards) and ONE finishing block adds the slots in a
 * fixed order (thread t: slots t, t + 256, ... of head 0, 1, ..., then a fixed tree over the 256 threads) into block[1..3]; the
 * finishing kernel of the atomic form follows (one launch more): the same input gives the same bits in every run, eager or as a replayed graph node.  Same arguments, checks,
 * grids and block layout; the value differs from the atomic form's by rounding only; timhip_det_side_loss_bwd reads either block.
 * partials NULL: TIMHIP_EINVAL. */
#define TIMHIP_DET_SIDE_PARTIALS 4096
int timhip_det_side_loss_fwd_ordered(const float* const* logits, const float* const* targets, const int* C, int nheads, int rows,
                                     const float* iou, const float* offsets, const float* reg_pred, float iou_threshold, float alpha,
                                     float gamma, float eps, float lambda_reg, float momentum, float* normaliser, float* block,
                                     float* partials, void* stream);
/* The ordered forward with the SIDE STATISTICS a detection meter needs (additive to ABI 6): what the reference's loop
 * gets from a second focal pass with reduction="none" over the action head (det scripts/train.py:262-273, :315-326) comes out of the
 * pass that is made anyway.  Arguments of _fwd_ordered plus `stats` (device float[TIMHIP_DET_SIDE_STATS_WORDS], every word written):
 *   TIMHIP_DET_STAT_HEAD_SUM + k   focal sum of head k < nheads (0 for the other k < 4)
 *   TIMHIP_DET_STAT_POS_SUM        the LAST head's focal sum over the rows with iou >= 0 and offsets[r, 0] != inf
 *   TIMHIP_DET_STAT_NEG_SUM        the LAST head's focal sum over the rows with iou >= 0 and offsets[r, 0] == inf
 *   TIMHIP_DET_STAT_VALID          rows with iou >= 0              _POSITIVES   = block[3]      _DIOU_SUM = block[2]
 *   TIMHIP_DET_STAT_NORMALISER     = block[4]                      _LOSS        = block[0]
 *   TIMHIP_DET_STAT_CLS            focal / (nheads * nm)           _REG         positives > 0 ? lambda_reg * DIoU / nm : 0
 *   TIMHIP_DET_STAT_HEAD + k       HEAD_SUM[k] / nm                _POS, _NEG   POS_SUM / nm, NEG_SUM / nm      (nm = block[4])
 * all fp32; counts are exact floats.  partials: float[TIMHIP_DET_SIDE_STATS_PARTIALS] (the ordered form's slots, then the last head's
 * (positive, negative) per block and the valid rows per wave).  No float atomics.  The last head's launch keeps two more accumulators
 * and reads offsets[r, 0] beside iou[r]; the accumulators behind block[1..3] are the ordered form's: for one input block[0..7] and
 * normaliser are bit for bit those of _fwd_ordered, and timhip_det_side_loss_bwd reads the block as before.  Same launches as the
 * ordered form (its kernels' stats arms).  Refused before any launch, nothing written: what _fwd_ordered refuses, stats or partials
 * NULL - TIMHIP_EINVAL; rows > 2^24 - TIMHIP_EUNSUPPORTED.  rows == 0: zeros, with NORMALISER = block[4] advanced as by _fwd_ordered. */
enum { TIMHIP_DET_STAT_HEAD_SUM = 0, TIMHIP_DET_STAT_POS_SUM = 4, TIMHIP_DET_STAT_NEG_SUM = 5, TIMHIP_DET_STAT_VALID = 6,
       TIMHIP_DET_STAT_POSITIVES = 7, TIMHIP_DET_STAT_DIOU_SUM = 8, TIMHIP_DET_STAT_NORMALISER = 9, TIMHIP_DET_STAT_LOSS = 10,
       TIMHIP_DET_STAT_CLS = 11, TIMHIP_DET_STAT_REG = 12, TIMHIP_DET_STAT_HEAD = 13, TIMHIP_DET_STAT_POS = 17, TIMHIP_DET_STAT_NEG = 18,
       TIMHIP_DET_STAT_RESERVED = 19 };
#define TIMHIP_DET_SIDE_STATS_WORDS 20
#define TIMHIP_DET_SIDE_STATS_PARTIALS 6144
int timhip_det_side_loss_fwd_stats(const float* const* logits, const float* const* targets, const int* C, int nheads, int rows,
                                   const float* iou, const float* offsets, const float* reg_pred, float iou_threshold, float alpha,
                                   float gamma, float eps, float lambda_reg, float momentum, float* normaliser, float* block,
                                   float* partials, float* stats, void* stream);
int timhip_det_side_loss_bwd(const float* const* logits, const float* const* targets, const int* C, int nheads, int rows,
                             const float* iou, const float* offsets, const float* reg_pred, float iou_threshold, float alpha,
                             float gamma, float eps, float lambda_reg, const float* block, const float* grad_out,
                             float* const* dlogits, float* dreg, void* stream);


/* ---------------------------------------------------------------- 1-D segment NMS */
/* Batched soft-NMS over independent groups (one per video x class), bit-identical in its selection to
 * detection/eval_detection/csrc/nms_cpu.cpp:69-170 (softnms_1d_cpu) run on each group:
 *   segs [N,2], scores [N] grouped contiguously; group g = rows [group_offsets[g], group_offsets[g+1]) (int32, device copy
 *   and host copy of the same G+1 values); method 0 vanilla / 1 linear / 2 gaussian.
 *   dets [N,3]: for group g rows group_offsets[g] .. +count[g]-1 hold (start, end, score at selection) in selection order,
 *   inds [N]: the selected segments' indices relative to the group's first row; count [G].
 * workspace: timhip_softnms_1d_workspace_bytes(N, G) bytes of device memory.  Synchronises `stream` before returning
 * (it stages per-size-class group lists from pageable host memory). */
size_t timhip_softnms_1d_workspace_bytes(int64_t n_total, int n_groups);
int timhip_softnms_1d(const float* segs, const float* scores, const int32_t* group_offsets,
                      const int32_t* group_offsets_host, int n_groups, float iou_threshold, float sigma, float min_score,
                      int method, float* dets, int32_t* inds, int32_t* count, void* workspace, size_t workspace_bytes,
                      void* stream);
/* Batched vanilla NMS (nms_cpu.cpp:19-60): order [N] = for each group the positions (relative to the group) sorted by
 * descending score; keep [N] receives per group the kept positions in that order, count [G] their number;
 * removed_scratch: N bytes. */
int timhip_nms_1d(const float* segs, const int32_t* order, const int32_t* group_offsets, int n_groups, float iou_threshold,
                  uint8_t* removed_scratch, int32_t* keep, int32_t* count, void* stream);

/* ---------------------------------------------------------------- detection candidates */
/* The inference tail between the detection heads and the NMS, per batch and per head, as the reference computes it in
 * detection/time_interval_machine/utils/meters.py (FeatureMeter.update) and detection/eval_detection/format_predictions.py
 * (main): proposal r = w * Nq + q of window w becomes clamp(reg[r], 0, *max_time) * window_size (fp32) + window_start[w]
 * (fp64), rounded to three decimals as numpy.round does on float64; it is kept iff its rounded width is > 0.  Class c of a
 * kept proposal is a candidate iff score = (float)(1 / (1 + exp(-(double)logit))) > score_threshold (fp32 compare).
 * Candidates are listed proposal by proposal and by ascending class inside a proposal; that order is part of the result.
 *
 * timhip_det_candidates_count: logits [R, C] fp32 with row stride ld_logits (elements, >= C: a head's slice needs no copy),
 *   reg [R, 2] fp32, window_start [R / Nq] fp64, max_time: DEVICE pointer to one float (no host read).  Writes seg32 [R, 2]
 *   (the rounded segment cast to fp32), seg_ok [R] (1: kept) and row_offsets [R + 1]: row r's candidates occupy output
 *   slots [row_offsets[r], row_offsets[r + 1]), row_offsets[R] is their total.  Two launches (count, scan).
 * timhip_det_candidates_emit: the same walk over the same logits; writes candidate k of row r at row_offsets[r] + k:
 *   seg [N, 2], score [N], key [N] = video_index[w] * C + class, row [N] = r.  `capacity` = the number of candidates the four
 *   output buffers hold; a slot at or beyond it (or beyond its row's range) is not written, so a worst-case-sized output
 *   (R * C) makes the pair replayable in a HIP graph.  One launch.
 * Neither call allocates, synchronises or reads device memory on the host.  R * C must fit in int32; R must be a multiple
 * of Nq. */
int timhip_det_candidates_count(const float* logits, int64_t ld_logits, const float* reg, const double* window_start,
                                float window_size, const float* max_time, int R, int C, int Nq, float score_threshold,
                                float* seg32, uint8_t* seg_ok, int32_t* row_offsets, void* stream);
int timhip_det_candidates_emit(const float* logits, int64_t ld_logits, const float* seg32, const uint8_t* seg_ok,
                               const int32_t* row_offsets, const int32_t* video_index, int R, int C, int Nq,
                               float score_threshold, int64_t capacity, float* seg, float* score, int64_t* key,
                               int32_t* row, void* stream);

/* ---------------------------------------------------------------- two-stream detection fusion */
/* The fusion of a verb stream and a noun stream over the same proposals into (verb, noun) action candidates, per batch, as
 * the reference computes it on the host in detection/eval_detection/format_two_stream_predictions_epic.py (main).  Scores
 * and decoded proposals are those of the detection candidates above, per stream, the proposals unrounded:
 * prop = (double)(clamp(reg, 0, *max_time) * window_size) + window_start[w].  Of each row the top_k classes of either stream
 * are selected on the fp32 score (equal scores: the lower class first; a NaN ranks above every number).  Pair (i, j) of the
 * i-th verb (score vs) and the j-th noun (score ns), both by descending score, is a candidate iff vs > thr, ns > thr,
 * score = (float)pow(vs, alpha32) * (float)pow(ns, beta32) > thr (fp32 compares, the powers in fp64 rounded once) and the
 * segment w * prop_verb + (1 - w) * prop_noun, w = vs / (vs + ns) in fp32, products and sum in fp64, rounded to three
 * decimals as numpy.round does, has a width > 0.  The caller passes alpha32 = (float)alpha and beta32 = (float)(1.0 - alpha).
 * Candidates are listed proposal by proposal, pair i * top_k + j ascending inside a proposal; that order is part of the
 * result.
 *
 * timhip_ts_candidates_count: verb_logits [R, Cv] / noun_logits [R, Cn] fp32 with row strides ld_v / ld_n (elements, >= C:
 *   a head's slice needs no copy), verb_reg / noun_reg [R, 2] fp32, window_start [R / Nq] fp64, max_time: DEVICE pointer to
 *   one float.  Writes the per-row records - sel_idx [R, 2, top_k] and sel_score [R, 2, top_k] (verbs, then nouns),
 *   pair_score [R, top_k^2], pair_seg [R, top_k^2, 2] (fp32), pair_mask [R] (bit p: pair p is a candidate) - and
 *   row_offsets [R + 1]: row r's candidates occupy output slots [row_offsets[r], row_offsets[r + 1]), row_offsets[R] is
 *   their total.  Two launches (select, scan).  R == 0 is a valid empty call that still writes row_offsets[0] = 0.
 * timhip_ts_candidates_emit: reads the records only; writes candidate j of row r at row_offsets[r] + j: seg [N, 2],
 *   score [N], key [N] = video_index[w] * (Cv * Cn) + verb * Cn + noun, row [N] = r.  `capacity` = the number of candidates
 *   the four output buffers hold; a slot at or beyond it (or beyond its row's range) is not written, so a worst-case-sized
 *   output (R * top_k^2) makes the pair replayable in a HIP graph.  One launch.
 * Neither call allocates, synchronises or reads device memory on the host.  TIMHIP_EINVAL: a null pointer with R > 0,
 * top_k < 1, top_k > min(Cv, Cn), R not a multiple of Nq, ld < C.  TIMHIP_EUNSUPPORTED: top_k > 8 (one lane per pair),
 * Cv + Cn > 4096 (a block's scores live in 64 KiB of LDS), R * top_k^2 beyond int32. */
int timhip_ts_candidates_count(const float* verb_logits, int64_t ld_v, const float* noun_logits, int64_t ld_n,
                               const float* verb_reg, const float* noun_reg, const double* window_start, float window_size,
                               const float* max_time, int R, int Cv, int Cn, int Nq, int top_k, float score_threshold,
                               float alpha32, float beta32, int32_t* sel_idx, float* sel_score, float* pair_score,
                               float* pair_seg, uint64_t* pair_mask, int32_t* row_offsets, void* stream);
int timhip_ts_candidates_emit(const int32_t* sel_idx, const float* pair_score, const float* pair_seg, const uint64_t* pair_mask,
                              const int32_t* row_offsets, const int32_t* video_index, int R, int Cv, int Cn, int Nq, int top_k,
                              int64_t capacity, float* seg, float* score, int64_t* key, int32_t* row, void* stream);

/* ---------------------------------------------------------------- recognition scores and accuracies */
/* The inference tail behind the recognition heads, as the reference computes it on the host in
 * recognition/time_interval_machine/utils/meters.py (InferenceMeter / FeatureMeter: index_add_ of the valid query rows into
 * per-action accumulators, division by the seen count, softmax) and utils/metrics.py (accuracy, multitask_accuracy).
 *
 * State, all persistent device buffers the caller zero-fills (labels_state: -1) before the first batch: per head
 * sum [num_actions, pitch] fp32 (pitch >= C; a multiple of 64 aligns the stores), seen [num_actions] fp32 (one vector for
 * all modalities, as in the reference), and per modality labels_state [num_actions, n_labels] int32, touched [num_actions]
 * bytes; one int32 error word.
 *
 * rec_accumulate: one batch of one modality.  heads: HOST array of n_heads (<= TIMHIP_REC_MAX_HEADS) heads that share the id
 *   vector; logits [R, C] fp32 with row stride ld (elements, >= C: a strided view needs no copy).  ids [R] int64.  A row is
 *   valid iff valid[r] != 0, or with valid = NULL iff labels[r * ld_labels + valid_col] != -1; labels [R, n_labels] int64
 *   (NULL with a valid vector: labels_state is left alone).  Invalid rows are not read.  A valid row whose id is outside
 *   [0, num_actions) is skipped and ORs 1 into *err.  For every id of the batch: sum[id] = (((sum[id] + x_r0) + x_r1) + ...)
 *   in fp32 over its valid rows in ascending row order - what a serial index_add_ leaves - so the state does not depend on
 *   how a stream is cut into batches; seen[id] += the number of those rows; labels_state[id] = the labels of the last of
 *   them; touched[id] = 1.  work: 3 * R int32 of scratch.  Three launches on `stream`, no floating-point atomics, no
 *   allocation, no host read: replayable in a HIP graph.
 * rec_finalize: one head over the touched actions.  mean = sum / seen (fp32, correctly rounded);
 *   rank[a] = #{c : mean_c > mean_l} + #{c < l : mean_c == mean_l} for l = labels_state[a, label_col] (0x7fffffff for an
 *   untouched action, a label outside [0, C) or labels_state = NULL); with prob != NULL also
 *   prob[a, c] = (float)(exp((double)mean_c - max) / sum of those exps in double) for c < C, [num_actions, pitch]; rows of
 *   untouched actions are not written.
 * rec_counts: counts[0] = #(r < 1), counts[1] = #(r < 5), counts[2] = #touched over the touched actions, r = rank_a or, with
 *   rank_b != NULL, max(rank_a, rank_b) (the multitask accuracy). */
#define TIMHIP_REC_MAX_HEADS 3
typedef struct TimRecHead {
  const float* logits;
  float* sum;
  int64_t ld;
  int32_t C, pitch;
} TimRecHead;
int timhip_rec_accumulate(const TimRecHead* heads, int n_heads, const int64_t* ids, const uint8_t* valid,
                          const int64_t* labels, int64_t ld_labels, int n_labels, int valid_col, int R, int num_actions,
                          float* seen, int32_t* labels_state, uint8_t* touched, int32_t* err, int32_t* work, void* stream);
int timhip_rec_finalize(const float* sum, int pitch, int C, const float* seen, const int32_t* labels_state, int n_labels,
                        int label_col, const uint8_t* touched, int num_actions, float* prob, int32_t* rank, void* stream);
int timhip_rec_counts(const int32_t* rank_a, const int32_t* rank_b, const uint8_t* touched, int num_actions, int32_t* counts,
                      void* stream);

/* rec_combined: the AVE-only "combined" accuracy of the reference's meters (meters.py:283-285, :563-565).  prob_v /
 * prob_a: the probabilities rec_finalize wrote for the action head and the audio head ([num_actions, pitch_*], the same C).
 * The reference adds the two POSITIONALLY over the labelled actions of each modality: the k-th touched visual id a (ascending)
 * is paired with the k-th touched audio id b.  rank[a] = the rank of l = labels_state[a, label_col] over
 * (prob_v[a, c] + prob_a[b, c]) * 0.5f (fp32, the sum rounded, then the product) with rec_finalize's tie rule; 0x7fffffff for
 * an untouched visual id, a visual id without a partner or a label outside [0, C).  rec_counts over touched_v then gives the
 * counts.  One launch; a wavefront finds its pair with two scans of the touched bytes (num_actions / 64 steps each). */
int timhip_rec_combined(const float* prob_v, int pitch_v, const float* prob_a, int pitch_a, int C, const int32_t* labels_state,
                        int n_labels, int label_col, const uint8_t* touched_v, const uint8_t* touched_a, int num_actions,
                        int32_t* rank, void* stream);

/* ---------------------------------------------------------------- training meter (additive to ABI 6) */
/* The loss averages and batch accuracies of a recognition training run, kept in device memory: what the reference's TrainMeter
 * (recognition/time_interval_machine/utils/meters.py:30-167) keeps on the host after copying every head's logits there.
 *
 * STATE BLOCK: TIMHIP_METER_STATE_WORDS 32-bit words, 8-byte aligned, zero before the first update (and to reset).  The enum
 * gives WORD offsets; 64-bit fields (marked) start on even words:
 *   TIMHIP_METER_UPDATES             int64   updates so far
 *   TIMHIP_METER_SUM   + 4 * slot    double  sum of val * n          slot = TIMHIP_METER_TOTAL .. _AUDIO
 *   TIMHIP_METER_COUNT + 4 * slot    int64   sum of n                (avg = sum / count is the reader's division; 0 -> 0.0)
 *   TIMHIP_METER_RUN + 6 * head + 2 * k   int64   k = 0 rows, 1 top-1 hits, 2 top-5 hits since the reset, head = TIMHIP_METER_HEAD_*
 *   TIMHIP_METER_VAL   + slot        float   the loss of the last update that touched the slot
 *   TIMHIP_METER_LAST + 3 * head + k int32   the same three counts of the last update alone
 *   TIMHIP_METER_NV, TIMHIP_METER_NA int32   valid visual / audio rows of the last update
 *
 * meter_update: one batch.  v_heads / a_heads: HOST arrays of up to TIMHIP_METER_MAX_HEADS heads per modality over the
 *   UNFILTERED fp32 logits [R, C] with row stride ld (elements, >= C).  v_labels [Rv, >= 3] int64 (verb, noun, action; row
 *   stride ld_v_labels), a_labels [Ra, >= 1]; under mixup these are target_a.  A visual row is valid iff its action label
 *   (column 2) is not -1, an audio row iff column 0 is not -1; nv and na are those counts, taken on the device.
 *   losses: HOST array of TIMHIP_METER_SLOTS DEVICE pointers to one fp32 each (NULL: that loss counts as 0).  One thread does,
 *   in this order and in double / int64, sum = sum + (double)val * n (the product rounded on its own), count += n:
 *     TOTAL, DRLOC with n = nv + na, always;  VISUAL, then VERB and NOUN (only with TIMHIP_METER_VERB_NOUN), then ACTION
 *     with n = nv, only when nv > 0;  AUDIO with n = na, only when na > 0   (the conditions of meters.py:140-167).
 *   With TIMHIP_METER_BATCH_ACCURACY every valid row of every head is ranked over its raw logits x:
 *     rank = #{c : x_c > x_y} + #{c < y : x_c == x_y}, y = labels[r, head.label_col]; no rank (counted as a row, never a hit)
 *     when y is outside [0, C) or x_y is NaN.  head.slot names the counters it feeds; with a VERB and a NOUN head the MT
 *     counters take the larger of the two ranks (multitask accuracy).  work: timhip_meter_work_words(...) int32 of scratch.
 *   At most two launches on `stream`, no floating-point atomics, no allocation, no host read: replayable in a HIP graph, and
 *   every word is the same in every run.  Rv == 0 and Ra == 0 launches nothing.  Refused before any launch: NULL state /
 *   losses / heads / labels (logits with rows), more than TIMHIP_METER_MAX_HEADS heads in a group, C < 1, ld < C, a label
 *   column or slot out of range, unknown flags - TIMHIP_EINVAL; a state block off 8 bytes - TIMHIP_EALIGN. */
enum { TIMHIP_METER_TOTAL = 0, TIMHIP_METER_DRLOC = 1, TIMHIP_METER_VISUAL = 2, TIMHIP_METER_VERB = 3, TIMHIP_METER_NOUN = 4,
       TIMHIP_METER_ACTION = 5, TIMHIP_METER_AUDIO = 6 };
#define TIMHIP_METER_SLOTS 7
enum { TIMHIP_METER_HEAD_VERB = 0, TIMHIP_METER_HEAD_NOUN = 1, TIMHIP_METER_HEAD_ACTION = 2, TIMHIP_METER_HEAD_MT = 3,
       TIMHIP_METER_HEAD_AUDIO = 4 };
#define TIMHIP_METER_HEADS 5
enum { TIMHIP_METER_UPDATES = 0, TIMHIP_METER_SUM = 2, TIMHIP_METER_COUNT = 4, TIMHIP_METER_RUN = 30, TIMHIP_METER_VAL = 60,
       TIMHIP_METER_LAST = 67, TIMHIP_METER_NV = 82, TIMHIP_METER_NA = 83 };
#define TIMHIP_METER_STATE_WORDS 84
#define TIMHIP_METER_MAX_HEADS 3
enum { TIMHIP_METER_VERB_NOUN = 1, TIMHIP_METER_BATCH_ACCURACY = 2 };   /* flags */
typedef struct TimMeterHead {
  const float* logits;
  int64_t ld;
  int32_t C, label_col, slot, reserved;
} TimMeterHead;
size_t timhip_meter_work_words(const TimMeterHead* v_heads, int n_v, int Rv, const TimMeterHead* a_heads, int n_a, int Ra);
int timhip_meter_update(const TimMeterHead* v_heads, int n_v, const int64_t* v_labels, int64_t ld_v_labels, int Rv,
                        const TimMeterHead* a_heads, int n_a, const int64_t* a_labels, int64_t ld_a_labels, int Ra,
                        const float* const* losses, int flags, void* state, int32_t* work, void* stream);

/* ---------------------------------------------------------------- detection meter (additive to ABI 6) */
/* The eleven loss averages of the reference's detection TrainMeter and InferenceMeter (detection/time_interval_machine/utils/
 * meters.py:29-315, :317-572), kept in device memory and fed by the side statistics of timhip_det_side_loss_fwd_stats: what
 * det scripts/train.py:413-430 hands over after thirteen .cpu().item() / .cpu() reads.
 *
 * STATE BLOCK: TIMHIP_DET_METER_STATE_WORDS 32-bit words, 8-byte aligned, zero before the first update (and to reset).  WORD
 * offsets; 64-bit fields (marked) start on even words:
 *   TIMHIP_DET_METER_UPDATES                    int64   updates so far
 *   TIMHIP_DET_METER_SUM   + 4 * slot           double  sum of val * n        slot = TIMHIP_DET_METER_TOTAL .. _NEGATIVE
 *   TIMHIP_DET_METER_COUNT + 4 * slot           int64   sum of n              (avg = sum / count is the reader's division; 0 -> 0.0)
 *   TIMHIP_DET_METER_RUN  + 4 * side + 2 * k    int64   k = 0 valid rows (iou >= 0), 1 positives since the reset; side 0 visual, 1 audio
 *   TIMHIP_DET_METER_VAL   + slot               float   the value of the last update that touched the slot
 *   TIMHIP_DET_METER_LAST + 2 * side + k        int32   the same two counts of the last update alone
 *   TIMHIP_DET_METER_NORM + side                float   the normaliser the side's last update used
 *
 * det_meter_update: sides: HOST array of two DEVICE pointers to stats blocks (visual, audio; NULL: the side is absent and counts as
 *   zero rows).  nheads: the visual side's heads, 3 (verb, noun, action) or 1.  total_loss / drloc_loss: device scalars, NULL
 *   counts as 0.  One launch of one block; one thread does, in this order and in double / int64, sum = sum + (double)val * n
 *   (the product rounded on its own), count += n   (meters.py:94-137), with v_cls / v_pos / a_cls / a_pos the sides' VALID /
 *   POSITIVES words and every value its own side's, divided by that side's normaliser:
 *     v_cls > 0:  VISUAL = CLS, then VERB = HEAD[0] and NOUN = HEAD[1] (nheads == 3), then ACTION = HEAD[nheads - 1], n = v_cls;
 *                 VISUAL_REG = REG and POSITIVE = POS with n = v_pos;  NEGATIVE = NEG with n = v_cls - v_pos
 *     a_cls > 0:  AUDIO = CLS with n = a_cls;  AUDIO_REG = REG and POSITIVE = POS with n = a_pos;  NEGATIVE = NEG, n = a_cls - a_pos
 *     always:     TOTAL, DRLOC with n = v_cls + a_cls
 *   No synchronisation, no host read, no atomics: every word has the same bits eagerly and as a replayed graph node.  Refused
 *   before the launch: NULL state / sides, both sides NULL, nheads not 1 or 3 - TIMHIP_EINVAL; a state block off 8 bytes -
 *   TIMHIP_EALIGN. */
enum { TIMHIP_DET_METER_TOTAL = 0, TIMHIP_DET_METER_DRLOC = 1, TIMHIP_DET_METER_VISUAL = 2, TIMHIP_DET_METER_VERB = 3,
       TIMHIP_DET_METER_NOUN = 4, TIMHIP_DET_METER_ACTION = 5, TIMHIP_DET_METER_VISUAL_REG = 6, TIMHIP_DET_METER_AUDIO = 7,
       TIMHIP_DET_METER_AUDIO_REG = 8, TIMHIP_DET_METER_POSITIVE = 9, TIMHIP_DET_METER_NEGATIVE = 10 };
#define TIMHIP_DET_METER_SLOTS 11
enum { TIMHIP_DET_METER_UPDATES = 0, TIMHIP_DET_METER_SUM = 2, TIMHIP_DET_METER_COUNT = 4, TIMHIP_DET_METER_RUN = 46,
       TIMHIP_DET_METER_VAL = 54, TIMHIP_DET_METER_LAST = 65, TIMHIP_DET_METER_NORM = 69 };
#define TIMHIP_DET_METER_STATE_WORDS 72
int timhip_det_meter_update(void* state, const float* const* sides, int nheads, const float* total_loss, const float* drloc_loss,
                            void* stream);

/* ---------------------------------------------------------------- detection scoring: detections to AP */
/* The ActivityNet-style interpolated average precision of the reference's scoring script (detection/eval_detection/
 * evaluate_detection_json.py: compute_average_precision_detection, segment_iou, interpolated_prec_rec), on tables the caller
 * has sorted and grouped (tim_amd/detmap.py does it with device sorts).  All segment arithmetic is in double.
 *
 * timhip_det_match: pred_seg [n_pred, 2]: the predictions ordered by class, inside a class by descending score; a
 *   prediction's row is its position.  gt_seg [n_gt, 2]: the ground-truth segments grouped by (class, video); group g holds
 *   rows [group_gt_off[g], group_gt_off[g + 1]) (n_groups + 1 values).  group_pred [n_pred]: the predictions' positions
 *   grouped the same way, ascending inside a group; group g's predictions are group_pred[group_pred_lo[g] ..
 *   group_pred_hi[g]) (an empty range: the group has none), group_pos0[g] the position of the first prediction of g's class.
 *   For every prediction, in the order of its group's range, and every threshold t < T: tiou = inter / union with
 *   inter = max(min(pe, ge) - max(ps, gs), 0), union = (ge - gs) + (pe - ps) - inter against each segment of the group; the
 *   segment with the largest tiou among those with tiou >= thresholds[t] that no earlier prediction took at t (equal tiou:
 *   the higher row) is taken: tp[t, position] = 1 and lock[t, segment row] = position - group_pos0[g], the prediction's rank
 *   inside its class.  tp [T, n_pred] must be zero-filled and lock [T, n_gt] filled with -1 by the caller: a prediction
 *   that takes nothing (or belongs to no group: no ground truth of its class in its video) keeps 0 - a false positive, the
 *   false-positive flag is 1 - tp.  work: n_gt uint32 of scratch (lock bits of groups of more than 256 segments; need not
 *   be cleared).  One launch, one wavefront per group, no atomics; does not allocate, synchronise or read device memory on
 *   the host.
 * timhip_det_ap: tp as above, class c's predictions are positions [class_off[c], class_off[c + 1]) (n_classes + 1 values),
 *   npos[c] its number of ground-truth segments.  ap[t, c] ([T, n_classes] double) = the sum over the true positives k of
 *   the class of (tpc_k / npos - (tpc_k - 1) / npos) * max_{j >= k} tpc_j / (j + 1), tpc the inclusive count of true
 *   positives and k the rank inside the class: interpolated_prec_rec.  A class without predictions gets 0.  One launch.
 * Both return TIMHIP_EINVAL on T outside 1 .. TIMHIP_DET_MAX_THRESHOLDS, a negative count or (with work to do) a null
 * pointer, TIMHIP_EUNSUPPORTED on counts beyond int32; with no group, no prediction or no class they launch nothing and
 * leave their outputs as the caller filled them. */
#define TIMHIP_DET_MAX_THRESHOLDS 16
int timhip_det_match(const double* pred_seg, int64_t n_pred, const int32_t* group_pred, const int32_t* group_pred_lo,
                     const int32_t* group_pred_hi, const int32_t* group_pos0, const double* gt_seg, int64_t n_gt,
                     const int32_t* group_gt_off, int n_groups, const double* thresholds, int T, uint8_t* tp, int32_t* lock,
                     uint32_t* work, void* stream);
int timhip_det_ap(const uint8_t* tp, int64_t n_pred, const int32_t* class_off, const int32_t* npos, int n_classes, int T,
                  double* ap, void* stream);

/* ---------------------------------------------------------------- sliding-window batch assembly */
/* recognition datasets/sliding_window.py:341-421 (__getitem__) for a batch, on feature stores resident in HBM.
 * feats [sum_v N_feat(v) * num_aug, C] fp32: every video's [N_feat, num_aug, C] array, concatenated;
 * video_row0[w] = first feature row (before the num_aug factor) of window w's video; feat_indices [W, num_feats] (int32);
 * windows [B] = the window ids of the batch; aug_indices [B*num_feats] in [0, num_aug) or NULL (0).
 * out [B, num_feats, C] = feats[(video_row0[w] + feat_indices[w, j]) * num_aug + aug[b, j]]            (:352-358, :364-370) */
int timhip_window_gather(const float* feats, int C, int num_aug, const int64_t* video_row0, const int32_t* feat_indices,
                         int num_feats, const int32_t* windows, int B, const int32_t* aug_indices, float* out,
                         void* stream);
/* times [B, T, 2], T = (v ? nf : 0) + (a ? nf : 0) + max_v + max_a, rows ordered vis feats | aud feats | v queries | a queries:
 * clamp((t - start_sec[w]) / window_size, min=0)   (:359-360, :371-372, :402-404).  *_feat_times [rows, ld >= 2] per-video
 * feature (start, end) tables concatenated like feats (without the num_aug factor); *_queries [W, max, 2] zero padded. */
int timhip_window_times(const float* v_feat_times, int v_ld, const int64_t* v_row0, const float* a_feat_times, int a_ld,
                        const int64_t* a_row0, const int32_t* feat_indices, int num_feats, const int32_t* windows, int B,
                        const float* v_queries, int max_v, const float* a_queries, int max_a, const float* start_sec,
                        float window_size, float* times, void* stream);

/* ---------------------------------------------------------------- device-side batch sampler (additive to ABI 6) */
/* Draw: the batch of ONE training iteration of a seeded, epoch-shuffled, rank-sharded order, nothing on the host taking part.
 * counter: one 64-bit word in device memory, the number of the NEXT iteration; the kernel (one block) reads it (t), stores t + 1
 * (one thread, after every thread has read it) and writes iteration t's batch, so the k-th draw is the same bits whether its
 * launch is eager or the k-th replay of a captured graph.  Everything below is integer arithmetic on (seed, t, the arguments).
 *   geometry    N = num_windows, W = world, r = rank, B.  per_rank = ceil(N / W) (torch's DistributedSampler with drop_last =
 *               False); I = iterations per epoch = ceil(per_rank / B) with last = TIMHIP_SAMPLER_WRAP, floor(per_rank / B) with
 *               TIMHIP_SAMPLER_DROP (I = 0: TIMHIP_EINVAL).  e = t / I, k = t % I.  Row b: p = k * B + b, valid[b] = p < per_rank,
 *               g = (p % per_rank) * W + r, i = g % N, window[b] = shuffle ? perm(seed, e, i) : i.  The valid rows of an epoch
 *               over all ranks are the epoch's permutation followed by its own head as padding, dealt round-robin - the lists
 *               DistributedSampler builds (its own randperm stream is not reproduced); a short last batch becomes rows with
 *               valid = 0, which still carry a real (wrapped) window number.
 *   perm        a keyed bijection of [0, N) computed per element, no table: a balanced Feistel network with cycle walking.
 *               bits = max(2, bit_length(N - 1)), h = (bits + 1) / 2, domain 2^(2h) in [N, 4N).  v = (L << h) | R; 6 rounds
 *               (L, R) <- (R, L ^ (F & (2^h - 1))) with F = word x of philox4x32_7(key = seed, site = SITE_SAMPLER (9), counter
 *               ((e mod 2^23) << 40) | (round << 32) | R); repeated while the value is >= N (a bijection of the domain returns
 *               to [0, N): the walk needs no cap; the longest over all elements is 40 passes at N = 4097, 26 at N = 100000).
 *               The order repeats after 2^23 epochs; the Python wrapper refuses to be set beyond.
 *   aug         v_aug / a_aug int32 [B, num_feats] (NULL: modality absent), one index per (row, feature, modality) in
 *               [0, num_aug): (uint64(word) * num_aug) >> 32 with element q = b * num_feats + j reading word q & 3 of the Philox
 *               block with counter 2^63 | ((t mod 2^40) << 23) | (modality << 22) | (q >> 2), modality 0 visual, 1 audio (bit
 *               63 keeps these blocks apart from the permutation's).  B * num_feats <= TIMHIP_SAMPLER_MAX_AUG, else TIMHIP_EINVAL.
 *   outputs     window int32 [B], valid uint8 [B]; epoch, iteration: int64 words (NULL: not written) = e and k of the batch
 *               just written.
 * TIMHIP_EINVAL: counter / window / valid NULL, N < 1, W < 1, rank outside [0, W), B outside [1, 2^20], last not one of the two,
 * an aug pointer with num_aug < 1 or num_feats < 1.  A refused call launches nothing: the counter keeps its value.  The dropout
 * salt takes no part. */
#define TIMHIP_SAMPLER_WRAP 0
#define TIMHIP_SAMPLER_DROP 1
#define TIMHIP_SAMPLER_MAX_AUG (1 << 24)
int timhip_sampler_draw(uint64_t seed, uint64_t* counter, int num_windows, int world, int rank, int B, int shuffle, int last,
                        int num_feats, int v_num_aug, int a_num_aug, int32_t* window, uint8_t* valid, int32_t* v_aug,
                        int32_t* a_aug, int64_t* epoch, int64_t* iteration, void* stream);

/* Batch assembly from DEVICE words, one launch: what timhip_window_gather (per modality), timhip_window_times and the label
 * gathers of a batch produce, written to caller-owned outputs.  Tables as above (feats, feat_times with leading dimension ld >=
 * 2, row0, feat_indices [W, num_feats], queries [W, max, 2], start_sec [W]) plus v_labels / a_labels int64 [W, max, 4] (verb,
 * noun, action, class id; -1 padded) and v_ids / a_ids int64 [W, max] (-1 padded).  v_feats / a_feats NULL: that modality is
 * absent (its feat_times must be NULL too) and its outputs are not touched.
 *   window int32 [B], valid uint8 [B], v_aug / a_aug int32 [B, num_feats] (NULL: index 0): device words, read by the kernel.  A
 *   window outside [0, num_windows) or an index outside [0, num_aug) is read as 0: nothing is read out of bounds.
 *   visual [B, num_feats, Cv], audio [B, num_feats, Ca] fp32: the rows timhip_window_gather copies; 16-byte accesses for
 *   a row whose source and destination are 16-byte aligned and whose width is a multiple of 4, element by element otherwise.
 *   times [B, T, 2]: timhip_window_times to the bit (one IEEE subtraction, one IEEE division, max with 0).
 *   verb, noun, action, v_action_ids int64 [B, max_v]; class_id, a_action_ids int64 [B, max_a]: the window's entries where
 *   valid[b] != 0, -1 ("no query") in a row with valid[b] == 0; features and times of such a row are the wrapped window's.
 * A flat work index over (section, row, item; a feature item is up to four 16-byte chunks), at most 2048 blocks of 256 threads.  TIMHIP_EINVAL on a null pointer that
 * the shape needs, B / num_windows / num_feats < 1, window_size <= 0; TIMHIP_EALIGN on a float pointer off 4 bytes. */
typedef struct TimWindowBatch {
  const float* v_feats; const float* a_feats;
  const float* v_feat_times; const float* a_feat_times;
  const int64_t* v_row0; const int64_t* a_row0;
  const int32_t* feat_indices;
  const float* v_queries; const float* a_queries; const float* start_sec;
  const int64_t* v_labels; const int64_t* a_labels; const int64_t* v_ids; const int64_t* a_ids;
  const int32_t* window; const uint8_t* valid; const int32_t* v_aug; const int32_t* a_aug;
  float* visual; float* audio; float* times;
  int64_t* verb; int64_t* noun; int64_t* action; int64_t* class_id; int64_t* v_action_ids; int64_t* a_action_ids;
  int32_t Cv, Ca, v_num_aug, a_num_aug, v_ld, a_ld, num_feats, max_v, max_a, B, num_windows;
  float window_size;
} TimWindowBatch;
int timhip_window_batch(const TimWindowBatch* desc, void* stream);

/* Batch assembly of the DETECTION dataset (reference detection/.../datasets/sliding_window.py:324-399 plus default_collate) from
 * the device words timhip_sampler_draw writes, one launch into caller-owned outputs.  Tables: feats, feat_times (leading
 * dimension ld >= 2), row0, feat_indices [W, num_feats] and start_sec fp32 [W] as in timhip_window_batch; v_segments /
 * a_segments fp32 [W, max, 2], the stored ground-truth segments in seconds (0 padded); v_labels / a_labels int64 [W, max, 4]
 * (verb, noun, action, class id; -1 padded: a slot whose four words are all -1 holds no action); window_start_sec float64 [W] and
 * video_of int32 [W] (the window's index in the dataset's sorted video list).  v_feats / a_feats NULL: that modality is absent (its
 * feat_times must be NULL too) and its outputs are not touched; at least one is present.
 *   window, valid, v_aug / a_aug: device words as in timhip_window_batch, with the same reading of a word outside its table as 0.
 *   visual [B, num_feats, Cv], audio [B, num_feats, Ca] fp32: the rows timhip_window_batch copies, by the same code.
 *   times fp32 [B, T, 2], T = num_feats per present modality (visual rows first; the model builds its own queries): per element
 *       d = t - start_sec[w]                 one IEEE fp32 subtraction
 *       r = rintf(d * 1000.0f) / 1000.0f     a correctly rounded fp32 product, round half to even, a correctly rounded fp32
 *                                            division: torch.round(d, decimals=3) on fp32 (not a product with 0.001f, not double)
 *       out = fmaxf(r / window_size, 0)      one IEEE fp32 division
 *   v_gt_segments fp32 [B, max_v, 2], a_gt_segments fp32 [B, max_a, 2]: the same three steps on the stored segment; exactly 0.0
 *   in a padded slot and in every slot of a row with valid[b] == 0.
 *   verb, noun, action int64 [B, max_v], class_id int64 [B, max_a]: the window's entries (action reads label column action_col
 *   in 0..2), -1 in a padded slot and in a row with valid[b] == 0.
 *   window_start float64 [B] = window_start_sec[w], video_index int32 [B] = video_of[w]: the wrapped window's, also where
 *   valid[b] == 0, as features and times are.
 * A flat work index over (section, row, item), feature sections first, at most 2048 blocks of 256 threads.  TIMHIP_EINVAL on a
 * null pointer that the shape needs, B / num_windows / num_feats < 1, window_size <= 0, action_col outside 0..2, a modality's
 * times without its features, no modality; TIMHIP_EALIGN on a float pointer off 4 bytes or a double pointer off 8.  A refused
 * call launches nothing. */
typedef struct TimDetWindowBatch {
  const float* v_feats; const float* a_feats;
  const float* v_feat_times; const float* a_feat_times;
  const int64_t* v_row0; const int64_t* a_row0;
  const int32_t* feat_indices;
  const float* v_segments; const float* a_segments; const float* start_sec;
  const double* window_start_sec; const int32_t* video_of;
  const int64_t* v_labels; const int64_t* a_labels;
  const int32_t* window; const uint8_t* valid; const int32_t* v_aug; const int32_t* a_aug;
  float* visual; float* audio; float* times; float* v_gt_segments; float* a_gt_segments;
  int64_t* verb; int64_t* noun; int64_t* action; int64_t* class_id;
  double* window_start; int32_t* video_index;
  int32_t Cv, Ca, v_num_aug, a_num_aug, v_ld, a_ld, num_feats, max_v, max_a, B, num_windows, action_col;
  float window_size;
} TimDetWindowBatch;
int timhip_det_window_batch(const TimDetWindowBatch* desc, void* stream);

/* 16-bit feature stores (additive to ABI 6).  The three feature movers above with the element type of the visual and of the
 * audio store named beside their arguments: under these entries feats / v_feats / a_feats point at elements of that type (the
 * descriptors keep their layout and their `const float*` fields; every other table and every output is what it is above).
 *   TIMHIP_STORE_F32    the entries above: with fp32 for every store a call runs the same kernel and writes the same bits
 *   TIMHIP_STORE_F16    IEEE binary16; the fp32 output element is the exact widening of the stored value, subnormals honoured
 *                       (not flushed), +-0 and +-inf kept, a NaN stays a NaN
 *   TIMHIP_STORE_BF16   the upper half of an fp32 word; the fp32 output element is the stored word shifted left by 16 bits
 * A 16-bit row moves in 16-byte chunks of 8 elements, each becoming two 16-byte fp32 stores, where the width is a multiple of 8
 * and source row and destination row are 16-byte aligned; element by element otherwise.  Times, segments, labels, ids, window
 * start, video index, the rows with valid[b] == 0 and the reading of a window or augmentation word outside its table as 0 are
 * the code of the entries above.  The store type of an absent modality (NULL feats) is checked against the enum and otherwise
 * unused.  TIMHIP_EINVAL on a store type outside the enum, TIMHIP_EALIGN on a 16-bit store pointer off 2 bytes, and every refusal
 * of the entry above (an fp32 store pointer off 4 bytes among them: the gather entry has no alignment refusal for fp32); a
 * refused call launches nothing. */
enum { TIMHIP_STORE_F32 = 0, TIMHIP_STORE_F16 = 1, TIMHIP_STORE_BF16 = 2 };
int timhip_window_gather_st(const void* feats, int store, int C, int num_aug, const int64_t* video_row0,
                            const int32_t* feat_indices, int num_feats, const int32_t* windows, int B,
                            const int32_t* aug_indices, float* out, void* stream);
int timhip_window_batch_st(const TimWindowBatch* desc, int v_store, int a_store, void* stream);
int timhip_det_window_batch_st(const TimDetWindowBatch* desc, int v_store, int a_store, void* stream);

/* DRLoc sample positions (reference helpers/losses/drloc.py:4-7) from a device counter of their own: one block reads the counter
 * (c), stores c + 1 and writes draw c.  pos_1, pos_2 int64 [n, m] in [0, l): (uint64(word) * l) >> 32, element i = row * m + col
 * reading words (x, y) of the Philox block with key = seed, site = SITE_DRLOC (10), counter ((c mod 2^40) << 24) | (i >> 1) when
 * i is even and words (z, w) when it is odd.  deltax fp32 [n, m] = float(|pos_1 - pos_2|) * (1.0f / float(l)): the conversion is
 * exact, the reciprocal is one IEEE division and the product one IEEE multiplication - the bits torch gives on the device for
 * abs((pos_1 - pos_2).float()) followed by `/= l` (a tensor divided by a host scalar is multiplied by the scalar's reciprocal
 * there; for l = 6, 7, 50 some quotients differ from x / l in the last place).  1 <= l <= 2^24, n, m >= 1, n * m <= TIMHIP_DRLOC_MAX_SAMPLES and no null pointer, else
 * TIMHIP_EINVAL (nothing launched, the counter keeps its value). */
#define TIMHIP_DRLOC_MAX_SAMPLES (1 << 25)
int timhip_drloc_draw(uint64_t seed, uint64_t* counter, int n, int m, int l, int64_t* pos_1, int64_t* pos_2, float* deltax,
                      void* stream);

/* ---------------------------------------------------------------- AVGA pooling of the AVE recipe (additive to ABI 6) */
/* Audio-guided visual attention pooling (reference helpers/pool.py:6-43, models/tim.py:137-144): per pooled row r (one time step
 * of one window) with cells X[r] : [S, Cv] and audio a[r] : [Ca]
 *   hv = relu(X W_video^T + b_video) [S, H]      ha = relu(W_audio a + b_audio) [H]      g = W_g ha [S]  (indexed by the CELL)
 *   c[s, j] = (W_v hv[s])[j] + g[s]              z[s] = sum_j w_h[j] tanh(c[s, j])        alpha = softmax_s(z)
 *   out[r] = sum_s alpha[s] X[r, s]              [Cv]
 * TimAvga describes one call: video = fp32 cells, row r at video + r * pitch floats ([S, Cv] contiguous inside a row; pitch >=
 * S * Cv, a multiple of 4: a [B, T, 7, 7, Cv] tensor is read in place); audio [R, ld_audio >= Ca] fp32 with ANY row stride and
 * the 4-byte alignment of a float (the kernels make their own zero-padded operand copy of it); the weights as operand-dtype
 * copies [N, ld] (K-contiguous, ld a multiple of 64, zero padded: what timhip_cast_weights writes) - w_video [H, >= Cv],
 * w_audio [H, >= Ca], w_v [S, >= H], w_g [S, >= H]; the backward also takes the TRANSPOSED copies w_v_t, w_g_t [H, >= 64] and, in
 * the 16-bit precisions, the SPLIT copies w_video_s [H, ld = 3 ru(Cv)], w_audio_s [H, ld = 3 ru(Ca)] as timhip_split3_many writes them in
 * mode 1 ([hi | hi | lo]; the leading dimension is exactly three blocks, anything else is TIMHIP_EALIGN) (all NULL in a forward); fp32 b_video [H], b_audio [H], w_h [S].
 * Supported: 1 <= S <= 64 with S == map_size, H == Cv, Cv a multiple of 64 in [64, 1024], Ca >= 1, R >= 1 with R * S * Cv < 2^31,
 * TIMHIP_PREC_BF16 / _F16 / _FP32 - everything else TIMHIP_EUNSUPPORTED (TIMHIP_PREC_BF16X3 included); NULL pointers, a pitch
 * below S * Cv or a leading dimension below its width TIMHIP_EINVAL; pitches / leading dimensions / pointers off their
 * alignment (16 bytes, audio 4; weight ld % 64) TIMHIP_EALIGN; a workspace below timhip_avga_workspace_bytes TIMHIP_EWORKSPACE. */
typedef struct TimAvga {
  const float* video;
  const float* audio;
  const void* w_video;
  const void* w_audio;
  const void* w_v;
  const void* w_g;
  const void* w_v_t;
  const void* w_g_t;
  const void* w_video_s;
  const void* w_audio_s;
  const float* b_video;
  const float* b_audio;
  const float* w_h;
  int64_t pitch;
  int32_t R, S, Cv, Ca, H, map_size;
  int32_t ld_audio, ld_w_video, ld_w_audio, ld_w_v, ld_w_g, ld_w_v_t, ld_w_g_t, ld_w_video_s, ld_w_audio_s, reserved;
} TimAvga;
/* the seven parameter gradients, fp32, contiguous, shaped like the parameters */
typedef struct TimAvgaGrads {
  float* w_video;   /* [H, Cv] */
  float* b_video;   /* [H] */
  float* w_audio;   /* [H, Ca] */
  float* b_audio;   /* [H] */
  float* w_v;       /* [S, H] */
  float* w_g;       /* [S, H] */
  float* w_h;       /* [S] */
} TimAvgaGrads;
/* bytes of workspace for one call (backward != 0: timhip_avga_bwd); 0 for a shape or precision outside the supported set */
size_t timhip_avga_workspace_bytes(int precision, int R, int S, int Cv, int Ca, int backward);
/* out [R, ldo >= Cv] fp32 (ldo % 4 == 0) and, when alpha != NULL, alpha [R, ld_alpha >= S] fp32.  One fused kernel over the
 * pooled rows behind two [R]-row products (ha, g: timhip_gemm_nt into the workspace): hv and c never reach memory, nothing with
 * R * S rows is written.  16-bit precisions round X, W_video, hv, W_v, a, W_audio, ha, W_g to the operand dtype where the
 * matrix cores read them; the weighted sum over the cells reads the fp32 cells.  Deterministic (no atomics). */
int timhip_avga_fwd(int precision, const TimAvga* p, float* out, int ldo, float* alpha, int ld_alpha, void* workspace,
                    size_t workspace_bytes, void* stream);
/* PARAMETER gradients of timhip_avga_fwd for the cotangent d_out [R, ldd >= Cv] fp32: all seven tensors of `grads` are WRITTEN
 * (not accumulated) at true scale; no input gradient.  Nothing of the forward is needed: hv, c and alpha are recomputed per row.
 * Two [R * S, Cv] operand-dtype intermediates live in the workspace (d_pre and the cast cells; timhip_wgrad's kernels turn them
 * into dW_video / db_video).  16-bit precisions: the relu MASKS of the backward (hv > 0, ha > 0) are taken from split products
 * (x_hi w_hi + x_lo w_hi + x_hi w_lo, about twice the operand's mantissa) - with 16-bit operands alone, pre-activations that
 * rounding moves across zero flip mask bits, each a full-size term of dW_video / dW_audio; hv and ha themselves stay the
 * forward's.  grad_scale: NULL, or (TIMHIP_PREC_F16 only) the 8-word block of timhip_grad_scale - the 16-bit
 * gradient operands are stored times S, the outputs multiplied by 1/S, and word 4 is ORed when a gradient written is inf / nan.
 * ORDER OF ADDITIONS: dW_v and dw_h are summed over the pooled rows with float atomics (one add per element per row), so their
 * last bits vary from call to call, as timhip_colsum's do; the other five gradients are reduced in a fixed order in the 16-bit
 * precisions (TIMHIP_PREC_FP32: db_video and db_audio end in the transposing kernel's atomics as well). */
int timhip_avga_bwd(int precision, const TimAvga* p, const float* d_out, int ldd, const TimAvgaGrads* grads,
                    const float* grad_scale, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------- measurement hook (bench.py roofline) */
/* While armed, every NT / TN GEMM launch of at least min_flops algorithmic FLOPs (2*M*N*K) is bracketed by two HIP events
 * recorded on the stream it is launched on (up to `capacity` launches).  stop() waits for them and returns the summed
 * durations [ms], the summed FLOPs and the number of launches.  Not thread-safe against concurrent start/stop. */
int timhip_gemm_timing_start(int capacity, double min_flops);
int timhip_gemm_timing_stop(double* total_ms, double* total_flops, int* launches);
/* ABI 6: the same stop, per kernel family - [0] the GEMM launches (work = FLOPs), [1] the attention launches, [2] the LayerNorm
 * launches (work = their algorithmic bytes: operand rows read + rows written); each array has three entries.  While armed the
 * attention / LayerNorm launches are bracketed like the GEMMs (no min_flops filter). */
int timhip_timing_stop_families(double* ms3, double* work3, int* launches3);

#ifdef __cplusplus
}
#endif
#endif /* TIMHIP_H */

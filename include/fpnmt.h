/*
 * fpnmt.h — C-ABI of the MI355X-native FPN + multi-view-transformer captioning
 * hot path (libfpnmt.so, gfx950 only).
 *
 * Every entry point replaces a TensorFlow/Keras op that the reference calls on
 * its training / decoding path (samkoesnadi/fpn-MT-image-captioning; all
 * file:line below point into that repository):
 *
 *   fpnmt_conv2d_*         Conv2D            models/retinanet.py:55-62,94-100,118-138,287-294,
 *                                            keras-resnet convs behind models/resnet.py:99,101
 *   fpnmt_gemm             Dense / MatMul    models/transformer.py:88,102,117-121,153,165-168,211-214,357
 *   fpnmt_attention_*      scaled_dot_product_attention  models/transformer.py:70-104
 *   fpnmt_fpn_topdown_*    UpsampleLike + Add           models/retinanet.py:119,123-125,129-130; layers/_misc.py:39-42
 *   fpnmt_maxpool2d_*      MaxPooling2D()               models/retinanet.py:135,139,293 (+ keras-resnet pool1)
 *   fpnmt_spatial_softmax_* CoAttention_CNN.call        models/coattention.py:13-32
 *   fpnmt_layernorm_*      LayerNormalization(1e-6)     models/transformer.py:170-171,216-218,264
 *   fpnmt_embed_posenc_*   Embedding + positional enc.  models/transformer.py:314,326-329
 *   fpnmt_xent_fwd_bwd     masked sparse CE             utils/pipeline.py:50-57
 *   fpnmt_amsgrad_step     Adam(amsgrad, clipnorm=1)    utils/pipeline.py:29-30,78; utils/utils.py:45-50
 *   fpnmt_dropout          Dropout(rate)                models/transformer.py:173-174,219-222,262,319
 *   fpnmt_decode_attention scaled_dot_product_attention, last query row   utils/pipeline.py:105-113
 *   fpnmt_beam_step        softmax + top_k + gather + argmax of predict   utils/pipeline.py:115-147
 *   fpnmt_beam_step_log, fpnmt_beam_finalize   beam search proper (log-prob beams, n-best)   not in the reference
 *   fpnmt_beam_step_groups                     diverse beam search (beam groups, Hamming penalty) not in the reference
 *   fpnmt_sample_step, fpnmt_sample_uniform    sampled decoding (temperature, top-k, top-p)    not in the reference
 *   fpnmt_logits_constrain                     n-gram blocking, repetition penalty, min length  not in the reference
 *   fpnmt_ciderd_reward, fpnmt_scst_pack       CIDEr-D reward and advantages on the device     not in the reference
 *   fpnmt_ciderd_consensus                     consensus (MBR) caption selection under CIDEr-D not in the reference
 *   fpnmt_logits_ensemble                      several models' logits rows folded into one     not in the reference
 *   fpnmt_xent_distill_fwd_bwd                 smoothed CE mixed with KL to teachers' rows     not in the reference
 *
 * Conventions (all functions):
 *   - Return 0 on success or a negative FPNMT_E* code; never throw across the ABI.
 *     fpnmt_last_error() returns a thread-local message for the last failure.
 *   - Memory is caller-owned device memory; pointers are never retained.
 *   - Work is enqueued on the given stream only: no allocation, no device
 *     synchronisation, no host blocking — every call is hipGraph-capturable.
 *   - Activations are NHWC; conv weights HWIO (Keras layout) for the fp32 master
 *     copy, OHWI ("fwd") and flipped IHWO ("bwd") for the compute copies made by
 *     fpnmt_weight_prep. Dense kernels are (in, out) like Keras.
 *   - dtype selects the element type of activations / compute weights:
 *     FPNMT_F32 (exact f32 MFMA path, parity mode) or FPNMT_BF16 (bf16 MFMA,
 *     fp32 accumulate). Master weights, gradients and optimizer state are fp32.
 */
#ifndef FPNMT_H
#define FPNMT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* fpnmt_stream_t; /* hipStream_t */

enum { FPNMT_F32 = 0, FPNMT_BF16 = 1 };
enum { FPNMT_ACT_NONE = 0, FPNMT_ACT_RELU = 1, FPNMT_ACT_LEAKY = 2, FPNMT_ACT_RELU6 = 3 };
enum {
  FPNMT_OK = 0,
  FPNMT_E_ARG = -1,         /* bad descriptor / null pointer / inconsistent sizes */
  FPNMT_E_UNSUPPORTED = -2, /* shape or alignment not handled by any kernel */
  FPNMT_E_HIP = -3          /* HIP launch error */
};

/* ---- library ---------------------------------------------------------- */
const char* fpnmt_last_error(void);
int fpnmt_version(void);
/* Build provenance: the first 16 hex digits of the sha256 over the csrc/
 * sources, headers, Makefile and this header the library was built from
 * (csrc/Makefile BUILD_ID). fpnmt/_lib.py refuses a library whose id does not
 * match the tree it sits in (a stale prebuilt .so). */
const char* fpnmt_build_id(void);
/* Zero `bytes` of device memory as a kernel node (a captured hipMemsetAsync
 * was measured not to re-zero on graph replay; tools/probes/conv_noise.py):
 * the gradient arena's per-step zeroing. */
int fpnmt_fill_zero(void* p, long long bytes, fpnmt_stream_t stream);
/* fpnmt_fill_zero on at most max_blocks workgroups (a 16-B aligned buffer;
 * else it is fpnmt_fill_zero): the gradient arena's zeroing as a trickle on a
 * side stream beside the forward pass (TrainEngine, zero_grad_overlap_grid),
 * instead of a full-chip fill on the critical path (keras' fresh tape
 * gradients per tape.gradient, utils/pipeline.py:77).                      */
int fpnmt_fill_zero_grid(void* p, long long bytes, int max_blocks, fpnmt_stream_t stream);

/* Process-wide GEMM workspace (device memory, ZERO-initialised by the caller,
 * >= 72 KiB, 256-B aligned; NULL detaches). Under-filled small-M GEMMs split
 * K across blocks and combine the partial tiles here in a fixed order (the
 * result is deterministic); the per-tile arrival counters are re-zeroed by
 * the kernels, so the buffer stays valid across launches and graph replays.
 * GEMMs using it must not run concurrently on different streams.          */
int fpnmt_set_workspace(void* ws, long long bytes);

/* Test / probe hook: the tile form of the wide bf16 conv classes, process-wide.
 * 0 (the default): chosen per launch by tile count. 6: the 128-row M step in
 * both classes (128x256 loader tile, cfg 6; 128x128 loader tile, cfg 7).
 * 10: the 112-row M step on the 128x256 tile (cfg 10); the 128x128 class stays
 * automatic. 12: the 144-row M step on a 160x256 image (cfg 12) for every
 * bf16 conv with N >= 256 and 64-channel K-tiles, whatever its tile count and
 * K, and every grouped launch's levels in one launch; the 128x128 class is
 * not reached. Every form computes the same bytes (tests/test_gpu_kernels.py:
 * test_conv_wide_tiles_bitwise, tests/test_gpu_heads_one_launch.py); only the
 * tiling differs. Any other value: FPNMT_E_ARG, the setting unchanged.
 * Callers reset it to 0 when done.
 * fpnmt_get_wide_cfg: the current setting.                                  */
int fpnmt_set_wide_cfg(int cfg);
int fpnmt_get_wide_cfg(void);

/* The launch plan of a grouped bf16 conv (fpnmt_conv2d_fwd_grouped,
 * fpnmt_conv2d_bwd_data_grouped*) whose launches can take the wide tile
 * class: level_rows[0 .. n_levels) are the levels' output rows (n_levels <=
 * 6), n_out the GEMM's N (the output channels), k_red its K (r * s * c), cus
 * the chip's CU count. Returns the number of launches L (< 0: FPNMT_E_ARG) and
 * fills, per launch in level order, how many levels it takes, the M step of
 * its tiles as a wide-class launch (112, 128 or 144 rows) and its tile count
 * at that step; each out pointer holds n_levels entries or is NULL. Pure host
 * arithmetic with the automatic setting of fpnmt_set_wide_cfg: no device is
 * touched (csrc/wide_plan.h has the cost model).                            */
int fpnmt_plan_wide_levels(int n_levels, const long long* level_rows, int n_out, int k_red, int cus,
                           int* launch_levels, int* launch_ms, long long* launch_tiles);

/* Deferred ordered reductions. Between fpnmt_defer_begin and
 * fpnmt_defer_flush, the ordered second passes of the fp32 gradient
 * reductions — split-K weight-gradient slabs -> dw (bwd-filter / transposed
 * GEMMs with accumulate = 2), per-chunk column partials -> bias / LayerNorm
 * gamma / beta gradients (fpnmt_act_bwd, fpnmt_layernorm_bwd) — keep their
 * inputs in `arena` (device memory, 256-B aligned, caller-owned, untouched
 * until the flush) and are queued instead of launched; fpnmt_defer_flush
 * enqueues them on `stream` as a few batched launches. Results are bitwise
 * those of immediate mode (each reduction keeps its order; a reduction into
 * a destination that already has a queued one, or an immediate accumulation
 * into it, runs the queue first) — except the Dense weight-gradient GEMMs
 * entered through fpnmt_gemm_wgrad (below), which the flush runs as whole-K
 * tiles: equal to immediate mode up to fp32 summation order. Gradients are
 * complete only after the flush. A full arena falls back to immediate
 * reductions. Single stream. A plain fpnmt_gemm is never queued.
 * fpnmt_defer_peak_bytes: the most arena bytes in use so far.              */
int fpnmt_defer_begin(void* arena, long long bytes);
int fpnmt_defer_flush(fpnmt_stream_t stream);
long long fpnmt_defer_peak_bytes(void);
/* Conv weight-gradient GEMMs in the deferred queue. classes: bit mask of the
 * LDS-DMA weight-gradient tile classes (bit 0 128x128, 1 128x64, 2 64x256,
 * 3 128x256 with loader waves, 4 256x128); 0 (the default): none. While a bit
 * is set, a split (split-K > 1) launch of that class made by
 * fpnmt_conv2d_bwd_filter / _bias inside a deferred region, whose slabs fit
 * the arena, is queued and runs at the flush in grouped launches, ahead of its
 * queued slab reduce: THE CALLER KEEPS x AND dz ALIVE AND UNCHANGED UNTIL THE
 * FLUSH. The gradients are bitwise those of the immediate launches. Not
 * queued: the grouped (multi-level) entry points, unsplit launches, the other
 * kernels, slabs that fell back to the workspace. Set outside a region.    */
int fpnmt_set_defer_conv_wgrads(int classes);

/* ---- general batched GEMM on MFMA (Dense layers, attention products) ---
 * C[z] = epilogue(alpha * op(A[z]) @ op(B[z]))  for z in [0, batch)
 * z is split as (zo, zi) = (z / batch_inner, z % batch_inner); operand X of
 * batch z starts at X + zo*X_so + zi*X_si (elements).
 * a_trans = 0: A is M x K, element (m,k) at A[m*lda + k]
 * a_trans = 1: A is stored K x M, element (m,k) at A[k*lda + m]
 * b_trans = 0: B is stored N x K (k contiguous), element (k,n) at B[n*ldb + k]
 * b_trans = 1: B is stored K x N (n contiguous), element (k,n) at B[k*ldb + n]
 * Epilogue: v = acc*alpha; v *= col_scale[n]; v += bias[n]; v += R[m*ldr+n];
 *           v = act(v); C = v (or C += v when accumulate; atomic when
 *           accumulate == 2, which also allows split-K over blocks).
 * c_f32 = 1 writes C as fp32 regardless of dtype.                        */
typedef struct fpnmt_gemm_desc {
  int m, n, k;
  int batch, batch_inner;
  int dtype;
  int a_trans, b_trans;
  long long lda, ldb, ldc, ldr;
  long long a_so, a_si, b_so, b_si, c_so, c_si, r_so, r_si;
  float alpha;
  int act;
  float act_alpha;
  int accumulate; /* 0 store, 1 read-modify-write, 2 fp32 atomic add */
  int c_f32;
  int split_k;    /* >=1; >1 requires accumulate == 2 */
  /* fused dropout (batch == 1, accumulate != 2): when drop_p > 0 the output is
   * R + dropout(act(alpha*AB*col_scale + bias)) — residual AFTER the dropout —
   * with keep(row, col) = uniform01(key, row*n + col) >= drop_p, scaled by
   * 1/(1-drop_p), key = drop_seed + (*drop_seed_dev) * 0x9E3779B97F4A7C15
   * (the fpnmt_dropout mask of the dense (m, n) output).                   */
  float drop_p;
  unsigned long long drop_seed;
  const long long* drop_seed_dev;
} fpnmt_gemm_desc;

int fpnmt_gemm(const fpnmt_gemm_desc* d, const void* A, const void* B, void* C,
               const float* col_scale, const float* bias, const void* R,
               fpnmt_stream_t stream);
/* Dense weight gradient C (+)= alpha * A^T B (a_trans = b_trans = 1, fp32 C,
 * accumulate 1 or 2, no epilogue ops; same descriptor as fpnmt_gemm).
 * Replaces Keras' kernel gradient of Dense (transformer.py:117-121, 165-168,
 * 211-214, 357 under tape.gradient, utils/pipeline.py:77). Outside a deferred
 * region it is fpnmt_gemm. Between fpnmt_defer_begin and fpnmt_defer_flush
 * it MAY be queued and run at the flush: A and B must then stay valid and
 * unmodified until fpnmt_defer_flush returns, and C is complete only after
 * it (the result equals immediate mode up to fp32 summation order).        */
int fpnmt_gemm_wgrad(const fpnmt_gemm_desc* d, const void* A, const void* B, void* C, fpnmt_stream_t stream);
/* C = (A B) * act_in'(y_in): the backward-data GEMM of a Dense layer whose
 * input y_in is the activated output of the previous Dense (the FFN's
 * ffn2 <- LeakyReLU(ffn1), transformer.py:165-168 / 211-214) with that
 * activation's derivative applied in the epilogue; y_in rows of
 * stride d->ldr. act_in: relu (0/1), relu6 (0/1), leaky_relu (1 / act_alpha,
 * read from the sign of y_in). Plain single GEMMs only (no act, dropout,
 * accumulate, batch).                                                      */
int fpnmt_gemm_act_in(const fpnmt_gemm_desc* d, const void* A, const void* B, void* C, const void* y_in,
                      int act_in, float act_alpha, fpnmt_stream_t stream);

/* ---- fused ResNet identity bottleneck (inference) ----------------------
 * keras-resnet bottleneck_2d, blocks 1.. of a stage (reference
 * models/resnet.py:99-112, keras_resnet.blocks.bottleneck_2d with
 * freeze_bn=True) in ONE launch:
 *   y = relu(x + bc + Wc * relu(b3 + W3 (*) pad1(relu(ba + Wa * x))))
 * x, y: NHWC bf16 (n, h, w, c), y must not alias x; wa: OHWI bf16 (cm, 1, 1,
 * c), w3: (cm, 3, 3, cm), wc: (c, 1, 1, cm) with the frozen BN scale folded
 * (fpnmt_weight_prep); ba / b3 / bc: fp32 folded BN shifts. The same values
 * as the three fpnmt_conv2d_fwd calls up to fp32 summation order (the 64 /
 * 128-channel intermediates are rounded to bf16 as the unfused path stores
 * them). Shapes with a kernel: (h, w, c, cm) = (56, 56, 256, 64) and (28, 28,
 * 512, 128) (ResNet-50/101/152 res2 / res3 at 224^2); any other shape returns
 * FPNMT_E_UNSUPPORTED without launching (the caller runs the three convs).
 * Needs the workspace (fpnmt_set_workspace) for its zero page.            */
int fpnmt_bottleneck_fwd(int n, int h, int w, int c, int cm, const void* x, const void* wa, const float* ba,
                         const void* w3, const float* b3, const void* wc, const float* bc, void* y,
                         fpnmt_stream_t stream);

/* ---- implicit-GEMM convolution ----------------------------------------
 * Output size: ho = (h + pad_t + pad_b - r)/stride_h + 1 (same for w).
 * fwd:   y = act((conv(x, w_ohwi)) * scale[k] + bias[k] + residual)
 *        (scale/bias/residual optional; scale carries a frozen BatchNorm)
 * bwd_data: dx (+)= conv_transpose(dz, w) with w_flip = flipped IHWO copy;
 *        supports stride 1 (any r,s, symmetric pads) and 1x1 stride s, pad 0.
 * bwd_filter: dw_hwio (fp32) += col_scale[k] * sum_pixels im2col(x)^T dz
 *        (atomic accumulate, split-K over pixels).                          */
typedef struct fpnmt_conv_desc {
  int n, h, w, c;
  int k, r, s;
  int stride_h, stride_w;
  int pad_t, pad_b, pad_l, pad_r;
  int dtype;
  int act;
  float act_alpha;
} fpnmt_conv_desc;

int fpnmt_conv2d_fwd(const fpnmt_conv_desc* d, const void* x, const void* w_ohwi,
                     const float* scale, const float* bias, const void* residual,
                     void* y, fpnmt_stream_t stream);
int fpnmt_conv2d_bwd_data(const fpnmt_conv_desc* d, const void* dz, const void* w_flip,
                          void* dx, int accumulate, fpnmt_stream_t stream);
int fpnmt_conv2d_bwd_filter(const fpnmt_conv_desc* d, const void* x, const void* dz,
                            const float* col_scale, float* dw_hwio, fpnmt_stream_t stream);
/* bwd_filter and the layer's bias gradient in one call: also db (fp32 [k]) +=
 * sum over pixels of dz (the Keras Conv2D bias gradient, reference
 * models/retinanet.py Conv2D(use_bias=True) layers under utils/pipeline.py:
 * 64-80's tape.gradient). The column sums ride in the LDS-DMA weight-gradient
 * kernel, which streams dz through LDS anyway (per-(split, m-tile, wave row)
 * partial rows summed in a fixed order); other weight-gradient paths run
 * fpnmt_bias_grad's column pass after it. Deterministic either way.         */
int fpnmt_conv2d_bwd_filter_bias(const fpnmt_conv_desc* d, const void* x, const void* dz,
                                 const float* col_scale, float* dw_hwio, float* db,
                                 fpnmt_stream_t stream);
/* bwd_data with the PRODUCING layer's activation backward fused into the
 * epilogue: dx = conv_transpose(dz, w) * act_in'(y_in), y_in = the (n,h,w,c)
 * activation output that was this conv's input x, act_in = FPNMT_ACT_RELU or
 * FPNMT_ACT_RELU6 (0/1 derivatives). Equals fpnmt_conv2d_bwd_data followed by
 * fpnmt_act_bwd(act_in, y_in) bit for bit (a conv chain's backward: the
 * Keras layer pair Conv2D(activation='relu') -> Conv2D). Stride 1 only.    */
int fpnmt_conv2d_bwd_data_act(const fpnmt_conv_desc* d, const void* dz, const void* w_flip,
                              void* dx, const void* y_in, int act_in, fpnmt_stream_t stream);
/* bwd_data into an input gradient that the PRODUCING layer's activation
 * backward is folded into, one consumer at a time (round 6): dx (+)=
 * conv_transpose(dz, w) * act'(y), y = that activation's (n,h,w,c) output
 * (this conv's input x), act = FPNMT_ACT_RELU / RELU6. With accumulate = 1
 * the old dx must already carry the mask (zero where act'(y) = 0: every
 * earlier consumer used this entry); the result is then act'(y) * (old + new),
 * the value fpnmt_conv2d_bwd_data (accumulating) + fpnmt_act_bwd would give
 * (a zero may differ in sign). Stride 1, or 1x1 stride s pad 0 (the rows
 * scattered into the zero-filled / accumulated dx). Replaces the keras-resnet
 * stage output's ReLU backward of tape.gradient (utils/pipeline.py:77) that
 * runs after the stage's consumers (next stage's projection block, FPN
 * lateral conv) have summed their gradients.                              */
int fpnmt_conv2d_bwd_data_mask(const fpnmt_conv_desc* d, const void* dz, const void* w_flip,
                               void* dx, int accumulate, const void* y, int act,
                               fpnmt_stream_t stream);
/* bwd_data with a second gradient of the same input added in the epilogue:
 * dx = conv_transpose(dz, w) + res, res an (n,h,w,c) tensor of the dtype —
 * keras-resnet's identity bottleneck (models/resnet.py: the block input x is
 * conv 2a's input AND the residual of 2c's add), so x's two gradients need no
 * separate add. One rounding of the fp32 sum (bf16); equal to bwd_data then
 * an fp32 add bit for bit in fp32. Stride 1 only.                        */
int fpnmt_conv2d_bwd_data_res(const fpnmt_conv_desc* d, const void* dz, const void* w_flip,
                              void* dx, const void* res, fpnmt_stream_t stream);
/* bwd_data_res followed by the activation backward of the layer that
 * produced the input: dx = (conv_transpose(dz, w) + res) * act_in'(y_in),
 * y_in = the input x itself (the previous bottleneck's ReLU output: its
 * `Activation('relu')` after the Add), act_in = FPNMT_ACT_RELU / RELU6. The
 * mask is applied in the GEMM epilogue where the launch takes the pipe
 * kernel (bf16), else by an in-place pass after it; either way equal to
 * bwd_data_res then fpnmt_act_bwd(act_in, y_in) bit for bit. Stride 1 only. */
int fpnmt_conv2d_bwd_data_res_act(const fpnmt_conv_desc* d, const void* dz, const void* w_flip,
                                  void* dx, const void* res, const void* y_in, int act_in,
                                  fpnmt_stream_t stream);

/* ---- grouped convolution: one shared-weight conv over several inputs ----
 * The retinanet submodels / heads / co-attention convs run ONE weight set
 * over the five pyramid levels (models/retinanet.py:297-301, the
 * `[self.level(f) for f in features]` loop): these launch every level in one
 * grouped implicit GEMM (groups split the output rows for fwd / bwd-data and
 * the pixel reduction for bwd-filter). d gives c, k, r, s, strides, pads,
 * dtype, act; d->n/h/w are ignored (per level below). Levels with no output
 * pixels are skipped (bwd-data zero-fills their dx unless accumulating).
 * bwd-data: stride 1 only.                                                 */
typedef struct fpnmt_conv_level {
  int n, h, w;            /* this level's input shape (n, h, w, c) */
  const void* x;          /* fwd / bwd-filter: input;  bwd-data: dz */
  const void* dz;         /* bwd-filter: output gradient (n, ho, wo, k) */
  const void* residual;   /* fwd: optional (n, ho, wo, k);
                             bwd-data _act: the level's y_in (n, h, w, c) */
  void* y;                /* fwd: output;  bwd-data: dx */
} fpnmt_conv_level;
int fpnmt_conv2d_fwd_grouped(const fpnmt_conv_desc* d, int n_levels, const fpnmt_conv_level* lv,
                             const void* w_ohwi, const float* scale, const float* bias,
                             fpnmt_stream_t stream);
int fpnmt_conv2d_bwd_data_grouped(const fpnmt_conv_desc* d, int n_levels, const fpnmt_conv_level* lv,
                                  const void* w_flip, int accumulate, fpnmt_stream_t stream);
int fpnmt_conv2d_bwd_filter_grouped(const fpnmt_conv_desc* d, int n_levels, const fpnmt_conv_level* lv,
                                    const float* col_scale, float* dw_hwio, fpnmt_stream_t stream);
/* the grouped form of fpnmt_conv2d_bwd_filter_bias: db += the column sums of
 * every level's dz (a shared head conv's bias gradient over P3..P7)         */
int fpnmt_conv2d_bwd_filter_grouped_bias(const fpnmt_conv_desc* d, int n_levels, const fpnmt_conv_level* lv,
                                         const float* col_scale, float* dw_hwio, float* db,
                                         fpnmt_stream_t stream);
/* grouped bwd-data with the producing layer's act' fused (per level y_in in
 * lv[i].residual), as fpnmt_conv2d_bwd_data_act                            */
int fpnmt_conv2d_bwd_data_grouped_act(const fpnmt_conv_desc* d, int n_levels, const fpnmt_conv_level* lv,
                                      const void* w_flip, int act_in, fpnmt_stream_t stream);
/* grouped bwd-data with each level's contribution times act'(y_i), y_i in
 * lv[i].residual (the level input's producing activation output; NULL: that
 * level unmasked), accumulating too (then, as fpnmt_conv2d_bwd_data_mask, the
 * old dx must already carry the mask): the heads' first conv over the FPN
 * levels P3..P5 (ReLU convs, retinanet.py:105-136) into their summed gradient. */
int fpnmt_conv2d_bwd_data_grouped_mask(const fpnmt_conv_desc* d, int n_levels, const fpnmt_conv_level* lv,
                                       const void* w_flip, int accumulate, int act, fpnmt_stream_t stream);

/* Compute copies of an fp32 HWIO master (r,s,c,k), each scaled per output
 * channel k by scale[k] (frozen BN; NULL = 1):
 *   w_ohwi[k][r][s][c]            (forward B operand, row stride r*s*c)
 *   w_flip[c][R-1-r][S-1-s][k]    (backward-data B operand; row c starts at
 *                                  c*ld_flip, ld_flip = 0 means r*s*k — a
 *                                  larger ld interleaves grouped Dense layers)
 * Either destination may be NULL.                                          */
int fpnmt_weight_prep(const float* w_hwio, int r, int s, int c, int k, const float* scale,
                      int dtype, void* w_ohwi, void* w_flip, long long ld_flip, fpnmt_stream_t stream);
/* The same for a whole model in ONE launch: items_dev is a device array of
 * n_items descriptors; tile_start[i] = sum over j < i of r*s*ceil(c/32)*ceil(k/32)
 * and total_tiles the full sum (each 32x32 (c,k) tile is read once and
 * written to both layouts).                                                */
typedef struct fpnmt_wprep_item {
  const float* w_hwio;
  const float* scale;
  void* w_ohwi;
  void* w_flip;
  int r, s, c, k;
  long long tile_start;
  long long ld_flip;   /* as fpnmt_weight_prep; 0 = r*s*k */
} fpnmt_wprep_item;
int fpnmt_weight_prep_batched(const fpnmt_wprep_item* items_dev, int n_items, long long total_tiles,
                              int dtype, fpnmt_stream_t stream);

/* ---- elementwise / reductions ---------------------------------------- */
/* dz = dy * act'(y)   (y is the activation OUTPUT; relu/leaky sign tests);
 * optionally db[c] += sum_rows dz  (rows x c, c = channel count). With a
 * workspace ws of fpnmt_act_bwd_ws_bytes() the column sums go through
 * per-chunk partials and one atomic per column; ws == NULL falls back to
 * one atomic per column per row chunk (contended: ~10x slower for wide c). */
long long fpnmt_act_bwd_ws_bytes(int dtype, long long rows, int c);
/* drop_p > 0: dz also carries the dropout mask of a fused GEMM epilogue
 * (fpnmt_gemm_desc.drop_*; same seed / key), dz = dy * keep / (1 - drop_p)
 * * act'(y), y then being the pre-dropout activation.                     */
int fpnmt_act_bwd(int dtype, long long rows, int c, int act, float act_alpha,
                  const void* dy, const void* y, void* dz, float* db, float* ws,
                  float drop_p, unsigned long long drop_seed, const long long* drop_seed_dev,
                  fpnmt_stream_t stream);
/* out = cast(in) between f32 / bf16; n elements */
/* db += column sums of dy (rows x c): a bias gradient (Dense / Conv2D
 * use_bias with a linear output, or after a fused act' epilogue). Equals
 * fpnmt_act_bwd(act NONE, dz = dy) bit for bit. Between fpnmt_defer_begin and
 * fpnmt_defer_flush the launch is QUEUED (batched with the other queued
 * bias gradients at the flush): dy must stay allocated and unmodified until
 * the flush.                                                               */
int fpnmt_bias_grad(int dtype, long long rows, int c, const void* dy, float* db, fpnmt_stream_t stream);
int fpnmt_cast(int in_dtype, int out_dtype, long long n, const void* in, void* out,
               fpnmt_stream_t stream);
/* y = x * keep / (1-p), keep = u(key, i) >= p with key = seed + *seed_dev
 * (seed_dev: optional device int64, e.g. the optimizer step, so a replayed
 * hipGraph draws a fresh mask every step); in place allowed.              */
int fpnmt_dropout(int dtype, long long n, float p, unsigned long long seed,
                  const long long* seed_dev, const void* x, void* y, fpnmt_stream_t stream);
/* out = a + b (n elements) — residual join of two gradient branches */
int fpnmt_add(int dtype, long long n, const void* a, const void* b, void* out,
              fpnmt_stream_t stream);

/* ---- pooling ----------------------------------------------------------
 * Max pool NHWC, window (kh,kw), stride (sh,sw), pads (pt,pl) — padded taps
 * never win (TF "same" pads with -inf); output size (ho,wo) given.
 * argmax (optional, n*ho*wo*c bytes): window tap r*kw+q of the first max.  */
int fpnmt_maxpool2d_fwd(int dtype, int n, int h, int w, int c, int kh, int kw, int sh, int sw,
                        int pt, int pl, int ho, int wo, const void* x, void* y,
                        uint8_t* argmax, fpnmt_stream_t stream);
/* dx = routed dy (the first max in window order gets the gradient; every dx
 * element is written, gather form, no atomics). Routing comes from argmax
 * when non-null (x may then be null), else is recomputed from x.           */
int fpnmt_maxpool2d_bwd(int dtype, int n, int h, int w, int c, int kh, int kw, int sh, int sw,
                        int pt, int pl, int ho, int wo, const void* x, const uint8_t* argmax,
                        const void* dy, void* dx, fpnmt_stream_t stream);
/* fpnmt_maxpool2d_bwd (argmax routing) times the PRODUCER's activation
 * derivative: dx = routed dy * act'(x), x = the pool's input (that
 * activation's output), act = FPNMT_ACT_RELU / RELU6, or
 * FPNMT_ACT_LEAKY (slope alpha) when the windows do not overlap (kh <= sh,
 * kw <= sw: one rounding, as the separate pass). Equals fpnmt_maxpool2d_bwd
 * + fpnmt_act_bwd(act, x) (a zero may differ in sign): the ResNet stem's
 * ReLU under its max pool (models/resnet.py conv1 -> pool1), the feature
 * extractor's LeakyReLU coatt conv under MaxPooling2D (retinanet.py:292-293),
 * in tape.gradient (utils/pipeline.py:77).                                */
int fpnmt_maxpool2d_bwd_act(int dtype, int n, int h, int w, int c, int kh, int kw, int sh, int sw,
                            int pt, int pl, int ho, int wo, const uint8_t* argmax, const void* dy,
                            const void* x, int act, float alpha, void* dx, fpnmt_stream_t stream);

/* ---- FPN top-down pathway (one sweep) ----------------------------------
 * P4m = lat4 + up(lat5 -> h4 x w4);  P3m = lat3 + up(P4m -> h3 x w3)
 * up = TF2 nearest resize (half-pixel centres): src = min(floor((d+.5)*in/out), in-1)
 * All (n, h_i, w_i, c). bwd: d_lat5 (+)= down(d_P4 + down(d_P3)),
 * d_lat4 = d_P4m + down(d_P3m); d_lat3 = d_P3m (caller aliases, no copy).
 * h3 = w3 = 0 with null lat3 / p3m / d_p3m is the plain upsample-and-add.
 * c must be a multiple of 8 (bf16) / 4 (f32) and every non-null pointer
 * 16-byte aligned (the kernels move 16-byte vectors): FPNMT_E_UNSUPPORTED /
 * FPNMT_E_ARG otherwise, before any launch.                                */
int fpnmt_fpn_topdown_fwd(int dtype, int n, int c, int h5, int w5, int h4, int w4, int h3,
                          int w3, const void* lat5, const void* lat4, const void* lat3,
                          void* p4m, void* p3m, fpnmt_stream_t stream);
int fpnmt_fpn_topdown_bwd(int dtype, int n, int c, int h5, int w5, int h4, int w4, int h3,
                          int w3, const void* d_p4m, const void* d_p3m, void* d_lat4,
                          void* d_lat5, int accumulate_lat5, fpnmt_stream_t stream);

/* ---- co-attention spatial softmax (models/coattention.py:13-32) --------
 * a = softmax over the hw positions of score (n, hw);  ctx = a (x) hs (n, hw, c)
 * fwd also writes a (fp32, n*hw) for the backward.                        */
int fpnmt_spatial_softmax_fwd(int dtype, int n, int hw, int c, const void* score, const void* hs,
                              void* ctx, float* a_out, fpnmt_stream_t stream);
int fpnmt_spatial_softmax_bwd(int dtype, int n, int hw, int c, const float* a, const void* hs,
                              const void* d_ctx, void* d_score, void* d_hs, double* ws,
                              fpnmt_stream_t stream); /* ws: n*hw fp64 (da, kept in fp64) */

/* ---- attention (models/transformer.py:70-104) ---------------------------
 * q: (B, Lq, H*D) rows of stride ldq, head h at column h*D; k, v likewise.
 * mask (optional, fp32): additive mask * -1e9, element (b,h,i,j) at
 *   mask[b*m_sb + h*m_sh + i*m_si + j*m_sj] (strides may be 0 = broadcast).
 * out: (B, Lq, H*D) stride ldo. weights (B,H,Lq,Lk) in dtype, row stride ldw >= lk
 * (padded to a multiple of 8; pad columns are written as 0). ws: fp32
 * scratch of fpnmt_attention_ws_bytes().                                   */
typedef struct fpnmt_attn_desc {
  int b, h, lq, lk, d;
  int dtype;
  long long ldq, ldk, ldv, ldo, ldw;
  float scale;
  long long m_sb, m_sh, m_si, m_sj;
} fpnmt_attn_desc;
size_t fpnmt_attention_ws_bytes(const fpnmt_attn_desc* d);
int fpnmt_attention_fwd(const fpnmt_attn_desc* d, const void* q, const void* k, const void* v,
                        const float* mask, void* out, void* weights, void* ws,
                        fpnmt_stream_t stream);
/* Backward: given dO (ldo), the forward's weights P and the inputs, write dq,
 * dk, dv (same strides as q,k,v). ws as above.                             */
int fpnmt_attention_bwd(const fpnmt_attn_desc* d, const void* q, const void* k, const void* v,
                        const void* weights, const void* d_out, void* dq, void* dk, void* dv,
                        void* ws, fpnmt_stream_t stream);
/* The n <= FPNMT_MAX_VIEWS per-view attentions of one EncoderLayer
 * (transformer.py:184-190: the baseline's query row against each view's
 * keys), each with its own descriptor / pointers (table entry i): the
 * results of n fpnmt_attention_fwd / _bwd calls up to fp32 summation order
 * (the grouped launch runs every view on the multi-wave one-query body; the
 * single-view call sends views with fewer than 128 keys to a one-wave body,
 * so short views such as P6 / P7 may differ in the last bits). Views sharing
 * b, h and scale that are all one-query bf16, D = 64, without a mask run as
 * ONE launch; otherwise the calls are made one by one (ws[i] as above).    */
#define FPNMT_MAX_VIEWS 4
int fpnmt_attention_fwd_views(int n, const fpnmt_attn_desc* d, const void* const* q, const void* const* k,
                              const void* const* v, const float* const* mask, void* const* out,
                              void* const* weights, void* const* ws, fpnmt_stream_t stream);
int fpnmt_attention_bwd_views(int n, const fpnmt_attn_desc* d, const void* const* q, const void* const* k,
                              const void* const* v, const void* const* weights, const void* const* d_out,
                              void* const* dq, void* const* dk, void* const* dv, void* const* ws,
                              fpnmt_stream_t stream);

/* ---- multi-view encoder output (reference models/transformer.py
 * EncoderLayer.call :184-190: out = baseline + sum_i Dropout(mha_i.dense(o_i)))
 * fwd: out (m, n) = R + sum_{i < nseg} dropout_i(A_i W_i + bias[i*n ..]) with
 *   A = the views' attention outputs side by side (m, nseg*k; row stride lda,
 *   view i at column i*k), W = the views' Dense kernels as ONE stacked
 *   (nseg*n, k) k-contiguous operand (rows i*n .. i*n+n-1 = view i's OHWI
 *   copy), bias nseg*n fp32 (optional), R (m, n; optional). Dropout of view i
 *   at (row, col): keep = uniform01(key, row*(nseg*n) + i*n + col) >= drop_p,
 *   scaled by 1/(1-drop_p), key as fpnmt_gemm_desc's — the fpnmt_dropout mask
 *   of the virtual (m, nseg*n) matrix of the views' pre-sum outputs.
 *   nseg == 4 (NUM_OF_PYRAMIDS - 1); k % 16 == 0.
 * bwd_dz: dz (m, nseg*n) = that mask applied to dy broadcast over the views;
 *   db[nseg*n] += dz's column sums (fixed order; optional). The views' dA and
 *   dW are then batched fpnmt_gemm launches over dz.                        */
int fpnmt_view_proj_fwd(int dtype, int m, int n, int k, int nseg, const void* A, long long lda, const void* W,
                        const float* bias, const void* R, long long ldr, void* out, long long ldo, float drop_p,
                        unsigned long long seed, const long long* seed_dev, fpnmt_stream_t stream);
int fpnmt_view_proj_bwd_dz(int dtype, int m, int n, int nseg, const void* dy, long long lddy, void* dz, float* db,
                           float drop_p, unsigned long long seed, const long long* seed_dev,
                           fpnmt_stream_t stream);

/* ---- LayerNorm (eps, last axis, affine), optional fused residual --------
 * x' = x + res (res optional); y = (x'-mu)/sqrt(var+eps)*gamma + beta + pe[row % pe_rows]
 * (pe optional: positional encoding added after the norm, Encoder path).
 * Saves mean/rstd (fp32, rows) for the backward.                           */
int fpnmt_layernorm_fwd(int dtype, long long rows, int d, float eps, const void* x,
                        const void* res, const float* gamma, const float* beta, const float* pe,
                        int pe_rows, void* y, float* mean, float* rstd, fpnmt_stream_t stream);
/* dx = LN'(dy) (x' recomputed from x [+ res]); dgamma/dbeta (fp32) += column
 * sums (per-block partials reduced in block order: deterministic). dx is also
 * the gradient of res.                                                      */
int fpnmt_layernorm_bwd(int dtype, long long rows, int d, const void* x, const void* res,
                        const float* gamma, const float* mean, const float* rstd, const void* dy,
                        void* dx, float* dgamma, float* dbeta, fpnmt_stream_t stream);
/* The Encoder's view LayerNorms (transformer.py:279-292: per view, the shared
 * LayerNormalization, + pe[:L_i], dropout) as ONE launch per pass. View i:
 * x (rows, d) -> y = dropout(LN(x) + pe[row % pe_rows]) with the mask
 * fpnmt_dropout(seed_i) would draw on the (rows, d) output (drop_p 0: none);
 * mean / rstd saved per row. Backward: dx of view i from its dy, the dropout
 * mask applied to dy first; dgamma / dbeta (+=) summed view by view, each
 * view's rows in the order of its own fpnmt_layernorm_bwd (same results).  */
#define FPNMT_MAX_LN_VIEWS 8
typedef struct fpnmt_ln_view {
  const void* x;     /* fwd / bwd: the view's input rows                    */
  void* y;           /* fwd: output;  bwd: dx                                */
  const void* dy;    /* bwd: the gradient of y                               */
  float* mean;
  float* rstd;
  long long rows;
  int pe_rows;       /* fwd with pe: the view's positions (L_i)              */
  unsigned long long seed;
} fpnmt_ln_view;
int fpnmt_layernorm_views_fwd(int dtype, int n, int d, float eps, const fpnmt_ln_view* views,
                              const float* gamma, const float* beta, const float* pe, float drop_p,
                              const long long* seed_dev, fpnmt_stream_t stream);
int fpnmt_layernorm_views_bwd(int dtype, int n, int d, const fpnmt_ln_view* views, const float* gamma,
                              float drop_p, const long long* seed_dev, float* dgamma, float* dbeta,
                              fpnmt_stream_t stream);
/* fpnmt_layernorm_bwd + the backward of the dropout fused into the Dense
 * that produced x (x = dropout(A W + b), transformer.py:232-242 / :190-194):
 * also dz = keep(row * d + col) ? dx / (1 - drop_p) : 0 with the forward
 * GEMM epilogue's mask (drop_seed + *drop_seed_dev * golden), computed from
 * the stored dx exactly as fpnmt_act_bwd would — one launch instead of two.
 * dz (rows x d) feeds that Dense's bias / weight / data gradients.          */
int fpnmt_layernorm_bwd_drop(int dtype, long long rows, int d, const void* x, const void* res,
                             const float* gamma, const float* mean, const float* rstd, const void* dy,
                             void* dx, float* dgamma, float* dbeta, float drop_p,
                             unsigned long long drop_seed, const long long* drop_seed_dev, void* dz,
                             fpnmt_stream_t stream);

/* ---- one-key cross-attention sublayer (DecoderLayer, transformer.py:226-233)
 * With ONE unmasked encoder key the softmax weight is exactly 1: the
 * attention output is v[b] for each of an image's t query rows, and the
 * sublayer's Dense output row is c[b] + cbias, c[b] = v[b] W_o (fp32, the
 * unrounded GEMM accumulator). `out2 = LN(out1 + dropout(dense))` then needs
 * no (rows, d) Dense output in memory: the LayerNorm synthesises its x operand
 *   x[r, col] = T(keep(r*d + col) ? (c[r / t, col] + cbias[col]) / (1 - p) : 0)
 * with keep / key of fpnmt_gemm's dropout epilogue (the value that GEMM
 * would have stored from the same accumulator), rows = b*t, c (rows / t, d)
 * fp32, cbias optional. Row striding, the T(x + res) rounding, mean / rstd and
 * y are fpnmt_layernorm_fwd's on the materialised x, bit for bit. x_out
 * (optional, rows x d): the synthesised x is also stored, for a backward that
 * reads it (fpnmt_layernorm_bwd / _bwd_drop) instead of recomputing it.
 * bcast_bwd: fpnmt_layernorm_bwd_drop on that x: dx (now the only gradient of
 * res), dgamma / dbeta partials in the same layout and order, and
 * dz = keep ? dx / (1 - p) : 0 (dz may be NULL when drop_p == 0: dz == dx).  */
int fpnmt_layernorm_bcast_fwd(int dtype, long long rows, int d, int t, float eps, const float* c,
                              const float* cbias, float drop_p, unsigned long long drop_seed,
                              const long long* drop_seed_dev, const void* res, const float* gamma,
                              const float* beta, void* y, float* mean, float* rstd, void* x_out,
                              fpnmt_stream_t stream);
int fpnmt_layernorm_bcast_bwd(int dtype, long long rows, int d, int t, const float* c, const float* cbias,
                              float drop_p, unsigned long long drop_seed, const long long* drop_seed_dev,
                              const void* res, const float* gamma, const float* mean, const float* rstd,
                              const void* dy, void* dx, float* dgamma, float* dbeta, void* dz,
                              fpnmt_stream_t stream);
/* The gradients of c for n layers in one launch: dc[l][i, col] = sum over the
 * t rows of image i of dz[l][i*t + j, col], fp32, ascending j, no atomics
 * (deterministic). dz: n host pointers to (b*t, d) tensors of the dtype
 * (n <= FPNMT_MAX_ROWSUM_GROUPS); dc (n, b, d) fp32; dc_lp (optional): the
 * same sums rounded to the dtype (a GEMM operand). zero (optional): the launch
 * also stores zeros of the dtype to n (b, d) blocks, element (l, i, col) at
 * zero + l*zero_so + i*zero_ld + col (elements): the gradient of the key
 * projections, which one-key attention does not depend on, written into the
 * grouped projection's gradient buffer beside dv with no fill launch.       */
#define FPNMT_MAX_ROWSUM_GROUPS 16
int fpnmt_rowsum_groups(int dtype, int n, int b, int t, int d, const void* const* dz, float* dc, void* dc_lp,
                        void* zero, long long zero_ld, long long zero_so, fpnmt_stream_t stream);

/* ---- decoder embedding + positional encoding ---------------------------
 * y[b,t,:] = E[tok[b,t],:] + pe[t,:]   (no sqrt(d) scale, transformer.py:326-329)
 * bwd: dE[tok] += dy rows, each id's rows summed in position order (no
 * atomics: deterministic); sumsq += sum of squared row grads (TF
 * IndexedSlices norm for clip_by_norm, duplicates counted), in fixed order.
 * Uses the fpnmt workspace (fpnmt_set_workspace) as scratch.             */
int fpnmt_embed_posenc_fwd(int dtype, int b, int t, int d, const int32_t* tok, const float* emb,
                           const float* pe, void* y, fpnmt_stream_t stream);
int fpnmt_embed_posenc_bwd(int dtype, int b, int t, int d, const int32_t* tok, const void* dy,
                           float* d_emb, float* sumsq, fpnmt_stream_t stream);
/* The same with the decoder's Dropout after the embedding (transformer.py:
 * 331) fused: y = dropout(E[tok] + pe) with fpnmt_dropout(seed)'s mask on
 * the (b*t, d) output; the backward applies that mask to dy first.        */
int fpnmt_embed_posenc_fwd_drop(int dtype, int b, int t, int d, const int32_t* tok, const float* emb,
                                const float* pe, void* y, float drop_p, unsigned long long seed,
                                const long long* seed_dev, fpnmt_stream_t stream);
int fpnmt_embed_posenc_bwd_drop(int dtype, int b, int t, int d, const int32_t* tok, const void* dy,
                                float* d_emb, float* sumsq, float drop_p, unsigned long long seed,
                                const long long* seed_dev, fpnmt_stream_t stream);

/* ---- train-step targets (utils/pipeline.py:66-69, transformer.py:42-67)
 * From padded captions tok (b, t_full) of int64 (tok_bytes 8) or int32 (4)
 * ids, row stride ld_tok elements, in one launch: tar_inp = tok[:, :-1] and
 * tar_real = tok[:, 1:] (int32, (b, t_full-1)) and the decoder mask (b, 1,
 * t, t) fp32 = max(padding mask of tar_inp, look-ahead mask): 1 where
 * tar_inp[b, j] == 0 or j > i.                                             */
int fpnmt_decoder_targets(int b, int t_full, const void* tok, int tok_bytes, long long ld_tok, int32_t* tar_inp,
                          int32_t* tar_real, float* mask, fpnmt_stream_t stream);

/* ---- masked sparse cross-entropy (utils/pipeline.py:50-57) -------------
 * loss = mean over ALL rows of ce(row) * (label != 0); writes loss (fp32
 * scalar, overwritten) and dlogits = d loss / d logits * dloss_scale.     */
int fpnmt_xent_fwd_bwd(int dtype, long long rows, int v, const float* logits, long long ld,
                       const int32_t* labels, float* loss, void* dlogits, long long ldd,
                       float dloss_scale, fpnmt_stream_t stream);

/* ---- advantage-weighted masked cross-entropy (self-critical training) ---
 * The loss of a step whose caption rows carry a weight each (a sampled
 * caption's advantage): row r weighs w[r / w_div] (device memory, read at
 * execution: a replayed graph sees new weights once they are copied in;
 * w_div = the rows per caption), mask_r = (labels[r] != 0);
 *   loss         = (1 / rows) * sum_r w[r / w_div] * mask_r * ce_r
 *                  (a mean over ALL rows, fpnmt_xent_fwd_bwd's convention;
 *                  scalar, overwritten; summed in row order through the
 *                  workspace: bitwise repeatable),
 *   dlogits[r,j] = dloss_scale * w[r / w_div] * mask_r / rows * (softmax_j - [j == label_r])
 *                  (may be NULL: loss and row_logp only; exact zeros for a
 *                  pad row and for a zero weight),
 *   row_logp[r]  = logits[r, label_r] - logsumexp(logits[r, :]), 0 for a pad
 *                  row (may be NULL): the log-probability the decode paths sum.
 * Weights may be negative or zero. A label outside [0, v) is never
 * dereferenced and counts as a pad. Each row is read once (16-B loads where
 * the row starts are 16-B aligned, i.e. ld % 4 == 0 on an aligned base) and
 * held in registers up to v = 10 240; wider rows are read twice.
 * FPNMT_E_ARG: a null pointer (but row_logp / dlogits), w_div < 1,
 * rows % w_div != 0, ld < v, no workspace attached.                       */
int fpnmt_xent_weighted_fwd_bwd(int dtype, long long rows, int v, const float* logits, long long ld,
                                const int32_t* labels, const float* w, int w_div, float* loss, float* row_logp,
                                void* dlogits, long long ldd, float dloss_scale, fpnmt_stream_t stream);

/* ---- n caption rows per image: y[i * n + s, :] = x[i, :] for s < n -------
 * x (b, len), y (b * n, len), len elements of dtype per image (the encoder
 * output's S * d): the encoder runs once per image and the decoder on b * n
 * rows. 16-B copies when len * sizeof(dtype) and both pointers allow. The
 * backward, dx[i] = sum_s dy[i * n + s] in fp32 in ascending s, rounded once,
 * is fpnmt_rowsum_groups(dtype, 1, b, n, len, {dy}, dx_f32, dx, ...).        */
int fpnmt_repeat_rows(int dtype, int b, int n, long long len, const void* x, void* y, fpnmt_stream_t stream);

/* ---- label-smoothed masked cross-entropy, gradient optional ---------------
 * The masked CE against the target (1 - eps) * onehot + eps / v (Keras
 * CategoricalCrossentropy(label_smoothing=eps)), mask_r = label_r in (0, v),
 * lse_r = logsumexp(logits[r, :]):
 *   ce_r         = lse_r - (1 - eps) * logits[r, label_r] - (eps / v) * sum_j logits[r, j]
 *   loss         = (1 / rows) * sum_r mask_r * ce_r   (a mean over ALL rows;
 *                  scalar, overwritten; summed in row order through the
 *                  workspace: bitwise repeatable),
 *   dlogits[r,j] = dloss_scale * mask_r / rows * (softmax_j - (1 - eps) [j == label_r] - eps / v)
 *                  (dtype bf16 or fp32; may be NULL: the evaluation form, the
 *                  row is then read once at every width; exact zeros on a pad),
 *   row_logp[r]  = logits[r, label_r] - lse_r, the UNSMOOTHED log-probability,
 *                  0 on a pad (may be NULL),
 *   row_hit[r]   = 1 when the lowest-index arg-max of the row is label_r, else
 *                  0; 0 on a pad (may be NULL). Float comparisons only: exact.
 * fp32 logits; a pad label is never dereferenced. Each row is read once and
 * held in registers up to v = 10 240 (wider rows with a gradient: twice).
 * No allocation, no synchronisation, capturable.
 * FPNMT_E_ARG: eps outside [0, 1) or NaN, null loss / logits / labels, a bad
 * dtype, v < 1, ld < v, ldd < v with a gradient, rows outside [0, 2^31), no
 * workspace attached.                                                        */
int fpnmt_xent_smooth_fwd_bwd(int dtype, long long rows, int v, const float* logits, long long ld,
                              const int32_t* labels, float eps, float* loss, float* row_logp, int32_t* row_hit,
                              void* dlogits, long long ldd, float dloss_scale, fpnmt_stream_t stream);

/* ---- token-level knowledge distillation: CE mixed with KL to a teacher row --
 * The label-smoothed masked CE above mixed with the KL divergence from a
 * dense teacher row at temperature T (Hinton et al. 2015; word-level
 * distillation, Kim & Rush 2016). teacher holds fp32 logits in the sense that
 * the kernel normalises them: raw logits, log-probabilities or the fold
 * fpnmt_logits_ensemble writes all do. With a = desc->alpha, T =
 * desc->temperature, mask_r = label_r in (0, v), p = softmax(x), pT =
 * softmax(x / T), q = softmax(t / T) per row:
 *   ce_r         = lse(x) - (1 - eps) x_lab - (eps / v) sum_j x_j   (as fpnmt_xent_smooth_fwd_bwd)
 *   kl_r         = sum_j q_j (log q_j - log pT_j)
 *   loss[0]      = (1 / rows) sum_r mask_r ((1 - a) ce_r + a T^2 kl_r)
 *   loss[1]      = (1 / rows) sum_r mask_r ce_r        (without the 1 - a)
 *   loss[2]      = (1 / rows) sum_r mask_r kl_r        (without the a T^2)
 *                  (means over ALL rows; each summed in row order by one block
 *                  through the workspace: bitwise repeatable),
 *   dlogits[r,j] = dloss_scale * mask_r / rows * ((1 - a) (p_j - (1 - eps) [j == label_r] - eps / v)
 *                                                 + a T (pT_j - q_j))
 *                  (dtype bf16 or fp32; may be NULL; exact zeros on a pad row
 *                  and for dloss_scale == 0),
 *   row_logp[r]  = x_lab - lse(x), 0 on a pad (may be NULL).
 * desc is DEVICE memory, read by the kernel at execution: a captured step
 * changes alpha or T by writing the 16 bytes, without recapture. The entry
 * point cannot validate them (callers keep alpha in [0, 1], T finite > 0).
 * A pad row reads neither logits nor teacher. A -inf teacher entry is a token
 * of probability zero: it adds exactly 0 to kl_r and its gradient is
 * a T pT_j. A teacher row with a NaN or +inf, or -inf throughout, makes kl_r,
 * loss[0] and loss[2] NaN (and that row's gradient); nothing faults and the
 * other rows' gradients are unaffected. Both rows are read once and held in
 * registers up to v = 10 240; wider rows take an online pass and a second
 * read. Nothing is touched past column v - 1 of a row.
 * rows == 0 zeroes loss[0..2]. No allocation, no synchronisation, capturable.
 * FPNMT_E_ARG: null logits / teacher / labels / desc / loss, eps outside
 * [0, 1) or NaN, a bad dtype, v < 1, ld < v, ldt < v, ldd < v with a gradient,
 * rows outside [0, 2^31), no workspace attached.                            */
typedef struct fpnmt_distill_desc {
  float alpha;       /* weight of the KL term, in [0, 1] */
  float temperature; /* T, finite and > 0 */
  float reserved[2]; /* 0 */
} fpnmt_distill_desc;
int fpnmt_xent_distill_fwd_bwd(int dtype, long long rows, int v, const float* logits, long long ld,
                               const float* teacher, long long ldt, const int32_t* labels, float eps,
                               const fpnmt_distill_desc* desc /* device */, float* loss /* [3] */, float* row_logp,
                               void* dlogits, long long ldd, float dloss_scale, fpnmt_stream_t stream);

/* ---- per-caption and total statistics of a teacher-forced batch -----------
 * Rows are captions * t, caption-major; a position is live when its label is
 * > 0. Per caption: cap_logp = the sum of row_logp over its live positions
 * (ascending, fp64, rounded once to fp32), cap_len = their number, cap_hit =
 * the sum of row_hit over them (each may be NULL). totals[0..2] = the sums of
 * log-probability, tokens and hits over all captions as fp64, added in caption
 * order by one block; accumulate == 0 overwrites them, non-zero adds to what
 * they hold (a validation loop's running sums, no framework add).
 * FPNMT_E_ARG: null labels / row_logp / row_hit / totals, t < 1, captions < 0,
 * captions * t >= 2^31.                                                      */
int fpnmt_caption_stats(long long captions, int t, const int32_t* labels, const float* row_logp,
                        const int32_t* row_hit, float* cap_logp, int32_t* cap_len, int32_t* cap_hit, double* totals,
                        int accumulate, fpnmt_stream_t stream);

/* ---- optimizer: Keras Adam(amsgrad) + per-tensor clip_by_norm ----------
 * Tensors are segments [off[i], off[i+1]) of flat fp32 arrays, processed in
 * blocks of block_elems that never cross a segment: block b covers
 * [blk_start[b], min(blk_start[b]+block_elems, off[blk_seg[b]+1])).
 * seg_flags[i]: bit0 = sumsq[i] is supplied by the caller (TF IndexedSlices
 * norm of the embedding, fpnmt_embed_posenc_bwd), bit1 = apply the Keras
 * sparse-path update formula (m*b1 + (1-b1)g) instead of the fused dense
 * kernel's (m += (g-m)(1-b1)).
 * fpnmt_grad_sumsq writes blk_part[b] = sum(g^2) over block b (scaled
 * gradient g*grad_scale) for segments without bit0; fpnmt_amsgrad_step sums
 * segment i's partials blk_part[seg_blk0[i] .. seg_blk0[i+1]) in block order
 * (deterministic: no atomics), or takes sumsq[i] for bit0 segments. With
 * clipnorm <= 0 no norm is read (blk_part / seg_blk0 may be null).
 * step: device int64 = Keras `iterations` (0-based), incremented on device.
 * lr = d_model^-0.5 * min(rsqrt(step)/max((step-warm)*mult/(2*warm),1), step*warm_pow)
 * with warm_pow = warm^-1.5 (CustomSchedule, utils/utils.py:45-50); when
 * sched_d_model <= 0 the constant const_lr is used.                       */
int fpnmt_grad_sumsq(int nblocks, const int32_t* blk_seg, const long long* blk_start,
                     int block_elems, const long long* off, const int32_t* seg_flags,
                     const float* g, float grad_scale, float* blk_part, fpnmt_stream_t stream);
typedef struct fpnmt_adam_desc {
  float beta1, beta2, eps, clipnorm;
  float sched_d_model, sched_warmup, sched_mult, sched_warm_pow;
  float const_lr;
  float grad_scale; /* gradients are used as g*grad_scale (1/world after a SUM all-reduce);
                       caller-supplied (bit0) sumsq entries are scaled by grad_scale^2 */
} fpnmt_adam_desc;
int fpnmt_amsgrad_step(const fpnmt_adam_desc* d, int nblocks, const int32_t* blk_seg,
                       const long long* blk_start, int block_elems, const long long* off,
                       const int32_t* seg_flags, float* param, const float* grad, float* m,
                       float* v, float* vhat, const float* sumsq, const float* blk_part,
                       const int32_t* seg_blk0, long long* step, fpnmt_stream_t stream);
/* fpnmt_amsgrad_step_prep: the same step, and for every segment whose
 * preps[seg].ohwi is non-null (a conv / dense kernel in HWIO (r,s,c,k) order,
 * k a power of two <= block_elems dividing it) the bf16 compute copies of
 * the updated weights are written from the same pass, as
 * fpnmt_weight_prep(dtype FPNMT_BF16) would write them from the new masters:
 * ohwi[k][r][s][c] and flip[c*ld_flip + ((r-1-i)*s + (s-1-j))*k + kk], both
 * scaled by scale[kk] when scale is non-null. preps may be null (plain step).
 * Replaces the separate refresh pass after apply_gradients (utils/pipeline.py:78). */
typedef struct fpnmt_seg_prep {
  void* ohwi;
  void* flip;
  const float* scale;
  int r, s, c, k;
  long long ld_flip; /* 0 = r*s*k */
  uint32_t c_magic, c_shift; /* c as a fast divisor: q / c = (hi32(q*magic) + q) >> shift */
} fpnmt_seg_prep;
int fpnmt_amsgrad_step_prep(const fpnmt_adam_desc* d, int nblocks, const int32_t* blk_seg,
                            const long long* blk_start, int block_elems, const long long* off,
                            const int32_t* seg_flags, float* param, const float* grad, float* m,
                            float* v, float* vhat, const float* sumsq, const float* blk_part,
                            const int32_t* seg_blk0, long long* step, const fpnmt_seg_prep* preps,
                            fpnmt_stream_t stream);
/* Block-range forms: the blocks [blk_first, blk_first + nblocks) of the same
 * tables (all other pointers as above: blk_seg / blk_start / blk_part /
 * seg_blk0 index the WHOLE arena's blocks), for a step whose segments are
 * updated in parts, e.g. the transformer's while the feature extractor's
 * backward still runs. The range must hold whole segments. inc_step = 0
 * leaves `step` as it is (every part of one step must read the same value;
 * the last part increments it). max_grid > 0: at most that many workgroups,
 * each striding over the range (a small footprint beside other work); 0:
 * one workgroup per block. Results do not depend on max_grid.            */
int fpnmt_grad_sumsq_part(int blk_first, int nblocks, int max_grid, const int32_t* blk_seg,
                          const long long* blk_start, int block_elems, const long long* off,
                          const int32_t* seg_flags, const float* g, float grad_scale, float* blk_part,
                          fpnmt_stream_t stream);
int fpnmt_amsgrad_step_part(const fpnmt_adam_desc* d, int blk_first, int nblocks, int inc_step, int max_grid,
                            const int32_t* blk_seg, const long long* blk_start, int block_elems,
                            const long long* off, const int32_t* seg_flags, float* param,
                            const float* grad, float* m, float* v, float* vhat, const float* sumsq,
                            const float* blk_part, const int32_t* seg_blk0, long long* step,
                            const fpnmt_seg_prep* preps, fpnmt_stream_t stream);
/* Parameter groups: the block-range forms with a per-segment device table
 * groups[i] (one 16-B entry per segment, read once per block like preps[i];
 * no per-element load is added). For a segment that is not frozen, per
 * element in fp32, with lr, alpha, m, v, vhat as in the plain step,
 * s = lr_scale, w = weight_decay:
 *   p_new = (p - (m_new * (alpha * s)) / (sqrtf(vhat_new) + eps)) - (lr * s * w) * p
 * (decoupled, AdamW-style decay on the old p; the term is not evaluated at
 * w == 0, and s == 1, w == 0 gives fpnmt_amsgrad_step_part's result bit for
 * bit). s == 0 is legal: m, v, vhat advance and p only decays. Clipping stays
 * per tensor and comes first; seg_flags keep their meaning.
 * frozen != 0: the segment's blocks return before any load: its grad is
 * never read, its param, m, v, vhat, norm partials and compute copies
 * (preps) are never written. A caller that knows frozen segments at the head
 * or tail of a range should not launch their blocks at all. The table is
 * read at execution time: values written into it (stream-ordered) between
 * two replays of a captured launch take effect at the next replay.
 * FPNMT_E_ARG: groups null, otherwise as fpnmt_amsgrad_step_part.          */
typedef struct fpnmt_seg_group {
  float lr_scale;
  float weight_decay;
  int32_t frozen;
  int32_t reserved;
} fpnmt_seg_group;
int fpnmt_grad_sumsq_groups(int blk_first, int nblocks, int max_grid, const int32_t* blk_seg,
                            const long long* blk_start, int block_elems, const long long* off,
                            const int32_t* seg_flags, const fpnmt_seg_group* groups, const float* g,
                            float grad_scale, float* blk_part, fpnmt_stream_t stream);
int fpnmt_amsgrad_step_groups(const fpnmt_adam_desc* d, int blk_first, int nblocks, int inc_step, int max_grid,
                              const int32_t* blk_seg, const long long* blk_start, int block_elems,
                              const long long* off, const int32_t* seg_flags, float* param,
                              const float* grad, float* m, float* v, float* vhat, const float* sumsq,
                              const float* blk_part, const int32_t* seg_blk0, long long* step,
                              const fpnmt_seg_prep* preps, const fpnmt_seg_group* groups,
                              fpnmt_stream_t stream);
/* Weight averaging: fpnmt_amsgrad_step_groups with a shadow array `ema` (fp32,
 * the arena's layout) that follows the parameters inside the same kernel, in
 * the manner of tf.train.ExponentialMovingAverage. Per element of a segment
 * that is not frozen, after p has its new value:
 *   e = fmaf(omd_t, p_new - e, e)
 *   omd_t = debias ? fmaxf(one_minus_decay, 9 / (10 + t)) : one_minus_decay
 * with t = iterations + 1: TF's decay_t = min(decay, (1 + t) / (10 + t)),
 * written on 1 - decay so that nothing cancels. param, m, v, vhat and the
 * compute copies are bit for bit those of the step without `ema`; e is one
 * more streamed fp32 array (8 B per element per step), no launch is added.
 * ema_desc is device-resident, 16 B, read once per block at execution time:
 * values written into it (stream-ordered) between two replays of a captured
 * launch take effect at the next replay. one_minus_decay is 1 - decay
 * computed in double and rounded once. A frozen segment's e is neither read
 * nor written; alignment gaps of `ema` are never touched. groups and preps
 * may each be null (the plain step / no fused refresh).
 * FPNMT_E_ARG: ema or ema_desc null, ema aliasing param / grad / m / v /
 * vhat, otherwise as fpnmt_amsgrad_step_part.                                */
typedef struct fpnmt_ema_desc {
  float one_minus_decay;
  int32_t debias;
  int32_t reserved[2];
} fpnmt_ema_desc;
int fpnmt_amsgrad_step_ema(const fpnmt_adam_desc* d, int blk_first, int nblocks, int inc_step, int max_grid,
                           const int32_t* blk_seg, const long long* blk_start, int block_elems,
                           const long long* off, const int32_t* seg_flags, float* param,
                           const float* grad, float* m, float* v, float* vhat, const float* sumsq,
                           const float* blk_part, const int32_t* seg_blk0, long long* step,
                           const fpnmt_seg_prep* preps, const fpnmt_seg_group* groups, float* ema,
                           const fpnmt_ema_desc* ema_desc, fpnmt_stream_t stream);
/* Global-norm clipping and the non-finite step guard. Two device-resident
 * records, both read or written at execution time only (values written
 * stream-ordered between two replays of a captured launch take effect at the
 * next replay):
 *   fpnmt_guard_desc   16 B, written by the host. global_clipnorm > 0: every
 *                      gradient is scaled by clip / max(||g||, clip) with
 *                      ||g|| the norm over ALL trainable tensors (Keras
 *                      global_clipnorm, tf.clip_by_global_norm); 0: no global
 *                      clip, only the guard.
 *   fpnmt_guard_state  32 B, written by the device (zero it once).
 * fpnmt_grad_norm_total: one workgroup of 256 threads, launched after
 * fpnmt_grad_sumsq_* of the same step over the whole arena (nblocks = all of
 * its blocks). It sums, in a fixed order without atomics, for every segment
 * that is not frozen (groups may be null: none is) its blocks' blk_part
 * entries, or for a bit0 segment sumsq[seg] * grad_scale^2 once: exactly the
 * ||g||^2 the per-tensor clip uses for that segment. Partials of frozen and
 * of bit0 blocks, which fpnmt_grad_sumsq_* never writes, are not read. It
 * writes
 *   sumsq_total
 *   skipped     = !isfinite(sumsq_total)
 *   clip_factor = global_clipnorm > 0 ? clip / max(sqrtf(total), clip) : 1,
 *                 computed once (0 on a skipped step)
 * and leaves the counters alone. A FINITE gradient whose squares overflow
 * fp32 (sumsq_total = +Inf) counts as non-finite: its norm cannot be
 * represented, so the step is skipped.
 * fpnmt_amsgrad_step_guard: fpnmt_amsgrad_step_ema's arguments plus the two
 * records; groups, preps and ema / ema_desc (both or neither) may be null.
 * Per block, after the frozen check, one uniform 32-B load of the state:
 *   skipped != 0   the block returns before any load of param, grad, m, v,
 *                  vhat, ema, the prep table or the norms; nothing is
 *                  written, compute copies included.
 *   otherwise      the existing step. With d->clipnorm <= 0 the gradient is
 *                  g = grad * grad_scale * clip_factor (clip_factor is 1.0
 *                  without a global clip, and x * 1.0f is x: every output is
 *                  bit for bit the unguarded entry point's); with
 *                  d->clipnorm > 0 the per-tensor clip runs as before.
 * inc_step != 0 launches a guarded increment: on an applied step
 * iterations += 1, n_applied += 1, consecutive = 0; on a skipped one
 * n_skipped += 1, consecutive += 1 and `iterations` stays, so the step after
 * a skipped one sees the counter (and the dropout keys derived from it) the
 * skipped one saw.
 * The block range and max_grid keep their meaning (frozen heads and tails are
 * still trimmed), but the launched range MUST contain every block that is
 * not frozen, and the step must be one launch with inc_step != 0: the total
 * covers the whole arena, and a step updated in parts cannot be undone.
 * FPNMT_E_ARG: a null record; ema without ema_desc or the reverse; ema
 * aliasing another array; d->clipnorm > 0 together with global_clipnorm > 0
 * (Keras makes the two exclusive as well). The last check reads the 16-B
 * descriptor back (one stream synchronisation) and is made only when
 * d->clipnorm > 0 and the stream is not capturing; in a captured launch the
 * caller keeps the two exclusive, and the per-tensor clip takes precedence.
 * Otherwise as fpnmt_amsgrad_step_part.                                     */
typedef struct fpnmt_guard_desc {
  float global_clipnorm;
  int32_t reserved[3];
} fpnmt_guard_desc;
typedef struct fpnmt_guard_state {
  float sumsq_total;   /* ||g||^2 of the last step, all trainable tensors */
  float clip_factor;
  int32_t skipped;     /* this step */
  int32_t consecutive; /* skipped steps in a row, 0 after an applied one */
  long long n_skipped;
  long long n_applied;
} fpnmt_guard_state;
int fpnmt_grad_norm_total(int nblocks, const int32_t* blk_seg, const int32_t* seg_flags,
                          const fpnmt_seg_group* groups, const float* sumsq, const float* blk_part,
                          const int32_t* seg_blk0, float grad_scale, const fpnmt_guard_desc* guard_desc,
                          fpnmt_guard_state* guard_state, fpnmt_stream_t stream);
int fpnmt_amsgrad_step_guard(const fpnmt_adam_desc* d, int blk_first, int nblocks, int inc_step, int max_grid,
                             const int32_t* blk_seg, const long long* blk_start, int block_elems,
                             const long long* off, const int32_t* seg_flags, float* param,
                             const float* grad, float* m, float* v, float* vhat, const float* sumsq,
                             const float* blk_part, const int32_t* seg_blk0, long long* step,
                             const fpnmt_seg_prep* preps, const fpnmt_seg_group* groups, float* ema,
                             const fpnmt_ema_desc* ema_desc, const fpnmt_guard_desc* guard_desc,
                             fpnmt_guard_state* guard_state, fpnmt_stream_t stream);
/* a[i] <-> b[i] for i < n, in place (the averaged weights under the model and
 * back without moving a pointer; two swaps are the identity). float4 body
 * when both pointers are 16-B aligned, scalar otherwise and for the last
 * n % 4 elements. n == 0 is a no-op. FPNMT_E_ARG: n < 0, a null pointer with
 * n > 0, overlapping buffers.                                                */
int fpnmt_swap_f32(float* a, float* b, long long n, fpnmt_stream_t stream);

/* ---- batched beam decode (BASELINE C5; utils/pipeline.py:82-154) --------
 * fpnmt_decode_attention: softmax(q k^T * scale) v for ONE query position per
 * row (the last position of the reference's full-prefix recompute; its
 * look-ahead mask row keeps every position <= t). Row r, head h:
 *   q at q + r*ldq + h*depth; key / value of position j at
 *   kv + R*row_stride + j*pos_stride + {k_off | v_off} + h*depth, where
 *   R = src ? src[r*src_ld + j] : r / row_div
 * (src: the beam's cache-row table, so beams share history without copies;
 * row_div: rows per encoder output for the cross-attention). heads <= 8,
 * depth <= 64. out at out + r*ldo + h*depth. Attention weights are not
 * materialised on this path.
 * fpnmt_beam_step: per image (beam_n consecutive rows): p = softmax(logits
 * row), candidates p * beam_prob over beam_n x vocab, top beam_n in
 * tf.math.top_k order (value desc, lower flat index first); new beams take
 * parent = flat / vocab, token = flat % vocab:
 *   hist_out[r][0..t] = hist_in[parent][0..t], hist_out[r][t+1] = token,
 *   src_out[r][0..t] = src_in[parent][0..t], src_out[r][t+1] = r,
 *   tok_out[r] = token, beam_prob[r] = candidate value.
 * While status[img] == 0 the best beam (first argmax of the new
 * probabilities) is copied to result[img] (tokens after <start>, without a
 * final <end>), result_len[img] set, and status[img] = 1 once it ends.     */
int fpnmt_decode_attention(int dtype, int rows, int heads, int depth, int lk, float scale, const void* q,
                           long long ldq, const void* kv, long long row_stride, long long pos_stride,
                           long long k_off, long long v_off, const int32_t* src, int src_ld, int row_div,
                           void* out, long long ldo, fpnmt_stream_t stream);
int fpnmt_beam_step(int n_images, int beam_n, int vocab, const float* logits, long long ldl, float* beam_prob,
                    const int32_t* hist_in, int32_t* hist_out, int hist_ld, int t, const int32_t* src_in,
                    int32_t* src_out, int src_ld, int end_token, int32_t* tok_out, int32_t* result, int result_ld,
                    int32_t* result_len, int32_t* status, fpnmt_stream_t stream);
/* Beam search proper (not in the reference, whose beams start identical and
 * stay so). State per row: beam_score (fp32 sum of log-probabilities),
 * beam_len (tokens after <start>, a final <end> counted), beam_fin (0 / 1);
 * hist / src / tok_out / t as in fpnmt_beam_step. The caller starts step 0
 * with score 0 on each image's first beam and -inf on the others.
 * fpnmt_beam_step_log: candidates over beam_n x vocab at flat = b*vocab + j:
 *   live beam b:     beam_score[b] + log_softmax(logits row b)[j];
 *   finished beam b: one candidate, beam_score[b] at j = end_token;
 *   beam at -inf:    none.
 * Top beam_n in the order of fpnmt_beam_step (value desc, lower flat index
 * first), parent = flat / vocab, token = flat % vocab; hist_out / src_out /
 * tok_out as there (src_out[r][t+1] = r); beam_score[r] = candidate value; the
 * child of a finished parent keeps beam_fin = 1 and its beam_len, a live
 * child gets beam_len = t + 1, beam_fin = (token == end_token).
 * status[img] = 1 once all beam_n beams have finished; an image entered with
 * status 1 is frozen: its rows are carried to hist_out / src_out unchanged
 * (position t+1: end_token / r) and nothing else of it is read or written.
 * Requires beam_n <= 16, vocab >= beam_n, 0 <= end_token < vocab,
 * hist_ld >= t + 2, src_ld >= t + 1.
 * fpnmt_beam_finalize: per image the beams ranked by
 * beam_score / max(beam_len, 1)^alpha (desc, ties to the lower beam; alpha 0:
 * the raw sum) -> nbest_tok (n_images, beam_n, tok_ld) tokens after <start>
 * without a final <end>, zero-padded; nbest_len, nbest_score (the ranking
 * value) (n_images, beam_n), best first.                                    */
int fpnmt_beam_step_log(int n_images, int beam_n, int vocab, const float* logits, long long ldl, float* beam_score,
                        int32_t* beam_len, int32_t* beam_fin, const int32_t* hist_in, int32_t* hist_out,
                        int hist_ld, int t, const int32_t* src_in, int32_t* src_out, int src_ld, int end_token,
                        int32_t* tok_out, int32_t* status, fpnmt_stream_t stream);
int fpnmt_beam_finalize(int n_images, int beam_n, const int32_t* hist, int hist_ld, const float* beam_score,
                        const int32_t* beam_len, const int32_t* beam_fin, float alpha, int32_t* nbest_tok,
                        int tok_ld, int32_t* nbest_len, float* nbest_score, fpnmt_stream_t stream);
/* Diverse beam search (Vijayakumar et al.): fpnmt_beam_step_log's step with
 * the image's beam_n rows split into `groups` groups of Kg = beam_n / groups
 * contiguous rows (group g: rows g*Kg .. (g+1)*Kg - 1), ranked in group
 * order at every position. cnt[token] starts empty at every position.
 *   live row b of group g: token j is offered at
 *     (logits[b][j] + coff[b]) - diversity_penalty * cnt[j],
 *     coff[b] = beam_score[b] - logsumexp(logits row b); the product is an
 *     fp32 product, subtracted after the add;
 *   finished row b: one candidate, beam_score[b] at j = end_token, never
 *     penalised and never counted;  row at -inf: none.
 * Only the rows of group g compete; order and flat index (b*vocab + j, b the
 * row inside the image) as in fpnmt_beam_step_log. Group g takes its Kg best
 * into its own rows, best first, and every live child that took token j
 * (<end> included) adds 1 to cnt[j] for the groups after it.
 * A live child's beam_score is the UNPENALISED logits[b][j] + coff[b]: scores
 * stay sums of log-probabilities. beam_len / beam_fin / hist_out / src_out /
 * tok_out, the slot without a candidate and the frozen image are those of
 * fpnmt_beam_step_log; status[img] = 1 once all beam_n rows have finished.
 * The caller starts step 0 with score 0 on each GROUP's first row and -inf
 * on the others. groups == 1 writes what fpnmt_beam_step_log writes, byte
 * for byte, whatever the penalty; diversity_penalty == 0 writes what
 * fpnmt_beam_step_log(n_images * groups, Kg, ...) writes on the same buffers
 * (status apart). fpnmt_beam_finalize(n_images * groups, Kg, ...) ranks each
 * group on its own.
 * Requires what fpnmt_beam_step_log requires; FPNMT_E_ARG also for
 * groups < 1, beam_n % groups != 0, and a negative or non-finite penalty.  */
int fpnmt_beam_step_groups(int n_images, int beam_n, int groups, float diversity_penalty, int vocab,
                           const float* logits, long long ldl, float* beam_score, int32_t* beam_len,
                           int32_t* beam_fin, const int32_t* hist_in, int32_t* hist_out, int hist_ld, int t,
                           const int32_t* src_in, int32_t* src_out, int src_ld, int end_token, int32_t* tok_out,
                           int32_t* status, fpnmt_stream_t stream);

/* Sampled decoding (not in the reference): the last launch of a decode step
 * that draws one token per row from its fp32 logits. Rows are independent
 * (no re-ranking: no src tables, hist is updated in place). State per row:
 * score (fp32 sum of log-probabilities), slen (tokens after <start>, a final
 * <end> counted), fin (0 / 1).
 * fpnmt_sample_step, live row r (fin[r] == 0):
 *   weights  w_j = exp((l_j - max l) / temperature); a -inf logit weighs 0.
 *     Sums run on q_j = trunc(w_j * 2^40) as integers: exact in any order, so
 *     the kept set and the token are a function of the logits and u alone; a
 *     weight below 2^-40 of the maximum counts as 0.
 *   top_k > 0: keep the tokens whose logit is >= the top_k-th largest logit
 *     of the row (every token equal to that boundary is kept; -0 == +0);
 *     top_k == 0 or >= vocab: off.
 *   top_p < 1: of those, by weight descending, the shortest prefix whose
 *     weight is >= top_p * (their total weight), and every token whose logit
 *     equals the last kept one; top_p == 1: off. The maximum is always kept.
 *   draw     u = uniform01(key, ((uint64)r << 16) | t) (csrc/common.h), key =
 *     seed + (seed_dev ? *seed_dev * 0x9E3779B97F4A7C15 : 0) as for dropout:
 *     a replayed graph draws anew when the host changes the device word. The
 *     token is the smallest kept index whose prefix sum of kept weights, in
 *     index order, exceeds u * W (W the kept total); it always has w > 0.
 *   writes   tok_out[r] = hist[r][t+1] = token; score[r] += l_token -
 *     logsumexp(l) (temperature 1, unfiltered: the model's log-probability);
 *     slen[r] = t + 1; fin[r] = (token == end_token); kept_out[r] (may be
 *     NULL) = size of the kept set.
 * Finished row: logits not read; hist[r][t+1] = tok_out[r] = end_token,
 *   kept_out[r] = 0, score / slen / fin unchanged.
 * Row with no drawable token (a NaN or +inf logit, or all -inf): token
 *   end_token, fin = 1, score = -inf, slen = t + 1, kept_out = 0.
 * Requires temperature finite > 0, 0 < top_p <= 1, top_k >= 0, 0 <=
 * end_token < vocab <= ldl, 0 <= t < 65536, hist_ld >= t + 2; with a filter
 * on, vocab <= FPNMT_SAMPLE_FILTER_MAX_VOCAB (the row is staged in 64 KB of
 * LDS), else FPNMT_E_UNSUPPORTED.
 * fpnmt_sample_uniform: u_out[r] = the u row r would use at step t.         */
#define FPNMT_SAMPLE_FILTER_MAX_VOCAB 16384
int fpnmt_sample_step(int rows, int vocab, const float* logits, long long ldl, float temperature, int top_k,
                      float top_p, unsigned long long seed, const long long* seed_dev, float* score, int32_t* slen,
                      int32_t* fin, int32_t* hist, int hist_ld, int t, int end_token, int32_t* tok_out,
                      int32_t* kept_out /* may be NULL */, fpnmt_stream_t stream);
int fpnmt_sample_uniform(int rows, int t, unsigned long long seed, const long long* seed_dev, float* u_out,
                         fpnmt_stream_t stream);

/* Constrained decoding (not in the reference; csrc/constrain.hip): rewrites
 * the fp32 logits (rows, vocab) of a decode position in place, before
 * fpnmt_beam_step_log or fpnmt_sample_step, from the rows' token history on
 * the device. A ban is a -inf logit, which both step kernels define: weight 0
 * in the draw, exp(-inf - max) = 0 in the logsumexp and a -inf candidate. The
 * step's scores are therefore sums over the CONSTRAINED logits (beam: score +
 * log_softmax(constrained row); sample: l_token - logsumexp(constrained l)),
 * the log-probability under the constrained, renormalised distribution; in
 * sampled decoding the constraints come before temperature, top_k and top_p.
 * A row r with fin != NULL and fin[r] != 0 is neither read nor written. For
 * every other row, with h[0..t] = hist[r*hist_ld + 0..t] (h[0] is <start>;
 * the token being chosen is number t + 1) and l = logits + r*ldl, the final
 * value of l[j], 0 <= j < vocab, is
 *   -inf, if one of
 *     n-gram   g = no_repeat_ngram > 0 and an i in [0, t - g + 1] exists with
 *              h[i .. i+g-2] == h[t-g+2 .. t] and h[i+g-1] == j: the g - 1
 *              tokens before the one being chosen open an earlier complete
 *              g-gram that j would complete again (g == 1: every token of
 *              h[0..t]; g > t + 1: none);
 *     list     j is one of banned[0 .. n_banned);
 *     length   j == end_token and t < min_len (<end> now would give a caption
 *              of t tokens);
 *   else l[j] > 0 ? l[j] / p : l[j] * p (p = repetition_penalty, one IEEE fp32
 *     divide or multiply), if p != 1 and j occurs in h[0..t]: applied exactly
 *     once however often j occurs; a NaN keeps its bits, -inf stays -inf;
 *   else unchanged, bit for bit. Columns vocab .. ldl-1 are never written.
 * History or banned ids outside [0, vocab) are ignored: they match nothing
 * (not even each other) and no address is formed from them.
 * FPNMT_E_ARG: null logits / hist, rows <= 0, vocab <= 0, ldl < vocab, t < 0,
 * hist_ld < t + 1, no_repeat_ngram < 0, min_len < 0, repetition_penalty not
 * finite or <= 0, end_token outside [0, vocab), n_banned < 0, or n_banned > 0
 * with banned NULL. FPNMT_E_UNSUPPORTED: t + 1 > FPNMT_CONSTRAIN_MAX_LEN (the
 * history row is staged in LDS), n_banned > FPNMT_CONSTRAIN_MAX_BANNED. With
 * every rule off (no_repeat_ngram 0, repetition_penalty 1, min_len <= t,
 * n_banned 0) nothing is launched.                                          */
#define FPNMT_CONSTRAIN_MAX_LEN    1024   /* t + 1 positions staged per row */
#define FPNMT_CONSTRAIN_MAX_BANNED 4096
int fpnmt_logits_constrain(int rows, int vocab, float* logits, long long ldl, const int32_t* hist, int hist_ld, int t,
                           const int32_t* fin /* may be NULL */, int no_repeat_ngram, float repetition_penalty,
                           int min_len, int end_token, const int32_t* banned /* may be NULL */, int n_banned,
                           fpnmt_stream_t stream);

/* Ensemble decoding (not in the reference; csrc/ensemble.hip): folds the fp32
 * logits rows of n_models models into one fp32 row per decode row, in one
 * launch, before fpnmt_logits_constrain and the step kernels, which normalise
 * the row they are given themselves. logits, ldl and weight are HOST arrays
 * of n_models entries (logits[m] a device pointer to model m's (rows, vocab)
 * logits with leading dimension ldl[m]); they are copied into the launch
 * arguments, so a captured graph holds them and no device-side table has to
 * stay alive. The weights are used as given: the caller normalises them to
 * sum 1 (in fp64, before rounding to fp32); nothing is renormalised here.
 * A row r with fin != NULL and fin[r] != 0 is neither read nor written. For
 * every other row, with l_m = logits[m] + r*ldl[m], lse_m = logsumexp of
 * l_m[0 .. vocab) and w_m = weight[m], out[r*ldo + j], 0 <= j < vocab, is
 *   mode 0 "prob"     log(sum_m w_m * softmax(l_m)[j]), the arithmetic mean of
 *                     the models' distributions, computed as logsumexp_m(
 *                     l_m[j] + log w_m - lse_m) and never as a sum of exp of
 *                     raw logits: a normalised row (its logsumexp is 0);
 *   mode 1 "logprob"  sum_m w_m * (l_m[j] - lse_m), the geometric mean
 *                     (log-linear interpolation), left unnormalised: the step
 *                     kernels renormalise, as they do for constrained rows.
 * A -inf logit is a token its model gives probability 0: mode 0 leaves that
 * model out of the column (-inf only where every model has -inf), mode 1
 * gives -inf where any model has it; such a column is exactly -inf, never a
 * NaN from inf - inf or 0 * inf. A bad row, in which a model's row holds a
 * NaN or +inf or is -inf in all columns, has every output column NaN (what
 * fpnmt_sample_step defines as a row with no drawable token); nothing faults.
 * Columns vocab .. ldo-1 of out are never written and nothing is read past
 * column vocab-1 of an input row (ldl[m] may equal vocab). out may be
 * logits[0] itself (same pointer, ldo == ldl[0]); it may overlap no other
 * input and logits[0] in no other way. n_models == 1 gives l - lse at weight
 * 1 in both modes.
 * FPNMT_E_ARG: a null pointer (the arrays, an entry of logits, out), rows <=
 * 0, vocab <= 0, n_models < 1, an ldl[m] or ldo < vocab, a weight not finite
 * or <= 0, mode not 0 or 1, an out that overlaps an input other than as
 * above. FPNMT_E_UNSUPPORTED: n_models > FPNMT_ENSEMBLE_MAX.                */
#define FPNMT_ENSEMBLE_MAX 8
int fpnmt_logits_ensemble(int rows, int vocab, int n_models, const float* const* logits /* host array */,
                          const long long* ldl /* host array */, const float* weight /* host array */,
                          int mode /* 0 "prob", 1 "logprob" */, const int32_t* fin /* may be NULL */, float* out,
                          long long ldo, fpnmt_stream_t stream);

/* Device-side CIDEr-D reward (not in the reference; csrc/cider.hip): the
 * arithmetic of utils/cider_reward.py CiderDReward (n = 4, clipped counts,
 * Gaussian length penalty, x 10) on the sampler's device state, against
 * reference tables packed once on the host (fpnmt/cider_device.py). All
 * table pointers are device memory.
 *   key      a k-gram (k <= 4) as one uint64: sum_i (tok_i + 1) << (16 i);
 *            exact for 0 <= tok <= 65533.
 *   df_keys  [n_df] ascending, unique; df_idf[n_df] = log(N) - log(max(1,
 *            df)); a key absent from df_keys has idf idf_absent (= log N).
 *   img_off  [n_images + 1]: image i's references are j in [img_off[i],
 *            img_off[i + 1]); ref_off[R + 1]: reference j's entries are e in
 *            [ref_off[j], ref_off[j + 1]), ref_keys ascending inside;
 *            ref_w[e] = tf * idf; ref_norm[j][4] per order; ref_len[j] = the
 *            sum of its bigram counts.
 *   gauss    [n_gauss], gauss[d] the length factor at |len_h - len_r| = d
 *            (an index past the table reads its last entry).
 *   max_len  the longest candidate served, <= FPNMT_CIDER_MAX_LEN.
 * fpnmt_ciderd_reward: reward[r] (fp64), r < rows, = the CIDEr-D of the
 *   candidate hist[r][1 : 1 + slen[r] - fin[r]] (what the sampler drew,
 *   without <start> and a final <end>; the length is clamped to [0, hist_ld -
 *   1]) against the references of image img_index[r / n]. rows % n == 0. A
 *   candidate of length 0 scores exactly 0; an img_index outside [0,
 *   n_images) gives reward 0 with no table read. fp64, fixed-order sums, no
 *   atomics: bitwise repeatable, and a row's value does not depend on the
 *   other rows of the launch. hist_ld - 1 > max_len, or max_len >
 *   FPNMT_CIDER_MAX_LEN: FPNMT_E_UNSUPPORTED.
 * fpnmt_scst_pack: per image i < b, from reward[b * n] (fp64):
 *   adv[i * n + s] (fp32) = reward - baseline, computed in fp64 and rounded
 *     once; mode FPNMT_SCST_MEAN (n >= 2): the baseline of sample s is
 *     (sum over s' != s, ascending, of reward[i * n + s']) / (n - 1); mode
 *     FPNMT_SCST_GREEDY: greedy[i] (fp64[b]).
 *   tok[i * n + s][width] (int64) = fpnmt.scst.pack_tokens' row: start_token,
 *     the candidate's ids, end_token iff the candidate is shorter than
 *     max_tokens (the positions the sampler ran: iff the row finished), zeros;
 *     cut at width.
 *   scalars[0..2] (fp64) = the means over all b * n rows of reward, baseline
 *     and score (the sampler's fp32 log-probabilities), each summed by one
 *     wave in a fixed order (lane-strided partials, a shuffle tree).
 * Both: no allocation, no synchronisation, capturable.                     */
#define FPNMT_CIDER_MAX_LEN 128
#define FPNMT_SCST_MEAN 0
#define FPNMT_SCST_GREEDY 1
typedef struct fpnmt_cider_tables {
  const unsigned long long* df_keys;
  const double* df_idf;
  long long n_df;
  double idf_absent;
  const int32_t* img_off;
  int n_images;
  int max_len;
  const long long* ref_off;
  const unsigned long long* ref_keys;
  const double* ref_w;
  const double* ref_norm;
  const int32_t* ref_len;
  const double* gauss;
  int n_gauss;
} fpnmt_cider_tables;
int fpnmt_ciderd_reward(const fpnmt_cider_tables* t, int rows, int n, const int32_t* hist, int hist_ld,
                        const int32_t* slen, const int32_t* fin, const int32_t* img_index, double* reward,
                        fpnmt_stream_t stream);
int fpnmt_scst_pack(int b, int n, int mode, const double* reward, const double* greedy /* may be NULL (mean) */,
                    const int32_t* hist, int hist_ld, const int32_t* slen, const int32_t* fin, const float* score,
                    int start_token, int end_token, int max_tokens, long long* tok, int width, float* adv,
                    double* scalars, fpnmt_stream_t stream);

/* Consensus (minimum-Bayes-risk) caption selection under CIDEr-D (not in the
 * reference; csrc/consensus.hip): among the n candidates of an image, rows
 * img * n .. img * n + n - 1 of the sampler's or the beam search's device
 * state (candidate r = hist[r][1 : 1 + len[r] - fin[r]], clamped to
 * min(hist_ld - 1, max_len) tokens), the one that agrees most with the others.
 *   sim(h, r)  CiderDReward's score_one of h with r as the ONLY reference:
 *              tf * idf vectors with the corpus's idf, counts clipped as
 *              min(w_h, w_r) * w_r, each order divided by nh * nr where both
 *              are non-zero and multiplied by gauss[|len_h - len_r|] (lengths
 *              are bigram counts), the mean of the four orders, x 10. Not
 *              symmetric.
 *   util[r]    (fp64, rows = images * n) = sum over j != s of p_j sim(c_s,
 *              c_j) / sum over j != s of p_j for r = img * n + s, both sums
 *              over ascending j, 0 where the denominator is 0; p = weight
 *              (non-negative, per row) or 1 where weight is NULL. Self is
 *              excluded by index: a duplicate at another index counts. An
 *              empty caption has utility 0 and contributes 0; n = 1 gives 0.
 *   pick[img]  the index s < n of the greatest util, ties to the lowest.
 *   pair       NULL, or [images][n][n] fp64: pair[img][s][j] = sim(c_s, c_j),
 *              the diagonal included.
 * Of the tables only df_keys, df_idf, n_df, idf_absent, gauss, n_gauss and
 * max_len are read. One block per image keeps every candidate's keys and
 * weights in LDS: 16 n E + 64 E + 44 n bytes with E = L + (L - 1) + (L - 2) +
 * (L - 3) (the terms above zero) at L = min(hist_ld - 1, max_len) must not
 * exceed 160 KiB (n = 64 up to L = 38, n = 16 up to L = 128), else
 * FPNMT_E_UNSUPPORTED, as for n > FPNMT_CONSENSUS_MAX_CANDS, hist_ld - 1 >
 * max_len and max_len > FPNMT_CIDER_MAX_LEN. images == 0 returns 0 without a
 * launch. fp64, fixed-order sums, no atomics: bitwise repeatable, and an
 * image's outputs do not depend on the other images of the launch. No
 * allocation, no synchronisation, capturable.                              */
#define FPNMT_CONSENSUS_MAX_CANDS 64
int fpnmt_ciderd_consensus(const fpnmt_cider_tables* t, int images, int n, const int32_t* hist, int hist_ld,
                           const int32_t* len, const int32_t* fin, const double* weight /* rows, or NULL: uniform */,
                           double* util /* rows */, int32_t* pick /* images */,
                           double* pair /* images * n * n, or NULL */, fpnmt_stream_t stream);

/* ---- MobileNetV2 backbone (models/mobilenet.py:43-72 ->
 * keras MobileNetV2(alpha=1.0), models/retinanet.py:274) -------------------
 * BatchNormalization(epsilon, momentum) in training mode over the channels
 * of (rows, c) NHWC activations, c % 8 == 0:
 *   fpnmt_bn_stats: batch mean / biased variance (fp32) into mean, var;
 *     when moving_mean / moving_var are given they move toward the batch
 *     statistics: m = m*momentum + mean*(1-momentum), v likewise with the
 *     Bessel-corrected variance (Keras fused batch norm).
 *   fpnmt_bn_apply: y = act((x - mean) * rsqrt(var + eps) * gamma + beta)
 *     [+ residual]; act in {NONE, RELU, RELU6}. Inference passes the moving
 *     statistics as mean / var.
 *   fpnmt_bn_bwd: g = dy * act'(y); dbeta += sum g, dgamma += sum g*xhat;
 *     dx = gamma*rstd*(g - mean(g) - xhat*mean(g*xhat)) (training-mode BN).
 * DepthwiseConv2D (kh, kw <= 3, no bias), weights in the Keras (kh, kw, C, 1)
 * order = (kh, kw, C) fp32; 4 independent pads (TF / correct_pad):
 *   fwd y (n, ho, wo, c); bwd_data dx (n, h, w, c) overwritten;
 *   bwd_filter dw += sum over pixels.
 * Every reduction is per-block partials summed in a fixed order through the
 * fpnmt workspace (deterministic).                                         */
int fpnmt_bn_stats(int dtype, long long rows, int c, const void* x, float* mean, float* var,
                   float* moving_mean, float* moving_var, float momentum, fpnmt_stream_t stream);
int fpnmt_bn_apply(int dtype, long long rows, int c, const void* x, const float* mean, const float* var,
                   const float* gamma, const float* beta, float eps, int act, const void* residual, void* y,
                   fpnmt_stream_t stream);
int fpnmt_bn_bwd(int dtype, long long rows, int c, const void* x, const float* mean, const float* var,
                 const float* gamma, float eps, int act, const void* y, const void* dy, void* dx,
                 float* dgamma, float* dbeta, fpnmt_stream_t stream);
/* Cross-replica (sync) BatchNorm under data parallelism, the statistics of
 * the GLOBAL batch as the reference computes them on one device
 * (models/mobilenet.py:61 Keras BatchNormalization): each rank
 * reduces its rows to fp64 sums (2c + 1 doubles: [0, c) and [c, 2c) the
 * per-channel sums, [2c] the row count), the caller SUM-all-reduces them
 * over the ranks (RCCL / gloo), then
 *   fpnmt_bn_stats_sums: sum x, sum x^2 of this rank's rows;
 *   fpnmt_bn_stats_finalize: mean / biased variance (and the moving
 *     averages) from the all-reduced sums;
 *   fpnmt_bn_bwd_sums: sum g, sum g*xhat of this rank's rows
 *     (g = dy * act'(y)); the rank's own parts are added to dgamma / dbeta;
 *   fpnmt_bn_bwd_dx: dx from the all-reduced backward sums; the global row
 *     count is read on the device from sums[2c] (the all-reduced count, so
 *     ranks whose shards differ in size normalise by the same total).
 * With one rank the sequence equals fpnmt_bn_stats / fpnmt_bn_bwd. */
int fpnmt_bn_stats_sums(int dtype, long long rows, int c, const void* x, double* sums, fpnmt_stream_t stream);
int fpnmt_bn_stats_finalize(int c, const double* sums, float* mean, float* var, float* moving_mean,
                            float* moving_var, float momentum, fpnmt_stream_t stream);
int fpnmt_bn_bwd_sums(int dtype, long long rows, int c, const void* x, const float* mean, const float* var,
                      float eps, int act, const void* y, const void* dy, double* sums, float* dgamma,
                      float* dbeta, fpnmt_stream_t stream);
int fpnmt_bn_bwd_dx(int dtype, long long rows, int c, const void* x, const float* mean, const float* var,
                    const float* gamma, float eps, int act, const void* y, const void* dy, const double* sums,
                    void* dx, fpnmt_stream_t stream);
int fpnmt_depthwise_fwd(int dtype, int n, int h, int w, int c, int kh, int kw, int stride, int pad_t,
                        int pad_b, int pad_l, int pad_r, const void* x, const float* w_hwc, void* y,
                        fpnmt_stream_t stream);
int fpnmt_depthwise_bwd_data(int dtype, int n, int h, int w, int c, int kh, int kw, int stride, int pad_t,
                             int pad_b, int pad_l, int pad_r, const void* dy, const float* w_hwc, void* dx,
                             fpnmt_stream_t stream);
int fpnmt_depthwise_bwd_filter(int dtype, int n, int h, int w, int c, int kh, int kw, int stride, int pad_t,
                               int pad_b, int pad_l, int pad_r, const void* x, const void* dy, float* dw_hwc,
                               fpnmt_stream_t stream);

/* ---- input pipeline (dataset.py:19-26 load_image) --------
 * Replaces tf.image.resize(img, (out_h, out_w)) (bilinear, TF2 half-pixel
 * centres, no antialias) followed by mobilenet_v2.preprocess_input
 * (x / 127.5 - 1; pass div = 127.5, sub = 1) for a batch of decoded RGB
 * uint8 images of any sizes, in one launch:
 *   out[i] (out_h, out_w, 3) NHWC = resize(image i) / div - sub,
 * image i = the h*w*3 bytes at pixels + items_dev[i].offset (rows of w RGB
 * triples, as tf.image.decode_jpeg(channels=3) returns them). items_dev is a
 * device array of n items; max_w >= every item's w sizes the LDS row window
 * (a wider row is read from global memory instead). pixel_bytes = the
 * packed buffer's size (no read past it). fp32 arithmetic bit-identical to
 * TF's formula (no FMA contraction, IEEE divide); bf16 output is the RNE
 * rounding of that fp32 value. Items with h or w <= 0 produce zeros.      */
typedef struct fpnmt_image_item {
  long long offset; /* byte offset of pixel (0, 0) in the packed buffer */
  int h, w;         /* decoded rows / columns */
} fpnmt_image_item;
int fpnmt_image_resize_normalize(const fpnmt_image_item* items_dev, int n, const uint8_t* pixels,
                                 long long pixel_bytes, int max_w, int out_h, int out_w, float div, float sub,
                                 int dtype, void* out, fpnmt_stream_t stream);

/* ---- train-time augmentation of the same packed batch ------------------
 * One fpnmt_image_aug per image, in device memory: a crop box in source
 * pixels, a left-right mirror and three colour factors.
 *   out[i] = normalise(colour(resize(box of image i, mirrored if flip)))
 * resize: the bilinear formula above with in_size = ch / cw and the source
 * indices offset by y0 / x0; with flip, box column k is read at source
 * column x0 + cw - 1 - k. The colour steps run on the resized fp32 value
 * v in [0, 255] in this order, every multiply and add rounded separately,
 * with a clamp to [0, 255] after each executed step:
 *   contrast   (c != 1 and sums != NULL): v = m + (v - m) * c, where
 *              m = (float)((double)(299 S_R + 587 S_G + 114 S_B) /
 *              (double)(1000 ch cw)) is the mean luma of the SOURCE box from
 *              its integer byte sums (fpnmt_image_crop_stats);
 *   brightness (b != 1): v = v * b;
 *   saturation (s != 1): g = 0.299f r + 0.587f g + 0.114f b (left to right),
 *              v = g + (v - g) * s.
 * Then v / div - sub. A factor of exactly 1.0f SKIPS its step, so the
 * identity record (full box, no flip, factors 1) reproduces
 * fpnmt_image_resize_normalize bit for bit. The records are device data the
 * entry cannot check: the kernels clamp a box to its image, and a box or an
 * image with no pixels writes zeros. max_cw >= every box's cw sizes the LDS
 * window (a wider box is read from global memory instead).
 *
 * fpnmt_image_crop_stats writes sums[4 i + 0..2] = the R, G, B byte sums of
 * image i's (clamped) box and sums[4 i + 3] = 0. It zeroes `sums` itself on
 * the stream; integer sums do not depend on the order the blocks finish in. */
typedef struct fpnmt_image_aug {
  int y0, x0, ch, cw; /* crop box in source pixels, inside the image, ch, cw >= 1 */
  int flip;           /* 1: mirror the box left-right */
  float brightness, contrast, saturation; /* factors; exactly 1.0f = step skipped */
} fpnmt_image_aug;
int fpnmt_image_crop_stats(const fpnmt_image_item* items_dev, const fpnmt_image_aug* aug_dev, int n,
                           const uint8_t* pixels, long long pixel_bytes, unsigned long long* sums,
                           fpnmt_stream_t stream);
int fpnmt_image_augment_resize_normalize(const fpnmt_image_item* items_dev, const fpnmt_image_aug* aug_dev,
                                         const unsigned long long* sums, int n, const uint8_t* pixels,
                                         long long pixel_bytes, int max_cw, int out_h, int out_w, float div,
                                         float sub, int dtype, void* out, fpnmt_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FPNMT_H */

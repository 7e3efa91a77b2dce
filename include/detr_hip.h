/* detr_hip.h -- C ABI of libdetr_hip.so: the MI355X (gfx950) hot path of DETR
 * (ResNet backbone convolutions, transformer GEMMs/attention pieces, Hungarian set loss,
 * clip+Adam) as hand-written HIP kernels.
 *
 * The reference (Visual-Behavior/detr-tensorflow) has NO native/FFI boundary: its hot path is
 * TensorFlow ops plus one host callback into SciPy.  Each entry point below therefore cites the
 * reference Python lines whose arithmetic it replaces (paths relative to the reference root).
 * INTEGRATION.md shows the ctypes binding a maintainer of the reference would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (torch.Tensor storage); nothing is
 *     allocated, freed or synchronised inside; every call only enqueues work on `stream`
 *     (a hipStream_t passed as void*) and is safe to capture in a hipGraph; whatever changes from one
 *     training step to the next (dropout step seed, Adam step sizes) is read from DEVICE memory, so a
 *     captured step can be replayed;
 *   - all arithmetic is fp32 ("f32" in the names); indices are int32 on the device;
 *   - return value: 0 = ok, negative = rejected (bad shape / alignment / launch failure); the
 *     reason is retrievable with detr_hip_last_error() (thread-local);
 *   - thread-safe for distinct streams.
 */
#ifndef DETR_HIP_H
#define DETR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DETR_HIP_ABI_VERSION 9

const char *detr_hip_last_error(void);
int detr_hip_abi_version(void);
/* The integer tuning variables DETR_HIP_<NAME> (A/B switches of the kernel dispatch; all default 0 = the measured heuristic) are
 * read from the environment ONCE, when the library is loaded -- never on the launch path.  A process that changes one afterwards
 * (tests, tuning scripts) calls this to have it re-read. */
int detr_hip_reload_tuning(void);
/* ABI self-check for hand-written mirrors of the descriptor structs below (ctypes / cgo / JNI): for struct `which` writes
 * out[0] = sizeof, out[1..] = offsetof of every field in declaration order, and returns the number of values even when that
 * exceeds `cap` (never more than `cap` values are written; call again with a larger buffer).  An unknown id returns a negative
 * code and leaves a message.  The ids are opaque numbers, and the id behind each known one stays unknown (10..99, 101, 201, ...,
 * 801): a binder may probe it.
 *     0 detr_reduce_desc      1 detr_gemm_desc        2 detr_conv3x3_desc       3 detr_stem_desc       4 detr_layernorm_desc
 *     5 detr_attn_desc        6 detr_setloss_desc     7 detr_input_desc         8 detr_postprocess_desc
 *     9 detr_map_match_desc 100 detr_detect_desc    200 detr_tile_merge_desc  300 detr_overlay_desc  400 detr_track_desc
 *   500 detr_track_embed_desc                       600 detr_track_motion_desc
 *   700 detr_conv3x3d_desc  800 detr_coco_match_desc */
int detr_hip_struct_layout(int32_t which, int32_t *out, int32_t cap);
/* zero fill of accumulators (an ordinary kernel: a captured hipMemsetAsync node did not replay reliably) */
int detr_hip_memset_zero(void *ptr, size_t bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Generic batched GEMM with fused epilogue:   C = epi( A(MxK) * B(KxN) )
 *   replaces: every tf.matmul / 1x1 Conv2D / Linear on the path --
 *     detr_tf/networks/custom_layers.py:49-50 (Linear), resnet_backbone.py:101,107,111 (1x1 convs),
 *     detr.py:44 (input_proj), transformer.py:294-304,317,343,346 (MHA projections, QK^T, PV),
 *     and their tape gradients (optimizers.py:115): dgrad and wgrad are the same kernel with
 *     other operand layouts.
 *   epilogue, in this order:  v = acc; v *= scale[n]; v += bias[n]; v *= alpha;
 *                             v += residual[m,n]; act(v); v = mask[m,n] > 0 ? v : 0
 *     (frozen-BN fold custom_layers.py:21-24, bias, q-scaling transformer.py:307, residual adds,
 *      ReLU, sigmoid detr.py:188, ReLU-backward masking)
 *   a_kcontig = 1: A[m*lda + k]   0: A[k*lda + m]        (same for B with n)
 *   batch z in [0,batch): z0 = z / batch_inner, z1 = z % batch_inner, operand offset z0*s?0 + z1*s?1
 *   split_k > 1: the K range is split over split_k workgroups whose partial results are
 *     atomically ADDED to C (C must hold zeros or the value to accumulate onto); only
 *     scale and alpha are allowed in the epilogue then.
 * ------------------------------------------------------------------------------------------- */
/* one deferred deterministic split-K reduction: C[r][c] += alpha * scale[c] * sum_s ws[s*part_stride + r*cols + c]
 * (+ the fused bias gradient rs_out[r] += rs_alpha * sum_s rs_ws[s*rows + r]); filled by detr_hip_gemm_f32 /
 * detr_hip_gemm_group_f32 when detr_gemm_desc.defer_out is set, consumed by detr_hip_splitk_reduce_many */
typedef struct detr_reduce_desc {
    const float *ws; int32_t splits; int64_t part_stride; int32_t rows, cols;
    float *C; int64_t ldc; float alpha; const float *scale;
    const float *rs_ws; float *rs_out; float rs_alpha;
    /* ABI 5: slab layout.  ts_bm == 0: row-major slabs (ws[s*part_stride + r*cols + c]).  ts_bm > 0: tile-ordered slabs as the
     * split kernels of this library write them when the workspace holds detr_hip_workspace_bytes_* bytes -- tiles of
     * ts_bm x ts_bn (ts_tiles_n of them per tile row), each a lane-linear image of the MFMA accumulator registers
     * (csrc/gemm_core.h: store_slab_ts); part_stride then counts the padded tile grid. */
    int32_t ts_bm, ts_bn, ts_tiles_n;
} detr_reduce_desc;

typedef struct {
    int32_t M, N, K;
    const float *A; int64_t lda; int32_t a_kcontig;
    const float *B; int64_t ldb; int32_t b_kcontig;
    float *C; int64_t ldc;
    int32_t batch, batch_inner;
    int64_t sA0, sA1, sB0, sB1, sC0, sC1;
    float alpha;
    const float *scale;
    const float *bias;
    const float *residual; int64_t ldr;
    const float *mask; int64_t ldmask;
    int32_t act;            /* 0 none, 1 relu, 2 sigmoid */
    int32_t split_k;        /* 0/1 = no split */
    /* optional caller-provided scratch for DETERMINISTIC split-K: when it holds at least
     * split_k*M*N floats (and batch == 1) every split stores its partial tile there with plain
     * 16-byte stores and a second launch reduces them onto C (C += alpha*scale*sum); otherwise
     * the partials are accumulated with fp32 atomics. */
    float *workspace; int64_t workspace_bytes;
    /* fused dropout (training mode, transformer.py:169,174-176): keep-mask = keyed counter hash of
     * (site = dropout_seed, step seed = *dropout_step, element row*N + col), kept values scaled by 1/(1-p); applied
     * before the residual add when a residual is given, otherwise after the activation.  0 = off.
     * dropout_step (last field of this struct) is a DEVICE pointer to the uint32 seed of the current training step
     * (NULL = 0): a hipGraph replay of a captured step reads a fresh seed. */
    float dropout_p; uint32_t dropout_seed;
    /* 0 = exact fp32 MFMA (parity mode); 1 = bf16 MFMA with fp32 storage / accumulation (BASELINE config C3:
     * operands are rounded to bf16 on their way into LDS); 2 (ABI 9, "f32x3") = fp32 storage AND fp32 accuracy on the bf16
     * matrix pipe: every fp32 operand value is split exactly into three bf16 values (x = h + m + l) and a product is the sum
     * of the six largest of the nine bf16 partial products, accumulated in fp32 (relative error of a product <= 2^-23, the
     * size of one fp32 rounding; csrc/gemm_core.h: mma_ktile_split3) -- 6 bf16 MFMAs instead of 8 fp32 MFMAs per 32x32x16
     * block at 16x the instruction rate.  Both forms are fp32-accurate; the split kernel takes the shapes on which it is the
     * faster one (csrc/gemm_f32.hip: gemm_split3_shape) -- N > 32 and M >= 128, N >= 128, K >= 256; DETR_HIP_SPLIT3_ALL=1 leaves
     * N > 32 alone -- and every other shape runs the exact kernel.  Any other value of `compute` is rejected.
     * THE STORAGE RULE (here, detr_conv3x3_desc, detr_conv3x3d_desc, detr_stem_desc): every *_dtype field is 0 (fp32) or 1 (bf16;
     * m_dtype also 2, bit-packed), anything else is rejected; a field other than 0 needs compute = 1 -- under compute 0 and 2
     * operands, C, residual and mask are all fp32.  Under compute = 1 the fields are independent of each other: any mix of fp32 and
     * bf16 A, B, C, residual and mask is accepted (subject to the alignment each bf16 operand states below) and computes the same
     * fp32 epilogue values, rounded once where C is bf16; only the bit-packed masks need the all-bf16 form (maskbits_out). */
    int32_t compute;
    /* optional fused bias gradient of a weight-gradient GEMM (dW = dy^T x): rowsum_a[m] += rowsum_alpha * sum_k A[m][k]
     * (A must be MN-contiguous, a_kcontig = 0; batch == 1; with split_k > 1 the deterministic workspace path is
     * required and the workspace must hold split_k*(M*N + M) floats).  Replaces the reference's separate
     * reduce_sum for every Linear bias gradient (tape gradient of custom_layers.py Linear bias). */
    float *rowsum_a; float rowsum_alpha;
    /* 0: B is fp32.  1: B points to bf16 data (uint16, RNE-rounded weights; ldb in elements) -- bf16 compute only: the
     * engine keeps a per-step bf16 shadow of the weights so that the weight operand is read at half the bytes and
     * without conversion (K %% 8 == 0 for a k-contiguous B, N %% 4 == 0 otherwise). */
    int32_t b_dtype;
    /* bf16 STORAGE of activation tensors (bf16 compute only, see `compute`; the engine's backbone tensors in bf16 mode): 1 = the
     * tensor is bf16 in memory (uint16, RNE; leading dimensions in elements), 0 = fp32.  The epilogue arithmetic stays
     * fp32 and the result is rounded once.  Not with split_k / batch (partial slabs and gradients of parameters stay fp32). */
    int32_t a_dtype, c_dtype, r_dtype, m_dtype;     /* A, C, residual, mask (m_dtype 2: bit-packed, see maskbits_out) */
    const uint32_t *dropout_step;                   /* see dropout_p */
    /* optional (HOST pointer): with deterministic split-K, do not launch the reduction but describe it here (splits = 0 when
     * no reduction is pending); the caller keeps `workspace` intact and reduces many slabs per launch with
     * detr_hip_splitk_reduce_many -- the weight gradients of a backward pass are only needed by the optimiser */
    detr_reduce_desc *defer_out;
    /* ABI 5: bit-packed ReLU masks (bf16 activation storage only, N %% 8 == 0).  The backward of `relu` only needs the SIGN of the
     * saved activation: a GEMM whose epilogue ends in the ReLU can emit, next to C, one byte per 8 outputs --
     * bit (n & 7) of maskbits_out[m * ld_maskbits_out + n / 8] = (C[m][n] > 0) as stored -- and a later GEMM takes it instead of
     * the activation tensor: `mask` pointing to those bytes with m_dtype = 2 and ldmask = their row pitch in BYTES (1/16 of the
     * bytes of the bf16 tensor on an HBM-bound launch; resnet_backbone.py:132-135 backward). */
    uint8_t *maskbits_out; int64_t ld_maskbits_out;
    /* Optional fused LayerNormalization of the output rows (ln_y != NULL; transformer.py:151-152 behind every attention / FFN block,
     * :169-170,177,215-233): C = drop((A B^T + bias) * alpha) + residual is written as usual (the backward reads the LayerNorm INPUT)
     * and, from the same launch,  ln_y = LayerNorm(C; ln_gamma, ln_beta, ln_eps), ln_mean / ln_rstd [M], optionally
     * ln_y2[r] = ln_y[r] + ln_add[r % ln_add_rows] and the bf16 twin ln_y16 -- the outputs of detr_hip_layernorm_fwd, bit for bit.
     * Needs: compute = 1, N = 256 = ldc (contiguous fp32 C / ln_y / ln_y2 / residual rows), a_kcontig = b_kcontig = 1, b_dtype = 1,
     * K % 8 == 0, batch = split_k = 1, act = 0, no scale / mask; anything else is rejected. */
    const float *ln_gamma, *ln_beta; float *ln_y, *ln_mean, *ln_rstd; const float *ln_add; int32_t ln_add_rows; float *ln_y2;
    uint16_t *ln_y16; float ln_eps;
    /* Optional residual row map (appended; all 0 = identity): the output rows are the pixels of [.., res_sub_h, res_sub_w] maps
     * (M %% (res_sub_h * res_sub_w) == 0) and `residual` is the COMPACT [.., res_sub_ho, res_sub_wo, N] tensor of their even pixels
     * (res_sub_ho = (res_sub_h + 1) / 2, res_sub_wo = (res_sub_w + 1) / 2): output pixel (n, y, x) adds residual row (n, y / 2, x / 2)
     * when y and x are both even and nothing otherwise (an exact zero, no memory request).  C and the mask keep their own rows.
     * This is the input gradient of a stride-2 1x1 convolution (the projection shortcut of a stage's first block) added without
     * scattering it into a zero-filled full-resolution tensor first.  All-bf16 epilogues only: bf16 C and residual (c_dtype =
     * r_dtype = 1), compute = 1, N %% 8 == 0, 16-byte aligned rows, no batch / split_k / fused LayerNorm; anything else is rejected. */
    int32_t res_sub_h, res_sub_w, res_sub_ho, res_sub_wo;
} detr_gemm_desc;
int detr_hip_gemm_f32(const detr_gemm_desc *d, void *stream);
/* the kernel family detr_hip_gemm_f32 would launch for this descriptor (no launch): 0 tile engine, 1 streaming kernel, 2 ring kernel (bf16),
 * 3 ring kernel (fp32), 4 GEMM + LayerNorm, 5 ring weight gradient; negative = rejected.  For callers that bill launches to roofline families. */
int detr_hip_gemm_family(const detr_gemm_desc *d);
/* the split_k a reduction-heavy [M, N] = [M, K] x [K, N] GEMM (a weight gradient) should ask for (appended; no launch): as many splits, at most
 * max_split, as fill the chip with the tiles detr_hip_gemm_f32 runs that split on -- the plan and the tile rule share their shape predicates.
 * compute as in detr_gemm_desc.  Tuning: DETR_HIP_SPLIT_TARGET / _SPLIT_TARGET64 / _X3_SPLIT_TARGET (workgroups aimed at on bf16 128 x 128, on
 * 64 x 64 and on f32x3 128 x 128 tiles; a negative _X3_SPLIT_TARGET plans f32x3 on 64 x 64 tiles) and DETR_HIP_SPLIT3_T128.
 * Returns the split (>= 1); -1 (detr_hip_last_error) for a non-positive dimension, compute outside 0 .. 2 or max_split < 1. */
int32_t detr_hip_gemm_split_plan(int32_t M, int32_t N, int32_t K, int32_t compute, int32_t max_split);
int detr_hip_splitk_reduce_many(const detr_reduce_desc *descs, int32_t n, void *stream);
/* n independent GEMMs in one call.  Consecutive members (up to 4) that share one kernel variant -- 64x64 tiles, same operand
 * layouts / storage types, no batch -- are issued as ONE launch (members on blockIdx.y) and their split-K reductions as one
 * more; otherwise the members are launched one after the other.  Members must not alias each other's outputs or workspaces.
 * Used for the Q / K / V projections of an attention block and their gradients (transformer.py:297-309), whose individual
 * launches fill only 1-2 workgroups per CU. */
int detr_hip_gemm_group_f32(const detr_gemm_desc *descs, int32_t n, void *stream);

/* ---------------------------------------------------------------------------------------------
 * 3x3 convolution (explicit zero pad `pad`, then VALID, stride 1|2; dilation 1 -- dilation 2 is detr_hip_conv3x3_dilated at the
 * end of this header), NHWC / HWIO,
 * as an implicit GEMM (no im2col buffer):
 *   replaces: ZeroPadding2D + Conv2D(3x3) + FrozenBatchNorm2D + ReLU
 *             detr_tf/networks/resnet_backbone.py:98,104-105,123-126 and its gradients.
 *   mode 0 fwd  : y[N,Ho,Wo,Co]  = epi( conv(x[N,Hi,Wi,Ci], w[3,3,Ci,Co]) )
 *   mode 1 dgrad: dx[N,Hi,Wi,Ci] = epi( conv^T(dy[N,Ho,Wo,Co], w) )          (x = dy in, y = dx out)
 *   mode 2 wgrad: dw[3,3,Ci,Co] += scale[co] * sum_m x[pix(m,tap),ci] * dy[m,co]   (atomic; y = dw)
 *   epilogue fields as in detr_gemm_desc (rows = output pixels, ld = channel count).
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    int32_t N, Hi, Wi, Ci, Ho, Wo, Co, stride, pad;
    const float *x;      /* fwd: input; dgrad: dy; wgrad: input x */
    const float *w;      /* fwd/dgrad: weights; wgrad: dy */
    float *y;            /* fwd: output; dgrad: dx; wgrad: dw (pre-zeroed / accumulated onto) */
    float alpha;
    const float *scale;
    const float *bias;
    const float *residual;
    const float *mask;
    int32_t act;
    int32_t split;       /* wgrad: number of row splits (0 = auto) */
    float *workspace; int64_t workspace_bytes;   /* wgrad: scratch for deterministic split reduction (see detr_gemm_desc) */
    int32_t compute;     /* 0 = exact fp32 MFMA, 1 = bf16 MFMA, 2 = fp32 accuracy on the bf16 matrix pipe (see detr_gemm_desc) */
    int32_t w_dtype;     /* modes 0/1 with compute = 1: 1 = `w` points to bf16 data (weight shadow, see detr_gemm_desc.b_dtype) */
    /* bf16 storage of the activation tensors (see detr_gemm_desc.a_dtype): x = the tensor passed as `x`, y = the one passed as `y`
     * (mode 2: x = input activations, `w` = dy whose dtype is w_dtype, y = dw always fp32), r = residual, m = mask */
    int32_t x_dtype, y_dtype, r_dtype, m_dtype;
    /* ABI 5: bit-packed ReLU masks as in detr_gemm_desc (bf16 tensors only): mode 0 with act = 1 also writes one byte per 8 output
     * channels, bit = (y > 0), row pitch Co / 8 bytes per pixel; modes 0 / 1 take `mask` as such bytes when m_dtype = 2 */
    uint8_t *maskbits_out;
} detr_conv3x3_desc;
int detr_hip_conv3x3_f32(const detr_conv3x3_desc *d, int32_t mode, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Stem helpers (detr_tf/networks/resnet_backbone.py:11-26):
 *   3x3 stride-2 max pool over the ZERO-padded (pad 1) map (padding takes part in the max, as
 *   ZeroPadding2D + MaxPool2D('valid') does) with argmax for the backward;
 *   maxpool backward fused with the stem ReLU mask.
 * ------------------------------------------------------------------------------------------- */
/* fp32 -> bf16 (RNE) copies that feed the bf16 weight operands: a flat conversion (n %% 4 == 0) and the frozen-BN fold
 * out[r][c] = bf16(w[r][c] * scale[c]) (custom_layers.py:21-24 folded into the conv kernel). */
int detr_hip_cvt_bf16(const float *x, uint16_t *out, int64_t n, void *stream);
int detr_hip_scale_cols_bf16(const float *w, const float *scale, uint16_t *out, int64_t rows, int32_t cols, void *stream);
/* The same fold for a whole list of kernels in ONE launch (the backbone has 52 folded convs and refolds them after every
 * optimiser step).  `table` is DEVICE memory holding n entries of this layout; c4 = cols/4, n4 = rows*cols/4. */
typedef struct detr_scale_entry {
    const float *w;
    const float *scale;
    uint16_t *out;
    int64_t n4;
    int32_t c4;
    int32_t reserved;
} detr_scale_entry;
int detr_hip_scale_cols_bf16_group(const detr_scale_entry *table, int32_t n, void *stream);

/* The stem convolution as an IMPLICIT GEMM (no im2col buffer): ZeroPadding2D(3) + 7x7 stride-2 VALID conv 3 -> 64
 * (+ folded frozen BN + ReLU), resnet_backbone.py:11-26.   mode 0: y[M,64] = act((gather(img) @ w[147][64]) * scale + bias) * ...
 * with the GEMM epilogue order of detr_gemm_desc; mode 2 (weight gradient): w = dy [M,64], y = dw [147][64],
 * dw += alpha * scale[co] * sum_m gather(img)[m][k] * dy[m][co], reduction split over `split` workgroups through
 * `workspace` (split*147*64 floats, deterministic).  M = N*Ho*Wo, k = (kh*7 + kw)*3 + c. */
typedef struct {
    int32_t N, H, W, Ho, Wo;
    const float *img;       /* [N, H, W, 3] */
    const float *w;         /* mode 0: kernel [147][64]; mode 2: dy [M][64] */
    float *y;               /* mode 0: output [M][64]; mode 2: dw [147][64] */
    float alpha;
    const float *scale;
    const float *bias;
    int32_t act;
    int32_t split;
    float *workspace; int64_t workspace_bytes;
    int32_t compute;        /* 0 = exact fp32 MFMA, 1 = bf16 MFMA, 2 = fp32 accuracy on the bf16 matrix pipe (see detr_gemm_desc) */
    int32_t w_dtype;        /* mode 2: 1 = dy is bf16 in memory (bf16 activation storage) */
    int32_t y_dtype;        /* mode 0: 1 = the output is stored as bf16 */
} detr_stem_desc;
int detr_hip_stem_conv7x7_f32(const detr_stem_desc *d, int32_t mode, void *stream);
int detr_hip_maxpool3x3s2_fwd_f32(const float *x, float *y, uint8_t *argmax, int32_t N, int32_t H,
                                  int32_t W, int32_t C, int32_t Ho, int32_t Wo, void *stream);
/* dx[n,h,w,c] = (x[n,h,w,c] > 0) * sum over windows whose argmax is (h,w) of dy */
int detr_hip_maxpool3x3s2_bwd_f32(const float *dy, const uint8_t *argmax, const float *x, float *dx,
                                  int32_t N, int32_t H, int32_t W, int32_t C, int32_t Ho, int32_t Wo,
                                  void *stream);
/* stride-2 1x1 downsample helpers (resnet_backbone.py:111-113): gather / zero-filled scatter */
/* bf16-storage twins of the stem max pooling (see detr_gemm_desc.a_dtype); the subsample kernels are plain 16-byte copies and
 * serve bf16 tensors with C/2 "float" channels. */
int detr_hip_maxpool3x3s2_fwd_bf16(const uint16_t *x, uint16_t *y, uint8_t *argmax, int32_t N, int32_t H, int32_t W,
                                   int32_t C, int32_t Ho, int32_t Wo, void *stream);
int detr_hip_maxpool3x3s2_bwd_bf16(const uint16_t *dy, const uint8_t *argmax, const uint16_t *x, uint16_t *dx, int32_t N,
                                   int32_t H, int32_t W, int32_t C, int32_t Ho, int32_t Wo, void *stream);
int detr_hip_subsample2_fwd_f32(const float *x, float *y, int32_t N, int32_t H, int32_t W, int32_t C,
                                int32_t Ho, int32_t Wo, void *stream);
int detr_hip_subsample2_bwd_f32(const float *dy, float *dx, int32_t N, int32_t H, int32_t W, int32_t C,
                                int32_t Ho, int32_t Wo, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Row kernels of the transformer (detr_tf/networks/transformer.py):
 *   LayerNormalization(eps) over the last dim C (C % 4 == 0, C <= 1024) :151-152,169-170,177
 *   softmax over rows of the score tensor :340, and their backwards;
 *   column sums (bias gradients), broadcast add (src + pos :161-163, tgt + query_pos :209),
 *   sigmoid backward (detr.py:188).
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    int32_t rows, C; float eps;
    const float *x;                 /* fwd: input rows; bwd: the forward INPUT (xhat is recomputed from mean / rstd) */
    const float *gamma, *beta;
    float *y;                       /* fwd output */
    float *mean, *rstd;             /* [rows]: written by fwd, read by bwd */
    /* fwd, optional fused second output  y2[r] = y[r] + add[r % add_rows]  -- the `src + pos` / `tgt + query_pos`
     * operand of the NEXT attention block (transformer.py:161-163,209,219), written while y is still in registers */
    const float *add; int32_t add_rows; float *y2;
    uint16_t *y16;                  /* fwd, optional: bf16 (RNE) twin of y -- the A operand of the next bf16-compute GEMM */
    /* bwd */
    const float *dy; float *dx; float *dgamma, *dbeta;     /* dgamma / dbeta are ACCUMULATED */
    /* dgamma/dbeta reduction: deterministic (per-block partials in `workspace` + a finish launch) when the workspace
     * holds at least 512*2*C floats, fp32 atomics otherwise (workspace may be NULL) */
    float *workspace; int64_t workspace_bytes;
    const float *dx_add;            /* optional: dx += dx_add (a second gradient branch into the same tensor) */
    /* optional fused second output dx_drop[i] = keep(site, step, i) ? dx[i] / (1-p) : 0 -- the gradient through the
     * Dropout that precedes the residual add in front of this LayerNorm (transformer.py:169,176,215,226,232), i.e. the
     * mask of the forward GEMM epilogue regenerated on the gradient (element index row*C + col) */
    float *dx_drop; float dropout_p; uint32_t dropout_site; const uint32_t *dropout_step;
    uint16_t *dx_drop16;            /* optional bf16 twin of dx_drop (dropout_p = 0: of dx) */
    /* optional (HOST pointer; needs the workspace path): do not launch the dgamma / dbeta finish but report the number of
     * partial blocks -- the caller owns `workspace` ([blocks][2*C]: gamma partials, then beta partials, per block) and
     * reduces it later through detr_hip_splitk_reduce_many (two entries: rows 1, cols C, splits = blocks, part_stride 2*C) */
    int32_t *defer_blocks_out;
    const float *dy_add;            /* bwd, optional: the incoming gradient is dy + dy_add (two branches meeting at this LayerNorm's output) */
} detr_layernorm_desc;
int detr_hip_layernorm_fwd(const detr_layernorm_desc *d, void *stream);
int detr_hip_layernorm_bwd(const detr_layernorm_desc *d, void *stream);
/* out[c] += alpha * sum_r x[r*ld + c] (atomic) */
int detr_hip_colsum_f32(const float *x, float *out, int64_t rows, int32_t cols, int64_t ld, float alpha,
                        void *stream);
/* The same sum in a FIXED order (round 5: the bias gradients of input_proj and of the heads -- detr.py:172-175, 192-203 -- were the one
 * gradient of the step that differed between two runs, by float-atomic order): per-chunk partial sums into `scratch` (at least
 * detr_hip_colsum_det_scratch_floats(rows, cols) floats), then one ordered pass over the chunks.  Two launches, no atomics. */
int64_t detr_hip_colsum_det_scratch_floats(int64_t rows, int32_t cols);
int detr_hip_colsum_det_f32(const float *x, float *out, int64_t rows, int32_t cols, int64_t ld, float alpha, float *scratch,
                            int64_t scratch_floats, void *stream);
/* Backward of a bottleneck 1x1 convolution 64 -> 256 channels in ONE pass over dY (round 5; reference: resnet_backbone.py:116-137 -- conv3 and the
 * projection shortcut of a BottleNeck -- and optimizers.py:110-120): da = (use_mask ? (a > 0) : 1) . (dY W^T) and dW += alpha * scale[n] * (a^T dY).
 * dY [M][ldg] (d2 = 256 columns), a [M][lda] (d1 = 64 columns: weight-gradient operand AND ReLU mask), W [64][ldw] (256 columns contiguous),
 * da [M][ldda] -- bf16; dW [64][lddw] fp32, scale [256] fp32 or NULL.  workspace: at least detr_hip_conv1x1_bwd_fused_workspace_floats(M) floats
 * (one 64 x 256 partial per workgroup, summed in a fixed order).  da is bit-identical to detr_hip_gemm_f32 on the same operands. */
int64_t detr_hip_conv1x1_bwd_fused_workspace_floats(int64_t M);
int detr_hip_conv1x1_bwd_fused_bf16(const uint16_t *dy, int64_t ldg, const uint16_t *a, int64_t lda, const uint16_t *w, int64_t ldw, uint16_t *da,
                                    int64_t ldda, int32_t use_mask, float *dw, int64_t lddw, const float *scale, float alpha, int64_t M, int32_t d1,
                                    int32_t d2, float *workspace, int64_t workspace_floats, void *stream);
/* out[i] = x[i] + p[i % period]   (n, period multiples of 4) */
int detr_hip_add_bcast_f32(const float *x, const float *p, float *out, int64_t n, int64_t period,
                           void *stream);
/* out[i] = a[i] + b[i] */
int detr_hip_add_f32(const float *a, const float *b, float *out, int64_t n, void *stream);
/* dz[i] = dy[i] * y[i] * (1 - y[i]) */
int detr_hip_sigmoid_bwd_f32(const float *dy, const float *y, float *dz, int64_t n, void *stream);
/* out[i] = keep(site, *step, i) ? x[i] / (1-p) : 0   -- the dropout mask of detr_gemm_desc regenerated on a gradient */
int detr_hip_dropout_f32(const float *x, float *out, int64_t n, float p, uint32_t site, const uint32_t *step, void *stream);
/* n independent flat copies (mode 0: 16-byte units, any element type) or fp32 accumulations dst += src (mode 1) in ONE launch;
 * `table` is DEVICE memory.  Gathers the per-layer decoder cross-attention K / V projection weights (transformer.py:221-223,
 * the memory operand is layer-invariant) into one [layers*256, 256] GEMM operand and scatters its gradient back. */
typedef struct detr_copy_entry {
    const void *src;
    void *dst;
    int64_t n16;        /* number of 16-byte units */
    int32_t mode;       /* 0 copy, 1 fp32 accumulate */
    int32_t reserved;
} detr_copy_entry;
int detr_hip_multi_copy(const detr_copy_entry *table, int32_t n, int32_t blocks_per_entry, void *stream);
/* tf_backbone=True (tf.keras.applications ResNet50, detr.py:146-148: convs WITH a trainable bias under a frozen BatchNorm):
 *   out[c] += scale[c] * sum_r x[r*ld + c]   (x fp32: x_dtype 0, bf16: 1) -- the bias gradient through the folded BN;
 *   out[i] = a[i]*b[i] + c[i] for n small vectors in one launch (table in DEVICE memory) -- the effective shift
 *   beta - mean*scale + scale*bias of every conv, rebuilt when the biases move. */
typedef struct detr_fma_entry {
    const float *a, *b, *c;
    float *out;
    int32_t n;
    int32_t reserved;
} detr_fma_entry;
int detr_hip_colsum_scaled(const void *x, int32_t x_dtype, int64_t rows, int32_t cols, int64_t ld, const float *scale,
                           float *out, void *stream);
int detr_hip_fma_vec_group(const detr_fma_entry *table, int32_t n, void *stream);
/* dst[0..7] = v0..v7 (uint32; the values travel as kernel arguments): the per-step dropout seed */
int detr_hip_set_u32x8(uint32_t *dst, uint32_t v0, uint32_t v1, uint32_t v2, uint32_t v3, uint32_t v4, uint32_t v5,
                       uint32_t v6, uint32_t v7, void *stream);
/* out[i] = (ref[i] > 0) ? g[i] : 0 */
int detr_hip_relu_mask_f32(const float *g, const float *ref, float *out, int64_t n, void *stream);
/* w_out[k, co] = w[k, co] * scale[co]   (frozen-BN scale folded into conv kernels, HWIO flat) */
int detr_hip_scale_cols_f32(const float *w, const float *scale, float *w_out, int64_t rows, int32_t cols,
                            void *stream);
/* w_out_t[co, k] = w[k, co] * scale[co] (scale may be NULL): transposed copy, i.e. a K-contiguous GEMM B operand */
int detr_hip_scale_cols_t_f32(const float *w, const float *scale, float *w_out_t, int32_t rows, int32_t cols,
                              void *stream);
/* frozen BN vectors -> (scale, shift)  custom_layers.py:21-23 */
int detr_hip_bn_fold_f32(const float *weight, const float *bias, const float *mean, const float *var,
                         float *scale, float *shift, int32_t C, float eps, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Fused multi-head attention core, head_dim 32 (detr_tf/networks/transformer.py:308-345):
 *   o[b,t,h*32:+32] = softmax_s( q[b,t,h] . k[b,s,h] ) v[b,s,h]      (scale = head_dim**-0.5, :307)
 * on batch-first token matrices; the [T,S] probability tensor is never
 * written to memory.  lse [B*H, T] (log-sum-exp per score row) is saved for the backward, which
 * recomputes the probabilities; delta [B*H, T] is scratch (rowsum(dO*O)).
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    int32_t B, H, T, S;
    /* batch-first token matrices; every tensor has its OWN row stride (floats), so q / k / v (and their gradients) may
     * be column blocks of one packed projection buffer: [rows, 768] for self-attention, [rows, layers*256] for the
     * layer-invariant decoder cross-attention K / V of all layers */
    const float *q; int64_t ldq;
    const float *k; int64_t ldk;
    const float *v; int64_t ldv;
    float *o; int64_t ldo;          /* fwd: output; bwd: the forward output */
    float *lse;                     /* [B*H, T] */
    const float *d_o; int64_t ldd_o;
    float *dq; int64_t lddq;
    float *dk; int64_t lddk;
    float *dv; int64_t lddv;
    float *delta;                   /* [B*H, T] scratch */
    /* softmax(scale * q.k): the reference scales the projected query (WQ *= head_dim**-0.5, transformer.py:307); here
     * the factor is folded into the constant q is loaded with, and dq is the gradient w.r.t. the UNSCALED q */
    float scale;
    /* attention-probability dropout (transformer.py:341): element index ((b*H + h)*T + t)*Sp + s, Sp = S rounded up to
     * even (one keyed counter hash per pair of adjacent keys, csrc/common.h); site / step as in detr_gemm_desc */
    float dropout_p; uint32_t dropout_site; const uint32_t *dropout_step;
    /* 0 = exact fp32 MFMA on fp32 tensors (io_dtype = 0; 2 runs the same kernels); 1 = bf16 MFMA, valid only with
     * bf16 tensors (io_dtype = 1, below) -- io_dtype = 0 with compute = 1 is rejected */
    int32_t compute;
    /* ABI 8.  io_dtype = 1 (compute = 1 only; csrc/attention_dma.hip): q, k, v, o, d_o, dq, dk, dv point to bf16 data (uint16, RNE;
     * row strides in elements, multiples of 8), `q` holds bf16(scale * log2(e) * q_unscaled) -- the projection GEMM's alpha -- and dq
     * is still the gradient w.r.t. the UNSCALED q; lse stays fp32 and `delta` must hold 2*B*H*T floats (delta / keep-scale and
     * lse * log2(e) - log2(keep-scale), handed from the dQ kernel to the dK / dV kernel).  With dropout_p > 0 the keep flags are read
     * as BITS from `dropmask` (detr_hip_attention_dropmask_words(B, H, T, S) uint32 words: one word per (query, 32-key tile), word
     * (bh * ceil(S/32) + tile) * 32 ceil(T/32) + query, bit = key), which detr_hip_attention_dropmask fills
     * from (dropout_site, *dropout_step) -- the same function as the keyed counter hash above, evaluated once per step instead of in
     * each of the three kernels. */
    int32_t io_dtype;
    uint32_t *dropmask;
} detr_attn_desc;
int detr_hip_attention_fwd(const detr_attn_desc *d, void *stream);
int detr_hip_attention_bwd(const detr_attn_desc *d, void *stream);
/* keep bits of the attention-probability dropout of one site and step (io_dtype = 1): uses B, H, T, S, dropout_p, dropout_site,
 * dropout_step and dropmask of the descriptor */
int64_t detr_hip_attention_dropmask_words(int32_t B, int32_t H, int32_t T, int32_t S);
int detr_hip_attention_dropmask(const detr_attn_desc *d, void *stream);
/* the same for n sites of one step in ONE launch (they must share B*H, dropout_p and dropout_step; a DETR step has 18 sites) */
int detr_hip_attention_dropmask_many(const detr_attn_desc *descs, int32_t n, void *stream);
/* Key padding mask (detr_tf/networks/transformer.py:322-337 -- the reference's commented-out key_padding_mask branch -- as if
 * enabled, fed by source_key_padding_mask / memory_key_padding_mask, :43-50): the same attention with the scores of invalid keys
 * set to -inf before the softmax.  key_valid: detr_hip_attention_keymask_words(B, S) uint32 words, word (b * ceil(S/32) + t) bit j
 * = key 32 t + j of batch entry b is valid; bits past S must be 0.  Queries are never masked.  Both the exact-fp32 kernels
 * (io_dtype = 0) and the all-bf16 kernels (io_dtype = 1) have a masked form.  Every batch entry needs at least one valid key (otherwise its rows are NaN: see detr_hip_padding_mask_prepare's
 * status).  Masked keys get exact zeros in dk / dv; dropout keep bits are those of the unmasked call. */
int64_t detr_hip_attention_keymask_words(int32_t B, int32_t S);
int detr_hip_attention_fwd_masked(const detr_attn_desc *d, const uint32_t *key_valid, void *stream);
int detr_hip_attention_bwd_masked(const detr_attn_desc *d, const uint32_t *key_valid, void *stream);
/* transformer.py:349-354 (need_weights): w[b, t, s] = (1/H) sum_h softmax_s(scale q.k)[b,h,t,s], written as fp32 rows of
 * stride ldw (floats, >= S); uses B, H, T, S, q/ldq, k/ldk, lse, scale, compute, io_dtype of the descriptor (v, o and the
 * gradient fields are ignored); lse is the one the forward wrote for the same q, k (and the same key_valid).
 * key_valid: NULL or the words of detr_hip_attention_fwd_masked; a masked key gets an exact 0.
 * dropout_p must be 0 (rejected otherwise).  H <= 8, S <= 8192.  One pass that never forms the per-head [B*H, T, S] tensor: the H
 * score tiles of a 32 x 32 block are accumulated in registers (csrc/attention_weights.hip); bound by the B*T*S*4 bytes it writes. */
int detr_hip_attention_weights(const detr_attn_desc *d, const uint32_t *key_valid, float *w, int64_t ldw, void *stream);
/* Padding mask -> transformer inputs (detr_tf/networks/detr.py:57-72 downsample_masks, position_embeddings.py:23-50 with
 * normalize=True), one launch: mask [B, H, W] uint8 / bool (nonzero = padding) is brought to the Hf x Wf feature map by TF-legacy
 * nearest neighbour (src = min(floor(dst * in / out), in - 1) per axis), and per image
 *   key_valid [B][ceil(Hf*Wf/32)]  the words of detr_hip_attention_*_masked (bit = feature position is valid),
 *   pos [B * Hf * Wf, 256]         [pos_y | pos_x] gathered from tab_y [Hf+1][Hf+1][128] / tab_x [Wf+1][Wf+1][128]: entry [n][c] is
 *                                  the encoding of cumulative count c of an axis with n valid positions (c / (n + 1e-6) * 2 pi),
 *   status [B]                     1 when the image has no valid feature position, else 0.
 * Hf, Wf <= 128 and Hf * Wf <= 8192.  tab_y, tab_x and pos 16-byte aligned. */
int detr_hip_padding_mask_prepare(const uint8_t *mask, int32_t B, int32_t H, int32_t W, int32_t Hf, int32_t Wf, const float *tab_y,
                                  const float *tab_x, uint32_t *key_valid, float *pos, int32_t *status, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Hungarian set loss (detr_tf/loss/hungarian_matching.py:163-203, detr_tf/loss/loss.py:22-179,
 * detr_tf/bbox.py:29-124,171-183).  P = levels * B problems; prediction p of level lv, image b:
 *   logits + lv*sL_l + b*sL_b + q*sL_q + c ,  boxes + lv*sB_l + b*sB_b + q*sB_q + k
 * targets in the reference's header layout (detr_tf/data/processing.py:35-55):
 *   t_bbox [B, R, 4] f32 (row 0 = [n,0,0,0]), t_class [B, R] int64 (row 0 = 0).
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    int32_t levels, B, Q, C, R;        /* R = target rows incl. header (100) */
    const float *logits; int64_t sL_l, sL_b, sL_q;
    const float *boxes;  int64_t sB_l, sB_b, sB_q;
    const float *t_bbox; const int64_t *t_class;
    int32_t background_class;
} detr_setloss_desc;

/* K12: cost[p][q][j] (ld = R-1 per q) = 5*L1 + 1*(-softmax[class_j]) + 2*(-GIoU)   hungarian_matching.py:171-195 */
int detr_hip_match_cost_f32(const detr_setloss_desc *d, float *cost, void *stream);
/* K13: exact rectangular assignment per problem (replaces the tf.numpy_function -> SciPy call,
 *   hungarian_matching.py:27-46,197).  cost [P][Q][ldc] f32, n[P] taken from the t_bbox headers
 *   (n_from_header[b*R*4]) ; outputs tgt_for_pred [P][Q] int32 (-1 = unmatched prediction = the
 *   complement of the reference's bool selector) and pred_for_tgt [P][ldc] int32 (-1 padded).
 *   status[P]: 0 ok, 1 infeasible/NaN (the reference raises there). */
int detr_hip_assign_f32(const float *cost, int32_t P, int32_t Q, int32_t ldc, const float *t_bbox,
                        int32_t B, int32_t R, int32_t *tgt_for_pred, int32_t *pred_for_tgt,
                        int32_t *status, void *stream);
/* K14: loss.py:37-96.  Three steps so that data-parallel ranks can all-reduce `sums` in between:
 *   sums [levels][8] = {sum w*CE, -, n_neg_correct, n_neg, n_pos, n_pos_not_bg, n_pos_correct, -}
 *                      {.. [1], [7] unused ([1] stays 0 here; the *_crit_* entry points below keep the matched targets' class
 *                      weights in it): the normaliser sum w is derived as 0.1*n_neg + n_pos from the counts, which
 *                      float atomics accumulate exactly in any order -- the gradients are then a deterministic function
 *                      of the matching};  box sums [levels][2] are stored at sums + levels*8:
 *                      {sum L1, sum (1-GIoU)} ; all ACCUMULATED atomically (zero them first). */
int detr_hip_set_loss_sums_f32(const detr_setloss_desc *d, const int32_t *tgt_for_pred, float *sums,
                               void *stream);
/* losses [levels][6] = label_cost,true_neg,true_pos,pos_accuracy,giou_loss,l1_loss (loss.py:172-179);
 * total[0] = sum_lv 1*label + 2*giou + 5*l1 (loss.py:6-19) */
int detr_hip_set_loss_finalize_f32(const float *sums, int32_t levels, float *losses, float *total,
                                   void *stream);
/* gradients of loss_scale*total w.r.t. logits and boxes (same strides as the inputs) */
int detr_hip_set_loss_grad_f32(const detr_setloss_desc *d, const int32_t *tgt_for_pred, const float *sums,
                               float loss_scale, float *d_logits, float *d_boxes, void *stream);

/* The same four launches with a configurable criterion (appended; the ABI version is unchanged).  The four entry points above
 * run the reference's criterion, compiled in; these run the same kernel bodies on run-time values.  Per level, with N the
 * unmatched queries, M the matched pairs (q, j), w[c] = class_weights[c] (1 without class weights, and 1 for a label
 * outside [0, C)):
 *   cost[q][j]  = set_cost_bbox*L1 + set_cost_class*(-softmax[class_j]) + set_cost_giou*(-GIoU)
 *   W           = eos_coef*|N| + sum_M w[class_j]          (a matched target gets w[class_j] even when that is the background class)
 *   label_cost  = (eos_coef*sum_N CE(q, bg) + sum_M w[class_j]*CE(q, class_j)) / W
 *   npos'       = num_boxes_min_one ? max(|M|, 1) : |M| ;   l1_loss = sum_M |p - t|_1 / npos' ;   giou_loss = sum_M (1 - GIoU) / npos'
 *   total       = sum_lv class_loss_coef*label_cost + giou_loss_coef*giou_loss + bbox_loss_coef*l1_loss   (main level first)
 * losses[] stay unweighted; true_pos / pos_accuracy divide by |M| itself.  sums_crit accumulates sum_M w[class_j] into slot
 * [1] of a level's eight, and finalize_crit / grad_crit use W = eos_coef*sums[3] + sums[1]: callers keep class weights on
 * multiples of 1/64 in [0, 16] and world*B*(R-1) <= 16384, so that this float atomic sum is exact in any order and the
 * gradients stay a deterministic function of the matching.  At the reference's values the cost, the matching and the
 * gradients are bit-identical to the four entry points above.
 * criterion: DETR_CRITERION_FLOATS floats in HOST memory, read during the call:
 *   [0] set_cost_class [1] set_cost_bbox [2] set_cost_giou [3] class_loss_coef [4] bbox_loss_coef [5] giou_loss_coef
 *   [6] eos_coef [7] num_boxes_min_one (0 or 1).  class_weights: DEVICE float [C] or NULL (all 1).
 * Rejected on the host, before anything is launched: a null criterion, a value that is not finite or is negative, [7] other
 * than 0 or 1, and everything the entry points above reject. */
#define DETR_CRITERION_FLOATS 8
int detr_hip_match_cost_crit_f32(const detr_setloss_desc *d, const float *criterion, float *cost, void *stream);
int detr_hip_set_loss_sums_crit_f32(const detr_setloss_desc *d, const float *criterion, const float *class_weights,
                                    const int32_t *tgt_for_pred, float *sums, void *stream);
int detr_hip_set_loss_finalize_crit_f32(const float *sums, int32_t levels, const float *criterion, float *losses, float *total, void *stream);
int detr_hip_set_loss_grad_crit_f32(const detr_setloss_desc *d, const float *criterion, const float *class_weights,
                                    const int32_t *tgt_for_pred, const float *sums, float loss_scale,
                                    float *d_logits, float *d_boxes, void *stream);

/* The same four launches with a sigmoid focal class term (appended; the ABI version is unchanged): the *_crit_* signatures
 * with a `focal` block and without class weights.  The class head keeps its C logits, column background_class included, and no
 * column is special in the loss: a matched query is one-hot on its target's class, an unmatched one all zero.  With x a logit,
 * sp(z) = max(z, 0) + log1p(exp(-|z|)) and p = sigmoid(x), an element is
 *   t = 1:  pos(x) = alpha * exp(-gamma * sp(x)) * sp(-x)            (= alpha * (1 - p)^gamma * -log p)
 *   t = 0:  neg(x) = (1 - alpha) * exp(-gamma * sp(-x)) * sp(x)      (= (1 - alpha) * p^gamma * -log(1 - p))
 * finite for every finite logit.  Per level, with M the matched pairs:
 *   cost[q][j]  = set_cost_bbox*L1 + set_cost_class*(pos(x) - neg(x)) + set_cost_giou*(-GIoU),  x = logits[q][class_j]; a label
 *                 outside [0, C) costs 0 in the class term.  No 1e-8 is added inside a logarithm: this differs from the published
 *                 matcher only where p or 1 - p is below about 1e-6.
 *   label_cost  = (sum of all B*Q*C elements) / max(|M|, 1)          (always clamped; eos_coef is not read)
 *   l1_loss, giou_loss, total: as the *_crit_* entry points (the box sums follow num_boxes_min_one)
 *   metrics: a query predicts the background class when its largest non-background logit is <= 0, otherwise the first arg-max over
 *            c != background_class; true_neg, true_pos and pos_accuracy follow from that prediction as above.
 * sums: slot 0 = the sum of the elements, slot 1 stays 0, slots 2..6 the counts; finalize_focal / grad_focal normalise by
 * max(sums[4], 1), so the gradients are a deterministic function of the matching.  A matched label outside [0, C): the level's
 * label_cost (and the total) is NaN, the gradient that of a row without a positive class, nothing is read out of bounds.
 * focal: DETR_FOCAL_FLOATS floats in HOST memory, read during the call: [0] alpha in (0, 1), [1] gamma in [0, 8].
 * Rejected on the host, before anything is launched: a null focal block, a value outside its range or not finite, and
 * everything the *_crit_* entry points reject. */
#define DETR_FOCAL_FLOATS 2
int detr_hip_match_cost_focal_f32(const detr_setloss_desc *d, const float *criterion, const float *focal, float *cost, void *stream);
int detr_hip_set_loss_sums_focal_f32(const detr_setloss_desc *d, const float *criterion, const float *focal,
                                     const int32_t *tgt_for_pred, float *sums, void *stream);
int detr_hip_set_loss_finalize_focal_f32(const float *sums, int32_t levels, const float *criterion, const float *focal, float *losses,
                                         float *total, void *stream);
int detr_hip_set_loss_grad_focal_f32(const detr_setloss_desc *d, const float *criterion, const float *focal,
                                     const int32_t *tgt_for_pred, const float *sums, float loss_scale,
                                     float *d_logits, float *d_boxes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Device-side input stage (the step's producer side; detr_tf/data/processing.py:6-21,35-55, data/transformation.py:82-91).
 *   detr_hip_input_stage: uint8 NHWC batch -> fixed-size resize (cv2.resize semantics in fp32: half-pixel centres,
 *     replicated border, cubic a = -0.75; rounded + saturated back to uint8) -> normalisation through a [3][256] float
 *     lookup table the host builds in float64 exactly as `normalized_images` does (dst channel c = lut[c][src channel
 *     perm[c]]; "tf_resnet" = BGR order, perm {2,1,0}) -> float32 NHWC.
 *   detr_hip_pad_labels: ragged targets (boxes [N,4] cx,cy,w,h; classes [N]; offsets [B+1]) -> the reference's padded
 *     layout with the in-band header row: t_bbox [B,R,4] (row 0 = [n,0,0,0]), t_class [B,R] (row 0 = 0), zero padded.
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    int32_t B, Hs, Ws, Hd, Wd;
    const uint8_t *src; int64_t src_batch_stride;    /* bytes between images */
    float *dst;                                      /* [B, Hd, Wd, 3] */
    const float *lut;                                /* [3][256] */
    int32_t perm[3];
    int32_t interpolation;                           /* 0 nearest, 1 linear, 2 cubic (imgaug's Resize default) */
} detr_input_desc;
int detr_hip_input_stage(const detr_input_desc *d, void *stream);
/* Padded mixed-size batch (the reference's (images, masks) input, detr_tf/networks/detr.py:65-72): image b, [hw[2b], hw[2b+1], 3]
 * uint8 at src + offsets[b] (device arrays), is normalised through `lut` / `perm` (host array of 3) exactly as detr_hip_input_stage
 * does and written to the top-left of the float32 canvas dst [B, H, W, 3]; the rest of the canvas is 0.0 and mask [B, H, W] (uint8)
 * is 1 there (padding), 0 on valid pixels.  No resize.  Images larger than the canvas are cropped to it. */
int detr_hip_input_stage_padded(const uint8_t *src, const int64_t *offsets, const int32_t *hw, int32_t B, int32_t H, int32_t W,
                                const float *lut, const int32_t *perm, float *dst, uint8_t *mask, void *stream);
int detr_hip_pad_labels(const float *boxes, const int64_t *classes, const int32_t *offsets, int32_t B, int32_t R,
                        float *t_bbox, int64_t *t_class, void *stream);
/* Training augmentation (the reference's imgaug `detr_aug_seq`, data/transformation.py:54-94; csrc/augment.hip): image b of a
 * ragged uint8 batch, packed back to back in src (src_bytes bytes, device), goes through flip -> stage B -> final resize to
 * (Hd, Wd) and the normalisation of detr_hip_input_stage (lut / perm as there, perm a host array of 3) into dst [B, Hd, Wd, 3]
 * float32.  One launch.  Per-image records (device arrays):
 *   irec[b][DETR_AUG_IREC] int32: 0,1 byte offset of image b in src (low, high 32 bits); 2 h0; 3 w0; 4 flip (0/1);
 *     5 stage B: 0 none, 1 resize to (Hd, Wd), 2 crop to min(Hd, h0) x min(Wd, w0) at (8, 9), 3 affine zoom about the centre;
 *     6 stage-B resize interpolation; 7 final interpolation (0 nearest, 1 linear, 2 cubic, 3 area); 8 crop y0; 9 crop x0
 *   frec[b][DETR_AUG_FREC] float32: 0 1/sx, 1 1/sy (affine: source x = (x - cx) * (1/sx) + cx, cx = w0/2 - 0.5, bilinear,
 *     0 outside the image)
 * Stage B's output is rounded to uint8 before the final resize, as in imgaug.  Source reads are clamped into each image and
 * into src_bytes, so a wrong record cannot read outside src. */
#define DETR_AUG_IREC 10
#define DETR_AUG_FREC 2
int detr_hip_augment(const uint8_t *src, int64_t src_bytes, const int32_t *irec, const float *frec, int32_t B, int32_t Hd, int32_t Wd,
                     const float *lut, const int32_t *perm, float *dst, void *stream);
/* Aspect-preserving multi-scale input (csrc/augment_padded.hip): image b of a ragged uint8 batch, packed back to back in src
 * (src_bytes bytes, device), is flipped, windowed, resized to its own (hd, wd) with detr_hip_augment's resize formulas, normalised
 * through lut / perm (as detr_hip_input_stage; perm a host array of 3) and written at the top-left of the float32 canvas
 * dst [B, H, W, 3]; the rest of the canvas is 0.0 and mask [B, H, W] (uint8) is 1 there (padding), 0 on valid pixels.  One launch
 * for pixels and mask.  Per-image records (device array):
 *   irec[b][DETR_AUGP_IREC] int32: 0,1 byte offset of image b in src (low, high 32 bits); 2 h0; 3 w0; 4 flip (0/1);
 *     5 y0, 6 x0, 7 hc, 8 wc: the source window, in whole pixels of the flipped image; 9 hd, 10 wd: destination size;
 *     11 interpolation (0 nearest, 1 linear, 2 cubic, 3 area)
 * The window is clamped into the image, (hd, wd) to the canvas, and source reads into src_bytes, so a wrong record cannot read
 * outside src; writes depend on B, H, W only. */
#define DETR_AUGP_IREC 12
int detr_hip_augment_padded(const uint8_t *src, int64_t src_bytes, const int32_t *irec, int32_t B, int32_t H, int32_t W,
                            const float *lut, const int32_t *perm, float *dst, uint8_t *mask, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Batched post-processing (detr_tf/inference.py:68-95, which handles batch element 0 only; the validation loops call it
 * once per image, logger/training_logging.py:61-88, eval.py:41-55).  One launch for the whole batch: per query
 * score = max softmax probability, label = first arg-max of the probabilities; queries whose label is `background_class`
 * are dropped (order preserved); boxes converted (bbox.py:171-196: xyxy / yxyx are clipped to [0, 1]); the kept detections
 * of image b are written compacted to out_*[b][0 .. counts[b]).
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    int32_t B, Q, C;
    const float *logits; int64_t sL_b, sL_q;     /* [B, Q, C], unit class stride */
    const float *boxes;  int64_t sB_b, sB_q;     /* [B, Q, 4] cx, cy, w, h */
    int32_t background_class;
    int32_t bbox_format;                         /* 0 "xy_center", 1 "xyxy", 2 "yxyx" */
    float *out_boxes;                            /* [B, Q, 4] */
    int64_t *out_labels;                         /* [B, Q] */
    float *out_scores;                           /* [B, Q] */
    int32_t *counts;                             /* [B] */
} detr_postprocess_desc;
int detr_hip_postprocess(const detr_postprocess_desc *d, void *stream);
/* The same launch with the scoring as an argument (appended; the ABI version is unchanged).  scoring 0 "softmax": exactly
 * detr_hip_postprocess.  scoring 1 "sigmoid" (the class head of the focal criterion): label = first arg-max of the logits over
 * c != background_class, score = sigmoid of that logit = 1 / (1 + exp(-x)); every query is kept, so image b gets Q rows in query
 * order and counts[b] = Q.  A NaN among the non-background logits of a query makes its score NaN.  Rejected: C < 2 or a
 * background_class outside [0, C) with scoring 1, a scoring other than 0 or 1, and everything detr_hip_postprocess rejects. */
int detr_hip_postprocess_scored(const detr_postprocess_desc *d, int32_t scoring, void *stream);

/* ---------------------------------------------------------------------------------------------
 * mAP accumulation, per-image half (compute_map.py:183-272 cal_map, which eval.py:41-55 calls once per image on the host;
 * semantics pinned by detr_tf/loss/compute_map.py: APAccumulator.add_image).  One launch per batch, one workgroup per image
 * (csrc/map_match.hip).  Inputs: what detr_hip_postprocess wrote with bbox_format 2 ("yxyx") -- boxes / labels / scores, image b
 * at row b * sD_b, counts[b] of them -- and the padded targets as the loaders ship them: t_bbox [B, R, 4] cx, cy, w, h with the
 * header row 0 (t_bbox[b][0][0] = number of targets, data/processing.py:35-55), t_class [B, R, 1].
 * Outputs, for image b, in DESCENDING-SCORE order (stable: ties by position, i.e. np.argsort(-scores, kind="stable")):
 *   rec_score[b][r], rec_class[b][r], rec_flags[b][r] with bit t set = true positive at thresholds[t]: the detection took the
 *   unused same-class ground truth of largest IoU strictly above thresholds[t] (lowest index on ties; a ground truth is consumed
 *   per threshold; IoU in fp64 exactly as compute_overlaps, targets converted in fp32 with the clip to [0, 1]).  All Q slots are
 *   written: r >= counts[b] and skipped detections get rec_class -1, score 0, flags 0.
 *   num_gt[c] += ground truths of class c (integer atomics; the caller zeroes it once per evaluation).
 *   status |= DETR_MAP_BAD_*: a label or target class outside [0, nb_class) (that detection / ground truth is skipped), a header
 *   count outside [0, R-1] (the image is treated as having no targets), counts[b] outside [0, Q] (clamped).  Nothing is accessed
 *   out of bounds; the caller zeroes the word once and reads it with the records.
 * Limits: Q <= 1024, R <= 256, 1..DETR_MAP_MAX_THR finite thresholds; boxes 16-byte aligned.
 * ------------------------------------------------------------------------------------------- */
#define DETR_MAP_MAX_THR 16
#define DETR_MAP_BAD_LABEL 1
#define DETR_MAP_BAD_TARGET_CLASS 2
#define DETR_MAP_BAD_HEADER 4
#define DETR_MAP_BAD_COUNT 8
typedef struct {
    int32_t B, Q, R, nb_class, n_thr;
    const float *boxes;                          /* [B, Q, 4] y1, x1, y2, x2 */
    const int64_t *labels;                       /* [B, Q] */
    const float *scores;                         /* [B, Q] */
    const int32_t *counts;                       /* [B] */
    int64_t sD_b;                                /* rows between two images of boxes / labels / scores (>= Q) */
    const float *t_bbox;  int64_t sT_b;          /* [B, R, 4]; floats between two images (>= 4 R) */
    const int64_t *t_class; int64_t sC_b;        /* [B, R, 1]; elements between two images (>= R) */
    double thresholds[DETR_MAP_MAX_THR];
    float *rec_score;                            /* [B, Q] */
    int32_t *rec_class;                          /* [B, Q] */
    uint32_t *rec_flags;                         /* [B, Q] */
    int64_t *num_gt;                             /* [nb_class] */
    int32_t *status;                             /* [1] */
} detr_map_match_desc;
int detr_hip_map_match(const detr_map_match_desc *d, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Optimiser (detr_tf/optimizers.py:86-88,137-163): per-tensor clip-by-norm then Keras Adam on
 * a flat fp32 parameter buffer.  Tensor t occupies [seg_off[t], seg_off[t+1]) ; chunk c of
 * `chunk` elements belongs to tensor chunk_tensor[c] and starts at chunk_start[c].
 *   hyper (device, float[8]) = {lr_t group0, lr_t group1, lr_t group2, clipnorm, beta1, beta2, eps, -}
 *   with lr_t = lr*sqrt(1-b2^t)/(1-b1^t) computed by the host each step.
 *   sumsq [n_chunks]: sumsq_segments stores one partial per chunk; clip_adam sums the partials of a tensor (its chunks are
 *   consecutive) in a fixed order -- no atomics, so data-parallel replicas apply bit-identical updates.
 * ------------------------------------------------------------------------------------------- */
int detr_hip_sumsq_segments_f32(const float *g, const int32_t *chunk_tensor, const int64_t *chunk_start,
                                const int64_t *seg_end, int32_t n_chunks, int32_t chunk, float *sumsq,
                                void *stream);
int detr_hip_clip_adam_f32(float *param, const float *g, float *m, float *v, const int32_t *chunk_tensor,
                           const int64_t *chunk_start, const int64_t *seg_end, const int32_t *tensor_group,
                           const float *sumsq, const float *hyper, int32_t n_chunks, int32_t chunk,
                           void *stream);
/* dst[0..7] = v0..v7: the values travel as kernel arguments, so the host never has to
 * synchronise to update `hyper` (stream ordered, race free) */
int detr_hip_set_floats8_f32(float *dst, float v0, float v1, float v2, float v3, float v4, float v5, float v6,
                             float v7, void *stream);
/* acc[i] += a * g[i] (gradient accumulation optimizers.py:157) */
int detr_hip_axpy_f32(float *acc, const float *g, float a, int64_t n, void *stream);

/* ---------------------------------------------------------------------------------------------
 * AdamW (opt-in): decoupled weight decay, and the clip either per tensor (as above) or over ONE norm of every trained
 * tensor (tf.clip_by_global_norm).  Same chunk tables as above; one table may span all groups.
 *   hyper (device, float[16]) = {lr_t group0..2, clip, beta1, beta2, eps, weight_decay, lr group0..2,
 *                                trained group0..2 (1 or 0), -, -}
 *   per element:  g *= s;  m, v as Adam;  p -= lr*weight_decay*p;  p -= lr_t * m / (sqrt(v) + eps)
 * Joint sequence: detr_hip_sumsq_segments_f32 over the table, detr_hip_global_clip_scale_f32 (one workgroup sums the
 * partials of the trained groups in a fixed order: scale[0] = clip / max(G, clip), exactly 1 when G <= clip or clip <= 0;
 * scale[1] = G), detr_hip_adamw_f32 with that `scale`.  With scale == NULL detr_hip_adamw_f32 clips per tensor, like
 * detr_hip_clip_adam_f32.  Tensors of a group with trained == 0 (or tensor_group < 0) are neither counted nor touched.
 * ------------------------------------------------------------------------------------------- */
/* dst[0..15] = values[0..15] (values: HOST memory, read before the call returns; they travel as kernel arguments) */
int detr_hip_set_floats16_f32(float *dst, const float *values, void *stream);
int detr_hip_global_clip_scale_f32(const float *sumsq, const int32_t *chunk_tensor, const int32_t *tensor_group,
                                   const float *hyper, int32_t n_chunks, float *scale, void *stream);
int detr_hip_adamw_f32(float *param, const float *g, float *m, float *v, const int32_t *chunk_tensor,
                       const int64_t *chunk_start, const int64_t *seg_end, const int32_t *tensor_group,
                       const float *sumsq, const float *hyper, const float *scale, int32_t n_chunks, int32_t chunk,
                       void *stream);

/* ---------------------------------------------------------------------------------------------
 * Exponential moving average of the weights (opt-in; tf.train.ExponentialMovingAverage).  `shadow` is a second flat fp32
 * buffer laid out like `param`; the chunk tables are those of detr_hip_adamw_f32 (one table over all trained groups).
 *   hyper (device, float[>= 1]): hyper[0] = omd = 1 - decay of this step, read by the kernel (stream ordered after a
 *   detr_hip_set_floats8_f32 / detr_hip_set_floats16_f32 write, so a replayed launch sees the new value)
 *   per element of the listed chunks, TensorFlow's form, every operation rounded on its own (no fused multiply-add):
 *       t = shadow - param;  t = omd * t;  shadow = shadow - t
 * Reads param and shadow, writes shadow; elements no chunk lists are not touched.  Null operands, shadow == param and
 * n_chunks <= 0 or chunk <= 0 are rejected before any launch.
 * detr_hip_exchange_f32 swaps a[0, n) and b[0, n) element for element (the averaged weights in, the trained ones out, and
 * back: exact in both directions).  a == b and overlapping ranges are rejected; n may exceed 2^31 bytes.
 * ------------------------------------------------------------------------------------------- */
int detr_hip_ema_f32(float *shadow, const float *param, const int32_t *chunk_tensor, const int64_t *chunk_start,
                     const int64_t *seg_end, const float *hyper, int32_t n_chunks, int32_t chunk, void *stream);
int detr_hip_exchange_f32(float *a, float *b, int64_t n, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Scratch sizing: the number of bytes `workspace` must hold for the call described by the descriptor to take its
 * DETERMINISTIC split-reduction path (0 = the call needs no scratch; negative = malformed descriptor).  Pointers inside the
 * descriptor are not dereferenced; only shapes, split counts, dtypes and (gemm) whether rowsum_a is set are read.  The same
 * value is what a deferred reduction (detr_gemm_desc.defer_out / detr_layernorm_desc.defer_blocks_out) needs as its private slab. */
int64_t detr_hip_workspace_bytes_gemm(const detr_gemm_desc *d);
int64_t detr_hip_workspace_bytes_conv3x3(const detr_conv3x3_desc *d, int32_t mode);
int64_t detr_hip_workspace_bytes_stem(const detr_stem_desc *d, int32_t mode);
int64_t detr_hip_workspace_bytes_layernorm(const detr_layernorm_desc *d);

/* ---------------------------------------------------------------------------------------------
 * Tile plan of the 8-wave LDS-DMA "ring" GEMM (csrc/gemm_ring.h, round 5) that detr_hip_gemm_f32 takes for the tall unsplit
 * bf16 GEMMs (the K >= 512 1x1 convolutions of resnet_backbone.py:119-135 -- forward and input gradient -- and the FFN of
 * transformer.py:172-177): out[0..7] = {32-row blocks per wave, 32-column blocks per wave, ring stages, row pitch of the tile
 * grid, tiles along M, tiles along N, workgroups, LDS bytes}.  Returns 1 when the shape has a plan, 0 when it has none.  Pure
 * host arithmetic (tests, tuning scripts); `out` may be null. */
int detr_hip_gemm_ring_plan(int32_t M, int32_t N, int32_t K, int32_t *out);

/* ---------------------------------------------------------------------------------------------
 * Dilation-2 3x3 convolution, appended (the ABI version and detr_conv3x3_desc are unchanged):
 *   replaces: ZeroPadding2D(2) + Conv2D(3x3, dilation_rate=2) + FrozenBatchNorm2D + ReLU of the blocks >= 1 of a stage built with
 *             replace_stride_with_dilation (DETR-DC5), detr_tf/networks/resnet_backbone.py:74-85,98,104-105, and its gradients.
 * The fields of detr_conv3x3_desc with the same meaning -- modes 0 / 1 / 2, epilogue (alpha, scale, bias, residual, mask, act),
 * compute 0 / 1 / 2, bf16 storage flags, maskbits_out, split / workspace -- plus `dilation`.  Accepted: dilation == 2, stride == 1,
 * pad == 2, Ho == Hi, Wo == Wi; anything else is rejected with a message (detr_hip_last_error).  Tap (kh, kw) of output pixel (h, w)
 * reads input pixel (h - 2 + 2 kh, w - 2 + 2 kw).  bf16 tensors: modes 0 / 1 are one launch that walks the four pixel-parity planes
 * as dense convolutions (csrc/conv_dilated.hip); mode 2 reduces its row splits through `workspace` in a fixed order.
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    int32_t N, Hi, Wi, Ci, Ho, Wo, Co, stride, pad;
    const float *x;
    const float *w;
    float *y;
    float alpha;
    const float *scale;
    const float *bias;
    const float *residual;
    const float *mask;
    int32_t act;
    int32_t split;
    float *workspace; int64_t workspace_bytes;
    int32_t compute;
    int32_t w_dtype;
    int32_t x_dtype, y_dtype, r_dtype, m_dtype;
    uint8_t *maskbits_out;
    int32_t dilation;    /* 2 */
} detr_conv3x3d_desc;
int detr_hip_conv3x3_dilated(const detr_conv3x3d_desc *d, int32_t mode, void *stream);
int64_t detr_hip_workspace_bytes_conv3x3_dilated(const detr_conv3x3d_desc *d, int32_t mode);

/* ---------------------------------------------------------------------------------------------
 * Detections in pixel space, appended (the ABI version is unchanged):
 *   replaces: get_model_inference (detr_tf/inference.py:68-95) + the host-side numpy rescale of bbox.py:230-294 + the score
 *             threshold / ordering every caller adds (webcam_inference.py:26-34, eval.py:41-55).
 * One launch per batch, one workgroup per image (csrc/detect.hip), Q <= 1024.  Per query score = max softmax probability and
 * label = first arg-max, the very code of detr_hip_postprocess (bit-identical).  A query is kept when
 * label != background_class and score >= score_threshold; the kept queries are ordered by descending score, ties by ascending
 * query index (np.argsort(-score, kind="stable")), and cut to max_detections.  Boxes: (cx, cy, w, h) * (W_b, H_b, W_b, H_b) with
 * sizes[b] = (H_b, W_b) the ORIGINAL size of image b (the boxes of a padded batch are normalised per image, not per canvas), then
 *   bbox_format 0 "xy_center": cx, cy, w, h        (never clipped)
 *               1 "xyxy":      x0, y0, x1, y1      corners cx -+ w / 2, cy -+ h / 2
 *               2 "yxyx":      y0, x0, y1, x1
 *               3 "xywh":      x0, y0, x1 - x0, y1 - y0   (top-left + extent: the COCO results form)
 * clip = 1 clamps the corners of formats 1..3 to [0, W_b] x [0, H_b] (format 3 takes its extent from the clamped corners).
 * Outputs for image b at rows [b * max_detections, (b + 1) * max_detections): counts[b] detections, then zeros.  out_query is the
 * source query index (the row of an attention map).  No atomics: a rerun is bit-identical.  out_boxes 16-byte aligned.
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    int32_t B, Q, C;
    const float *logits; int64_t sL_b, sL_q;     /* [B, Q, C], unit class stride */
    const float *boxes;  int64_t sB_b, sB_q;     /* [B, Q, 4] cx, cy, w, h in [0, 1] */
    const int32_t *sizes;                        /* [B, 2] (height, width), DEVICE memory */
    int32_t background_class;
    float score_threshold;                       /* finite */
    int32_t max_detections;                      /* 1..Q */
    int32_t bbox_format;                         /* 0..3, above */
    int32_t clip;                                /* 0 | 1 */
    float *out_boxes;                            /* [B, max_detections, 4] */
    int64_t *out_labels;                         /* [B, max_detections] */
    float *out_scores;                           /* [B, max_detections] */
    int32_t *out_query;                          /* [B, max_detections] */
    int32_t *counts;                             /* [B] */
} detr_detect_desc;
int detr_hip_detect(const detr_detect_desc *d, void *stream);
/* The same launch with the scoring as an argument (appended; the ABI version is unchanged): scoring 0 is detr_hip_detect, scoring
 * 1 scores as detr_hip_postprocess_scored does (bit-identical) and makes every query a candidate: score >= score_threshold alone
 * decides (a NaN score fails it), then the ordering and the cut to max_detections as above.  Rejections as there. */
int detr_hip_detect_scored(const detr_detect_desc *d, int32_t scoring, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Multi-label detections under sigmoid scoring, appended (the ABI version is unchanged; no struct, no layout id): the K best of
 * an image's Q x (C - 1) (query, class) pairs, the rule of the detectors trained with a sigmoid focal class loss (Deformable
 * DETR's PostProcess and its successors).  One query may emit several classes; the number of detections is bounded by
 * max_detections, not by Q.
 *   replaces: sigmoid -> flatten -> topk -> gather over [B, Q * C] on the framework's side.
 * One launch per batch, one workgroup per image (csrc/detect_multilabel.hip), Q <= 1024.  Per image b:
 *   candidates: every pair (q, c), 0 <= q < Q, 0 <= c < C, c != background_class, with
 *     s = 1 / (1 + expf(-logits[b, q, c])) >= score_threshold -- the sigmoid of detr_hip_detect_scored (scoring 1): an element
 *     both score gets the same bits.  A NaN logit is never a candidate; -inf gives 0.0f, a candidate at score_threshold 0; +inf
 *     and every logit above about 17 give exactly 1.0f.
 *   order: descending s, exact ties by ascending flat index q * C + c: np.argsort(-s, kind="stable") over the flattened
 *     row-major [Q, C] scores with the non-candidates removed.  An exact radix select on the bits of s, then a sort of the
 *     survivors; no float atomics, a rerun is bit-identical.
 *   output: the first K = max_detections of that order; K is independent of Q and may exceed it.  out_labels = c, out_scores = s,
 *     out_query = q (it repeats where a query emits several classes), out_boxes = the box of query q; counts[b] =
 *     min(K, candidates); rows [counts[b], K) of every output are zero.
 * detr_hip_detect_multilabel: detr_detect_desc, UNCHANGED, every field with its meaning there except max_detections, which is
 *   1..1024 here, not 1..Q.  Boxes in pixels of the image's own size exactly as detr_hip_detect writes them for that query
 *   (bbox_format 0..3, clip).  Rejected before any launch: what detr_hip_detect_scored rejects with scoring 1 (null operands, bad
 *   shapes, strides, formats, clip, a non-finite threshold, an unaligned out_boxes, C < 2, background_class outside [0, C)), and
 *   max_detections outside 1..1024.
 * detr_hip_postprocess_multilabel: the same selection on detr_postprocess_desc, UNCHANGED, with out_boxes / out_labels /
 *   out_scores [B, max_detections(, 4)] and the boxes NORMALISED in detr_hip_postprocess's formats (0..2) and arithmetic -- the
 *   rows detr_hip_map_match and detr_hip_coco_match read, with Q = max_detections as their row capacity.  There is no out_query.
 *   Rejected: as above, on the fields this descriptor has; sL_q < C or other strides too small; an out_boxes that is not 16-byte
 *   aligned.
 * ------------------------------------------------------------------------------------------- */
int detr_hip_detect_multilabel(const detr_detect_desc *d, void *stream);
int detr_hip_postprocess_multilabel(const detr_postprocess_desc *d, int32_t max_detections, float score_threshold, void *stream);

/* ---------------------------------------------------------------------------------------------
 * COCO-protocol evaluation, per-image half, appended (the ABI version is unchanged):
 *   restates COCOeval's bbIou / evaluateImg for boxes (crowd regions, area ranges, ignore flags); the accumulate / summarize half
 *   is detr_tf/loss/coco_eval.py: COCOAccumulator.result.  One launch per batch, one workgroup per image (csrc/coco_match.hip).
 * Inputs: the detections and padded targets of detr_hip_map_match (same layout, conversion and clip), plus per target row
 * t_crowd[b][r] (iscrowd) and t_area[b][r] (the annotation's area in pixels^2 of the original image) -- rows line up with t_bbox,
 * row 0 (the header) is unused -- and sizes[b] = (H_b, W_b), the ORIGINAL size of image b.
 * Semantics, all in fp64 on the fp32 inputs (the file is compiled with -ffp-contract=off), boxes y1, x1, y2, x2 normalised:
 *   IoU(d, g): w = min(dx2, gx2) - max(dx1, gx1), h = min(dy2, gy2) - max(dy1, gy1); 0 unless w > 0 and h > 0; i = w * h;
 *     u = area_d when g is a crowd, else area_d + area_g - i (area = (x2 - x1) * (y2 - y1)); IoU = i / u.
 *   ignore(g, a) = t_crowd[g] or t_area[g] < lo_a or t_area[g] > hi_a, with area_ranges[2 a] = lo_a, area_ranges[2 a + 1] = hi_a.
 *   Detections are visited per class by descending score (stable, NaN last).  For every (area range a, threshold t) the bound starts
 *   at cur = min(thresholds[t], 1 - 1e-10).  Phase 1 walks the class's ground truths with ignore(g, a) false in index order, skips
 *   one already matched at (a, t), and takes g when IoU >= cur, then cur = IoU (non-strict: the LATER index wins ties).  Phase 2 runs
 *   only when phase 1 took nothing: the ground truths with ignore(g, a) true, in index order, skipping one already matched at (a, t)
 *   unless it is a crowd, same rule.  A match consumes g at (a, t).  The detection is `ignored` at (a, t) when it matched an ignored
 *   ground truth, or matched nothing and its pixel area ((y2 - y1) * H_b) * ((x2 - x1) * W_b) lies outside [lo_a, hi_a].
 * Outputs, for image b in visiting order (descending score over all classes, as detr_hip_map_match):
 *   rec_score[b][r], rec_class[b][r], rec_rank[b][r] = 0-based rank of the detection among the image's detections of its class,
 *   rec_flags[a][b][r]: bit t = matched at (a, t), bit 16 + t = ignored at (a, t).  All Q slots are written: r >= counts[b] and
 *   skipped detections get class -1, rank 0, flags 0 (a slot past counts[b] also score 0).
 *   npig[c][a] += ground truths of class c with ignore(g, a) false (integer atomics; the caller zeroes it once per evaluation).
 *   status |= DETR_MAP_BAD_* as detr_hip_map_match, DETR_COCO_BAD_SIZE for H_b <= 0 or W_b <= 0 (the size is used as it is: it only
 *   enters the pixel area).  Nothing is accessed out of bounds.  No float atomics: a rerun is bit-identical.
 * Limits: Q <= 1024, R <= 256, 1..DETR_COCO_MAX_THR finite thresholds, 1..DETR_COCO_MAX_AREA finite ranges lo <= hi; boxes 16-byte
 * aligned.
 * ------------------------------------------------------------------------------------------- */
#define DETR_COCO_MAX_THR 10
#define DETR_COCO_MAX_AREA 4
#define DETR_COCO_BAD_SIZE 16
typedef struct {
    int32_t B, Q, R, nb_class, n_thr, n_area;
    const float *boxes;                          /* [B, Q, 4] y1, x1, y2, x2 */
    const int64_t *labels;                       /* [B, Q] */
    const float *scores;                         /* [B, Q] */
    const int32_t *counts;                       /* [B] */
    int64_t sD_b;                                /* rows between two images of boxes / labels / scores (>= Q) */
    const float *t_bbox;  int64_t sT_b;          /* [B, R, 4]; floats between two images (>= 4 R) */
    const int64_t *t_class; int64_t sC_b;        /* [B, R, 1]; elements between two images (>= R) */
    const uint8_t *t_crowd;                      /* [B, R] */
    const float *t_area;                         /* [B, R] */
    int64_t sM_b;                                /* elements between two images of t_crowd / t_area (>= R) */
    const int32_t *sizes;                        /* [B, 2] (height, width), DEVICE memory */
    double thresholds[DETR_COCO_MAX_THR];
    double area_ranges[2 * DETR_COCO_MAX_AREA];
    float *rec_score;                            /* [B, Q] */
    int32_t *rec_class;                          /* [B, Q] */
    int32_t *rec_rank;                           /* [B, Q] */
    uint32_t *rec_flags;                         /* [n_area, B, Q] */
    int64_t *npig;                               /* [nb_class, n_area] */
    int32_t *status;                             /* [1] */
} detr_coco_match_desc;
int detr_hip_coco_match(const detr_coco_match_desc *d, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Cross-tile merge of sliced inference, appended (the ABI version is unchanged):
 *   replaces: the host loop a user of get_model_inference writes to run a model on overlapping windows of a large image -- boxes
 *             of every window mapped back to the image, sorted, duplicates removed by a class-wise greedy NMS.
 * One launch per batch, one workgroup per image (csrc/tile_merge.hip), Q <= 1024.  The N rows of logits / boxes are the tiles of
 * all B images, the tiles of image b at rows [tile_start[b], tile_start[b + 1]); windows[n] = (y0, x0, hc, wc) is tile n's window
 * in pixels of its image, sizes[b] = (H_b, W_b).  Per image, in this order:
 *   1. candidates: score / label per query as detr_hip_detect (bit-identical); kept when label != background_class and
 *      score >= score_threshold; ordered by (tile, query).
 *   2. mapping, every operation ONE fp32 rounding: cx = x0 + bx * wc, cy = y0 + by * hc, w = bw * wc, h = bh * hc, corners
 *      c -+ size * 0.5; clip = 1 clamps the corners to [0, W_b] x [0, H_b].  A window that is the whole image gives
 *      detr_hip_detect's bits.
 *   3. edge rule (edge_margin > 0): a candidate of a window that is not the whole image is dropped when an UNCLIPPED corner lies
 *      within edge_margin pixels of -- or beyond -- a window edge that is interior to the image: x_lo - x0 <= edge_margin with
 *      x0 > 0, (x0 + wc) - x_hi <= edge_margin with x0 + wc < W_b, and the same in y (differences in fp32).
 *   4. order: descending score, ties by lower tile, then lower query.
 *   5. greedy suppression in that order: a candidate is dropped when an earlier KEPT candidate of the same label (any label with
 *      class_agnostic) matches it by more than nms_threshold (strict).  The measure is fp64 on the fp32 corners of step 2:
 *      inter = max(0, min(x1) - max(x0)) * max(0, min(y1) - max(y0)), area = (x1 - x0) * (y1 - y0);
 *      match 0: inter / (area_i + area_j - inter), match 1: inter / min(area_i, area_j); a zero denominator gives 0.
 *   6. the first max_detections survivors are written at rows [b * max_detections, ...) in bbox_format (as detr_hip_detect;
 *      format 0 is cx, cy, w, h of step 2), with out_tile the tile's index within its image; counts[b] of them, then zeros.
 * An image with more than DETR_TILE_MAX_CAND candidates after step 3 sets DETR_TILE_OVER_CAP in *status (the caller zeroes it) and
 * gets counts[b] = 0 and zero rows; a device tile_start entry that is not monotone inside [0, N] sets DETR_TILE_BAD_START, same
 * outcome.  Nothing is accessed out of bounds.  No float atomics: a rerun is bit-identical.  out_boxes 16-byte aligned.
 * tile_start_host is the HOST copy of tile_start: it is what this entry point validates (monotone, [0] == 0, [B] == N).
 * ------------------------------------------------------------------------------------------- */
#define DETR_TILE_MAX_CAND 2048
#define DETR_TILE_OVER_CAP 1
#define DETR_TILE_BAD_START 2
typedef struct {
    int32_t B, N, Q, C;
    const float *logits; int64_t sL_b, sL_q;     /* [N, Q, C], unit class stride */
    const float *boxes;  int64_t sB_b, sB_q;     /* [N, Q, 4] cx, cy, w, h normalised to the tile */
    const int32_t *tile_start;                   /* [B + 1], DEVICE memory */
    const int32_t *tile_start_host;              /* [B + 1], HOST memory, the same values */
    const int32_t *windows;                      /* [N, 4] (y0, x0, hc, wc), DEVICE memory */
    const int32_t *sizes;                        /* [B, 2] (height, width), DEVICE memory */
    int32_t background_class;
    float score_threshold;                       /* finite */
    int32_t max_detections;                      /* 1..DETR_TILE_MAX_CAND */
    int32_t bbox_format;                         /* 0..3, as detr_detect_desc */
    int32_t clip;                                /* 0 | 1 */
    int32_t match;                               /* 0 IoU | 1 intersection over the smaller area */
    int32_t class_agnostic;                      /* 0 | 1 */
    float edge_margin;                           /* pixels, finite, >= 0 */
    double nms_threshold;                        /* finite */
    float *out_boxes;                            /* [B, max_detections, 4] */
    int64_t *out_labels;                         /* [B, max_detections] */
    float *out_scores;                           /* [B, max_detections] */
    int32_t *out_query;                          /* [B, max_detections] */
    int32_t *out_tile;                           /* [B, max_detections] */
    int32_t *counts;                             /* [B] */
    int32_t *status;                             /* [1] */
} detr_tile_merge_desc;
int detr_hip_tile_merge(const detr_tile_merge_desc *d, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Detections and attention heat maps drawn onto frames, appended (the ABI version is unchanged):
 *   replaces: numpy_bbox_to_image (detr_tf/inference.py:10-65) -- cv2.rectangle / cv2.putText per box on the host -- and the
 *             matplotlib overlay of an attention map the notebooks do.  Deviations: a bitmap font passed as an atlas, colours from a
 *             table, outlines that grow inwards.  Pixel parity with OpenCV is not claimed.
 * One call annotates a ragged batch of uint8 RGB frames in at most two launches (csrc/overlay.hip: a preparation launch, one workgroup
 * per image, writes an ordered command list into `workspace`; a raster launch, one workgroup per run of 1024 pixels, applies it), no
 * host synchronisation, no atomics except the integer OR on *status, vector stores only: a rerun is bit-identical.
 * Frames: image b is [H_b, W_b, 3] bytes at src + src_off[b] (any alignment) and is written to dst + dst_off[b] (any alignment; a
 *   4-byte aligned image is stored a dword at a time).  sizes[b] = (H_b, W_b) in DEVICE memory; sizes_host holds the same values in
 *   HOST memory and is what this entry point validates and sizes its grid with.  dst == src with dst_off == src_off is allowed: every
 *   output pixel depends on its own source pixel only.  Any other overlap of the two is the caller's error.
 * Detections: what detr_hip_detect / detr_hip_tile_merge write with bbox_format 1: boxes [B, D, 4] fp32 x0, y0, x1, y1 in pixels,
 *   labels [B, D] int64, scores [B, D] fp32 or NULL, counts [B] int32 (DEVICE; a value outside [0, D] is clamped and sets
 *   DETR_OVERLAY_BAD_COUNT in *status, which the caller zeroes).  D <= DETR_TILE_MAX_CAND.
 * Geometry, all integer: x1 = clamp(floor(bx0), 0, W - 1), x2 = clamp(floor(bx1), 0, W - 1), y1, y2 likewise with H.  A box with a
 *   non-finite corner, with bx1 < bx0 or by1 < by0, or with a negative label is skipped.  Paint order: descending integer area
 *   (x2 - x1) * (y2 - y1), ties by ascending detection index; the smallest box is painted last and ends up on top.
 * Per box, with t = thickness, s = clamp(scale[b], 1, DETR_OVERLAY_MAX_SCALE) and colour = colors[label % n_colors], in this order:
 *   1. interior tint: colour blended with fill_alpha over [x1, x2] x [y1, y2];
 *   2. label background: colour blended with label_alpha over the label rectangle;
 *   3. label text, opaque: black when 299 R + 587 G + 114 B >= 128000 for the colour, else white;
 *   4. outline, opaque colour: the pixels of [x1, x2] x [y1, y2] outside [x1 + t, x2 - t] x [y1 + t, y2 - t] (a box thinner than
 *      2 t is all outline; the outline never leaves the image).
 *   blend(c, p, a) = (c * a + p * (255 - a) + 127) / 255 in integers, per channel.
 * Label text: the glyph indices names[label][0 .. name_len[label]) when 0 <= label < n_names (name_len clamped to [0, name_cap]),
 *   then, with scores, glyph_colon (only behind a name) and d.dd: q = rint((double)score * 100.0) (half to even; the product is
 *   exact), clamped to [0, 999], NaN -> 0; the digits q / 100, glyph_dot, q / 10 % 10, q % 10, each digit as glyph_digit0 + digit.
 *   A label outside [0, n_names) without scores has no label rectangle.  Label rectangle: pad = t + s, width = n_chars * gw * s +
 *   2 pad, height = gh * s + 2 pad, origin (max(0, min(x1, W - width)), max(0, min(y1, H - height))), cut by the image; text origin =
 *   origin + (pad, pad).  Font: atlas [n_glyph, gh, gw] bytes, non-zero = ink, every font pixel an s x s block; a glyph index
 *   >= n_glyph draws nothing.
 * Heat map (all of heat, map_step, map_valid, map_scale, lut given, or none), applied to the source pixel before any box.  For pixel
 *   (y, x) of image b, with (sy, sx) = map_step[b], (vh, vw) = map_valid[b] clamped to [1, Hf] x [1, Wf], every fp32 operation
 *   rounded once, in this order (the file is compiled with -ffp-contract=off):
 *     fy = ((float)y + 0.5f) * sy - 0.5f; fy = min(max(fy, 0), (float)(vh - 1)); y0 = (int)floorf(fy); wy = fy - (float)y0;
 *     y1 = min(y0 + 1, vh - 1); the same in x;  m_rc = heat[b][y_r][x_c];
 *     top = m00 + wx * (m01 - m00); bot = m10 + wx * (m11 - m10); m = top + wy * (bot - top);
 *     v = m * map_scale[b]; v = v > 0 ? min(v, 1) : 0 (NaN -> 0);
 *     pixel = blend(lut[(int)(v * 255.0f + 0.5f)], pixel, (int)(v * (float)heat_alpha + 0.5f)).   v = 0 leaves the bytes unchanged.
 * workspace: detr_hip_workspace_bytes_overlay(d) bytes (reads B, D, name_cap only; negative = malformed), 16-byte aligned.
 * Limits: B 1..65535, D 1..DETR_TILE_MAX_CAND, H_b, W_b 1..DETR_OVERLAY_MAX_SIDE, thickness 1..DETR_OVERLAY_MAX_THICKNESS,
 *   gw, gh 1..DETR_OVERLAY_MAX_GLYPH, name_cap 1..DETR_OVERLAY_MAX_NAME, n_colors >= 1, n_glyph >= 1, alphas 0..255.
 * Nothing is read or written out of bounds for any label, score, count, glyph index or scale.
 * ------------------------------------------------------------------------------------------- */
#define DETR_OVERLAY_BAD_COUNT 1
#define DETR_OVERLAY_MAX_SCALE 64
#define DETR_OVERLAY_MAX_GLYPH 64
#define DETR_OVERLAY_MAX_NAME 251
#define DETR_OVERLAY_MAX_SIDE 32768
#define DETR_OVERLAY_MAX_THICKNESS 1024
typedef struct {
    int32_t B, D;
    const uint8_t *src;                          /* packed frames */
    const int64_t *src_off;                      /* [B] byte offsets, DEVICE memory */
    uint8_t *dst;
    const int64_t *dst_off;                      /* [B] byte offsets, DEVICE memory */
    const int32_t *sizes;                        /* [B, 2] (height, width), DEVICE memory */
    const int32_t *sizes_host;                   /* [B, 2], HOST memory, the same values */
    const float *boxes;                          /* [B, D, 4] x0, y0, x1, y1 in pixels */
    const int64_t *labels;                       /* [B, D] */
    const float *scores;                         /* [B, D] or NULL */
    const int32_t *counts;                       /* [B], DEVICE memory */
    int32_t thickness, label_alpha, fill_alpha;
    const uint8_t *colors;                       /* [n_colors, 3] */
    int32_t n_colors;
    const uint8_t *names;                        /* [n_names, name_cap] glyph indices (NULL with n_names == 0) */
    const int32_t *name_len;                     /* [n_names] */
    int32_t n_names, name_cap;
    const uint8_t *atlas;                        /* [n_glyph, gh, gw] */
    int32_t n_glyph, gh, gw;
    int32_t glyph_digit0, glyph_colon, glyph_dot;
    const int32_t *scale;                        /* [B], DEVICE memory */
    const float *heat;                           /* [B, Hf, Wf] or NULL */
    int64_t sH_b, sH_y, sH_x;                    /* its strides in elements */
    int32_t Hf, Wf;
    const float *map_step;                       /* [B, 2] (sy, sx), DEVICE memory */
    const int32_t *map_valid;                    /* [B, 2] (vh, vw), DEVICE memory */
    const float *map_scale;                      /* [B], DEVICE memory */
    const uint8_t *lut;                          /* [256, 3] */
    int32_t heat_alpha;
    void *workspace;
    int64_t workspace_bytes;
    int32_t *status;                             /* [1] */
} detr_overlay_desc;
int detr_hip_overlay(const detr_overlay_desc *d, void *stream);
int64_t detr_hip_workspace_bytes_overlay(const detr_overlay_desc *d);

/* ---------------------------------------------------------------------------------------------
 * Multi-object tracking across video frames, appended (the ABI version is unchanged):
 *   replaces: the host loop a user of the video program (webcam_inference.py:26-34) writes to tell that a detection of this frame is
 *             the object of the last one -- detections read back every frame, an O(tracks x detections) IoU association in NumPy.
 * One launch per batch of frames, one workgroup per video stream (csrc/track.hip); the tracks of a stream live in `state` on the
 * device, DETR_TRACK_MAX slots per stream.  A live slot holds x = (cx, cy, w, h) fp32 pixels, v = its change per frame, label, id >= 1,
 * hits, miss, confirmed and the last score; a free slot is all zeros (id 0).  The stream holds frame and next_id (1 in a fresh state).
 * Input of stream s: counts[s] <= D detections, boxes "xyxy" pixels (bbox_format 1 of detr_hip_detect / detr_hip_tile_merge), labels,
 * scores, optionally query, in the detector's order.  Every fp32 operation below is ONE rounding (no fused multiply-add); every IoU is
 * the fp64 measure of detr_hip_tile_merge with match 0 on fp32 corners.  Per stream with active[s] != 0, in this order:
 *   1. predict: for every live slot p = x + v; p.w, p.h below 0 become 0 (p.w < 0 ? 0 : p.w); corners p.c -+ p.size * 0.5f.
 *   2. detections: z = ((x0 + x1) * 0.5f, (y0 + y1) * 0.5f, x1 - x0, y1 - y0); `high` when score >= track_threshold, else `low`.
 *   3. stage 1: the pairs (live slot, high detection) of equal label (any label with class_agnostic) with
 *      IoU(corners of p, detection) > match_threshold (strict; a NaN IoU is no pair) are walked by descending IoU, ties by lower
 *      track id, then lower detection index; a pair is taken when both sides are still free.
 *   4. stage 2: the same walk with > low_match_threshold over the slots still unmatched that are confirmed and came into the frame
 *      with miss == 0, and the low detections.
 *   5. a matched slot: r = z - p; x = p + alpha * r; v = v + beta * r; hits += 1; miss = 0; score = the detection's;
 *      confirmed |= hits >= min_hits.  The label never changes.
 *   6. an unmatched slot: x = p; miss += 1; it is freed (zeroed) when it is not confirmed or miss > max_age.
 *   7. spawn: the unmatched high detections with score >= new_threshold, by ascending index, each take the lowest free slot (those of
 *      step 6 included): id = next_id++, x = z, v = 0, hits = 1, miss = 0, confirmed = (min_hits <= 1), label and score the
 *      detection's.  Without a free slot the detection is not tracked and DETR_TRACK_FULL is set in *status.
 *   8. emit, by ascending detection index: every detection matched to (or spawned as) a confirmed track -- box, label, score and
 *      query copied unchanged, plus the track's id and hits -- at rows [s * D, s * D + out_counts[s]); the rows behind are zero.
 *      frame += 1.
 * counts[s] outside [0, D] sets DETR_TRACK_BAD_COUNT and the stream is run with no detections.  active[s] == 0 leaves the state of
 * stream s untouched: out_counts[s] = 0 and zero rows.  The caller zeroes *status.  Nothing is accessed out of bounds for any input.
 * Integer atomics on *status only, no float atomics: a rerun from the same state is bit-identical.
 * state: detr_hip_track_state_bytes(S) bytes (negative: S outside 1..65535), 16-byte aligned; stream s at byte s * (that / S), as
 *   float x[DETR_TRACK_MAX][4]; float v[DETR_TRACK_MAX][4]; int64_t label[DETR_TRACK_MAX]; float score[DETR_TRACK_MAX];
 *   int32_t id[DETR_TRACK_MAX], hits[DETR_TRACK_MAX], miss[DETR_TRACK_MAX], confirmed[DETR_TRACK_MAX]; int32_t frame, next_id, pad[2].
 * Limits: S 1..65535, D 1..1024; thresholds, alpha, beta finite; max_age >= 0; min_hits >= 1; boxes, out_boxes, state 16-byte aligned.
 * detr_hip_struct_layout knows detr_track_desc as 400.
 * ------------------------------------------------------------------------------------------- */
#define DETR_TRACK_MAX 256
#define DETR_TRACK_FULL 1
#define DETR_TRACK_BAD_COUNT 2
typedef struct {
    int32_t S, D;
    void *state;                                 /* detr_hip_track_state_bytes(S) bytes, read and written */
    int64_t state_bytes;
    const float *boxes;                          /* [S, D, 4] x0, y0, x1, y1 in pixels */
    const int64_t *labels;                       /* [S, D] */
    const float *scores;                         /* [S, D] */
    const int32_t *query;                        /* [S, D] or NULL (emitted as 0) */
    const int32_t *counts;                       /* [S], DEVICE memory */
    const int32_t *active;                       /* [S], DEVICE memory */
    float track_threshold, new_threshold;        /* finite */
    double match_threshold, low_match_threshold; /* finite */
    int32_t max_age, min_hits;
    float alpha, beta;                           /* finite */
    int32_t class_agnostic;                      /* 0 | 1 */
    float *out_boxes;                            /* [S, D, 4] */
    int64_t *out_labels;                         /* [S, D] */
    float *out_scores;                           /* [S, D] */
    int32_t *out_query, *out_ids, *out_hits;     /* [S, D] */
    int32_t *out_counts;                         /* [S] */
    int32_t *status;                             /* [1] */
} detr_track_desc;
int detr_hip_track(const detr_track_desc *d, void *stream);
int64_t detr_hip_track_state_bytes(int32_t streams);

/* ---------------------------------------------------------------------------------------------
 * Tracking by appearance, appended (the ABI version is unchanged): detr_hip_track with an embedding per detection -- a fused
 * IoU / similarity cost in stage 1 and a re-identification stage for tracks that were lost (csrc/track_embed.hip; the kernel body is
 * the one of detr_hip_track, csrc/track_core.h).  Every field of detr_track_desc means what it means there; the steps 1..8 of
 * detr_hip_track stand, with the changes below.  Still one launch per batch of frames and one workgroup per stream.
 * Embeddings: embed is [S, R, E] fp32, row r of stream s at embed + s * sE_s + r * sE_r (strides in elements, sE_r >= E).  The RAW
 *   embedding f of detection d of stream s is row query[s, d], or row d with query == NULL.  Any tensor will do; the default source
 *   is the last decoder layer's hidden state of the model (DetrModel return_embeddings, E = 256, query = detr_hip_detect's out_query).
 * dot64(a, b) of two fp32 vectors of length E, in this order: lane partials p[l] = sum over j ascending of (double)a[l + 64 j] *
 *   (double)b[l + 64 j] for l = 0..63 (the products are exact in fp64), p[l] = 0 for l >= E; then for o = 32, 16, 8, 4, 2, 1:
 *   p[l] = p[l] + p[l ^ o] for all l at once.  Every lane ends with the same value, which is the result.
 * The unit embedding n of a detection: nrm = sqrt(dot64(f, f)) (fp64, correctly rounded), n[k] = (float)((double)f[k] / nrm); n is
 *   all zeros when nrm is 0 or not finite, or when the row index is outside [0, R).  The last two cases -- an index outside [0, R),
 *   a NaN or an infinity in the row -- set DETR_TRACK_BAD_EMBED in *status; they are looked for in all counts[s] detections of an
 *   active stream.  n is recomputed from f wherever it is needed.
 * The bank: embed_state holds float e[DETR_TRACK_MAX][E] per stream, the unit embedding of every slot (zeros for a free slot), in
 *   detr_hip_track_embed_state_bytes(S, E) bytes; it is a second state buffer next to `state`, whose layout is detr_hip_track's.
 *   sim(t, d) = dot64(e_t, n_d).
 * Per stream with active[s] != 0:
 *   3. stage 1 takes the same pairs by the same gate, IoU > match_threshold, but walks them by descending
 *      m = (1 - w) * IoU + w * sim(t, d), w = appearance_weight: fp64, (1 - w), the two products and the sum one rounding each; ties by
 *      lower track id, then lower detection index.  With w == 0 no similarity is computed and m is the IoU itself.  (A NaN m is no pair.)
 *   4. stage 2 is unchanged: IoU only.
 *   4b. with reid != 0, re-identification: the slots still unmatched that are confirmed and came into the frame with miss >= 1, against
 *      the high detections still unmatched with score >= new_threshold, of equal label (any label with class_agnostic), with
 *      sim(t, d) > reid_threshold (strict) and NO IoU gate, walked by descending sim, ties by lower id, then lower detection.
 *      A slot matched here takes x = z, v = 0, hits += 1, miss = 0, score = the detection's; its detection does not spawn (step 7) and
 *      is emitted with the slot's id (step 8).
 *   5..8 are unchanged for every other slot.  Then the bank: a slot matched in stage 1 or 4b, in fp32 with one rounding per operation,
 *      u[k] = momentum * e[k] + (1 - momentum) * n_d[k], then e[k] = (float)((double)u[k] / sqrt(dot64(u, u))) (zeros when that root
 *      is 0 or not finite); a slot matched in stage 2 keeps e; a spawned slot takes e = n_d; a freed slot is zeroed.
 * active[s] == 0 leaves both states of stream s untouched.  Nothing is read or written out of bounds for any count, query or embedding
 * value.  Integer atomics on *status only, no float atomics: a rerun from the same two states is bit-identical.
 * workspace: detr_hip_workspace_bytes_track_embed(d) bytes (reads S, D only; negative = malformed), 16-byte aligned: the fp64
 *   similarities [S][DETR_TRACK_MAX][D] of the pairs that pass a walk's gate, filled by whole waves before the walk.
 * Limits: those of detr_hip_track; R >= 1; E a multiple of 4 in 4..512; sE_r >= E, sE_s >= 0; embed, embed_state and workspace
 *   16-byte aligned; appearance_weight in [0, 1]; reid 0 or 1; reid_threshold finite; momentum in [0, 1].
 * detr_hip_struct_layout knows detr_track_embed_desc as 500.
 * ------------------------------------------------------------------------------------------- */
#define DETR_TRACK_BAD_EMBED 4
typedef struct {
    int32_t S, D;
    void *state;                                 /* detr_hip_track_state_bytes(S) bytes, read and written */
    int64_t state_bytes;
    const float *boxes;                          /* [S, D, 4] x0, y0, x1, y1 in pixels */
    const int64_t *labels;                       /* [S, D] */
    const float *scores;                         /* [S, D] */
    const int32_t *query;                        /* [S, D] or NULL (emitted as 0; the embedding of detection d is then row d) */
    const int32_t *counts;                       /* [S], DEVICE memory */
    const int32_t *active;                       /* [S], DEVICE memory */
    float track_threshold, new_threshold;        /* finite */
    double match_threshold, low_match_threshold; /* finite */
    int32_t max_age, min_hits;
    float alpha, beta;                           /* finite */
    int32_t class_agnostic;                      /* 0 | 1 */
    float *out_boxes;                            /* [S, D, 4] */
    int64_t *out_labels;                         /* [S, D] */
    float *out_scores;                           /* [S, D] */
    int32_t *out_query, *out_ids, *out_hits;     /* [S, D] */
    int32_t *out_counts;                         /* [S] */
    int32_t *status;                             /* [1] */
    const float *embed;                          /* [S, R, E] */
    int64_t sE_s, sE_r;                          /* its stream and row strides in elements */
    int32_t R, E;
    void *embed_state;                           /* detr_hip_track_embed_state_bytes(S, E) bytes, read and written */
    int64_t embed_state_bytes;
    void *workspace;
    int64_t workspace_bytes;
    double appearance_weight;                    /* in [0, 1] */
    int32_t reid;                                /* 0 | 1 */
    double reid_threshold;                       /* finite */
    float momentum;                              /* in [0, 1] */
} detr_track_embed_desc;
int detr_hip_track_embed(const detr_track_embed_desc *d, void *stream);
int64_t detr_hip_track_embed_state_bytes(int32_t streams, int32_t embed_dim);
int64_t detr_hip_workspace_bytes_track_embed(const detr_track_embed_desc *d);

/* ---------------------------------------------------------------------------------------------
 * Camera-motion compensation for the trackers, appended (the ABI version is unchanged): a global translation per stream and frame,
 * estimated from the frames themselves and added to the track positions BEFORE detr_hip_track / detr_hip_track_embed run on the same
 * `state` (csrc/track_motion.hip).  A hand-held or vehicle-mounted camera moves every box by tens of pixels between two frames;
 * the alpha-beta velocity cannot learn jitter, so every IoU gate fails at once.  Three launches on the caller's stream (thumbnail:
 * one workgroup per stream and thumbnail row; block matching: one workgroup per stream and block; finalise: one workgroup per
 * stream), no read-back, no host synchronisation.  All arithmetic up to the shift is integer: the result is exact, and a rerun from
 * the same states is bit-identical.  Translation only -- zoom and roll are not modelled --, quantised to f pixels (f = 4 for
 * 800 x 1333, 5 for 1080p); the alpha-beta update of the tracker absorbs the remainder.
 * Frames: stream s is [h, w, 3] uint8 RGB at frames + offsets[s] (any alignment), (h, w) = sizes[s], both in DEVICE memory.  A side
 *   outside 1..DETR_OVERLAY_MAX_SIDE, a negative offset or offsets[s] + 3 h w > frames_bytes sets DETR_TRACK_BAD_FRAME in *status (which
 *   the caller zeroes; the bit is apart from detr_hip_track's, so the word may be shared), and the stream is run as (h, w) = (0, 0):
 *   no pixel is read, there is no estimate.
 * With SIDE = DETR_MOTION_SIDE, R = radius, per stream with active[s] != 0:
 *   1. thumbnail: f = max(1, ceil(w / SIDE), ceil(h / SIDE)), tw = w / f, th = h / f (integer division; the partial right and bottom
 *      edges are dropped).  Luma y = (77 R + 150 G + 29 B + 128) >> 8; thumbnail pixel (j, i) = (sum of y over its f x f cell) / (f f),
 *      integer division, stored as uint8 into thumb[1 - slot] (slot = the header's: where the previous frame's thumbnail is), dense with
 *      row stride tw; the bytes behind th * tw keep what they held.
 *   2. whether an estimate exists: none when the header's valid is 0 (the first frame after a reset), when (h, w) differs from the
 *      header's, or when gx = (tw - 2 R) / 16 < 1 or gy = (th - 2 R) / 16 < 1 (tw == 0 and th == 0 fall under this).
 *   3. block votes: block (bx, by), bx < gx, by < gy, is the 16 x 16 window of the current thumbnail at (R + 16 bx, R + 16 by); it is
 *      valid when max - min of its pixels is >= DETR_MOTION_MIN_CONTRAST.  For every (dx, dy) in [-R, R]^2,
 *      SAD = sum over the window of |cur(x, y) - prev(x - dx, y - dy)|; the block's vote is the displacement with the smallest key
 *      (SAD, dx dx + dy dy, dy, dx), compared lexicographically.
 *   4. global shift: n = number of valid blocks; no estimate when n < DETR_MOTION_MIN_BLOCKS.  dx*, dy* = the lower medians of the
 *      votes' dx and of their dy, taken independently (index (n - 1) / 2 of the sorted list); agree = number of valid blocks with
 *      |dx - dx*| <= 1 and |dy - dy*| <= 1; no estimate when 2 agree < n (a scene cut, or a frame dominated by moving foreground).
 *      (sx, sy) = (dx* f, dy* f) pixels.
 *   5. apply: with an estimate, every live slot (id >= 1) of the stream's track state gets x.cx = x.cx + (float)sx and
 *      x.cy = x.cy + (float)sy, one fp32 rounding each; v, w, h and the free slots are not touched.
 *   6. book-keeping, with or without an estimate: the header takes the new h, w, f, tw, th, valid = 1, slot = 1 - slot, and
 *      estimated, sx, sy, n, agree as reported.  out_motion[s] = (estimated, sx, sy, n, agree, f): sx = sy = 0 without an estimate;
 *      n = agree = 0 when step 2 found none; agree = 0 when n < DETR_MOTION_MIN_BLOCKS.
 * active[s] == 0 leaves the motion state and the track state of stream s untouched: out_motion[s] is six zeros.
 * motion_state: detr_hip_track_motion_state_bytes(S) bytes (negative: S outside 1..65535), 16-byte aligned; per stream
 *   int32_t head[16] = h, w, f, tw, th, valid, slot, estimated, sx, sy, n, agree, 0, 0, 0, 0; uint8_t thumb[2][SIDE * SIDE].
 *   A fresh state is all zeros.
 * state: the track state of detr_hip_track.  workspace: detr_hip_workspace_bytes_track_motion(d) bytes (reads S only; negative =
 *   malformed), 16-byte aligned: the votes.
 * Limits: S 1..65535; radius 1..16; frames_bytes >= 1; motion_state, state and workspace 16-byte aligned, offsets 8-byte aligned.
 * No float atomics; integer atomics on *status and inside a workgroup's LDS only.  Nothing is read or written out of bounds for any
 * size or offset.  detr_hip_struct_layout knows detr_track_motion_desc as 600.
 * ------------------------------------------------------------------------------------------- */
#define DETR_MOTION_SIDE 384
#define DETR_MOTION_BLOCK 16
#define DETR_MOTION_MIN_BLOCKS 4
#define DETR_MOTION_MIN_CONTRAST 16
#define DETR_MOTION_MAX_RADIUS 16
#define DETR_TRACK_BAD_FRAME 8
typedef struct {
    int32_t S;
    const uint8_t *frames;                       /* base of the frames */
    int64_t frames_bytes;                        /* bytes readable behind it */
    const int64_t *offsets;                      /* [S] byte offsets, DEVICE memory */
    const int32_t *sizes;                        /* [S, 2] (height, width), DEVICE memory */
    const int32_t *active;                       /* [S], DEVICE memory */
    int32_t radius;                              /* 1..DETR_MOTION_MAX_RADIUS */
    void *motion_state;                          /* detr_hip_track_motion_state_bytes(S) bytes, read and written */
    int64_t motion_state_bytes;
    void *state;                                 /* detr_hip_track_state_bytes(S) bytes, read and written */
    int64_t state_bytes;
    void *workspace;
    int64_t workspace_bytes;
    int32_t *out_motion;                         /* [S, 6] estimated, sx, sy, n, agree, f */
    int32_t *status;                             /* [1] */
} detr_track_motion_desc;
int detr_hip_track_motion(const detr_track_motion_desc *d, void *stream);
int64_t detr_hip_track_motion_state_bytes(int32_t streams);
int64_t detr_hip_workspace_bytes_track_motion(const detr_track_motion_desc *d);

/* ---------------------------------------------------------------------------------------------
 * Fusion of the detections of several VIEWS of an image (test-time augmentation), appended (the ABI version is unchanged):
 *   replaces: the host loop a user of get_model_inference writes to run a model on the mirrored image and / or at several shortest
 *             sides and to combine the V x Q rows -- hard NMS, soft-NMS (Bodla et al. 2017) or weighted box fusion (Solovyev et al.
 *             2021), each a sequential algorithm.
 * One launch per batch, one workgroup per image (csrc/fuse_views.hip).  The descriptor is detr_tile_merge_desc, UNCHANGED, every
 * field with its meaning there (a "tile" is a view; nms_threshold is the match threshold of every method, compared strictly); no
 * struct, no layout id.  view_flip[n] != 0 says that view n saw the MIRRORED image: its window is a window of the mirrored image
 * (flip, then window -- the rule of detr_hip_augment_padded).  fuse[] is read on the host during the call:
 *   [0] method: 0 hard NMS, 1 soft-NMS linear, 2 soft-NMS Gaussian, 3 weighted box fusion
 *   [1] sigma (method 2, > 0)          [2] score_min (methods 1, 2, >= 0)
 *   [3] expected_views (method 3; 0 = no rescaling, otherwise an integer >= 1)      [4] min_members (method 3, integer >= 1)
 *   [5] reserved, 0
 * Per image:
 *   1..4. candidates, mapping, edge rule and order are detr_hip_tile_merge's steps 1..4, the same code.  The one addition: for a
 *      flipped view the mapping and the edge rule run in the view's own, mirrored frame; then the UNCLIPPED corners are mirrored,
 *      (x0, x1) <- (W_b - x1, W_b - x0), one fp32 rounding each; the clip follows the mirror.
 *   5. method 0: detr_hip_tile_merge's step 5.  With no flipped view and bbox_format 1..3 every output equals detr_hip_tile_merge's
 *      bit for bit.
 *      methods 1, 2 (soft-NMS): current scores in fp64, initialised from the fp32 scores; every candidate starts alive.  Repeat:
 *      select the alive candidate with the largest current score (ties: lower position, i.e. lower view, then lower query; a NaN
 *      score is never selected); stop when there is none or max_detections are emitted; emit it with score (float)current, it
 *      dies; for every alive candidate j of its label (any label with class_agnostic) m = measure(selected, j) (step 5's fp64
 *      measure): method 1: if m > nms_threshold, s_j <- s_j * (1.0 - m); method 2: s_j <- s_j * exp(-(m * m) / sigma) for every m;
 *      then j dies if s_j < score_min (whether or not s_j changed).  fp64, one rounding per operation; exp is the device's
 *      double-precision exp (method 2's scores are exact up to its last bit; exp(-0) = 1 leaves a score's bits alone).
 *      method 3 (weighted box fusion): walk the candidates in the order of step 4.  Clusters are kept in creation order; a
 *      cluster's label is its first member's.  For a candidate (score s, corners x_c) take the clusters of its label (all with
 *      class_agnostic), m_k = measure(fused_k, box); the largest m_k wins, ties to the lower cluster (NaN never wins).  If that
 *      m_k > nms_threshold the candidate joins cluster k: sw += s; sx[c] += s * x_c; cnt += 1; fused_c = (float)(sx[c] / sw) --
 *      fp64, every product, sum and quotient one rounding.  Otherwise it founds a cluster: sw = s, sx[c] = s * x_c, cnt = 1,
 *      fused = its own corners (copied), founder = its (view, query).  After the walk, which visits ALL candidates:
 *      conf = sw / cnt; with expected_views = E > 0, conf = conf * min(cnt, E) / E, left to right; score = (float)conf; clusters
 *      with cnt < min_members are dropped; the rest are ordered by descending score, ties by lower cluster.
 *   6. the first max_detections rows are written as detr_hip_tile_merge writes them, with two differences: bbox_format 0 is
 *      derived from the final corners for EVERY method, ((x0 + x1) * 0.5, (y0 + y1) * 0.5, x1 - x0, y1 - y0), single fp32
 *      roundings; and out_members[row] = 1 (methods 0..2) or cnt, with out_query / out_tile the founder's (method 3).  counts[b]
 *      rows, then zeros (out_members too).
 * Status: DETR_TILE_OVER_CAP and DETR_TILE_BAD_START as detr_hip_tile_merge; method 3 holds at most DETR_FUSE_MAX_CLUSTERS clusters
 * per image: one that would found more sets DETR_FUSE_OVER_CLUSTERS and gets counts[b] = 0 and zero rows.  Nothing is truncated
 * silently; nothing is accessed out of bounds.  No float atomics: a rerun is bit-identical.
 * Rejected before any launch: everything detr_hip_tile_merge rejects; null fuse or out_members; a non-finite fuse[] value; an
 * unknown method; a non-integral or out-of-range [3] or [4]; sigma <= 0 with method 2; score_min < 0 with methods 1, 2; [5] != 0.
 * ------------------------------------------------------------------------------------------- */
#define DETR_FUSE_PARAMS 6
#define DETR_FUSE_MAX_CLUSTERS 1024
#define DETR_FUSE_OVER_CLUSTERS 4
int detr_hip_fuse_views(const detr_tile_merge_desc *d,
                        const int32_t *view_flip,   /* DEVICE [N], 0 | 1, or NULL = none flipped */
                        const double  *fuse,        /* HOST [DETR_FUSE_PARAMS], read during the call */
                        int32_t       *out_members, /* DEVICE [B, max_detections] */
                        void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DETR_HIP_H */

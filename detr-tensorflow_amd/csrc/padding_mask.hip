// padding_mask.hip -- padded mixed-size batches: the image-level padding mask (True = padding, detr_tf/networks/detr.py:65-72)
// brought to the feature map and turned into what the transformer consumes, and the padded input canvas.
//   * detr_hip_padding_mask_prepare: per image, TF-legacy nearest downsampling of the mask (downsample_masks, detr.py:57-63;
//     resize_nearest_neighbor with align_corners = half_pixel_centers = False: src = min(floor(dst * in / out), in - 1)), the
//     key-validity words of the masked attention kernels, the per-image sine positional encoding (position_embeddings.py:23-50,
//     normalize=True) and a status word (1 = the image has no valid feature position; the reference would produce NaN there).
//     The encoding of a position depends only on (cumulative count c, axis total n) of its column (y) and row (x): the host
//     builds sin / cos tables [n][c][128] per axis once per feature size with the float32 NumPy expressions of
//     engine.position_embedding_sine_host, and the kernel gathers -- an all-False mask reproduces the unmasked constant bit for bit.
//   * detr_hip_input_stage_padded: ragged uint8 images -> zero-padded float32 NHWC canvas + its mask, one launch, valid pixels
//     through the normalisation table of detr_hip_input_stage (image_resample.h: lut_pixel; no resize: that stays the caller's job,
//     as in the reference).
// Everything runs on the device: a masked step adds no host synchronisation, and a captured graph re-reads the mask buffer.
#include "image_resample.h"

namespace detr {

constexpr int PM_MAX_SIDE = 128;         // feature-map sides up to 128 (counts fit a byte; 800 x 1333 gives 25 x 42)
constexpr int PM_MAX_L = 8192;           // feature positions per image

struct PadMaskArgs {
    const unsigned char *mask;           // [B, H, W], nonzero = padding
    int B, H, W, Hf, Wf, kv_words;
    const float *tab_y, *tab_x;          // [Hf + 1][Hf + 1][128], [Wf + 1][Wf + 1][128]
    uint32_t *key_valid;                 // [B][kv_words]
    float *pos;                          // [B * Hf * Wf, 256]
    int *status;                         // [B]
};

// one workgroup per image
__global__ __launch_bounds__(256) void padding_mask_prepare_kernel(PadMaskArgs a) {
    __shared__ unsigned char valid[PM_MAX_L], cy[PM_MAX_L], cx[PM_MAX_L];
    __shared__ unsigned char ny[PM_MAX_SIDE], nx[PM_MAX_SIDE];
    __shared__ int any;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int L = a.Hf * a.Wf;
    const unsigned char *m = a.mask + (long long)b * a.H * a.W;
    if (tid == 0) any = 0;
    __syncthreads();
    for (int l = tid; l < L; l += blockDim.x) {
        const int i = l / a.Wf, j = l % a.Wf;
        const int sy = min((int)(((long long)i * a.H) / a.Hf), a.H - 1), sx = min((int)(((long long)j * a.W) / a.Wf), a.W - 1);
        const unsigned char v = m[(long long)sy * a.W + sx] ? 0 : 1;
        valid[l] = v;
        if (v) any = 1;
    }
    __syncthreads();
    // cumulative counts: one thread per column (y) / per row (x)
    for (int j = tid; j < a.Wf; j += blockDim.x) {
        int c = 0;
        for (int i = 0; i < a.Hf; ++i) { c += valid[i * a.Wf + j]; cy[i * a.Wf + j] = (unsigned char)c; }
        ny[j] = (unsigned char)c;
    }
    for (int i = tid; i < a.Hf; i += blockDim.x) {
        int c = 0;
        for (int j = 0; j < a.Wf; ++j) { c += valid[i * a.Wf + j]; cx[i * a.Wf + j] = (unsigned char)c; }
        nx[i] = (unsigned char)c;
    }
    for (int t = tid; t < a.kv_words; t += blockDim.x) {
        uint32_t w = 0;
        for (int j = 0; j < 32; ++j) {
            const int l = 32 * t + j;
            if (l < L && valid[l]) w |= 1u << j;
        }
        a.key_valid[(long long)b * a.kv_words + t] = w;
    }
    if (tid == 0) a.status[b] = any ? 0 : 1;
    __syncthreads();
    // pos[b, l, 0:128] = tab_y[ny(col)][cy(l)], pos[b, l, 128:256] = tab_x[nx(row)][cx(l)]: one float4 per thread and step
    const int Hs = a.Hf + 1, Ws = a.Wf + 1;
    float4 *out = reinterpret_cast<float4 *>(a.pos + (long long)b * L * 256);
    for (int u = tid; u < L * 64; u += blockDim.x) {
        const int l = u >> 6, q = u & 63;
        const int i = l / a.Wf, j = l % a.Wf;
        const float4 *src = q < 32 ? reinterpret_cast<const float4 *>(a.tab_y + ((long long)ny[j] * Hs + cy[l]) * 128) + q
                                   : reinterpret_cast<const float4 *>(a.tab_x + ((long long)nx[i] * Ws + cx[l]) * 128) + (q - 32);
        out[u] = *src;
    }
}

struct PadInputArgs {
    const unsigned char *src;            // packed images, image b at src + offsets[b]: [h_b, w_b, 3] uint8
    const long long *offsets;            // [B] byte offsets
    const int *hw;                       // [B][2] = (h_b, w_b)
    float *dst;                          // [B, H, W, 3]
    unsigned char *mask;                 // [B, H, W]: 1 = padding
    const float *lut;                    // [3][256]
    int B, H, W, perm0, perm1, perm2;
};

__global__ __launch_bounds__(256) void input_stage_padded_kernel(PadInputArgs a) {
    const long long total = (long long)a.B * a.H * a.W;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int x = (int)(i % a.W);
        const long long t = i / a.W;
        const int y = (int)(t % a.H), b = (int)(t / a.H);
        const int h = a.hw[2 * b], w = a.hw[2 * b + 1];
        float *o = a.dst + i * 3;
        if (y < h && x < w) {
            const unsigned char *p = a.src + a.offsets[b] + ((long long)y * w + x) * 3;
            const int v[3] = {p[0], p[1], p[2]};
            lut_pixel(a.lut, a.perm0, a.perm1, a.perm2, v, o);
            a.mask[i] = 0;
        } else {
            o[0] = 0.0f; o[1] = 0.0f; o[2] = 0.0f;
            a.mask[i] = 1;
        }
    }
}

}  // namespace detr

using namespace detr;

extern "C" int detr_hip_padding_mask_prepare(const uint8_t *mask, int32_t B, int32_t H, int32_t W, int32_t Hf, int32_t Wf,
                                             const float *tab_y, const float *tab_x, uint32_t *key_valid, float *pos, int32_t *status,
                                             void *stream) {
    DETR_REQUIRE(mask && tab_y && tab_x && key_valid && pos && status, "padding_mask_prepare: null operand");
    DETR_REQUIRE(B > 0 && H > 0 && W > 0 && Hf > 0 && Wf > 0, "padding_mask_prepare: bad shape B=%d H=%d W=%d Hf=%d Wf=%d", B, H, W, Hf, Wf);
    DETR_REQUIRE(Hf <= PM_MAX_SIDE && Wf <= PM_MAX_SIDE && Hf * Wf <= PM_MAX_L,
                 "padding_mask_prepare: feature map %d x %d exceeds %d per side / %d positions", Hf, Wf, PM_MAX_SIDE, PM_MAX_L);
    DETR_REQUIRE(aligned16(tab_y) && aligned16(tab_x) && aligned16(pos), "padding_mask_prepare: tables and pos must be 16-byte aligned");
    DETR_REQUIRE(((uintptr_t)key_valid & 3) == 0 && ((uintptr_t)status & 3) == 0, "padding_mask_prepare: key_valid / status must be 4-byte aligned");
    PadMaskArgs a;
    a.mask = mask; a.B = B; a.H = H; a.W = W; a.Hf = Hf; a.Wf = Wf; a.kv_words = cdiv(Hf * Wf, 32);
    a.tab_y = tab_y; a.tab_x = tab_x; a.key_valid = key_valid; a.pos = pos; a.status = status;
    hipLaunchKernelGGL(padding_mask_prepare_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, a);
    DETR_LAUNCH_CHECK("padding_mask_prepare");
    return 0;
}

extern "C" int detr_hip_input_stage_padded(const uint8_t *src, const int64_t *offsets, const int32_t *hw, int32_t B, int32_t H, int32_t W,
                                           const float *lut, const int32_t *perm, float *dst, uint8_t *mask, void *stream) {
    DETR_REQUIRE(src && offsets && hw && lut && perm && dst && mask, "input_stage_padded: null operand");
    DETR_REQUIRE(B > 0 && H > 0 && W > 0, "input_stage_padded: bad shape B=%d H=%d W=%d", B, H, W);
    DETR_REQUIRE(check_perm(perm), "input_stage_padded: channel permutation out of range");
    PadInputArgs a;
    a.src = src; a.offsets = reinterpret_cast<const long long *>(offsets); a.hw = hw; a.dst = dst; a.mask = mask; a.lut = lut;
    a.B = B; a.H = H; a.W = W; a.perm0 = perm[0]; a.perm1 = perm[1]; a.perm2 = perm[2];
    const long long total = (long long)B * H * W;
    hipLaunchKernelGGL(input_stage_padded_kernel, dim3(capped_grid(total, 256, 16384)), dim3(256), 0, (hipStream_t)stream, a);
    DETR_LAUNCH_CHECK("input_stage_padded");
    return 0;
}

// augment_padded.hip -- aspect-preserving multi-scale input on the device: a ragged batch of uint8 images (each at its own
// size) -> the zero-padded float32 NHWC canvas [B, H, W, 3] and its padding mask [B, H, W] (1 = padding), one launch.  This is
// the input DETR is trained and evaluated with (random shortest side 480..800 / shortest side 800, longest side <= 1333,
// random-size crop; the reference names the constants in data/transformation.py:59-64 and keeps the evaluation rule as
// commented-out code in :96-112).  The host only draws one record per image (detr_tf/data/transformation.py:
// draw_multiscale / eval_record); the kernel applies it:
//   F  horizontal flip (exact index mirror),
//   W  the window (y0, x0, hc, wc) of F, in whole source pixels,
//   R  resize of the window to (hd, wd) by image_resample.h's resample() (as augment.hip and input_stage.hip; result rounded
//      and saturated to uint8), then the normalisation table of detr_hip_input_stage,
// written at the canvas's top-left; every canvas pixel outside hd x wd is 0.0f with mask 1, inside the mask is 0.  The resized
// images never exist on the host and no intermediate image is written to HBM.
//
// Bound: the floor is the canvas write, 12 B of pixels + 1 B of mask per canvas pixel (the uint8 source is at most a quarter
// of that).  Measured (B = 8, 480 x 640 -> 800 x 1066 on an 800 x 1344 canvas, bilinear): 58 us against 26 us for a device
// copy of the same bytes and 66 us for augment_kernel writing 800 x 1344; the padding part runs at the copy's rate, the valid
// part is bound by the byte gather (4 to 16 taps of three byte loads per pixel), as in augment_kernel (NOTEBOOK 12).  One lane
// owns AUG_PIX = 4 consecutive pixels of a canvas row-major run: three 16-byte pixel stores and one 4-byte mask store.
//
// Safety (augment.hip's rule): every source index is clamped into its own window and image, a record that does not fit in
// the `src_bytes` bytes of `src` is read as a single pixel at offset 0, the window is clamped into the image and (hd, wd)
// to the canvas, so no record can read outside src; writes depend on B, H, W only.
#include "image_resample.h"

namespace detr {

struct AugPadArgs {
    const unsigned char *src; long long src_bytes;
    const int *irec;                     // [B][DETR_AUGP_IREC]
    float *dst;                          // [B, H, W, 3]
    unsigned char *mask;                 // [B, H, W]
    const float *lut;                    // [3][256]
    int B, H, W, perm0, perm1, perm2, vec;
};

// grid = (ceil(H * W / (AUG_THREADS * AUG_PIX)), B): the image index is uniform per workgroup, so is its record
__global__ __launch_bounds__(AUG_THREADS) void augment_padded_kernel(AugPadArgs a) {
    const int b = blockIdx.y;
    const int *ir = a.irec + (long long)b * DETR_AUGP_IREC;
    AugImage m = aug_image(a.src, a.src_bytes, ir);
    m.cy0 = min(max(ir[5], 0), m.h0 - 1);            // the window, clamped into the image and at least one pixel
    m.cx0 = min(max(ir[6], 0), m.w0 - 1);
    const int hc = min(max(ir[7], 1), m.h0 - m.cy0), wc = min(max(ir[8], 1), m.w0 - m.cx0);
    const int hd = min(max(ir[9], 0), a.H), wd = min(max(ir[10], 0), a.W);
    const int interp = min(max(ir[11], 0), 3);
    m.isx = m.isy = 1.0f;
    const int HW = a.H * a.W;                        // <= 2^30 (checked by the entry point)
    const long long p0l = ((long long)blockIdx.x * AUG_THREADS + threadIdx.x) * AUG_PIX;
    if (p0l >= HW) return;
    const int p0 = (int)p0l;
    int y = (int)((unsigned)p0 / (unsigned)a.W), x = p0 - y * a.W;
    float out[AUG_PIX * 3];
    unsigned pad = 0;                                // byte q = mask of pixel q
#pragma unroll
    for (int q = 0; q < AUG_PIX; ++q) {
        if (y < hd && x < wd) {                      // (a pixel past the canvas end has y >= H >= hd: padding, never stored)
            float v[3];
            resample(FetchWindow{m}, hc, wc, hd, wd, interp, y, x, v);
            lut_pixel(a.lut, a.perm0, a.perm1, a.perm2, v, out + 3 * q);
        } else {
            out[3 * q + 0] = 0.0f; out[3 * q + 1] = 0.0f; out[3 * q + 2] = 0.0f;
            pad |= 1u << (8 * q);
        }
        if (++x >= a.W) { x = 0; ++y; }
    }
    const long long base = (long long)b * HW + p0;
    unsigned char *mk = a.mask + base;
    const bool vec = a.vec && p0 + AUG_PIX <= HW;
    store_pixels(a.dst + base * 3, out, vec, HW - p0);
    if (vec) {
        *reinterpret_cast<unsigned *>(mk) = pad;
    } else {
        for (int q = 0; q < AUG_PIX && p0 + q < HW; ++q) mk[q] = (unsigned char)((pad >> (8 * q)) & 1u);
    }
}

}  // namespace detr

using namespace detr;

extern "C" int detr_hip_augment_padded(const uint8_t *src, int64_t src_bytes, const int32_t *irec, int32_t B, int32_t H, int32_t W,
                                       const float *lut, const int32_t *perm, float *dst, uint8_t *mask, void *stream) {
    DETR_REQUIRE(src && irec && lut && perm && dst && mask, "augment_padded: null operand");
    DETR_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0 && (long long)H * W <= (1ll << 30),
                 "augment_padded: bad shape B=%d H=%d W=%d", B, H, W);
    DETR_REQUIRE(src_bytes >= 3, "augment_padded: src_bytes must cover at least one pixel");
    DETR_REQUIRE(check_perm(perm), "augment_padded: channel permutation out of range");
    AugPadArgs a;
    a.src = src; a.src_bytes = src_bytes; a.irec = irec; a.dst = dst; a.mask = mask; a.lut = lut;
    a.B = B; a.H = H; a.W = W; a.perm0 = perm[0]; a.perm1 = perm[1]; a.perm2 = perm[2];
    const long long HW = (long long)H * W;
    // every lane's 12 floats start on a 16-byte boundary and its 4 mask bytes on a 4-byte one
    a.vec = aligned16(dst) && ((uintptr_t)mask & 3) == 0 && HW % AUG_PIX == 0;
    const long long groups = (HW + (long long)AUG_THREADS * AUG_PIX - 1) / ((long long)AUG_THREADS * AUG_PIX);
    hipLaunchKernelGGL(augment_padded_kernel, dim3((unsigned)groups, (unsigned)B), dim3(AUG_THREADS), 0, (hipStream_t)stream, a);
    DETR_LAUNCH_CHECK("augment_padded");
    return 0;
}

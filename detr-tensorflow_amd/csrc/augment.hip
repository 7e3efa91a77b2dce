// augment.hip -- training augmentation on the device: a ragged batch of uint8 images (each at its own size) -> the
// augmented, resized and normalised float32 NHWC batch, one launch.  The reference runs this on the host per image with
// imgaug (data/transformation.py:54-94,163-196: `detr_aug_seq`); here the host only draws one transform record per image
// (detr_tf/data/transformation.py) and the kernel applies it, in the reference's order:
//   F  horizontal flip (exact index mirror),
//   B  none | resize to (Hd, Wd) with interpolation `ia` | crop to min(Hd, h0) x min(Wd, w0) at (y0, x0) |
//      affine zoom about the centre (u = (x - cx) * (1/sx) + cx, cx = w0/2 - 0.5; bilinear, 0 outside the image),
//      output rounded to uint8 as in imgaug,
//   R  final resize of B's output to (Hd, Wd) with interpolation `if` (identity when the sizes agree),
// then the normalisation table of detr_hip_input_stage.  Stage B is fused into R: every tap of the final resize recomputes
// the stage-B pixel it reads (rounded to uint8 first), so the result is that of the two stages applied one after the other.
//
// Every resize is image_resample.h's resample(), the one input_stage_kernel calls: a record without flip and stage B gives
// detr_hip_input_stage's bits.  Area is OpenCV's INTER_AREA restated from its documentation: for r = src / dst >= 1 on both axes the fractional-overlap
// box average of the source footprint divided by rx * ry, otherwise per axis the linear taps with OpenCV's area-mode
// coefficient.  OpenCV's uint8 paths use fixed-point coefficients: parity with cv2 / imgaug is unpinned, as for cubic.
//
// Safety: every source index is clamped into its own image, and an image whose record does not fit in the `src_bytes`
// bytes of `src` is read as a single pixel at offset 0, so no record can read outside src; writes depend on B, Hd, Wd only.
#include "image_resample.h"

namespace detr {

struct AugArgs {
    const unsigned char *src; long long src_bytes;
    const int *irec;                     // [B][DETR_AUG_IREC]
    const float *frec;                   // [B][DETR_AUG_FREC]
    float *dst;                          // [B, Hd, Wd, 3]
    const float *lut;                    // [3][256]
    int B, Hd, Wd, perm0, perm1, perm2, vec;
};

// stage B = affine zoom about the image centre, bilinear, 0 outside the image, rounded to uint8
struct FetchAffine {
    const AugImage &m;
    __device__ __forceinline__ void operator()(int y, int x, float (&v)[3]) const {
        const float cx = (float)m.w0 * 0.5f - 0.5f, cy = (float)m.h0 * 0.5f - 0.5f;
        // clamping keeps floorf finite and in int range; any u outside [-2, w0 + 1] has both taps outside the image anyway
        const float u = fminf(fmaxf(((float)x - cx) * m.isx + cx, -2.0f), (float)m.w0 + 1.0f);
        const float w = fminf(fmaxf(((float)y - cy) * m.isy + cy, -2.0f), (float)m.h0 + 1.0f);
        const int x0 = (int)floorf(u), y0 = (int)floorf(w);
        const float cxs[2] = {1.0f - (u - (float)x0), u - (float)x0};
        const float cys[2] = {1.0f - (w - (float)y0), w - (float)y0};
        float acc[3] = {0.f, 0.f, 0.f};
        for (int j = 0; j < 2; ++j) {
            const int yy = y0 + j;
            float row[3] = {0.f, 0.f, 0.f};
            for (int k = 0; k < 2; ++k) {
                const int xx = x0 + k;
                float p[3] = {0.f, 0.f, 0.f};
                if (yy >= 0 && yy < m.h0 && xx >= 0 && xx < m.w0) fetch_f(m, yy, xx, p);
                row[0] += cxs[k] * p[0]; row[1] += cxs[k] * p[1]; row[2] += cxs[k] * p[2];
            }
            acc[0] += cys[j] * row[0]; acc[1] += cys[j] * row[1]; acc[2] += cys[j] * row[2];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = fminf(fmaxf(rintf(acc[c]), 0.0f), 255.0f);
    }
};

// grid = (ceil(Hd * Wd / (AUG_THREADS * AUG_PIX)), B): the image index is uniform per workgroup, so is its record
__global__ __launch_bounds__(AUG_THREADS) void augment_kernel(AugArgs a) {
    const int b = blockIdx.y;
    const int *ir = a.irec + (long long)b * DETR_AUG_IREC;
    const float *fr = a.frec + (long long)b * DETR_AUG_FREC;
    AugImage m = aug_image(a.src, a.src_bytes, ir);
    const int kind = ir[5], ia = min(max(ir[6], 0), 3), ifin = min(max(ir[7], 0), 3);
    m.cy0 = kind == 2 ? min(max(ir[8], 0), m.h0) : 0;   // crop offset (stage B = crop only)
    m.cx0 = kind == 2 ? min(max(ir[9], 0), m.w0) : 0;
    m.isx = fr[0]; m.isy = fr[1];
    const int Hd = a.Hd, Wd = a.Wd;
    const long long HW = (long long)Hd * Wd;
    const long long p0 = ((long long)blockIdx.x * AUG_THREADS + threadIdx.x) * AUG_PIX;
    if (p0 >= HW) return;
    float out[AUG_PIX * 3];
#pragma unroll
    for (int q = 0; q < AUG_PIX; ++q) {
        const long long p = min(p0 + q, HW - 1);
        const int y = (int)(p / Wd), x = (int)(p % Wd);
        float v[3];
        if (kind == 1) {                             // resize to (Hd, Wd): the final resize is the identity
            resample(FetchWindow{m}, m.h0, m.w0, Hd, Wd, ia, y, x, v);
        } else if (kind == 3) {
            resample(FetchAffine{m}, m.h0, m.w0, Hd, Wd, ifin, y, x, v);
        } else if (kind == 2) {
            resample(FetchWindow{m}, min(Hd, m.h0), min(Wd, m.w0), Hd, Wd, ifin, y, x, v);
        } else {
            resample(FetchWindow{m}, m.h0, m.w0, Hd, Wd, ifin, y, x, v);
        }
        lut_pixel(a.lut, a.perm0, a.perm1, a.perm2, v, out + 3 * q);
    }
    store_pixels(a.dst + ((long long)b * HW + p0) * 3, out, a.vec && p0 + AUG_PIX <= HW, HW - p0);
}

}  // namespace detr

using namespace detr;

extern "C" int detr_hip_augment(const uint8_t *src, int64_t src_bytes, const int32_t *irec, const float *frec, int32_t B, int32_t Hd,
                                int32_t Wd, const float *lut, const int32_t *perm, float *dst, void *stream) {
    DETR_REQUIRE(src && irec && frec && lut && perm && dst, "augment: null operand");
    DETR_REQUIRE(B > 0 && B <= 65535 && Hd > 0 && Wd > 0 && (long long)Hd * Wd <= (1ll << 30),
                 "augment: bad shape B=%d Hd=%d Wd=%d", B, Hd, Wd);
    DETR_REQUIRE(src_bytes >= 3, "augment: src_bytes must cover at least one pixel");
    DETR_REQUIRE(check_perm(perm), "augment: channel permutation out of range");
    AugArgs a;
    a.src = src; a.src_bytes = src_bytes; a.irec = irec; a.frec = frec; a.dst = dst; a.lut = lut;
    a.B = B; a.Hd = Hd; a.Wd = Wd; a.perm0 = perm[0]; a.perm1 = perm[1]; a.perm2 = perm[2];
    const long long HW = (long long)Hd * Wd;
    a.vec = aligned16(dst) && HW % AUG_PIX == 0;     // every lane's 12 floats start on a 16-byte boundary
    const long long groups = (HW + (long long)AUG_THREADS * AUG_PIX - 1) / ((long long)AUG_THREADS * AUG_PIX);
    hipLaunchKernelGGL(augment_kernel, dim3((unsigned)groups, (unsigned)B), dim3(AUG_THREADS), 0, (hipStream_t)stream, a);
    DETR_LAUNCH_CHECK("augment");
    return 0;
}

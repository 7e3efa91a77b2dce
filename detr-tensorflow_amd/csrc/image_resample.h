// image_resample.h -- what the uint8 -> float32 image-input kernels share (input_stage.hip, padding_mask.hip: input_stage_padded,
// augment.hip, augment_padded.hip):
//   * resample(): nearest / linear / cubic / area resize of whatever image a fetch functor reads.  Nearest / linear / cubic are the
//     documented kernels of cv2.resize in fp32 (half-pixel centres, replicated border, a = -0.75); area is OpenCV's INTER_AREA
//     restated from its documentation (see augment.hip).  It is the ONLY statement of these formulas, and every file that calls it
//     is compiled with -ffp-contract=off: one source, one result, whichever kernel asks;
//   * the ragged-batch side of the two augment kernels: the record header decoded into an AugImage, the clamped fetch of a flipped
//     image, the 4-pixel store of a lane;
//   * lut_pixel(): the normalise-and-permute lookup; check_perm(): its host-side check.
#pragma once
#include "common.h"

namespace detr {

constexpr int AUG_THREADS = 256;
constexpr int AUG_PIX = 4;               // output pixels per lane of the augment kernels: 12 floats = three 16-byte stores

static inline bool check_perm(const int32_t *perm) {
    for (int c = 0; c < 3; ++c)
        if (perm[c] < 0 || perm[c] >= 3) return false;
    return true;
}

// normalisation + channel order: o[c] = lut[c][v[perm_c]], v = one pixel's uint8 values (as int or float)
template <class V>
__device__ __forceinline__ void lut_pixel(const float *lut, int perm0, int perm1, int perm2, const V (&v)[3], float *o) {
    o[0] = lut[(int)v[perm0]]; o[1] = lut[256 + (int)v[perm1]]; o[2] = lut[512 + (int)v[perm2]];
}

struct AugImage {
    const unsigned char *src; long long lo, hi;      // readable byte range of this image: [lo, hi]
    int h0, w0, flip, cy0, cx0;
    float isx, isy;
};

// record header ir[0..4] = (offset lo, offset hi, h0, w0, flip) -> the image; the window and the zoom are the caller's
__device__ __forceinline__ AugImage aug_image(const unsigned char *src, long long src_bytes, const int *ir) {
    AugImage m;
    m.src = src;
    long long off = (long long)(unsigned)ir[0] | ((long long)ir[1] << 32);
    m.h0 = ir[2]; m.w0 = ir[3];
    if (off < 0 || m.h0 < 1 || m.w0 < 1 || m.h0 > 65536 || m.w0 > 65536 || off + (long long)m.h0 * m.w0 * 3 > src_bytes) {
        off = 0; m.h0 = 1; m.w0 = 1;                 // a record that does not fit: one pixel at offset 0
    }
    m.lo = off; m.hi = off + (long long)m.h0 * m.w0 * 3 - 3;
    m.flip = ir[4] & 1;
    return m;
}

// a lane's AUG_PIX pixels: three 16-byte stores when `vec` (all of them inside the image and o 16-byte aligned), else the first n
__device__ __forceinline__ void store_pixels(float *o, const float (&out)[AUG_PIX * 3], bool vec, long long n) {
    if (vec) {
        float4 *o4 = reinterpret_cast<float4 *>(o);
        o4[0] = make_float4(out[0], out[1], out[2], out[3]);
        o4[1] = make_float4(out[4], out[5], out[6], out[7]);
        o4[2] = make_float4(out[8], out[9], out[10], out[11]);
    } else {
        for (int q = 0; q < AUG_PIX && q < n; ++q) {
            o[3 * q + 0] = out[3 * q + 0]; o[3 * q + 1] = out[3 * q + 1]; o[3 * q + 2] = out[3 * q + 2];
        }
    }
}

// pixel (y, x) of the flipped source image (stage F), clamped into the image
__device__ __forceinline__ void fetch_f(const AugImage &m, int y, int x, float (&v)[3]) {
    y = min(max(y, 0), m.h0 - 1);
    x = min(max(x, 0), m.w0 - 1);
    if (m.flip) x = m.w0 - 1 - x;
    const long long o = min(max(m.lo + ((long long)y * m.w0 + x) * 3, m.lo), m.hi);
    const unsigned char *p = m.src + o;
    v[0] = p[0]; v[1] = p[1]; v[2] = p[2];
}

// stage B = none / crop: a shifted window of F
struct FetchWindow {
    const AugImage &m;
    __device__ __forceinline__ void operator()(int y, int x, float (&v)[3]) const { fetch_f(m, y + m.cy0, x + m.cx0, v); }
};

__device__ __forceinline__ void cubic_coeffs(float f, float (&c)[4]) {
    const float A = -0.75f;
    c[0] = ((A * (f + 1.0f) - 5.0f * A) * (f + 1.0f) + 8.0f * A) * (f + 1.0f) - 4.0f * A;
    c[1] = ((A + 2.0f) * f - (A + 3.0f)) * f * f + 1.0f;
    c[2] = ((A + 2.0f) * (1.0f - f) - (A + 3.0f)) * (1.0f - f) * (1.0f - f) + 1.0f;
    c[3] = 1.0f - c[0] - c[1] - c[2];
}

// area mode, one axis, linear-tap form (some ratio < 1): s = floor(d * r), f = (d + 1) - (s + 1) / r, f <= 0 ? 0 : frac(f)
__device__ __forceinline__ void area_linear_axis(int d, float r, int &s, float (&c)[4]) {
    s = (int)floorf((float)d * r);
    float f = ((float)d + 1.0f) - ((float)s + 1.0f) / r;
    f = f <= 0.0f ? 0.0f : f - floorf(f);
    c[0] = 1.0f - f; c[1] = f;
}

// resize of the Hs x Ws image `fetch` reads to Hd x Wd at output pixel (y, x); result rounded + saturated to uint8 values.
// AREA = false: the caller never passes mode 3 (detr_hip_input_stage rejects it), and its kernel does not carry the area code --
// with it input_stage_kernel's cubic resize measured 2 % slower (NOTEBOOK 20).
template <bool AREA = true, class Fetch>
__device__ __forceinline__ void resample(const Fetch &fetch, int Hs, int Ws, int Hd, int Wd, int mode, int y, int x, float (&v)[3]) {
    if (Hs == Hd && Ws == Wd) { fetch(y, x, v); return; }
    const float sy = (float)Hs / (float)Hd, sx = (float)Ws / (float)Wd;
    if (mode == 0) {
        const int yy = min(max((int)floorf((float)y * sy), 0), Hs - 1), xx = min(max((int)floorf((float)x * sx), 0), Ws - 1);
        fetch(yy, xx, v);
        return;
    }
    float acc[3] = {0.f, 0.f, 0.f};
    if (AREA && mode == 3 && sy >= 1.0f && sx >= 1.0f) {
        // box average: fractional overlap of [d * r, (d + 1) * r) with every source cell, / (rx * ry)
        const float fy1 = (float)y * sy, fy2 = (float)(y + 1) * sy, fx1 = (float)x * sx, fx2 = (float)(x + 1) * sx;
        const int ylo = min((int)floorf(fy1), Hs - 1), yhi = min((int)ceilf(fy2) - 1, Hs - 1);
        const int xlo = min((int)floorf(fx1), Ws - 1), xhi = min((int)ceilf(fx2) - 1, Ws - 1);
        for (int j = ylo; j <= yhi; ++j) {
            const float oy = fminf(fy2, (float)(j + 1)) - fmaxf(fy1, (float)j);
            float row[3] = {0.f, 0.f, 0.f};
            for (int k = xlo; k <= xhi; ++k) {
                const float ox = fminf(fx2, (float)(k + 1)) - fmaxf(fx1, (float)k);
                float p[3];
                fetch(j, k, p);
                row[0] += ox * p[0]; row[1] += ox * p[1]; row[2] += ox * p[2];
            }
            acc[0] += oy * row[0]; acc[1] += oy * row[1]; acc[2] += oy * row[2];
        }
        const float inv = 1.0f / (sx * sy);
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] = acc[c] * inv;
    } else {
        int n, off, y0, x0;
        float cy[4], cx[4];
        if (AREA && mode == 3) {
            area_linear_axis(y, sy, y0, cy);
            area_linear_axis(x, sx, x0, cx);
            n = 2; off = 0;
        } else {
            const float fy = ((float)y + 0.5f) * sy - 0.5f, fx = ((float)x + 0.5f) * sx - 0.5f;
            y0 = (int)floorf(fy); x0 = (int)floorf(fx);
            if (mode == 1) {
                cy[0] = 1.0f - (fy - (float)y0); cy[1] = fy - (float)y0;
                cx[0] = 1.0f - (fx - (float)x0); cx[1] = fx - (float)x0;
                n = 2; off = 0;
            } else {
                cubic_coeffs(fy - (float)y0, cy);
                cubic_coeffs(fx - (float)x0, cx);
                n = 4; off = -1;
            }
        }
        for (int j = 0; j < n; ++j) {
            const int yy = min(max(y0 + off + j, 0), Hs - 1);
            float row[3] = {0.f, 0.f, 0.f};
            for (int k = 0; k < n; ++k) {
                const int xx = min(max(x0 + off + k, 0), Ws - 1);
                float p[3];
                fetch(yy, xx, p);
                row[0] += cx[k] * p[0]; row[1] += cx[k] * p[1]; row[2] += cx[k] * p[2];
            }
            acc[0] += cy[j] * row[0]; acc[1] += cy[j] * row[1]; acc[2] += cy[j] * row[2];
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = fminf(fmaxf(rintf(acc[c]), 0.0f), 255.0f);      // back to uint8 like cv2 (saturate_cast)
}

}  // namespace detr

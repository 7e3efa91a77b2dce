// pool.hip -- elementwise companions of the ResNet stem and of the stride-2 shortcuts (NHWC) for gfx950:
//   * 3x3/s2 max pool over the zero-padded map + its backward, fp32 and bf16 storage (4 or 8 channels per lane);
//   * stride-2 subsample gather / scatter.
// Reference: detr_tf/networks/resnet_backbone.py:11-32,98-137 (see include/detr_hip.h).
#include "gemm_core.h"
namespace detr {

__global__ void maxpool_fwd_kernel(const float *__restrict__ x, float *__restrict__ y, uint8_t *__restrict__ amax,
                                   int N, int H, int W, int C, int Ho, int Wo, long long total) {
    for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < total;
         idx += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(idx % C);
        long long t = idx / C;
        const int wo = (int)(t % Wo);
        t /= Wo;
        const int ho = (int)(t % Ho);
        const int n = (int)(t / Ho);
        float best = -INFINITY;
        int bi = 0;
#pragma unroll
        for (int kh = 0; kh < 3; ++kh)
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                const int hi = 2 * ho - 1 + kh, wi = 2 * wo - 1 + kw;
                float v = 0.0f;  // the explicit ZeroPadding2D(1) takes part in the max
                if (hi >= 0 && wi >= 0 && hi < H && wi < W) v = x[(((long long)n * H + hi) * W + wi) * C + c];
                if (v > best) {
                    best = v;
                    bi = kh * 3 + kw;
                }
            }
        y[idx] = best;
        amax[idx] = (uint8_t)bi;
    }
}

// dx[n,h,w,c] = (x > 0) * sum over the (<= 4) pooling windows that contain (h,w) and selected it.
// Four channels per thread: float4 x / dy / dx accesses, one 32-bit load of the four argmax bytes.
__global__ __launch_bounds__(256) void maxpool_bwd_kernel(const float *__restrict__ dy, const uint8_t *__restrict__ amax,
                                                          const float *__restrict__ x, float *__restrict__ dx, int N, int H,
                                                          int W, int C, int Ho, int Wo, long long total4) {
    const int C4 = C >> 2;
    for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < total4;
         idx += (long long)gridDim.x * blockDim.x) {
        const int c4 = (int)(idx % C4);
        const unsigned pix = (unsigned)(idx / C4);
        const int w = (int)(pix % (unsigned)W);
        const unsigned t = pix / (unsigned)W;
        const int h = (int)(t % (unsigned)H);
        const int n = (int)(t / (unsigned)H);
        const float4 xv = reinterpret_cast<const float4 *>(x)[idx];
        float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int kh = 0; kh < 3; ++kh) {
            const int th = h + 1 - kh;
            if (th < 0 || (th & 1)) continue;
            const int ho = th >> 1;
            if (ho >= Ho) continue;
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                const int tw = w + 1 - kw;
                if (tw < 0 || (tw & 1)) continue;
                const int wo = tw >> 1;
                if (wo >= Wo) continue;
                const long long o4 = ((long long)(n * Ho + ho) * Wo + wo) * C4 + c4;
                const uint32_t am = reinterpret_cast<const uint32_t *>(amax)[o4];
                const float4 d = reinterpret_cast<const float4 *>(dy)[o4];
                const uint32_t tap = (uint32_t)(kh * 3 + kw);
                if ((am & 0xFFu) == tap) g.x += d.x;
                if (((am >> 8) & 0xFFu) == tap) g.y += d.y;
                if (((am >> 16) & 0xFFu) == tap) g.z += d.z;
                if ((am >> 24) == tap) g.w += d.w;
            }
        }
        g.x = xv.x > 0.0f ? g.x : 0.0f;
        g.y = xv.y > 0.0f ? g.y : 0.0f;
        g.z = xv.z > 0.0f ? g.z : 0.0f;
        g.w = xv.w > 0.0f ? g.w : 0.0f;
        reinterpret_cast<float4 *>(dx)[idx] = g;
    }
}

// bf16-storage twins of the two pooling kernels (4 channels = 8 bytes per thread)
__device__ __forceinline__ float4 bf4_to_f4(uint2 v) {
    return make_float4(bf16_bits_to_f32(v.x & 0xFFFFu), bf16_bits_to_f32(v.x >> 16), bf16_bits_to_f32(v.y & 0xFFFFu), bf16_bits_to_f32(v.y >> 16));
}
__global__ __launch_bounds__(256) void maxpool_fwd_bf16_kernel(const uint2 *__restrict__ x, uint2 *__restrict__ y,
                                                               uint32_t *__restrict__ amax, int N, int H, int W, int C4,
                                                               int Ho, int Wo, long long total4) {
    for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < total4;
         idx += (long long)gridDim.x * blockDim.x) {
        const int c4 = (int)(idx % C4);
        const unsigned pix = (unsigned)(idx / C4);
        const int wo = (int)(pix % (unsigned)Wo);
        const unsigned t = pix / (unsigned)Wo;
        const int ho = (int)(t % (unsigned)Ho);
        const int n = (int)(t / (unsigned)Ho);
        float best[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        uint32_t bi[4] = {0, 0, 0, 0};
#pragma unroll
        for (int kh = 0; kh < 3; ++kh)
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                const int hi = 2 * ho - 1 + kh, wi = 2 * wo - 1 + kw;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);   // the explicit ZeroPadding2D(1) takes part in the max
                if (hi >= 0 && wi >= 0 && hi < H && wi < W) v = bf4_to_f4(x[((long long)(n * H + hi) * W + wi) * C4 + c4]);
                const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (vv[e] > best[e]) { best[e] = vv[e]; bi[e] = (uint32_t)(kh * 3 + kw); }
            }
        y[idx] = make_uint2(f32_to_bf16_pair(best[0], best[1]), f32_to_bf16_pair(best[2], best[3]));   // exact: inputs are bf16
        amax[idx] = bi[0] | (bi[1] << 8) | (bi[2] << 16) | (bi[3] << 24);
    }
}

__global__ __launch_bounds__(256) void maxpool_bwd_bf16_kernel(const uint2 *__restrict__ dy, const uint32_t *__restrict__ amax,
                                                               const uint2 *__restrict__ x, uint2 *__restrict__ dx, int N, int H,
                                                               int W, int C4, int Ho, int Wo, long long total4) {
    for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < total4;
         idx += (long long)gridDim.x * blockDim.x) {
        const int c4 = (int)(idx % C4);
        const unsigned pix = (unsigned)(idx / C4);
        const int w = (int)(pix % (unsigned)W);
        const unsigned t = pix / (unsigned)W;
        const int h = (int)(t % (unsigned)H);
        const int n = (int)(t / (unsigned)H);
        const float4 xv = bf4_to_f4(x[idx]);
        float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int kh = 0; kh < 3; ++kh) {
            const int th = h + 1 - kh;
            if (th < 0 || (th & 1)) continue;
            const int ho = th >> 1;
            if (ho >= Ho) continue;
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                const int tw = w + 1 - kw;
                if (tw < 0 || (tw & 1)) continue;
                const int wo = tw >> 1;
                if (wo >= Wo) continue;
                const long long o4 = ((long long)(n * Ho + ho) * Wo + wo) * C4 + c4;
                const uint32_t am = amax[o4];
                const float4 d = bf4_to_f4(dy[o4]);
                const uint32_t tap = (uint32_t)(kh * 3 + kw);
                if ((am & 0xFFu) == tap) g.x += d.x;
                if (((am >> 8) & 0xFFu) == tap) g.y += d.y;
                if (((am >> 16) & 0xFFu) == tap) g.z += d.z;
                if ((am >> 24) == tap) g.w += d.w;
            }
        }
        g.x = xv.x > 0.0f ? g.x : 0.0f;
        g.y = xv.y > 0.0f ? g.y : 0.0f;
        g.z = xv.z > 0.0f ? g.z : 0.0f;
        g.w = xv.w > 0.0f ? g.w : 0.0f;
        dx[idx] = make_uint2(f32_to_bf16_pair(g.x, g.y), f32_to_bf16_pair(g.z, g.w));
    }
}
// 8-channel (16-byte) forms of the two bf16 pooling kernels: half the memory instructions and half the index arithmetic per
// byte of the 4-channel forms above (which stay for C % 8 != 0).  rocprofv3, stem map 8 x 400 x 667 x 64: backward 266 us
// at 2.3 TB/s with 8-byte accesses.
__device__ __forceinline__ void bf8_to_f8(uint4 v, float (&o)[8]) {
    o[0] = __builtin_bit_cast(float, v.x << 16); o[1] = __builtin_bit_cast(float, v.x & 0xFFFF0000u);
    o[2] = __builtin_bit_cast(float, v.y << 16); o[3] = __builtin_bit_cast(float, v.y & 0xFFFF0000u);
    o[4] = __builtin_bit_cast(float, v.z << 16); o[5] = __builtin_bit_cast(float, v.z & 0xFFFF0000u);
    o[6] = __builtin_bit_cast(float, v.w << 16); o[7] = __builtin_bit_cast(float, v.w & 0xFFFF0000u);
}

__global__ __launch_bounds__(256) void maxpool_fwd_bf16x8_kernel(const uint4 *__restrict__ x, uint4 *__restrict__ y,
                                                                 uint2 *__restrict__ amax, int N, int H, int W, int C8,
                                                                 int Ho, int Wo, long long total8) {
    for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < total8;
         idx += (long long)gridDim.x * blockDim.x) {
        const int c8 = (int)(idx % C8);
        const unsigned pix = (unsigned)(idx / C8);
        const int wo = (int)(pix % (unsigned)Wo);
        const unsigned t = pix / (unsigned)Wo;
        const int ho = (int)(t % (unsigned)Ho);
        const int n = (int)(t / (unsigned)Ho);
        // bf16 values compare like their bit patterns moved to the high half of a float: keep the raw winners, no re-rounding
        float best[8];
        uint32_t bi[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) { best[e] = -INFINITY; bi[e] = 0; }
#pragma unroll
        for (int kh = 0; kh < 3; ++kh)
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                const int hi = 2 * ho - 1 + kh, wi = 2 * wo - 1 + kw;
                uint4 raw = make_uint4(0u, 0u, 0u, 0u);       // the explicit ZeroPadding2D(1) takes part in the max
                if (hi >= 0 && wi >= 0 && hi < H && wi < W) raw = x[((long long)(n * H + hi) * W + wi) * C8 + c8];
                float vv[8];
                bf8_to_f8(raw, vv);
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    if (vv[e] > best[e]) { best[e] = vv[e]; bi[e] = (uint32_t)(kh * 3 + kw); }
            }
        y[idx] = make_uint4(f32_to_bf16_pair(best[0], best[1]), f32_to_bf16_pair(best[2], best[3]),
                            f32_to_bf16_pair(best[4], best[5]), f32_to_bf16_pair(best[6], best[7]));      // exact: inputs are bf16
        amax[idx] = make_uint2(bi[0] | (bi[1] << 8) | (bi[2] << 16) | (bi[3] << 24), bi[4] | (bi[5] << 8) | (bi[6] << 16) | (bi[7] << 24));
    }
}

__global__ __launch_bounds__(256) void maxpool_bwd_bf16x8_kernel(const uint4 *__restrict__ dy, const uint2 *__restrict__ amax,
                                                                 const uint4 *__restrict__ x, uint4 *__restrict__ dx, int N, int H,
                                                                 int W, int C8, int Ho, int Wo, long long total8) {
    for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < total8;
         idx += (long long)gridDim.x * blockDim.x) {
        const int c8 = (int)(idx % C8);
        const unsigned pix = (unsigned)(idx / C8);
        const int w = (int)(pix % (unsigned)W);
        const unsigned t = pix / (unsigned)W;
        const int h = (int)(t % (unsigned)H);
        const int n = (int)(t / (unsigned)H);
        const uint4 xraw = x[idx];
        float g[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) g[e] = 0.0f;
#pragma unroll
        for (int kh = 0; kh < 3; ++kh) {
            const int th = h + 1 - kh;
            if (th < 0 || (th & 1)) continue;
            const int ho = th >> 1;
            if (ho >= Ho) continue;
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                const int tw = w + 1 - kw;
                if (tw < 0 || (tw & 1)) continue;
                const int wo = tw >> 1;
                if (wo >= Wo) continue;
                const long long o8 = ((long long)(n * Ho + ho) * Wo + wo) * C8 + c8;
                const uint2 am = amax[o8];
                float d[8];
                bf8_to_f8(dy[o8], d);
                const uint32_t tap = (uint32_t)(kh * 3 + kw);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (((am.x >> (8 * e)) & 0xFFu) == tap) g[e] += d[e];
                    if (((am.y >> (8 * e)) & 0xFFu) == tap) g[4 + e] += d[4 + e];
                }
            }
        }
        float xv[8];
        bf8_to_f8(xraw, xv);
#pragma unroll
        for (int e = 0; e < 8; ++e) g[e] = xv[e] > 0.0f ? g[e] : 0.0f;
        dx[idx] = make_uint4(f32_to_bf16_pair(g[0], g[1]), f32_to_bf16_pair(g[2], g[3]), f32_to_bf16_pair(g[4], g[5]), f32_to_bf16_pair(g[6], g[7]));
    }
}



__global__ void subsample2_fwd_kernel(const float4 *__restrict__ x, float4 *__restrict__ y, int H, int W, int C4,
                                      int Ho, int Wo, long long total) {
    for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < total;
         idx += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(idx % C4);
        long long t = idx / C4;
        const int wo = (int)(t % Wo);
        t /= Wo;
        const int ho = (int)(t % Ho);
        const long long n = t / Ho;
        y[idx] = x[((n * H + 2 * ho) * W + 2 * wo) * C4 + c];
    }
}

__global__ void subsample2_bwd_kernel(const float4 *__restrict__ dy, float4 *__restrict__ dx, int H, int W, int C4,
                                      int Ho, int Wo, long long total) {
    for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < total;
         idx += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(idx % C4);
        long long t = idx / C4;
        const int w = (int)(t % W);
        t /= W;
        const int h = (int)(t % H);
        const long long n = t / H;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (!(h & 1) && !(w & 1) && (h >> 1) < Ho && (w >> 1) < Wo)
            v = dy[((n * Ho + (h >> 1)) * Wo + (w >> 1)) * C4 + c];
        dx[idx] = v;
    }
}

static inline int ew_grid(long long total, int block) {
    long long g = (total + block - 1) / block;
    return (int)(g > 8192 ? 8192 : (g < 1 ? 1 : g));
}

}  // namespace detr

using namespace detr;

extern "C" int detr_hip_maxpool3x3s2_fwd_f32(const float *x, float *y, uint8_t *argmax, int32_t N, int32_t H, int32_t W,
                                             int32_t C, int32_t Ho, int32_t Wo, void *stream) {
    DETR_REQUIRE(x && y && argmax, "maxpool fwd: null operand");
    DETR_REQUIRE(Ho == (H + 2 - 3) / 2 + 1 && Wo == (W + 2 - 3) / 2 + 1, "maxpool fwd: bad output size");
    const long long total = (long long)N * Ho * Wo * C;
    hipLaunchKernelGGL(maxpool_fwd_kernel, dim3(ew_grid(total, 256)), dim3(256), 0, (hipStream_t)stream, x, y, argmax, N,
                       H, W, C, Ho, Wo, total);
    DETR_LAUNCH_CHECK("maxpool fwd");
    return 0;
}

extern "C" int detr_hip_maxpool3x3s2_bwd_f32(const float *dy, const uint8_t *argmax, const float *x, float *dx, int32_t N,
                                             int32_t H, int32_t W, int32_t C, int32_t Ho, int32_t Wo, void *stream) {
    DETR_REQUIRE(dy && argmax && x && dx, "maxpool bwd: null operand");
    DETR_REQUIRE(C % 4 == 0 && aligned16(dy) && aligned16(x) && aligned16(dx) && ((uintptr_t)argmax % 4 == 0),
                 "maxpool bwd: C must be a multiple of 4 and the tensors 16-byte aligned");
    const long long total = (long long)N * H * W * (C / 4);
    hipLaunchKernelGGL(maxpool_bwd_kernel, dim3(ew_grid(total, 256)), dim3(256), 0, (hipStream_t)stream, dy, argmax, x,
                       dx, N, H, W, C, Ho, Wo, total);
    DETR_LAUNCH_CHECK("maxpool bwd");
    return 0;
}

extern "C" int detr_hip_subsample2_fwd_f32(const float *x, float *y, int32_t N, int32_t H, int32_t W, int32_t C,
                                           int32_t Ho, int32_t Wo, void *stream) {
    DETR_REQUIRE(x && y && C % 4 == 0 && aligned16(x) && aligned16(y), "subsample2 fwd: bad operands");
    DETR_REQUIRE(Ho == (H - 1) / 2 + 1 && Wo == (W - 1) / 2 + 1, "subsample2 fwd: bad output size");
    const long long total = (long long)N * Ho * Wo * (C / 4);
    hipLaunchKernelGGL(subsample2_fwd_kernel, dim3(ew_grid(total, 256)), dim3(256), 0, (hipStream_t)stream,
                       (const float4 *)x, (float4 *)y, H, W, C / 4, Ho, Wo, total);
    DETR_LAUNCH_CHECK("subsample2 fwd");
    return 0;
}

extern "C" int detr_hip_subsample2_bwd_f32(const float *dy, float *dx, int32_t N, int32_t H, int32_t W, int32_t C,
                                           int32_t Ho, int32_t Wo, void *stream) {
    DETR_REQUIRE(dy && dx && C % 4 == 0 && aligned16(dy) && aligned16(dx), "subsample2 bwd: bad operands");
    const long long total = (long long)N * H * W * (C / 4);
    hipLaunchKernelGGL(subsample2_bwd_kernel, dim3(ew_grid(total, 256)), dim3(256), 0, (hipStream_t)stream,
                       (const float4 *)dy, (float4 *)dx, H, W, C / 4, Ho, Wo, total);
    DETR_LAUNCH_CHECK("subsample2 bwd");
    return 0;
}

extern "C" int detr_hip_maxpool3x3s2_fwd_bf16(const uint16_t *x, uint16_t *y, uint8_t *argmax, int32_t N, int32_t H, int32_t W,
                                              int32_t C, int32_t Ho, int32_t Wo, void *stream) {
    DETR_REQUIRE(x && y && argmax && C % 4 == 0, "maxpool fwd bf16: bad operands");
    DETR_REQUIRE(((uintptr_t)x % 8 == 0) && ((uintptr_t)y % 8 == 0) && ((uintptr_t)argmax % 4 == 0), "maxpool fwd bf16: alignment");
    DETR_REQUIRE(Ho == (H + 2 - 3) / 2 + 1 && Wo == (W + 2 - 3) / 2 + 1, "maxpool fwd: bad output size");
    if (C % 8 == 0 && ((uintptr_t)x % 16 == 0) && ((uintptr_t)y % 16 == 0) && ((uintptr_t)argmax % 8 == 0)) {
        const long long total8 = (long long)N * Ho * Wo * (C / 8);
        hipLaunchKernelGGL(maxpool_fwd_bf16x8_kernel, dim3(ew_grid(total8, 256)), dim3(256), 0, (hipStream_t)stream, (const uint4 *)x,
                           (uint4 *)y, (uint2 *)argmax, N, H, W, C / 8, Ho, Wo, total8);
        DETR_LAUNCH_CHECK("maxpool fwd bf16 (8 channels per lane)");
        return 0;
    }
    const long long total = (long long)N * Ho * Wo * (C / 4);
    hipLaunchKernelGGL(maxpool_fwd_bf16_kernel, dim3(ew_grid(total, 256)), dim3(256), 0, (hipStream_t)stream, (const uint2 *)x,
                       (uint2 *)y, (uint32_t *)argmax, N, H, W, C / 4, Ho, Wo, total);
    DETR_LAUNCH_CHECK("maxpool fwd bf16");
    return 0;
}

extern "C" int detr_hip_maxpool3x3s2_bwd_bf16(const uint16_t *dy, const uint8_t *argmax, const uint16_t *x, uint16_t *dx, int32_t N,
                                              int32_t H, int32_t W, int32_t C, int32_t Ho, int32_t Wo, void *stream) {
    DETR_REQUIRE(dy && argmax && x && dx && C % 4 == 0, "maxpool bwd bf16: bad operands");
    DETR_REQUIRE(((uintptr_t)dy % 8 == 0) && ((uintptr_t)x % 8 == 0) && ((uintptr_t)dx % 8 == 0) && ((uintptr_t)argmax % 4 == 0),
                 "maxpool bwd bf16: alignment");
    if (C % 8 == 0 && ((uintptr_t)dy % 16 == 0) && ((uintptr_t)x % 16 == 0) && ((uintptr_t)dx % 16 == 0) && ((uintptr_t)argmax % 8 == 0)) {
        const long long total8 = (long long)N * H * W * (C / 8);
        hipLaunchKernelGGL(maxpool_bwd_bf16x8_kernel, dim3(ew_grid(total8, 256)), dim3(256), 0, (hipStream_t)stream, (const uint4 *)dy,
                           (const uint2 *)argmax, (const uint4 *)x, (uint4 *)dx, N, H, W, C / 8, Ho, Wo, total8);
        DETR_LAUNCH_CHECK("maxpool bwd bf16 (8 channels per lane)");
        return 0;
    }
    const long long total = (long long)N * H * W * (C / 4);
    hipLaunchKernelGGL(maxpool_bwd_bf16_kernel, dim3(ew_grid(total, 256)), dim3(256), 0, (hipStream_t)stream, (const uint2 *)dy,
                       (const uint32_t *)argmax, (const uint2 *)x, (uint2 *)dx, N, H, W, C / 4, Ho, Wo, total);
    DETR_LAUNCH_CHECK("maxpool bwd bf16");
    return 0;
}

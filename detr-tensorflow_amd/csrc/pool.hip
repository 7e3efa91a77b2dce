// pool.hip -- elementwise companions of the ResNet stem and of the stride-2 shortcuts (NHWC) for gfx950:
//   * 3x3/s2 max pool over the zero-padded map + its backward: ONE forward and ONE backward body (maxpool_*_kernel<T, V>) over the
//     storage type T and the channels per lane V, instantiated as f32 x 1 (forward), f32 x 4 (backward), bf16 x 4 and bf16 x 8;
//   * stride-2 subsample gather / scatter.
// Reference: detr_tf/networks/resnet_backbone.py:11-32,98-137 (see include/detr_hip.h).
#include "gemm_core.h"
namespace detr {

// What one lane holds of one pixel: V channels of storage type T (float, or uint16_t = bf16 bits) as one vector `vec`, and their V
// argmax bytes (one per channel, kh * 3 + kw) as V / 4 32-bit words (V = 1: the byte itself).
template <class T, int V> struct PoolLane;
template <> struct PoolLane<float, 1> {
    using vec = float;
    using amax_t = uint8_t;
    static __device__ __forceinline__ void to_f32(vec r, float (&o)[1]) { o[0] = r; }
    static __device__ __forceinline__ vec from_f32(const float (&v)[1]) { return v[0]; }
};
template <> struct PoolLane<float, 4> {
    using vec = float4;
    using amax_t = uint32_t;
    static __device__ __forceinline__ void to_f32(vec r, float (&o)[4]) { o[0] = r.x; o[1] = r.y; o[2] = r.z; o[3] = r.w; }
    static __device__ __forceinline__ vec from_f32(const float (&v)[4]) { return make_float4(v[0], v[1], v[2], v[3]); }
};
template <> struct PoolLane<uint16_t, 4> {
    using vec = uint2;
    using amax_t = uint32_t;
    static __device__ __forceinline__ void to_f32(vec r, float (&o)[4]) {
        o[0] = bf16_bits_to_f32(r.x & 0xFFFFu); o[1] = bf16_bits_to_f32(r.x >> 16);
        o[2] = bf16_bits_to_f32(r.y & 0xFFFFu); o[3] = bf16_bits_to_f32(r.y >> 16);
    }
    static __device__ __forceinline__ vec from_f32(const float (&v)[4]) { return make_uint2(f32_to_bf16_pair(v[0], v[1]), f32_to_bf16_pair(v[2], v[3])); }
};
// 8 channels (16 bytes) per lane: half the memory instructions and half the index arithmetic per byte of the 4-channel form (which
// stays for C % 8 != 0).  rocprofv3, stem map 8 x 400 x 667 x 64: backward 266 us at 2.3 TB/s with 8-byte accesses.
template <> struct PoolLane<uint16_t, 8> {
    using vec = uint4;
    using amax_t = uint2;
    static __device__ __forceinline__ void to_f32(vec r, float (&o)[8]) {
        o[0] = __builtin_bit_cast(float, r.x << 16); o[1] = __builtin_bit_cast(float, r.x & 0xFFFF0000u);
        o[2] = __builtin_bit_cast(float, r.y << 16); o[3] = __builtin_bit_cast(float, r.y & 0xFFFF0000u);
        o[4] = __builtin_bit_cast(float, r.z << 16); o[5] = __builtin_bit_cast(float, r.z & 0xFFFF0000u);
        o[6] = __builtin_bit_cast(float, r.w << 16); o[7] = __builtin_bit_cast(float, r.w & 0xFFFF0000u);
    }
    static __device__ __forceinline__ vec from_f32(const float (&v)[8]) {
        return make_uint4(f32_to_bf16_pair(v[0], v[1]), f32_to_bf16_pair(v[2], v[3]), f32_to_bf16_pair(v[4], v[5]), f32_to_bf16_pair(v[6], v[7]));
    }
};
__device__ __forceinline__ uint8_t pack_taps(const uint32_t (&t)[1]) { return (uint8_t)t[0]; }
__device__ __forceinline__ uint32_t pack_taps(const uint32_t (&t)[4]) { return t[0] | (t[1] << 8) | (t[2] << 16) | (t[3] << 24); }
__device__ __forceinline__ uint2 pack_taps(const uint32_t (&t)[8]) {
    return make_uint2(t[0] | (t[1] << 8) | (t[2] << 16) | (t[3] << 24), t[4] | (t[5] << 8) | (t[6] << 16) | (t[7] << 24));
}
__device__ __forceinline__ uint32_t tap_of(uint32_t a, int e) { return (a >> (8 * e)) & 0xFFu; }
__device__ __forceinline__ uint32_t tap_of(uint2 a, int e) { return ((e < 4 ? a.x : a.y) >> (8 * (e & 3))) & 0xFFu; }

// pixel index -> (n, row, col) of an N x rows x cols map; every max-pool entry point checks that N * H * W fits in 31 bits
__device__ __forceinline__ void pool_pixel(long long idx, int CV, int rows, int cols, int &cv, int &n, int &r, int &c) {
    cv = (int)(idx % CV);
    const unsigned pix = (unsigned)(idx / CV);
    c = (int)(pix % (unsigned)cols);
    const unsigned t = pix / (unsigned)cols;
    r = (int)(t % (unsigned)rows);
    n = (int)(t / (unsigned)rows);
}

// y[n,ho,wo,c] = max over the 3x3 / stride-2 window of the zero-padded map; the FIRST maximal tap wins (strict `>` in kh-major order).
// A NaN tap is taken too and then never replaced (nothing compares greater than it): a window that holds a NaN gives NaN, as
// F.max_pool2d does, and its argmax byte names a NaN tap (the last one), where the backward then puts the window's gradient.
template <class T, int V>
__global__ __launch_bounds__(256) void maxpool_fwd_kernel(const typename PoolLane<T, V>::vec *__restrict__ x,
                                                          typename PoolLane<T, V>::vec *__restrict__ y,
                                                          typename PoolLane<T, V>::amax_t *__restrict__ amax, int N, int H, int W, int CV,
                                                          int Ho, int Wo, long long total) {
    using L = PoolLane<T, V>;
    for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < total;
         idx += (long long)gridDim.x * blockDim.x) {
        int cv, n, ho, wo;
        pool_pixel(idx, CV, Ho, Wo, cv, n, ho, wo);
        float best[V];
        uint32_t bi[V];
#pragma unroll
        for (int e = 0; e < V; ++e) { best[e] = -INFINITY; bi[e] = 0; }
#pragma unroll
        for (int kh = 0; kh < 3; ++kh)
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                const int hi = 2 * ho - 1 + kh, wi = 2 * wo - 1 + kw;
                // the explicit ZeroPadding2D(1) takes part in the max.  Select the raw vector, convert after: converting under the
                // branch into a zeroed float[V] costs the 8-channel form 31 VGPRs.
                typename L::vec raw = {};
                if (hi >= 0 && wi >= 0 && hi < H && wi < W) raw = x[((long long)(n * H + hi) * W + wi) * CV + cv];
                float v[V];
                L::to_f32(raw, v);
#pragma unroll
                for (int e = 0; e < V; ++e)
                    if (v[e] > best[e] || v[e] != v[e]) { best[e] = v[e]; bi[e] = (uint32_t)(kh * 3 + kw); }
            }
        y[idx] = L::from_f32(best);                  // exact: inputs are bf16
        amax[idx] = pack_taps(bi);
    }
}

// dx[n,h,w,c] = (x > 0) * sum over the (<= 4) pooling windows that contain (h,w) and selected it: only taps of the parity of
// (h + 1, w + 1) can reach the pixel.  One vector access of x / dy / dx and one load of the V argmax bytes per window.
// The candidate windows are enumerated, not searched: tap row kh0 = the one of the parity of h + 1 and, for odd h, tap row 2 (the
// same for the columns), in the (kh, kw) order of the forward's taps -- the order of the sum.  Every request of a pixel is issued
// before the first value is used.  (The former loop over the nine taps skipped the others with `continue`: neighbouring pixels
// of a wave differ in parity, so the wave walked the windows one exec-masked branch after the other, a memory round trip each --
// 191 -> 150 us at 8 x 400 x 667 x 64 bf16 by HIP events, 181 -> 131 us in the step's trace, profiles/shortcut_pool_shadow_ab.txt.)  A window that does not exist gets the tap
// 0xFF, which no argmax byte holds, and zeros for dy: adding nothing, as before.
template <class T, int V>
__global__ __launch_bounds__(256) void maxpool_bwd_kernel(const typename PoolLane<T, V>::vec *__restrict__ dy,
                                                          const typename PoolLane<T, V>::amax_t *__restrict__ amax,
                                                          const typename PoolLane<T, V>::vec *__restrict__ x,
                                                          typename PoolLane<T, V>::vec *__restrict__ dx, int N, int H, int W, int CV,
                                                          int Ho, int Wo, long long total) {
    using L = PoolLane<T, V>;
    for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < total;
         idx += (long long)gridDim.x * blockDim.x) {
        int cv, n, h, w;
        pool_pixel(idx, CV, H, W, cv, n, h, w);
        const int kh0 = (h & 1) ? 0 : 1, kw0 = (w & 1) ? 0 : 1;
        const int khs[2] = {kh0, 2}, kws[2] = {kw0, 2};
        const int hos[2] = {(h + 1 - kh0) >> 1, (h - 1) >> 1}, wos[2] = {(w + 1 - kw0) >> 1, (w - 1) >> 1};
        const bool hv[2] = {hos[0] < Ho, (h & 1) && hos[1] < Ho}, wv[2] = {wos[0] < Wo, (w & 1) && wos[1] < Wo};
        const typename L::vec xraw = x[idx];
        typename L::vec dyr[4];
        typename L::amax_t am[4];
        uint32_t tap[4];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int q = 2 * i + j;
                const bool live = hv[i] && wv[j];
                tap[q] = live ? (uint32_t)(khs[i] * 3 + kws[j]) : 0xFFu;
                dyr[q] = {};
                am[q] = {};
                if (live) {
                    const long long o = ((long long)(n * Ho + hos[i]) * Wo + wos[j]) * CV + cv;
                    am[q] = amax[o];
                    dyr[q] = dy[o];
                }
            }
        float g[V];
#pragma unroll
        for (int e = 0; e < V; ++e) g[e] = 0.0f;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float d[V];
            L::to_f32(dyr[q], d);
#pragma unroll
            for (int e = 0; e < V; ++e)
                if (tap_of(am[q], e) == tap[q]) g[e] += d[e];
        }
        float xv[V];
        L::to_f32(xraw, xv);
#pragma unroll
        for (int e = 0; e < V; ++e) g[e] = xv[e] <= 0.0f ? 0.0f : g[e];      // (a NaN pixel keeps its gradient, like the oracle's ReLU)
        dx[idx] = L::from_f32(g);
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

// V channels per lane need C % V == 0, every tensor aligned to its V * sizeof(T)-byte vector and the argmax buffer to its V bytes
template <class T, int V>
static bool pool_fits(int C, const void *argmax, const void *t0, const void *t1, const void *t2 = nullptr) {
    const uintptr_t tensors = (uintptr_t)t0 | (uintptr_t)t1 | (uintptr_t)t2;
    return C % V == 0 && tensors % (V * sizeof(T)) == 0 && (uintptr_t)argmax % V == 0;
}

template <class T, int V>
static void maxpool_fwd_launch(const T *x, T *y, uint8_t *argmax, int N, int H, int W, int C, int Ho, int Wo, void *stream) {
    using L = PoolLane<T, V>;
    const long long total = (long long)N * Ho * Wo * (C / V);
    hipLaunchKernelGGL((maxpool_fwd_kernel<T, V>), dim3(capped_grid(total, 256, 8192)), dim3(256), 0, (hipStream_t)stream,
                       (const typename L::vec *)x, (typename L::vec *)y, (typename L::amax_t *)argmax, N, H, W, C / V, Ho, Wo, total);
}

template <class T, int V>
static void maxpool_bwd_launch(const T *dy, const uint8_t *argmax, const T *x, T *dx, int N, int H, int W, int C, int Ho, int Wo,
                               void *stream) {
    using L = PoolLane<T, V>;
    const long long total = (long long)N * H * W * (C / V);
    hipLaunchKernelGGL((maxpool_bwd_kernel<T, V>), dim3(capped_grid(total, 256, 8192)), dim3(256), 0, (hipStream_t)stream,
                       (const typename L::vec *)dy, (const typename L::amax_t *)argmax, (const typename L::vec *)x, (typename L::vec *)dx, N,
                       H, W, C / V, Ho, Wo, total);
}

}  // namespace detr

using namespace detr;

extern "C" int detr_hip_maxpool3x3s2_fwd_f32(const float *x, float *y, uint8_t *argmax, int32_t N, int32_t H, int32_t W,
                                             int32_t C, int32_t Ho, int32_t Wo, void *stream) {
    DETR_REQUIRE(x && y && argmax, "maxpool fwd: null operand");
    DETR_REQUIRE((long long)N * H * W <= INT32_MAX, "maxpool fwd: N * H * W = %lld input pixels do not fit in 31 bits (the kernels index pixels in int)", (long long)N * H * W);
    DETR_REQUIRE(Ho == (H + 2 - 3) / 2 + 1 && Wo == (W + 2 - 3) / 2 + 1, "maxpool fwd: bad output size");
    maxpool_fwd_launch<float, 1>(x, y, argmax, N, H, W, C, Ho, Wo, stream);       // any C, no alignment demand
    DETR_LAUNCH_CHECK("maxpool fwd");
    return 0;
}

extern "C" int detr_hip_maxpool3x3s2_bwd_f32(const float *dy, const uint8_t *argmax, const float *x, float *dx, int32_t N,
                                             int32_t H, int32_t W, int32_t C, int32_t Ho, int32_t Wo, void *stream) {
    DETR_REQUIRE(dy && argmax && x && dx, "maxpool bwd: null operand");
    DETR_REQUIRE((long long)N * H * W <= INT32_MAX, "maxpool bwd: N * H * W = %lld input pixels do not fit in 31 bits (the kernels index pixels in int)", (long long)N * H * W);
    DETR_REQUIRE((pool_fits<float, 4>(C, argmax, dy, x, dx)), "maxpool bwd: C must be a multiple of 4 and the tensors 16-byte aligned");
    maxpool_bwd_launch<float, 4>(dy, argmax, x, dx, N, H, W, C, Ho, Wo, stream);
    DETR_LAUNCH_CHECK("maxpool bwd");
    return 0;
}

extern "C" int detr_hip_subsample2_fwd_f32(const float *x, float *y, int32_t N, int32_t H, int32_t W, int32_t C,
                                           int32_t Ho, int32_t Wo, void *stream) {
    DETR_REQUIRE(x && y && C % 4 == 0 && aligned16(x) && aligned16(y), "subsample2 fwd: bad operands");
    DETR_REQUIRE(Ho == (H - 1) / 2 + 1 && Wo == (W - 1) / 2 + 1, "subsample2 fwd: bad output size");
    const long long total = (long long)N * Ho * Wo * (C / 4);
    hipLaunchKernelGGL(subsample2_fwd_kernel, dim3(capped_grid(total, 256, 8192)), dim3(256), 0, (hipStream_t)stream,
                       (const float4 *)x, (float4 *)y, H, W, C / 4, Ho, Wo, total);
    DETR_LAUNCH_CHECK("subsample2 fwd");
    return 0;
}

extern "C" int detr_hip_subsample2_bwd_f32(const float *dy, float *dx, int32_t N, int32_t H, int32_t W, int32_t C,
                                           int32_t Ho, int32_t Wo, void *stream) {
    DETR_REQUIRE(dy && dx && C % 4 == 0 && aligned16(dy) && aligned16(dx), "subsample2 bwd: bad operands");
    const long long total = (long long)N * H * W * (C / 4);
    hipLaunchKernelGGL(subsample2_bwd_kernel, dim3(capped_grid(total, 256, 8192)), dim3(256), 0, (hipStream_t)stream,
                       (const float4 *)dy, (float4 *)dx, H, W, C / 4, Ho, Wo, total);
    DETR_LAUNCH_CHECK("subsample2 bwd");
    return 0;
}

extern "C" int detr_hip_maxpool3x3s2_fwd_bf16(const uint16_t *x, uint16_t *y, uint8_t *argmax, int32_t N, int32_t H, int32_t W,
                                              int32_t C, int32_t Ho, int32_t Wo, void *stream) {
    DETR_REQUIRE(x && y && argmax && C % 4 == 0, "maxpool fwd bf16: bad operands");
    DETR_REQUIRE((long long)N * H * W <= INT32_MAX, "maxpool fwd bf16: N * H * W = %lld input pixels do not fit in 31 bits (the kernels index pixels in int)", (long long)N * H * W);
    DETR_REQUIRE((pool_fits<uint16_t, 4>(C, argmax, x, y)), "maxpool fwd bf16: alignment");
    DETR_REQUIRE(Ho == (H + 2 - 3) / 2 + 1 && Wo == (W + 2 - 3) / 2 + 1, "maxpool fwd: bad output size");
    if (pool_fits<uint16_t, 8>(C, argmax, x, y)) {
        maxpool_fwd_launch<uint16_t, 8>(x, y, argmax, N, H, W, C, Ho, Wo, stream);
        DETR_LAUNCH_CHECK("maxpool fwd bf16 (8 channels per lane)");
        return 0;
    }
    maxpool_fwd_launch<uint16_t, 4>(x, y, argmax, N, H, W, C, Ho, Wo, stream);
    DETR_LAUNCH_CHECK("maxpool fwd bf16");
    return 0;
}

extern "C" int detr_hip_maxpool3x3s2_bwd_bf16(const uint16_t *dy, const uint8_t *argmax, const uint16_t *x, uint16_t *dx, int32_t N,
                                              int32_t H, int32_t W, int32_t C, int32_t Ho, int32_t Wo, void *stream) {
    DETR_REQUIRE(dy && argmax && x && dx && C % 4 == 0, "maxpool bwd bf16: bad operands");
    DETR_REQUIRE((long long)N * H * W <= INT32_MAX, "maxpool bwd bf16: N * H * W = %lld input pixels do not fit in 31 bits (the kernels index pixels in int)", (long long)N * H * W);
    DETR_REQUIRE((pool_fits<uint16_t, 4>(C, argmax, dy, x, dx)), "maxpool bwd bf16: alignment");
    if (pool_fits<uint16_t, 8>(C, argmax, dy, x, dx)) {
        maxpool_bwd_launch<uint16_t, 8>(dy, argmax, x, dx, N, H, W, C, Ho, Wo, stream);
        DETR_LAUNCH_CHECK("maxpool bwd bf16 (8 channels per lane)");
        return 0;
    }
    maxpool_bwd_launch<uint16_t, 4>(dy, argmax, x, dx, N, H, W, C, Ho, Wo, stream);
    DETR_LAUNCH_CHECK("maxpool bwd bf16");
    return 0;
}

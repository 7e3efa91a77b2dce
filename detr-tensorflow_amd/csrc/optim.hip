// optim.hip -- multi-tensor optimiser step on a flat fp32 parameter buffer:
// per-TENSOR clip-by-norm (Keras `clipnorm`, i.e. tf.clip_by_norm) followed by Keras Adam
// (detr_tf/optimizers.py:86-88,137-163).  One launch computes every tensor's sum of squares,
// one launch applies clip + Adam to all tensors; HBM-bound (reads g,m,v,p; writes m,v,p).
// Opt-in second family (below): AdamW -- decoupled weight decay -- with the clip taken per tensor or over ONE norm of every
// trained tensor (partials, a one-workgroup finalize, one update launch for all groups).
#include "common.h"

namespace detr {

__global__ __launch_bounds__(256) void sumsq_segments_kernel(const float *__restrict__ g,
                                                             const int *__restrict__ chunk_tensor,
                                                             const long long *__restrict__ chunk_start,
                                                             const long long *__restrict__ seg_end, int chunk,
                                                             float *__restrict__ sumsq) {
    __shared__ float red[4];
    const int c = blockIdx.x;
    const int t = chunk_tensor[c];
    const long long s0 = chunk_start[c];
    long long s1 = s0 + chunk;
    if (s1 > seg_end[t]) s1 = seg_end[t];
    float acc = 0.f;
    for (long long i = s0 + threadIdx.x; i < s1; i += blockDim.x) {
        const float v = g[i];
        acc += v * v;
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    // one partial per chunk, plain store: the per-tensor sum is formed in a FIXED order by clip_adam_kernel, so that every
    // data-parallel replica (and every replay) clips with bit-identical norms -- fp32 atomics here made replicas drift by ulps
    if (threadIdx.x == 0) sumsq[c] = (red[0] + red[1]) + (red[2] + red[3]);
}

// tf.clip_by_norm / tf.clip_by_global_norm: clip / max(nrm, clip), exactly 1 when nrm <= clip.  Not fmaxf(), which ignores a NaN
// operand: a NaN norm (one NaN gradient element) must give a NaN factor, so that the update poisons what the reference's does
// instead of going through unclipped.  An Inf norm gives 0, as the formula does.
__device__ __forceinline__ float clip_factor(float nrm, float clip) { return nrm > clip ? clip / nrm : (nrm == nrm ? 1.0f : nrm); }

__global__ __launch_bounds__(256) void clip_adam_kernel(float *__restrict__ param, const float *__restrict__ g,
                                                        float *__restrict__ m, float *__restrict__ v,
                                                        const int *__restrict__ chunk_tensor,
                                                        const long long *__restrict__ chunk_start,
                                                        const long long *__restrict__ seg_end,
                                                        const int *__restrict__ tensor_group,
                                                        const float *__restrict__ sumsq,
                                                        const float *__restrict__ hyper, int chunk, int n_chunks) {
    const int c = blockIdx.x;
    const int t = chunk_tensor[c];
    const long long s0 = chunk_start[c];
    long long s1 = s0 + chunk;
    if (s1 > seg_end[t]) s1 = seg_end[t];
    const int grp = tensor_group[t];
    if (grp < 0) return;                       // group not trained this step (config.train_<group> false)
    const float lr_t = hyper[grp];
    const float clip = hyper[3], b1 = hyper[4], b2 = hyper[5], eps = hyper[6];
    // tf.clip_by_norm: g * clip / max(||g||, clip)   (clip <= 0 disables)
    float cs = 1.0f;
    if (clip > 0.f) {
        // the chunks of tensor t are consecutive: [lo, hi) by binary search, partials summed in a fixed order
        __shared__ int s_lo, s_hi;
        __shared__ float s_red[4];
        if (threadIdx.x == 0) {
            int a = 0, b = c;                      // first index with chunk_tensor >= t  (chunk_tensor[c] == t)
            while (a < b) { const int mid = (a + b) >> 1; if (chunk_tensor[mid] < t) a = mid + 1; else b = mid; }
            s_lo = a;
            a = c; b = n_chunks;                   // first index with chunk_tensor > t
            while (a < b) { const int mid = (a + b) >> 1; if (chunk_tensor[mid] <= t) a = mid + 1; else b = mid; }
            s_hi = a;
        }
        __syncthreads();
        float acc = 0.f;
        for (int k = s_lo + (int)threadIdx.x; k < s_hi; k += blockDim.x) acc += sumsq[k];
        acc = wave_sum(acc);
        if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = acc;
        __syncthreads();
        const float nrm = sqrtf((s_red[0] + s_red[1]) + (s_red[2] + s_red[3]));
        cs = clip_factor(nrm, clip);
    }
    for (long long i = s0 + threadIdx.x; i < s1; i += blockDim.x) {
        const float gi = g[i] * cs;
        const float mi = b1 * m[i] + (1.0f - b1) * gi;
        const float vi = b2 * v[i] + (1.0f - b2) * gi * gi;
        m[i] = mi;
        v[i] = vi;
        param[i] = param[i] - lr_t * mi / (sqrtf(vi) + eps);
    }
}

__global__ void set_floats8_kernel(float *dst, float v0, float v1, float v2, float v3, float v4, float v5, float v6,
                                   float v7) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        dst[0] = v0; dst[1] = v1; dst[2] = v2; dst[3] = v3; dst[4] = v4; dst[5] = v5; dst[6] = v6; dst[7] = v7;
    }
}

// ---- AdamW with one MODEL-WIDE gradient norm (tf.keras.optimizers.AdamW + tf.clip_by_global_norm) ------------------
// hyper16 (device): [0..2] bias-corrected step size per group, [3] clip threshold (per tensor, or over all trained
// tensors in the joint mode), [4] beta1, [5] beta2, [6] eps, [7] weight decay, [8..10] plain learning rate per group,
// [11..13] 1 = group trained this step, [14..15] unused.  The first seven are the block of clip_adam_kernel.
struct Floats16 { float v[16]; };

__global__ void set_floats16_kernel(float *dst, Floats16 f) {
    if (blockIdx.x == 0 && threadIdx.x < 16) dst[threadIdx.x] = f.v[threadIdx.x];
}

// ONE workgroup turns the per-chunk partials of every trained tensor into scale[0] = clip / max(G, clip) and scale[1] = G.
// Thread i adds partials i, i + 256, ... in that order, then the 256 lane sums are combined as in sumsq_segments_kernel:
// the order depends on nothing but n_chunks, so replays and data-parallel replicas get the same bits.  ~5000 partials of a
// ResNet-50 DETR are 20 loads per thread; the 5000 workgroups of the update then read two floats each.
__global__ __launch_bounds__(256) void global_clip_scale_kernel(const float *__restrict__ sumsq,
                                                                const int *__restrict__ chunk_tensor,
                                                                const int *__restrict__ tensor_group,
                                                                const float *__restrict__ hyper, int n_chunks,
                                                                float *__restrict__ scale) {
    __shared__ float red[4];
    float acc = 0.f;
    for (int k = threadIdx.x; k < n_chunks; k += 256) {
        const int grp = tensor_group[chunk_tensor[k]];
        if (grp >= 0 && hyper[11 + grp] != 0.f) acc += sumsq[k];
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        const float clip = hyper[3];
        const float nrm = sqrtf((red[0] + red[1]) + (red[2] + red[3]));
        scale[0] = clip > 0.f ? clip_factor(nrm, clip) : 1.0f;
        scale[1] = nrm;
    }
}

__device__ __forceinline__ void adamw_elem(float &p, float gi, float &m, float &v, float cs, float b1, float b2,
                                           float eps, float lr_t, float lr_wd) {
    // every operation rounded on its own: whether the compiler fuses a multiply into an add depends on how it unrolls and
    // vectorises the loop around this (clip_adam_kernel's paired and remainder iterations differ that way), and the 16-byte
    // body, the scalar tail and the two instantiations below must give the same bits for the same element
#pragma clang fp contract(off)
    gi = gi * cs;
    const float mi = b1 * m + (1.0f - b1) * gi;
    const float vi = b2 * v + (1.0f - b2) * gi * gi;
    m = mi;
    v = vi;
    p = p - lr_wd * p;                           // decoupled decay: the plain learning rate, not the bias-corrected step
    p = p - lr_t * mi / (sqrtf(vi) + eps);
}

// Clip + decay + Adam on one chunk per workgroup, every trained group in one launch.  JOINT: the clip factor is the one
// global_clip_scale_kernel left in scale[0]; otherwise the tensor's own norm, re-reduced as in clip_adam_kernel.
// A pure stream (reads g, m, v, p; writes m, v, p): 16-byte loads and stores where the chunk starts on a 16-byte boundary
// (the parameter store aligns every tensor to 8 floats and chunks are multiples of 4), scalar code for the tail.
template <bool JOINT>
__global__ __launch_bounds__(256) void adamw_kernel(float *__restrict__ param, const float *__restrict__ g,
                                                    float *__restrict__ m, float *__restrict__ v,
                                                    const int *__restrict__ chunk_tensor,
                                                    const long long *__restrict__ chunk_start,
                                                    const long long *__restrict__ seg_end,
                                                    const int *__restrict__ tensor_group,
                                                    const float *__restrict__ sumsq, const float *__restrict__ hyper,
                                                    const float *__restrict__ scale, int chunk, int n_chunks,
                                                    int aligned16) {
    const int c = blockIdx.x;
    const int t = chunk_tensor[c];
    const long long s0 = chunk_start[c];
    long long s1 = s0 + chunk;
    if (s1 > seg_end[t]) s1 = seg_end[t];
    const int grp = tensor_group[t];
    if (grp < 0 || hyper[11 + grp] == 0.f) return;      // group not trained this step (uniform over the workgroup)
    const float lr_t = hyper[grp];
    const float clip = hyper[3], b1 = hyper[4], b2 = hyper[5], eps = hyper[6];
    const float lr_wd = hyper[8 + grp] * hyper[7];
    float cs = 1.0f;
    if (JOINT) {
        cs = scale[0];
    } else if (clip > 0.f) {
        __shared__ int s_lo, s_hi;
        __shared__ float s_red[4];
        if (threadIdx.x == 0) {
            int a = 0, b = c;                      // first index with chunk_tensor >= t  (chunk_tensor[c] == t)
            while (a < b) { const int mid = (a + b) >> 1; if (chunk_tensor[mid] < t) a = mid + 1; else b = mid; }
            s_lo = a;
            a = c; b = n_chunks;                   // first index with chunk_tensor > t
            while (a < b) { const int mid = (a + b) >> 1; if (chunk_tensor[mid] <= t) a = mid + 1; else b = mid; }
            s_hi = a;
        }
        __syncthreads();
        float acc = 0.f;
        for (int k = s_lo + (int)threadIdx.x; k < s_hi; k += blockDim.x) acc += sumsq[k];
        acc = wave_sum(acc);
        if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = acc;
        __syncthreads();
        const float nrm = sqrtf((s_red[0] + s_red[1]) + (s_red[2] + s_red[3]));
        cs = clip_factor(nrm, clip);
    }
    long long i0 = s0;
    if (aligned16 && (s0 & 3) == 0) {
        const long long nvec = (s1 - s0) >> 2;
        float4 *__restrict__ p4 = reinterpret_cast<float4 *>(param + s0);
        float4 *__restrict__ m4 = reinterpret_cast<float4 *>(m + s0);
        float4 *__restrict__ v4 = reinterpret_cast<float4 *>(v + s0);
        const float4 *__restrict__ g4 = reinterpret_cast<const float4 *>(g + s0);
        for (long long j = threadIdx.x; j < nvec; j += blockDim.x) {
            const float4 gg = g4[j];
            float4 pp = p4[j], mm = m4[j], vv = v4[j];
            adamw_elem(pp.x, gg.x, mm.x, vv.x, cs, b1, b2, eps, lr_t, lr_wd);
            adamw_elem(pp.y, gg.y, mm.y, vv.y, cs, b1, b2, eps, lr_t, lr_wd);
            adamw_elem(pp.z, gg.z, mm.z, vv.z, cs, b1, b2, eps, lr_t, lr_wd);
            adamw_elem(pp.w, gg.w, mm.w, vv.w, cs, b1, b2, eps, lr_t, lr_wd);
            m4[j] = mm;
            v4[j] = vv;
            p4[j] = pp;
        }
        i0 = s0 + (nvec << 2);
    }
    for (long long i = i0 + threadIdx.x; i < s1; i += blockDim.x) {
        float pi = param[i], mi = m[i], vi = v[i];
        adamw_elem(pi, g[i], mi, vi, cs, b1, b2, eps, lr_t, lr_wd);
        m[i] = mi;
        v[i] = vi;
        param[i] = pi;
    }
}

// ---- exponential moving average of the weights (tf.train.ExponentialMovingAverage) ----------------------------------
// TensorFlow's form, shadow -= (1 - decay) * (shadow - param), as three operations that are each rounded on their own: the
// 16-byte body, the scalar tail and a NumPy float32 restatement then give the same bits.
__device__ __forceinline__ float ema_elem(float s, float p, float omd) {
#pragma clang fp contract(off)
    float t = s - p;
    t = omd * t;
    return s - t;
}

// One chunk per workgroup, the tables of adamw_kernel (the chunk list of the trained groups).  omd = 1 - decay is read from
// device memory, so a replayed launch sees this step's value.  A pure stream: reads param and shadow, writes shadow; what
// no chunk lists (alignment gaps, tensors of untrained groups) is not touched.
__global__ __launch_bounds__(256) void ema_kernel(float *__restrict__ shadow, const float *__restrict__ param,
                                                  const int *__restrict__ chunk_tensor,
                                                  const long long *__restrict__ chunk_start,
                                                  const long long *__restrict__ seg_end,
                                                  const float *__restrict__ hyper, int chunk, int aligned16) {
    const int c = blockIdx.x;
    const int t = chunk_tensor[c];
    const long long s0 = chunk_start[c];
    long long s1 = s0 + chunk;
    if (s1 > seg_end[t]) s1 = seg_end[t];
    const float omd = hyper[0];
    long long i0 = s0;
    if (aligned16 && (s0 & 3) == 0) {
        const long long nvec = (s1 - s0) >> 2;
        float4 *__restrict__ s4 = reinterpret_cast<float4 *>(shadow + s0);
        const float4 *__restrict__ p4 = reinterpret_cast<const float4 *>(param + s0);
        for (long long j = threadIdx.x; j < nvec; j += blockDim.x) {
            const float4 pp = p4[j];
            float4 ss = s4[j];
            ss.x = ema_elem(ss.x, pp.x, omd);
            ss.y = ema_elem(ss.y, pp.y, omd);
            ss.z = ema_elem(ss.z, pp.z, omd);
            ss.w = ema_elem(ss.w, pp.w, omd);
            s4[j] = ss;
        }
        i0 = s0 + (nvec << 2);
    }
    for (long long i = i0 + threadIdx.x; i < s1; i += blockDim.x) shadow[i] = ema_elem(shadow[i], param[i], omd);
}

// a[i] <-> b[i] over two disjoint ranges: nvec 16-byte pairs (only when both pointers are 16-byte aligned), then the scalar
// tail [4 * nvec, n).  Grid-stride with 64-bit indices: n may exceed 2^31 bytes.
__global__ __launch_bounds__(256) void exchange_kernel(float *__restrict__ a, float *__restrict__ b, long long n,
                                                       long long nvec) {
    const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long stride = (long long)gridDim.x * blockDim.x;
    float4 *__restrict__ a4 = reinterpret_cast<float4 *>(a);
    float4 *__restrict__ b4 = reinterpret_cast<float4 *>(b);
    for (long long j = tid; j < nvec; j += stride) {
        const float4 x = a4[j], y = b4[j];
        a4[j] = y;
        b4[j] = x;
    }
    for (long long i = (nvec << 2) + tid; i < n; i += stride) {
        const float x = a[i], y = b[i];
        a[i] = y;
        b[i] = x;
    }
}

}  // namespace detr

using namespace detr;

extern "C" int detr_hip_ema_f32(float *shadow, const float *param, const int32_t *chunk_tensor, const int64_t *chunk_start,
                                const int64_t *seg_end, const float *hyper, int32_t n_chunks, int32_t chunk, void *stream) {
    DETR_REQUIRE(shadow && param && chunk_tensor && chunk_start && seg_end && hyper, "ema: null operand");
    DETR_REQUIRE(shadow != param, "ema: shadow and param are the same buffer");
    DETR_REQUIRE(n_chunks > 0 && chunk > 0, "ema: bad chunking");
    const int aligned16 = (((uintptr_t)shadow | (uintptr_t)param) & 15) == 0;       // the rule of detr_hip_adamw_f32
    hipLaunchKernelGGL(ema_kernel, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, shadow, param, chunk_tensor,
                       reinterpret_cast<const long long *>(chunk_start), reinterpret_cast<const long long *>(seg_end), hyper,
                       chunk, aligned16);
    DETR_LAUNCH_CHECK("ema");
    return 0;
}

extern "C" int detr_hip_exchange_f32(float *a, float *b, int64_t n, void *stream) {
    DETR_REQUIRE(a && b, "exchange: null operand");
    DETR_REQUIRE(n > 0, "exchange: bad length");
    const uintptr_t ua = (uintptr_t)a, ub = (uintptr_t)b, bytes = (uintptr_t)n * 4;
    DETR_REQUIRE(ua + bytes <= ub || ub + bytes <= ua, "exchange: the two ranges overlap");
    const long long nvec = ((ua | ub) & 15) == 0 ? (long long)(n >> 2) : 0;
    const long long work = nvec > 0 ? nvec + (n & 3) : (long long)n;
    long long blocks = (work + 255) / 256;
    if (blocks > 2048) blocks = 2048;                    // 256 CUs x 8 workgroups; the rest of the range by grid stride
    hipLaunchKernelGGL(exchange_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a, b, (long long)n, nvec);
    DETR_LAUNCH_CHECK("exchange");
    return 0;
}

extern "C" int detr_hip_set_floats16_f32(float *dst, const float *values, void *stream) {
    DETR_REQUIRE(dst && values, "set_floats16: null operand");
    Floats16 f;
    for (int i = 0; i < 16; ++i) f.v[i] = values[i];
    hipLaunchKernelGGL(set_floats16_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, dst, f);
    DETR_LAUNCH_CHECK("set_floats16");
    return 0;
}

extern "C" int detr_hip_global_clip_scale_f32(const float *sumsq, const int32_t *chunk_tensor,
                                              const int32_t *tensor_group, const float *hyper, int32_t n_chunks,
                                              float *scale, void *stream) {
    DETR_REQUIRE(sumsq && chunk_tensor && tensor_group && hyper && scale, "global_clip_scale: null operand");
    DETR_REQUIRE(n_chunks > 0, "global_clip_scale: bad chunking");
    hipLaunchKernelGGL(global_clip_scale_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, sumsq, chunk_tensor,
                       tensor_group, hyper, n_chunks, scale);
    DETR_LAUNCH_CHECK("global_clip_scale");
    return 0;
}

extern "C" int detr_hip_adamw_f32(float *param, const float *g, float *m, float *v, const int32_t *chunk_tensor,
                                  const int64_t *chunk_start, const int64_t *seg_end, const int32_t *tensor_group,
                                  const float *sumsq, const float *hyper, const float *scale, int32_t n_chunks,
                                  int32_t chunk, void *stream) {
    DETR_REQUIRE(param && g && m && v && chunk_tensor && chunk_start && seg_end && tensor_group && sumsq && hyper,
                 "adamw: null operand");
    DETR_REQUIRE(n_chunks > 0 && chunk > 0, "adamw: bad chunking");
    // 16-byte accesses need 16-byte aligned buffers (and a chunk start that is a multiple of 4 floats: checked per chunk)
    const int aligned16 = (((uintptr_t)param | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0;
    const auto cs = reinterpret_cast<const long long *>(chunk_start);
    const auto se = reinterpret_cast<const long long *>(seg_end);
    if (scale)
        hipLaunchKernelGGL(adamw_kernel<true>, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, param, g, m, v,
                           chunk_tensor, cs, se, tensor_group, sumsq, hyper, scale, chunk, n_chunks, aligned16);
    else
        hipLaunchKernelGGL(adamw_kernel<false>, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, param, g, m, v,
                           chunk_tensor, cs, se, tensor_group, sumsq, hyper, scale, chunk, n_chunks, aligned16);
    DETR_LAUNCH_CHECK("adamw");
    return 0;
}

extern "C" int detr_hip_set_floats8_f32(float *dst, float v0, float v1, float v2, float v3, float v4, float v5, float v6,
                                        float v7, void *stream) {
    DETR_REQUIRE(dst, "set_floats8: null dst");
    hipLaunchKernelGGL(set_floats8_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, dst, v0, v1, v2, v3, v4, v5, v6, v7);
    DETR_LAUNCH_CHECK("set_floats8");
    return 0;
}

extern "C" int detr_hip_sumsq_segments_f32(const float *g, const int32_t *chunk_tensor, const int64_t *chunk_start,
                                           const int64_t *seg_end, int32_t n_chunks, int32_t chunk, float *sumsq,
                                           void *stream) {
    DETR_REQUIRE(g && chunk_tensor && chunk_start && seg_end && sumsq && n_chunks > 0 && chunk > 0, "sumsq: bad args");
    hipLaunchKernelGGL(sumsq_segments_kernel, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, g, chunk_tensor,
                       reinterpret_cast<const long long *>(chunk_start), reinterpret_cast<const long long *>(seg_end),
                       chunk, sumsq);
    DETR_LAUNCH_CHECK("sumsq_segments");
    return 0;
}

extern "C" int detr_hip_clip_adam_f32(float *param, const float *g, float *m, float *v, const int32_t *chunk_tensor,
                                      const int64_t *chunk_start, const int64_t *seg_end, const int32_t *tensor_group,
                                      const float *sumsq, const float *hyper, int32_t n_chunks, int32_t chunk,
                                      void *stream) {
    DETR_REQUIRE(param && g && m && v && chunk_tensor && chunk_start && seg_end && tensor_group && sumsq && hyper,
                 "clip_adam: null operand");
    DETR_REQUIRE(n_chunks > 0 && chunk > 0, "clip_adam: bad chunking");
    hipLaunchKernelGGL(clip_adam_kernel, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, param, g, m, v, chunk_tensor,
                       reinterpret_cast<const long long *>(chunk_start), reinterpret_cast<const long long *>(seg_end),
                       tensor_group, sumsq, hyper, chunk, n_chunks);
    DETR_LAUNCH_CHECK("clip_adam");
    return 0;
}

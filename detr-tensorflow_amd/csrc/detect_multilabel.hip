// detect_multilabel.hip -- the K best (query, class) pairs of every image under sigmoid scoring: the multi-label rule of the
// detectors trained with a sigmoid focal class loss (Deformable DETR's PostProcess and its successors), where one query may emit
// several classes and the number of detections is bounded by K, not by Q.
//
// ONE launch serves the batch, one workgroup per image (the family rule of detections.h).  Per image:
//   1. candidates: every pair (q, c), c != background, with s = sigmoid_score(logits[q, c]) >= score_threshold (a NaN fails it).
//      s lies in [0, 1], so its fp32 bits order as an unsigned 30-bit key (1.0f = 0x3F800000 < 2^30).
//   2. a radix select over that key, three histogram passes of 10 bits in LDS (integer LDS atomics): it finds the K-th largest key,
//      the `cut`, and how many entries of exactly that key still fit, the `budget`.  With fewer than K candidates all are taken.
//   3. when more entries tie at the cut than the budget admits, a counting pass gives every wave the number of ties in the rows
//      before its own; otherwise every tie is taken and the pass is skipped.
//   4. one collecting pass takes every key above the cut and the first `budget` ties in flat order q * C + c.
//   5. the at most 1024 survivors are ordered by det_before on (score, flat index): np.argsort(-s, kind="stable") over the
//      flattened row-major scores.  The slots of step 4 come from an LDS counter, in no fixed order; the order of the OUTPUT
//      depends on (score, flat index) alone, so a rerun gives identical bytes.  No float atomics.
//   6. rows: label = c, score = s, query = q, and the box of query q from the box stage -- pixels of the image's own size with the
//      helpers detect_kernel uses (detr_hip_detect_multilabel), or normalised in detr_hip_postprocess's formats and arithmetic
//      (detr_hip_postprocess_multilabel).  Rows [counts[b], K) of every output are zero.
// The keys are not kept: every pass re-reads the image's logits (about 110 KB at 300 x 92, resident in L2) and scores them again,
// 3 + 1 passes, 5 with the counting pass.  Wave w owns the queries [Q * w / 4, Q * (w + 1) / 4): it walks them in flat order, so
// steps 3 and 4 need no workgroup barrier per step.
#include "detections.h"

namespace detr {

constexpr int ML_BITS = 10, ML_BUCKETS = 1 << ML_BITS, ML_PASSES = 3;       // 3 x 10 bits cover the keys of [0.0f, 1.0f]

struct MultilabelArgs {
    const float *logits; long long sl_b, sl_q;      // [B, Q, C]
    const float *boxes; long long sb_b, sb_q;       // [B, Q, 4] cx, cy, w, h
    int Q, C, background, K;
    float thr;
    float *out_boxes;                               // [B, K, 4]
    long long *out_labels;                          // [B, K]
    float *out_scores;                              // [B, K]
    int *out_query;                                 // [B, K] or nullptr
    int *counts;                                    // [B]
};

// the box stage of detr_hip_detect_multilabel: detect_kernel's, the whole image is the window
struct PixelBoxStage {
    const int *sizes;                               // [B, 2] height, width
    int fmt, clip;
    __device__ __forceinline__ float4 operator()(int b, const float *bx) const {
        const float H = (float)sizes[2 * b], W = (float)sizes[2 * b + 1];
        return emit_pixel_box(fmt, decode_pixel_box(bx, -0.f, -0.f, W, H, W, H, clip), bx, -0.f, -0.f, W, H);
    }
};

// the box stage of detr_hip_postprocess_multilabel: postprocess_kernel's formats and arithmetic (w / 2 is exact, so the
// differences and sums are single roundings however they are contracted)
struct UnitBoxStage {
    int fmt;                                        // 0 xy_center, 1 xyxy (clipped to [0, 1]), 2 yxyx (clipped)
    __device__ __forceinline__ float4 operator()(int, const float *bx) const {
        const float cx = bx[0], cy = bx[1], w = bx[2], h = bx[3];
        if (fmt == 0) return make_float4(cx, cy, w, h);
        const float x0 = fminf(fmaxf(cx - w / 2, 0.f), 1.f), y0 = fminf(fmaxf(cy - h / 2, 0.f), 1.f);
        const float x1 = fminf(fmaxf(cx + w / 2, 0.f), 1.f), y1 = fminf(fmaxf(cy + h / 2, 0.f), 1.f);
        return fmt == 1 ? make_float4(x0, y0, x1, y1) : make_float4(y0, x0, y1, x1);
    }
};

// The pairs of the queries [q_lo, q_hi) in flat order, 64 classes per step: visit(q, c, key, ok) runs in ALL lanes of the wave
// (ok = false where there is no candidate), so it may ballot.  key = the bits of the score; a 0.0f score has key 0 and ok set.
// One wave is alone on its SIMD, so nothing hides a load but the wave's own further loads: ML_AHEAD steps are fetched before the
// first of them is scored.  A lane without a pair (c >= C, the background column, behind the last step) holds a NaN, which
// scores NaN and fails the threshold like a NaN logit.
constexpr int ML_AHEAD = 8;
template <class Visit>
__device__ __forceinline__ void visit_pairs(const float *lg, long long sl_q, int q_lo, int q_hi, int C, int background, float thr,
                                            Visit visit) {
    const int lane = threadIdx.x & 63;
    const int steps = (q_hi - q_lo) * ((C + 63) >> 6);
    int q = q_lo, c0 = 0;                            // the step about to be visited
    for (int t0 = 0; t0 < steps; t0 += ML_AHEAD) {
        float x[ML_AHEAD];
        int fq = q, fc0 = c0;                        // the step about to be fetched
#pragma unroll
        for (int u = 0; u < ML_AHEAD; ++u) {
            const int c = fc0 + lane;
            x[u] = (t0 + u < steps && c < C && c != background) ? lg[fq * sl_q + c] : NAN;
            fc0 += 64;
            if (fc0 >= C) { fc0 = 0; ++fq; }
        }
        float s[ML_AHEAD];                           // scored together: ML_AHEAD independent chains of expf and division to interleave
#pragma unroll
        for (int u = 0; u < ML_AHEAD; ++u) s[u] = sigmoid_score(x[u]);
#pragma unroll
        for (int u = 0; u < ML_AHEAD; ++u) {
            if (t0 + u >= steps) break;
            visit(q, c0 + lane, __float_as_uint(s[u]), s[u] >= thr);  // a NaN score fails the threshold
            c0 += 64;
            if (c0 >= C) { c0 = 0; ++q; }
        }
    }
}

template <class BoxStage>
__global__ __launch_bounds__(DET_THREADS) void detect_multilabel_kernel(MultilabelArgs a, BoxStage box_of) {
    __shared__ int s_hist[ML_BUCKETS];
    __shared__ unsigned s_key[PP_MAXQ];          // the survivors: score bits ...
    __shared__ int s_flat[PP_MAXQ];              // ... and flat index q * C + c
    __shared__ int s_order[PP_MAXQ];             // s_order[rank] = survivor
    __shared__ int s_wave_cnt[4];
    __shared__ int s_sel[3];                     // the selected bucket, what is still wanted inside it, its population
    __shared__ int s_slots;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float *lg = a.logits + b * a.sl_b;
    const int q_lo = (int)((long long)a.Q * wave / 4), q_hi = (int)((long long)a.Q * (wave + 1) / 4);
    const unsigned long long below = (1ull << lane) - 1ull;

    // ---- 2. radix select: `cut` = the K-th largest key, `budget` = how many entries equal to it are wanted, `ties` = how many there are
    unsigned cut = 0u;
    int budget = a.K, ties = 0;
    for (int pass = 0; pass < ML_PASSES; ++pass) {
        const int shift = ML_BITS * (ML_PASSES - 1 - pass);
        for (int i = tid; i < ML_BUCKETS; i += DET_THREADS) s_hist[i] = 0;
        __syncthreads();
        visit_pairs(lg, a.sl_q, q_lo, q_hi, a.C, a.background, a.thr, [&](int, int, unsigned key, bool ok) {
            ok = ok && (pass == 0 || (key >> (shift + ML_BITS)) == cut);      // the digits found so far
            const int bucket = (int)((key >> shift) & (ML_BUCKETS - 1));
            const unsigned long long m = __ballot(ok);
            if (m == 0ull) return;
            // a wave whose entries all fall into one bucket (an image of equal scores) adds once instead of 64 times to one address
            const int first = __shfl(bucket, __ffsll((long long)m) - 1, 64);
            if (__ballot(ok && bucket == first) == m) {
                if (lane == 0) atomicAdd(&s_hist[first], __popcll(m));
            } else if (ok) {
                atomicAdd(&s_hist[bucket], 1);
            }
        });
        __syncthreads();
        // thread t owns the buckets 4t .. 4t + 3; `incl` = the entries in the buckets >= 4t, `excl` = in the buckets >= 4t + 4
        int h[4], own = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) { h[k] = s_hist[4 * tid + k]; own += h[k]; }
        int suf = own;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int v = __shfl_down(suf, o, 64);
            if (lane + o < 64) suf += v;
        }
        if (lane == 0) s_wave_cnt[wave] = suf;
        __syncthreads();
        int incl = suf;
        for (int w = wave + 1; w < 4; ++w) incl += s_wave_cnt[w];
        const int total = s_wave_cnt[0] + s_wave_cnt[1] + s_wave_cnt[2] + s_wave_cnt[3];
        const int excl = incl - own;
        if (excl < budget && budget <= incl) {                                  // exactly one thread, when total >= budget
            int run = excl;
#pragma unroll
            for (int k = 3; k >= 0; --k) {
                if (run < budget && budget <= run + h[k]) { s_sel[0] = 4 * tid + k; s_sel[1] = budget - run; s_sel[2] = h[k]; }
                run += h[k];
            }
        }
        __syncthreads();
        if (total < budget) {            // fewer candidates than K (the first pass only; later the bucket holds >= budget): take them all
            cut = 0u; budget = INT_MAX; ties = 0;
            break;
        }
        cut = (cut << ML_BITS) | (unsigned)s_sel[0];
        budget = s_sel[1];
        ties = s_sel[2];
    }

    // ---- 3. more ties at the cut than wanted: the first `budget` in flat order win, so a wave must know the ties before its rows
    int tie_seen = 0;
    if (tid == 0) s_slots = 0;
    if (ties > budget) {
        int mine = 0;
        visit_pairs(lg, a.sl_q, q_lo, q_hi, a.C, a.background, a.thr,
                    [&](int, int, unsigned key, bool ok) { mine += __popcll(__ballot(ok && key == cut)); });
        if (lane == 0) s_wave_cnt[wave] = mine;
        __syncthreads();
        for (int w = 0; w < wave; ++w) tie_seen += s_wave_cnt[w];
    }
    __syncthreads();

    // ---- 4. collect: every key above the cut, and the ties while the budget lasts
    visit_pairs(lg, a.sl_q, q_lo, q_hi, a.C, a.background, a.thr, [&](int q, int c, unsigned key, bool ok) {
        const bool tie = ok && key == cut;
        const unsigned long long mt = __ballot(tie);
        const bool keep = tie ? tie_seen + __popcll(mt & below) < budget : (ok && key > cut);
        tie_seen += __popcll(mt);
        const unsigned long long mk = __ballot(keep);
        if (mk == 0ull) return;
        int base = 0;
        if (lane == 0) base = atomicAdd(&s_slots, __popcll(mk));
        base = __shfl(base, 0, 64);
        const int slot = base + __popcll(mk & below);
        if (keep && slot < PP_MAXQ) {                // the selection admits min(K, candidates) <= PP_MAXQ entries
            s_key[slot] = key;
            s_flat[slot] = q * a.C + c;
        }
    });
    __syncthreads();
    const int n = s_slots < a.K ? s_slots : a.K;

    // ---- 5. order the survivors: descending score, ties by flat index (rank_sort's loop with the flat index for the position)
    for (int i = tid; i < n; i += DET_THREADS) {
        const float si = __uint_as_float(s_key[i]);
        const int fi = s_flat[i];
        int rank = 0;
        for (int j = 0; j < n; ++j) rank += det_before(__uint_as_float(s_key[j]), s_flat[j], si, fi) ? 1 : 0;
        s_order[rank] = i;
    }
    __syncthreads();

    // ---- 6. rows
    for (int r = tid; r < a.K; r += DET_THREADS) {
        const long long row = (long long)b * a.K + r;
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        long long label = 0;
        float score = 0.f;
        int query = 0;
        if (r < n) {
            const int i = s_order[r];
            query = s_flat[i] / a.C;
            label = s_flat[i] - query * a.C;
            score = __uint_as_float(s_key[i]);
            o = box_of(b, a.boxes + b * a.sb_b + query * a.sb_q);
        }
        *reinterpret_cast<float4 *>(a.out_boxes + row * 4) = o;
        a.out_labels[row] = label;
        a.out_scores[row] = score;
        if (a.out_query) a.out_query[row] = query;
    }
    if (tid == 0) a.counts[b] = n;
}

}  // namespace detr

using namespace detr;

// the checks both entry points share, on the fields their descriptors have in common
template <class Desc>
static int check_multilabel(const char *who, const Desc *d, int K, float thr) {
    DETR_REQUIRE(d->B > 0 && d->Q > 0 && d->Q <= PP_MAXQ && d->C > 0, "%s: bad shape B=%d Q=%d C=%d (Q 1..%d)", who, d->B, d->Q, d->C, PP_MAXQ);
    DETR_REQUIRE(d->C >= 2, "%s: sigmoid scoring needs a class beside the background class, C=%d", who, d->C);
    DETR_REQUIRE(d->background_class >= 0 && d->background_class < d->C, "%s: background_class=%d outside [0, C=%d)", who,
                 d->background_class, d->C);
    DETR_REQUIRE((long long)d->Q * d->C < (1ll << 31), "%s: Q * C = %lld pairs, fewer than 2^31 are supported", who, (long long)d->Q * d->C);
    DETR_REQUIRE(K >= 1 && K <= PP_MAXQ, "%s: max_detections=%d must be in 1..%d", who, K, PP_MAXQ);
    DETR_REQUIRE(thr - thr == 0.f, "%s: score_threshold is not finite", who);
    return 0;
}

template <class Desc>
static MultilabelArgs multilabel_args(const Desc *d, int K, float thr, int *out_query) {
    MultilabelArgs a;
    a.logits = d->logits; a.sl_b = d->sL_b; a.sl_q = d->sL_q;
    a.boxes = d->boxes; a.sb_b = d->sB_b; a.sb_q = d->sB_q;
    a.Q = d->Q; a.C = d->C; a.background = d->background_class; a.K = K; a.thr = thr;
    a.out_boxes = d->out_boxes; a.out_labels = reinterpret_cast<long long *>(d->out_labels); a.out_scores = d->out_scores;
    a.out_query = out_query; a.counts = d->counts;
    return a;
}

extern "C" int detr_hip_detect_multilabel(const detr_detect_desc *d, void *stream) {
    const char *who = "detect_multilabel";
    DETR_REQUIRE(d, "%s: null descriptor", who);
    DETR_REQUIRE(d->logits && d->boxes && d->sizes, "%s: null operand (logits, boxes, sizes)", who);
    DETR_REQUIRE(d->out_boxes && d->out_labels && d->out_scores && d->out_query && d->counts,
                 "%s: null operand (out_boxes, out_labels, out_scores, out_query, counts)", who);
    if (check_multilabel(who, d, d->max_detections, d->score_threshold) || check_model_outputs(who, d)) return -1;
    const PixelBoxStage box = {d->sizes, d->bbox_format, d->clip};
    hipLaunchKernelGGL(detect_multilabel_kernel<PixelBoxStage>, dim3(d->B), dim3(DET_THREADS), 0, (hipStream_t)stream,
                       multilabel_args(d, d->max_detections, d->score_threshold, d->out_query), box);
    DETR_LAUNCH_CHECK("detect_multilabel");
    return 0;
}

extern "C" int detr_hip_postprocess_multilabel(const detr_postprocess_desc *d, int32_t max_detections, float score_threshold, void *stream) {
    const char *who = "postprocess_multilabel";
    DETR_REQUIRE(d, "%s: null descriptor", who);
    DETR_REQUIRE(d->logits && d->boxes && d->out_boxes && d->out_labels && d->out_scores && d->counts,
                 "%s: null operand (logits, boxes, out_boxes, out_labels, out_scores, counts)", who);
    if (check_multilabel(who, d, max_detections, score_threshold)) return -1;
    DETR_REQUIRE(d->sL_q >= d->C && d->sL_b >= 0 && d->sB_q >= 4 && d->sB_b >= 0,
                 "%s: strides sL_b=%lld sL_q=%lld (>= C) sB_b=%lld sB_q=%lld (>= 4) are too small", who, (long long)d->sL_b, (long long)d->sL_q,
                 (long long)d->sB_b, (long long)d->sB_q);
    DETR_REQUIRE(d->bbox_format >= 0 && d->bbox_format <= 2, "%s: bbox_format must be 0 (xy_center), 1 (xyxy) or 2 (yxyx)", who);
    DETR_REQUIRE(aligned16(d->out_boxes), "%s: out_boxes must be 16-byte aligned", who);
    const UnitBoxStage box = {d->bbox_format};
    hipLaunchKernelGGL(detect_multilabel_kernel<UnitBoxStage>, dim3(d->B), dim3(DET_THREADS), 0, (hipStream_t)stream,
                       multilabel_args(d, max_detections, score_threshold, nullptr), box);
    DETR_LAUNCH_CHECK("postprocess_multilabel");
    return 0;
}

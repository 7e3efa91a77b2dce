// detections.h -- the primitives of the post-model kernels (postprocess.hip, detect.hip, tile_merge.hip, track.hip, map_match.hip,
// coco_match.hip): each algorithm is written once here, so two entry points that promise the same bits run the same code.
// Every kernel of the family is one workgroup of DET_THREADS threads (4 waves) per image; the helpers take pointers to the
// caller's __shared__ arrays and own no LDS.
#pragma once
#include "common.h"

namespace detr {

constexpr int DET_THREADS = 256;  // 4 waves: the shape query_scores_labels and compact_pass assume
constexpr int PP_MAXQ = 1024;     // queries / detections of one image held in LDS
constexpr int DET_MAXR = 256;     // rows of the padded targets incl. the header (the loaders ship 100)

// How a logit row becomes a (score, label): the scoring policy of query_scores_labels (the `scoring` argument of the *_scored
// entry points, include/detr_hip.h).
constexpr int SCORE_SOFTMAX = 0;  // max softmax probability over all C classes; the callers drop label == background
constexpr int SCORE_SIGMOID = 1;  // sigmoid of the largest non-background logit: the class head of the focal criterion

// The one sigmoid of the post-model kernels: every entry point that scores with SCORE_SIGMOID gives these bits.
__device__ __forceinline__ float sigmoid_score(float x) { return 1.0f / (1.0f + expf(-x)); }

// One wave per query, 4 waves; the logit rows are lg[q * sl_q + 0 .. C), q < Q.  The caller synchronises the workgroup.
// SCORE_SOFTMAX: s_score[q] = max softmax probability, s_label[q] = first arg-max of the PROBABILITIES (inference.py:73-75 takes
// argmax(softmax)); `background` is not read.
// SCORE_SIGMOID: s_label[q] = first arg-max of the logits over c != background, s_score[q] = sigmoid of that logit (C >= 2).  A
// NaN among those logits makes the score NaN (det_before ranks it last, no threshold accepts it); the label is the first arg-max of
// the others, or the first non-background class when there is none.
template <int SCORING = SCORE_SOFTMAX>
__device__ __forceinline__ void query_scores_labels(const float *lg, long long sl_q, int Q, int C, float *s_score, int *s_label,
                                                    int background = -1) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int q = wave; q < Q; q += 4) {
        const float *row = lg + q * sl_q;
        if constexpr (SCORING == SCORE_SIGMOID) {
            float best = -INFINITY;
            int arg = INT_MAX;
            bool nan = false;
            for (int c = lane; c < C; c += 64) {
                if (c == background) continue;
                const float x = row[c];
                nan |= x != x;
                if (x > best) { best = x; arg = c; }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float ob = __shfl_xor(best, o, 64);
                const int oa = __shfl_xor(arg, o, 64);
                if (ob > best || (ob == best && oa < arg)) { best = ob; arg = oa; }
            }
            const bool any_nan = __ballot(nan) != 0ull;
            if (lane == 0) {
                s_score[q] = any_nan ? NAN : sigmoid_score(best);
                s_label[q] = arg != INT_MAX ? arg : (background == 0 ? 1 : 0);
            }
            continue;
        }
        float mx = -INFINITY;
        for (int c = lane; c < C; c += 64) mx = fmaxf(mx, row[c]);
        mx = wave_max(mx);
        float s = 0.f;
        for (int c = lane; c < C; c += 64) s += expf(row[c] - mx);
        s = wave_sum(s);
        // arg-max of the PROBABILITIES (inference.py:75 takes argmax(softmax)), first occurrence on ties
        float best = -1.f;
        int arg = INT_MAX;
        for (int c = lane; c < C; c += 64) {
            const float p = expf(row[c] - mx) / s;
            if (p > best) { best = p; arg = c; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ob = __shfl_xor(best, o, 64);
            const int oa = __shfl_xor(arg, o, 64);
            if (ob > best || (ob == best && oa < arg)) { best = ob; arg = oa; }
        }
        if (lane == 0) { s_score[q] = best; s_label[q] = arg; }
    }
}

// One pass of the order-preserving compaction: thread t offers item t of the pass with `keep`; the kept items get the slots
// base, base + 1, ... in thread order.  store(slot, total) runs in the threads that keep, total = base + the pass's count, known
// before anything is stored; the return value is that total, the next pass's base (workgroup-uniform).
// Barriers: every thread of the workgroup calls this, uniformly.  One barrier publishes s_wave_cnt[4] before the slots are
// computed; a second one follows the stores, so on return s_wave_cnt may be rewritten and what store() wrote to LDS is visible.
template <class Store>
__device__ __forceinline__ int compact_pass(bool keep, int base, int *s_wave_cnt, Store store) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long m = __ballot(keep);
    if (lane == 0) s_wave_cnt[wave] = __popcll(m);
    __syncthreads();
    int off = base;
    for (int w = 0; w < wave; ++w) off += s_wave_cnt[w];
    const int total = base + s_wave_cnt[0] + s_wave_cnt[1] + s_wave_cnt[2] + s_wave_cnt[3];
    if (keep) store(off + __popcll(m & ((1ull << lane) - 1ull)), total);
    __syncthreads();
    return total;
}

// does detection (sa, ia) come before (sb, ib) in np.argsort(-scores, kind="stable")?  Descending score, ties by index, NaN last.
__device__ __forceinline__ bool det_before(float sa, int ia, float sb, int ib) {
    const bool na = sa != sa, nb = sb != sb;
    if (na || nb) return na == nb ? ia < ib : nb;
    return sa > sb || (sa == sb && ia < ib);
}

// Rank sort of n items by det_before over score_at(i): order[rank] = i.  O(n^2 / DET_THREADS) reads of LDS, no atomics.  Ends
// with the barrier that publishes `order`; the caller has synchronised what score_at reads.
template <class ScoreAt>
__device__ __forceinline__ void rank_sort(int n, ScoreAt score_at, int *order) {
    for (int i = threadIdx.x; i < n; i += DET_THREADS) {
        const float si = score_at(i);
        int rank = 0;
        for (int j = 0; j < n; ++j) rank += det_before(score_at(j), j, si, i) ? 1 : 0;
        order[rank] = i;
    }
    __syncthreads();
}

// ---- boxes in image pixels.  A window of the image (the whole image for detect.hip) starts at (ox, oy) and is ew x eh pixels;
// bx = (cx, cy, w, h) normalised to the window.  Every product, sum and difference is one fp32 rounding (contraction is off
// inside these functions, whatever the including file is compiled with), so every caller gets the same bits.
__device__ __forceinline__ float4 pixel_cxcywh(const float *bx, float ox, float oy, float ew, float eh) {
#pragma clang fp contract(off)
    return make_float4(ox + bx[0] * ew, oy + bx[1] * eh, bx[2] * ew, bx[3] * eh);
}

__device__ __forceinline__ float clip_to(float x, float hi) { return fminf(fmaxf(x, 0.f), hi); }

// corners x0, y0, x1, y1 clipped to the W x H image
__device__ __forceinline__ float4 clip_pixel_box(float4 c, float W, float H) {
    return make_float4(clip_to(c.x, W), clip_to(c.y, H), clip_to(c.z, W), clip_to(c.w, H));
}

// the corners x0, y0, x1, y1 = centre -+ size * 0.5, clipped to the W x H image when `clip` is set
__device__ __forceinline__ float4 decode_pixel_box(const float *bx, float ox, float oy, float ew, float eh, float W, float H, int clip) {
#pragma clang fp contract(off)
    const float4 p = pixel_cxcywh(bx, ox, oy, ew, eh);
    const float4 c = make_float4(p.x - p.z * 0.5f, p.y - p.w * 0.5f, p.x + p.z * 0.5f, p.y + p.w * 0.5f);
    return clip ? clip_pixel_box(c, W, H) : c;
}

// the box in bbox_format 0 xy_center (never clipped: recomputed from bx), 1 xyxy, 2 yxyx, 3 xywh (differences of the corners c)
__device__ __forceinline__ float4 emit_pixel_box(int fmt, float4 c, const float *bx, float ox, float oy, float ew, float eh) {
#pragma clang fp contract(off)
    if (fmt == 0) return pixel_cxcywh(bx, ox, oy, ew, eh);
    if (fmt == 1) return c;
    if (fmt == 2) return make_float4(c.y, c.x, c.w, c.z);
    return make_float4(c.x, c.y, c.z - c.x, c.w - c.y);
}

// the match measure of two boxes (x0, y0, x1, y1), fp64 on fp32 corners, every operation one rounding: match 0 = IoU, 1 = intersection
// over the smaller area; a zero denominator gives 0 (a NaN one NaN, which no threshold comparison accepts).  The suppression of
// tile_merge.hip and the association of track.hip run this one definition.
__device__ __forceinline__ double match_measure(const float4 p, const float4 g, int match) {
#pragma clang fp contract(off)
    const double px0 = p.x, py0 = p.y, px1 = p.z, py1 = p.w, gx0 = g.x, gy0 = g.y, gx1 = g.z, gy1 = g.w;
    const double ix = (px1 < gx1 ? px1 : gx1) - (px0 > gx0 ? px0 : gx0);
    const double iy = (py1 < gy1 ? py1 : gy1) - (py0 > gy0 ? py0 : gy0);
    const double inter = (ix > 0.0 ? ix : 0.0) * (iy > 0.0 ? iy : 0.0);
    const double ap = (px1 - px0) * (py1 - py0), ag = (gx1 - gx0) * (gy1 - gy0);
    const double den = match == 0 ? ap + ag - inter : (ap < ag ? ap : ag);
    return den == 0.0 ? 0.0 : inter / den;
}

// ---- staging for the matchers (map_match.hip, coco_match.hip).  Both return the DETR_MAP_BAD_* bits THIS THREAD found; thread
// t stages the items t, t + DET_THREADS, ..., and the caller synchronises the workgroup before another thread reads them.

// The detections detr_hip_postprocess wrote for one image (boxes / labels / scores point at its row 0): *n = count clamped to
// [0, Q]; s_label = -1 marks a label outside [0, nb_class), the detection is skipped.
__device__ __forceinline__ int stage_detections(const float *boxes, const long long *labels, const float *scores, int count, int Q,
                                                int nb_class, float *s_score, int *s_label, float (*s_box)[4], int *n) {
    int bad = 0;
    if (count < 0 || count > Q) { bad |= DETR_MAP_BAD_COUNT; count = count < 0 ? 0 : Q; }
    for (int i = threadIdx.x; i < count; i += DET_THREADS) {
        const long long l = labels[i];
        const bool ok = l >= 0 && l < nb_class;
        if (!ok) bad |= DETR_MAP_BAD_LABEL;
        s_label[i] = ok ? (int)l : -1;
        s_score[i] = scores[i];
        const float4 bx = *reinterpret_cast<const float4 *>(boxes + (long long)i * 4);
        s_box[i][0] = bx.x; s_box[i][1] = bx.y; s_box[i][2] = bx.z; s_box[i][3] = bx.w;
    }
    *n = count;
    return bad;
}

// The padded targets of one image (t_bbox / t_class point at its header row): *G = int(t_bbox[0]), 0 when that is outside
// [0, R-1]; rows 1..G become yxyx in fp32 with the clip to [0, 1] of bbox.py:171-196; s_gcls = -1 marks a class outside
// [0, nb_class), the ground truth is skipped.
__device__ __forceinline__ int stage_targets(const float *t_bbox, const long long *t_class, int R, int nb_class, float (*s_gt)[4], int *s_gcls,
                                             int *G) {
    int bad = 0, g = 0;
    const float head = t_bbox[0];
    if (head > -1.f && head < (float)R) g = (int)head;             // int(t_bbox[b, 0, 0]); NaN fails both comparisons
    else bad |= DETR_MAP_BAD_HEADER;
    auto clip01 = [](float x) { return x < 0.f ? 0.f : (x > 1.f ? 1.f : x); };
    for (int j = threadIdx.x; j < g; j += DET_THREADS) {
        const float *t = t_bbox + (long long)(j + 1) * 4;
        const float cx = t[0], cy = t[1], w = t[2], h = t[3];
        s_gt[j][0] = clip01(cy - h / 2); s_gt[j][1] = clip01(cx - w / 2);
        s_gt[j][2] = clip01(cy + h / 2); s_gt[j][3] = clip01(cx + w / 2);
        const long long c = t_class[j + 1];
        const bool ok = c >= 0 && c < nb_class;
        if (!ok) bad |= DETR_MAP_BAD_TARGET_CLASS;
        s_gcls[j] = ok ? (int)c : -1;
    }
    *G = g;
    return bad;
}

// ---- host side: the argument checks detr_hip_detect and detr_hip_tile_merge share, on the fields their descriptors have in
// common; `who` prefixes the messages.  Returns 0 or -1 with the error text set, like the entry points themselves.
// detr_hip_postprocess is left out on purpose: it never checked strides, clip, a threshold or alignment, and its shape and
// format messages are worded differently, so no check of its own could run here with its text unchanged.
template <class Desc>
static inline int check_model_outputs(const char *who, const Desc *d) {
    DETR_REQUIRE(d->sL_q >= d->C && d->sL_b >= 0 && d->sB_q >= 4 && d->sB_b >= 0,
                 "%s: strides sL_b=%lld sL_q=%lld (>= C) sB_b=%lld sB_q=%lld (>= 4) are too small", who, (long long)d->sL_b, (long long)d->sL_q,
                 (long long)d->sB_b, (long long)d->sB_q);
    DETR_REQUIRE(d->bbox_format >= 0 && d->bbox_format <= 3, "%s: bbox_format must be 0 (xy_center), 1 (xyxy), 2 (yxyx) or 3 (xywh)", who);
    DETR_REQUIRE(d->clip == 0 || d->clip == 1, "%s: clip=%d must be 0 or 1", who, d->clip);
    DETR_REQUIRE(d->score_threshold - d->score_threshold == 0.f, "%s: score_threshold is not finite", who);
    DETR_REQUIRE(aligned16(d->out_boxes), "%s: out_boxes must be 16-byte aligned", who);
    return 0;
}

}  // namespace detr

// detect.hip -- model outputs -> the detections a user draws, on the device (reference webcam_inference.py:26-34, eval.py:41-55).
//
// The reference takes get_model_inference (inference.py:68-95: background queries dropped, boxes normalised, query order) back to
// the host and rescales there with the numpy helpers of bbox.py:230-294; thresholding and ordering are left to the caller.  Here ONE
// launch serves the batch, one workgroup per image, everything in LDS:
//   1. score = max softmax probability and label = first arg-max per query -- query_scores_labels of detections.h, the code
//      postprocess_kernel runs, so both entry points give the same bits;
//   2. a query is kept when label != background and score >= score_threshold (a NaN score fails the comparison); the kept queries
//      are compacted in query order (ballot prefix count, as postprocess_kernel does);
//   3. a rank sort (as map_match.hip) orders them by descending score, ties by query index: np.argsort(-score, kind="stable");
//      the first max_detections are written;
//   4. boxes: (cx, cy, w, h) * (W, H, W, H) of the image's OWN original size -- with padded batches the model's boxes are normalised
//      per image, not per canvas --, then the corners cx -+ w / 2, clipped to [0, W] x [0, H] when `clip` is set; the xywh width and
//      height are the differences of the (clipped) corners.  Products, sums and differences are single fp32 roundings (no
//      contraction), so a rerun and a rebuild give the same bits.
// Rows [counts[b], max_detections) of every output are zero.  No atomics.
#include "detections.h"

namespace detr {

struct DetectArgs {
    const float *logits; long long sl_b, sl_q;      // [B, Q, C]
    const float *boxes; long long sb_b, sb_q;       // [B, Q, 4] cx, cy, w, h
    const int *sizes;                               // [B, 2] height, width
    int Q, C, background, max_det, fmt, clip;
    float thr;
    float *out_boxes;                               // [B, max_det, 4]
    long long *out_labels;                          // [B, max_det]
    float *out_scores;                              // [B, max_det]
    int *out_query;                                 // [B, max_det]
    int *counts;                                    // [B]
};

// SCORING: SCORE_SOFTMAX drops the queries whose label is the background class; under SCORE_SIGMOID every query is a candidate
// and the threshold alone decides.
template <int SCORING>
__global__ __launch_bounds__(DET_THREADS) void detect_kernel(DetectArgs a) {
    __shared__ float s_score[PP_MAXQ];
    __shared__ int s_label[PP_MAXQ];
    __shared__ int s_kept[PP_MAXQ];              // s_kept[i] = query of the i-th kept detection, ascending
    __shared__ int s_order[PP_MAXQ];             // s_order[rank] = position in s_kept
    __shared__ int s_wave_cnt[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    query_scores_labels<SCORING>(a.logits + b * a.sl_b, a.sl_q, a.Q, a.C, s_score, s_label, a.background);
    __syncthreads();

    int n = 0;
    for (int q0 = 0; q0 < a.Q; q0 += DET_THREADS) {
        const int q = q0 + tid;
        const bool keep = q < a.Q && (SCORING == SCORE_SIGMOID || s_label[q] != a.background) && s_score[q] >= a.thr;
        n = compact_pass(keep, n, s_wave_cnt, [&](int i, int) { s_kept[i] = q; });
    }
    rank_sort(n, [&](int i) { return s_score[s_kept[i]]; }, s_order);      // a kept score passed >= thr: never NaN, plain descending order

    const int cnt = n < a.max_det ? n : a.max_det;
    const float H = (float)a.sizes[2 * b], W = (float)a.sizes[2 * b + 1];
    for (int r = tid; r < a.max_det; r += DET_THREADS) {
        const long long row = (long long)b * a.max_det + r;
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        long long label = 0;
        float score = 0.f;
        int query = 0;
        if (r < cnt) {
            query = s_kept[s_order[r]];
            label = s_label[query];
            score = s_score[query];
            // the whole image is the window; the origin -0 adds nothing, not even to a -0 product
            const float *bx = a.boxes + b * a.sb_b + query * a.sb_q;
            o = emit_pixel_box(a.fmt, decode_pixel_box(bx, -0.f, -0.f, W, H, W, H, a.clip), bx, -0.f, -0.f, W, H);
        }
        *reinterpret_cast<float4 *>(a.out_boxes + row * 4) = o;
        a.out_labels[row] = label;
        a.out_scores[row] = score;
        a.out_query[row] = query;
    }
    if (tid == 0) a.counts[b] = cnt;
}

}  // namespace detr

using namespace detr;

static int launch_detect(const detr_detect_desc *d, int scoring, void *stream) {
    DETR_REQUIRE(d, "detect: null descriptor");
    DETR_REQUIRE(d->logits && d->boxes && d->sizes, "detect: null operand (logits, boxes, sizes)");
    DETR_REQUIRE(d->out_boxes && d->out_labels && d->out_scores && d->out_query && d->counts,
                 "detect: null operand (out_boxes, out_labels, out_scores, out_query, counts)");
    DETR_REQUIRE(d->B > 0 && d->Q > 0 && d->Q <= PP_MAXQ && d->C > 0, "detect: bad shape B=%d Q=%d C=%d (Q 1..%d)", d->B, d->Q, d->C, PP_MAXQ);
    if (check_model_outputs("detect", d)) return -1;
    DETR_REQUIRE(d->max_detections >= 1 && d->max_detections <= d->Q, "detect: max_detections=%d must be in 1..Q=%d", d->max_detections, d->Q);
    DetectArgs a;
    a.logits = d->logits; a.sl_b = d->sL_b; a.sl_q = d->sL_q;
    a.boxes = d->boxes; a.sb_b = d->sB_b; a.sb_q = d->sB_q;
    a.sizes = d->sizes;
    a.Q = d->Q; a.C = d->C; a.background = d->background_class; a.max_det = d->max_detections; a.fmt = d->bbox_format; a.clip = d->clip;
    a.thr = d->score_threshold;
    a.out_boxes = d->out_boxes; a.out_labels = reinterpret_cast<long long *>(d->out_labels); a.out_scores = d->out_scores;
    a.out_query = d->out_query; a.counts = d->counts;
    if (scoring == SCORE_SIGMOID) {
        DETR_REQUIRE(d->C >= 2, "detect: sigmoid scoring needs a class beside the background class, C=%d", d->C);
        DETR_REQUIRE(d->background_class >= 0 && d->background_class < d->C, "detect: background_class=%d outside [0, C=%d)",
                     d->background_class, d->C);
        hipLaunchKernelGGL(detect_kernel<SCORE_SIGMOID>, dim3(d->B), dim3(DET_THREADS), 0, (hipStream_t)stream, a);
    } else {
        hipLaunchKernelGGL(detect_kernel<SCORE_SOFTMAX>, dim3(d->B), dim3(DET_THREADS), 0, (hipStream_t)stream, a);
    }
    DETR_LAUNCH_CHECK("detect");
    return 0;
}

extern "C" int detr_hip_detect(const detr_detect_desc *d, void *stream) { return launch_detect(d, SCORE_SOFTMAX, stream); }

extern "C" int detr_hip_detect_scored(const detr_detect_desc *d, int32_t scoring, void *stream) {
    DETR_REQUIRE(scoring == SCORE_SOFTMAX || scoring == SCORE_SIGMOID, "detect: scoring=%d must be 0 (softmax) or 1 (sigmoid)", scoring);
    return launch_detect(d, scoring, stream);
}

// tile_merge.hip -- sliced inference, the merge: the model ran on overlapping windows ("tiles") of every image, plus usually the whole
// image; this kernel maps every tile's boxes back to the image and removes the duplicates the overlaps create, by a class-wise
// greedy non-maximum suppression.  The reference has nothing of the kind: a user of get_model_inference (inference.py:68-95) writes
// this as a NumPy loop per image.  Here ONE launch serves the batch, one workgroup per image, everything in LDS:
//   1. per tile, score = max softmax probability and label = first arg-max per query -- query_scores_labels of detections.h,
//      the code detect_kernel and postprocess_kernel run, so the bits agree; a query is kept when label != background and
//      score >= score_threshold (a NaN score fails the comparison);
//   2. its box is mapped to image pixels: cx = x0 + bx * wc, cy = y0 + by * hc, w = bw * wc, h = bh * hc, corners c -+ size * 0.5,
//      every operation one fp32 rounding (decode_pixel_box of detections.h), clipped to the image when `clip` is set;
//      with the whole image as the window these are detect_kernel's bits;
//   3. the edge rule: an unclipped corner within edge_margin pixels of (or beyond) a window edge that is interior to the image
//      drops the candidate -- the object is probably truncated and another tile, or the full view, sees it whole;
//      the survivors are compacted in (tile, query) order (ballot prefix count, as detect_kernel does);
//   4. a rank sort orders them by descending score, ties by position, i.e. lower tile, then lower query;
//   5. the greedy suppression walks that order.  The next candidate that is still alive is kept; all lanes then test the alive
//      candidates behind it against it (fp64 IoU or intersection over the smaller area, IEEE division, strict >) and mark the
//      matches dead; one barrier, and the scan goes on.  That is the sequential algorithm exactly, at ONE BARRIER PER KEPT BOX; it
//      stops after max_detections kept boxes, since later ones cannot change earlier ones;
//   6. the kept boxes are written in bbox_format; rows [counts[b], max_detections) are zero.
// An image with more than TM_MAXC candidates sets DETR_TILE_OVER_CAP in the status word and gets no detections: nothing is
// truncated silently, nothing is read or written out of bounds.  No atomics except the integer OR on the status word.
#include "detections.h"

namespace detr {

constexpr int TM_MAXC = DETR_TILE_MAX_CAND;      // candidates of one image held in LDS

struct TileMergeArgs {
    const float *logits; long long sl_b, sl_q;      // [N, Q, C]
    const float *boxes; long long sb_b, sb_q;       // [N, Q, 4] cx, cy, w, h of the tile
    const int *tile_start;                          // [B + 1]
    const int *windows;                             // [N, 4] y0, x0, hc, wc
    const int *sizes;                               // [B, 2] height, width
    int N, Q, C, background, max_det, fmt, clip, match, agnostic;
    float thr, margin;
    double nms;
    float *out_boxes;                               // [B, max_det, 4]
    long long *out_labels;                          // [B, max_det]
    float *out_scores;                              // [B, max_det]
    int *out_query, *out_tile;                      // [B, max_det]
    int *counts;                                    // [B]
    int *status;                                    // [1]
};

__global__ __launch_bounds__(DET_THREADS) void tile_merge_kernel(TileMergeArgs a) {
    __shared__ float s_score[PP_MAXQ];             // the tile being staged
    __shared__ int s_label[PP_MAXQ];
    __shared__ float4 c_box[TM_MAXC];              // candidates in (tile, query) order: corners x0, y0, x1, y1 of step 2
    __shared__ float c_score[TM_MAXC];
    __shared__ int c_label[TM_MAXC];
    __shared__ int c_tile[TM_MAXC];                // tile index within the image
    __shared__ int c_query[TM_MAXC];
    __shared__ int s_order[TM_MAXC];               // s_order[rank] = candidate
    __shared__ int s_keep[TM_MAXC];                // s_keep[i] = rank of the i-th kept candidate
    __shared__ unsigned char s_dead[TM_MAXC];      // by rank
    __shared__ int s_wave_cnt[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float H = (float)a.sizes[2 * b], W = (float)a.sizes[2 * b + 1];
    const int Hi = a.sizes[2 * b], Wi = a.sizes[2 * b + 1];

    int bad = 0;
    int ts = a.tile_start[b], te = a.tile_start[b + 1];
    if (ts < 0 || te < ts || te > a.N) { bad |= DETR_TILE_BAD_START; ts = te = 0; }

    // ---- 1..3: candidates of every tile, mapped, edge rule, compacted in (tile, query) order
    int n = 0;                                     // workgroup-uniform
    for (int t = ts; t < te && !(bad & DETR_TILE_OVER_CAP); ++t) {
        query_scores_labels(a.logits + t * a.sl_b, a.sl_q, a.Q, a.C, s_score, s_label);
        __syncthreads();
        const int wy0 = a.windows[4 * t], wx0 = a.windows[4 * t + 1], whc = a.windows[4 * t + 2], wwc = a.windows[4 * t + 3];
        const float fx0 = (float)wx0, fy0 = (float)wy0, fwc = (float)wwc, fhc = (float)whc;
        const bool whole = wx0 == 0 && wy0 == 0 && wwc == Wi && whc == Hi;
        const bool edges = a.margin > 0.f && !whole;
        const bool in_l = wx0 > 0, in_t = wy0 > 0;                      // which window edges are interior to the image
        const bool in_r = (long long)wx0 + wwc < Wi, in_b = (long long)wy0 + whc < Hi;
        const float ex1 = (float)((long long)wx0 + wwc), ey1 = (float)((long long)wy0 + whc);
        for (int q0 = 0; q0 < a.Q; q0 += DET_THREADS) {
            const int q = q0 + tid;
            bool keep = q < a.Q && s_label[q] != a.background && s_score[q] >= a.thr;
            float4 box = make_float4(0.f, 0.f, 0.f, 0.f);
            if (keep) {
                box = decode_pixel_box(a.boxes + t * a.sb_b + q * a.sb_q, fx0, fy0, fwc, fhc, W, H, 0);
                if (edges) {
                    const bool drop = (in_l && box.x - fx0 <= a.margin) || (in_r && ex1 - box.z <= a.margin) ||
                                      (in_t && box.y - fy0 <= a.margin) || (in_b && ey1 - box.w <= a.margin);
                    keep = !drop;
                }
                if (a.clip) box = clip_pixel_box(box, W, H);
            }
            n = compact_pass(keep, n, s_wave_cnt, [&](int i, int total) {
                if (total > TM_MAXC) return;                            // uniform: nothing of this pass is stored
                c_box[i] = box; c_score[i] = s_score[q]; c_label[i] = s_label[q]; c_tile[i] = t - ts; c_query[i] = q;
            });
            if (n > TM_MAXC) { bad |= DETR_TILE_OVER_CAP; break; }      // uniform
        }
    }
    if (bad) {
        if (tid == 0) atomicOr(a.status, bad);
        n = 0;
    }

    // ---- 4: rank sort, descending score, ties by position
    for (int i = tid; i < n; i += DET_THREADS) s_dead[i] = 0;
    rank_sort(n, [&](int i) { return c_score[i]; }, s_order);           // a candidate's score passed >= thr: never NaN

    // ---- 5: greedy suppression, one barrier per kept box
    int kept = 0;
    for (int r = 0; r < n && kept < a.max_det; ++r) {
        if (s_dead[r]) continue;                                        // uniform: every thread reads the same flag
        const int i = s_order[r];
        if (tid == 0) s_keep[kept] = r;
        ++kept;
        const float4 bi = c_box[i];
        const int li = c_label[i];
        for (int rj = r + 1 + tid; rj < n; rj += DET_THREADS) {
            if (s_dead[rj]) continue;
            const int j = s_order[rj];
            if (!a.agnostic && c_label[j] != li) continue;
            if (match_measure(bi, c_box[j], a.match) > a.nms) s_dead[rj] = 1;
        }
        __syncthreads();
    }
    __syncthreads();                                                    // s_keep of thread 0 (n == 0 or no suppression pass ran last)

    // ---- 6: output
    for (int r = tid; r < a.max_det; r += DET_THREADS) {
        const long long row = (long long)b * a.max_det + r;
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        long long label = 0;
        float score = 0.f;
        int query = 0, tile = 0;
        if (r < kept) {
            const int i = s_order[s_keep[r]];
            label = c_label[i]; score = c_score[i]; query = c_query[i]; tile = c_tile[i];
            const int t = ts + tile;
            float wx = 0.f, wy = 0.f, ww = 0.f, wh = 0.f;               // only format 0 reads the window again: cx, cy, w, h of step 2 recomputed
            if (a.fmt == 0) { wx = (float)a.windows[4 * t + 1]; wy = (float)a.windows[4 * t]; ww = (float)a.windows[4 * t + 3]; wh = (float)a.windows[4 * t + 2]; }
            o = emit_pixel_box(a.fmt, c_box[i], a.boxes + t * a.sb_b + query * a.sb_q, wx, wy, ww, wh);
        }
        *reinterpret_cast<float4 *>(a.out_boxes + row * 4) = o;
        a.out_labels[row] = label;
        a.out_scores[row] = score;
        a.out_query[row] = query;
        a.out_tile[row] = tile;
    }
    if (tid == 0) a.counts[b] = kept;
}

}  // namespace detr

using namespace detr;

extern "C" int detr_hip_tile_merge(const detr_tile_merge_desc *d, void *stream) {
    DETR_REQUIRE(d, "tile_merge: null descriptor");
    DETR_REQUIRE(d->logits && d->boxes && d->tile_start && d->tile_start_host && d->windows && d->sizes,
                 "tile_merge: null operand (logits, boxes, tile_start, tile_start_host, windows, sizes)");
    DETR_REQUIRE(d->out_boxes && d->out_labels && d->out_scores && d->out_query && d->out_tile && d->counts && d->status,
                 "tile_merge: null operand (out_boxes, out_labels, out_scores, out_query, out_tile, counts, status)");
    DETR_REQUIRE(d->B > 0 && d->B <= 65535 && d->N > 0 && d->Q > 0 && d->Q <= PP_MAXQ && d->C > 0,
                 "tile_merge: bad shape B=%d N=%d Q=%d C=%d (B 1..65535, N >= 1, Q 1..%d)", d->B, d->N, d->Q, d->C, PP_MAXQ);
    if (check_model_outputs("tile_merge", d)) return -1;
    DETR_REQUIRE(d->tile_start_host[0] == 0 && d->tile_start_host[d->B] == d->N,
                 "tile_merge: tile_start must run from 0 to N=%d, got %d .. %d", d->N, d->tile_start_host[0], d->tile_start_host[d->B]);
    for (int b = 0; b < d->B; ++b)
        DETR_REQUIRE(d->tile_start_host[b + 1] >= d->tile_start_host[b], "tile_merge: tile_start is not monotone at image %d (%d then %d)", b,
                     d->tile_start_host[b], d->tile_start_host[b + 1]);
    DETR_REQUIRE(d->max_detections >= 1 && d->max_detections <= TM_MAXC, "tile_merge: max_detections=%d must be in 1..%d (the candidate cap)",
                 d->max_detections, TM_MAXC);
    DETR_REQUIRE(d->match == 0 || d->match == 1, "tile_merge: match=%d must be 0 (IoU) or 1 (intersection over the smaller area)", d->match);
    DETR_REQUIRE(d->class_agnostic == 0 || d->class_agnostic == 1, "tile_merge: class_agnostic=%d must be 0 or 1", d->class_agnostic);
    DETR_REQUIRE(d->nms_threshold - d->nms_threshold == 0.0, "tile_merge: nms_threshold is not finite");
    DETR_REQUIRE(d->edge_margin - d->edge_margin == 0.f && d->edge_margin >= 0.f, "tile_merge: edge_margin must be finite and >= 0");
    TileMergeArgs a;
    a.logits = d->logits; a.sl_b = d->sL_b; a.sl_q = d->sL_q;
    a.boxes = d->boxes; a.sb_b = d->sB_b; a.sb_q = d->sB_q;
    a.tile_start = d->tile_start; a.windows = d->windows; a.sizes = d->sizes;
    a.N = d->N; a.Q = d->Q; a.C = d->C; a.background = d->background_class; a.max_det = d->max_detections; a.fmt = d->bbox_format;
    a.clip = d->clip; a.match = d->match; a.agnostic = d->class_agnostic;
    a.thr = d->score_threshold; a.margin = d->edge_margin; a.nms = d->nms_threshold;
    a.out_boxes = d->out_boxes; a.out_labels = reinterpret_cast<long long *>(d->out_labels); a.out_scores = d->out_scores;
    a.out_query = d->out_query; a.out_tile = d->out_tile; a.counts = d->counts; a.status = d->status;
    hipLaunchKernelGGL(tile_merge_kernel, dim3(d->B), dim3(DET_THREADS), 0, (hipStream_t)stream, a);
    DETR_LAUNCH_CHECK("tile_merge");
    return 0;
}

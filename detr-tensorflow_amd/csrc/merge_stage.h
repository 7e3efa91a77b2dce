// merge_stage.h -- what the merge kernels of the model's views share (tile_merge.hip: the tiles of sliced inference; fuse_views.hip:
// flipped and rescaled views): the kernel arguments, steps 1..3 of include/detr_hip.h's detr_tile_merge_desc -- candidates, mapping,
// edge rule, compaction in (view, query) order --, the greedy suppression of its step 5, and the host-side checks of the descriptor.
// Each is written once here, so detr_hip_fuse_views with method 0 and no flipped view gives detr_hip_tile_merge's bits by
// construction.  The helpers take pointers to the caller's __shared__ arrays and own no LDS.
#pragma once
#include "detections.h"

namespace detr {

constexpr int TM_MAXC = DETR_TILE_MAX_CAND;      // candidates of one image held in LDS

struct MergeArgs {
    const float *logits; long long sl_b, sl_q;      // [N, Q, C]
    const float *boxes; long long sb_b, sb_q;       // [N, Q, 4] cx, cy, w, h of the tile
    const int *tile_start;                          // [B + 1]
    const int *windows;                             // [N, 4] y0, x0, hc, wc
    const int *sizes;                               // [B, 2] height, width
    const int *view_flip;                           // [N] or null: the view is of the mirrored image (fuse_views.hip only)
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

// the candidates of one image in (tile, query) order, [TM_MAXC] each: corners x0, y0, x1, y1 of step 2 in image pixels
struct Candidates {
    float4 *box;
    float *score;
    int *label, *tile, *query;                      // tile: index within the image
};

// Steps 1..3 for image b: the candidates of every tile, mapped, edge rule, compacted in (tile, query) order.  Returns their number
// n (workgroup-uniform), 0 with the DETR_TILE_* bits in *bad when tile_start is broken or there are more than TM_MAXC; *first_tile
// is the image's first row of logits / boxes.  A FLIPPED view (a.view_flip[t] != 0) saw the mirrored image: its window is one of
// the mirrored image, the mapping and the edge rule run in that frame, then the unclipped corners are mirrored back,
// (x0, x1) <- (W - x1, W - x0), one fp32 rounding each; the clip follows.  s_score / s_label [PP_MAXQ] stage one tile and are free
// again on return; ends with a barrier (compact_pass), so the candidates are visible to every thread.
__device__ __forceinline__ int stage_candidates(const MergeArgs &a, int b, float *s_score, int *s_label, int *s_wave_cnt, Candidates c,
                                                int *first_tile, int *bad_out) {
    const int tid = threadIdx.x;
    const float H = (float)a.sizes[2 * b], W = (float)a.sizes[2 * b + 1];
    const int Hi = a.sizes[2 * b], Wi = a.sizes[2 * b + 1];

    int bad = 0;
    int ts = a.tile_start[b], te = a.tile_start[b + 1];
    if (ts < 0 || te < ts || te > a.N) { bad |= DETR_TILE_BAD_START; ts = te = 0; }

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
        const bool flipped = a.view_flip != nullptr && a.view_flip[t] != 0;
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
                if (flipped) {
                    const float mx0 = W - box.z, mx1 = W - box.x;
                    box.x = mx0; box.z = mx1;
                }
                if (a.clip) box = clip_pixel_box(box, W, H);
            }
            n = compact_pass(keep, n, s_wave_cnt, [&](int i, int total) {
                if (total > TM_MAXC) return;                            // uniform: nothing of this pass is stored
                c.box[i] = box; c.score[i] = s_score[q]; c.label[i] = s_label[q]; c.tile[i] = t - ts; c.query[i] = q;
            });
            if (n > TM_MAXC) { bad |= DETR_TILE_OVER_CAP; break; }      // uniform
        }
    }
    *first_tile = ts;
    *bad_out = bad;
    return bad ? 0 : n;
}

// Step 5, the greedy suppression over the rank order s_order[0 .. n) (rank_sort of detections.h).  The next candidate that is still
// alive is kept; all lanes then test the alive candidates behind it against it -- suppresses(box and label of the kept one, j), the
// caller's rule: same label unless class-agnostic, fp64 match measure, strict > -- and mark the matches dead; one barrier, and the scan
// goes on: the sequential algorithm exactly, at ONE BARRIER PER KEPT BOX.  It stops after max_det kept boxes, since later ones cannot
// change earlier ones.  Returns their number (uniform); s_keep[i] = rank of the i-th kept candidate, published by the closing
// barrier.  s_dead [TM_MAXC] is scratch.
template <class Suppresses>
__device__ __forceinline__ int greedy_suppress(int n, int max_det, Suppresses suppresses, const float4 *c_box, const int *c_label, const int *s_order,
                                               unsigned char *s_dead, int *s_keep) {
    const int tid = threadIdx.x;
    for (int i = tid; i < n; i += DET_THREADS) s_dead[i] = 0;
    __syncthreads();
    int kept = 0;
    for (int r = 0; r < n && kept < max_det; ++r) {
        if (s_dead[r]) continue;                                        // uniform: every thread reads the same flag
        const int i = s_order[r];
        if (tid == 0) s_keep[kept] = r;
        ++kept;
        const float4 bi = c_box[i];
        const int li = c_label[i];
        for (int rj = r + 1 + tid; rj < n; rj += DET_THREADS) {
            if (s_dead[rj]) continue;
            if (suppresses(bi, li, s_order[rj])) s_dead[rj] = 1;
        }
        __syncthreads();
    }
    __syncthreads();                                                    // s_keep of thread 0 (n == 0 or no suppression pass ran last)
    return kept;
}

// ---- host side: the checks of detr_tile_merge_desc that detr_hip_tile_merge and detr_hip_fuse_views share; `who` prefixes the
// messages.  Returns 0 or -1 with the error text set.
static inline int check_merge_desc(const char *who, const detr_tile_merge_desc *d) {
    DETR_REQUIRE(d, "%s: null descriptor", who);
    DETR_REQUIRE(d->logits && d->boxes && d->tile_start && d->tile_start_host && d->windows && d->sizes,
                 "%s: null operand (logits, boxes, tile_start, tile_start_host, windows, sizes)", who);
    DETR_REQUIRE(d->out_boxes && d->out_labels && d->out_scores && d->out_query && d->out_tile && d->counts && d->status,
                 "%s: null operand (out_boxes, out_labels, out_scores, out_query, out_tile, counts, status)", who);
    DETR_REQUIRE(d->B > 0 && d->B <= 65535 && d->N > 0 && d->Q > 0 && d->Q <= PP_MAXQ && d->C > 0,
                 "%s: bad shape B=%d N=%d Q=%d C=%d (B 1..65535, N >= 1, Q 1..%d)", who, d->B, d->N, d->Q, d->C, PP_MAXQ);
    if (check_model_outputs(who, d)) return -1;
    DETR_REQUIRE(d->tile_start_host[0] == 0 && d->tile_start_host[d->B] == d->N, "%s: tile_start must run from 0 to N=%d, got %d .. %d", who, d->N,
                 d->tile_start_host[0], d->tile_start_host[d->B]);
    for (int b = 0; b < d->B; ++b)
        DETR_REQUIRE(d->tile_start_host[b + 1] >= d->tile_start_host[b], "%s: tile_start is not monotone at image %d (%d then %d)", who, b,
                     d->tile_start_host[b], d->tile_start_host[b + 1]);
    DETR_REQUIRE(d->max_detections >= 1 && d->max_detections <= TM_MAXC, "%s: max_detections=%d must be in 1..%d (the candidate cap)", who,
                 d->max_detections, TM_MAXC);
    DETR_REQUIRE(d->match == 0 || d->match == 1, "%s: match=%d must be 0 (IoU) or 1 (intersection over the smaller area)", who, d->match);
    DETR_REQUIRE(d->class_agnostic == 0 || d->class_agnostic == 1, "%s: class_agnostic=%d must be 0 or 1", who, d->class_agnostic);
    DETR_REQUIRE(d->nms_threshold - d->nms_threshold == 0.0, "%s: nms_threshold is not finite", who);
    DETR_REQUIRE(d->edge_margin - d->edge_margin == 0.f && d->edge_margin >= 0.f, "%s: edge_margin must be finite and >= 0", who);
    return 0;
}

// the kernel arguments of a checked descriptor
static inline MergeArgs merge_args(const detr_tile_merge_desc *d, const int *view_flip) {
    MergeArgs a;
    a.logits = d->logits; a.sl_b = d->sL_b; a.sl_q = d->sL_q;
    a.boxes = d->boxes; a.sb_b = d->sB_b; a.sb_q = d->sB_q;
    a.tile_start = d->tile_start; a.windows = d->windows; a.sizes = d->sizes; a.view_flip = view_flip;
    a.N = d->N; a.Q = d->Q; a.C = d->C; a.background = d->background_class; a.max_det = d->max_detections; a.fmt = d->bbox_format;
    a.clip = d->clip; a.match = d->match; a.agnostic = d->class_agnostic;
    a.thr = d->score_threshold; a.margin = d->edge_margin; a.nms = d->nms_threshold;
    a.out_boxes = d->out_boxes; a.out_labels = reinterpret_cast<long long *>(d->out_labels); a.out_scores = d->out_scores;
    a.out_query = d->out_query; a.out_tile = d->out_tile; a.counts = d->counts; a.status = d->status;
    return a;
}

}  // namespace detr

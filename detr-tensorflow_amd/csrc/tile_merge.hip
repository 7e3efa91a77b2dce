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
// Steps 1..3 and 5 and the host-side checks live in merge_stage.h, which fuse_views.hip runs too.
#include "merge_stage.h"

namespace detr {

__global__ __launch_bounds__(DET_THREADS) void tile_merge_kernel(MergeArgs a) {
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

    // ---- 1..3: candidates of every tile, mapped, edge rule, compacted in (tile, query) order
    int ts, bad;
    const int n = stage_candidates(a, b, s_score, s_label, s_wave_cnt, Candidates{c_box, c_score, c_label, c_tile, c_query}, &ts, &bad);
    if (bad && tid == 0) atomicOr(a.status, bad);

    // ---- 4: rank sort, descending score, ties by position
    rank_sort(n, [&](int i) { return c_score[i]; }, s_order);           // a candidate's score passed >= thr: never NaN

    // ---- 5: greedy suppression, one barrier per kept box
    const int kept = greedy_suppress(n, a.max_det, [&](const float4 &bi, int li, int j) {
        return (a.agnostic || c_label[j] == li) && match_measure(bi, c_box[j], a.match) > a.nms;
    }, c_box, c_label, s_order, s_dead, s_keep);

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
    if (check_merge_desc("tile_merge", d)) return -1;
    hipLaunchKernelGGL(tile_merge_kernel, dim3(d->B), dim3(DET_THREADS), 0, (hipStream_t)stream, merge_args(d, nullptr));
    DETR_LAUNCH_CHECK("tile_merge");
    return 0;
}

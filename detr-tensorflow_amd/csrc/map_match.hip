// map_match.hip -- the per-image half of the COCO-style mAP accumulation on the device (detr_tf/loss/compute_map.py:
// APAccumulator.add_image, which pins the reference's cal_map, compute_map.py:183-272).
//
// The reference's eval loop (eval.py:41-55) calls cal_map once per image on the host.  Here ONE launch serves the batch, one
// workgroup per image, entirely in LDS:
//   1. the detections detr_hip_postprocess wrote for the image (yxyx boxes, labels, scores, count) and the padded targets
//      (header row, cx cy w h -> yxyx in fp32 with the clip of bbox.py:171-196) are staged; the ground truths are counted into
//      num_gt[class] with integer atomics;
//   2. a rank sort gives the visiting order of cal_map :207, np.argsort(-scores, kind="stable"): descending score, ties by query
//      position, NaN last;
//   3. the greedy matching.  Classes are independent, so wave w owns the classes c with c % 4 == w; the only sequential dimension
//      is the detections of one class in score order.  For one detection the lanes first hold one ground truth each (64 per
//      pass): IoU in fp64 with compute_overlaps' operation order (compute_map.py:124-139; this file is compiled with
//      -ffp-contract=off, the division is IEEE), and a ballot of the same-class ground truths above the smallest threshold.
//      Almost every detection has zero to two of them.  Then the lanes change roles and hold one THRESHOLD each: the candidates
//      are walked in index order (their IoU broadcast from the lane that computed it) and lane t keeps the unused one of largest
//      IoU strictly above thresholds[t] -- the strict comparison keeps the lowest index on ties (cal_map :233-247).  A ground
//      truth is consumed per threshold: bit t of its LDS word.  The ballot of the lanes that found one is the record's flag word.
// A label or target class outside [0, nb_class), a header count outside [0, R-1] or a detection count outside [0, Q] sets the
// status word and the item is skipped (the image is treated as having no targets / the count is clamped): nothing is read or
// written out of bounds.
#include "detections.h"

namespace detr {

constexpr int MM_WAVES = DET_THREADS / 64;

struct MapArgs {
    const float *boxes; const long long *labels; const float *scores; const int *counts; long long sd_b;
    const float *t_bbox; long long st_b;
    const long long *t_class; long long sc_b;
    int Q, R, nb_class, n_thr;
    double thr[DETR_MAP_MAX_THR];
    double thr_min;
    float *rec_score; int *rec_class; uint32_t *rec_flags;
    unsigned long long *num_gt;
    int *status;
};

__global__ __launch_bounds__(DET_THREADS) void map_match_kernel(MapArgs a) {
    __shared__ float s_score[PP_MAXQ];
    __shared__ int s_label[PP_MAXQ];             // -1: label out of range, the detection is skipped
    __shared__ int s_order[PP_MAXQ];             // s_order[rank] = position among the image's detections
    __shared__ float s_box[PP_MAXQ][4];
    __shared__ float s_gt[DET_MAXR][4];
    __shared__ int s_gcls[DET_MAXR];             // -1: class out of range, the ground truth is skipped
    __shared__ uint32_t s_used[DET_MAXR];        // bit t: consumed at threshold t
    __shared__ double s_thr[DETR_MAP_MAX_THR];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    int n, G;
    int bad = stage_detections(a.boxes + b * a.sd_b * 4, a.labels + b * a.sd_b, a.scores + b * a.sd_b, a.counts[b], a.Q, a.nb_class, s_score, s_label,
                               s_box, &n);
    bad |= stage_targets(a.t_bbox + b * a.st_b, a.t_class + b * a.sc_b, a.R, a.nb_class, s_gt, s_gcls, &G);
    if (tid < DETR_MAP_MAX_THR) s_thr[tid] = tid < a.n_thr ? a.thr[tid] : INFINITY;
    for (int j = tid; j < G; j += DET_THREADS) {                   // the thread that staged row j
        s_used[j] = 0u;
        if (s_gcls[j] >= 0) atomicAdd(a.num_gt + s_gcls[j], 1ull);
    }
    if (bad) atomicOr(a.status, bad);
    __syncthreads();
    rank_sort(n, [&](int i) { return s_score[i]; }, s_order);

    const long long rec = (long long)b * a.Q;
    for (int r = tid; r < a.Q; r += DET_THREADS) {
        const int i = r < n ? s_order[r] : -1;
        const int c = i >= 0 ? s_label[i] : -1;
        a.rec_score[rec + r] = i >= 0 ? s_score[i] : 0.f;
        a.rec_class[rec + r] = c;
        if (c < 0) a.rec_flags[rec + r] = 0u;                      // the matching below writes the flags of every other record
    }

    const double my_thr = s_thr[lane & (DETR_MAP_MAX_THR - 1)];
    const bool thr_lane = lane < a.n_thr;
    for (int r = 0; r < n; ++r) {
        const int i = s_order[r];
        const int c = s_label[i];
        if (c < 0 || (c & (MM_WAVES - 1)) != wave) continue;       // wave-uniform
        const double py1 = s_box[i][0], px1 = s_box[i][1], py2 = s_box[i][2], px2 = s_box[i][3];
        const double area1 = (py2 - py1) * (px2 - px1);
        double best = 0.0;
        int best_j = -1;
        for (int j0 = 0; j0 < G; j0 += 64) {
            const int j = j0 + lane;
            double iou = 0.0;
            bool cand = false;
            if (j < G && s_gcls[j] == c) {
                const double gy1 = s_gt[j][0], gx1 = s_gt[j][1], gy2 = s_gt[j][2], gx2 = s_gt[j][3];
                const double area2 = (gy2 - gy1) * (gx2 - gx1);
                const double y1 = py1 > gy1 ? py1 : gy1, y2 = py2 < gy2 ? py2 : gy2;
                const double x1 = px1 > gx1 ? px1 : gx1, x2 = px2 < gx2 ? px2 : gx2;
                const double dx = x2 - x1, dy = y2 - y1;
                const double inter = (dx > 0.0 ? dx : 0.0) * (dy > 0.0 ? dy : 0.0);
                iou = inter / (area1 + area2 - inter);
                cand = iou > a.thr_min;                            // false for the NaN of a zero-area pair
            }
            unsigned long long m = __ballot(cand);
            while (m) {                                            // wave-uniform; ascending ground-truth index
                const int src = __ffsll((long long)m) - 1;
                m &= m - 1;
                const double v = __shfl(iou, src, 64);
                const uint32_t used = s_used[j0 + src];
                if (thr_lane && !((used >> lane) & 1u) && v > my_thr && (best_j < 0 || v > best)) { best = v; best_j = j0 + src; }
            }
        }
        const bool hit = best_j >= 0;
        if (hit) atomicOr(&s_used[best_j], 1u << lane);
        const unsigned long long f = __ballot(hit);
        if (lane == 0) a.rec_flags[rec + r] = (uint32_t)f;
        wave_lds_sync();                                           // the next detection of this wave reads s_used
    }
}

}  // namespace detr

using namespace detr;

extern "C" int detr_hip_map_match(const detr_map_match_desc *d, void *stream) {
    DETR_REQUIRE(d, "map_match: null descriptor");
    DETR_REQUIRE(d->boxes && d->labels && d->scores && d->counts && d->t_bbox && d->t_class, "map_match: null operand (boxes, labels, scores, counts, t_bbox, t_class)");
    DETR_REQUIRE(d->rec_score && d->rec_class && d->rec_flags && d->num_gt && d->status, "map_match: null operand (rec_score, rec_class, rec_flags, num_gt, status)");
    DETR_REQUIRE(d->B > 0 && d->B <= 65535 && d->Q > 0 && d->Q <= PP_MAXQ && d->R >= 1 && d->R <= DET_MAXR,
                 "map_match: bad shape B=%d Q=%d R=%d (B 1..65535, Q 1..%d, R 1..%d)", d->B, d->Q, d->R, PP_MAXQ, DET_MAXR);
    DETR_REQUIRE(d->nb_class > 0, "map_match: nb_class=%d must be positive", d->nb_class);
    DETR_REQUIRE(d->n_thr >= 1 && d->n_thr <= DETR_MAP_MAX_THR, "map_match: n_thr=%d thresholds, 1..%d are supported", d->n_thr, DETR_MAP_MAX_THR);
    for (int t = 0; t < d->n_thr; ++t)
        DETR_REQUIRE(d->thresholds[t] - d->thresholds[t] == 0.0, "map_match: threshold %d is not finite", t);
    DETR_REQUIRE(d->sD_b >= d->Q && d->sT_b >= (int64_t)d->R * 4 && d->sC_b >= d->R,
                 "map_match: batch strides sD_b=%lld (>= Q rows), sT_b=%lld (>= 4 R floats), sC_b=%lld (>= R) are too small", (long long)d->sD_b,
                 (long long)d->sT_b, (long long)d->sC_b);
    DETR_REQUIRE(aligned16(d->boxes), "map_match: boxes must be 16-byte aligned");
    MapArgs a;
    a.boxes = d->boxes; a.labels = reinterpret_cast<const long long *>(d->labels); a.scores = d->scores; a.counts = d->counts; a.sd_b = d->sD_b;
    a.t_bbox = d->t_bbox; a.st_b = d->sT_b;
    a.t_class = reinterpret_cast<const long long *>(d->t_class); a.sc_b = d->sC_b;
    a.Q = d->Q; a.R = d->R; a.nb_class = d->nb_class; a.n_thr = d->n_thr;
    a.thr_min = INFINITY;
    for (int t = 0; t < DETR_MAP_MAX_THR; ++t) {
        a.thr[t] = t < d->n_thr ? d->thresholds[t] : 0.0;
        if (t < d->n_thr && a.thr[t] < a.thr_min) a.thr_min = a.thr[t];
    }
    a.rec_score = d->rec_score; a.rec_class = d->rec_class; a.rec_flags = d->rec_flags;
    a.num_gt = reinterpret_cast<unsigned long long *>(d->num_gt);
    a.status = d->status;
    hipLaunchKernelGGL(map_match_kernel, dim3(d->B), dim3(DET_THREADS), 0, (hipStream_t)stream, a);
    DETR_LAUNCH_CHECK("map_match");
    return 0;
}

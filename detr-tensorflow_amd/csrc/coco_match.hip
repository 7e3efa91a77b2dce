// coco_match.hip -- the per-image half of the COCO evaluation protocol on the device: COCOeval's bbIou / evaluateImg for boxes,
// restated in include/detr_hip.h (detr_hip_coco_match) and pinned by detr_tf/loss/coco_eval.py: COCOAccumulator.add_image.
//
// Modelled on map_match.hip: ONE launch serves the batch, one workgroup per image, entirely in LDS:
//   1. the detections detr_hip_postprocess wrote (yxyx boxes, labels, scores, count) and the padded targets (header row,
//      cx cy w h -> yxyx in fp32 with the clip of bbox.py:171-196) are staged with each target's crowd flag and pixel area; the
//      non-ignored ground truths are counted into npig[class][area range] with integer atomics;
//   2. the same rank sort gives the visiting order, np.argsort(-scores, kind="stable"), and in the same pass the rank of each
//      detection among the detections of its class (what maxDets cuts on);
//   3. the greedy matching.  Wave w owns the classes c with c % 4 == w.  For one detection the lanes first hold one ground truth
//      each (64 per pass): IoU in fp64 (compiled with -ffp-contract=off, the division is IEEE) into a wave-private LDS row, and a
//      ballot of the same-class ground truths at or above the smallest starting bound.  Then the lanes change roles and hold one
//      (area range, threshold) PAIR each -- 40 of the 64 lanes with COCO's 4 x 10 -- and walk the candidates in index order twice:
//      phase 1 over the ground truths the lane's area range does not ignore, phase 2 (only for lanes phase 1 left empty) over the
//      ignored ones, where a crowd may be taken again.  `>=` against a bound that rises to every taken IoU: the LATER index wins
//      ties.  A ground truth is consumed per pair: bit `lane` of its two LDS words.  Two ballots give the flag words.
// This kernel is bound by the latency of that dependent chain (one detection after the other, LDS round trips in between), not
// by bandwidth: a batch moves a few hundred KB.
// A label or target class outside [0, nb_class), a header count outside [0, R-1], a detection count outside [0, Q] or a
// non-positive image size sets the status word; the first three skip the item / clamp the count as map_match.hip does, the size
// only enters the pixel area.  Nothing is read or written out of bounds.
#include "detections.h"

namespace detr {

constexpr int CM_WAVES = DET_THREADS / 64;
constexpr int CM_CHUNKS = DET_MAXR / 64;

struct CocoArgs {
    const float *boxes; const long long *labels; const float *scores; const int *counts; long long sd_b;
    const float *t_bbox; long long st_b;
    const long long *t_class; long long sc_b;
    const unsigned char *t_crowd; const float *t_area; long long sm_b;
    const int *sizes;
    int B, Q, R, nb_class, n_thr, n_area;
    double cur0[DETR_COCO_MAX_THR];              // min(thresholds[t], 1 - 1e-10)
    double lo[DETR_COCO_MAX_AREA], hi[DETR_COCO_MAX_AREA];
    double cur_min;
    float *rec_score; int *rec_class; int *rec_rank; uint32_t *rec_flags;
    unsigned long long *npig;
    int *status;
};

__global__ __launch_bounds__(DET_THREADS) void coco_match_kernel(CocoArgs a) {
    __shared__ float s_score[PP_MAXQ];
    __shared__ int s_label[PP_MAXQ];             // -1: label out of range, the detection is skipped
    __shared__ int s_order[PP_MAXQ];             // s_order[rank] = position among the image's detections
    __shared__ int s_crank[PP_MAXQ];             // rank among the detections of the same class
    __shared__ float s_box[PP_MAXQ][4];
    __shared__ float s_gt[DET_MAXR][4];
    __shared__ int s_gcls[DET_MAXR];             // -1: class out of range, the ground truth is skipped
    __shared__ int s_gcrowd[DET_MAXR];
    __shared__ float s_garea[DET_MAXR];
    __shared__ uint32_t s_used[DET_MAXR][2];     // bit (a * n_thr + t): consumed at that pair
    __shared__ double s_iou[CM_WAVES][DET_MAXR]; // wave-private: the IoUs of the detection the wave is on
    __shared__ double s_cur0[DETR_COCO_MAX_THR], s_lo[DETR_COCO_MAX_AREA], s_hi[DETR_COCO_MAX_AREA];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    int n, G;
    int bad = stage_detections(a.boxes + b * a.sd_b * 4, a.labels + b * a.sd_b, a.scores + b * a.sd_b, a.counts[b], a.Q, a.nb_class, s_score, s_label,
                               s_box, &n);
    bad |= stage_targets(a.t_bbox + b * a.st_b, a.t_class + b * a.sc_b, a.R, a.nb_class, s_gt, s_gcls, &G);
    const int H = a.sizes[2 * b], W = a.sizes[2 * b + 1];
    if (H <= 0 || W <= 0) bad |= DETR_COCO_BAD_SIZE;

    if (tid < DETR_COCO_MAX_THR) s_cur0[tid] = tid < a.n_thr ? a.cur0[tid] : INFINITY;
    if (tid < DETR_COCO_MAX_AREA) { s_lo[tid] = tid < a.n_area ? a.lo[tid] : 0.0; s_hi[tid] = tid < a.n_area ? a.hi[tid] : 0.0; }
    for (int j = tid; j < G; j += DET_THREADS) {                   // the thread that staged row j: its crowd flag and area
        const bool crowd = a.t_crowd[b * a.sm_b + j + 1] != 0;
        const float ga = a.t_area[b * a.sm_b + j + 1];
        s_gcrowd[j] = crowd ? 1 : 0;
        s_garea[j] = ga;
        s_used[j][0] = 0u; s_used[j][1] = 0u;
        if (s_gcls[j] >= 0)
            for (int ar = 0; ar < a.n_area; ++ar)
                if (!(crowd || (double)ga < a.lo[ar] || (double)ga > a.hi[ar])) atomicAdd(a.npig + s_gcls[j] * a.n_area + ar, 1ull);
    }
    if (bad) atomicOr(a.status, bad);
    __syncthreads();

    for (int i = tid; i < n; i += DET_THREADS) {
        const float si = s_score[i];
        const int li = s_label[i];
        int rank = 0, crank = 0;
        for (int j = 0; j < n; ++j) {
            const bool before = det_before(s_score[j], j, si, i);
            rank += before ? 1 : 0;
            crank += (before && s_label[j] == li) ? 1 : 0;
        }
        s_order[rank] = i;
        s_crank[i] = crank;
    }
    __syncthreads();

    const long long rec = (long long)b * a.Q, plane = (long long)a.B * a.Q;
    for (int r = tid; r < a.Q; r += DET_THREADS) {
        const int i = r < n ? s_order[r] : -1;
        const int c = i >= 0 ? s_label[i] : -1;
        a.rec_score[rec + r] = i >= 0 ? s_score[i] : 0.f;
        a.rec_class[rec + r] = c;
        a.rec_rank[rec + r] = c >= 0 ? s_crank[i] : 0;
        if (c < 0)                                                 // the matching below writes the flags of every other record
            for (int ar = 0; ar < a.n_area; ++ar) a.rec_flags[ar * plane + rec + r] = 0u;
    }

    const int n_pair = a.n_area * a.n_thr;                         // <= 40
    const bool act = lane < n_pair;
    const int my_a = act ? lane / a.n_thr : 0, my_t = act ? lane % a.n_thr : 0;
    const double my_cur0 = s_cur0[my_t], my_lo = s_lo[my_a], my_hi = s_hi[my_a];
    const int uw = lane >> 5;
    const uint32_t ubit = 1u << (lane & 31);
    const uint32_t tmask = (1u << a.n_thr) - 1u;
    for (int r = 0; r < n; ++r) {
        const int i = s_order[r];
        const int c = s_label[i];
        if (c < 0 || (c & (CM_WAVES - 1)) != wave) continue;       // wave-uniform
        const double dy1 = s_box[i][0], dx1 = s_box[i][1], dy2 = s_box[i][2], dx2 = s_box[i][3];
        const double area_d = (dx2 - dx1) * (dy2 - dy1);
        const double pix_d = ((dy2 - dy1) * (double)H) * ((dx2 - dx1) * (double)W);
        unsigned long long cand[CM_CHUNKS];
#pragma unroll
        for (int k = 0; k < CM_CHUNKS; ++k) {
            cand[k] = 0ull;
            if (k * 64 < G) {                                      // wave-uniform
                const int j = k * 64 + lane;
                bool cd = false;
                if (j < G && s_gcls[j] == c) {
                    const double gy1 = s_gt[j][0], gx1 = s_gt[j][1], gy2 = s_gt[j][2], gx2 = s_gt[j][3];
                    const double w = (dx2 < gx2 ? dx2 : gx2) - (dx1 > gx1 ? dx1 : gx1);
                    const double h = (dy2 < gy2 ? dy2 : gy2) - (dy1 > gy1 ? dy1 : gy1);
                    double iou = 0.0;
                    if (w > 0.0 && h > 0.0) {                      // false for NaN
                        const double inter = w * h;
                        const double uni = s_gcrowd[j] ? area_d : area_d + (gx2 - gx1) * (gy2 - gy1) - inter;
                        iou = inter / uni;
                    }
                    s_iou[wave][j] = iou;
                    cd = iou >= a.cur_min;                         // false for NaN
                }
                cand[k] = __ballot(cd);
            }
        }
        wave_lds_sync();                                           // the lanes read each other's s_iou entries below
        double cur = my_cur0;
        int m = -1;
#pragma unroll
        for (int k = 0; k < CM_CHUNKS; ++k) {                      // phase 1: the ground truths this lane's area range keeps
            unsigned long long mm = cand[k];
            while (mm) {                                           // wave-uniform; ascending ground-truth index
                const int g = k * 64 + __ffsll((long long)mm) - 1;
                mm &= mm - 1;
                const double v = s_iou[wave][g];
                const double ga = (double)s_garea[g];
                const bool ig = s_gcrowd[g] || ga < my_lo || ga > my_hi;
                const bool used = (s_used[g][uw] & ubit) != 0u;
                if (act && !ig && !used && v >= cur) { cur = v; m = g; }
            }
        }
        const bool second = act && m < 0;
        if (__ballot(second)) {                                    // phase 2: the ignored ones; a crowd may be taken again
#pragma unroll
            for (int k = 0; k < CM_CHUNKS; ++k) {
                unsigned long long mm = cand[k];
                while (mm) {
                    const int g = k * 64 + __ffsll((long long)mm) - 1;
                    mm &= mm - 1;
                    const double v = s_iou[wave][g];
                    const double ga = (double)s_garea[g];
                    const bool crowd = s_gcrowd[g] != 0;
                    const bool ig = crowd || ga < my_lo || ga > my_hi;
                    const bool used = (s_used[g][uw] & ubit) != 0u;
                    if (second && ig && (!used || crowd) && v >= cur) { cur = v; m = g; }
                }
            }
        }
        const bool hit = act && m >= 0;
        bool ign;
        if (hit) {
            const double ga = (double)s_garea[m];
            ign = s_gcrowd[m] || ga < my_lo || ga > my_hi;
            atomicOr(&s_used[m][uw], ubit);
        } else {
            ign = act && (pix_d < my_lo || pix_d > my_hi);
        }
        const unsigned long long fm = __ballot(hit), fi = __ballot(ign);
        if (lane < a.n_area) {
            const int sh = lane * a.n_thr;
            a.rec_flags[lane * plane + rec + r] = ((uint32_t)(fm >> sh) & tmask) | (((uint32_t)(fi >> sh) & tmask) << 16);
        }
        wave_lds_sync();                                           // the next detection of this wave reads s_used, rewrites s_iou
    }
}

}  // namespace detr

using namespace detr;

extern "C" int detr_hip_coco_match(const detr_coco_match_desc *d, void *stream) {
    DETR_REQUIRE(d, "coco_match: null descriptor");
    DETR_REQUIRE(d->boxes && d->labels && d->scores && d->counts && d->t_bbox && d->t_class && d->t_crowd && d->t_area && d->sizes,
                 "coco_match: null operand (boxes, labels, scores, counts, t_bbox, t_class, t_crowd, t_area, sizes)");
    DETR_REQUIRE(d->rec_score && d->rec_class && d->rec_rank && d->rec_flags && d->npig && d->status,
                 "coco_match: null operand (rec_score, rec_class, rec_rank, rec_flags, npig, status)");
    DETR_REQUIRE(d->B > 0 && d->B <= 65535 && d->Q > 0 && d->Q <= PP_MAXQ && d->R >= 1 && d->R <= DET_MAXR,
                 "coco_match: bad shape B=%d Q=%d R=%d (B 1..65535, Q 1..%d, R 1..%d)", d->B, d->Q, d->R, PP_MAXQ, DET_MAXR);
    DETR_REQUIRE(d->nb_class > 0, "coco_match: nb_class=%d must be positive", d->nb_class);
    DETR_REQUIRE(d->n_thr >= 1 && d->n_thr <= DETR_COCO_MAX_THR, "coco_match: n_thr=%d thresholds, 1..%d are supported", d->n_thr, DETR_COCO_MAX_THR);
    DETR_REQUIRE(d->n_area >= 1 && d->n_area <= DETR_COCO_MAX_AREA, "coco_match: n_area=%d area ranges, 1..%d are supported", d->n_area,
                 DETR_COCO_MAX_AREA);
    for (int t = 0; t < d->n_thr; ++t)
        DETR_REQUIRE(d->thresholds[t] - d->thresholds[t] == 0.0, "coco_match: threshold %d is not finite", t);
    for (int ar = 0; ar < d->n_area; ++ar) {
        const double lo = d->area_ranges[2 * ar], hi = d->area_ranges[2 * ar + 1];
        DETR_REQUIRE(lo - lo == 0.0 && hi - hi == 0.0 && lo <= hi, "coco_match: area range %d is not a finite [lo, hi] with lo <= hi", ar);
    }
    DETR_REQUIRE(d->sD_b >= d->Q && d->sT_b >= (int64_t)d->R * 4 && d->sC_b >= d->R && d->sM_b >= d->R,
                 "coco_match: batch strides sD_b=%lld (>= Q rows), sT_b=%lld (>= 4 R floats), sC_b=%lld (>= R), sM_b=%lld (>= R) are too small",
                 (long long)d->sD_b, (long long)d->sT_b, (long long)d->sC_b, (long long)d->sM_b);
    DETR_REQUIRE(aligned16(d->boxes), "coco_match: boxes must be 16-byte aligned");
    CocoArgs a;
    a.boxes = d->boxes; a.labels = reinterpret_cast<const long long *>(d->labels); a.scores = d->scores; a.counts = d->counts; a.sd_b = d->sD_b;
    a.t_bbox = d->t_bbox; a.st_b = d->sT_b;
    a.t_class = reinterpret_cast<const long long *>(d->t_class); a.sc_b = d->sC_b;
    a.t_crowd = d->t_crowd; a.t_area = d->t_area; a.sm_b = d->sM_b;
    a.sizes = d->sizes;
    a.B = d->B; a.Q = d->Q; a.R = d->R; a.nb_class = d->nb_class; a.n_thr = d->n_thr; a.n_area = d->n_area;
    a.cur_min = INFINITY;
    for (int t = 0; t < DETR_COCO_MAX_THR; ++t) {
        const double th = t < d->n_thr ? d->thresholds[t] : 0.0;
        a.cur0[t] = th < 1.0 - 1e-10 ? th : 1.0 - 1e-10;
        if (t < d->n_thr && a.cur0[t] < a.cur_min) a.cur_min = a.cur0[t];
    }
    for (int ar = 0; ar < DETR_COCO_MAX_AREA; ++ar) {
        a.lo[ar] = ar < d->n_area ? d->area_ranges[2 * ar] : 0.0;
        a.hi[ar] = ar < d->n_area ? d->area_ranges[2 * ar + 1] : 0.0;
    }
    a.rec_score = d->rec_score; a.rec_class = d->rec_class; a.rec_rank = d->rec_rank; a.rec_flags = d->rec_flags;
    a.npig = reinterpret_cast<unsigned long long *>(d->npig);
    a.status = d->status;
    hipLaunchKernelGGL(coco_match_kernel, dim3(d->B), dim3(DET_THREADS), 0, (hipStream_t)stream, a);
    DETR_LAUNCH_CHECK("coco_match");
    return 0;
}

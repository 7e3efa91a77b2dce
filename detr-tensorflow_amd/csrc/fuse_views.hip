// fuse_views.hip -- test-time augmentation, the fusion: the model ran on several VIEWS of every image -- mirrored and / or resized to
// several shortest sides, whole or tiled --; this kernel maps every view's boxes back to the image and combines them by one of the
// rules a user of get_model_inference (inference.py:68-95) otherwise writes as a NumPy loop per image over V x Q read-back rows:
// hard NMS, soft-NMS with linear or Gaussian decay, or weighted box fusion.  ONE launch serves the batch, one workgroup of
// DET_THREADS per image, everything in LDS; include/detr_hip.h (detr_hip_fuse_views) is the normative text.
//   1..3. candidates, mapping, edge rule, compaction in (view, query) order: stage_candidates of merge_stage.h, the code
//      tile_merge_kernel runs, with its one addition -- a flipped view is mapped and edge-tested in the mirrored frame, then its
//      unclipped corners are mirrored back, (x0, x1) <- (W - x1, W - x0); the clip follows;
//   4. the rank sort by descending score, ties by position (methods 0 and 3; soft-NMS selects by its CURRENT scores instead and an
//      arg-max with ties to the lower position visits equal scores in the same order);
//   5. the method:
//      0 hard NMS: greedy_suppress of merge_stage.h, tile_merge_kernel's: ONE BARRIER PER KEPT BOX;
//      1 / 2 soft-NMS: current scores in fp64.  Every lane offers the best alive candidate among its own (position % DET_THREADS ==
//        lane), a shuffle arg-max inside each wave, four values across the waves (wg_argmax): the selected candidate is emitted with
//        (float)current; then every lane decays ITS OWN candidates against it -- s * (1 - m) where m > threshold, or
//        s * exp(-(m * m) / sigma) -- and lets those below score_min die.  A candidate's current score and alive flag are only ever
//        touched by the lane that owns it, so the decay needs no barrier of its own: ONE BARRIER PER KEPT BOX, the arg-max's
//        (its slots are double-buffered by the step's parity).  The sequential algorithm exactly;
//      3 weighted box fusion: the candidates are walked in rank order; every lane measures the candidate against its own clusters
//        (cluster % DET_THREADS == lane), the same arg-max picks the best-matching cluster (ties: the lower cluster), and the
//        owner of that cluster adds the candidate to its fp64 sums and refreshes the fused box -- or the owner of the next free
//        cluster founds one.  Cluster state is owner-only too: ONE BARRIER PER CANDIDATE (not per kept box: the walk visits all n
//        candidates, so its worst case is TM_MAXC barriers).  Then confidence = sum of scores / members, rescaled by
//        min(members, expected_views) / expected_views, clusters under min_members dropped, the rest ranked by score;
//   6. the rows are written in bbox_format; format 0 is derived from the FINAL corners here (a fused box has no single model
//      row to recompute it from): ((x0 + x1) * 0.5, (y0 + y1) * 0.5, x1 - x0, y1 - y0).  out_members = members of the cluster
//      (1 for methods 0..2).  Rows [counts[b], max_detections) are zero.
// LDS plan (160 KB per workgroup on gfx950).  The staging and the candidates are tile_merge_kernel's: 8 KB + 64 KB, and the rank
// order 8 KB.  The methods never run together, so they share ONE 68 KB scratch block:
//      method 0: the kept ranks 8 KB + the dead flags 2 KB;
//      methods 1, 2: current scores (double) 16 KB + kept candidates 8 KB + emitted scores 8 KB + alive flags 2 KB;
//      method 3: per cluster the fp64 sums sw, sx[4] (40 B), the fused float4 (16 B), members, founder and rank (12 B) = 68 B x
//        FV_MAXK = 1024 clusters; the cluster's label and score reuse the staging arrays (PP_MAXQ = 1024 entries each), the list of
//        surviving clusters reuses the rank order.  2048 clusters would need 136 KB beside the 80 KB above, so the cluster cap is
//        LOWER than the candidate cap: an image that founds more than FV_MAXK clusters sets DETR_FUSE_OVER_CLUSTERS and gets no
//        detections, exactly as DETR_TILE_OVER_CAP does -- never a silent truncation.
// 148 KB in all.  Nothing is read or written out of bounds for any input; no atomics except the integer OR on the status word, so a
// rerun is bit-identical.
#include "merge_stage.h"

namespace detr {

constexpr int FV_MAXK = DETR_FUSE_MAX_CLUSTERS;  // clusters of one image held in LDS (method 3)
constexpr int FV_WORK_BYTES = FV_MAXK * 68;
static_assert(FV_MAXK <= PP_MAXQ && FV_MAXK <= TM_MAXC, "the cluster labels / scores reuse the staging arrays, the survivors the rank order");
static_assert(FV_WORK_BYTES >= TM_MAXC * (8 + 4 + 4 + 1), "the soft-NMS state must fit the scratch block");

struct FuseArgs {
    MergeArgs m;
    int method;                                     // 0 hard NMS, 1 soft-NMS linear, 2 soft-NMS Gaussian, 3 weighted box fusion
    double sigma, score_min;
    int expected, min_members;
    int *out_members;                               // [B, max_det]
};

// Arg-max over the workgroup of the pairs (v, i) every thread offers: the larger v wins, equal v the lower i; a thread with nothing
// to offer passes (-inf, INT_MAX), and i == INT_MAX comes back when no thread had anything.  Shuffles inside a wave, four values
// across the waves, ONE barrier.  Consecutive calls alternate `parity`: a thread can write the slots of call k + 2 only after the
// barrier of call k + 1, which every thread passes only after it has read the slots of call k.
__device__ __forceinline__ void wg_argmax(double &v, int &i, double (*s_v)[4], int (*s_i)[4], int parity) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(v, o, 64);
        const int oi = __shfl_xor(i, o, 64);
        if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
    }
    if (lane == 0) { s_v[parity][wave] = v; s_i[parity][wave] = i; }
    __syncthreads();
    v = s_v[parity][0]; i = s_i[parity][0];
#pragma unroll
    for (int w = 1; w < 4; ++w) {
        const double ov = s_v[parity][w];
        const int oi = s_i[parity][w];
        if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
    }
}

// the final corners c = (x0, y0, x1, y1) in bbox_format; format 0 from the corners, single fp32 roundings
__device__ __forceinline__ float4 emit_corners(int fmt, float4 c) {
#pragma clang fp contract(off)
    if (fmt == 0) return make_float4((c.x + c.z) * 0.5f, (c.y + c.w) * 0.5f, c.z - c.x, c.w - c.y);
    return emit_pixel_box(fmt, c, nullptr, 0.f, 0.f, 0.f, 0.f);         // formats 1..3 never read the model's row
}

__global__ __launch_bounds__(DET_THREADS) void fuse_views_kernel(FuseArgs f) {
#pragma clang fp contract(off)
    __shared__ float s_score[PP_MAXQ];             // the view being staged; method 3: the clusters' scores
    __shared__ int s_label[PP_MAXQ];               //                        method 3: the clusters' labels
    __shared__ float4 c_box[TM_MAXC];              // candidates in (view, query) order: corners x0, y0, x1, y1
    __shared__ float c_score[TM_MAXC];
    __shared__ int c_label[TM_MAXC];
    __shared__ int c_tile[TM_MAXC];                // view index within the image
    __shared__ int c_query[TM_MAXC];
    __shared__ int s_order[TM_MAXC];               // s_order[rank] = candidate; method 3, after the walk: the surviving clusters
    __shared__ __attribute__((aligned(16))) unsigned char s_work[FV_WORK_BYTES];   // the method's own state, see the LDS plan
    __shared__ double s_red_v[2][4];
    __shared__ int s_red_i[2][4];
    __shared__ int s_wave_cnt[4];
    const MergeArgs &a = f.m;
    const int b = blockIdx.x, tid = threadIdx.x;
    // the scratch block as each method carves it
    int *s_keep = reinterpret_cast<int *>(s_work + (f.method == 0 ? 0 : TM_MAXC * 8));   // methods 0..2: the i-th kept candidate
    unsigned char *s_dead = s_work + TM_MAXC * 4;                       // method 0, by rank
    double *cur = reinterpret_cast<double *>(s_work);                   // methods 1, 2: [TM_MAXC] current scores, owner = candidate % DET_THREADS
    float *k_out = reinterpret_cast<float *>(s_work + TM_MAXC * 12);    //               the emitted scores
    unsigned char *alive = s_work + TM_MAXC * 16;
    double *k_sw = reinterpret_cast<double *>(s_work);                  // method 3: [FV_MAXK] sum of the members' scores
    double *k_sx = k_sw + FV_MAXK;                                      //           [FV_MAXK][4] sum of score * corner
    float4 *k_fused = reinterpret_cast<float4 *>(k_sx + 4 * FV_MAXK);
    int *k_cnt = reinterpret_cast<int *>(k_fused + FV_MAXK);
    int *k_first = k_cnt + FV_MAXK;                                     //           the founder, a candidate
    int *k_order = k_first + FV_MAXK;
    float *k_score = s_score;
    int *k_label = s_label;

    // ---- 1..3
    int ts, bad;
    const int n = stage_candidates(a, b, s_score, s_label, s_wave_cnt, Candidates{c_box, c_score, c_label, c_tile, c_query}, &ts, &bad);

    int kept = 0;                                  // rows to write (uniform)
    if (f.method == 0) {
        rank_sort(n, [&](int i) { return c_score[i]; }, s_order);
        kept = greedy_suppress(n, a.max_det, [&](const float4 &bi, int li, int j) {
            return (a.agnostic || c_label[j] == li) && match_measure(bi, c_box[j], a.match) > a.nms;
        }, c_box, c_label, s_order, s_dead, s_keep);
        for (int r = tid; r < kept; r += DET_THREADS) s_keep[r] = s_order[s_keep[r]];   // rank -> candidate, as the soft methods leave it
        __syncthreads();
    } else if (f.method == 1 || f.method == 2) {
        for (int j = tid; j < n; j += DET_THREADS) { cur[j] = (double)c_score[j]; alive[j] = 1; }
        while (kept < a.max_det) {
            double v = -INFINITY;
            int sel = INT_MAX;
            for (int j = tid; j < n; j += DET_THREADS)
                if (alive[j] && cur[j] > v) { v = cur[j]; sel = j; }    // ascending j: equal scores keep the lower position
            wg_argmax(v, sel, s_red_v, s_red_i, kept & 1);
            if (sel == INT_MAX) break;                                  // uniform: nothing alive
            if (tid == 0) { s_keep[kept] = sel; k_out[kept] = (float)v; }
            ++kept;
            const float4 bs = c_box[sel];
            const int ls = c_label[sel];
            for (int j = tid; j < n; j += DET_THREADS) {
                if (j == sel) { alive[j] = 0; continue; }
                if (!alive[j] || (!a.agnostic && c_label[j] != ls)) continue;
                const double m = match_measure(bs, c_box[j], a.match);
                double s = cur[j];
                if (f.method == 1) { if (m > a.nms) s = s * (1.0 - m); }
                else s = s * exp(-(m * m) / f.sigma);
                cur[j] = s;
                if (s < f.score_min) alive[j] = 0;
            }
        }
        __syncthreads();                                                // s_keep / k_out of thread 0
    } else {
        rank_sort(n, [&](int i) { return c_score[i]; }, s_order);
        int nc = 0;                                                     // clusters so far (uniform); cluster k is owned by thread k % DET_THREADS
        bool over = false;
        for (int r = 0; r < n; ++r) {
            const int i = s_order[r];
            const float4 bi = c_box[i];
            const int li = c_label[i];
            double v = -INFINITY;
            int best = INT_MAX;
            for (int k = tid; k < nc; k += DET_THREADS) {
                if (!a.agnostic && k_label[k] != li) continue;
                const double m = match_measure(k_fused[k], bi, a.match);
                if (m > v) { v = m; best = k; }                         // ascending k: equal measures keep the lower cluster
            }
            wg_argmax(v, best, s_red_v, s_red_i, r & 1);
            const double s = (double)c_score[i];
            const double x[4] = {(double)bi.x, (double)bi.y, (double)bi.z, (double)bi.w};
            if (best != INT_MAX && v > a.nms) {
                if ((best & (DET_THREADS - 1)) == tid) {
                    const double sw = k_sw[best] + s;
                    double q[4];
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const double p = s * x[c];
                        const double sx = k_sx[4 * best + c] + p;
                        k_sx[4 * best + c] = sx;
                        q[c] = sx / sw;
                    }
                    k_sw[best] = sw;
                    k_cnt[best] += 1;
                    k_fused[best] = make_float4((float)q[0], (float)q[1], (float)q[2], (float)q[3]);
                }
            } else {
                if (nc == FV_MAXK) { over = true; break; }              // uniform
                if ((nc & (DET_THREADS - 1)) == tid) {
                    k_sw[nc] = s;
#pragma unroll
                    for (int c = 0; c < 4; ++c) k_sx[4 * nc + c] = s * x[c];
                    k_cnt[nc] = 1;
                    k_fused[nc] = bi;
                    k_first[nc] = i;
                    k_label[nc] = li;
                }
                ++nc;
            }
        }
        if (over) { bad |= DETR_FUSE_OVER_CLUSTERS; nc = 0; }
        // confidence of every cluster (still owner-only), then the survivors in cluster order, then their rank by score
        for (int k = tid; k < nc; k += DET_THREADS) {
            const int cnt = k_cnt[k];
            double conf = k_sw[k] / (double)cnt;
            if (f.expected > 0) {
                conf = conf * (double)(cnt < f.expected ? cnt : f.expected);
                conf = conf / (double)f.expected;
            }
            k_score[k] = (float)conf;
        }
        __syncthreads();                                                // the clusters of every owner; s_order is free
        int ns = 0;
        for (int k0 = 0; k0 < nc; k0 += DET_THREADS) {
            const int k = k0 + tid;
            ns = compact_pass(k < nc && k_cnt[k] >= f.min_members, ns, s_wave_cnt, [&](int slot, int) { s_order[slot] = k; });
        }
        rank_sort(ns, [&](int i) { return k_score[s_order[i]]; }, k_order);   // ties by slot = by cluster index
        kept = ns < a.max_det ? ns : a.max_det;
    }
    if (bad) {
        if (tid == 0) atomicOr(a.status, bad);
        kept = 0;
    }

    // ---- 6: output
    for (int r = tid; r < a.max_det; r += DET_THREADS) {
        const long long row = (long long)b * a.max_det + r;
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        long long label = 0;
        float score = 0.f;
        int query = 0, tile = 0, members = 0;
        if (r < kept) {
            if (f.method == 3) {
                const int k = s_order[k_order[r]];
                const int i = k_first[k];
                o = emit_corners(a.fmt, k_fused[k]);
                label = k_label[k]; score = k_score[k]; query = c_query[i]; tile = c_tile[i]; members = k_cnt[k];
            } else {
                const int i = s_keep[r];
                o = emit_corners(a.fmt, c_box[i]);
                label = c_label[i]; query = c_query[i]; tile = c_tile[i]; members = 1;
                score = f.method == 0 ? c_score[i] : k_out[r];
            }
        }
        *reinterpret_cast<float4 *>(a.out_boxes + row * 4) = o;
        a.out_labels[row] = label;
        a.out_scores[row] = score;
        a.out_query[row] = query;
        a.out_tile[row] = tile;
        f.out_members[row] = members;
    }
    if (tid == 0) a.counts[b] = kept;
}

}  // namespace detr

using namespace detr;

extern "C" int detr_hip_fuse_views(const detr_tile_merge_desc *d, const int32_t *view_flip, const double *fuse, int32_t *out_members,
                                   void *stream) {
    if (check_merge_desc("fuse_views", d)) return -1;
    DETR_REQUIRE(fuse && out_members, "fuse_views: null operand (fuse, out_members)");
    for (int i = 0; i < DETR_FUSE_PARAMS; ++i) DETR_REQUIRE(fuse[i] - fuse[i] == 0.0, "fuse_views: fuse[%d] is not finite", i);
    DETR_REQUIRE(fuse[0] == 0.0 || fuse[0] == 1.0 || fuse[0] == 2.0 || fuse[0] == 3.0,
                 "fuse_views: method fuse[0]=%g must be 0 (NMS), 1 (soft-NMS linear), 2 (soft-NMS Gaussian) or 3 (weighted box fusion)", fuse[0]);
    const int method = (int)fuse[0];
    DETR_REQUIRE(method != 2 || fuse[1] > 0.0, "fuse_views: sigma fuse[1]=%g must be > 0 with method 2", fuse[1]);
    DETR_REQUIRE((method != 1 && method != 2) || fuse[2] >= 0.0, "fuse_views: score_min fuse[2]=%g must be >= 0", fuse[2]);
    DETR_REQUIRE(fuse[3] >= 0.0 && fuse[3] <= 2147483647.0 && fuse[3] == (double)(long long)fuse[3],
                 "fuse_views: expected_views fuse[3]=%g must be 0 (no rescaling) or an integer >= 1", fuse[3]);
    DETR_REQUIRE(fuse[4] >= 1.0 && fuse[4] <= 2147483647.0 && fuse[4] == (double)(long long)fuse[4],
                 "fuse_views: min_members fuse[4]=%g must be an integer >= 1", fuse[4]);
    DETR_REQUIRE(fuse[5] == 0.0, "fuse_views: fuse[5] is reserved and must be 0, got %g", fuse[5]);
    FuseArgs f;
    f.m = merge_args(d, view_flip);
    f.method = method; f.sigma = fuse[1]; f.score_min = fuse[2]; f.expected = (int)fuse[3]; f.min_members = (int)fuse[4];
    f.out_members = out_members;
    hipLaunchKernelGGL(fuse_views_kernel, dim3(d->B), dim3(DET_THREADS), 0, (hipStream_t)stream, f);
    DETR_LAUNCH_CHECK("fuse_views");
    return 0;
}

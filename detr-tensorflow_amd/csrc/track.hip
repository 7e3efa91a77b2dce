// track.hip -- multi-object tracking across video frames: which detection of this frame is the object of the last one.  The reference's
// only end-to-end program is a video loop (webcam_inference.py:26-34) that treats every frame as the first; a user writes the
// association as a NumPy loop over tracks x detections on detections read back every frame.  Here ONE launch serves a batch of
// frames, one workgroup per video stream, the tracks of a stream in device memory (include/detr_hip.h: detr_track_desc gives the
// algorithm, steps 1..8, and the state layout).  DET_THREADS == DETR_TRACK_MAX: thread t OWNS slot t, whose state stays in its
// registers from the load to the write-back; the detections of the frame are staged in LDS.
//   association (steps 3, 4): the sequential walk over all pairs by descending (IoU, then lower id, then lower detection) is
//   reproduced as rounds.  Every slot keeps the best detection still free in its row -- (IoU, lower index), the id is the row's --;
//   a round takes the workgroup arg-max of those by (IoU, lower id), which is the first pair of the walk with both sides free; then
//   only the slots whose cached best was that detection rescan their row.  One barrier per matched pair (the arg-max slots are
//   double-buffered), as tile_merge_kernel pays one per kept box.
//   spawn (step 7): the k-th unmatched high detection takes the k-th free slot, both lists from compact_pass of detections.h.
// No atomics except the integer OR on the status word, no float atomics: a rerun from the same state is bit-identical.
#include "detections.h"

namespace detr {

constexpr int TRK_MAX = DETR_TRACK_MAX;
static_assert(TRK_MAX == DET_THREADS, "thread t owns slot t");

// the tracks of one stream in device memory (include/detr_hip.h documents these offsets)
struct TrackState {
    float x[TRK_MAX][4];
    float v[TRK_MAX][4];
    long long label[TRK_MAX];
    float score[TRK_MAX];
    int id[TRK_MAX], hits[TRK_MAX], miss[TRK_MAX], confirmed[TRK_MAX];
    int frame, next_id, pad[2];
};
static_assert(sizeof(TrackState) % 16 == 0, "streams stay 16-byte aligned");

struct TrackArgs {
    TrackState *state;
    const float *boxes;                             // [S, D, 4]
    const long long *labels;                        // [S, D]
    const float *scores;                            // [S, D]
    const int *query;                               // [S, D] or null
    const int *counts, *active;                     // [S]
    int D, max_age, min_hits, agnostic;
    float thr_track, thr_new, alpha, beta;
    double thr_match, thr_low;
    float *out_boxes;                               // [S, D, 4]
    long long *out_labels;
    float *out_scores;
    int *out_query, *out_ids, *out_hits;
    int *out_counts;                                // [S]
    int *status;                                    // [1]
};

// everything a workgroup holds in LDS: 1024 detections, the per-slot exchange arrays, the arg-max slots
struct TrackLds {
    float4 d_box[PP_MAXQ];                          // the detections' corners x0, y0, x1, y1
    long long d_label[PP_MAXQ];
    float d_score[PP_MAXQ];
    int d_slot[PP_MAXQ];                            // the slot a detection was matched to / spawned in, -1 none
    int free_slot[TRK_MAX];                         // free_slot[k] = k-th free slot after step 6
    int spawn_det[TRK_MAX];                         // by slot: the detection spawned in it this frame, -1 none
    int spawn_rank[TRK_MAX];                        // by slot: its position among this frame's spawns
    int t_id[TRK_MAX], t_hits[TRK_MAX], t_conf[TRK_MAX];   // by slot, after steps 5..7: what step 8 emits
    double r_iou[2][4];                             // per wave, double-buffered by round parity
    int r_id[2][4], r_slot[2][4], r_det[2][4];
    int wave_cnt[4];
};
static_assert(sizeof(TrackLds) <= 64 * 1024, "the static LDS limit of a workgroup");

// One stage of the association.  `mine`: this thread's slot takes part; box / label / id: its predicted corners, label, id;
// want_high: the detections of this stage are the high (1) or the low (0) ones.  Returns the detection matched to this slot or -1.
// Every thread of the workgroup calls this, uniformly (it holds barriers and wave shuffles); on return the d_slot entries it wrote
// are visible to all threads.
__device__ __forceinline__ int associate(TrackLds &L, const TrackArgs &a, int n, bool mine, float4 box, long long label, int id, int want_high,
                                         double thr) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int matched = -1, last = -1, cand = -1;
    double cand_iou = -INFINITY;
    bool rescan = mine;
    for (int round = 0;; ++round) {
        if (rescan) {                               // this slot's best detection still free: highest IoU, lowest index on ties
            cand = -1; cand_iou = -INFINITY;
            for (int d = 0; d < n; ++d) {
                if (d == last || L.d_slot[d] >= 0) continue;          // `last` was taken in the round before: its flag may not be visible yet
                if ((L.d_score[d] >= a.thr_track ? 1 : 0) != want_high) continue;
                if (!a.agnostic && L.d_label[d] != label) continue;
                const double iou = match_measure(box, L.d_box[d], 0);
                if (iou > thr && iou > cand_iou) { cand_iou = iou; cand = d; }      // NaN fails both
            }
            rescan = false;
        }
        // workgroup arg-max by (IoU, lower id): ids are unique, so the key names its slot and no further key is needed
        double b_iou = cand_iou;
        int b_id = cand >= 0 ? id : INT_MAX, b_slot, b_det;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double o_iou = __shfl_xor(b_iou, o, 64);
            const int o_id = __shfl_xor(b_id, o, 64);
            if (o_iou > b_iou || (o_iou == b_iou && o_id < b_id)) { b_iou = o_iou; b_id = o_id; }
        }
        const int par = round & 1;
        if (cand >= 0 ? id == b_id : (lane == 0 && b_id == INT_MAX)) {          // the wave's winner, or lane 0 for a wave without a candidate
            L.r_iou[par][wave] = b_iou; L.r_id[par][wave] = b_id; L.r_slot[par][wave] = tid; L.r_det[par][wave] = cand;
        }
        __syncthreads();
        b_iou = L.r_iou[par][0]; b_id = L.r_id[par][0]; b_slot = L.r_slot[par][0]; b_det = L.r_det[par][0];
#pragma unroll
        for (int w = 1; w < 4; ++w) {
            const double o_iou = L.r_iou[par][w];
            const int o_id = L.r_id[par][w];
            if (o_iou > b_iou || (o_iou == b_iou && o_id < b_id)) { b_iou = o_iou; b_id = o_id; b_slot = L.r_slot[par][w]; b_det = L.r_det[par][w]; }
        }
        if (b_det < 0) break;                       // uniform: no pair is left.  The barrier above published the last d_slot entry
        if (tid == b_slot) { L.d_slot[b_det] = tid; matched = b_det; cand = -1; cand_iou = -INFINITY; }
        else if (cand == b_det) rescan = true;
        last = b_det;
    }
    __syncthreads();                                // the arg-max slots are free for the next stage
    return matched;
}

__global__ __launch_bounds__(DET_THREADS) void track_kernel(TrackArgs a) {
#pragma clang fp contract(off)
    __shared__ TrackLds L;
    const int s = blockIdx.x, tid = threadIdx.x;
    const long long row0 = (long long)s * a.D;
    if (a.active[s] == 0) {                         // uniform: the state is left alone, nothing is emitted
        for (int r = tid; r < a.D; r += DET_THREADS) {
            *reinterpret_cast<float4 *>(a.out_boxes + (row0 + r) * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
            a.out_labels[row0 + r] = 0; a.out_scores[row0 + r] = 0.f; a.out_query[row0 + r] = 0; a.out_ids[row0 + r] = 0; a.out_hits[row0 + r] = 0;
        }
        if (tid == 0) a.out_counts[s] = 0;
        return;
    }
    TrackState &st = a.state[s];
    int bad = 0;
    int n = a.counts[s];
    if (n < 0 || n > a.D) { bad |= DETR_TRACK_BAD_COUNT; n = 0; }

    // ---- 2: the detections of the frame
    for (int d = tid; d < n; d += DET_THREADS) {
        L.d_box[d] = *reinterpret_cast<const float4 *>(a.boxes + (row0 + d) * 4);
        L.d_label[d] = a.labels[row0 + d];
        L.d_score[d] = a.scores[row0 + d];
        L.d_slot[d] = -1;
    }
    L.spawn_det[tid] = -1;

    // ---- 1: this thread's slot, predicted
    float4 x = *reinterpret_cast<const float4 *>(st.x[tid]), v = *reinterpret_cast<const float4 *>(st.v[tid]);
    long long label = st.label[tid];
    float score = st.score[tid];
    int id = st.id[tid], hits = st.hits[tid], miss = st.miss[tid], conf = st.confirmed[tid];
    const int next_id = st.next_id, frame = st.frame;
    const bool live = id >= 1;
    float4 p = make_float4(x.x + v.x, x.y + v.y, x.z + v.z, x.w + v.w);
    p.z = p.z < 0.f ? 0.f : p.z;
    p.w = p.w < 0.f ? 0.f : p.w;
    const float4 pc = make_float4(p.x - p.z * 0.5f, p.y - p.w * 0.5f, p.x + p.z * 0.5f, p.y + p.w * 0.5f);
    __syncthreads();

    // ---- 3, 4: the two stages
    const int det1 = associate(L, a, n, live, pc, label, id, 1, a.thr_match);
    const int det2 = associate(L, a, n, live && det1 < 0 && conf != 0 && miss == 0, pc, label, id, 0, a.thr_low);
    const int det = det1 >= 0 ? det1 : det2;

    // ---- 5, 6: update or coast
    if (live) {
        if (det >= 0) {
            const float4 b = L.d_box[det];
            const float4 z = make_float4((b.x + b.z) * 0.5f, (b.y + b.w) * 0.5f, b.z - b.x, b.w - b.y);
            const float4 r = make_float4(z.x - p.x, z.y - p.y, z.z - p.z, z.w - p.w);
            x = make_float4(p.x + a.alpha * r.x, p.y + a.alpha * r.y, p.z + a.alpha * r.z, p.w + a.alpha * r.w);
            v = make_float4(v.x + a.beta * r.x, v.y + a.beta * r.y, v.z + a.beta * r.z, v.w + a.beta * r.w);
            hits += 1; miss = 0; score = L.d_score[det];
            conf = (conf != 0 || hits >= a.min_hits) ? 1 : 0;
        } else {
            x = p; miss += 1;
            if (conf == 0 || miss > a.max_age) {
                x = v = make_float4(0.f, 0.f, 0.f, 0.f);
                label = 0; score = 0.f; id = hits = miss = conf = 0;
            }
        }
    }

    // ---- 7: spawn.  The k-th unmatched high detection (score >= new_threshold) takes the k-th free slot
    const int n_free = compact_pass(id == 0, 0, L.wave_cnt, [&](int i, int) { L.free_slot[i] = tid; });
    int n_spawn = 0;                                // workgroup-uniform
    for (int d0 = 0; d0 < n; d0 += DET_THREADS) {
        const int d = d0 + tid;
        const bool want = d < n && L.d_slot[d] < 0 && L.d_score[d] >= a.thr_track && L.d_score[d] >= a.thr_new;
        n_spawn = compact_pass(want, n_spawn, L.wave_cnt, [&](int i, int) {
            if (i >= n_free) return;                // no slot is left: the detection is not tracked
            const int slot = L.free_slot[i];
            L.d_slot[d] = slot; L.spawn_det[slot] = d; L.spawn_rank[slot] = i;
        });
    }
    if (n_spawn > n_free) { bad |= DETR_TRACK_FULL; n_spawn = n_free; }
    if (L.spawn_det[tid] >= 0) {                    // published by compact_pass's closing barrier
        const int d = L.spawn_det[tid];
        const float4 b = L.d_box[d];
        x = make_float4((b.x + b.z) * 0.5f, (b.y + b.w) * 0.5f, b.z - b.x, b.w - b.y);
        v = make_float4(0.f, 0.f, 0.f, 0.f);
        label = L.d_label[d]; score = L.d_score[d];
        id = next_id + L.spawn_rank[tid]; hits = 1; miss = 0; conf = a.min_hits <= 1 ? 1 : 0;
    }
    L.t_id[tid] = id; L.t_hits[tid] = hits; L.t_conf[tid] = conf;

    // ---- the state goes back
    *reinterpret_cast<float4 *>(st.x[tid]) = x;
    *reinterpret_cast<float4 *>(st.v[tid]) = v;
    st.label[tid] = label; st.score[tid] = score;
    st.id[tid] = id; st.hits[tid] = hits; st.miss[tid] = miss; st.confirmed[tid] = conf;
    if (tid == 0) { st.frame = frame + 1; st.next_id = next_id + n_spawn; }
    __syncthreads();                                // t_id, t_hits, t_conf

    // ---- 8: emit, ascending detection index
    int count = 0;                                  // workgroup-uniform
    for (int d0 = 0; d0 < n; d0 += DET_THREADS) {
        const int d = d0 + tid;
        const int slot = d < n ? L.d_slot[d] : -1;
        const bool keep = slot >= 0 && L.t_conf[slot] != 0;
        count = compact_pass(keep, count, L.wave_cnt, [&](int i, int) {
            const long long row = row0 + i;
            *reinterpret_cast<float4 *>(a.out_boxes + row * 4) = L.d_box[d];
            a.out_labels[row] = L.d_label[d];
            a.out_scores[row] = L.d_score[d];
            a.out_query[row] = a.query ? a.query[row0 + d] : 0;
            a.out_ids[row] = L.t_id[slot];
            a.out_hits[row] = L.t_hits[slot];
        });
    }
    for (int r = count + tid; r < a.D; r += DET_THREADS) {
        const long long row = row0 + r;
        *reinterpret_cast<float4 *>(a.out_boxes + row * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
        a.out_labels[row] = 0; a.out_scores[row] = 0.f; a.out_query[row] = 0; a.out_ids[row] = 0; a.out_hits[row] = 0;
    }
    if (tid == 0) {
        a.out_counts[s] = count;
        if (bad) atomicOr(a.status, bad);
    }
}

}  // namespace detr

using namespace detr;

extern "C" int64_t detr_hip_track_state_bytes(int32_t streams) {
    if (streams < 1 || streams > 65535) {
        set_error("track_state_bytes: streams=%d must be in 1..65535", streams);
        return -1;
    }
    return (int64_t)streams * (int64_t)sizeof(TrackState);
}

extern "C" int detr_hip_track(const detr_track_desc *d, void *stream) {
    DETR_REQUIRE(d, "track: null descriptor");
    DETR_REQUIRE(d->state && d->boxes && d->labels && d->scores && d->counts && d->active,
                 "track: null operand (state, boxes, labels, scores, counts, active)");
    DETR_REQUIRE(d->out_boxes && d->out_labels && d->out_scores && d->out_query && d->out_ids && d->out_hits && d->out_counts && d->status,
                 "track: null operand (out_boxes, out_labels, out_scores, out_query, out_ids, out_hits, out_counts, status)");
    DETR_REQUIRE(d->S > 0 && d->S <= 65535 && d->D > 0 && d->D <= PP_MAXQ, "track: bad shape S=%d D=%d (S 1..65535, D 1..%d)", d->S, d->D, PP_MAXQ);
    DETR_REQUIRE(d->state_bytes >= (int64_t)d->S * (int64_t)sizeof(TrackState), "track: state of %lld bytes, %lld needed (detr_hip_track_state_bytes)",
                 (long long)d->state_bytes, (long long)d->S * (long long)sizeof(TrackState));
    DETR_REQUIRE(d->track_threshold - d->track_threshold == 0.f, "track: track_threshold is not finite");
    DETR_REQUIRE(d->new_threshold - d->new_threshold == 0.f, "track: new_threshold is not finite");
    DETR_REQUIRE(d->match_threshold - d->match_threshold == 0.0, "track: match_threshold is not finite");
    DETR_REQUIRE(d->low_match_threshold - d->low_match_threshold == 0.0, "track: low_match_threshold is not finite");
    DETR_REQUIRE(d->alpha - d->alpha == 0.f && d->beta - d->beta == 0.f, "track: alpha and beta must be finite");
    DETR_REQUIRE(d->max_age >= 0, "track: max_age=%d must be >= 0", d->max_age);
    DETR_REQUIRE(d->min_hits >= 1, "track: min_hits=%d must be >= 1", d->min_hits);
    DETR_REQUIRE(d->class_agnostic == 0 || d->class_agnostic == 1, "track: class_agnostic=%d must be 0 or 1", d->class_agnostic);
    DETR_REQUIRE(aligned16(d->state) && aligned16(d->boxes) && aligned16(d->out_boxes), "track: state, boxes and out_boxes must be 16-byte aligned");
    TrackArgs a;
    a.state = reinterpret_cast<TrackState *>(d->state);
    a.boxes = d->boxes; a.labels = reinterpret_cast<const long long *>(d->labels); a.scores = d->scores; a.query = d->query;
    a.counts = d->counts; a.active = d->active;
    a.D = d->D; a.max_age = d->max_age; a.min_hits = d->min_hits; a.agnostic = d->class_agnostic;
    a.thr_track = d->track_threshold; a.thr_new = d->new_threshold; a.alpha = d->alpha; a.beta = d->beta;
    a.thr_match = d->match_threshold; a.thr_low = d->low_match_threshold;
    a.out_boxes = d->out_boxes; a.out_labels = reinterpret_cast<long long *>(d->out_labels); a.out_scores = d->out_scores;
    a.out_query = d->out_query; a.out_ids = d->out_ids; a.out_hits = d->out_hits; a.out_counts = d->out_counts; a.status = d->status;
    hipLaunchKernelGGL(track_kernel, dim3(d->S), dim3(DET_THREADS), 0, (hipStream_t)stream, a);
    DETR_LAUNCH_CHECK("track");
    return 0;
}

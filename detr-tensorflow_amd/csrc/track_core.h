// track_core.h -- the ONE body of the trackers: detr_hip_track (track.hip, association by IoU) and detr_hip_track_embed
// (track_embed.hip, IoU blended with an appearance similarity, plus re-identification) are the two instances of track_kernel<EMBED>.
// Predict, the association rounds, update, spawn and emit are written once here; what differs is the measure functor handed to
// associate() and the parts inside `if constexpr (EMBED)`, which the plain instance does not contain: its bits are those of the
// kernel this file was cut out of.  include/detr_hip.h (detr_track_desc, detr_track_embed_desc) is the normative text.
// DET_THREADS == DETR_TRACK_MAX: thread t OWNS slot t, whose state stays in its registers from the load to the write-back; the
// detections of the frame are staged in LDS.
//   association (steps 3, 4 and the re-identification stage): the sequential walk over all pairs by descending (measure, then lower
//   id, then lower detection) is reproduced as rounds.  Every slot keeps the best detection still free in its row -- (measure, lower
//   index), the id is the row's --; a round takes the workgroup arg-max of those by (measure, lower id), which is the first pair of
//   the walk with both sides free; then only the slots whose cached best was that detection rescan their row.  One barrier per
//   matched pair (the arg-max slots are double-buffered), as tile_merge_kernel pays one per kept box.
//   spawn (step 7): the k-th unmatched high detection takes the k-th free slot, both lists from compact_pass of detections.h.
//   appearance (EMBED): the similarities the walks need are computed BEFORE them by whole waves into an fp64 table in global scratch
//   (sim_table), so a rescan reads a number, not two vectors; only pairs that pass the walk's own gate pay for a dot product.
// No atomics except the integer OR on the status word, no float atomics: a rerun from the same state(s) is bit-identical.
#pragma once
#include <type_traits>

#include "detections.h"

namespace detr {

constexpr int TRK_MAX = DETR_TRACK_MAX;
constexpr int TRK_MAX_E = 512;                      // longest embedding: 8 elements per lane
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

struct TrackEmbedArgs : TrackArgs {
    const float *embed;                             // [S, R, E], strides sE_s, sE_r in elements
    long long sE_s, sE_r;
    int R, E, reid;
    float *bank;                                    // [S, TRK_MAX, E]: the unit embedding of every slot
    double *table;                                  // [S, TRK_MAX, D] scratch: sim(slot, detection) of the gated pairs
    double w, w1, thr_reid;                         // appearance_weight, 1 - appearance_weight
    float momentum, momentum1;                      // momentum, 1 - momentum
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

// what the appearance instance holds on top: the detections' norms and what a WAVE must know of a slot it does not own
struct TrackEmbedLds {
    double d_nrm[PP_MAXQ];                          // |raw embedding| of a detection; 0 = it has the zero embedding
    float4 t_box[TRK_MAX];                          // by slot: the predicted corners
    long long t_label[TRK_MAX];
    int t_gate[TRK_MAX];                            // by slot: takes part in the table pass now being run
    int e_op[TRK_MAX], e_det[TRK_MAX];              // by slot: what happens to its bank row (EMB_*), and with which detection
};
struct TrackNoLds {};
static_assert(sizeof(TrackLds) + sizeof(TrackEmbedLds) <= 64 * 1024, "the static LDS limit of a workgroup");

enum { EMB_KEEP = 0, EMB_BLEND = 1, EMB_SET = 2, EMB_ZERO = 3 };

// One stage of the association.  `mine`: this thread's slot takes part; label / id: its label and id; want_high: the detections of
// this stage are the high (1) or the low (0) ones; measure(d, m): does the pair (this slot, detection d) pass the stage's gate, and
// if so m = the value the walk orders it by (a NaN m is no pair).  Returns the detection matched to this slot or -1.
// Every thread of the workgroup calls this, uniformly (it holds barriers and wave shuffles); on return the d_slot entries it wrote
// are visible to all threads.
template <class Measure>
__device__ __forceinline__ int associate(TrackLds &L, const TrackArgs &a, int n, bool mine, long long label, int id, int want_high, Measure measure) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int matched = -1, last = -1, cand = -1;
    double cand_iou = -INFINITY;
    bool rescan = mine;
    for (int round = 0;; ++round) {
        if (rescan) {                               // this slot's best detection still free: highest measure, lowest index on ties
            cand = -1; cand_iou = -INFINITY;
            for (int d = 0; d < n; ++d) {
                if (d == last || L.d_slot[d] >= 0) continue;          // `last` was taken in the round before: its flag may not be visible yet
                if ((L.d_score[d] >= a.thr_track ? 1 : 0) != want_high) continue;
                if (!a.agnostic && L.d_label[d] != label) continue;
                double iou;
                if (measure(d, iou) && iou > cand_iou) { cand_iou = iou; cand = d; }      // NaN fails both
            }
            rescan = false;
        }
        // workgroup arg-max by (measure, lower id): ids are unique, so the key names its slot and no further key is needed
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

// ---- appearance: every function below is called by whole waves, uniformly, and holds wave shuffles but no barrier ----------------

// dot64 of include/detr_hip.h: lane partials over k = lane, lane + 64, ... ascending, then the xor tree; every lane gets the value
template <class A, class B>
__device__ __forceinline__ double dot64(int E, A a_at, B b_at) {
#pragma clang fp contract(off)
    double p = 0.0;
    for (int k = threadIdx.x & 63; k < E; k += 64) p = p + (double)a_at(k) * (double)b_at(k);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) p = p + __shfl_xor(p, o, 64);
    return p;
}

// element k of the unit embedding of a detection with the raw row f and the norm nrm (0: the zero embedding, f is not read)
__device__ __forceinline__ float unit_elem(const float *f, int k, double nrm) {
    return nrm > 0.0 ? (float)((double)f[k] / nrm) : 0.f;
}

// the raw row of detection d of stream s; only called for a detection whose d_nrm is > 0, i.e. whose row index was found inside [0, R)
__device__ __forceinline__ const float *embed_row(const TrackEmbedArgs &a, int s, int d) {
    const int r = a.query ? a.query[(long long)s * a.D + d] : d;
    return a.embed + (long long)s * a.sE_s + (long long)r * a.sE_r;
}

// d_nrm of every detection, one wave per detection.  Returns DETR_TRACK_BAD_EMBED (wave-uniform) when the wave met a row index
// outside [0, R) or a non-finite row: such a detection gets the norm 0 and its row is never read again.
__device__ __forceinline__ int embed_norms(TrackEmbedLds &X, const TrackEmbedArgs &a, int s, int n) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int bad = 0;
    for (int d = wave; d < n; d += 4) {
        const int r = a.query ? a.query[(long long)s * a.D + d] : d;
        double nrm = 0.0;
        if (r < 0 || r >= a.R) bad |= DETR_TRACK_BAD_EMBED;
        else {
            const float *f = a.embed + (long long)s * a.sE_s + (long long)r * a.sE_r;
            auto at = [&](int k) { return f[k]; };
            nrm = sqrt(dot64(a.E, at, at));
            if (!(nrm - nrm == 0.0)) { bad |= DETR_TRACK_BAD_EMBED; nrm = 0.0; }      // a NaN or an infinity in the row
        }
        if (lane == 0) X.d_nrm[d] = nrm;
    }
    return bad;
}

// table[t][d] = sim(slot t, detection d) for every pair with t_gate[t] set and gate(t, d): wave w takes the slots t = w, w + 4, ...;
// its lanes evaluate the gate of 64 detections at once, and for every set bit of the ballot the whole wave computes one dot64 with
// coalesced reads.  The caller synchronises the workgroup before (t_gate, d_nrm, the staged detections) and after (the table).
template <class Gate>
__device__ __forceinline__ void sim_table(const TrackEmbedLds &X, const TrackEmbedArgs &a, int s, int n, Gate gate) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int t = wave; t < TRK_MAX; t += 4) {
        if (X.t_gate[t] == 0) continue;             // wave-uniform
        const float *e = a.bank + ((long long)s * TRK_MAX + t) * a.E;
        double *row = a.table + ((long long)s * TRK_MAX + t) * a.D;
        for (int d0 = 0; d0 < n; d0 += 64) {
            const int d = d0 + lane;
            unsigned long long todo = __ballot(d < n && gate(t, d));
            while (todo) {
                const int dd = d0 + __builtin_ctzll(todo);
                todo &= todo - 1;
                const double nrm = X.d_nrm[dd];
                const float *f = nrm > 0.0 ? embed_row(a, s, dd) : nullptr;
                const double sim = dot64(a.E, [&](int k) { return e[k]; }, [&](int k) { return unit_elem(f, k, nrm); });
                if (lane == 0) row[dd] = sim;
            }
        }
    }
}

// the bank rows after the frame: a slot matched by appearance (stage 1 or re-identification) blends its row with the detection's unit
// embedding and is normalised again, a spawned slot takes the detection's, a freed slot is zeroed.  The caller has synchronised e_op / e_det.
__device__ __forceinline__ void bank_update(const TrackEmbedLds &X, const TrackEmbedArgs &a, int s) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int t = wave; t < TRK_MAX; t += 4) {
        const int op = X.e_op[t];                   // wave-uniform
        if (op == EMB_KEEP) continue;
        float *e = a.bank + ((long long)s * TRK_MAX + t) * a.E;
        if (op == EMB_ZERO) {
            for (int k = lane; k < a.E; k += 64) e[k] = 0.f;
            continue;
        }
        const int d = X.e_det[t];
        const double nrm = X.d_nrm[d];
        const float *f = nrm > 0.0 ? embed_row(a, s, d) : nullptr;
        float u[TRK_MAX_E / 64];
        double p = 0.0;
#pragma unroll
        for (int j = 0; j < TRK_MAX_E / 64; ++j) {
            const int k = lane + 64 * j;
            u[j] = 0.f;
            if (k < a.E) {
                const float nk = unit_elem(f, k, nrm);
                u[j] = op == EMB_SET ? nk : a.momentum * e[k] + a.momentum1 * nk;
                p = p + (double)u[j] * (double)u[j];
            }
        }
        if (op == EMB_BLEND) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) p = p + __shfl_xor(p, o, 64);
            const double nu = sqrt(p);
            const double div = (nu > 0.0 && nu - nu == 0.0) ? nu : 0.0;
#pragma unroll
            for (int j = 0; j < TRK_MAX_E / 64; ++j) u[j] = div > 0.0 ? (float)((double)u[j] / div) : 0.f;
        }
#pragma unroll
        for (int j = 0; j < TRK_MAX_E / 64; ++j) {
            const int k = lane + 64 * j;
            if (k < a.E) e[k] = u[j];
        }
    }
}

template <bool EMBED>
__global__ __launch_bounds__(DET_THREADS) void track_kernel(const std::conditional_t<EMBED, TrackEmbedArgs, TrackArgs> a) {
#pragma clang fp contract(off)
    __shared__ TrackLds L;
    __shared__ std::conditional_t<EMBED, TrackEmbedLds, TrackNoLds> X;
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
    int bad_embed = 0;                              // wave-uniform, where `bad` is workgroup-uniform
    if constexpr (EMBED) {
        X.t_box[tid] = pc; X.t_label[tid] = label; X.t_gate[tid] = live ? 1 : 0;
        bad_embed = embed_norms(X, a, s, n);
    }
    __syncthreads();

    // ---- 3, 4: the two stages
    auto iou_above = [&](double thr) {
        return [pc, thr](int d, double &m) { m = match_measure(pc, L.d_box[d], 0); return m > thr; };
    };
    int det1, det3 = -1;
    if constexpr (EMBED) {
        const double *sim = a.table + ((long long)s * TRK_MAX + tid) * a.D;
        if (a.w != 0.0) {                           // uniform.  The same gate as the walk's, evaluated by the waves of sim_table
            sim_table(X, a, s, n, [&](int t, int d) {
                return L.d_score[d] >= a.thr_track && (a.agnostic || L.d_label[d] == X.t_label[t]) && match_measure(X.t_box[t], L.d_box[d], 0) > a.thr_match;
            });
            __syncthreads();
        }
        det1 = associate(L, a, n, live, label, id, 1, [&](int d, double &m) {
            const double iou = match_measure(pc, L.d_box[d], 0);
            if (!(iou > a.thr_match)) return false;
            m = a.w != 0.0 ? a.w1 * iou + a.w * sim[d] : iou;
            return true;
        });
    } else {
        det1 = associate(L, a, n, live, label, id, 1, iou_above(a.thr_match));
    }
    const int det2 = associate(L, a, n, live && det1 < 0 && conf != 0 && miss == 0, label, id, 0, iou_above(a.thr_low));
    const int det = det1 >= 0 ? det1 : det2;
    if constexpr (EMBED) {
        if (a.reid) {                               // uniform.  Re-identification: lost confirmed tracks against the new-track candidates, no IoU gate
            const bool lost = live && det < 0 && conf != 0 && miss >= 1;
            const double *sim = a.table + ((long long)s * TRK_MAX + tid) * a.D;
            X.t_gate[tid] = lost ? 1 : 0;
            __syncthreads();
            sim_table(X, a, s, n, [&](int t, int d) {
                return L.d_slot[d] < 0 && L.d_score[d] >= a.thr_track && L.d_score[d] >= a.thr_new && (a.agnostic || L.d_label[d] == X.t_label[t]);
            });
            __syncthreads();
            det3 = associate(L, a, n, lost, label, id, 1, [&](int d, double &m) {
                if (!(L.d_score[d] >= a.thr_new)) return false;
                m = sim[d];
                return m > a.thr_reid;
            });
        }
    }

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
        } else if (EMBED && det3 >= 0) {            // found again by appearance: the track restarts where the detection is
            const float4 b = L.d_box[det3];
            x = make_float4((b.x + b.z) * 0.5f, (b.y + b.w) * 0.5f, b.z - b.x, b.w - b.y);
            v = make_float4(0.f, 0.f, 0.f, 0.f);
            hits += 1; miss = 0; score = L.d_score[det3];
        } else {
            x = p; miss += 1;
            if (conf == 0 || miss > a.max_age) {
                x = v = make_float4(0.f, 0.f, 0.f, 0.f);
                label = 0; score = 0.f; id = hits = miss = conf = 0;
            }
        }
    }
    int e_op = EMB_KEEP, e_det = -1;                // stage 2 does not touch the bank
    if (live) {
        if (det1 >= 0) { e_op = EMB_BLEND; e_det = det1; }
        else if (det3 >= 0) { e_op = EMB_BLEND; e_det = det3; }
        else if (id == 0) e_op = EMB_ZERO;
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
        e_op = EMB_SET; e_det = d;
    }
    L.t_id[tid] = id; L.t_hits[tid] = hits; L.t_conf[tid] = conf;
    if constexpr (EMBED) { X.e_op[tid] = e_op; X.e_det[tid] = e_det; }

    // ---- the state goes back
    *reinterpret_cast<float4 *>(st.x[tid]) = x;
    *reinterpret_cast<float4 *>(st.v[tid]) = v;
    st.label[tid] = label; st.score[tid] = score;
    st.id[tid] = id; st.hits[tid] = hits; st.miss[tid] = miss; st.confirmed[tid] = conf;
    if (tid == 0) { st.frame = frame + 1; st.next_id = next_id + n_spawn; }
    __syncthreads();                                // t_id, t_hits, t_conf (and e_op, e_det)
    if constexpr (EMBED) bank_update(X, a, s);

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
    if (EMBED && (tid & 63) == 0 && bad_embed) atomicOr(a.status, bad_embed);
}

// ---- host side: the checks and the argument block the two entry points share, on the fields their descriptors have in common; `who`
// prefixes the messages.  Returns 0 or -1 with the error text set, like the entry points themselves.
template <class Desc>
static inline int check_track_desc(const char *who, const Desc *d) {
    DETR_REQUIRE(d->state && d->boxes && d->labels && d->scores && d->counts && d->active,
                 "%s: null operand (state, boxes, labels, scores, counts, active)", who);
    DETR_REQUIRE(d->out_boxes && d->out_labels && d->out_scores && d->out_query && d->out_ids && d->out_hits && d->out_counts && d->status,
                 "%s: null operand (out_boxes, out_labels, out_scores, out_query, out_ids, out_hits, out_counts, status)", who);
    DETR_REQUIRE(d->S > 0 && d->S <= 65535 && d->D > 0 && d->D <= PP_MAXQ, "%s: bad shape S=%d D=%d (S 1..65535, D 1..%d)", who, d->S, d->D, PP_MAXQ);
    DETR_REQUIRE(d->state_bytes >= (int64_t)d->S * (int64_t)sizeof(TrackState), "%s: state of %lld bytes, %lld needed (detr_hip_track_state_bytes)", who,
                 (long long)d->state_bytes, (long long)d->S * (long long)sizeof(TrackState));
    DETR_REQUIRE(d->track_threshold - d->track_threshold == 0.f, "%s: track_threshold is not finite", who);
    DETR_REQUIRE(d->new_threshold - d->new_threshold == 0.f, "%s: new_threshold is not finite", who);
    DETR_REQUIRE(d->match_threshold - d->match_threshold == 0.0, "%s: match_threshold is not finite", who);
    DETR_REQUIRE(d->low_match_threshold - d->low_match_threshold == 0.0, "%s: low_match_threshold is not finite", who);
    DETR_REQUIRE(d->alpha - d->alpha == 0.f && d->beta - d->beta == 0.f, "%s: alpha and beta must be finite", who);
    DETR_REQUIRE(d->max_age >= 0, "%s: max_age=%d must be >= 0", who, d->max_age);
    DETR_REQUIRE(d->min_hits >= 1, "%s: min_hits=%d must be >= 1", who, d->min_hits);
    DETR_REQUIRE(d->class_agnostic == 0 || d->class_agnostic == 1, "%s: class_agnostic=%d must be 0 or 1", who, d->class_agnostic);
    DETR_REQUIRE(aligned16(d->state) && aligned16(d->boxes) && aligned16(d->out_boxes), "%s: state, boxes and out_boxes must be 16-byte aligned", who);
    return 0;
}

template <class Desc>
static inline void fill_track_args(TrackArgs &a, const Desc *d) {
    a.state = reinterpret_cast<TrackState *>(d->state);
    a.boxes = d->boxes; a.labels = reinterpret_cast<const long long *>(d->labels); a.scores = d->scores; a.query = d->query;
    a.counts = d->counts; a.active = d->active;
    a.D = d->D; a.max_age = d->max_age; a.min_hits = d->min_hits; a.agnostic = d->class_agnostic;
    a.thr_track = d->track_threshold; a.thr_new = d->new_threshold; a.alpha = d->alpha; a.beta = d->beta;
    a.thr_match = d->match_threshold; a.thr_low = d->low_match_threshold;
    a.out_boxes = d->out_boxes; a.out_labels = reinterpret_cast<long long *>(d->out_labels); a.out_scores = d->out_scores;
    a.out_query = d->out_query; a.out_ids = d->out_ids; a.out_hits = d->out_hits; a.out_counts = d->out_counts; a.status = d->status;
}

}  // namespace detr

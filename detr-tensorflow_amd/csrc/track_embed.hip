// track_embed.hip -- tracking by appearance: detr_hip_track with an embedding per detection.  A track that coasts through an occlusion
// drifts off its object and the object comes back under a new id; two objects of one class that pass each other hand their ids to
// whichever box overlaps more.  Both are decided here by what the objects LOOK like: stage 1 orders its pairs by a blend of IoU and
// the cosine similarity to the track's stored embedding, and a lost track is found again by similarity alone (include/detr_hip.h:
// detr_track_embed_desc is the normative text).  The kernel is track_kernel<true> of track_core.h -- the body of detr_hip_track with
// the appearance parts compiled in --; this file holds the entry point, its checks and the size queries.
#include "track_core.h"

using namespace detr;

static int64_t table_bytes(int32_t S, int32_t D) { return (int64_t)S * TRK_MAX * (int64_t)D * (int64_t)sizeof(double); }

extern "C" int64_t detr_hip_track_embed_state_bytes(int32_t streams, int32_t embed_dim) {
    if (streams < 1 || streams > 65535 || embed_dim < 4 || embed_dim > TRK_MAX_E || embed_dim % 4 != 0) {
        set_error("track_embed_state_bytes: streams=%d must be in 1..65535 and embed_dim=%d a multiple of 4 in 4..%d", streams, embed_dim, TRK_MAX_E);
        return -1;
    }
    return (int64_t)streams * TRK_MAX * (int64_t)embed_dim * (int64_t)sizeof(float);
}

extern "C" int64_t detr_hip_workspace_bytes_track_embed(const detr_track_embed_desc *d) {
    if (!d || d->S < 1 || d->S > 65535 || d->D < 1 || d->D > PP_MAXQ) {
        set_error("workspace_bytes_track_embed: bad shape (S 1..65535, D 1..%d)", PP_MAXQ);
        return -1;
    }
    return table_bytes(d->S, d->D);
}

extern "C" int detr_hip_track_embed(const detr_track_embed_desc *d, void *stream) {
    DETR_REQUIRE(d, "track_embed: null descriptor");
    if (check_track_desc("track_embed", d)) return -1;
    DETR_REQUIRE(d->embed && d->embed_state && d->workspace, "track_embed: null operand (embed, embed_state, workspace)");
    DETR_REQUIRE(d->R >= 1 && d->E >= 4 && d->E <= TRK_MAX_E && d->E % 4 == 0, "track_embed: bad shape R=%d E=%d (R >= 1, E a multiple of 4 in 4..%d)",
                 d->R, d->E, TRK_MAX_E);
    DETR_REQUIRE(d->sE_r >= d->E && d->sE_s >= 0, "track_embed: strides sE_s=%lld (>= 0) sE_r=%lld (>= E) are too small", (long long)d->sE_s,
                 (long long)d->sE_r);
    const int64_t bank = (int64_t)d->S * TRK_MAX * (int64_t)d->E * (int64_t)sizeof(float), table = table_bytes(d->S, d->D);
    DETR_REQUIRE(d->embed_state_bytes >= bank, "track_embed: embed_state of %lld bytes, %lld needed (detr_hip_track_embed_state_bytes)",
                 (long long)d->embed_state_bytes, (long long)bank);
    DETR_REQUIRE(d->workspace_bytes >= table, "track_embed: workspace of %lld bytes, %lld needed (detr_hip_workspace_bytes_track_embed)",
                 (long long)d->workspace_bytes, (long long)table);
    DETR_REQUIRE(d->appearance_weight >= 0.0 && d->appearance_weight <= 1.0, "track_embed: appearance_weight=%g must be in [0, 1]", d->appearance_weight);
    DETR_REQUIRE(d->reid == 0 || d->reid == 1, "track_embed: reid=%d must be 0 or 1", d->reid);
    DETR_REQUIRE(d->reid_threshold - d->reid_threshold == 0.0, "track_embed: reid_threshold is not finite");
    DETR_REQUIRE(d->momentum >= 0.f && d->momentum <= 1.f, "track_embed: momentum=%g must be in [0, 1]", (double)d->momentum);
    DETR_REQUIRE(aligned16(d->embed) && aligned16(d->embed_state) && aligned16(d->workspace),
                 "track_embed: embed, embed_state and workspace must be 16-byte aligned");
    TrackEmbedArgs a;
    fill_track_args(a, d);
    a.embed = d->embed; a.sE_s = d->sE_s; a.sE_r = d->sE_r; a.R = d->R; a.E = d->E; a.reid = d->reid;
    a.bank = reinterpret_cast<float *>(d->embed_state); a.table = reinterpret_cast<double *>(d->workspace);
    a.w = d->appearance_weight; a.w1 = 1.0 - d->appearance_weight; a.thr_reid = d->reid_threshold;
    a.momentum = d->momentum; a.momentum1 = 1.0f - d->momentum;
    hipLaunchKernelGGL(track_kernel<true>, dim3(d->S), dim3(DET_THREADS), 0, (hipStream_t)stream, a);
    DETR_LAUNCH_CHECK("track_embed");
    return 0;
}

// track.hip -- multi-object tracking across video frames: which detection of this frame is the object of the last one.  The reference's
// only end-to-end program is a video loop (webcam_inference.py:26-34) that treats every frame as the first; a user writes the
// association as a NumPy loop over tracks x detections on detections read back every frame.  Here ONE launch serves a batch of
// frames, one workgroup per video stream, the tracks of a stream in device memory (include/detr_hip.h: detr_track_desc gives the
// algorithm, steps 1..8, and the state layout).  The kernel is track_kernel<false> of track_core.h, the body this entry point shares
// with detr_hip_track_embed (track_embed.hip): association by IoU alone, no appearance.
#include "track_core.h"

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
    if (check_track_desc("track", d)) return -1;
    TrackArgs a;
    fill_track_args(a, d);
    hipLaunchKernelGGL(track_kernel<false>, dim3(d->S), dim3(DET_THREADS), 0, (hipStream_t)stream, a);
    DETR_LAUNCH_CHECK("track");
    return 0;
}

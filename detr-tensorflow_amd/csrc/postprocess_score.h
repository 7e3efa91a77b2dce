// postprocess_score.h -- the per-query softmax statistics shared by postprocess.hip and detect.hip: both kernels run THIS code, so
// the score and the label of a query are bit-identical whichever entry point produced them.
#pragma once
#include "common.h"

namespace detr {

constexpr int PP_MAXQ = 1024;     // queries of one image held in LDS

// One wave per query, 4 waves: s_score[q] = max softmax probability, s_label[q] = first arg-max of the PROBABILITIES
// (inference.py:73-75 takes argmax(softmax)) of the logit rows lg[q * sl_q + 0 .. C), q < Q.  The caller synchronises the workgroup.
__device__ __forceinline__ void query_scores_labels(const float *lg, long long sl_q, int Q, int C, float *s_score, int *s_label) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int q = wave; q < Q; q += 4) {
        const float *row = lg + q * sl_q;
        float mx = -INFINITY;
        for (int c = lane; c < C; c += 64) mx = fmaxf(mx, row[c]);
        mx = wave_max(mx);
        float s = 0.f;
        for (int c = lane; c < C; c += 64) s += expf(row[c] - mx);
        s = wave_sum(s);
        // arg-max of the PROBABILITIES (inference.py:75 takes argmax(softmax)), first occurrence on ties
        float best = -1.f;
        int arg = INT_MAX;
        for (int c = lane; c < C; c += 64) {
            const float p = expf(row[c] - mx) / s;
            if (p > best) { best = p; arg = c; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ob = __shfl_xor(best, o, 64);
            const int oa = __shfl_xor(arg, o, 64);
            if (ob > best || (ob == best && oa < arg)) { best = ob; arg = oa; }
        }
        if (lane == 0) { s_score[q] = best; s_label[q] = arg; }
    }
}

}  // namespace detr

// track_motion.hip -- camera-motion compensation for the trackers: a global translation per stream and frame, estimated from the frames
// themselves and added to the track positions before detr_hip_track / detr_hip_track_embed associate (include/detr_hip.h:
// detr_track_motion_desc is the normative text, steps 1..6).  A camera that jitters moves every box at once, which no per-track
// velocity can learn; what is needed is ONE vector per frame, and block matching on a small luma thumbnail finds it.
// Three launches, everything integer up to the fp32 add that moves a track:
//   motion_thumb_kernel  one workgroup per (thumbnail row, stream): the f x f box filter of the luma into the slot of the motion state
//                        the previous frame does not occupy.
//   motion_match_kernel  one workgroup per (block, stream): the (16 + 2R)^2 window of the previous thumbnail and the 16 x 16 block of the
//                        current one are staged in LDS as dwords; the (2R + 1)^2 candidates are strided over the threads, four pixels
//                        per v_sad_u8 with the window's dwords shifted into place by v_alignbyte; a workgroup min over the packed key
//                        (SAD, dx^2 + dy^2, dy, dx) leaves one vote in the workspace.
//   motion_final_kernel  one workgroup per stream: histograms of the votes' dx and dy in LDS give the lower medians, a second pass the
//                        agreement; thread t then moves slot t of the track state, thread 0 writes the header and out_motion.
// The grids are sized for the largest thumbnail (the sizes are in device memory): a workgroup without work returns at once.
// Every kernel derives the same geometry from (sizes, offsets, header) with motion_geo; only the last launch changes the header.
#include "track_core.h"

namespace detr {

constexpr int MO_SIDE = DETR_MOTION_SIDE, MO_BLOCK = DETR_MOTION_BLOCK, MO_MAX_R = DETR_MOTION_MAX_RADIUS;
constexpr int MO_MAX_GRID = (MO_SIDE - 2) / MO_BLOCK;                     // blocks per side at R = 1
constexpr int MO_MAX_BLOCKS = MO_MAX_GRID * MO_MAX_GRID;                   // 529
constexpr int MO_MAX_WIN = MO_BLOCK + 2 * MO_MAX_R;                        // 48: side of the search window
constexpr int MO_MAX_STRIDE = (MO_MAX_WIN + 3) / 4 + 1;                    // 13 dwords: a window row plus the dword the funnel shift reads behind it
constexpr int MO_THUMB_THREADS = 128;
static_assert(MO_BLOCK == 16, "motion_match_kernel: one thread per pixel of a block, four dwords per block row");
static_assert(MO_SIDE % MO_THUMB_THREADS == 0, "a thumbnail row is a whole number of passes");

// head[] of include/detr_hip.h
enum { MH_H = 0, MH_W, MH_F, MH_TW, MH_TH, MH_VALID, MH_SLOT, MH_EST, MH_SX, MH_SY, MH_N, MH_AGREE };

struct MotionState {
    int head[16];
    unsigned char thumb[2][MO_SIDE * MO_SIDE];
};
static_assert(sizeof(MotionState) % 16 == 0, "streams stay 16-byte aligned");

struct MotionArgs {
    const unsigned char *frames;
    long long frames_bytes;
    const long long *offsets;                       // [S]
    const int *sizes;                               // [S, 2]
    const int *active;                              // [S]
    int R;
    MotionState *motion;
    TrackState *state;
    int *votes;                                     // [S, MO_MAX_BLOCKS, 2]: valid, (dy + 16) << 6 | (dx + 16)
    int *out;                                       // [S, 6]
    int *status;
};

struct MotionGeo {
    const unsigned char *frame;
    int h, w, f, tw, th, gx, gy, slot;              // slot: where the PREVIOUS thumbnail is
    bool bad, exists;
};

// Steps 1 and 2 for stream s, from memory no launch of this call has written yet.  A frame that does not lie inside
// [frames, frames + frames_bytes) or has a side outside 1..DETR_OVERLAY_MAX_SIDE is run as 0 x 0: none of its bytes is addressed.
__device__ __forceinline__ MotionGeo motion_geo(const MotionArgs &a, int s) {
    MotionGeo g;
    g.h = a.sizes[2 * s]; g.w = a.sizes[2 * s + 1];
    const long long off = a.offsets[s];
    g.bad = g.h < 1 || g.h > DETR_OVERLAY_MAX_SIDE || g.w < 1 || g.w > DETR_OVERLAY_MAX_SIDE || off < 0 ||
            off > a.frames_bytes || 3LL * g.h * g.w > a.frames_bytes - off;
    if (g.bad) g.h = g.w = 0;
    g.frame = a.frames + (g.bad ? 0 : off);
    const int fw = (g.w + MO_SIDE - 1) / MO_SIDE, fh = (g.h + MO_SIDE - 1) / MO_SIDE;
    g.f = fw > fh ? fw : fh;
    g.f = g.f < 1 ? 1 : g.f;
    g.tw = g.w / g.f; g.th = g.h / g.f;
    g.gx = g.tw >= 2 * a.R + MO_BLOCK ? (g.tw - 2 * a.R) / MO_BLOCK : 0;
    g.gy = g.th >= 2 * a.R + MO_BLOCK ? (g.th - 2 * a.R) / MO_BLOCK : 0;
    const int *head = a.motion[s].head;
    g.slot = head[MH_SLOT] & 1;
    g.exists = head[MH_VALID] == 1 && head[MH_H] == g.h && head[MH_W] == g.w && g.gx >= 1 && g.gy >= 1;
    return g;
}

__global__ __launch_bounds__(MO_THUMB_THREADS) void motion_thumb_kernel(const MotionArgs a) {
    const int s = blockIdx.y, i = blockIdx.x;
    if (a.active[s] == 0) return;
    const MotionGeo g = motion_geo(a, s);
    if (i >= g.th) return;                          // uniform
    unsigned char *dst = a.motion[s].thumb[g.slot ^ 1] + i * g.tw;
    const int f = g.f, cell = f * f;
    for (int j = threadIdx.x; j < g.tw; j += MO_THUMB_THREADS) {
        int sum = 0;                                // <= 86 * 86 * 255
        for (int yy = 0; yy < f; ++yy) {
            const unsigned char *p = g.frame + ((long long)(i * f + yy) * g.w + (long long)j * f) * 3;
            for (int xx = 0; xx < f; ++xx, p += 3) sum += (77 * p[0] + 150 * p[1] + 29 * p[2] + 128) >> 8;
        }
        dst[j] = (unsigned char)(sum / cell);
    }
}

__global__ __launch_bounds__(DET_THREADS) void motion_match_kernel(const MotionArgs a) {
    __shared__ unsigned int s_prev[MO_MAX_WIN * MO_MAX_STRIDE];     // the window, row stride `stride` dwords, zeros behind a row's end
    __shared__ unsigned int s_cur[MO_BLOCK * MO_BLOCK / 4];
    __shared__ int s_min[4], s_max[4];
    __shared__ unsigned long long s_key[4];
    const int s = blockIdx.y, b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (a.active[s] == 0) return;
    const MotionGeo g = motion_geo(a, s);
    if (!g.exists || b >= g.gx * g.gy) return;      // uniform
    const int R = a.R, bx = b % g.gx, by = b / g.gx;
    const int win = MO_BLOCK + 2 * R, stride = (win + 3) / 4 + 1;
    const unsigned char *cur = a.motion[s].thumb[g.slot ^ 1] + (R + MO_BLOCK * by) * g.tw + R + MO_BLOCK * bx;
    const unsigned char *prev = a.motion[s].thumb[g.slot] + (MO_BLOCK * by) * g.tw + MO_BLOCK * bx;
    int *vote = a.votes + ((long long)s * MO_MAX_BLOCKS + b) * 2;

    // the block: thread t holds pixel (t / 16, t % 16); four neighbouring lanes pack their bytes into one dword
    const int px = cur[(tid >> 4) * g.tw + (tid & 15)];
    unsigned int word = (unsigned int)px << (8 * (tid & 3));
    word |= __shfl_xor(word, 1, 64);
    word |= __shfl_xor(word, 2, 64);
    if ((tid & 3) == 0) s_cur[tid >> 2] = word;
    int mn = px, mx = px;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int on = __shfl_xor(mn, o, 64), ox = __shfl_xor(mx, o, 64);
        mn = on < mn ? on : mn; mx = ox > mx ? ox : mx;
    }
    if (lane == 0) { s_min[wave] = mn; s_max[wave] = mx; }
    // the window
    for (int idx = tid; idx < win * stride; idx += DET_THREADS) {
        const int row = idx / stride, c = idx - row * stride;
        unsigned int v = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (4 * c + k < win) v |= (unsigned int)prev[row * g.tw + 4 * c + k] << (8 * k);
        s_prev[idx] = v;
    }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < 4; ++w) { mn = s_min[w] < mn ? s_min[w] : mn; mx = s_max[w] > mx ? s_max[w] : mx; }
    if (mx - mn < DETR_MOTION_MIN_CONTRAST) {       // uniform: a flat block has no vote
        if (tid == 0) { vote[0] = 0; vote[1] = 0; }
        return;
    }

    const int side = 2 * R + 1;
    unsigned long long best = ~0ull;
    for (int c = tid; c < side * side; c += DET_THREADS) {
        const int dyi = c / side, dxi = c - dyi * side, dx = dxi - R, dy = dyi - R;
        const int o = R - dx, q = o >> 2;           // cur(x, y) meets prev(x - dx, y - dy): window column o + j, row R - dy + i
        const unsigned int sh = (unsigned int)(o & 3);
        const unsigned int *pr = s_prev + (R - dy) * stride + q;
        unsigned int sad = 0;
#pragma unroll 4
        for (int i = 0; i < MO_BLOCK; ++i, pr += stride) {
            const unsigned int w0 = pr[0], w1 = pr[1], w2 = pr[2], w3 = pr[3], w4 = pr[4];
            sad = __builtin_amdgcn_sad_u8(s_cur[4 * i + 0], __builtin_amdgcn_alignbyte(w1, w0, sh), sad);
            sad = __builtin_amdgcn_sad_u8(s_cur[4 * i + 1], __builtin_amdgcn_alignbyte(w2, w1, sh), sad);
            sad = __builtin_amdgcn_sad_u8(s_cur[4 * i + 2], __builtin_amdgcn_alignbyte(w3, w2, sh), sad);
            sad = __builtin_amdgcn_sad_u8(s_cur[4 * i + 3], __builtin_amdgcn_alignbyte(w4, w3, sh), sad);
        }
        const unsigned long long key = ((unsigned long long)sad << 22) | ((unsigned long long)(dx * dx + dy * dy) << 12) |
                                       ((unsigned long long)(dy + 16) << 6) | (unsigned long long)(dx + 16);
        best = key < best ? key : best;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(best, o, 64);
        best = other < best ? other : best;
    }
    if (lane == 0) s_key[wave] = best;
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < 4; ++w) best = s_key[w] < best ? s_key[w] : best;
        vote[0] = 1; vote[1] = (int)(best & 0xfffu);
    }
}

__global__ __launch_bounds__(DET_THREADS) void motion_final_kernel(const MotionArgs a) {
    __shared__ int s_hx[2 * MO_MAX_R + 1], s_hy[2 * MO_MAX_R + 1];
    __shared__ int s_n, s_mx, s_my, s_agree;
    const int s = blockIdx.x, tid = threadIdx.x;
    int *out = a.out + 6 * s;
    if (a.active[s] == 0) {                         // uniform: both states are left alone
        if (tid < 6) out[tid] = 0;
        return;
    }
    const MotionGeo g = motion_geo(a, s);           // every thread reads the header here, thread 0 writes it behind the barriers below
    const int R = a.R, blocks = g.exists ? g.gx * g.gy : 0;
    const int *votes = a.votes + (long long)s * MO_MAX_BLOCKS * 2;
    if (tid < 2 * MO_MAX_R + 1) { s_hx[tid] = 0; s_hy[tid] = 0; }
    if (tid == 0) s_agree = 0;
    __syncthreads();
    for (int b = tid; b < blocks; b += DET_THREADS)
        if (votes[2 * b]) {
            const int v = votes[2 * b + 1];
            atomicAdd(&s_hx[(v & 63) - 16 + R], 1);
            atomicAdd(&s_hy[(v >> 6) - 16 + R], 1);
        }
    __syncthreads();
    if (tid == 0) {                                 // the lower medians: the value at index (n - 1) / 2 of each sorted list
        int n = 0;
        for (int k = 0; k <= 2 * R; ++k) n += s_hx[k];
        int mx = 0, my = 0;
        if (n >= DETR_MOTION_MIN_BLOCKS) {
            const int want = (n - 1) / 2;
            int seen = 0;
            for (int k = 0; k <= 2 * R; ++k) { seen += s_hx[k]; if (seen > want) { mx = k - R; break; } }
            seen = 0;
            for (int k = 0; k <= 2 * R; ++k) { seen += s_hy[k]; if (seen > want) { my = k - R; break; } }
        }
        s_n = n; s_mx = mx; s_my = my;
    }
    __syncthreads();
    const int n = s_n, mdx = s_mx, mdy = s_my;
    if (n >= DETR_MOTION_MIN_BLOCKS) {              // uniform
        int mine = 0;
        for (int b = tid; b < blocks; b += DET_THREADS)
            if (votes[2 * b]) {
                const int v = votes[2 * b + 1], ex = (v & 63) - 16 - mdx, ey = (v >> 6) - 16 - mdy;
                mine += (ex >= -1 && ex <= 1 && ey >= -1 && ey <= 1) ? 1 : 0;
            }
        if (mine) atomicAdd(&s_agree, mine);
        __syncthreads();
    }
    const int agree = s_agree;
    const int est = (n >= DETR_MOTION_MIN_BLOCKS && 2 * agree >= n) ? 1 : 0;
    const int sx = est ? mdx * g.f : 0, sy = est ? mdy * g.f : 0;
    if (est) {                                      // thread t owns slot t
        TrackState &st = a.state[s];
        if (st.id[tid] >= 1) {
            st.x[tid][0] = st.x[tid][0] + (float)sx;
            st.x[tid][1] = st.x[tid][1] + (float)sy;
        }
    }
    if (tid == 0) {
        int *head = a.motion[s].head;
        head[MH_H] = g.h; head[MH_W] = g.w; head[MH_F] = g.f; head[MH_TW] = g.tw; head[MH_TH] = g.th;
        head[MH_VALID] = 1; head[MH_SLOT] = g.slot ^ 1;
        head[MH_EST] = est; head[MH_SX] = sx; head[MH_SY] = sy; head[MH_N] = n; head[MH_AGREE] = agree;
        head[12] = head[13] = head[14] = head[15] = 0;
        out[0] = est; out[1] = sx; out[2] = sy; out[3] = n; out[4] = agree; out[5] = g.f;
        if (g.bad) atomicOr(a.status, DETR_TRACK_BAD_FRAME);
    }
}

static int64_t votes_bytes(int32_t S) { return (int64_t)S * MO_MAX_BLOCKS * 2 * (int64_t)sizeof(int32_t); }

}  // namespace detr

using namespace detr;

static_assert(TRK_MAX == DET_THREADS, "motion_final_kernel: thread t owns slot t");

extern "C" int64_t detr_hip_track_motion_state_bytes(int32_t streams) {
    if (streams < 1 || streams > 65535) {
        set_error("track_motion_state_bytes: streams=%d must be in 1..65535", streams);
        return -1;
    }
    return (int64_t)streams * (int64_t)sizeof(MotionState);
}

extern "C" int64_t detr_hip_workspace_bytes_track_motion(const detr_track_motion_desc *d) {
    if (!d || d->S < 1 || d->S > 65535) {
        set_error("workspace_bytes_track_motion: bad shape (S 1..65535)");
        return -1;
    }
    return votes_bytes(d->S);
}

extern "C" int detr_hip_track_motion(const detr_track_motion_desc *d, void *stream) {
    DETR_REQUIRE(d, "track_motion: null descriptor");
    DETR_REQUIRE(d->frames && d->offsets && d->sizes && d->active && d->motion_state && d->state && d->workspace && d->out_motion && d->status,
                 "track_motion: null operand (frames, offsets, sizes, active, motion_state, state, workspace, out_motion, status)");
    DETR_REQUIRE(d->S > 0 && d->S <= 65535, "track_motion: bad shape S=%d (S 1..65535)", d->S);
    DETR_REQUIRE(d->radius >= 1 && d->radius <= MO_MAX_R, "track_motion: radius=%d must be in 1..%d", d->radius, MO_MAX_R);
    DETR_REQUIRE(d->frames_bytes >= 1, "track_motion: frames_bytes=%lld must be positive", (long long)d->frames_bytes);
    const int64_t motion = (int64_t)d->S * (int64_t)sizeof(MotionState), tracks = (int64_t)d->S * (int64_t)sizeof(TrackState);
    DETR_REQUIRE(d->motion_state_bytes >= motion, "track_motion: motion_state of %lld bytes, %lld needed (detr_hip_track_motion_state_bytes)",
                 (long long)d->motion_state_bytes, (long long)motion);
    DETR_REQUIRE(d->state_bytes >= tracks, "track_motion: state of %lld bytes, %lld needed (detr_hip_track_state_bytes)", (long long)d->state_bytes,
                 (long long)tracks);
    DETR_REQUIRE(d->workspace_bytes >= votes_bytes(d->S), "track_motion: workspace of %lld bytes, %lld needed (detr_hip_workspace_bytes_track_motion)",
                 (long long)d->workspace_bytes, (long long)votes_bytes(d->S));
    DETR_REQUIRE(aligned16(d->motion_state) && aligned16(d->state) && aligned16(d->workspace),
                 "track_motion: motion_state, state and workspace must be 16-byte aligned");
    DETR_REQUIRE((reinterpret_cast<uintptr_t>(d->offsets) & 7) == 0 && (reinterpret_cast<uintptr_t>(d->sizes) & 3) == 0 &&
                     (reinterpret_cast<uintptr_t>(d->active) & 3) == 0 && (reinterpret_cast<uintptr_t>(d->out_motion) & 3) == 0 &&
                     (reinterpret_cast<uintptr_t>(d->status) & 3) == 0,
                 "track_motion: offsets must be 8-byte aligned, sizes, active, out_motion and status 4-byte aligned");
    MotionArgs a;
    a.frames = d->frames; a.frames_bytes = d->frames_bytes; a.offsets = reinterpret_cast<const long long *>(d->offsets);
    a.sizes = d->sizes; a.active = d->active; a.R = d->radius;
    a.motion = reinterpret_cast<MotionState *>(d->motion_state); a.state = reinterpret_cast<TrackState *>(d->state);
    a.votes = reinterpret_cast<int *>(d->workspace); a.out = d->out_motion; a.status = d->status;
    hipLaunchKernelGGL(motion_thumb_kernel, dim3(MO_SIDE, d->S), dim3(MO_THUMB_THREADS), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(motion_match_kernel, dim3(MO_MAX_BLOCKS, d->S), dim3(DET_THREADS), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(motion_final_kernel, dim3(d->S), dim3(DET_THREADS), 0, (hipStream_t)stream, a);
    DETR_LAUNCH_CHECK("track_motion");
    return 0;
}

// common.hip -- error reporting and trivial entry points of libdetr_hip.so.
#include "common.h"
#include <string.h>

namespace detr {
static thread_local char g_err[512] = "";
void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
static const char *const g_tune_names[T_COUNT] = {
    "DETR_HIP_GEMM_TILE",
    "DETR_HIP_SPLIT_XCD",
    "DETR_HIP_GEMM_STREAM",
    "DETR_HIP_GEMM_GROUP",
    "DETR_HIP_STREAM_SL",
    "DETR_HIP_STREAM_NW",
    "DETR_HIP_CONV_HALO",
    "DETR_HIP_CONV_TILE",
    "DETR_HIP_DGRAD_S2_CLASSES",
    "DETR_HIP_WGRAD_FUSED",
    "DETR_HIP_WGRAD_FUSED_WGS",
    "DETR_HIP_WGRAD_TILE",
    "DETR_HIP_STEM_ROWS",
    "DETR_HIP_ATTN_WAVES",
    "DETR_HIP_ATTN_SPLIT",
    "DETR_HIP_GEMM_K64",
    "DETR_HIP_EPI_WIDE",
    "DETR_HIP_SLAB_TS",
    "DETR_HIP_GEMM_RING",
    "DETR_HIP_RING_NS",
    "DETR_HIP_RING_BN",
    "DETR_HIP_RING_WGS",
    "DETR_HIP_RING_ROWS",
    "DETR_HIP_RING_WTILE",
    "DETR_HIP_CONV_DMA",
    "DETR_HIP_SPLIT3_T128",
    "DETR_HIP_X3_DB",
    "DETR_HIP_X3_T192",
    "DETR_HIP_X3_WG_ROUNDS",
    "DETR_HIP_X3_CONV",
    "DETR_HIP_SPLIT3_ALL",
    "DETR_HIP_SPLIT_TARGET",
    "DETR_HIP_SPLIT_TARGET64",
    "DETR_HIP_X3_SPLIT_TARGET",
};
static int g_tune[T_COUNT];
static void load_tuning() {
    for (int i = 0; i < T_COUNT; ++i) {
        const char *v = getenv(g_tune_names[i]);
        __atomic_store_n(&g_tune[i], v ? atoi(v) : 0, __ATOMIC_RELAXED);
    }
}
static const bool g_tune_loaded = (load_tuning(), true);      // at library load (dlopen), before any entry point can run
int tune(TuneKey k) { return __atomic_load_n(&g_tune[k], __ATOMIC_RELAXED); }
}  // namespace detr

extern "C" int detr_hip_reload_tuning(void) {
    detr::load_tuning();
    return 0;
}
extern "C" const char *detr_hip_last_error(void) { return detr::g_err; }
extern "C" int detr_hip_abi_version(void) { return DETR_HIP_ABI_VERSION; }
// Zero fill as an ordinary KERNEL, not hipMemsetAsync: a memset node captured into a hipGraph (eval-forward / train-step
// replay) was observed to fill with stale non-zero patterns after other work had run between replays (the decoder's zero
// target read 1e-28 .. 5e-9 instead of 0 on the replay that followed an eager training step; a kernel node replays exactly).
__global__ __launch_bounds__(256) void zero_fill_kernel(uint4 *__restrict__ p16, size_t n16, unsigned char *__restrict__ tail, int ntail) {
    const uint4 z = make_uint4(0u, 0u, 0u, 0u);
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n16; i += (size_t)gridDim.x * blockDim.x) p16[i] = z;
    if (blockIdx.x == 0 && (int)threadIdx.x < ntail) tail[threadIdx.x] = 0;
}

extern "C" int detr_hip_memset_zero(void *ptr, size_t bytes, void *stream) {
    if (bytes == 0) return 0;
    unsigned char *b = reinterpret_cast<unsigned char *>(ptr);
    const size_t head = (16 - (reinterpret_cast<uintptr_t>(b) & 15)) & 15;          // bytes up to the first 16-byte boundary
    if (head >= bytes || bytes < 64) {                                                // tiny or unaligned-only: byte stores
        if (bytes > 255) { detr::set_error("memset_zero: %zu unaligned bytes", bytes); return -2; }
        hipLaunchKernelGGL(zero_fill_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, nullptr, (size_t)0, b, (int)bytes);
    } else {
        if (head) hipLaunchKernelGGL(zero_fill_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, nullptr, (size_t)0, b, (int)head);
        const size_t n16 = (bytes - head) / 16;
        const int ntail = (int)((bytes - head) % 16);
        size_t grid = (n16 + 255) / 256;
        if (grid > 2048) grid = 2048;
        if (grid < 1) grid = 1;
        hipLaunchKernelGGL(zero_fill_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<uint4 *>(b + head), n16,
                           b + head + n16 * 16, ntail);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        detr::set_error("memset_zero: %s", hipGetErrorString(e));
        return -2;
    }
    return 0;
}
// ---- ABI layout self-check ---------------------------------------------------------------------------------------------
// A foreign binder mirrors the descriptor structs of include/detr_hip.h by hand (ctypes / cgo / JNI).  This entry point
// reports what THIS build of the library sees: for struct `which`, out[0] = sizeof and out[1..] = offsetof of every field in
// declaration order.  The binding compares them with its own mirror at load time (detr_tf/_hip.py: check_struct_layouts).
// A new descriptor takes one field list and one line of DETR_LAYOUTS; a field appended to a struct is appended to its list (the
// static_assert below fails the build until it is).
#include <stddef.h>
#define DETR_REDUCE_FIELDS(F) F(ws) F(splits) F(part_stride) F(rows) F(cols) F(C) F(ldc) F(alpha) F(scale) F(rs_ws) F(rs_out) \
    F(rs_alpha) F(ts_bm) F(ts_bn) F(ts_tiles_n)
#define DETR_GEMM_FIELDS(F) F(M) F(N) F(K) F(A) F(lda) F(a_kcontig) F(B) F(ldb) F(b_kcontig) F(C) F(ldc) F(batch) F(batch_inner) \
    F(sA0) F(sA1) F(sB0) F(sB1) F(sC0) F(sC1) F(alpha) F(scale) F(bias) F(residual) F(ldr) F(mask) F(ldmask) F(act) F(split_k) \
    F(workspace) F(workspace_bytes) F(dropout_p) F(dropout_seed) F(compute) F(rowsum_a) F(rowsum_alpha) F(b_dtype) F(a_dtype) \
    F(c_dtype) F(r_dtype) F(m_dtype) F(dropout_step) F(defer_out) F(maskbits_out) F(ld_maskbits_out) F(ln_gamma) F(ln_beta) \
    F(ln_y) F(ln_mean) F(ln_rstd) F(ln_add) F(ln_add_rows) F(ln_y2) F(ln_y16) F(ln_eps) F(res_sub_h) F(res_sub_w) F(res_sub_ho) \
    F(res_sub_wo)
#define DETR_CONV3X3_FIELDS(F) F(N) F(Hi) F(Wi) F(Ci) F(Ho) F(Wo) F(Co) F(stride) F(pad) F(x) F(w) F(y) F(alpha) F(scale) F(bias) \
    F(residual) F(mask) F(act) F(split) F(workspace) F(workspace_bytes) F(compute) F(w_dtype) F(x_dtype) F(y_dtype) F(r_dtype) \
    F(m_dtype) F(maskbits_out)
#define DETR_STEM_FIELDS(F) F(N) F(H) F(W) F(Ho) F(Wo) F(img) F(w) F(y) F(alpha) F(scale) F(bias) F(act) F(split) F(workspace) \
    F(workspace_bytes) F(compute) F(w_dtype) F(y_dtype)
#define DETR_LAYERNORM_FIELDS(F) F(rows) F(C) F(eps) F(x) F(gamma) F(beta) F(y) F(mean) F(rstd) F(add) F(add_rows) F(y2) F(y16) \
    F(dy) F(dx) F(dgamma) F(dbeta) F(workspace) F(workspace_bytes) F(dx_add) F(dx_drop) F(dropout_p) F(dropout_site) \
    F(dropout_step) F(dx_drop16) F(defer_blocks_out) F(dy_add)
#define DETR_ATTN_FIELDS(F) F(B) F(H) F(T) F(S) F(q) F(ldq) F(k) F(ldk) F(v) F(ldv) F(o) F(ldo) F(lse) F(d_o) F(ldd_o) F(dq) \
    F(lddq) F(dk) F(lddk) F(dv) F(lddv) F(delta) F(scale) F(dropout_p) F(dropout_site) F(dropout_step) F(compute) F(io_dtype) \
    F(dropmask)
#define DETR_SETLOSS_FIELDS(F) F(levels) F(B) F(Q) F(C) F(R) F(logits) F(sL_l) F(sL_b) F(sL_q) F(boxes) F(sB_l) F(sB_b) F(sB_q) \
    F(t_bbox) F(t_class) F(background_class)
#define DETR_INPUT_FIELDS(F) F(B) F(Hs) F(Ws) F(Hd) F(Wd) F(src) F(src_batch_stride) F(dst) F(lut) F(perm) F(interpolation)
#define DETR_POSTPROCESS_FIELDS(F) F(B) F(Q) F(C) F(logits) F(sL_b) F(sL_q) F(boxes) F(sB_b) F(sB_q) F(background_class) \
    F(bbox_format) F(out_boxes) F(out_labels) F(out_scores) F(counts)
#define DETR_MAP_MATCH_FIELDS(F) F(B) F(Q) F(R) F(nb_class) F(n_thr) F(boxes) F(labels) F(scores) F(counts) F(sD_b) F(t_bbox) \
    F(sT_b) F(t_class) F(sC_b) F(thresholds) F(rec_score) F(rec_class) F(rec_flags) F(num_gt) F(status)
#define DETR_DETECT_FIELDS(F) F(B) F(Q) F(C) F(logits) F(sL_b) F(sL_q) F(boxes) F(sB_b) F(sB_q) F(sizes) F(background_class) \
    F(score_threshold) F(max_detections) F(bbox_format) F(clip) F(out_boxes) F(out_labels) F(out_scores) F(out_query) F(counts)
#define DETR_TILE_MERGE_FIELDS(F) F(B) F(N) F(Q) F(C) F(logits) F(sL_b) F(sL_q) F(boxes) F(sB_b) F(sB_q) F(tile_start) \
    F(tile_start_host) F(windows) F(sizes) F(background_class) F(score_threshold) F(max_detections) F(bbox_format) F(clip) \
    F(match) F(class_agnostic) F(edge_margin) F(nms_threshold) F(out_boxes) F(out_labels) F(out_scores) F(out_query) F(out_tile) \
    F(counts) F(status)
#define DETR_OVERLAY_FIELDS(F) F(B) F(D) F(src) F(src_off) F(dst) F(dst_off) F(sizes) F(sizes_host) F(boxes) F(labels) F(scores) \
    F(counts) F(thickness) F(label_alpha) F(fill_alpha) F(colors) F(n_colors) F(names) F(name_len) F(n_names) F(name_cap) F(atlas) \
    F(n_glyph) F(gh) F(gw) F(glyph_digit0) F(glyph_colon) F(glyph_dot) F(scale) F(heat) F(sH_b) F(sH_y) F(sH_x) F(Hf) F(Wf) \
    F(map_step) F(map_valid) F(map_scale) F(lut) F(heat_alpha) F(workspace) F(workspace_bytes) F(status)
#define DETR_TRACK_FIELDS(F) F(S) F(D) F(state) F(state_bytes) F(boxes) F(labels) F(scores) F(query) F(counts) F(active) \
    F(track_threshold) F(new_threshold) F(match_threshold) F(low_match_threshold) F(max_age) F(min_hits) F(alpha) F(beta) \
    F(class_agnostic) F(out_boxes) F(out_labels) F(out_scores) F(out_query) F(out_ids) F(out_hits) F(out_counts) F(status)
#define DETR_TRACK_EMBED_FIELDS(F) DETR_TRACK_FIELDS(F) F(embed) F(sE_s) F(sE_r) F(R) F(E) F(embed_state) F(embed_state_bytes) \
    F(workspace) F(workspace_bytes) F(appearance_weight) F(reid) F(reid_threshold) F(momentum)
#define DETR_TRACK_MOTION_FIELDS(F) F(S) F(frames) F(frames_bytes) F(offsets) F(sizes) F(active) F(radius) F(motion_state) \
    F(motion_state_bytes) F(state) F(state_bytes) F(workspace) F(workspace_bytes) F(out_motion) F(status)
#define DETR_CONV3X3D_FIELDS(F) DETR_CONV3X3_FIELDS(F) F(dilation)
#define DETR_COCO_MATCH_FIELDS(F) F(B) F(Q) F(R) F(nb_class) F(n_thr) F(n_area) F(boxes) F(labels) F(scores) F(counts) F(sD_b) \
    F(t_bbox) F(sT_b) F(t_class) F(sC_b) F(t_crowd) F(t_area) F(sM_b) F(sizes) F(thresholds) F(area_ranges) F(rec_score) \
    F(rec_class) F(rec_rank) F(rec_flags) F(npig) F(status)
// id, struct, field list.  The ids are ABI (include/detr_hip.h); the id behind each one stays unknown.
#define DETR_LAYOUTS(X) \
    X(0, detr_reduce_desc, DETR_REDUCE_FIELDS) X(1, detr_gemm_desc, DETR_GEMM_FIELDS) X(2, detr_conv3x3_desc, DETR_CONV3X3_FIELDS) \
    X(3, detr_stem_desc, DETR_STEM_FIELDS) X(4, detr_layernorm_desc, DETR_LAYERNORM_FIELDS) X(5, detr_attn_desc, DETR_ATTN_FIELDS) \
    X(6, detr_setloss_desc, DETR_SETLOSS_FIELDS) X(7, detr_input_desc, DETR_INPUT_FIELDS) \
    X(8, detr_postprocess_desc, DETR_POSTPROCESS_FIELDS) X(9, detr_map_match_desc, DETR_MAP_MATCH_FIELDS) \
    X(100, detr_detect_desc, DETR_DETECT_FIELDS) X(200, detr_tile_merge_desc, DETR_TILE_MERGE_FIELDS) \
    X(300, detr_overlay_desc, DETR_OVERLAY_FIELDS) X(400, detr_track_desc, DETR_TRACK_FIELDS) \
    X(500, detr_track_embed_desc, DETR_TRACK_EMBED_FIELDS) X(600, detr_track_motion_desc, DETR_TRACK_MOTION_FIELDS) \
    X(700, detr_conv3x3d_desc, DETR_CONV3X3D_FIELDS) X(800, detr_coco_match_desc, DETR_COCO_MATCH_FIELDS)
// per struct: values[] = {sizeof, offsetof ...} as the entry point reports them, and ends[] = where each field ends -- the last
// listed field, rounded up to the struct's alignment, must close the struct
#define DETR_OFF(f) (int32_t)offsetof(ST, f),
#define DETR_END(f) offsetof(ST, f) + sizeof(ST::f),
#define DETR_DEFINE(id, S, FIELDS)                                                                                          \
    namespace layout_##S {                                                                                                  \
    using ST = S;                                                                                                           \
    constexpr int32_t values[] = {(int32_t)sizeof(ST), FIELDS(DETR_OFF)};                                                   \
    constexpr size_t ends[] = {FIELDS(DETR_END)};                                                                           \
    constexpr size_t last = ends[sizeof(ends) / sizeof(ends[0]) - 1];                                                       \
    static_assert((last + alignof(ST) - 1) / alignof(ST) * alignof(ST) == sizeof(ST), #S ": its field list stops before the struct ends"); \
    }
DETR_LAYOUTS(DETR_DEFINE)
#define DETR_ENTRY(id, S, FIELDS) {id, layout_##S::values, (int32_t)(sizeof(layout_##S::values) / sizeof(int32_t))},
static const struct { int32_t id; const int32_t *values; int32_t count; } g_layouts[] = {DETR_LAYOUTS(DETR_ENTRY)};

extern "C" int detr_hip_struct_layout(int32_t which, int32_t *out, int32_t cap) {
    for (const auto &e : g_layouts) {
        if (e.id != which) continue;
        for (int32_t i = 0; i < e.count && i < cap; ++i) out[i] = e.values[i];
        return e.count;        // number of values (may exceed cap: call again with a larger buffer)
    }
    detr::set_error("struct_layout: unknown struct %d", which);
    return -1;
}

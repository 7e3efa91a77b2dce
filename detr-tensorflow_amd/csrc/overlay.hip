// overlay.hip -- boxes, name:score labels and an attention heat map drawn onto uint8 RGB frames, for a ragged batch, on the device
// (the reference draws with cv2.rectangle / cv2.putText per box on the host: numpy_bbox_to_image, inference.py:10-65).  The rules --
// integer geometry, paint order, blend, label layout, score digits, the fp32 operation order of the heat map -- are stated in
// include/detr_hip.h: detr_overlay_desc; tests/overlay_ref.py restates them in NumPy and the comparison is exact.
// Two launches:
//   overlay_prep_kernel, one workgroup per image: validates every box, rank-sorts the valid ones by descending integer area (ties by
//     index) ONCE per image and writes, in paint order, one 48-byte command per box (corners, label rectangle, colour, text length) plus
//     its label text as glyph indices (name, ':', d.dd -- the score is formatted here, so nothing is read back) into the workspace;
//   overlay_raster_kernel, one workgroup per run of OV_TILE consecutive pixels of an image (blockIdx.y = image): a thread owns 4
//     consecutive pixels = 12 bytes, which are dword-aligned in a 4-byte aligned destination image whatever its width.  The source
//     bytes come as aligned dwords shifted into place (v_alignbyte), so an unaligned source image costs one more dword per thread, not
//     byte loads.  The heat map is blended first.  Then the command list is walked in passes of OV_LIST commands, PER WAVE: every lane
//     tests one command against the wave's run of 256 pixels (rows, and columns on the first / last row; without a tint a run that lies
//     wholly inside a box's outline touches nothing of it), a ballot compaction copies the hits to the wave's LDS list in order, and the
//     wave's pixels walk that short list -- a wave-uniform loop, so a wave in a box's interior does no per-pixel work for it.  A pass
//     can hit at most OV_LIST commands, so the list cannot overflow; a run that more boxes touch simply takes more passes, carrying
//     the running pixel value in registers.  Nothing is ever truncated.
// No atomics except the integer OR on the status word; every output byte is written by exactly one thread.
#include "common.h"

namespace detr {

constexpr int OV_THREADS = 256;
constexpr int OV_PX = 4;                          // pixels per thread: 12 bytes = 3 dwords
constexpr int OV_TILE = OV_THREADS * OV_PX;       // pixels per workgroup
constexpr int OV_WAVES = OV_THREADS / 64;
constexpr int OV_LIST = 64;                       // LDS command list of ONE wave: one cull pass, a command per lane
constexpr int OV_MAXD = DETR_TILE_MAX_CAND;
constexpr int OV_CMD_INTS = 12;                   // x1 y1 x2 y2 | lx0 ly0 lx1 ly1 | n_chars colour rank -

struct OvLayout {
    long long n_off, cmd_off, text_off, total;
    int text_cap;
};

static OvLayout ov_layout(int B, int D, int name_cap) {
    OvLayout l;
    l.text_cap = (name_cap + 5 + 3) & ~3;          // name, ':', d.dd
    l.n_off = 0;
    l.cmd_off = ((long long)B * 4 + 255) & ~255LL;
    l.text_off = l.cmd_off + (((long long)B * D * OV_CMD_INTS * 4 + 255) & ~255LL);
    l.total = l.text_off + (long long)B * D * l.text_cap;
    return l;
}

struct OvArgs {
    const unsigned char *src; const long long *src_off;
    unsigned char *dst; const long long *dst_off;
    const int *sizes;                               // [B, 2]
    const float *boxes; const long long *labels; const float *scores; const int *counts;
    int D, thickness, label_alpha, fill_alpha;
    const unsigned char *colors; int n_colors;
    const unsigned char *names; const int *name_len; int n_names, name_cap;
    const unsigned char *atlas; int n_glyph, gh, gw;
    int glyph_digit0, glyph_colon, glyph_dot;
    const int *scale;
    const float *heat; long long sh_b, sh_y, sh_x; int Hf, Wf;
    const float *map_step; const int *map_valid; const float *map_scale; const unsigned char *lut; int heat_alpha;
    int *ws_n; int *ws_cmd; unsigned char *ws_text; int text_cap;
    int *status;
};

__device__ __forceinline__ int ov_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ int ov_blend(int c, int p, int a) { return (c * a + p * (255 - a) + 127) / 255; }

// integer corners of detection i of image b; false when the box is skipped
__device__ __forceinline__ bool ov_corners(const OvArgs &a, long long row, int H, int W, int &x1, int &y1, int &x2, int &y2) {
    const float4 bx = *reinterpret_cast<const float4 *>(a.boxes + row * 4);
    if (!(isfinite(bx.x) && isfinite(bx.y) && isfinite(bx.z) && isfinite(bx.w))) return false;
    if (bx.z < bx.x || bx.w < bx.y) return false;
    if (a.labels[row] < 0) return false;
    const float fw = (float)(W - 1), fh = (float)(H - 1);
    x1 = (int)fminf(fmaxf(floorf(bx.x), 0.f), fw);
    x2 = (int)fminf(fmaxf(floorf(bx.z), 0.f), fw);
    y1 = (int)fminf(fmaxf(floorf(bx.y), 0.f), fh);
    y2 = (int)fminf(fmaxf(floorf(bx.w), 0.f), fh);
    return true;
}

__global__ __launch_bounds__(OV_THREADS) void overlay_prep_kernel(OvArgs a) {
    __shared__ long long s_area[OV_MAXD];          // -1: skipped
    const int b = blockIdx.x, tid = threadIdx.x;
    const int H = a.sizes[2 * b], W = a.sizes[2 * b + 1];
    int cnt = a.counts[b];
    if (cnt < 0 || cnt > a.D) {
        if (tid == 0) atomicOr(a.status, DETR_OVERLAY_BAD_COUNT);
        cnt = ov_clampi(cnt, 0, a.D);
    }
    if (H <= 0 || W <= 0) cnt = 0;
    const int s = ov_clampi(a.scale[b], 1, DETR_OVERLAY_MAX_SCALE);
    const int t = a.thickness;
    const long long row0 = (long long)b * a.D;

    for (int i = tid; i < cnt; i += OV_THREADS) {
        int x1, y1, x2, y2;
        const bool ok = ov_corners(a, row0 + i, H, W, x1, y1, x2, y2);
        s_area[i] = ok ? (long long)(x2 - x1) * (long long)(y2 - y1) : -1LL;
    }
    __syncthreads();

    int n = 0;                                      // workgroup-uniform
    for (int i0 = 0; i0 < cnt; i0 += OV_THREADS) {
        const int i = i0 + tid;
        const long long area = i < cnt ? s_area[i] : -1LL;
        const bool valid = area >= 0;
        if (valid) {
            int rank = 0;
            for (int j = 0; j < cnt; ++j) {
                const long long aj = s_area[j];
                rank += (aj > area || (aj == area && j < i)) ? 1 : 0;
            }
            int x1, y1, x2, y2;
            ov_corners(a, row0 + i, H, W, x1, y1, x2, y2);
            const long long label = a.labels[row0 + i];
            const bool named = label < a.n_names;                       // label >= 0 here
            const bool scored = a.scores != nullptr;
            int len = 0;
            if (named) len = ov_clampi(a.name_len[label], 0, a.name_cap);
            unsigned char *text = a.ws_text + (row0 + rank) * a.text_cap;
            for (int k = 0; k < len; ++k) text[k] = a.names[label * a.name_cap + k];
            int nch = len;
            if (scored) {
                const double qd = rint((double)a.scores[row0 + i] * 100.0);
                const int q = qd >= 999.0 ? 999 : (qd > 0.0 ? (int)qd : 0);       // NaN fails both comparisons: 0
                if (named) text[nch++] = (unsigned char)a.glyph_colon;
                text[nch++] = (unsigned char)(a.glyph_digit0 + q / 100);
                text[nch++] = (unsigned char)a.glyph_dot;
                text[nch++] = (unsigned char)(a.glyph_digit0 + q / 10 % 10);
                text[nch++] = (unsigned char)(a.glyph_digit0 + q % 10);
            }
            int lx0 = 0, ly0 = 0, lx1 = -1, ly1 = -1;                   // empty: no label rectangle
            if (named || scored) {
                const int pad = t + s;
                const int width = nch * a.gw * s + 2 * pad, height = a.gh * s + 2 * pad;
                lx0 = max(0, min(x1, W - width));
                ly0 = max(0, min(y1, H - height));
                lx1 = min(lx0 + width - 1, W - 1);
                ly1 = min(ly0 + height - 1, H - 1);
            }
            const unsigned char *col = a.colors + (label % a.n_colors) * 3;
            const int R = col[0], G = col[1], Bc = col[2];
            const int white = (299 * R + 587 * G + 114 * Bc >= 128000) ? 0 : 1;
            int4 *cmd = reinterpret_cast<int4 *>(a.ws_cmd + (row0 + rank) * OV_CMD_INTS);
            cmd[0] = make_int4(x1, y1, x2, y2);
            cmd[1] = make_int4(lx0, ly0, lx1, ly1);
            cmd[2] = make_int4(nch, R | (G << 8) | (Bc << 16) | (white << 24), rank, 0);
        }
        n += __syncthreads_count(valid ? 1 : 0);
    }
    if (tid == 0) a.ws_n[b] = n;
}

// does the command's footprint (box and label rectangle) touch the pixel run [first row ya from column xa .. last row yb to column xb]?
__device__ __forceinline__ bool ov_rect_hits(int rx0, int ry0, int rx1, int ry1, int ya, int xa, int yb, int xb) {
    if (rx1 < rx0 || ry1 < ry0 || ry1 < ya || ry0 > yb) return false;
    if (ya == yb) return rx1 >= xa && rx0 <= xb;
    if (ry0 <= ya && rx1 >= xa) return true;                            // the first row, from xa on
    if (ry1 >= yb && rx0 <= xb) return true;                            // the last row, up to xb
    return max(ry0, ya + 1) <= min(ry1, yb - 1);                        // a whole row in between
}

__global__ __launch_bounds__(OV_THREADS) void overlay_raster_kernel(OvArgs a) {
    __shared__ int4 s_cmd[OV_WAVES * OV_LIST * 3];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int H = a.sizes[2 * b], W = a.sizes[2 * b + 1];
    if (H <= 0 || W <= 0) return;
    if (H > DETR_OVERLAY_MAX_SIDE || W > DETR_OVERLAY_MAX_SIDE) return;  // (the entry point checked the host copy: pixel indices fit 32 bits)
    const int P = H * W;                                                // <= 2^30
    const int t0 = blockIdx.x * OV_TILE;
    if (t0 >= P) return;                                                // uniform
    const int r0 = t0 + wave * (64 * OV_PX);                            // the run of this wave, inclusive; it may lie behind the image
    const int r1 = min(r0 + 64 * OV_PX, P) - 1;
    const bool has_run = r0 < P;
    const unsigned uW = (unsigned)W;
    const int ya = (int)((unsigned)r0 / uW), xa = r0 - ya * W;
    const int yb = has_run ? (int)((unsigned)r1 / uW) : ya, xb = has_run ? r1 - yb * W : xa;

    const int p0 = t0 + tid * OV_PX;
    const int np = max(0, min(OV_PX, P - p0));                          // pixels this thread owns
    int py[OV_PX], px[OV_PX];
    {
        int y = (int)((unsigned)p0 / uW), x = p0 - y * W;
#pragma unroll
        for (int j = 0; j < OV_PX; ++j) {
            py[j] = y; px[j] = x;
            if (++x == W) { x = 0; ++y; }
        }
    }

    // ---- source bytes
    union { unsigned int w[3]; unsigned char c[12]; } u;
    u.w[0] = u.w[1] = u.w[2] = 0;
    const unsigned char *sp = a.src + a.src_off[b] + 3LL * p0;
    if (np == OV_PX) {
        const unsigned int sh = (unsigned int)(reinterpret_cast<uintptr_t>(sp) & 3);
        const unsigned int *q = reinterpret_cast<const unsigned int *>(sp - sh);     // every dword read holds a byte of this thread
        const unsigned int w0 = q[0], w1 = q[1], w2 = q[2];
        if (sh == 0) {
            u.w[0] = w0; u.w[1] = w1; u.w[2] = w2;
        } else {
            const unsigned int w3 = q[3];
            u.w[0] = __builtin_amdgcn_alignbyte(w1, w0, sh);
            u.w[1] = __builtin_amdgcn_alignbyte(w2, w1, sh);
            u.w[2] = __builtin_amdgcn_alignbyte(w3, w2, sh);
        }
    } else {
        for (int k = 0; k < 3 * np; ++k) u.c[k] = sp[k];
    }
    int r[OV_PX], g[OV_PX], bl[OV_PX];
#pragma unroll
    for (int j = 0; j < OV_PX; ++j) { r[j] = u.c[3 * j]; g[j] = u.c[3 * j + 1]; bl[j] = u.c[3 * j + 2]; }

    // ---- heat map, on the source pixel
    if (a.heat != nullptr) {
        const float sy = a.map_step[2 * b], sx = a.map_step[2 * b + 1];
        const int vh = ov_clampi(a.map_valid[2 * b], 1, a.Hf), vw = ov_clampi(a.map_valid[2 * b + 1], 1, a.Wf);
        const float ms = a.map_scale[b];
        const float *hb = a.heat + b * a.sh_b;
#pragma unroll
        for (int j = 0; j < OV_PX; ++j) {
            if (j >= np) break;
            float fy = ((float)py[j] + 0.5f) * sy - 0.5f;
            fy = fminf(fmaxf(fy, 0.f), (float)(vh - 1));
            float fx = ((float)px[j] + 0.5f) * sx - 0.5f;
            fx = fminf(fmaxf(fx, 0.f), (float)(vw - 1));
            const int y0 = ov_clampi((int)floorf(fy), 0, vh - 1), x0 = ov_clampi((int)floorf(fx), 0, vw - 1);    // (a NaN step: still in bounds)
            const float wy = fy - (float)y0, wx = fx - (float)x0;
            const int y1 = min(y0 + 1, vh - 1), x1 = min(x0 + 1, vw - 1);
            const float m00 = hb[y0 * a.sh_y + x0 * a.sh_x], m01 = hb[y0 * a.sh_y + x1 * a.sh_x];
            const float m10 = hb[y1 * a.sh_y + x0 * a.sh_x], m11 = hb[y1 * a.sh_y + x1 * a.sh_x];
            const float top = m00 + wx * (m01 - m00);
            const float bot = m10 + wx * (m11 - m10);
            const float m = top + wy * (bot - top);
            float v = m * ms;
            v = v > 0.f ? fminf(v, 1.f) : 0.f;
            const int idx = (int)(v * 255.0f + 0.5f);
            const int al = (int)(v * (float)a.heat_alpha + 0.5f);
            const unsigned char *c = a.lut + 3 * idx;
            r[j] = ov_blend(c[0], r[j], al); g[j] = ov_blend(c[1], g[j], al); bl[j] = ov_blend(c[2], bl[j], al);
        }
    }

    // ---- boxes: cull OV_LIST commands per pass into LDS (order kept), walk the hits
    const int n = min(max(a.ws_n[b], 0), a.D);
    const int s = ov_clampi(a.scale[b], 1, DETR_OVERLAY_MAX_SCALE);
    const int t = a.thickness, pad = t + s;
    const int gws = a.gw * s, ghs = a.gh * s;
    const long long row0 = (long long)b * a.D;
    int4 *w_cmd = s_cmd + wave * OV_LIST * 3;
    for (int base = 0; base < n; base += OV_LIST) {                      // n is workgroup-uniform: so are the barriers
        const int c = base + lane;
        bool hit = false;
        int4 c0, c1, c2;
        if (c < n && has_run) {
            const int4 *cmd = reinterpret_cast<const int4 *>(a.ws_cmd + (row0 + c) * OV_CMD_INTS);
            c0 = cmd[0]; c1 = cmd[1]; c2 = cmd[2];
            // without a tint a single-row run wholly inside [x1 + t, x2 - t] x [y1 + t, y2 - t] sees nothing of the box
            const bool inner = a.fill_alpha == 0 && ya == yb && ya >= c0.y + t && ya <= c0.w - t && xa >= c0.x + t && xb <= c0.z - t;
            hit = (!inner && ov_rect_hits(c0.x, c0.y, c0.z, c0.w, ya, xa, yb, xb)) || ov_rect_hits(c1.x, c1.y, c1.z, c1.w, ya, xa, yb, xb);
        }
        const unsigned long long m = __ballot(hit);
        const int total = __popcll(m);                                   // wave-uniform
        if (hit) {
            const int i = __popcll(m & ((1ull << lane) - 1ull));
            w_cmd[3 * i] = c0; w_cmd[3 * i + 1] = c1; w_cmd[3 * i + 2] = c2;
        }
        __syncthreads();
        for (int k = 0; k < total; ++k) {
            const int4 d0 = w_cmd[3 * k], d1 = w_cmd[3 * k + 1], d2 = w_cmd[3 * k + 2];
            const int cr = d2.y & 255, cg = (d2.y >> 8) & 255, cb = (d2.y >> 16) & 255;
            const int tc = (d2.y >> 24) ? 255 : 0;
            const unsigned char *text = a.ws_text + (row0 + d2.z) * a.text_cap;
#pragma unroll
            for (int j = 0; j < OV_PX; ++j) {
                const int x = px[j], y = py[j];
                const bool inbox = x >= d0.x && x <= d0.z && y >= d0.y && y <= d0.w;
                if (inbox && a.fill_alpha) {
                    r[j] = ov_blend(cr, r[j], a.fill_alpha); g[j] = ov_blend(cg, g[j], a.fill_alpha); bl[j] = ov_blend(cb, bl[j], a.fill_alpha);
                }
                if (x >= d1.x && x <= d1.z && y >= d1.y && y <= d1.w) {
                    r[j] = ov_blend(cr, r[j], a.label_alpha); g[j] = ov_blend(cg, g[j], a.label_alpha); bl[j] = ov_blend(cb, bl[j], a.label_alpha);
                    const int tx = x - d1.x - pad, ty = y - d1.y - pad;
                    if (tx >= 0 && ty >= 0 && tx < d2.x * gws && ty < ghs) {
                        const int ci = tx / gws;
                        const int gx = (tx - ci * gws) / s, gy = ty / s;
                        const int gl = text[ci];
                        if (gl < a.n_glyph && a.atlas[(gl * a.gh + gy) * a.gw + gx] != 0) { r[j] = tc; g[j] = tc; bl[j] = tc; }
                    }
                }
                if (inbox && !(x >= d0.x + t && x <= d0.z - t && y >= d0.y + t && y <= d0.w - t)) { r[j] = cr; g[j] = cg; bl[j] = cb; }
            }
        }
        __syncthreads();                                                // the list is rewritten by the next pass
    }

    // ---- store
    if (np <= 0) return;
#pragma unroll
    for (int j = 0; j < OV_PX; ++j) { u.c[3 * j] = (unsigned char)r[j]; u.c[3 * j + 1] = (unsigned char)g[j]; u.c[3 * j + 2] = (unsigned char)bl[j]; }
    unsigned char *dp = a.dst + a.dst_off[b] + 3LL * p0;
    if (np == OV_PX && (reinterpret_cast<uintptr_t>(dp) & 3) == 0) {
        unsigned int *q = reinterpret_cast<unsigned int *>(dp);
        q[0] = u.w[0]; q[1] = u.w[1]; q[2] = u.w[2];
    } else {
        for (int k = 0; k < 3 * np; ++k) dp[k] = u.c[k];
    }
}

}  // namespace detr

using namespace detr;

static int overlay_check_shape(const detr_overlay_desc *d) {
    DETR_REQUIRE(d, "overlay: null descriptor");
    DETR_REQUIRE(d->B > 0 && d->B <= 65535 && d->D > 0 && d->D <= OV_MAXD, "overlay: bad shape B=%d D=%d (B 1..65535, D 1..%d)", d->B, d->D, OV_MAXD);
    DETR_REQUIRE(d->name_cap >= 1 && d->name_cap <= DETR_OVERLAY_MAX_NAME, "overlay: name_cap=%d must be in 1..%d", d->name_cap,
                 DETR_OVERLAY_MAX_NAME);
    return 0;
}

extern "C" int64_t detr_hip_workspace_bytes_overlay(const detr_overlay_desc *d) {
    if (overlay_check_shape(d) != 0) return -1;
    return ov_layout(d->B, d->D, d->name_cap).total;
}

extern "C" int detr_hip_overlay(const detr_overlay_desc *d, void *stream) {
    if (overlay_check_shape(d) != 0) return -1;
    DETR_REQUIRE(d->src && d->src_off && d->dst && d->dst_off && d->sizes && d->sizes_host,
                 "overlay: null operand (src, src_off, dst, dst_off, sizes, sizes_host)");
    DETR_REQUIRE(d->boxes && d->labels && d->counts && d->colors && d->atlas && d->scale && d->workspace && d->status,
                 "overlay: null operand (boxes, labels, counts, colors, atlas, scale, workspace, status)");
    DETR_REQUIRE(d->thickness >= 1 && d->thickness <= DETR_OVERLAY_MAX_THICKNESS, "overlay: thickness=%d must be in 1..%d", d->thickness,
                 DETR_OVERLAY_MAX_THICKNESS);
    DETR_REQUIRE(d->label_alpha >= 0 && d->label_alpha <= 255, "overlay: label_alpha=%d must be in 0..255", d->label_alpha);
    DETR_REQUIRE(d->fill_alpha >= 0 && d->fill_alpha <= 255, "overlay: fill_alpha=%d must be in 0..255", d->fill_alpha);
    DETR_REQUIRE(d->heat_alpha >= 0 && d->heat_alpha <= 255, "overlay: heat_alpha=%d must be in 0..255", d->heat_alpha);
    DETR_REQUIRE(d->n_colors >= 1, "overlay: n_colors=%d must be >= 1", d->n_colors);
    DETR_REQUIRE(d->n_glyph >= 1 && d->gw >= 1 && d->gw <= DETR_OVERLAY_MAX_GLYPH && d->gh >= 1 && d->gh <= DETR_OVERLAY_MAX_GLYPH,
                 "overlay: bad font n_glyph=%d gh=%d gw=%d (n_glyph >= 1, gh and gw 1..%d)", d->n_glyph, d->gh, d->gw, DETR_OVERLAY_MAX_GLYPH);
    DETR_REQUIRE(d->glyph_digit0 >= 0 && d->glyph_digit0 <= 246 && d->glyph_colon >= 0 && d->glyph_colon <= 255 && d->glyph_dot >= 0 &&
                 d->glyph_dot <= 255, "overlay: glyph_digit0=%d (0..246), glyph_colon=%d, glyph_dot=%d (0..255) must fit a byte", d->glyph_digit0,
                 d->glyph_colon, d->glyph_dot);
    DETR_REQUIRE(d->n_names >= 0 && (d->n_names == 0 || (d->names && d->name_len)), "overlay: n_names=%d needs names and name_len", d->n_names);
    const bool any_heat = d->heat || d->map_step || d->map_valid || d->map_scale || d->lut;
    const bool all_heat = d->heat && d->map_step && d->map_valid && d->map_scale && d->lut;
    DETR_REQUIRE(!any_heat || all_heat, "overlay: heat, map_step, map_valid, map_scale and lut must be given together or not at all");
    if (all_heat)
        DETR_REQUIRE(d->Hf >= 1 && d->Wf >= 1 && d->sH_b >= 0 && d->sH_y >= 0 && d->sH_x >= 0, "overlay: bad heat map Hf=%d Wf=%d strides %lld %lld %lld",
                     d->Hf, d->Wf, (long long)d->sH_b, (long long)d->sH_y, (long long)d->sH_x);
    long long max_px = 0;
    for (int b = 0; b < d->B; ++b) {
        const int h = d->sizes_host[2 * b], w = d->sizes_host[2 * b + 1];
        DETR_REQUIRE(h >= 1 && h <= DETR_OVERLAY_MAX_SIDE && w >= 1 && w <= DETR_OVERLAY_MAX_SIDE, "overlay: image %d is %d x %d (each side 1..%d)", b, h,
                     w, DETR_OVERLAY_MAX_SIDE);
        max_px = std::max(max_px, (long long)h * w);
    }
    const OvLayout l = ov_layout(d->B, d->D, d->name_cap);
    DETR_REQUIRE(d->workspace_bytes >= l.total, "overlay: workspace of %lld bytes, %lld needed (detr_hip_workspace_bytes_overlay)",
                 (long long)d->workspace_bytes, l.total);
    DETR_REQUIRE(aligned16(d->workspace) && aligned16(d->boxes), "overlay: workspace and boxes must be 16-byte aligned");
    OvArgs a;
    a.src = d->src; a.src_off = reinterpret_cast<const long long *>(d->src_off);
    a.dst = d->dst; a.dst_off = reinterpret_cast<const long long *>(d->dst_off);
    a.sizes = d->sizes;
    a.boxes = d->boxes; a.labels = reinterpret_cast<const long long *>(d->labels); a.scores = d->scores; a.counts = d->counts;
    a.D = d->D; a.thickness = d->thickness; a.label_alpha = d->label_alpha; a.fill_alpha = d->fill_alpha;
    a.colors = d->colors; a.n_colors = d->n_colors;
    a.names = d->names; a.name_len = d->name_len; a.n_names = d->n_names; a.name_cap = d->name_cap;
    a.atlas = d->atlas; a.n_glyph = d->n_glyph; a.gh = d->gh; a.gw = d->gw;
    a.glyph_digit0 = d->glyph_digit0; a.glyph_colon = d->glyph_colon; a.glyph_dot = d->glyph_dot;
    a.scale = d->scale;
    a.heat = d->heat; a.sh_b = d->sH_b; a.sh_y = d->sH_y; a.sh_x = d->sH_x; a.Hf = d->Hf; a.Wf = d->Wf;
    a.map_step = d->map_step; a.map_valid = d->map_valid; a.map_scale = d->map_scale; a.lut = d->lut; a.heat_alpha = d->heat_alpha;
    unsigned char *ws = static_cast<unsigned char *>(d->workspace);
    a.ws_n = reinterpret_cast<int *>(ws + l.n_off);
    a.ws_cmd = reinterpret_cast<int *>(ws + l.cmd_off);
    a.ws_text = ws + l.text_off;
    a.text_cap = l.text_cap;
    a.status = d->status;
    hipLaunchKernelGGL(overlay_prep_kernel, dim3(d->B), dim3(OV_THREADS), 0, (hipStream_t)stream, a);
    DETR_LAUNCH_CHECK("overlay (preparation)");
    const unsigned tiles = (unsigned)((max_px + OV_TILE - 1) / OV_TILE);
    hipLaunchKernelGGL(overlay_raster_kernel, dim3(tiles, d->B), dim3(OV_THREADS), 0, (hipStream_t)stream, a);
    DETR_LAUNCH_CHECK("overlay (raster)");
    return 0;
}

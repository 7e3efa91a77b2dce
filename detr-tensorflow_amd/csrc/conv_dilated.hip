// conv_dilated.hip -- dilation-2 3x3 convolution (ZeroPadding2D(2) + Conv2D(3x3, dilation_rate=2), stride 1) forward / input gradient /
// weight gradient: the conv2 of blocks >= 1 of a stage built with replace_stride_with_dilation (DETR-DC5).
// Reference: detr_tf/networks/resnet_backbone.py:74-85,98,104-105 (see include/detr_hip.h: detr_conv3x3d_desc).
//
// A dilation-2, pad-2, stride-1 3x3 convolution never mixes pixels of different (row parity, column parity): it is four independent
// dense pad-1 convolutions, one per parity plane in_p(i, j) = in(2 i + py, 2 j + px), out(2 i + py, 2 j + px) = (in_p * w)(i, j) -- the
// zero padding agrees (out-of-range reads are zero on both sides), also for odd H / W where the planes have ceil / floor sizes.  The input
// gradient is the dense input gradient per plane, the weight gradient the sum of the planes' dense weight gradients.
//   * bf16 tensors, modes 0 / 1 (the hot path): ONE launch of the plane form of the halo-staged kernels (conv_halo.h, conv_halo_dma.h:
//     template parameter DIL).  The four planes ride on the grid like the parity classes of the stride-2 input gradient; a workgroup
//     stages its plane's (tile + 1 plane-pixel border) patch with a row pitch of 2 W C and a pixel pitch of 2 C elements -- at >= 64
//     channels a pixel's channel vector is whole 128-byte lines, so the doubled pitch fetches no extra bytes -- into the SAME LDS image as
//     the dense kernel, runs the same nine taps and writes its plane's pixels.  No gather copy, no im2col buffer.
//   * everything else (fp32 storage at compute 0 / 1 / 2; epilogues the halo kernels do not have) and mode 2: the implicit-GEMM tile
//     bodies of conv_f32.hip with their taps two pixels apart (template parameter DIL of the loaders); the weight gradient keeps the
//     deterministic row-split reduction through `workspace`.
// Every launch is bit-reproducible: no float atomics on a path with a workspace, fixed reduction orders.
#include "conv_halo.h"
#include "conv_halo_dma.h"

using namespace detr;

extern "C" int64_t detr_hip_workspace_bytes_conv3x3_dilated(const detr_conv3x3d_desc *d, int32_t mode) {
    if (!d || d->N <= 0 || d->Ci <= 0 || d->Co <= 0 || d->dilation != 2 || d->stride != 1 || d->pad != 2 || d->Ho != d->Hi || d->Wo != d->Wi) return -1;
    if (mode != 2) return 0;                       // forward / input gradient: no scratch
    const int split = conv_dilated_wgrad_splits(d->N, d->Ho, d->Wo, d->Ci, d->Co, d->compute, d->split);
    return split > 1 ? (int64_t)split * 9LL * d->Ci * d->Co * 4 : 0;
}

extern "C" int detr_hip_conv3x3_dilated(const detr_conv3x3d_desc *d, int32_t mode, void *stream) {
    DETR_REQUIRE(d != nullptr, "conv3x3 dilated: null descriptor");
    DETR_REQUIRE(mode >= 0 && mode <= 2, "conv3x3 dilated: bad mode %d", mode);
    DETR_REQUIRE(d->dilation == 2, "conv3x3 dilated: dilation %d unsupported (2 only; dilation 1 is detr_hip_conv3x3_f32)", d->dilation);
    DETR_REQUIRE(d->stride == 1, "conv3x3 dilated: stride %d unsupported (1 only)", d->stride);
    DETR_REQUIRE(d->pad == 2, "conv3x3 dilated: pad %d unsupported (pad = dilation = 2)", d->pad);
    DETR_REQUIRE(d->N > 0 && d->Hi > 0 && d->Wi > 0, "conv3x3 dilated: empty tensor N=%d %dx%d", d->N, d->Hi, d->Wi);
    DETR_REQUIRE(d->Ho == d->Hi && d->Wo == d->Wi, "conv3x3 dilated: output %dx%d must equal input %dx%d", d->Ho, d->Wo, d->Hi, d->Wi);
    DETR_REQUIRE(d->Ci > 0 && d->Co > 0 && d->Ci % 16 == 0 && d->Co % 16 == 0, "conv3x3 dilated: Ci=%d Co=%d must be multiples of 16", d->Ci, d->Co);
    DETR_REQUIRE(d->x && d->w && d->y, "conv3x3 dilated: null operand");
    DETR_REQUIRE(d->compute >= 0 && d->compute <= 2, "conv3x3 dilated: compute %d (0 = fp32, 1 = bf16, 2 = f32x3)", d->compute);
    DETR_REQUIRE((d->w_dtype == 0 || d->w_dtype == 1) && (d->x_dtype == 0 || d->x_dtype == 1) && (d->y_dtype == 0 || d->y_dtype == 1) &&
                 (d->r_dtype == 0 || d->r_dtype == 1) && d->m_dtype >= 0 && d->m_dtype <= 2,
                 "conv3x3 dilated: storage types w %d x %d y %d r %d (0 = fp32, 1 = bf16), m %d (2 = bit-packed as well)", d->w_dtype, d->x_dtype,
                 d->y_dtype, d->r_dtype, d->m_dtype);
    DETR_REQUIRE(aligned16(d->x) && aligned16(d->w) && aligned16(d->y), "conv3x3 dilated: operands must be 16-byte aligned");
    // 32-bit buffer offsets: a tensor past the limit is rejected, never wrapped (DC5's layer4 tensors are four times the plain model's)
    DETR_REQUIRE((long long)d->N * d->Hi * d->Wi * d->Ci * 4 <= BUF_MAX_BYTES && (long long)d->N * d->Ho * d->Wo * d->Co * 4 <= BUF_MAX_BYTES,
                 "conv3x3 dilated: a tensor spans more than 4 GB (32-bit buffer offsets)");
    hipStream_t s = (hipStream_t)stream;
    EpiArgs e;
    e.alpha = d->alpha;
    e.scale = d->scale;
    e.bias = d->bias;
    e.residual = d->residual;
    e.mask = d->mask;
    e.act = d->act;
    e.atomic = 0;
    e.drop_scale = 0.0f; e.drop_thresh = 0; e.drop_seed = 0;
    const bool bits_in = d->mask && d->m_dtype == 2, bits_out = mode == 0 && d->maskbits_out != nullptr;
    e.vec = (!d->scale || aligned16(d->scale)) && (!d->bias || aligned16(d->bias)) &&
            (!d->residual || aligned16(d->residual)) && (!d->mask || bits_in || aligned16(d->mask));
    e.c16 = (mode != 2 && d->y_dtype == 1); e.r16 = d->r_dtype == 1;
    e.m16 = (d->m_dtype == 1 || d->m_dtype == 2) ? d->m_dtype : 0;
    const bool bf = d->compute == 1 && d->Ci % 32 == 0 && d->Co % 32 == 0;
    if (mode == 2) {
        DETR_REQUIRE(!d->bias && !d->residual && !d->mask && d->act == 0, "conv3x3 dilated wgrad: only scale/alpha epilogue");
        ConvWgradArgs a;
        a.N = d->N; a.Hi = d->Hi; a.Wi = d->Wi; a.Ci = d->Ci; a.Ho = d->Ho; a.Wo = d->Wo; a.Co = d->Co;
        a.stride = 1; a.pad = 2; a.dil = 2;
        a.x = d->x; a.dy = d->w; a.dw = d->y;
        a.M = d->N * d->Ho * d->Wo;
        a.s16 = (d->x_dtype == 1);
        DETR_REQUIRE(d->x_dtype == d->w_dtype && d->y_dtype == 0, "conv3x3 dilated wgrad: x and dy must share their storage type, dw is fp32");
        DETR_REQUIRE(!a.s16 || bf, "conv3x3 dilated wgrad: bf16 tensors need compute = bf16 and channel counts %% 32 == 0");
        e.atomic = 1; e.ldr = 0; e.ldmask = 0;
        a.e = e;
        conv_dilated_wgrad_tiles(a, bf ? 1 : (d->compute == 2 ? 2 : 0), d->split, d->workspace, d->workspace_bytes, s);
        DETR_LAUNCH_CHECK("conv3x3 dilated wgrad");
        return 0;
    }
    ConvArgs a;
    a.N = d->N; a.stride = 1; a.pad = 2; a.dil = 2; a.Ci = d->Ci; a.Co = d->Co;
    a.w = d->w; a.src = d->x; a.dst = d->y;
    a.Hs = a.Hd = d->Hi; a.Ws = a.Wd = d->Wi;
    if (mode == 0) { a.Cs = d->Ci; a.Cd = d->Co; }
    else { a.Cs = d->Co; a.Cd = d->Ci; }
    a.M = d->N * a.Hd * a.Wd;
    a.tiles_m = a.tiles_n = 0;
    e.ldr = a.Cd;
    e.ldmask = bits_in ? a.Cd / 8 : a.Cd;
    e.mbits_out = bits_out ? d->maskbits_out : nullptr;
    e.ld_mbits_out = a.Cd / 8;
    e.wide16 = e.c16 && e.vec && (!d->residual || e.r16) && (!d->mask || e.m16) && (tune(T_EPI_WIDE) != 2 || bits_in || bits_out);
    DETR_REQUIRE(!(bits_in || bits_out) || (d->compute == 1 && e.wide16), "conv3x3 dilated: bit-packed masks need bf16 x / y / residual tensors (compute = bf16)");
    a.e = e;
    a.w16 = (d->w_dtype == 1);
    a.x16 = (d->x_dtype == 1);
    DETR_REQUIRE((d->x_dtype == 0 && d->y_dtype == 0 && d->r_dtype == 0 && d->m_dtype == 0) || bf,
                 "conv3x3 dilated: bf16 tensors need compute = bf16 and channel counts %% 32 == 0");
    DETR_REQUIRE(d->w_dtype == 0 || (d->w_dtype == 1 && bf), "conv3x3 dilated: a bf16 kernel tensor needs compute = bf16 and channel counts %% 32 == 0");
    a.par_on = 0; a.Hp = a.Wp = a.ph = a.pw = a.kh0 = a.kw0 = 0; a.nth = a.ntw = 3;
    a.cls_mix = 0;
    for (int k = 0; k < 4; ++k) a.cls_off[k] = a.cls_hp[k] = a.cls_wp[k] = 0;
    a.cls_off[4] = 0;
    const bool dgrad = mode == 1;
    // all-bf16 tensors: the plane form of the halo kernels, by the dense dispatch's rule (detr_hip_conv3x3_f32) -- 64-channel panels on
    // 8-row tiles, 128-channel panels on 4-row tiles filled by LDS-DMA (DETR_HIP_CONV_DMA = 2: register-staged; DETR_HIP_CONV_HALO = 2: tile kernel)
    if (d->compute == 1 && a.w16 && a.x16 && e.c16 && a.Cs % 32 == 0 && a.Cd % 64 == 0 && a.Cd <= 512 && (!d->mask || e.m16) &&
        !d->residual && !d->scale && d->alpha == 1.0f && (d->act == 0 || d->act == 1) && tune(T_CONV_HALO) != 2) {
        // (128-channel panels only where they are whole: the halo epilogue writes a panel's columns without a column bound)
        if (a.Cd % 128 == 0 && tune(T_CONV_DMA) != 2) { if (launch_conv_halo_dma_planes(a, dgrad, s)) return -1; }
        else if (a.Cd % 128 == 0) { if (launch_conv_halo_planes<128, 4>(a, dgrad, s)) return -1; }
        else if (launch_conv_halo_planes<64, 8>(a, dgrad, s)) return -1;
        DETR_LAUNCH_CHECK("conv3x3 dilated (halo planes)");
        return 0;
    }
    conv_dilated_tiles(a, dgrad, bf ? 1 : (d->compute == 2 ? 2 : 0), s);
    DETR_LAUNCH_CHECK("conv3x3 dilated");
    return 0;
}

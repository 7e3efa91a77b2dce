// conv_args.h -- argument structs of the 3x3 convolution kernels (conv_f32.hip, conv_x3.h, conv_halo.h, conv_halo_dma.h) and the
// dilation-2 launches conv_dilated.hip makes through conv_f32.hip
#pragma once
#include "gemm_core.h"

namespace detr {

// ------------------------------------------------------------------------------------------------
// forward / dgrad : rows = destination pixels, K = 9 taps x source channels
// ------------------------------------------------------------------------------------------------
struct ConvArgs {
    int N, Hs, Ws, Cs;  // source tensor (A operand): fwd x[N,Hi,Wi,Ci]; dgrad dy[N,Ho,Wo,Co]
    int Hd, Wd, Cd;     // destination tensor: fwd y[N,Ho,Wo,Co]; dgrad dx[N,Hi,Wi,Ci]
    int stride, pad;
    int Ci, Co;
    int M;
    const float *src;
    const float *w;
    float *dst;
    int tiles_m, tiles_n;
    EpiArgs e;
    // stride-2 dgrad, one launch per destination-pixel parity class (ph, pw): rows = (n, h2, w2) with h = 2*h2 + ph,
    // w = 2*w2 + pw; only the taps with kh = kh0 (+2), kw = kw0 (+2) contribute (1, 2, 2 or 4 of the 9), so the classes
    // together do 9/4 tap-GEMMs per pixel instead of 9 with 3/4 of the rows masked.
    int par_on, Hp, Wp, ph, pw, kh0, kw0, nth, ntw;
    int w16;                     // the kernel tensor is bf16 in memory (bf16 compute only)
    int x16;                     // the source tensor (x for fwd, dy for dgrad) is bf16 in memory
    // all four parity classes in ONE launch of the halo kernel's class form (conv_halo.h): class k = 0..3 is (ph, pw) =
    // (1,1), (0,1), (1,0), (0,0) -- heaviest first --, owns workgroups [cls_off[k], cls_off[k + 1]) and cls_hp / cls_wp tiles along H / W
    int cls_off[5], cls_hp[4], cls_wp[4];
    int cls_mix;                 // 1: the classes' workgroups round-robin in the grid instead of one class after the other (conv_halo.h)
    // dilation of the taps (1 | 2).  2 = the dilated entry point (conv_dilated.hip): the tile kernels step their taps by `dil` pixels, the halo
    // kernels walk the four pixel-parity PLANES of the tensors as four dense convolutions in one launch (the cls_* table carries the planes)
    int dil = 1;
};

// ------------------------------------------------------------------------------------------------
// wgrad : per tap, dw[tap][ci][co] += scale[co] * sum_m x[pix(m,tap)][ci] * dy[m][co]
// ------------------------------------------------------------------------------------------------
struct ConvWgradArgs {
    int N, Hi, Wi, Ci, Ho, Wo, Co, stride, pad;
    const float *x;
    const float *dy;
    float *dw;
    int M, rows_per_split;
    long long part_stride;   // 9*Ci*Co when the splits write partial slabs, 0 for the atomic fallback
    int tiles_m, tiles_n;
    EpiArgs e;
    int s16;                 // x and dy are bf16 in memory (bf16 activation storage; bf16 compute only)
    int dil = 1;             // dilation of the taps (1 | 2; 2: conv_dilated.hip)
    int slab_ts;             // partial slabs in tile order (gemm_core.h: store_slab_ts; tile = (tap * tiles_m + tm) * tiles_n + tn)
};

// dilation-2 launches of the tile bodies (defined in conv_f32.hip next to the kernels, called by conv_dilated.hip)
void conv_dilated_tiles(const ConvArgs &a, bool dgrad, int compute, hipStream_t s);
void conv_dilated_wgrad_tiles(const ConvWgradArgs &a, int compute, int split, float *ws, long long ws_bytes, hipStream_t s);
// row splits of that launch for an N x H x W map, from the same plan (the scratch-size query)
int conv_dilated_wgrad_splits(int N, int H, int W, int Ci, int Co, int compute, int split);

}  // namespace detr

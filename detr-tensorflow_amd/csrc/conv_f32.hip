// conv_f32.hip -- ResNet backbone convolution kernels (NHWC / HWIO, fp32) for gfx950:
//   3x3 implicit-GEMM convolution forward / dgrad / wgrad on the MFMA tile engine (no im2col buffer: the A-operand loader
//   gathers input pixels, zero-filling the halo; the f32x3 forms are conv_x3.h), the fused nine-tap bf16
//   weight gradient, and the dispatch of detr_hip_conv3x3_f32 (halo-staged kernels: conv_halo.h, conv_halo_dma.h).
//   The 7x7 stem convolution is stem_conv.hip, max pooling and the stride-2 subsample are pool.hip.
// Reference: detr_tf/networks/resnet_backbone.py:11-32,98-137 (see include/detr_hip.h).
#include "gemm_core.h"
#include "gemm_bf16_core.h"
#include "conv_args.h"
#include "conv_halo.h"
#include "conv_halo_dma.h"
namespace detr {

// DIL: pixel step of the taps (2: the dilated entry point, conv_dilated.hip)
template <int BM, bool DGRAD, int DIL = 1>
struct LoaderConvA {
    static constexpr int NV = BM / 64;
    BufSrc src;
    int n_[NV], h_[NV], w_[NV];
    bool ok[NV];
    int kq, tid;

    __device__ __forceinline__ void init(const ConvArgs &a, int m0, int tid_) {
        src.init(a.src, (long long)a.N * a.Hs * a.Ws * a.Cs);
        tid = tid_;
        kq = (tid & 3) * 4;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int m = m0 + (tid >> 2) + 64 * i;
            ok[i] = m < a.M;
            const int mm = ok[i] ? m : 0;
            int wd, hd;
            if (DGRAD && a.par_on) {
                const int t = mm / a.Wp;
                wd = 2 * (mm - t * a.Wp) + a.pw;
                hd = 2 * (t % a.Hp) + a.ph;
                n_[i] = t / a.Hp;
            } else {
                wd = mm % a.Wd;
                const int t = mm / a.Wd;
                hd = t % a.Hd;
                n_[i] = t / a.Hd;
            }
            h_[i] = DGRAD ? hd + a.pad : hd * a.stride - a.pad;
            w_[i] = DGRAD ? wd + a.pad : wd * a.stride - a.pad;
        }
    }
    // halo / stride-parity / tile-edge lanes take the out-of-range offset: the descriptor returns zeros, no branch
    // tap (kh, kw) and channel tile kc given by the caller (running counters in the main loop instead of divisions)
    __device__ __forceinline__ void load_tap(const ConvArgs &a, int kh, int kw, int kc, float4 (&r)[NV]) const {
        const int c0 = kc * GEMM_BK + kq;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            int hs, ws;
            bool v = ok[i];
            if (DGRAD) {
                const int th = h_[i] - kh * DIL, tw = w_[i] - kw * DIL;
                v = v && th >= 0 && tw >= 0;
                if (a.stride == 2) {
                    v = v && ((th & 1) == 0) && ((tw & 1) == 0);
                    hs = th >> 1;
                    ws = tw >> 1;
                } else {
                    hs = th;
                    ws = tw;
                }
                v = v && hs < a.Hs && ws < a.Ws;
            } else {
                hs = h_[i] + kh * DIL;
                ws = w_[i] + kw * DIL;
                v = v && hs >= 0 && ws >= 0 && hs < a.Hs && ws < a.Ws;
            }
            const unsigned off = ((unsigned)((n_[i] * a.Hs + hs) * a.Ws + ws) * (unsigned)a.Cs + (unsigned)c0) * 4u;
            r[i] = src.ld4(v ? off : BUF_OOB);
        }
    }
    template <int LD>
    __device__ __forceinline__ void store(float (*S)[LD], const float4 (&r)[NV]) const {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int row = (tid >> 2) + 64 * i;
            S[kq + 0][row] = r[i].x;
            S[kq + 1][row] = r[i].y;
            S[kq + 2][row] = r[i].z;
            S[kq + 3][row] = r[i].w;
        }
    }
};

// SPLIT3: the K tiles run on the bf16 matrix pipe at fp32 accuracy (gemm_core.h: mma_ktile_split3; detr_conv3x3_desc.compute = 2)
template <int BM, int BN, int WGM, int WGN, bool DGRAD, bool SPLIT3 = false, int DIL = 1>
__global__ __launch_bounds__(GEMM_THREADS) void conv3x3_kernel(ConvArgs a) {
    using T = TileCfg<BM, BN, WGM, WGN>;
    __shared__ __attribute__((aligned(16))) char smem_raw[SmemBytes<BM, BN, WGN>::VALUE];
    GemmSmem<BM, BN> &sm = *reinterpret_cast<GemmSmem<BM, BN> *>(smem_raw);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WGN, wn = wave % WGN;
    const int id = xcd_remap(blockIdx.x, gridDim.x);
    const int tn = id % a.tiles_n, tm = id / a.tiles_n;
    const int m0 = tm * BM, n0 = tn * BN;

    const int cpt = a.Cs / GEMM_BK;  // K tiles per tap
    const int nkt = (a.par_on ? a.nth * a.ntw : 9) * cpt;
    const long long tapstride = (long long)a.Ci * a.Co;

    LoaderConvA<BM, DGRAD, DIL> la;
    la.init(a, m0, tid);
    // B operand per tap: fwd  B[k=ci][n=co] = w[tap][ci][co]  (n contiguous, ld = Co, K = Ci)
    //                    dgrad B[k=co][n=ci] = w[tap][ci][co]  (k contiguous, ld = Co, K = Co)
    using LB = typename std::conditional<DGRAD, LoaderK<BN>, LoaderMN<BN>>::type;
    LB lb;
    lb.init(a.w, a.Co, n0, a.Cd, a.Cs, true, tid, 9 * tapstride);   // one descriptor over the 9 taps

    f32x16 acc[T::TM][T::TN];
#pragma unroll
    for (int i = 0; i < T::TM; ++i)
#pragma unroll
        for (int j = 0; j < T::TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    float4 ra[LoaderConvA<BM, DGRAD, DIL>::NV], rb[LB::NV];
    // K tiles are requested strictly in order: tap and channel tile are running counters (a kt / cpt division and a tap
    // decode cost ~40 scalar instructions per 16-deep K tile)
    const int tap_cols = a.par_on ? a.ntw : 3;
    int it_kc = 0, it_ti = 0, it_tj = 0;
    auto load_ab = [&]() {
        const int kh = a.par_on ? a.kh0 + 2 * it_ti : it_ti;
        const int kw = a.par_on ? a.kw0 + 2 * it_tj : it_tj;
        la.load_tap(a, kh, kw, it_kc, ra);
        lb.load(it_kc * GEMM_BK, a.Cs, rb, (unsigned)((kh * 3 + kw) * tapstride * 4));
        if (++it_kc == cpt) {
            it_kc = 0;
            if (++it_tj == tap_cols) {
                it_tj = 0;
                ++it_ti;
            }
        }
    };
    load_ab();
    la.store(sm.A[0], ra);
    lb.store(sm.B[0], rb);
    __syncthreads();
    int cur = 0;
    for (int kt = 0; kt < nkt; ++kt) {
        const bool more = (kt + 1) < nkt;
        if (more) load_ab();
        mma_ktile_sel<BM, BN, WGM, WGN, SPLIT3>(sm.A[cur], sm.B[cur], acc, wm, wn, lane);
        if (more) {
            la.store(sm.A[cur ^ 1], ra);
            lb.store(sm.B[cur ^ 1], rb);
        }
        __syncthreads();
        cur ^= 1;
    }
    epilogue<BM, BN, WGM, WGN>(acc, reinterpret_cast<float *>(smem_raw), a.dst, a.Cd, a.M, a.Cd, m0, n0, wm, wn, lane, wave, a.e);
}

// ------------------------------------------------------------------------------------------------
// wgrad : per tap, dw[tap][ci][co] += scale[co] * sum_m x[pix(m,tap)][ci] * dy[m][co]
// grid = (ci tiles * co tiles, 9 taps, row splits); reduction rows are the output pixels.
// ------------------------------------------------------------------------------------------------

}  // namespace detr
#include "conv_x3.h"
namespace detr {

template <int BM, int DIL = 1>
struct LoaderWgradA {
    static constexpr int VPR = BM / 4;
    static constexpr int TOTAL = GEMM_BK * VPR;
    static constexpr int NV = (TOTAL >= GEMM_THREADS) ? TOTAL / GEMM_THREADS : 1;
    BufSrc src;
    int n_[NV], h_[NV], w_[NV];  // output-pixel coordinates of this entry's current reduction row
    int m_[NV];
    int tid, ci0, kh, kw;

    __device__ __forceinline__ void init(const ConvWgradArgs &a, int ci0_, int tap, int m_begin, int tid_) {
        src.init(a.x, (long long)a.N * a.Hi * a.Wi * a.Ci);
        tid = tid_;
        ci0 = ci0_;
        kh = tap / 3;
        kw = tap - kh * 3;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int idx = tid + GEMM_THREADS * i;
            const int kr = idx / VPR;
            const int m = m_begin + kr;
            m_[i] = m;
            const int wo = m % a.Wo;
            const int t = m / a.Wo;
            w_[i] = wo;
            h_[i] = t % a.Ho;
            n_[i] = t / a.Ho;
        }
    }
    __device__ __forceinline__ void load(const ConvWgradArgs &a, int m_end, float4 (&r)[NV]) const {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int idx = tid + GEMM_THREADS * i;
            const int c4 = (idx % VPR) * 4;
            const int hs = h_[i] * a.stride - a.pad + kh * DIL;
            const int ws = w_[i] * a.stride - a.pad + kw * DIL;
            const bool v = (idx < TOTAL) && (m_[i] < m_end) && hs >= 0 && ws >= 0 && hs < a.Hi && ws < a.Wi &&
                           (ci0 + c4 < a.Ci);
            const unsigned off = ((unsigned)((n_[i] * a.Hi + hs) * a.Wi + ws) * (unsigned)a.Ci + (unsigned)(ci0 + c4)) * 4u;
            r[i] = src.ld4(v ? off : BUF_OOB);
        }
    }
    __device__ __forceinline__ void advance(const ConvWgradArgs &a) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            m_[i] += GEMM_BK;
            w_[i] += GEMM_BK;
            while (w_[i] >= a.Wo) {
                w_[i] -= a.Wo;
                h_[i] += 1;
            }
            while (h_[i] >= a.Ho) {
                h_[i] -= a.Ho;
                n_[i] += 1;
            }
        }
    }
    template <int LD>
    __device__ __forceinline__ void store(float (*S)[LD], const float4 (&r)[NV]) const {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int idx = tid + GEMM_THREADS * i;
            if (idx < TOTAL) {
                const int kr = idx / VPR;
                const int c4 = (idx % VPR) * 4;
                *reinterpret_cast<float4 *>(&S[kr][c4]) = r[i];
            }
        }
    }
};

template <int BM, int BN, int WGM, int WGN, bool SPLIT3 = false, int DIL = 1>
__global__ __launch_bounds__(GEMM_THREADS) void conv3x3_wgrad_kernel(ConvWgradArgs a) {
    using T = TileCfg<BM, BN, WGM, WGN>;
    __shared__ __attribute__((aligned(16))) char smem_raw[SmemBytes<BM, BN, WGN>::VALUE];
    GemmSmem<BM, BN> &sm = *reinterpret_cast<GemmSmem<BM, BN> *>(smem_raw);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WGN, wn = wave % WGN;
    const int tn = blockIdx.x % a.tiles_n, tm = blockIdx.x / a.tiles_n;
    const int ci0 = tm * BM, co0 = tn * BN;
    const int tap = blockIdx.y;
    const int m_begin = blockIdx.z * a.rows_per_split;
    const int m_end = min(a.M, m_begin + a.rows_per_split);
    if (m_begin >= m_end) return;
    const int nkt = (m_end - m_begin + GEMM_BK - 1) / GEMM_BK;

    LoaderWgradA<BM, DIL> la;
    la.init(a, ci0, tap, m_begin, tid);
    LoaderMN<BN> lb;
    lb.init(a.dy, a.Co, co0, a.Co, a.M, true, tid);

    f32x16 acc[T::TM][T::TN];
#pragma unroll
    for (int i = 0; i < T::TM; ++i)
#pragma unroll
        for (int j = 0; j < T::TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    float4 ra[LoaderWgradA<BM, DIL>::NV], rb[LoaderMN<BN>::NV];
    la.load(a, m_end, ra);
    lb.load(m_begin, m_end, rb);
    la.store(sm.A[0], ra);
    lb.store(sm.B[0], rb);
    __syncthreads();
    int cur = 0;
    for (int kt = 0; kt < nkt; ++kt) {
        const bool more = (kt + 1) < nkt;
        if (more) {
            la.advance(a);
            la.load(a, m_end, ra);
            lb.load(m_begin + (kt + 1) * GEMM_BK, m_end, rb);
        }
        mma_ktile_sel<BM, BN, WGM, WGN, SPLIT3>(sm.A[cur], sm.B[cur], acc, wm, wn, lane);
        if (more) {
            la.store(sm.A[cur ^ 1], ra);
            lb.store(sm.B[cur ^ 1], rb);
        }
        __syncthreads();
        cur ^= 1;
    }
    if constexpr (WGM == 2 && WGN == 2) {
        if (a.slab_ts) {
            float *slab = a.dw + (long long)blockIdx.z * a.part_stride + ((long long)(tap * a.tiles_m + tm) * a.tiles_n + tn) * (BM * BN);
            store_slab_ts<BM, BN, WGM, WGN>(acc, slab, wave, lane);
            return;
        }
    }
    float *dw = a.dw + (long long)tap * a.Ci * a.Co + (long long)blockIdx.z * a.part_stride;
    epilogue<BM, BN, WGM, WGN, false>(acc, reinterpret_cast<float *>(smem_raw), dw, a.Co, a.Ci, a.Co, ci0, co0, wm, wn, lane, wave, a.e);
}

// ------------------------------------------------------------------------------------------------
// bf16-compute variants (fp32 storage, bf16 MFMA; see gemm_bf16_core.h).  Channel counts must be % 32.
// ------------------------------------------------------------------------------------------------
// X16: the source tensor is bf16 in memory (bf16 activation storage): 16-byte chunks of 8 channels, no conversion
template <int BM, bool DGRAD, bool X16, int DIL = 1>
struct LoaderConvAb {
    static constexpr int NV = X16 ? BM / 64 : BM / 32;
    typedef typename std::conditional<X16, uint4, float4>::type Reg;
    BufSrc src;
    int n_[NV], h_[NV], w_[NV];
    bool ok[NV];
    int kq, tid;

    __device__ __forceinline__ void init(const ConvArgs &a, int m0, int tid_) {
        src.init_bytes(a.src, (long long)a.N * a.Hs * a.Ws * a.Cs * (X16 ? 2 : 4));
        tid = tid_;
        kq = X16 ? (tid & 3) * 8 : (tid & 7) * 4;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int m = m0 + (X16 ? (tid >> 2) + 64 * i : (tid >> 3) + 32 * i);
            ok[i] = m < a.M;
            const int mm = ok[i] ? m : 0;
            int wd, hd;
            if (DGRAD && a.par_on) {
                const int t = mm / a.Wp;
                wd = 2 * (mm - t * a.Wp) + a.pw;
                hd = 2 * (t % a.Hp) + a.ph;
                n_[i] = t / a.Hp;
            } else {
                wd = mm % a.Wd;
                const int t = mm / a.Wd;
                hd = t % a.Hd;
                n_[i] = t / a.Hd;
            }
            h_[i] = DGRAD ? hd + a.pad : hd * a.stride - a.pad;
            w_[i] = DGRAD ? wd + a.pad : wd * a.stride - a.pad;
        }
    }
    // halo / stride-parity / tile-edge lanes take the out-of-range offset: the descriptor returns zeros, no branch
    // live = false: a request past the last K tile (operand pipeline tail) -- every lane takes the out-of-range offset
    // the tap (kh, kw) and the channel tile kc inside the tap are given by the caller (the main loop keeps them as running
    // counters: dividing kt by the tiles per tap is ~40 scalar instructions per K tile, more than the tile's MFMAs)
    __device__ __forceinline__ void load_tap(const ConvArgs &a, int kh, int kw, int kc, Reg (&r)[NV], bool live = true) const {
        const int c0 = kc * BF_BK + kq;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            int hs, ws;
            bool v = ok[i] && live;
            if (DGRAD) {
                const int th = h_[i] - kh * DIL, tw = w_[i] - kw * DIL;
                v = v && th >= 0 && tw >= 0;
                if (a.stride == 2) {
                    v = v && ((th & 1) == 0) && ((tw & 1) == 0);
                    hs = th >> 1;
                    ws = tw >> 1;
                } else {
                    hs = th;
                    ws = tw;
                }
                v = v && hs < a.Hs && ws < a.Ws;
            } else {
                hs = h_[i] + kh * DIL;
                ws = w_[i] + kw * DIL;
                v = v && hs >= 0 && ws >= 0 && hs < a.Hs && ws < a.Ws;
            }
            const unsigned off = ((unsigned)((n_[i] * a.Hs + hs) * a.Ws + ws) * (unsigned)a.Cs + (unsigned)c0) * (X16 ? 2u : 4u);
            if constexpr (X16) r[i] = src.ld16(v ? off : BUF_OOB);
            else r[i] = src.ld4(v ? off : BUF_OOB);
        }
    }
    __device__ __forceinline__ void store(unsigned short (*S)[BF_LD], const Reg (&r)[NV]) const {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            if constexpr (X16) {
                *reinterpret_cast<uint4 *>(&S[(tid >> 2) + 64 * i][kq]) = r[i];
            } else {
                const int row = (tid >> 3) + 32 * i;
                *reinterpret_cast<uint2 *>(&S[row][kq]) = make_uint2(pack_bf16(r[i].x, r[i].y), pack_bf16(r[i].z, r[i].w));
            }
        }
    }
};

template <int BM, int BN, int WGM, int WGN, bool DGRAD, bool W16, bool X16, int DIL = 1>
__global__ __launch_bounds__(GEMM_THREADS, (BM * BN >= 128 * 128) ? 3 : (BM * BN == 64 * 64 ? MIN_WAVES_64X64 : 1)) void conv3x3_bf16c_kernel(ConvArgs a) {
    using T = TileCfg<BM, BN, WGM, WGN>;
    __shared__ __attribute__((aligned(16))) char smem_raw[BfSmemBytes<BM, BN, WGN>::VALUE];
    BfSmem<BM, BN> &sm = *reinterpret_cast<BfSmem<BM, BN> *>(smem_raw);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WGN, wn = wave % WGN;
    const int id = xcd_remap(blockIdx.x, gridDim.x);
    const int tn = id % a.tiles_n, tm = id / a.tiles_n;
    const int m0 = tm * BM, n0 = tn * BN;
    const int cpt = a.Cs / BF_BK;
    const int nkt = (a.par_on ? a.nth * a.ntw : 9) * cpt;
    const long long tapstride = (long long)a.Ci * a.Co;
    LoaderConvAb<BM, DGRAD, X16, DIL> la;
    la.init(a, m0, tid);
    // fwd weights: transpose-read image; W16: the kernel is already bf16 in memory (per-step weight shadow)
    using LB = typename std::conditional<W16, typename std::conditional<DGRAD, LoaderKh<BN>, LoaderMNth<BN, true>>::type,
                                         typename std::conditional<DGRAD, LoaderKb<BN>, LoaderMNt<BN>>::type>::type;
    constexpr int NRB = LB::NREG;
    LB lb;
    lb.init(a.w, a.Co, n0, a.Cd, a.Cs, true, tid, 9 * tapstride);   // one descriptor over the 9 taps
    f32x16 acc[T::TM][T::TN];
#pragma unroll
    for (int i = 0; i < T::TM; ++i)
#pragma unroll
        for (int j = 0; j < T::TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
    // Operand pipeline two K tiles deep with LDS-only barriers -- see gemm_bf16c_body (gemm_f32.hip): requests and LDS
    // stores are unconditional (past the last tile they resolve to the out-of-range offset / write a buffer nobody reads)
    // so that the compiler's vmcnt waits stay exact.
    using LAc = LoaderConvAb<BM, DGRAD, X16, DIL>;
    typename LAc::Reg ra0[LAc::NV], ra1[LAc::NV];
    typename LB::Reg rb0[NRB], rb1[NRB];
    // K tiles are requested strictly in order (0, 1, 2, then kt + 3 per iteration): the tap and the channel tile inside it
    // are running counters instead of divisions of kt
    const int tap_cols = a.par_on ? a.ntw : 3;
    int it_kc = 0, it_ti = 0, it_tj = 0;
    auto load_ab = [&](int kt, typename LAc::Reg (&ra)[LAc::NV], typename LB::Reg (&rb)[NRB]) {
        const bool live = kt < nkt;
        const int kh = a.par_on ? a.kh0 + 2 * it_ti : it_ti;
        const int kw = a.par_on ? a.kw0 + 2 * it_tj : it_tj;
        la.load_tap(a, kh, kw, it_kc, ra, live);
        lb.load(it_kc * BF_BK, live ? a.Cs : 0, rb, live ? (unsigned)((kh * 3 + kw) * tapstride * (W16 ? 2 : 4)) : 0u);
        if (++it_kc == cpt) {
            it_kc = 0;
            if (++it_tj == tap_cols) {
                it_tj = 0;
                ++it_ti;
            }
        }
    };
    load_ab(0, ra0, rb0);
    la.store(sm.A[0], ra0);
    lb.store(sm.B[0], rb0);
    load_ab(1, ra0, rb0);
    load_ab(2, ra1, rb1);
    lds_barrier();
    auto iter = [&](const int kt, const int cur, typename LAc::Reg (&rpa)[LAc::NV], typename LB::Reg (&rpb)[NRB]) {
        la.store(sm.A[cur ^ 1], rpa);
        lb.store(sm.B[cur ^ 1], rpb);
        load_ab(kt + 3, rpa, rpb);
        mma_ktile_bf16<BM, BN, WGM, WGN, false, !DGRAD>(sm.A[cur], sm.B[cur], acc, wm, wn, lane);
        lds_barrier();
    };
    {
        int kt = 0;
        for (; kt + 2 <= nkt; kt += 2) {
            iter(kt, 0, ra0, rb0);
            iter(kt + 1, 1, ra1, rb1);
        }
        if (kt < nkt) iter(kt, 0, ra0, rb0);
    }
    __syncthreads();
    epilogue<BM, BN, WGM, WGN>(acc, reinterpret_cast<float *>(smem_raw), a.dst, a.Cd, a.M, a.Cd, m0, n0, wm, wn, lane, wave, a.e);
}

// wgrad: A'[i = ci][k = m] gathered into a transpose-read image (gemm_bf16_core.h LoaderMNt): unit u = t + 256*i holds
// the float4 of channels ci0 + 16*ib + 4*c of reduction row (output pixel) k = 4*kb + kr of the tile.
template <int BM, bool S16, int DIL = 1>
struct LoaderWgradAt {
    static constexpr int NB = BM / 16;
    static constexpr int NU = BM / 32;
    typedef typename std::conditional<S16, uint2, float4>::type Reg;
    BufSrc src;
    int n_[NU], h_[NU], w_[NU], m_[NU];
    int tid, ci0, kh, kw;

    __device__ __forceinline__ void init(const ConvWgradArgs &a, int ci0_, int tap, int m_begin, int tid_) {
        src.init_bytes(a.x, (long long)a.N * a.Hi * a.Wi * a.Ci * (S16 ? 2 : 4));
        tid = tid_; ci0 = ci0_;
        kh = tap / 3; kw = tap - kh * 3;
#pragma unroll
        for (int i = 0; i < NU; ++i) {
            const int u = tid + 256 * i;
            const int m = m_begin + 4 * (u / (16 * NB)) + ((u >> 2) & 3);
            m_[i] = m;
            w_[i] = m % a.Wo;
            const int t = m / a.Wo;
            h_[i] = t % a.Ho;
            n_[i] = t / a.Ho;
        }
    }
    __device__ __forceinline__ void load(const ConvWgradArgs &a, int m_end, Reg (&r)[NU]) const {
#pragma unroll
        for (int i = 0; i < NU; ++i) {
            const int u = tid + 256 * i;
            const int c = ci0 + 16 * ((u >> 4) & (NB - 1)) + 4 * (u & 3);
            const int hs = h_[i] * a.stride - a.pad + kh * DIL, ws = w_[i] * a.stride - a.pad + kw * DIL;
            const bool v = m_[i] < m_end && hs >= 0 && ws >= 0 && hs < a.Hi && ws < a.Wi && c < a.Ci;
            const unsigned off = ((unsigned)((n_[i] * a.Hi + hs) * a.Wi + ws) * (unsigned)a.Ci + (unsigned)c) * (S16 ? 2u : 4u);
            if constexpr (S16) r[i] = src.ld8(v ? off : BUF_OOB);
            else r[i] = src.ld4(v ? off : BUF_OOB);
        }
    }
    __device__ __forceinline__ void advance(const ConvWgradArgs &a) {
#pragma unroll
        for (int i = 0; i < NU; ++i) {
            m_[i] += BF_BK;
            w_[i] += BF_BK;
            while (w_[i] >= a.Wo) { w_[i] -= a.Wo; h_[i] += 1; }
            while (h_[i] >= a.Ho) { h_[i] -= a.Ho; n_[i] += 1; }
        }
    }
    __device__ __forceinline__ void store(unsigned short (*S)[BF_LD], const Reg (&r)[NU]) const {
        unsigned short *flat = &S[0][0];
#pragma unroll
        for (int i = 0; i < NU; ++i) {
            if constexpr (S16) *reinterpret_cast<uint2 *>(flat + (tid + 256 * i) * 4) = r[i];
            else *reinterpret_cast<uint2 *>(flat + (tid + 256 * i) * 4) = make_uint2(pack_bf16(r[i].x, r[i].y), pack_bf16(r[i].z, r[i].w));
        }
    }
};

template <int BM, int BN, int WGM, int WGN, bool S16, int DIL = 1>
__global__ __launch_bounds__(GEMM_THREADS, (BM * BN >= 128 * 128) ? 3 : 1) void conv3x3_wgrad_bf16c_kernel(ConvWgradArgs a) {
    using T = TileCfg<BM, BN, WGM, WGN>;
    __shared__ __attribute__((aligned(16))) char smem_raw[BfSmemBytes<BM, BN, WGN>::VALUE];
    BfSmem<BM, BN> &sm = *reinterpret_cast<BfSmem<BM, BN> *>(smem_raw);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WGN, wn = wave % WGN;
    const int tn = blockIdx.x % a.tiles_n, tm = blockIdx.x / a.tiles_n;
    const int ci0 = tm * BM, co0 = tn * BN;
    const int tap = blockIdx.y;
    const int m_begin = blockIdx.z * a.rows_per_split;
    const int m_end = min(a.M, m_begin + a.rows_per_split);
    if (m_begin >= m_end) return;
    const int nkt = (m_end - m_begin + BF_BK - 1) / BF_BK;
    LoaderWgradAt<BM, S16, DIL> la;
    la.init(a, ci0, tap, m_begin, tid);
    typename std::conditional<S16, LoaderMNth<BN>, LoaderMNt<BN>>::type lb;      // dy: same storage type as x
    lb.init(a.dy, a.Co, co0, a.Co, a.M, true, tid);
    f32x16 acc[T::TM][T::TN];
#pragma unroll
    for (int i = 0; i < T::TM; ++i)
#pragma unroll
        for (int j = 0; j < T::TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
    typename LoaderWgradAt<BM, S16, DIL>::Reg ra[LoaderWgradAt<BM, S16, DIL>::NU];
    typename std::conditional<S16, uint2, float4>::type rb[LoaderMNt<BN>::NU];
    la.load(a, m_end, ra);
    lb.load(m_begin, m_end, rb);
    la.store(sm.A[0], ra);
    lb.store(sm.B[0], rb);
    __syncthreads();
    int cur = 0;
    for (int kt = 0; kt < nkt; ++kt) {
        const bool more = (kt + 1) < nkt;
        if (more) {
            la.advance(a);
            la.load(a, m_end, ra);
            lb.load(m_begin + (kt + 1) * BF_BK, m_end, rb);
        }
        mma_ktile_bf16<BM, BN, WGM, WGN, true, true>(sm.A[cur], sm.B[cur], acc, wm, wn, lane);
        if (more) {
            la.store(sm.A[cur ^ 1], ra);
            lb.store(sm.B[cur ^ 1], rb);
        }
        __syncthreads();
        cur ^= 1;
    }
    if constexpr (WGM == 2 && WGN == 2) {
        if (a.slab_ts) {
            float *slab = a.dw + (long long)blockIdx.z * a.part_stride + ((long long)(tap * a.tiles_m + tm) * a.tiles_n + tn) * (BM * BN);
            store_slab_ts<BM, BN, WGM, WGN>(acc, slab, wave, lane);
            return;
        }
    }
    float *dw = a.dw + (long long)tap * a.Ci * a.Co + (long long)blockIdx.z * a.part_stride;
    epilogue<BM, BN, WGM, WGN, false>(acc, reinterpret_cast<float *>(smem_raw), dw, a.Co, a.Ci, a.Co, ci0, co0, wm, wn, lane, wave, a.e);
}

// ------------------------------------------------------------------------------------------------
// bf16 weight gradient with the NINE TAPS FUSED (stride 1, pad 1, Ci % 64 == 0, Co % 64 == 0):
//   dw[tap][ci][co] += sum over output pixels of x[pix + tap][ci] * dy[pix][co]
// One workgroup owns a 64(ci) x 64(co) tile of all nine taps (9 accumulators of 16 registers per wave).  The reduction
// runs over UNITS of 32 consecutive output pixels of one output row: per unit the workgroup stages the dy tile
// [32 px][64 co] and the haloed input patch [3 rows][34 px][64 ci] ONCE (bf16, natural [pixel][channel] orientation
// cut into [4 px][16 ch] sub-blocks of 128 B) and every tap reads its MFMA fragments with ds_read_b64_tr_b16 at a
// shifted pixel row -- the per-tap kernel above re-loads x and dy for every tap (4.2x the LDS fill per MFMA).
// ------------------------------------------------------------------------------------------------
// STR = 2 (round 5; bf16 storage only): the stride-2 convolutions of layer2-4 (resnet_backbone.py:123-126 with strides 2) took the per-tap kernel
// until now (100 us per launch against 63 for the same FLOPs at stride 1).  A unit of 32 output pixels reads input columns 2 j + kw - 1: the
// patch is 3 rows x 65 pixels, staged DE-INTERLEAVED -- even patch columns in slots 0..32, odd ones in slots 33..65 -- so that the tap kw of
// output pixel j sits at slot (kw & 1) * 33 + j + (kw >> 1): consecutive slots for consecutive j, the same transpose-read fragments as at stride 1.
template <int STR>
struct WgradFusedGeom {
    static constexpr int PC = STR == 1 ? 34 : 66;                 // pixel slots of a patch row (stride 2: 33 even + 33 odd columns, the last odd one unused)
    static constexpr int NG = (PC + 3) / 4;                       // pixel groups of 4
    static constexpr int ROW = NG * 4 * 64;                       // shorts per patch row: pixel groups x 4 ci blocks x [4][16]
    __device__ static constexpr int slot(int c) { return STR == 1 ? c : (c & 1) * 33 + (c >> 1); }
};
constexpr int WF_ROW = WgradFusedGeom<1>::ROW;

template <int STR>
struct WgradFusedSmem {
    unsigned short X[2][3 * WgradFusedGeom<STR>::ROW];      // haloed input patch
    unsigned short D[2][32 * 64];         // dy tile (transpose-read image, BMN = 64)
};

template <bool S16, int STR = 1>
__global__ __launch_bounds__(GEMM_THREADS, 2) void conv3x3_wgrad_fused_bf16_kernel(ConvWgradArgs a, int units_per_split,
                                                                                 int chunks) {
    static_assert(STR == 1 || S16, "the stride-2 form exists for bf16-stored tensors");
    using WG = WgradFusedGeom<STR>;
    constexpr int WF_ROW = WG::ROW, PC = WG::PC, NPP = 3 * PC;
    constexpr int SMEM = (int)sizeof(WgradFusedSmem<STR>) > SmemBytes<64, 64, 2>::VALUE ? (int)sizeof(WgradFusedSmem<STR>)
                                                                                         : SmemBytes<64, 64, 2>::VALUE;
    __shared__ __attribute__((aligned(16))) char smem_raw[SMEM];
    WgradFusedSmem<STR> &sm = *reinterpret_cast<WgradFusedSmem<STR> *>(smem_raw);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int tn = blockIdx.x % a.tiles_n, tm = blockIdx.x / a.tiles_n;
    const int ci0 = tm * 64, co0 = tn * 64;
    const int total_units = a.N * a.Ho * chunks;
    const int u_begin = blockIdx.z * units_per_split;
    const int u_end = min(total_units, u_begin + units_per_split);
    if (u_begin >= u_end) return;
    BufSrc xs, ds;
    xs.init_bytes(a.x, (long long)a.N * a.Hi * a.Wi * a.Ci * (S16 ? 2 : 4));
    ds.init_bytes(a.dy, (long long)a.N * a.Ho * a.Wo * a.Co * (S16 ? 2 : 4));

    f32x16 acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;

    // S16: 16-byte granules (8 channels of one pixel; two adjacent 8-byte units of the transpose-read images) -- 5 requests
    // and 5 ds_write_b128 per thread and unit instead of 9 + 9 eight-byte ones; fp32 storage: float4 = 4 channels
    typedef typename std::conditional<S16, uint4, float4>::type Reg;
    constexpr int NRX = (NPP * (S16 ? 8 : 16) + 255) / 256, NRD = S16 ? 1 : 2;      // stride 1: 4 (bf16) / 7 (fp32); stride 2: 7
    // two register sets: the operand pipeline is two units deep (see gemm_bf16c_body); requests past u_end take the
    // out-of-range offset and every unit is stored, so that the vmcnt waits in front of the LDS stores stay exact
    Reg rx0[NRX], rd0[NRD], rx1[NRX], rd1[NRD];
    // units are requested strictly in order (u_begin, +1, +2, ...): (chunk, output row, image) are running counters
    // instead of three divisions per unit
    int it_chunk = u_begin % chunks, it_ho = (u_begin / chunks) % a.Ho, it_n = (u_begin / chunks) / a.Ho;
    auto load_unit = [&](int u, Reg (&rx)[NRX], Reg (&rd)[NRD]) {
        const bool live = u < u_end;
        const int ho = it_ho, n = it_n;
        const int wo0 = it_chunk * 32;
        if (++it_chunk == chunks) {
            it_chunk = 0;
            if (++it_ho == a.Ho) {
                it_ho = 0;
                ++it_n;
            }
        }
        // dy tile: LoaderMNt<64> map (row = pixel j, col = co); S16: unit pairs (2 v, 2 v + 1) = 8 channels
#pragma unroll
        for (int i = 0; i < NRD; ++i) {
            const int v = S16 ? 2 * tid : tid + 256 * i;
            const int j = 4 * (v >> 6) + ((v >> 2) & 3);
            const int col = 16 * ((v >> 4) & 3) + 4 * (v & 3);
            const bool ok = live && wo0 + j < a.Wo;
            const unsigned off = ((unsigned)((n * a.Ho + ho) * a.Wo + wo0 + j) * (unsigned)a.Co + (unsigned)(co0 + col)) * (S16 ? 2u : 4u);
            if constexpr (S16) rd[i] = ds.ld16(ok ? off : BUF_OOB);
            else rd[i] = ds.ld4(ok ? off : BUF_OOB);
        }
        // input patch: slot v -> (patch pixel pp in [0, 3 PC), channel granule): S16 8 granules of 8 channels, fp32 16 of 4
#pragma unroll
        for (int i = 0; i < NRX; ++i) {
            const int v = tid + 256 * i;
            const int pp = S16 ? v >> 3 : v >> 4, c4 = S16 ? 2 * (v & 7) : v & 15;
            const int kh = pp / PC, c = pp - kh * PC;
            const int hi = STR * ho - 1 + kh, wi = STR * wo0 - 1 + c;
            const bool ok = live && pp < NPP && hi >= 0 && hi < a.Hi && wi >= 0 && wi < a.Wi;
            const unsigned off = ((unsigned)((n * a.Hi + hi) * a.Wi + wi) * (unsigned)a.Ci + (unsigned)(ci0 + 4 * c4)) * (S16 ? 2u : 4u);
            if constexpr (S16) rx[i] = xs.ld16(ok ? off : BUF_OOB);
            else rx[i] = xs.ld4(ok ? off : BUF_OOB);
        }
    };
    auto store_unit = [&](int buf, const Reg (&rx)[NRX], const Reg (&rd)[NRD]) {
#pragma unroll
        for (int i = 0; i < NRD; ++i) {
            if constexpr (S16) *reinterpret_cast<uint4 *>(&sm.D[buf][tid * 8]) = rd[i];
            else *reinterpret_cast<uint2 *>(&sm.D[buf][(tid + 256 * i) * 4]) = make_uint2(pack_bf16(rd[i].x, rd[i].y), pack_bf16(rd[i].z, rd[i].w));
        }
#pragma unroll
        for (int i = 0; i < NRX; ++i) {
            const int v = tid + 256 * i;
            const int pp = S16 ? v >> 3 : v >> 4, c4 = S16 ? 2 * (v & 7) : v & 15;
            if (pp < NPP) {
                const int kh = pp / PC, c = WG::slot(pp - kh * PC);
                // (round 6) pixel (c & 3) of ci block cb sits in row ((c & 3) + cb) & 3 of its [4 px][16 ch] sub-block: the four blocks of one pixel -- the
                // 8 (bf16) / 16 (fp32) lanes of one store group -- used to land on the same 8 banks of 32, a 4-way conflict on every patch store
                // (SQ_LDS_BANK_CONFLICT 0.16 of the CU's cycles, rounds 3-5); the transpose read only cares which LANE hands in which chunk
                const int o = kh * WF_ROW + ((c >> 2) * 4 + (c4 >> 2)) * 64 + (((c & 3) + (c4 >> 2)) & 3) * 16 + (c4 & 3) * 4;
                if constexpr (S16) *reinterpret_cast<uint4 *>(&sm.X[buf][o]) = rx[i];
                else *reinterpret_cast<uint2 *>(&sm.X[buf][o]) = make_uint2(pack_bf16(rx[i].x, rx[i].y), pack_bf16(rx[i].z, rx[i].w));
            }
        }
    };
    typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
    typedef short s16x8 __attribute__((ext_vector_type(8)));
    const int g = lane >> 4, t16 = lane & 15;
    // fragment offsets (shorts) inside one buffer: they do not depend on the unit, the tap row kh is an immediate offset
    int xo[2][3][2], dofs[2];
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
        const int cib = 2 * wm + (g & 1);                        // 16-channel block of this lane group
        const int jbase = 16 * s2 + 8 * (g >> 1) + (t16 >> 2);   // output pixel handed in by this lane (read 1)
#pragma unroll
        for (int kw = 0; kw < 3; ++kw)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int c = STR == 1 ? jbase + kw + 4 * h : (kw & 1) * 33 + jbase + (kw >> 1) + 4 * h;
                xo[s2][kw][h] = ((c >> 2) * 4 + cib) * 64 + (((c & 3) + cib) & 3) * 16 + (t16 & 3) * 4;      // (rotated rows: see store_unit)
            }
        dofs[s2] = ((4 * s2 + 2 * (g >> 1)) * 4 + 2 * wn + (g & 1)) * 64 + t16 * 4;
    }
    load_unit(u_begin, rx0, rd0);
    store_unit(0, rx0, rd0);
    load_unit(u_begin + 1, rx0, rd0);
    load_unit(u_begin + 2, rx1, rd1);
    lds_barrier();
    // one unit: the set `rp` holds unit u+1 (stored now, then refilled with unit u+3); LDS buffer cur holds unit u
    auto iter = [&](const int u, const int cur, Reg (&rpx)[NRX], Reg (&rpd)[NRD]) {
        store_unit(cur ^ 1, rpx, rpd);
        load_unit(u + 3, rpx, rpd);
        const unsigned short *X = sm.X[cur];
        const unsigned short *D = sm.D[cur];
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
            // B fragment: dy[pixels 16 s2 + 8 hi ..][co = wn*32 + (lane & 31)]  (image of LoaderMNt<64>)
            const s16x4 blo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4 *)(D + dofs[s2]));
            const s16x4 bhi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4 *)(D + dofs[s2] + 4 * 64));
            const bf16x8 bfrag = __builtin_bit_cast(bf16x8, (s16x8)__builtin_shufflevector(blo, bhi, 0, 1, 2, 3, 4, 5, 6, 7));
#pragma unroll
            for (int kh = 0; kh < 3; ++kh)
#pragma unroll
                for (int kw = 0; kw < 3; ++kw) {
                    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4 *)(X + xo[s2][kw][0] + kh * WF_ROW));
                    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4 *)(X + xo[s2][kw][1] + kh * WF_ROW));
                    const bf16x8 afrag = __builtin_bit_cast(bf16x8, (s16x8)__builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
                    acc[kh * 3 + kw] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(afrag, bfrag, acc[kh * 3 + kw], 0, 0, 0);
                }
        }
        lds_barrier();
    };
    {
        int u = u_begin;
        for (; u + 2 <= u_end; u += 2) {
            iter(u, 0, rx0, rd0);
            iter(u + 1, 1, rx1, rd1);
        }
        if (u < u_end) iter(u, 0, rx0, rd0);
    }
    if (a.slab_ts) {       // nine 64 x 64 tiles in accumulator-register order: 36 lane-linear 16-byte stores per lane, no LDS
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            f32x16 one[1][1];
            one[0][0] = acc[t];
            float *slab = a.dw + (long long)blockIdx.z * a.part_stride + ((long long)(t * a.tiles_m + tm) * a.tiles_n + tn) * (64 * 64);
            store_slab_ts<64, 64, 2, 2>(one, slab, wave, lane);
        }
        return;
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        f32x16 one[1][1];
        one[0][0] = acc[t];
        float *dw = a.dw + (long long)t * a.Ci * a.Co + (long long)blockIdx.z * a.part_stride;
        epilogue<64, 64, 2, 2, false>(one, reinterpret_cast<float *>(smem_raw), dw, a.Co, a.Ci, a.Co, ci0, co0, wm, wn, lane, wave, a.e, t == 0);
    }
}

// ------------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------------
typedef void (*ConvKernel)(ConvArgs);
typedef void (*WgradKernel)(ConvWgradArgs);

// forward / input gradient: one workgroup per bm x bn tile of [destination pixels][destination channels]
static void launch_conv_tiles(ConvKernel kernel, int bm, int bn, const ConvArgs &a0, hipStream_t s) {
    ConvArgs a = a0;
    a.tiles_m = cdiv(a.M, bm);
    a.tiles_n = cdiv(a.Cd, bn);
    dim3 grid((unsigned)(a.tiles_m * a.tiles_n)), block(GEMM_THREADS);
    hipLaunchKernelGGL(kernel, grid, block, 0, s, a);
}

// bf16-compute kernel for the storage types of the kernel tensor (W16) and the source tensor (X16)
template <int BM, int BN, int DIL, bool W16, bool X16>
static ConvKernel conv_bf16c_dir(bool dgrad) {
    return dgrad ? conv3x3_bf16c_kernel<BM, BN, 2, 2, true, W16, X16, DIL> : conv3x3_bf16c_kernel<BM, BN, 2, 2, false, W16, X16, DIL>;
}
template <int BM, int BN, int DIL>
static ConvKernel conv_bf16c_for(const ConvArgs &a, bool dgrad) {
    if (a.w16 && a.x16) return conv_bf16c_dir<BM, BN, DIL, true, true>(dgrad);
    if (a.w16) return conv_bf16c_dir<BM, BN, DIL, true, false>(dgrad);
    if (a.x16) return conv_bf16c_dir<BM, BN, DIL, false, true>(dgrad);
    return conv_bf16c_dir<BM, BN, DIL, false, false>(dgrad);
}

// f32x3 split once into LDS (conv_x3.h): 1.0-1.25x the per-wave split (conv3x3_kernel<.., SPLIT3>) on the stride-1 / forward shapes, 0.92x on the
// parity classes of the stride-2 input gradient (1-4 taps: short K loops), which keep the first form (profiles/r06_micro_split3.txt).
// DETR_HIP_X3_CONV=2: first form everywhere, =1: second form everywhere
static bool x3_form(const ConvArgs &a) { return a.Cs % 32 == 0 && tune(T_X3_CONV) != 2 && (!a.par_on || tune(T_X3_CONV) == 1); }

template <int BM, int BN>
static void launch_conv(const ConvArgs &a, bool dgrad, hipStream_t s, bool split3 = false) {
    ConvKernel k = dgrad ? conv3x3_kernel<BM, BN, 2, 2, true> : conv3x3_kernel<BM, BN, 2, 2, false>;
    if constexpr (BM == BN) {
        if (split3 && x3_form(a)) k = dgrad ? conv3x3_x3_kernel<BM, BN, true> : conv3x3_x3_kernel<BM, BN, false>;
        else if (split3) k = dgrad ? conv3x3_kernel<BM, BN, 2, 2, true, true> : conv3x3_kernel<BM, BN, 2, 2, false, true>;
    }
    launch_conv_tiles(k, BM, BN, a, s);
}

// ------------------------------------------------------------------------------------------------
// weight-gradient plan: which kernel, which tile, how many splits of the reduction and how much scratch.  The scratch-size
// queries and the launches all read this one plan, so the caller's workspace is the size the launch expects.
// ------------------------------------------------------------------------------------------------
// row splits of the per-tap weight gradient (tiles = (Ci / tile) * (Co / tile) output tiles per tap)
static int wgrad_split_plan(int M, int tiles, int split, int &rps) {
    if (split <= 0) {
        split = cdiv(1536, tiles * 9);
        const int max_split = cdiv(M, 256);
        if (split > max_split) split = max_split;
        if (split < 1) split = 1;
    }
    rps = cdiv(M, split);
    rps = ((rps + BF_BK - 1) / BF_BK) * BF_BK;       // multiple of both K tiles (16 and 32)
    return cdiv(M, rps);
}
// f32x3 nine-tap-per-launch weight gradient (conv3x3_wgrad_x3_kernel): 512 (128 x 128 tiles, two workgroups per CU) or 1024 (64 x 64 tiles, four) slots.
// The exact kernel's plan above (1536 workgroups, rounded UP) lands just over three rounds of 512 -- 1548 / 1539 / 1584 workgroups for 256 / 128 / 512
// channels.  Whole rounds, rounded DOWN; two rounds measured best over the five 3x3 shapes (1 / 2 / 3: within 5 % of each other; DETR_HIP_X3_WG_ROUNDS)
static int wgrad_x3_split(int M, int tiles, int bm) {
    const int rounds = tune(T_X3_WG_ROUNDS) > 0 ? tune(T_X3_WG_ROUNDS) : 2;
    const int slots = bm >= 128 ? 512 : 1024;
    int split = (rounds * slots) / (tiles * 9);
    const int max_split = cdiv(M, 256);
    if (split > max_split) split = max_split;
    return split < 1 ? 1 : split;
}
// unit splits of the fused nine-tap weight gradient (units of 32 output pixels of one output row)
static int wgrad_fused_split_plan(int units, int tiles, int split, int &ups) {
    if (split <= 0) {
        int wgs = tune(T_WGRAD_FUSED_WGS);      // tuning hook: target workgroup count (512 measured best: 2 per CU)
        if (wgs <= 2) wgs = 512;
        split = cdiv(wgs, tiles);
    }
    if (split > units) split = units;
    if (split < 1) split = 1;
    ups = cdiv(units, split);
    return cdiv(units, ups);
}

struct WgradPlan {
    bool fused;         // the nine-tap bf16 kernel (reduction in units of 32 output pixels) | a per-tap kernel (reduction rows)
    int tile;           // 64 | 128: (ci, co) tile of a workgroup
    int split;          // grid.z: splits of the reduction
    int per_split;      // units (fused) or rows per split
    long long bytes;    // scratch for the splits' partial slabs (0: a single split accumulates onto dw)
};

// s16: x and dy are bf16 in memory; compute: detr_conv3x3_desc.compute; split: the descriptor's request (<= 0: ours)
static WgradPlan wgrad_plan(int N, int Ho, int Wo, int Ci, int Co, int stride, int pad, bool s16, int compute, int dil, int split) {
    WgradPlan p;
    const bool bf = compute == 1 && Ci % 32 == 0 && Co % 32 == 0;
    // nine taps per launch at stride 2 (round 5): bf16-stored tensors only, and only up to 128 channels -- measured (scripts/micro_conv.py,
    // profiles/r05_micro_conv_dma.txt; nine-tap | per-tap, us): 200x334x128 -> 100x167 100.1 | 115.9, 100x167x256 -> 50x84 96.7 | 90.5, 50x84x512 ->
    // 25x42 116.0 | 105.0: the stride-2 patch is twice the bytes per MFMA of the stride-1 one and every (ci, co) tile re-fetches it.
    // DETR_HIP_WGRAD_FUSED = 2: never, 3: per-tap kernel for all stride-2 convolutions, 4: nine-tap kernel for all (A/B).
    const int fmode = tune(T_WGRAD_FUSED);
    const bool s_ok = stride == 1 || (stride == 2 && s16 && fmode != 3 && (fmode == 4 || (Ci <= 128 && Co <= 128)));
    p.fused = dil == 1 && bf && s_ok && pad == 1 && Ci % 64 == 0 && Co % 64 == 0 && fmode != 2;
    if (p.fused) {
        p.tile = 64;
        p.split = wgrad_fused_split_plan(N * Ho * cdiv(Wo, 32), (Ci / 64) * (Co / 64), split, p.per_split);
    } else {
        const int wforce = (bf || dil != 1) ? 0 : tune(T_WGRAD_TILE);
        p.tile = (wforce == 3) ? 64 : ((wforce == 1 || (Ci >= 128 && Co >= 128)) ? 128 : 64);
        const int M = N * Ho * Wo, tiles = cdiv(Ci, p.tile) * cdiv(Co, p.tile);
        if (compute == 2 && split <= 0 && tune(T_X3_CONV) != 2) split = wgrad_x3_split(M, tiles, p.tile);
        p.split = wgrad_split_plan(M, tiles, split, p.per_split);
    }
    p.bytes = p.split > 1 ? (long long)p.split * 9LL * Ci * Co * 4 : 0;
    return p;
}

// Runs `launch(a, grid)` for the plan's (tiles, taps, splits) grid.  With a workspace the splits write partial slabs (tile-ordered where the
// tiles are whole and the final tensors 16-byte aligned -- the rule of gemm_slab_ts) and a fixed-order reduction applies alpha / scale onto dw;
// without one they accumulate onto dw (float atomics when split > 1).
template <class Launch>
static void wgrad_run(const ConvWgradArgs &a0, const WgradPlan &p, int taps_y, float *ws, long long ws_bytes, hipStream_t s, Launch launch) {
    ConvWgradArgs a = a0;
    a.tiles_m = cdiv(a.Ci, p.tile);
    a.tiles_n = cdiv(a.Co, p.tile);
    a.rows_per_split = p.per_split;
    const long long part = 9LL * a.Ci * a.Co;
    const bool partial = p.split > 1 && ws && aligned16(ws) && ws_bytes >= p.bytes;
    float *dw_final = a.dw;
    const EpiArgs final_e = a.e;
    a.part_stride = 0;
    a.slab_ts = 0;
    // (the tile-ordered reduce does 16-byte read-modify-writes of dw and 16-byte slab loads: `partial` already holds aligned16(ws);
    //  a gradient buffer that is only 4-byte aligned keeps the row-major slabs and the scalar reduce)
    const bool ts = partial && a.Ci % p.tile == 0 && a.Co % p.tile == 0 && (!final_e.scale || aligned16(final_e.scale)) &&
                    aligned16(dw_final) && tune(T_SLAB_TS) != 2;
    if (partial) {
        a.dw = ws; a.part_stride = part;
        a.e.alpha = 1.0f;
        a.e.scale = nullptr;
        a.e.atomic = 0;
        a.e.vec = 1;
        a.slab_ts = ts ? 1 : 0;
    } else {
        a.e.atomic = 1;   // accumulate onto dw
    }
    launch(a, dim3((unsigned)(a.tiles_m * a.tiles_n), (unsigned)taps_y, (unsigned)p.split));
    if (partial) {
        detr_reduce_desc r = {};
        r.ws = ws; r.splits = p.split; r.part_stride = part; r.rows = 9 * a.Ci; r.cols = a.Co;
        r.C = dw_final; r.ldc = a.Co; r.alpha = final_e.alpha; r.scale = final_e.scale; r.rs_alpha = 1.0f;
        if (ts) { r.ts_bm = r.ts_bn = p.tile; r.ts_tiles_n = a.tiles_n; }
        launch_splitk_reduce(r, s);
    }
}

// per-tap weight gradient on BT x BT tiles (BT = plan.tile)
template <int BT>
static void launch_wgrad(const ConvWgradArgs &a0, const WgradPlan &p, float *ws, long long ws_bytes, hipStream_t s, bool bf16c, bool split3) {
    WgradKernel k;
    if (a0.dil == 2) {                 // taps two pixels apart (conv_dilated.hip): the per-tap bodies, same plan and reduction
        if (bf16c) k = a0.s16 ? conv3x3_wgrad_bf16c_kernel<BT, BT, 2, 2, true, 2> : conv3x3_wgrad_bf16c_kernel<BT, BT, 2, 2, false, 2>;
        else k = split3 ? conv3x3_wgrad_kernel<BT, BT, 2, 2, true, 2> : conv3x3_wgrad_kernel<BT, BT, 2, 2, false, 2>;
    } else if (bf16c) k = a0.s16 ? conv3x3_wgrad_bf16c_kernel<BT, BT, 2, 2, true> : conv3x3_wgrad_bf16c_kernel<BT, BT, 2, 2, false>;
    else if (split3) k = tune(T_X3_CONV) != 2 ? conv3x3_wgrad_x3_kernel<BT, BT> : conv3x3_wgrad_kernel<BT, BT, 2, 2, true>;
    else k = conv3x3_wgrad_kernel<BT, BT, 2, 2>;
    wgrad_run(a0, p, 9, ws, ws_bytes, s, [&](const ConvWgradArgs &a, dim3 grid) { hipLaunchKernelGGL(k, grid, dim3(GEMM_THREADS), 0, s, a); });
}

// fused-tap bf16 weight gradient (pad 1, channel counts % 64 == 0)
static void launch_wgrad_fused(const ConvWgradArgs &a0, const WgradPlan &p, float *ws, long long ws_bytes, hipStream_t s) {
    const int chunks = cdiv(a0.Wo, 32);
    wgrad_run(a0, p, 1, ws, ws_bytes, s, [&](const ConvWgradArgs &a, dim3 grid) {
        const dim3 block(GEMM_THREADS);
        if (a.stride == 2) hipLaunchKernelGGL((conv3x3_wgrad_fused_bf16_kernel<true, 2>), grid, block, 0, s, a, p.per_split, chunks);
        else if (a.s16) hipLaunchKernelGGL(conv3x3_wgrad_fused_bf16_kernel<true>, grid, block, 0, s, a, p.per_split, chunks);
        else hipLaunchKernelGGL(conv3x3_wgrad_fused_bf16_kernel<false>, grid, block, 0, s, a, p.per_split, chunks);
    });
}

static void launch_wgrad_plan(const ConvWgradArgs &a, const WgradPlan &p, float *ws, long long ws_bytes, hipStream_t s, bool bf16c, bool split3) {
    if (p.fused) launch_wgrad_fused(a, p, ws, ws_bytes, s);
    else if (p.tile == 128) launch_wgrad<128>(a, p, ws, ws_bytes, s, bf16c, split3);
    else launch_wgrad<64>(a, p, ws, ws_bytes, s, bf16c, split3);
}

// ------------------------------------------------------------------------------------------------
// dilation 2 (conv_dilated.hip; conv_args.h declares these): the implicit-GEMM tile bodies above with their taps two pixels
// apart -- forward / input gradient on 64 x 64 tiles, weight gradient per tap on the dense rule's tiles
// ------------------------------------------------------------------------------------------------
void conv_dilated_tiles(const ConvArgs &a, bool dgrad, int compute, hipStream_t s) {
    ConvKernel k;
    if (compute == 1) k = conv_bf16c_for<64, 64, 2>(a, dgrad);
    else if (compute == 2) k = dgrad ? conv3x3_kernel<64, 64, 2, 2, true, true, 2> : conv3x3_kernel<64, 64, 2, 2, false, true, 2>;
    else k = dgrad ? conv3x3_kernel<64, 64, 2, 2, true, false, 2> : conv3x3_kernel<64, 64, 2, 2, false, false, 2>;
    launch_conv_tiles(k, 64, 64, a, s);
}

static WgradPlan conv_dilated_wgrad_plan(int N, int H, int W, int Ci, int Co, bool s16, int compute, int split) {
    return wgrad_plan(N, H, W, Ci, Co, 1, 2, s16, compute, 2, split);
}

void conv_dilated_wgrad_tiles(const ConvWgradArgs &a, int compute, int split, float *ws, long long ws_bytes, hipStream_t s) {
    launch_wgrad_plan(a, conv_dilated_wgrad_plan(a.N, a.Ho, a.Wo, a.Ci, a.Co, a.s16, compute, split), ws, ws_bytes, s, compute == 1, compute == 2);
}

// row splits that call will use (the scratch-size query)
int conv_dilated_wgrad_splits(int N, int H, int W, int Ci, int Co, int compute, int split) {
    return conv_dilated_wgrad_plan(N, H, W, Ci, Co, false, compute, split).split;
}

}  // namespace detr

using namespace detr;

static WgradPlan wgrad_plan(const detr_conv3x3_desc *d) {
    return wgrad_plan(d->N, d->Ho, d->Wo, d->Ci, d->Co, d->stride, d->pad, d->x_dtype == 1 && d->w_dtype == 1, d->compute, 1, d->split);
}

// The halo-staged kernels (conv_halo.h) take stride-1 convolutions on all-bf16 tensors with the epilogues they have (DETR_HIP_CONV_HALO=2 =
// off) and, in their class form, the stride-2 input gradient (dgrad_classes; DETR_HIP_DGRAD_S2_CLASSES = 3: tile kernel).  With 4-row tiles
// they also take the 512-channel convs of layer4 (25 x 42 maps: 92.9 -> 64.5 us forward, 103.2 -> 65.5 us input gradient against the
// 64x64 implicit-GEMM tiles; with 8-row tiles -- 64 workgroups x 4 channel slices, half of every tile padding -- it lost).
static bool halo_eligible(const detr_conv3x3_desc *d, const ConvArgs &a, const EpiArgs &e, bool dgrad_classes) {
    if (!(d->compute == 1 && d->pad == 1 && a.w16 && a.x16 && e.c16 && a.Cs % 32 == 0 && a.Cd % 64 == 0 && a.Cd <= 512 &&
          (!d->mask || e.m16) && !d->residual && !d->scale && d->alpha == 1.0f && tune(T_CONV_HALO) != 2)) return false;
    if (dgrad_classes) return d->stride == 2 && !d->bias && d->act == 0 && tune(T_DGRAD_S2_CLASSES) != 3;
    return d->stride == 1 && (d->act == 0 || d->act == 1);
}

extern "C" int64_t detr_hip_workspace_bytes_conv3x3(const detr_conv3x3_desc *d, int32_t mode) {
    if (!d || d->N <= 0 || d->Ci <= 0 || d->Co <= 0) return -1;
    if (mode != 2) return 0;                       // forward / input gradient: no scratch
    return wgrad_plan(d).bytes;
}

extern "C" int detr_hip_conv3x3_f32(const detr_conv3x3_desc *d, int32_t mode, void *stream) {
    DETR_REQUIRE(d != nullptr, "conv3x3: null descriptor");
    DETR_REQUIRE(mode >= 0 && mode <= 2, "conv3x3: bad mode %d", mode);
    DETR_REQUIRE(d->stride == 1 || d->stride == 2, "conv3x3: stride %d unsupported", d->stride);
    DETR_REQUIRE(d->Ci % 16 == 0 && d->Co % 16 == 0, "conv3x3: Ci=%d Co=%d must be multiples of 16", d->Ci, d->Co);
    DETR_REQUIRE(d->Ho == (d->Hi + 2 * d->pad - 3) / d->stride + 1 && d->Wo == (d->Wi + 2 * d->pad - 3) / d->stride + 1,
                 "conv3x3: output %dx%d inconsistent with input %dx%d pad %d stride %d", d->Ho, d->Wo, d->Hi, d->Wi,
                 d->pad, d->stride);
    DETR_REQUIRE(d->x && d->w && d->y, "conv3x3: null operand");
    DETR_REQUIRE(d->compute >= 0 && d->compute <= 2, "conv3x3: compute %d (0 = fp32, 1 = bf16, 2 = f32x3)", d->compute);
    DETR_REQUIRE((d->w_dtype == 0 || d->w_dtype == 1) && (d->x_dtype == 0 || d->x_dtype == 1) && (d->y_dtype == 0 || d->y_dtype == 1) &&
                 (d->r_dtype == 0 || d->r_dtype == 1) && d->m_dtype >= 0 && d->m_dtype <= 2,
                 "conv3x3: storage types w %d x %d y %d r %d (0 = fp32, 1 = bf16), m %d (2 = bit-packed as well)", d->w_dtype, d->x_dtype, d->y_dtype,
                 d->r_dtype, d->m_dtype);
    DETR_REQUIRE(aligned16(d->x) && aligned16(d->w) && aligned16(d->y), "conv3x3: operands must be 16-byte aligned");
    DETR_REQUIRE((long long)d->N * d->Hi * d->Wi * d->Ci * 4 <= BUF_MAX_BYTES &&
                     (long long)d->N * d->Ho * d->Wo * d->Co * 4 <= BUF_MAX_BYTES,
                 "conv3x3: a tensor spans more than 4 GB (32-bit buffer offsets)");
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
            (!d->residual || aligned16(d->residual)) && (!d->mask || bits_in || aligned16(d->mask));   // channel counts are % 16
    e.c16 = (mode != 2 && d->y_dtype == 1); e.r16 = d->r_dtype == 1;
    e.m16 = (d->m_dtype == 1 || d->m_dtype == 2) ? d->m_dtype : 0;          // 2: bit-packed mask (see detr_gemm_desc.maskbits_out)
    if (mode == 2) {
        DETR_REQUIRE(!d->bias && !d->residual && !d->mask && d->act == 0, "conv3x3 wgrad: only scale/alpha epilogue");
        ConvWgradArgs a;
        a.N = d->N; a.Hi = d->Hi; a.Wi = d->Wi; a.Ci = d->Ci; a.Ho = d->Ho; a.Wo = d->Wo; a.Co = d->Co;
        a.stride = d->stride; a.pad = d->pad;
        a.x = d->x; a.dy = d->w; a.dw = d->y;
        a.M = d->N * d->Ho * d->Wo;
        a.s16 = (d->x_dtype == 1);
        DETR_REQUIRE(d->x_dtype == d->w_dtype && d->y_dtype == 0, "conv3x3 wgrad: x and dy must share their storage type, dw is fp32");
        DETR_REQUIRE(!a.s16 || (d->compute == 1 && d->Ci % 32 == 0 && d->Co % 32 == 0), "conv3x3 wgrad: bf16 tensors need compute = bf16");
        e.atomic = 1; e.ldr = 0; e.ldmask = 0;
        a.e = e;
        const bool bf = d->compute == 1 && d->Ci % 32 == 0 && d->Co % 32 == 0;
        const WgradPlan p = wgrad_plan(d);
        launch_wgrad_plan(a, p, d->workspace, d->workspace_bytes, s, bf, !bf && d->compute == 2);
        DETR_LAUNCH_CHECK(p.fused ? "conv3x3 wgrad bf16 (fused taps)" : (bf ? "conv3x3 wgrad bf16" : "conv3x3 wgrad"));
        return 0;
    }
    ConvArgs a;
    a.N = d->N; a.stride = d->stride; a.pad = d->pad; a.Ci = d->Ci; a.Co = d->Co;
    a.w = d->w; a.src = d->x; a.dst = d->y;
    if (mode == 0) {
        a.Hs = d->Hi; a.Ws = d->Wi; a.Cs = d->Ci;
        a.Hd = d->Ho; a.Wd = d->Wo; a.Cd = d->Co;
    } else {
        a.Hs = d->Ho; a.Ws = d->Wo; a.Cs = d->Co;
        a.Hd = d->Hi; a.Wd = d->Wi; a.Cd = d->Ci;
    }
    a.M = d->N * a.Hd * a.Wd;
    e.ldr = a.Cd;
    e.ldmask = bits_in ? a.Cd / 8 : a.Cd;
    e.mbits_out = bits_out ? d->maskbits_out : nullptr;
    e.ld_mbits_out = a.Cd / 8;
    // all-bf16 epilogue streams (channel counts are % 16, rows 16-byte aligned): 8 columns per lane (gemm_core.h epilogue_wide16)
    e.wide16 = e.c16 && e.vec && (!d->residual || e.r16) && (!d->mask || e.m16) && (tune(T_EPI_WIDE) != 2 || bits_in || bits_out);
    DETR_REQUIRE(!(bits_in || bits_out) || (d->compute == 1 && e.wide16), "conv3x3: bit-packed masks need bf16 x / y / residual tensors (compute = bf16)");
    a.e = e;
    a.w16 = (d->w_dtype == 1);
    a.x16 = (d->x_dtype == 1);
    DETR_REQUIRE((d->x_dtype == 0 && d->y_dtype == 0 && d->r_dtype == 0 && d->m_dtype == 0) || (d->compute == 1 && d->Ci % 32 == 0 && d->Co % 32 == 0),
                 "conv3x3: bf16 tensors need compute = bf16 and channel counts %% 32 == 0");
    DETR_REQUIRE(d->w_dtype == 0 || (d->w_dtype == 1 && d->compute == 1 && mode != 2 && d->Ci % 32 == 0 && d->Co % 32 == 0),
                 "conv3x3: a bf16 kernel tensor needs compute = bf16, mode 0/1 and channel counts %% 32 == 0");
    a.par_on = 0; a.Hp = a.Wp = a.ph = a.pw = a.kh0 = a.kw0 = 0; a.nth = a.ntw = 3;
    a.cls_mix = 0;
    const bool dgrad = mode == 1;
    // stride-1 convs on bf16 tensors: the halo-staged kernel, for 128-channel panels on 4-row tiles its LDS-DMA form
    // (conv_halo_dma.h: bit-identical, 5-10 % faster; DETR_HIP_CONV_DMA=2 = off)
    if (halo_eligible(d, a, e, false)) {
        if (a.Cd >= 128 && a.Cd % 128 == 0 && tune(T_CONV_DMA) != 2 && tune(T_CONV_HALO) != 4) { if (launch_conv_halo_dma(a, dgrad, s)) return -1; }
        // (the halo epilogue has no column guard: a 128-channel tile needs Cd % 128 == 0; 192 / 320 / 448 channels take 64-channel tiles)
        else if (a.Cd % 128 == 0) { if (launch_conv_halo<128>(a, dgrad, s)) return -1; }
        else if (launch_conv_halo<64>(a, dgrad, s)) return -1;
        DETR_LAUNCH_CHECK("conv3x3 (halo)");
        return 0;
    }
    const int force = tune(T_CONV_TILE);     // tuning hook; 0 = heuristic
    auto launch = [&](const ConvArgs &c) {
        const long long big = (long long)cdiv(c.M, 128) * cdiv(c.Cd, 128);
        if (d->compute == 1 && c.Cs % 32 == 0 && c.Cd % 32 == 0) {
            // measured: profiles/tune_bf16_r1d.txt; round 3 (scripts/micro_conv.py, with the wide epilogue): the stride-2 forward at 128
            // channels 83 -> 72 us (cold 113 -> 97) and its input-gradient classes 173 -> 165 us on 128x128 tiles
            if (force == 3 || (force == 0 && (c.Cd < 128 || big < 256)))
                launch_conv_tiles(conv_bf16c_for<64, 64, 1>(c, dgrad), 64, 64, c, s);
            else launch_conv_tiles(conv_bf16c_for<128, 128, 1>(c, dgrad), 128, 128, c, s);
        } else if (d->compute == 2) {
            // f32x3: 64 x 64 wave tiles (128 x 128 workgroup tiles) are matrix-pipe bound, 32 x 32 ones VALU bound (see gemm_pick_tile)
            // 192 x 128 tiles where 128 x 128 ones overflow the 512 workgroup slots (two per CU) by a few: 256 channels at 50 x 84 are 526 tiles = two
            // rounds, 350 tiles of 192 rows one round of 1.5 x the work (common.h: the rule gemm_pick_tile shares; DETR_HIP_X3_T192 = 2: never, 1: always)
            const long long t192 = (long long)cdiv(c.M, 192) * cdiv(c.Cd, 128);
            const bool x3form = x3_form(c);
            if (force == 3 || (force == 0 && (c.Cd < 128 || big < x3_t128_threshold()))) launch_conv<64, 64>(c, dgrad, s, true);
            else if (force == 0 && x3form && tune(T_X3_T192) != 2 && tune(T_X3_T192) != 3 && (tune(T_X3_T192) == 1 || x3_t192_fewer_rounds(big, t192)))
                launch_conv_tiles(dgrad ? conv3x3_x3_kernel<192, 128, true> : conv3x3_x3_kernel<192, 128, false>, 192, 128, c, s);
            // 128 x 64 tiles, three workgroups per CU: one 128-channel panel (layer2: 1044 tiles of 128 x 128 = 2.04 rounds -> 290 vs 275 us) and grids
            // that leave CUs with a single 128 x 128 workgroup (layer4: 264 tiles -> 357 vs 338 us); DETR_HIP_X3_T192 = 3: wherever 128 x 128 would run
            else if (force == 0 && x3form && tune(T_X3_T192) != 2 && (tune(T_X3_T192) == 3 || c.Cd == 128 || big <= 384)) 
                launch_conv_tiles(dgrad ? conv3x3_x3_kernel<128, 64, true> : conv3x3_x3_kernel<128, 64, false>, 128, 64, c, s);
            else launch_conv<128, 128>(c, dgrad, s, true);
        } else if (force == 1) launch_conv<128, 128>(c, dgrad, s);
        else if (force == 2) launch_conv<128, 64>(c, dgrad, s);
        else launch_conv<64, 64>(c, dgrad, s);   // 64x64 measured best on every backbone shape (profiles/tune_r1.txt)
    };
    if (dgrad && d->stride == 2 && tune(T_DGRAD_S2_CLASSES) != 2) {
        // one launch per destination-pixel parity class: 1 + 2 + 2 + 4 tap-GEMMs instead of 9 with 3/4 of the rows masked
        // all-bf16 tensors: the class form of the halo-staged kernel
        if (halo_eligible(d, a, e, true)) {
            if (a.Cd % 128 == 0) { if (launch_conv_halo_s2classes<128>(a, s)) return -1; }
            else if (launch_conv_halo_s2classes<64>(a, s)) return -1;
            DETR_LAUNCH_CHECK("conv3x3 (halo, stride-2 classes)");
            return 0;
        }
        for (int ph = 0; ph < 2; ++ph)
            for (int pw = 0; pw < 2; ++pw) {
                ConvArgs c = a;
                c.par_on = 1; c.ph = ph; c.pw = pw;
                c.Hp = (a.Hd + 1 - ph) / 2;
                c.Wp = (a.Wd + 1 - pw) / 2;
                c.M = d->N * c.Hp * c.Wp;
                if (c.M <= 0) continue;
                c.kh0 = (ph + d->pad) & 1; c.kw0 = (pw + d->pad) & 1;
                c.nth = c.kh0 ? 1 : 2; c.ntw = c.kw0 ? 1 : 2;
                c.e.remap_w2 = c.Wp; c.e.remap_h2 = c.Hp; c.e.remap_W = a.Wd; c.e.remap_H = a.Hd;
                c.e.remap_ph = ph; c.e.remap_pw = pw;
                launch(c);
            }
    } else {
        launch(a);
    }
    DETR_LAUNCH_CHECK("conv3x3");
    return 0;
}

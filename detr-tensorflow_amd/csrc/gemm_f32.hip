// gemm_f32.hip -- generic batched fp32 GEMM with fused epilogue on the MFMA tile engine.
// Replaces every tf.matmul / 1x1 Conv2D / Linear of the reference's hot path and their
// gradients (see include/detr_hip.h for the reference lines).
#include "gemm_core.h"
#include "gemm_bf16_core.h"
#include "gemm_stream.h"

#include "gemm_kernels.h"
#include "gemm_x3.h"
#include "gemm_ring.h"

namespace detr {

// Reduction of the split-K partial slabs: 256 threads = (256 / G) float4 outputs x G split groups (the groups stride the
// split index), combined through LDS in a fixed order.  G = 4 for large outputs; G = 16 for small ones (a 256 x 256
// weight gradient has only 16 K float4 outputs: with G = 4 the launch is 256 blocks and purely latency bound).
// One planned reduction: the caller's record (ts_tiles_n >= 1 from reduce_plan on) plus what the launch adds.
struct ReduceOne : detr_reduce_desc {
    int vec;         // the row-major slabs and C take 16-byte accesses
    int nblocks;     // workgroups this reduction uses (its grid-stride loops run over nblocks, not over the launch's grid)
};

template <int G>
__device__ __forceinline__ void splitk_reduce_body(const float *__restrict__ ws, int splits, long long part_stride,
                                                   int rows, int cols, float *__restrict__ C, long long ldc,
                                                   float alpha, const float *__restrict__ scale, int vec,
                                                   const float *__restrict__ rs_ws, float *__restrict__ rs_out,
                                                   float rs_alpha, const int bid, const int nbid,
                                                   const int ts_bm = 0, const int ts_bn = 0, const int ts_tn = 1) {
    constexpr int OUT = 256 / G;
    __shared__ float4 red[G][OUT];
    if (rs_ws) {     // fused bias gradient: partial row sums [splits][rows] -> rs_out[rows] (fixed summation order)
        for (int m = bid * 256 + threadIdx.x; m < rows; m += nbid * 256) {
            float t = 0.0f;
            for (int k = 0; k < splits; ++k) t += rs_ws[(long long)k * rows + m];
            rs_out[m] += rs_alpha * t;
        }
    }
    const int lo = threadIdx.x % OUT, grp = threadIdx.x / OUT;
    if (ts_bm > 0) {
        // tile-ordered slabs: unit i (a float4 = 4 consecutive ROWS of one column, gemm_core.h: slab_ts_unit) is summed over the
        // splits in the same order as a row-major element would be (k = grp, grp + G, ..., then the G groups in order), so the
        // result is bit-identical to the row-major path.  Reads are lane-linear.  The four lanes of a quad hold a 4 x 4 block
        // (4 rows x 4 consecutive columns): it is transposed through LDS so that every lane updates C with ONE 16-byte
        // read-modify-write of a row (first version: four 4-byte ones per lane -- the reduce launches got 30 % slower).
        __shared__ float tr[OUT][5];
        const int upt = (ts_bm * ts_bn) >> 2;
        const long long total = part_stride >> 2;           // a multiple of 1024: a quad is inside or outside as a whole
        for (long long base = (long long)bid * OUT; base < total; base += (long long)nbid * OUT) {
            const long long i = base + lo;
            const bool valid = i < total;
            float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
            if (valid) {
                const float *p = ws + i * 4;
#pragma unroll 4
                for (int k = grp; k < splits; k += G) {
                    const float4 v = *reinterpret_cast<const float4 *>(p + k * part_stride);
                    s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
                }
            }
            red[grp][lo] = s;
            __syncthreads();
            if (grp == 0) {
#pragma unroll
                for (int q = 1; q < G; ++q) {
                    const float4 t = red[q][lo];
                    s.x += t.x; s.y += t.y; s.z += t.z; s.w += t.w;
                }
                tr[lo][0] = s.x; tr[lo][1] = s.y; tr[lo][2] = s.z; tr[lo][3] = s.w;
            }
            __syncthreads();
            if (grp == 0 && valid) {
                const int qb = lo & ~3, t = lo & 3;             // lane t of the quad takes row t of the block
                const long long iq = base + qb;
                const int tile = (int)(iq / upt), u = (int)(iq - (long long)tile * upt);
                int row0, col;
                slab_ts_unit(u, ts_bm, ts_bn, row0, col);
                const int row = row0 + (tile / ts_tn) * ts_bm + t;
                col += (tile % ts_tn) * ts_bn;
                if (row < rows && col < cols) {                 // (cols % 4 == 0, col % 4 == 0: the four columns exist together)
                    const float4 v = make_float4(tr[qb][t], tr[qb + 1][t], tr[qb + 2][t], tr[qb + 3][t]);
                    float4 sc = make_float4(1.f, 1.f, 1.f, 1.f);
                    if (scale) sc = *reinterpret_cast<const float4 *>(scale + col);
                    float4 *dst = reinterpret_cast<float4 *>(C + (long long)row * ldc + col);
                    float4 o = *dst;
                    o.x += alpha * sc.x * v.x; o.y += alpha * sc.y * v.y; o.z += alpha * sc.z * v.z; o.w += alpha * sc.w * v.w;
                    *dst = o;
                }
            }
            // (no third barrier: red[] is rewritten after barrier 2, behind every read of it; tr[] is rewritten after the NEXT
            //  iteration's barrier 1, which the lanes reading it here have to reach first)
        }
    } else if (vec) {
        const int c4n = cols >> 2;
        const long long total = (long long)rows * c4n;
        for (long long base = (long long)bid * OUT; base < total; base += (long long)nbid * OUT) {
            const long long i = base + lo;
            const bool valid = i < total;
            int r = 0, c = 0;
            float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
            if (valid) {
                r = (int)(i / c4n);
                c = (int)(i - (long long)r * c4n) * 4;
                const float *p = ws + (long long)r * cols + c;
#pragma unroll 4
                for (int k = grp; k < splits; k += G) {
                    const float4 v = *reinterpret_cast<const float4 *>(p + k * part_stride);
                    s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
                }
            }
            red[grp][lo] = s;
            __syncthreads();
            if (grp == 0 && valid) {
#pragma unroll
                for (int q = 1; q < G; ++q) {
                    const float4 t = red[q][lo];
                    s.x += t.x; s.y += t.y; s.z += t.z; s.w += t.w;
                }
                float4 sc = make_float4(1.f, 1.f, 1.f, 1.f);
                if (scale) sc = *reinterpret_cast<const float4 *>(scale + c);
                float4 *dst = reinterpret_cast<float4 *>(C + (long long)r * ldc + c);
                float4 o = *dst;
                o.x += alpha * sc.x * s.x; o.y += alpha * sc.y * s.y; o.z += alpha * sc.z * s.z; o.w += alpha * sc.w * s.w;
                *dst = o;
            }
            __syncthreads();
        }
    } else {
        const long long total = (long long)rows * cols;
        for (long long i = bid * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)nbid * blockDim.x) {
            const int r = (int)(i / cols), c = (int)(i - (long long)r * cols);
            float s = 0.f;
            for (int k = 0; k < splits; ++k) s += ws[k * part_stride + i];
            C[(long long)r * ldc + c] += alpha * (scale ? scale[c] : 1.0f) * s;
        }
    }
}

// Up to NMAX reductions of one size class in one launch: entry blockIdx.y.  NMAX = 1: a single reduction; GEMM_MAX_GROUP: the members
// of a grouped GEMM; REDUCE_MANY: the deferred reductions of a backward pass (detr_hip_splitk_reduce_many).
constexpr int REDUCE_MANY = 16;
template <int NMAX> struct ReduceArgs { ReduceOne r[NMAX]; };
template <int G, int NMAX>
__global__ __launch_bounds__(256) void splitk_reduce_kernel(ReduceArgs<NMAX> R) {
    const ReduceOne &r = R.r[NMAX == 1 ? 0 : blockIdx.y];
    if ((int)blockIdx.x >= r.nblocks) return;
    splitk_reduce_body<G>(r.ws, r.splits, r.part_stride, r.rows, r.cols, r.C, r.ldc, r.alpha, r.scale, r.vec, r.rs_ws, r.rs_out,
                          r.rs_alpha, blockIdx.x, r.nblocks, r.ts_bm, r.ts_bn, r.ts_tiles_n);
}

// `small` (16 instead of 4 split groups per block) is a function of (rows, cols, splits) alone -- the summation order, and with it
// the bits of the result, must not depend on the slab layout
static ReduceOne reduce_plan(const detr_reduce_desc &d, bool &small) {
    ReduceOne r;
    static_cast<detr_reduce_desc &>(r) = d;
    if (r.ts_tiles_n <= 0) r.ts_tiles_n = 1;
    r.vec = (r.cols % 4 == 0) && (r.ldc % 4 == 0) && (r.part_stride % 4 == 0) && aligned16(r.ws) && aligned16(r.C) &&
            (!r.scale || aligned16(r.scale));
    const bool ts = r.ts_bm > 0;
    const bool vec_like = r.vec || ts;
    const long long total = (long long)r.rows * (vec_like ? r.cols / 4 : r.cols);
    small = vec_like && total <= 65536 && r.splits >= 8;
    const long long units = ts ? r.part_stride / 4 : total;
    long long grid = vec_like ? (units + (small ? 15 : 63)) / (small ? 16 : 64) : (units + 255) / 256;
    if (grid > 8192) grid = 8192;
    if (grid < 1) grid = 1;
    r.nblocks = (int)grid;
    return r;
}

// One launch for the n <= NMAX planned reductions r[0..n), all of the size class `small`: grid.x is the largest of their block counts
// (an entry's surplus blocks leave at once), the unused slots repeat entry 0.
template <int NMAX>
static void launch_reduce_list(const ReduceOne *r, int n, bool small, hipStream_t s) {
    ReduceArgs<NMAX> R;
    unsigned rx = 1;
    for (int i = 0; i < NMAX; ++i) {
        R.r[i] = r[i < n ? i : 0];
        if ((unsigned)R.r[i].nblocks > rx) rx = (unsigned)R.r[i].nblocks;
    }
    const dim3 grid(rx, (unsigned)n), block(256);
    if (small) hipLaunchKernelGGL((splitk_reduce_kernel<16, NMAX>), grid, block, 0, s, R);
    else hipLaunchKernelGGL((splitk_reduce_kernel<4, NMAX>), grid, block, 0, s, R);
}

void launch_splitk_reduce(const detr_reduce_desc &d, hipStream_t stream) {
    bool small;
    const ReduceOne r = reduce_plan(d, small);
    launch_reduce_list<1>(&r, 1, small, stream);
}

// ---- kernel selection: a kernel family is a struct whose get<AK, BKC>() names one instantiation; by_layout picks the operand layouts ----
typedef void (*GemmKernel)(GemmArgs);
typedef void (*GemmGroupKernel)(GemmGroupArgs);

template <class F>
static auto by_layout(bool ak, bool bk) {
    return ak ? (bk ? F::template get<true, true>() : F::template get<true, false>())
              : (bk ? F::template get<false, true>() : F::template get<false, false>());
}

template <int BM, int BN, int WGM, int WGN> struct F32Kernels {
    template <bool AK, bool BKC> static GemmKernel get() { return gemm_f32_kernel<BM, BN, WGM, WGN, AK, BKC>; }
};
template <int BM, int BN, bool DB> struct X3Kernels {
    template <bool AK, bool BKC> static GemmKernel get() {
        // 192 x 128: K-contiguous A only (the transpose-read image of an MN-contiguous operand needs a power-of-two block count)
        if constexpr (BM == 192 && !AK) return nullptr;
        else return gemm_x3_kernel<BM, BN, AK, BKC, DB>;
    }
};
template <int BM, int BN, bool A16, bool B16> struct Bf16Kernels {
    template <bool AK, bool BKC> static GemmKernel get() { return gemm_bf16c_kernel<BM, BN, 2, 2, AK, BKC, A16, B16>; }
};
template <int BM, int BN> struct Bf16K64Kernels {
    template <bool AK, bool BKC> static GemmKernel get() { return gemm_bf16c_k64_kernel<BM, BN, 2, 2, AK, BKC>; }
};
struct GroupF32Kernels {
    template <bool AK, bool BKC> static GemmGroupKernel get() { return gemm_f32_group_kernel<64, 64, 2, 2, AK, BKC>; }
};
struct GroupX3Kernels {
    template <bool AK, bool BKC> static GemmGroupKernel get() { return gemm_x3_group_kernel<64, 64, AK, BKC>; }
};
template <bool A16, bool B16> struct GroupBf16Kernels {
    template <bool AK, bool BKC> static GemmGroupKernel get() { return gemm_bf16c_group_kernel<64, 64, 2, 2, AK, BKC, A16, B16>; }
};

// compute = 2 on the shapes of gemm_split3_shape: the f32x3 kernel (gemm_x3.h)
// DETR_HIP_X3_DB: 1 = double-buffered LDS (in-wave overlap); 0 / 2 = single-buffered, which measured faster on every shape of the step
// (profiles/r06_micro_split3.txt: two workgroups per CU overlap better than one with two buffers); 192 x 128 is single-buffered only
template <int BM, int BN>
static GemmKernel gemm_x3_for(bool ak, bool bk) {
    if constexpr (BM != 192) {
        if (tune(T_X3_DB) == 1) return by_layout<X3Kernels<BM, BN, true>>(ak, bk);
    }
    return by_layout<X3Kernels<BM, BN, false>>(ak, bk);
}

// k64: the 64-deep K tiles of the all-bf16 operands (64 x 64 and 128 x 128 tiles only)
template <int BM, int BN>
static GemmKernel gemm_bf16_for(bool ak, bool bk, bool a16, bool b16, bool k64) {
    if constexpr ((BM == 64 && BN == 64) || (BM == 128 && BN == 128)) {
        if (k64 && a16 && b16) return by_layout<Bf16K64Kernels<BM, BN>>(ak, bk);
    }
    if (a16) return b16 ? by_layout<Bf16Kernels<BM, BN, true, true>>(ak, bk) : by_layout<Bf16Kernels<BM, BN, true, false>>(ak, bk);
    return b16 ? by_layout<Bf16Kernels<BM, BN, false, true>>(ak, bk) : by_layout<Bf16Kernels<BM, BN, false, false>>(ak, bk);
}

static GemmGroupKernel gemm_group_for(bool bf16c, bool split3, bool ak, bool bk, bool a16, bool b16) {
    if (!bf16c) return split3 ? by_layout<GroupX3Kernels>(ak, bk) : by_layout<GroupF32Kernels>(ak, bk);
    if (a16) return b16 ? by_layout<GroupBf16Kernels<true, true>>(ak, bk) : by_layout<GroupBf16Kernels<true, false>>(ak, bk);
    return b16 ? by_layout<GroupBf16Kernels<false, true>>(ak, bk) : by_layout<GroupBf16Kernels<false, false>>(ak, bk);
}

// one workgroup per (bm x bn tile, batch member x split)
static int launch_gemm_tiles(GemmKernel kernel, int bm, int bn, const GemmArgs &g, int batch, hipStream_t s) {
    DETR_REQUIRE(kernel != nullptr && bm > 0 && bn > 0, "gemm: no kernel for this tile, precision and operand layout");
    GemmArgs a = g;
    a.tiles_m = cdiv(g.M, bm);
    a.tiles_n = cdiv(g.N, bn);
    const dim3 grid((unsigned)(a.tiles_m * a.tiles_n), 1, (unsigned)(batch * g.split_k));
    hipLaunchKernelGGL(kernel, grid, dim3(GEMM_THREADS), 0, s, a);
    return 0;
}

}  // namespace detr

using namespace detr;

// Tile ids.  The values are the interface of DETR_HIP_GEMM_TILE (gemm_pick_tile maps `force` to them) and stay as they are.
enum GemmTile {
    TILE_64x64 = 0,
    TILE_128x128 = 1,
    TILE_128x64 = 2,
    TILE_128x32 = 3,             // exact fp32 only (N <= 32)
    TILE_WIDE = 4,               // 64 x 256 (exact fp32) / 64 x 128 (bf16)
    TILE_256x64 = 5,             // exact fp32 only
    TILE_RING_128x256 = 6,       // ring weight gradient only (bf16; DETR_HIP_RING_WTILE)
    TILE_RING_256x128 = 7,
    TILE_X3_192x128 = 8          // f32x3 only, unsplit
};

// Host side of one GEMM: validation + kernel arguments (gemm_prepare), then the launch(es) (gemm_launch).  The grouped entry
// point prepares every member the same way and, when they share one kernel variant, issues ONE launch for all of them.
struct GemmPlan {
    GemmArgs g;
    int batch, split;
    bool ak, bk, bf16c, partial;
    bool split3;              // compute = 2: fp32 storage and accuracy on the bf16 matrix pipe (3-way operand split; gemm_x3.h)
    bool deep;                // the all-bf16 variants walk 64-deep K tiles instead of 32-deep ones (64x64 / 128x128 tiles only)
    GemmTile tile;
    long long part;           // floats per split slab (row-major: M*N; tile-ordered: the padded tile grid)
    int ts_bm, ts_bn, ts_tn;  // tile-ordered slabs (0: row-major)
    EpiArgs final_e;
    const detr_gemm_desc *d;
};

// The one table of tile shapes: BM x BN and the wave grid of a tile id for a precision (bf16c: compute = 1; otherwise the exact fp32 and
// the f32x3 kernels), shared by the launch path and by the scratch-size query.  slab_ts: the kernel can write tile-ordered split-K slabs
// (store_slab_ts / slab_ts_unit: 2 x 2 wave grids; the 4 x 1 / 1 x 4 grids of the narrow fp32 tiles keep row-major slabs).  A tile the
// precision does not have answers bm = bn = 0.
struct TileDims { int bm, bn, wgm, wgn; bool slab_ts; };
static TileDims gemm_tile_dims(bool bf16c, GemmTile tile) {
    switch (tile) {
        case TILE_64x64: return {64, 64, 2, 2, true};
        case TILE_128x128: return {128, 128, 2, 2, true};
        case TILE_128x64: return {128, 64, 2, 2, true};
        case TILE_128x32: if (!bf16c) return {128, 32, 4, 1, false}; break;
        case TILE_WIDE: if (bf16c) return {64, 128, 2, 2, true}; return {64, 256, 1, 4, false};
        case TILE_256x64: if (!bf16c) return {256, 64, 4, 1, false}; break;
        case TILE_RING_128x256: if (bf16c) return {128, 256, 2, 2, true}; break;
        case TILE_RING_256x128: if (bf16c) return {256, 128, 2, 2, true}; break;
        case TILE_X3_192x128: if (!bf16c) return {192, 128, 2, 2, true}; break;
    }
    return {0, 0, 0, 0, false};
}
// Split-K slab layout: tile-ordered when the reduce launch can keep its 16-byte form (the same conditions as its row-major
// `vec` path: the summation order -- the bits of the result -- must not depend on the layout).  DETR_HIP_SLAB_TS=2: row-major.
static bool gemm_slab_ts(const detr_gemm_desc *d, int split, int batch, GemmTile tile, int &bm, int &bn) {
    const TileDims t = gemm_tile_dims(d->compute == 1, tile);
    bm = t.bm; bn = t.bn;
    return t.slab_ts && split > 1 && batch == 1 && d->N % 4 == 0 && d->ldc % 4 == 0 && aligned16(d->C) && (!d->scale || aligned16(d->scale)) &&
           tune(T_SLAB_TS) != 2;
}
// The descriptor half of the ring weight gradient's predicate (gemm_ring.h: gemm_ring_wgrad_kernel): MN-contiguous bf16 operands in 16-byte
// requests, no fused row sums; DETR_HIP_GEMM_RING = 2 / 3 switch the form off.  gemm_route adds what the plan decides (tile, split, slabs).
static bool gemm_ring_wgrad_operands(const detr_gemm_desc *d) {
    return d->compute == 1 && d->a_dtype == 1 && d->b_dtype == 1 && !d->a_kcontig && !d->b_kcontig && !d->rowsum_a && d->M % 8 == 0 &&
           d->N % 8 == 0 && d->lda % 8 == 0 && d->ldb % 8 == 0 && aligned16(d->A) && aligned16(d->B) && tune(T_GEMM_RING) != 2 &&
           tune(T_GEMM_RING) != 3;
}

// compute = 2 (f32x3): the shapes whose products go through the split kernel (gemm_core.h: mma_ktile_split3).  The operand split is VALU work
// per fragment, so the narrow (N <= 64: 0.77x) and the short-K (K <= 128: 0.92-0.96x) 1x1-convolution GEMMs and the 64-row weight gradients
// (0.85x) keep the exact kernel (scripts/micro_split3.py, profiles/r06_micro_split3.txt) -- both are fp32-accurate, the mode only decides
// which matrix instruction computes the products.  DETR_HIP_SPLIT3_ALL=1: every shape (tests).
static bool gemm_x3_shape(int M, int N, int K) { return N >= 128 && K >= 256 && M >= 128; }
static bool gemm_split3_shape(const detr_gemm_desc *d) {
    return d->compute == 2 && d->N > 32 && (tune(T_SPLIT3_ALL) == 1 || gemm_x3_shape(d->M, d->N, d->K));
}
// compute = 1: the split-K shapes that run on 128 x 128 tiles (gemm_pick_tile) and are planned for them (gemm_split_plan).
// round 3, cold-cache sweeps (scripts/micro_wgrad.py, micro_gemm.py --cold; profiles/r03_micro_*): the layer4 weight
// gradients (M, N >= 512, K = 8400) gain 15-25 % on 128x128 tiles (512x2048: 64 -> 53 us, 1024x2048: 109 -> 80), and so do
// the wide K = 512 GEMMs of layer3's first block (M33600 N1024: 100 -> 89 us, with residual + mask 163 -> 151)
// round 4 (scripts/experiments/tile_force.sh): the encoder's FFN weight-gradient pair (256 x 2048 and 2048 x 256 outputs, K = 8400)
// 54.7 us as one grouped launch of 64x64 tiles -> 45.3 us as two launches of 128x128 tiles
static bool gemm_big_split(int M, int N, int K) {
    return (N >= 128 && K >= 16384) || (M >= 512 && N >= 512 && K >= 4096) || (K >= 4096 && ((M >= 256 && N >= 2048) || (M >= 2048 && N >= 256)));
}
static GemmTile gemm_pick_tile(const detr_gemm_desc *d, int split, int batch) {
    const bool bf16c = d->compute == 1;
    const int force = tune(T_GEMM_TILE);     // tuning hook (scripts/tune_gemm.py); 0 = heuristic
    GemmTile tile = TILE_64x64;
    if (bf16c) {
        // measured (profiles/tune_bf16_r1c.txt, buffer-descriptor loaders + transpose-read LDS images): the 64x64 tile
        // (7-8 waves/SIMD) wins every non-split shape and the short reductions; 128x128 (3 waves/SIMD, 4x the operand
        // reuse) pays only for the long split-K weight gradients (K >= 16384, N >= 128) and for unsplit K >= 1024 GEMMs
        // that still fill the chip with 128x128 tiles (M33600 N256 K1024: 54 vs 60 us)
        const long long t128 = (long long)cdiv(d->M, 128) * cdiv(d->N, 128) * batch;
        const bool big_split = gemm_big_split(d->M, d->N, d->K);
        // round 4 (scripts/experiments/tile_shapes.py, every unsplit shape of the step on every tile): the rules hold within +-5 % except
        // M133600 N256 K512 (layer2's projection shortcut and its input gradient): 81.9 us on 64x64 tiles, 71.1 on 128x128
        const bool big_plain = (d->K >= 1024 && t128 >= 512) || (d->K >= 512 && d->N >= 512 && t128 >= 1024) ||
                               (d->K >= 512 && d->N >= 256 && t128 >= 2048);
        const bool small = (split > 1) ? !big_split : !big_plain;
        if (force == 2) tile = TILE_128x64;
        else if (force == 5) tile = TILE_WIDE;
        else if (force == 3 || (force == 0 && small)) tile = TILE_64x64;
        else if (force == 0 && split > 1 && d->M <= 64) tile = TILE_WIDE;     // 64 output rows: half of a 128-row tile would be padding (M64 N256 K534400: 84 -> 74 us)
        else tile = TILE_128x128;
        // ring weight gradient (gemm_ring.h) on wider tiles -- experiment hook DETR_HIP_RING_WTILE: 1 = 128 x 256, 2 = 256 x 128
        // (the FULL predicate of the ring weight gradient in gemm_route -- ADVICE r5: a tile only that kernel has must not be handed to a
        //  launch the kernel will not take, nor size the slab scratch for it: the operands' half, and a split, unbatched output that can take
        //  tile-ordered slabs; whether the workspace holds them is checked again there)
        int bm, bn;
        if (tile == TILE_128x128 && gemm_ring_wgrad_operands(d) && gemm_slab_ts(d, split, batch, tile, bm, bn)) {
            const int wt = tune(T_RING_WTILE);
            if (wt == 1 && d->N >= 256) tile = TILE_RING_128x256;
            else if (wt == 2 && d->M >= 256) tile = TILE_RING_256x128;
        }
    } else if (gemm_split3_shape(d)) {
        // f32x3 (mma_ktile_split3): a wave's operand split costs VALU time per FRAGMENT, its 6 MFMAs per fragment PAIR -- 64 x 64 wave
        // tiles (128 x 128 workgroup tiles) are matrix-pipe bound where 32 x 32 ones are VALU bound; small grids keep the 64 x 64 tile
        const long long t128 = (long long)cdiv(d->M, 128) * cdiv(d->N, 128) * batch * split;
        if (force == 1 || (force == 0 && t128 >= x3_t128_threshold())) tile = TILE_128x128;
        else if (force == 2) tile = TILE_128x64;        // (128 x 64: three workgroups per CU)
        else tile = TILE_64x64;
        // Tile-count quantisation (profiles/r06_ab_results.txt #9): two 128 x 128 workgroups fit a CU = 512 slots, and M33600 N256 is 526 tiles -- two
        // rounds, the second with 14 workgroups.  192 x 128 tiles (tile id 8: 1.5 x the work per workgroup, the same two per CU; K-contiguous A,
        // unsplit, no fused row sums) take the GEMM when they need fewer rounds x 1.5.  DETR_HIP_X3_T192 = 2: never, 1: wherever eligible.
        if (tile == TILE_128x128 && force == 0 && split == 1 && batch == 1 && d->a_kcontig && !d->rowsum_a && tune(T_X3_T192) != 2) {
            const long long t192 = (long long)cdiv(d->M, 192) * cdiv(d->N, 128);
            if (tune(T_X3_T192) == 1 || x3_t192_fewer_rounds(t128, t192)) tile = TILE_X3_192x128;
        }
        // 128 x 64 tiles (three workgroups per CU = 768 slots) where the 128 x 128 grid is just over a whole number of rounds (M8400 N2048: 1056 tiles = 2.06
        // rounds: 142 -> 135 us, 88.7 -> 77.9 us at K = 256) or a short-K grid fills half the chip (M8400 N512 K256: 34.7 -> 30.4 us)
        if (tile == TILE_128x128 && force == 0 && split == 1 && batch == 1 && tune(T_X3_T192) != 2 && d->M >= 4096) {
            const long long over = t128 % 512;
            if ((t128 > 512 && over > 0 && over <= 128) || (t128 <= 384 && d->K <= 512)) tile = TILE_128x64;
        }
    } else if (force == 1) tile = TILE_128x128;
    else if (force == 2) tile = TILE_128x64;
    else if (force == 3) tile = TILE_64x64;
    else if (force == 4) tile = TILE_128x32;
    else if (force == 5) tile = TILE_WIDE;
    else if (force == 6) tile = TILE_256x64;
    else if (d->N <= 32) tile = TILE_128x32;
    else tile = TILE_64x64;      // measured (profiles/tune_r1.txt): 64x64 (8 waves/SIMD) beats 128x64 by 2-10 % and 128x128 by 15-50 % in fp32
    return tile;
}
// The split a reduction-heavy GEMM (a weight gradient) should ask for (detr_gemm_desc.split_k), so that enough workgroups exist to fill
// 256 CUs on the tile gemm_pick_tile gives that split: the same predicates decide both.  Workgroup targets (A/B hooks): 128x128 tiles
// DETR_HIP_SPLIT_TARGET, 512 -> 256 measured -0.23 ms per step on the same box (half the partial slabs to write and reduce;
// scripts/micro_wgrad.py shows the same 3-7 % per launch with cold caches); 64x64 tiles DETR_HIP_SPLIT_TARGET64; f32x3 on 128x128
// tiles DETR_HIP_X3_SPLIT_TARGET (negative: the 64x64 plan).  DETR_HIP_SPLIT3_ALL does not enter the plan.
static int gemm_split_plan(int M, int N, int K, int compute, int max_split) {
    const long long target128 = tune(T_SPLIT_TARGET) ? tune(T_SPLIT_TARGET) : 256;
    const long long target64 = tune(T_SPLIT_TARGET64) ? tune(T_SPLIT_TARGET64) : 1024;
    const long long target_x3 = tune(T_X3_SPLIT_TARGET) ? tune(T_X3_SPLIT_TARGET) : 512;
    const long long t128 = (long long)cdiv(M, 128) * cdiv(N, 128), most = max_split;
    if (compute == 1 && gemm_big_split(M, N, K)) {                               // 128x128 tiles
        const long long ktiles = cdiv(K, 32);
        return (int)std::max(1LL, std::min({std::max(1LL, target128 / t128), most, ktiles >= 16 ? ktiles / 8 : 1LL}));
    }
    if (compute == 2 && target_x3 > 0 && gemm_x3_shape(M, N, K)) {
        // f32x3 (gemm_x3.h): 128 x 128 tiles, two workgroups per CU = 512 slots; the 64 x 64 plan below left e.g. the 256 x 1024 weight gradient of layer3
        // with 16 tiles x 16 splits = 256 workgroups, half a round of single workgroups per CU (round 6)
        const long long ktiles = cdiv(K, 32);
        const long long cap = ktiles >= 64 ? ktiles / 8 : std::max(1LL, ktiles / 4);
        const long long s128 = std::max(1LL, std::min({target_x3 / t128, most, cap}));
        if (t128 * s128 >= x3_t128_threshold()) return (int)s128;                // (gemm_pick_tile: 128 x 128 tiles from that many of them on)
    }
    // 64x64 tiles (fp32 always; bf16 for small outputs, see gemm_pick_tile): ~1024 workgroups measured best
    const long long tiles = (long long)cdiv(M, 64) * cdiv(N, 64);
    const long long want = std::max(1LL, target64 / tiles);
    const long long ktiles = cdiv(K, compute == 1 ? 32 : 16);
    const long long cap = ktiles >= 64 ? ktiles / 8 : ktiles / 4;                // short reductions: 4 k-tiles per split are enough
    return (int)std::max(1LL, std::min({want, most, cap}));
}
extern "C" int32_t detr_hip_gemm_split_plan(int32_t M, int32_t N, int32_t K, int32_t compute, int32_t max_split) {
    DETR_REQUIRE(M > 0 && N > 0 && K > 0, "gemm_split_plan: bad shape M=%d N=%d K=%d", M, N, K);
    DETR_REQUIRE(compute >= 0 && compute <= 2, "gemm_split_plan: compute %d (0 = fp32, 1 = bf16, 2 = f32x3)", compute);
    DETR_REQUIRE(max_split >= 1, "gemm_split_plan: max_split %d < 1", max_split);
    return gemm_split_plan(M, N, K, compute, max_split);
}
// split count a GEMM really runs with: no empty splits (recomputed from the K tiles each split gets)
static int gemm_effective_split(const detr_gemm_desc *d) {
    int split = d->split_k > 1 ? d->split_k : 1;
    if (split > 1) {
        const int nkt = cdiv(d->K, (d->compute == 1 || gemm_split3_shape(d)) ? BF_BK : GEMM_BK);      // (the f32x3 kernel walks 32-deep K tiles)
        const int per = cdiv(nkt, split);
        split = cdiv(nkt, per);
    }
    return split;
}

extern "C" int64_t detr_hip_workspace_bytes_gemm(const detr_gemm_desc *d) {
    if (!d || d->M <= 0 || d->N <= 0 || d->K <= 0) return -1;
    const int batch = d->batch > 0 ? d->batch : 1;
    const int split = gemm_effective_split(d);
    if (split <= 1 || batch != 1) return 0;          // (batched split-K accumulates with atomics: no scratch)
    int bm, bn;
    int64_t part = (int64_t)d->M * d->N;
    if (gemm_slab_ts(d, split, batch, gemm_pick_tile(d, split, batch), bm, bn))      // tile-ordered slabs: whole tiles
        part = (int64_t)cdiv(d->M, bm) * cdiv(d->N, bn) * bm * bn;
    return (int64_t)split * (part + (d->rowsum_a ? d->M : 0)) * 4;
}

static int gemm_prepare(const detr_gemm_desc *d, GemmPlan &p) {
    DETR_REQUIRE(d != nullptr, "gemm: null descriptor");
    DETR_REQUIRE(d->M > 0 && d->N > 0 && d->K > 0, "gemm: bad shape M=%d N=%d K=%d", d->M, d->N, d->K);
    DETR_REQUIRE(d->A && d->B && d->C, "gemm: null operand");
    // the documented values only: any other one used to mean "exact fp32" / "fp32 storage" without a word
    DETR_REQUIRE(d->compute >= 0 && d->compute <= 2, "gemm: compute %d (0 = fp32, 1 = bf16, 2 = f32x3)", d->compute);
    DETR_REQUIRE((d->a_dtype == 0 || d->a_dtype == 1) && (d->b_dtype == 0 || d->b_dtype == 1) && (d->c_dtype == 0 || d->c_dtype == 1) &&
                 (d->r_dtype == 0 || d->r_dtype == 1) && d->m_dtype >= 0 && d->m_dtype <= 2,
                 "gemm: storage types a %d b %d c %d r %d (0 = fp32, 1 = bf16), m %d (2 = bit-packed as well)", d->a_dtype, d->b_dtype, d->c_dtype,
                 d->r_dtype, d->m_dtype);
    // bf16 storage is bf16 compute only (include/detr_hip.h): the exact and the f32x3 kernels are instantiated for fp32 tensors
    DETR_REQUIRE(d->compute == 1 || (d->c_dtype == 0 && d->r_dtype == 0 && d->m_dtype == 0),
                 "gemm: bf16 / bit-packed C, residual and mask need compute = bf16 (compute %d: c %d r %d m %d)", d->compute, d->c_dtype, d->r_dtype,
                 d->m_dtype);
    const int batch = d->batch > 0 ? d->batch : 1;
    const int inner = d->batch_inner > 0 ? d->batch_inner : 1;
    const bool bf16c = d->compute == 1;
    int split = gemm_effective_split(d);
    if (split > 1) {
        DETR_REQUIRE(!d->bias && !d->residual && !d->mask && d->act == 0,
                     "gemm: split_k allows only scale/alpha in the epilogue");
    }
    {   // operands are addressed through 32-bit buffer offsets (gemm_core.h BufSrc)
        const long long ea = d->a_kcontig ? (long long)(d->M - 1) * d->lda + d->K : (long long)(d->K - 1) * d->lda + d->M;
        const long long eb = d->b_kcontig ? (long long)(d->N - 1) * d->ldb + d->K : (long long)(d->K - 1) * d->ldb + d->N;
        DETR_REQUIRE(d->b_dtype == 0 || (d->b_dtype == 1 && bf16c && batch == 1 && aligned16(d->B) && d->ldb % 8 == 0 &&
                                         (d->b_kcontig ? d->K % 8 == 0 : d->N % 4 == 0)),
                     "gemm: a bf16 B operand needs compute = bf16, batch 1, 16-byte alignment, ldb %% 8 == 0 and K %% 8 (N %% 4) == 0");
        DETR_REQUIRE(ea * 4 <= BUF_MAX_BYTES && eb * 4 <= BUF_MAX_BYTES, "gemm: an operand spans more than 4 GB");
        DETR_REQUIRE(d->a_dtype == 0 || (d->a_dtype == 1 && bf16c && batch == 1 && ((uintptr_t)d->A % 16 == 0) &&
                                         (d->a_kcontig ? (d->lda % 8 == 0 && d->K % 8 == 0) : (d->lda % 4 == 0 && d->M % 4 == 0))),
                     "gemm: a bf16 A operand needs compute = bf16, batch 1, 16-byte alignment and K %% 8 (M %% 4) == 0");
        DETR_REQUIRE((d->c_dtype == 0 && d->r_dtype == 0 && d->m_dtype == 0) || (batch == 1 && split == 1),
                     "gemm: bf16 C / residual / mask need batch 1 and no split-K");
    }
    if (d->rowsum_a) DETR_REQUIRE(!d->a_kcontig && batch == 1, "gemm: rowsum_a needs an MN-contiguous A operand and batch == 1");
    DETR_REQUIRE((long long)batch * split <= 65535, "gemm: batch*split_k=%lld exceeds grid.z", (long long)batch * split);

    GemmArgs &g = p.g;
    g.M = d->M; g.N = d->N; g.K = d->K;
    g.A = d->A; g.lda = d->lda;
    g.B = d->B; g.ldb = d->ldb;
    g.C = d->C; g.ldc = d->ldc;
    g.batch_inner = inner;
    g.sA0 = d->sA0; g.sA1 = d->sA1; g.sB0 = d->sB0; g.sB1 = d->sB1; g.sC0 = d->sC0; g.sC1 = d->sC1;
    g.split_k = split;
    g.part_stride = 0;
    g.tiles_m = g.tiles_n = 0;
    auto strides_ok = [](long long ld, long long s0, long long s1) { return (ld % 4 == 0) && (s0 % 4 == 0) && (s1 % 4 == 0); };
    // vec: float4 tile loads; the extent along the contiguous axis must be a multiple of 4 so that a float4 is
    // entirely inside or outside the operand (branch-free guarded loads, gemm_core.h ld4_sel)
    g.a_vec = aligned16(d->A) && strides_ok(d->lda, d->sA0, d->sA1) && ((d->a_kcontig ? d->K : d->M) % 4 == 0);
    g.b_vec = aligned16(d->B) && strides_ok(d->ldb, d->sB0, d->sB1) && ((d->b_kcontig ? d->K : d->N) % 4 == 0);
    g.e.alpha = d->alpha;
    g.e.scale = d->scale;
    g.e.bias = d->bias;
    g.e.residual = d->residual; g.e.ldr = d->ldr;
    g.e.mask = d->mask; g.e.ldmask = d->ldmask;
    g.e.act = d->act;
    g.e.atomic = split > 1 ? 1 : 0;
    g.e.drop_scale = 0.0f; g.e.drop_thresh = 0; g.e.drop_seed = 0;
    if (d->dropout_p > 0.0f) {
        DETR_REQUIRE(d->dropout_p < 1.0f && split == 1 && batch == 1, "gemm: dropout needs 0<p<1, no split-K, no batch");
        g.e.drop_scale = 1.0f / (1.0f - d->dropout_p);
        g.e.drop_thresh = drop_thresh16(d->dropout_p);
        g.e.drop_seed = d->dropout_seed;
        g.e.drop_step = d->dropout_step;
    }
    g.e.c16 = d->c_dtype == 1; g.e.r16 = d->r_dtype == 1;
    g.e.m16 = (d->m_dtype == 1 || d->m_dtype == 2) ? d->m_dtype : 0;       // 2: bit-packed mask (one byte per 8 columns, ldmask in bytes)
    g.e.mbits_out = d->maskbits_out; g.e.ld_mbits_out = d->ld_maskbits_out;
    const bool bits_in = d->mask && d->m_dtype == 2, bits_out = d->maskbits_out != nullptr;
    g.e.vec = aligned16(d->C) && (d->ldc % 4 == 0) && (d->sC0 % 4 == 0) && (d->sC1 % 4 == 0) &&
              (!d->scale || aligned16(d->scale)) && (!d->bias || aligned16(d->bias)) &&
              (!d->residual || (aligned16(d->residual) && d->ldr % 4 == 0)) &&
              (!d->mask || bits_in || (aligned16(d->mask) && d->ldmask % 4 == 0));

    // all-bf16 epilogue streams, 16-byte rows: the 8-columns-per-lane epilogue (gemm_core.h epilogue_wide16); DETR_HIP_EPI_WIDE=2: off
    g.e.wide16 = g.e.c16 && split == 1 && batch == 1 && (!d->residual || g.e.r16) && (!d->mask || g.e.m16) && d->N % 8 == 0 &&
                 d->ldc % 8 == 0 && aligned16(d->C) && (!d->residual || (d->ldr % 8 == 0 && aligned16(d->residual))) &&
                 (!d->mask || bits_in || (d->ldmask % 8 == 0 && aligned16(d->mask))) && (!d->scale || aligned16(d->scale)) &&
                 (!d->bias || aligned16(d->bias)) && (tune(T_EPI_WIDE) != 2 || bits_in || bits_out || d->res_sub_w > 0);
    // bit-packed masks live in the all-bf16 epilogues (8 columns per lane = one byte) of the tile engine and of the streaming kernel
    DETR_REQUIRE(!(bits_in || bits_out) || (bf16c && g.e.wide16 && (!bits_in || d->ldmask >= d->N / 8) && (!bits_out || d->ld_maskbits_out >= d->N / 8)),
                 "gemm: bit-packed masks need bf16 C / residual, N %% 8 == 0, 16-byte aligned rows, no split-K / batch, and a row pitch >= N / 8 bytes");
    // the residual row map lives in the same epilogues (a launch that reaches any other one must fail, never ignore the map)
    if (d->res_sub_h || d->res_sub_w || d->res_sub_ho || d->res_sub_wo) {
        DETR_REQUIRE(d->res_sub_h > 0 && d->res_sub_w > 0 && d->res_sub_ho == (d->res_sub_h + 1) / 2 && d->res_sub_wo == (d->res_sub_w + 1) / 2 &&
                     d->M % ((long long)d->res_sub_h * d->res_sub_w) == 0,
                     "gemm: residual row map: M must be whole res_sub_h x res_sub_w maps and res_sub_ho / res_sub_wo their halves, rounded up");
        DETR_REQUIRE(d->residual && bf16c && g.e.wide16 && !d->ln_y,
                     "gemm: a residual row map needs a bf16 residual and bf16 C (compute = bf16), N %% 8 == 0, 16-byte aligned rows, no split-K / batch / LayerNorm");
        g.e.res_sub_h = d->res_sub_h; g.e.res_sub_w = d->res_sub_w; g.e.res_sub_ho = d->res_sub_ho; g.e.res_sub_wo = d->res_sub_wo;
    }

    const bool ak = d->a_kcontig != 0, bk = d->b_kcontig != 0;
    DETR_REQUIRE(!(bf16c && d->a_dtype == 1 && !ak) || (d->lda % 8 == 0 && d->M % 8 == 0 && aligned16(d->A)),
                 "gemm: an M-contiguous bf16 A operand needs lda %% 8 == 0, M %% 8 == 0 and a 16-byte aligned base (16-byte requests)");
    DETR_REQUIRE(!(bf16c && d->b_dtype == 1 && !bk) || (d->ldb % 8 == 0 && d->N % 8 == 0 && aligned16(d->B)),
                 "gemm: an N-contiguous bf16 B operand needs ldb %% 8 == 0, N %% 8 == 0 and a 16-byte aligned base (16-byte requests)");
    const GemmTile tile = gemm_pick_tile(d, split, batch);
    // deterministic split-K: partial slabs in the caller's workspace.  Tile-ordered slabs (whole tiles: a little more scratch than
    // split*M*N -- detr_hip_workspace_bytes_gemm reports it) when the workspace holds them, row-major slabs when it only holds
    // the documented split*M*N floats, fp32 atomics without a workspace.
    long long part = (long long)d->M * d->N;
    int ts_bm = 0, ts_bn = 0;
    const long long rs_extra = d->rowsum_a ? d->M : 0;
    bool ts = gemm_slab_ts(d, split, batch, tile, ts_bm, ts_bn);
    const long long part_ts = ts ? (long long)cdiv(d->M, ts_bm) * cdiv(d->N, ts_bn) * ts_bm * ts_bn : 0;
    const bool ws_ok = split > 1 && batch == 1 && d->workspace && aligned16(d->workspace);
    if (ts && !(ws_ok && d->workspace_bytes >= (long long)split * (part_ts + rs_extra) * 4)) ts = false;
    if (ts) part = part_ts;
    const bool partial = ws_ok && d->workspace_bytes >= (long long)split * (part + rs_extra) * 4;
    DETR_REQUIRE(!(d->rowsum_a && split > 1 && !partial), "gemm: rowsum_a with split_k needs the workspace path");
    g.rowsum = d->rowsum_a;
    g.rowsum_alpha = d->rowsum_alpha;
    g.rowsum_partial = 0;
    g.b16 = d->b_dtype == 1;
    g.a16 = d->a_dtype == 1;
    g.split_xcd = tune(T_SPLIT_XCD) != 2;
    g.slab_ts = 0;
    p.ts_bm = p.ts_bn = 0; p.ts_tn = 1;
    EpiArgs final_e = g.e;
    if (partial) {      // plain stores of the partial tiles, reduced by a second launch
        g.C = d->workspace;
        g.ldc = d->N;
        g.part_stride = part;
        g.e.alpha = 1.0f;
        g.e.scale = nullptr;
        g.e.atomic = 0;
        g.e.vec = (d->N % 4 == 0);
        if (ts) {
            g.slab_ts = 1;
            p.ts_bm = ts_bm; p.ts_bn = ts_bn; p.ts_tn = cdiv(d->N, ts_bn);
        }
        if (d->rowsum_a) {       // partial row sums go behind the tile slabs
            g.rowsum = d->workspace + (long long)split * part;
            g.rowsum_partial = 1;
        }
    }
    // 64-deep K tiles (all-bf16 operands, tiles 0 / 1): DETR_HIP_GEMM_K64 = 0 rule below, 1 every eligible GEMM, 2 never.
    // Measured (scripts/micro_gemm.py, profiles/r03_micro_gemm_k64.txt): 64x64 tiles gain 10-23 % from K >= 512 per split on (M8400
    // N512 K2048: 47.0 -> 39.2 us, M800 N256 K2048 cold: 28.0 -> 21.6); UNSPLIT 128x128 tiles lose 20-35 % (72 KB of LDS: two
    // workgroups per CU instead of three -- M33600 N1024 K512: 73 -> 92 us), split ones gain 0-7 % (cold: 82.0 -> 76.1 us)
    {
        const int k64 = tune(T_GEMM_K64);
        const int per_split = cdiv(d->K, split);
        p.deep = bf16c && g.a16 && g.b16 && (tile == TILE_64x64 || tile == TILE_128x128) && k64 != 2 &&
                 (k64 == 1 || (per_split >= 512 && (tile == TILE_64x64 || split > 1)));
    }
    p.batch = batch; p.split = split; p.ak = ak; p.bk = bk; p.bf16c = bf16c; p.partial = partial; p.tile = tile;
    p.split3 = gemm_split3_shape(d) && (tile == TILE_64x64 || tile == TILE_128x128 || tile == TILE_128x64 || tile == TILE_X3_192x128);
    p.part = part; p.final_e = final_e; p.d = d;
    return 0;
}

// The streaming kernel (gemm_stream.h) takes the short-K, tall GEMMs whose operands, output, residual and mask are all
// bf16 in memory: the layer1 / layer2 1x1 convolutions and their input gradients.  DETR_HIP_GEMM_STREAM=2 disables it.
static bool gemm_stream_eligible(const GemmPlan &p) {
    const detr_gemm_desc *d = p.d;
    const GemmArgs &g = p.g;
    if (!(p.bf16c && g.a16 && g.b16 && g.e.c16 && p.ak && p.batch == 1 && p.split == 1 && !g.rowsum)) return false;
    // M >= 16384: the backbone's 1x1 convolutions; the transformer's K = 256 FFN GEMMs (M = B*L = 8400: linear1 forward with its
    // fused dropout, the input gradient of linear2 with alpha = 1/(1-p) and the ReLU / dropout mask) take it from M >= 4096
    const bool ext = d->alpha != 1.0f || d->dropout_p > 0.0f;
    if (!((d->K == 64 || d->K == 128 || d->K == 256) && d->N % 64 == 0 && d->M >= ((d->K == 256 && d->N >= 1024) ? 4096 : 16384))) return false;
    if (d->scale || (ext && d->K != 256) || !(d->act == 0 || d->act == 1)) return false;
    if (d->residual && !(g.e.r16 && d->ldr % 8 == 0 && aligned16(d->residual))) return false;
    if (d->mask && g.e.m16 != 2 && !(g.e.m16 && d->ldmask % 8 == 0 && aligned16(d->mask))) return false;
    if (!(d->lda % 8 == 0 && d->ldb % 8 == 0 && d->ldc % 8 == 0 && aligned16(d->A) && aligned16(d->B) && aligned16(d->C))) return false;
    const long long ldm_eff = g.e.m16 == 2 ? 0 : d->ldmask;
    // (a mapped residual is the smaller compact tensor: bounding it by the M full-resolution rows is the safe side)
    long long pitch = d->ldr > ldm_eff ? d->ldr : ldm_eff;
    if (d->ldc > pitch) pitch = d->ldc;             // C is stored through a buffer descriptor as well (32-bit byte offsets)
    const long long span = (long long)(d->M - 1) * pitch + d->N;
    if (span * 2 > BUF_MAX_BYTES) return false;
    // mask bits OUT: the kernel is instantiated for the form that produces them in the step (block outputs: [k][n] weights + residual)
    if (d->maskbits_out && (p.bk || !d->residual || d->mask || ext)) return false;
    return tune(T_GEMM_STREAM) != 2;
}

static void gemm_stream_launch(const GemmPlan &p, hipStream_t s) {
    const detr_gemm_desc *d = p.d;
    StreamArgs a;
    a.M = d->M; a.N = d->N;
    a.A = reinterpret_cast<const unsigned short *>(d->A); a.lda = d->lda;
    a.B = reinterpret_cast<const unsigned short *>(d->B); a.ldb = d->ldb;
    a.C = reinterpret_cast<unsigned short *>(d->C); a.ldc = d->ldc;
    a.res = reinterpret_cast<const unsigned short *>(d->residual); a.ldr = d->ldr;
    a.mask = reinterpret_cast<const unsigned short *>(d->mask); a.ldm = d->ldmask;
    a.mbits_out = d->maskbits_out; a.ld_mbits = d->ld_maskbits_out;
    a.bias = d->bias;
    a.act = d->act;
    a.alpha = d->alpha;
    a.drop_scale = p.g.e.drop_scale; a.drop_thresh = p.g.e.drop_thresh; a.drop_seed = p.g.e.drop_seed; a.drop_step = p.g.e.drop_step;
    a.n_tiles = a.row_tiles = a.q = 0;
    a.res_sub_h = p.g.e.res_sub_h; a.res_sub_w = p.g.e.res_sub_w; a.res_sub_ho = p.g.e.res_sub_ho; a.res_sub_wo = p.g.e.res_sub_wo;
    a.res_rows = a.res_sub_w > 0 ? (long long)d->M / ((long long)a.res_sub_h * a.res_sub_w) * a.res_sub_ho * a.res_sub_wo : 0;
    const bool mb = d->mask && d->m_dtype == 2;
    if (d->K == 64) launch_gemm_stream<64>(a, p.bk, s, mb);
    else if (d->K == 128) launch_gemm_stream<128>(a, p.bk, s, mb);
    else launch_gemm_stream<256>(a, p.bk, s, mb);
}

// GEMM with the LayerNorm of its output rows fused (detr_gemm_desc.ln_y; gemm_core.h: epilogue_ln): row-complete 32 x 256 tiles
static int gemm_ln_launch(const GemmPlan &p, hipStream_t s) {
    const detr_gemm_desc *d = p.d;
    const GemmArgs &g0 = p.g;
    DETR_REQUIRE(p.bf16c && d->N == LN_TILE_N && d->ldc == LN_TILE_N && p.ak && p.bk && g0.b16 && p.batch == 1 && p.split == 1,
                 "gemm + LayerNorm: needs compute = 1, N = ldc = 256, k-contiguous A and bf16 k-contiguous B, no batch / split_k");
    DETR_REQUIRE(d->act == 0 && !d->scale && !d->mask && !g0.e.c16 && !g0.e.r16 && !d->rowsum_a && !d->maskbits_out && d->K % 8 == 0,
                 "gemm + LayerNorm: epilogue is bias, alpha, dropout and an fp32 residual only (K %% 8 == 0)");
    DETR_REQUIRE(d->ln_gamma && d->ln_beta && d->ln_mean && d->ln_rstd && (!d->ln_y2 || (d->ln_add && d->ln_add_rows > 0)),
                 "gemm + LayerNorm: gamma, beta, mean, rstd are required (and add / add_rows with y2)");
    DETR_REQUIRE((!d->residual || (d->ldr % 4 == 0 && aligned16(d->residual))) && aligned16(d->C) && aligned16(d->ln_y) &&
                 (!d->bias || aligned16(d->bias)) && aligned16(d->ln_gamma) && aligned16(d->ln_beta) &&
                 (!d->ln_y2 || (aligned16(d->ln_y2) && aligned16(d->ln_add))) && (!d->ln_y16 || aligned16(d->ln_y16)),
                 "gemm + LayerNorm: rows must be 16-byte aligned");
    GemmArgs a = g0;
    a.tiles_m = cdiv(d->M, LN_TILE_M);
    a.tiles_n = 1;
    a.ln.gamma = d->ln_gamma; a.ln.beta = d->ln_beta; a.ln.y = d->ln_y; a.ln.mean = d->ln_mean; a.ln.rstd = d->ln_rstd;
    a.ln.add = d->ln_add; a.ln.add_rows = d->ln_add_rows; a.ln.y2 = d->ln_y2; a.ln.y16 = d->ln_y16; a.ln.eps = d->ln_eps;
    const dim3 grid((unsigned)a.tiles_m), block(GEMM_THREADS);
    if (g0.a16) hipLaunchKernelGGL(gemm_bf16c_ln_kernel<true>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(gemm_bf16c_ln_kernel<false>, grid, block, 0, s, a);
    DETR_LAUNCH_CHECK("gemm + LayerNorm");
    if (d->defer_out) d->defer_out->splits = 0;
    return 0;
}

// The ring kernel (gemm_ring.h) takes the tall unsplit GEMMs whose operands are both bf16 in memory with a K-contiguous A: the
// K >= 512 1x1 convolutions of layer2-layer4 (forward and input gradient) and the encoder's FFN at M = B*L.  DETR_HIP_GEMM_RING=2
// disables it, =1 takes every eligible shape (tests: small M as well).
static bool gemm_ring_eligible(const GemmPlan &p, RingPlan &rp) {
    const detr_gemm_desc *d = p.d;
    const GemmArgs &g = p.g;
    const int mode = tune(T_GEMM_RING);
    if (mode == 2) return false;
    if (!(p.bf16c && g.a16 && g.b16 && p.ak && p.batch == 1 && p.split == 1 && !g.rowsum && !d->ln_y)) return false;
    if (!(d->K % RING_BK == 0 && d->K >= 2 * RING_BK && d->N >= 128 && d->N % 8 == 0 && d->lda % 8 == 0 && d->ldb % 8 == 0 && aligned16(d->A) &&
          aligned16(d->B))) return false;
    // which shapes (scripts/micro_gemm.py / micro_ring.py, profiles/r05_micro_gemm_ring.txt): every tall K >= 512 GEMM (-15 .. -30 % against the
    // 4-wave engine); the decoder's 800-row K = 2048 FFN GEMMs (15.2 -> 11.0 us); and, in front of the streaming kernel, two K = 256
    // families it runs faster than that kernel does: layer3's N = 1024 block outputs / input gradients (M33600: 51.5 -> 45.7,
    // 62.5 -> 51.8 us) and the encoder FFN's input gradient with [k][n] weights (M8400 N2048: 31.6 -> 26.6 us)
    const bool tall = d->M >= 4096 && d->K >= 512;
    const bool dec_ffn = d->M >= 512 && d->K >= 1024;
    const bool k256 = d->K == 256 && d->N >= 1024 && (d->M >= 16384 || (d->M >= 4096 && !p.bk));
    if (mode != 1 && !(tall || dec_ffn || k256)) return false;
    return gemm_ring_plan(d->M, d->N, d->K, rp);
}

// fp32 form (the exact-f32 parity mode): fp32 operands, K-contiguous A, unsplit; DETR_HIP_GEMM_RING as above
static bool gemm_ring_f32_eligible(const GemmPlan &p, RingPlan &rp) {
    const detr_gemm_desc *d = p.d;
    const GemmArgs &g = p.g;
    const int mode = tune(T_GEMM_RING);
    if (mode == 2) return false;
    if (p.bf16c || p.split3 || g.a16 || g.b16 || !p.ak || p.batch != 1 || p.split != 1 || g.rowsum || d->ln_y) return false;
    if (d->c_dtype || d->r_dtype || d->m_dtype) return false;
    if (!(d->K % 32 == 0 && d->K >= 64 && d->N >= 128 && d->lda % 4 == 0 && d->ldb % 4 == 0 && aligned16(d->A) && aligned16(d->B) &&
          (p.bk || d->N % 4 == 0))) return false;
    // measured (scripts/micro_ring.py, RING_F32=1, second-pass columns -- the first timings of a process run at a lower clock): -3 .. -9 % on
    // the backbone's M >= 33600 shapes, +-0 .. +3 % on the M = 8400 ones: the fp32 MFMA kernels sit at ~0.6 of the nominal peak whatever
    // the structure (NOTEBOOK 4c)
    if (mode != 1 && !(d->M >= 16384)) return false;
    return gemm_ring_f32_plan(d->M, d->N, d->K, rp);
}

// Split-K weight gradients of the backbone's 1x1 convolutions on 128 x 128 tiles (128 x 256 / 256 x 128: DETR_HIP_RING_WTILE): the 8-wave
// ring form (gemm_ring.h; bit-identical slabs).  Needs the tile-ordered slabs, that is a workspace of detr_hip_workspace_bytes_gemm bytes.
static bool gemm_ring_wgrad_eligible(const GemmPlan &p) {
    return (p.tile == TILE_128x128 || p.tile == TILE_RING_128x256 || p.tile == TILE_RING_256x128) && p.batch == 1 && p.split > 1 &&
           p.g.slab_ts && gemm_ring_wgrad_operands(p.d);
}

// The kernel family of a prepared GEMM; the values are what detr_hip_gemm_family promises (include/detr_hip.h).
enum GemmRoute { ROUTE_TILE = 0, ROUTE_STREAM = 1, ROUTE_RING = 2, ROUTE_RING_F32 = 3, ROUTE_LN = 4, ROUTE_RING_WGRAD = 5 };

// THE routing decision, in this order: fused LayerNorm; the ring kernel where it is eligible (in front of the streaming kernel, unless
// DETR_HIP_GEMM_STREAM=3, which takes the ring kernel out so that the streaming kernel keeps its K = 256 shapes); the streaming kernel;
// the fp32 ring kernel; the ring weight gradient; otherwise the 4-wave tile engine.  rp: the plan of the ring kernel that was chosen.
static GemmRoute gemm_route(const GemmPlan &p, RingPlan &rp) {
    if (p.d->ln_y) return ROUTE_LN;
    const bool ring_first = tune(T_GEMM_STREAM) != 3 && gemm_ring_eligible(p, rp);
    if (!ring_first && gemm_stream_eligible(p)) return ROUTE_STREAM;
    if (ring_first) return ROUTE_RING;
    if (gemm_ring_f32_eligible(p, rp)) return ROUTE_RING_F32;
    if (gemm_ring_wgrad_eligible(p)) return ROUTE_RING_WGRAD;
    return ROUTE_TILE;
}

// the deterministic split-K reduction a prepared GEMM (p.partial) leaves behind
static detr_reduce_desc gemm_reduce_desc(const GemmPlan &p) {
    const detr_gemm_desc *d = p.d;
    detr_reduce_desc r = {};
    r.ws = d->workspace; r.splits = p.split; r.part_stride = p.part; r.rows = d->M; r.cols = d->N;
    r.C = d->C; r.ldc = d->ldc; r.alpha = p.final_e.alpha; r.scale = p.final_e.scale;
    r.rs_ws = d->rowsum_a ? d->workspace + (long long)p.split * p.part : nullptr;
    r.rs_out = d->rowsum_a; r.rs_alpha = d->rowsum_alpha;
    r.ts_bm = p.ts_bm; r.ts_bn = p.ts_bn; r.ts_tiles_n = p.ts_tn;
    return r;
}

// the tile engine's kernel for a plan: the compile-time half of the tile table (gemm_tile_dims has the numbers)
static GemmKernel gemm_tile_kernel(const GemmPlan &p) {
    const bool ak = p.ak, bk = p.bk;
    if (p.bf16c) {
        const bool a16 = p.g.a16, b16 = p.g.b16;
        switch (p.tile) {
            case TILE_64x64: return gemm_bf16_for<64, 64>(ak, bk, a16, b16, p.deep);
            case TILE_128x128: return gemm_bf16_for<128, 128>(ak, bk, a16, b16, p.deep);
            case TILE_128x64: return gemm_bf16_for<128, 64>(ak, bk, a16, b16, false);
            case TILE_WIDE: return gemm_bf16_for<64, 128>(ak, bk, a16, b16, false);
            default: return nullptr;
        }
    }
    if (p.split3) {
        switch (p.tile) {
            case TILE_64x64: return gemm_x3_for<64, 64>(ak, bk);
            case TILE_128x128: return gemm_x3_for<128, 128>(ak, bk);
            case TILE_128x64: return gemm_x3_for<128, 64>(ak, bk);
            case TILE_X3_192x128: return gemm_x3_for<192, 128>(ak, bk);
            default: return nullptr;
        }
    }
    switch (p.tile) {
        case TILE_64x64: return by_layout<F32Kernels<64, 64, 2, 2>>(ak, bk);
        case TILE_128x128: return by_layout<F32Kernels<128, 128, 2, 2>>(ak, bk);
        case TILE_128x64: return by_layout<F32Kernels<128, 64, 2, 2>>(ak, bk);
        case TILE_128x32: return by_layout<F32Kernels<128, 32, 4, 1>>(ak, bk);
        case TILE_WIDE: return by_layout<F32Kernels<64, 256, 1, 4>>(ak, bk);
        case TILE_256x64: return by_layout<F32Kernels<256, 64, 4, 1>>(ak, bk);
        default: return nullptr;
    }
}

static int gemm_launch(const GemmPlan &p, hipStream_t s) {
    const detr_gemm_desc *d = p.d;
    RingPlan rp;
    switch (gemm_route(p, rp)) {
        case ROUTE_LN: return gemm_ln_launch(p, s);
        case ROUTE_STREAM:
            gemm_stream_launch(p, s);
            DETR_LAUNCH_CHECK("gemm (stream)");
            return 0;
        case ROUTE_RING:
            if (gemm_ring_launch(p.g, p.bk, rp, s)) return -1;
            DETR_LAUNCH_CHECK("gemm (ring)");
            if (d->defer_out) d->defer_out->splits = 0;
            return 0;
        case ROUTE_RING_F32:
            if (gemm_ring_f32_launch(p.g, p.bk, rp, s)) return -1;
            DETR_LAUNCH_CHECK("gemm (ring, fp32)");
            if (d->defer_out) d->defer_out->splits = 0;
            return 0;
        case ROUTE_RING_WGRAD:
            if (gemm_ring_wgrad_launch(p.g, p.ts_bm, p.ts_bn, p.split, s)) return -1;
            break;
        case ROUTE_TILE: {
            DETR_REQUIRE(p.tile != TILE_RING_128x256 && p.tile != TILE_RING_256x128, "gemm: the 128 x 256 / 256 x 128 tiles exist for the ring weight gradient only "
                         "(tile-ordered slabs in a workspace of detr_hip_workspace_bytes_gemm bytes are required)");
            const TileDims t = gemm_tile_dims(p.bf16c, p.tile);
            if (launch_gemm_tiles(gemm_tile_kernel(p), t.bm, t.bn, p.g, p.batch, s)) return -1;
            break;
        }
    }
    DETR_LAUNCH_CHECK("gemm");
    if (d->defer_out) {      // the caller reduces later, many slabs per launch (detr_hip_splitk_reduce_many)
        d->defer_out->splits = 0;
        if (p.partial) *d->defer_out = gemm_reduce_desc(p);
        return 0;
    }
    if (p.partial) {
        launch_splitk_reduce(gemm_reduce_desc(p), s);
        DETR_LAUNCH_CHECK("gemm split-k reduce");
    }
    return 0;
}

// Which kernel family detr_hip_gemm_f32 would launch for this descriptor -- the decision of gemm_launch itself, for callers that bill launches
// to roofline families (bench.py / scripts/pmc_summary.py through detr_tf/_hip.py; ADVICE r5: the Python copy of these rules had drifted).
// Negative: the descriptor is rejected (detr_hip_last_error).
extern "C" int detr_hip_gemm_family(const detr_gemm_desc *d) {
    GemmPlan p;
    if (gemm_prepare(d, p)) return -1;
    RingPlan rp;
    return gemm_route(p, rp);
}

extern "C" int detr_hip_gemm_f32(const detr_gemm_desc *d, void *stream) {
    GemmPlan p;
    if (gemm_prepare(d, p)) return -1;
    return gemm_launch(p, (hipStream_t)stream);
}

// ---- grouped launch ------------------------------------------------------------------------------
extern "C" int detr_hip_gemm_group_f32(const detr_gemm_desc *descs, int32_t n, void *stream) {
    DETR_REQUIRE(descs != nullptr && n >= 1 && n <= 64, "gemm group: 1..64 descriptors");
    hipStream_t s = (hipStream_t)stream;
    int done = 0;
    while (done < n) {
        const int m = (n - done) < GEMM_MAX_GROUP ? (n - done) : GEMM_MAX_GROUP;
        GemmPlan p[GEMM_MAX_GROUP];
        for (int i = 0; i < m; ++i) {
            DETR_REQUIRE(!descs[done + i].ln_y, "gemm group: the fused LayerNorm (ln_y) exists for single launches only");
            if (gemm_prepare(descs + done + i, p[i])) return -1;
        }
        // one launch needs ONE kernel variant: the tile engine's 64x64 tiles, same layouts / storage types, no batch; members may differ in shape
        bool same = m > 1 && tune(T_GEMM_GROUP) != 2;
        for (int i = 0; i < m && same; ++i) {
            RingPlan rp;
            same = p[i].tile == TILE_64x64 && p[i].batch == 1 && p[i].bf16c == p[0].bf16c && p[i].split3 == p[0].split3 && p[i].ak == p[0].ak &&
                   p[i].bk == p[0].bk && p[i].g.a16 == p[0].g.a16 && p[i].g.b16 == p[0].g.b16 && (p[i].split == 1 || p[i].partial) &&
                   gemm_route(p[i], rp) == ROUTE_TILE;
        }
        if (!same) {
            for (int i = 0; i < m; ++i)
                if (gemm_launch(p[i], s)) return -1;
            done += m;
            continue;
        }
        GemmGroupArgs G;
        G.n = m;
        G.work_off[0] = 0;
        for (int i = 0; i < m; ++i) {
            G.g[i] = p[i].g;
            G.g[i].tiles_m = cdiv(p[i].g.M, 64);
            G.g[i].tiles_n = cdiv(p[i].g.N, 64);
            G.work_off[i + 1] = G.work_off[i] + G.g[i].tiles_m * G.g[i].tiles_n * p[i].split;
        }
        for (int i = m; i < GEMM_MAX_GROUP; ++i) { G.g[i] = G.g[0]; G.work_off[i + 1] = G.work_off[m]; }
        const dim3 grid((unsigned)G.work_off[m]);      // exactly one workgroup per (member, split, tile): balanced over the XCDs
        hipLaunchKernelGGL(gemm_group_for(p[0].bf16c, p[0].split3, p[0].ak, p[0].bk, p[0].g.a16 != 0, p[0].g.b16 != 0), grid, dim3(GEMM_THREADS), 0, s, G);
        DETR_LAUNCH_CHECK("gemm group");
        // the members' split-K reductions, again as one launch (or handed back to the caller: detr_gemm_desc.defer_out)
        ReduceOne r[GEMM_MAX_GROUP];
        bool small[GEMM_MAX_GROUP];
        int nr = 0, nsmall = 0;
        for (int i = 0; i < m; ++i) {
            const detr_gemm_desc *d = p[i].d;
            if (d->defer_out) {
                d->defer_out->splits = 0;
                if (p[i].partial) *d->defer_out = gemm_reduce_desc(p[i]);
            } else if (p[i].partial) {
                r[nr] = reduce_plan(gemm_reduce_desc(p[i]), small[nr]);
                nsmall += small[nr++];
            }
        }
        if (nr > 0 && (nsmall == 0 || nsmall == nr)) {
            launch_reduce_list<GEMM_MAX_GROUP>(r, nr, nsmall > 0, s);
            DETR_LAUNCH_CHECK("gemm group split-k reduce");
        } else if (nr > 0) {      // mixed size classes: one launch each
            for (int i = 0; i < nr; ++i) launch_reduce_list<1>(&r[i], 1, small[i], s);
            DETR_LAUNCH_CHECK("gemm group split-k reduce (sequential)");
        }
        done += m;
    }
    return 0;
}



// Deferred split-K reductions (detr_gemm_desc.defer_out): n slab sets reduced by ceil(n / 16) launches per size class instead of
// one launch each -- the ~90 reductions of a training step were ~9 us latency-bound launches (rocprofv3: 0.9 ms per step).
extern "C" int detr_hip_splitk_reduce_many(const detr_reduce_desc *descs, int32_t n, void *stream) {
    DETR_REQUIRE(descs != nullptr && n >= 1, "splitk_reduce_many: bad args");
    hipStream_t s = (hipStream_t)stream;
    for (int pass = 0; pass < 2; ++pass) {           // pass 0: small outputs (16 split groups per block), pass 1: large ones
        ReduceOne r[REDUCE_MANY];
        int cnt = 0;
        for (int i = 0; i < n; ++i) {
            const detr_reduce_desc &d = descs[i];
            if (d.splits <= 0) continue;
            DETR_REQUIRE(d.ws && d.C && d.rows > 0 && d.cols > 0, "splitk_reduce_many: entry %d is malformed", i);
            DETR_REQUIRE(d.ts_bm == 0 || ((d.ts_bm == 64 || d.ts_bm == 128 || d.ts_bm == 256) && (d.ts_bn == 64 || d.ts_bn == 128 || d.ts_bn == 256) && d.ts_tiles_n > 0 &&
                                          d.part_stride % ((long long)d.ts_bm * d.ts_bn) == 0),
                         "splitk_reduce_many: entry %d has a malformed tile-ordered slab description", i);
            bool small;
            r[cnt] = reduce_plan(d, small);
            if (small != (pass == 0)) continue;
            if (++cnt == REDUCE_MANY) {
                launch_reduce_list<REDUCE_MANY>(r, cnt, pass == 0, s);
                cnt = 0;
            }
        }
        if (cnt > 0) launch_reduce_list<REDUCE_MANY>(r, cnt, pass == 0, s);
    }
    DETR_LAUNCH_CHECK("splitk_reduce_many");
    return 0;
}

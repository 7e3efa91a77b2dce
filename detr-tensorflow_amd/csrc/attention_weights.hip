// attention_weights.hip -- head-averaged attention maps (the need_weights branch of MultiHeadAttention.call,
// detr_tf/networks/transformer.py:285-286, 349-354) from what the fused cores leave behind:
//     w[b, t, s] = (1/H) sum_h exp(scale q[b,t,h] . k[b,s,h] - lse[b,h,t])
// One extra pass per requested site.  The per-head [B*H, T, S] tensor is never formed: the H score tiles of a 32 x 32 block of
// (query, key) pairs are accumulated in the same 16 registers and one fp32 tile is written.  No softmax reduction either -- the
// forward's lse [B*H, T] already is the row's log-sum-exp.
//
// What bounds it: the output, B*T*S*4 bytes written against (B*T + B*S) * H*32 * esz read.  So the score tile is computed in the
// orientation whose C/D map puts the KEY on the lane and 16 queries in registers (A = Q rows, B = K rows as columns): register r of
// lane l is w[query krow(r, l >> 5)][key l & 31], every store instruction of a wave writes two full 128-byte row segments, and the
// heads add up register by register with no lane movement.
//   * workgroup = 4 waves = 128 queries x a run of `chunk` key tiles of one batch entry.  A wave's Q fragments (32 queries x H heads)
//     are read ONCE into registers and stay there while the workgroup walks its key tiles;
//   * a key tile (32 keys x H*32 columns) is fetched once per workgroup into LDS (register-staged prefetch of the next tile while the
//     current one is computed), rows padded by 16 bytes: the 16-byte fragment reads of 16 lanes cover all 64 banks once;
//   * the contraction index of an MFMA is a free choice as long as both operands agree: lane half `hi` takes head columns
//     16 hi .. 16 hi + 15, which are contiguous in memory (fp32: 16 k-steps of v_mfma_f32_32x32x2_f32, bf16: the two
//     v_mfma_f32_32x32x16_bf16 of head_dim 32);
//   * scores in log2 units: fp32 operands have q multiplied by scale * log2(e) in registers (as attention_f32.hip does), bf16
//     operands carry it already (attention_dma.hip); -lse * log2(e) is converted once per row into LDS and is the C operand of the
//     head's first MFMA, so exp2 of the accumulator is the probability;
//   * key padding mask: a tile's validity word is workgroup-uniform.  A tile without a valid key stores zeros without computing; in a
//     partial one the masked lanes SELECT 0.0f (garbage in a masked K row stays in its own column of the MFMA and is never stored).
#include "attention_common.h"

namespace detr {

typedef __bf16 aw_bf16x8 __attribute__((ext_vector_type(8)));

constexpr int AW_QROWS = 128;        // queries per workgroup (4 waves x 32)
constexpr int AW_MAXH = 8;           // heads whose Q fragments a wave keeps in registers

struct AwArgs {
    const void *Q, *K;               // [B, T|S, ld] fp32 or bf16
    const float *LSE;                // [B*H, T] natural log
    float *W;                        // [B, T, ldw]
    int B, H, T, S;
    long long ldq, ldk, ldw;         // row strides in elements
    float qmul;                      // fp32 operands: scale * log2(e)
    float inv_h;
    const uint32_t *key_valid;       // MASK: [B][kv_words]
    int kv_words;
    int chunk;                       // key tiles per workgroup
};

template <bool BF, bool MASK>
__global__ __launch_bounds__(256) void attn_weights_kernel(AwArgs a) {
    constexpr int ESZ = BF ? 2 : 4;
    constexpr int ROWB = 256 * ESZ + 16;             // LDS pitch of a key row (bytes)
    constexpr int CPR = 256 * ESZ / 16;              // 16-byte chunks per key row
    constexpr int NLD = 32 * CPR / 256;              // chunks per thread and tile
    __shared__ __attribute__((aligned(16))) char Ks[32 * ROWB];
    __shared__ __attribute__((aligned(16))) float Ls[AW_MAXH][AW_QROWS];       // -lse * log2(e)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, hi = lane >> 5;
    const int b = blockIdx.z, q0 = blockIdx.x * AW_QROWS;
    const int ntiles = (a.S + 31) / 32;
    const int tile0 = blockIdx.y * a.chunk, tile1 = min(ntiles, tile0 + a.chunk);
    const int hchunks = a.H * (32 * ESZ / 16);       // 16-byte chunks of a row that hold heads

    for (int i = tid; i < AW_MAXH * AW_QROWS; i += 256) {
        const int h = i / AW_QROWS, t = q0 + (i % AW_QROWS);
        Ls[h][i % AW_QROWS] = (h < a.H && t < a.T) ? -(a.LSE[((long long)b * a.H + h) * a.T + t] * AT_LOG2E) : 0.0f;
    }

    // this wave's Q fragments: query q0 + 32 wave + l31, head columns 16 hi .. 16 hi + 15 of every head
    const int tq = q0 + wave * 32 + l31;
    const bool qok = tq < a.T;
    float qf[AW_MAXH][BF ? 1 : 16];
    aw_bf16x8 qb[AW_MAXH][BF ? 2 : 1];
    {
        const char *qrow = (const char *)a.Q + ((long long)b * a.T + (qok ? tq : 0)) * a.ldq * ESZ + hi * 16 * ESZ;
#pragma unroll
        for (int h = 0; h < AW_MAXH; ++h) {
            const bool ok = qok && h < a.H;
            if constexpr (BF) {
#pragma unroll
                for (int m = 0; m < 2; ++m) {
                    uint4 v = make_uint4(0u, 0u, 0u, 0u);
                    if (ok) v = *reinterpret_cast<const uint4 *>(qrow + h * 64 + m * 16);
                    qb[h][m] = __builtin_bit_cast(aw_bf16x8, v);
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (ok) v = *reinterpret_cast<const float4 *>(qrow + h * 128 + j * 16);
                    qf[h][4 * j + 0] = v.x * a.qmul; qf[h][4 * j + 1] = v.y * a.qmul;
                    qf[h][4 * j + 2] = v.z * a.qmul; qf[h][4 * j + 3] = v.w * a.qmul;
                }
            }
        }
    }

    const char *Kb = (const char *)a.K + (long long)b * a.S * a.ldk * ESZ;
    uint4 pre[NLD];
    auto load_tile = [&](int tile) {
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int u = tid + 256 * i, r = u / CPR, c = u % CPR;
            const int key = tile * 32 + r;
            pre[i] = make_uint4(0u, 0u, 0u, 0u);
            if (key < a.S && c < hchunks) pre[i] = *reinterpret_cast<const uint4 *>(Kb + (long long)key * a.ldk * ESZ + c * 16);
        }
    };
    auto store_tile = [&]() {
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int u = tid + 256 * i, r = u / CPR, c = u % CPR;
            *reinterpret_cast<uint4 *>(Ks + r * ROWB + c * 16) = pre[i];
        }
    };

    const uint32_t *kvw = MASK ? a.key_valid + (long long)b * a.kv_words : nullptr;
    const char *kfrag = Ks + l31 * ROWB + hi * 16 * ESZ;          // + h * 32 * ESZ: this lane's key, its half of the head
    const float *lrow = &Ls[0][wave * 32 + 4 * hi];               // + h * AW_QROWS + 8 g: the lane's rows 8 g + 4 hi .. + 3
    if (tile0 < tile1) load_tile(tile0);
    for (int tile = tile0; tile < tile1; ++tile) {
        __syncthreads();                     // the previous tile has been read (first trip: Ls is complete)
        store_tile();
        __syncthreads();
        if (tile + 1 < tile1) load_tile(tile + 1);
        unsigned kv = ~0u;
        if constexpr (MASK) kv = kvw[tile];
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
        if (!MASK || kv != 0u) {
#pragma unroll
            for (int h = 0; h < AW_MAXH; ++h) {
                if (h < a.H) {
                    f32x16 s;
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const float4 l4 = *reinterpret_cast<const float4 *>(lrow + h * AW_QROWS + 8 * g);
                        s[4 * g + 0] = l4.x; s[4 * g + 1] = l4.y; s[4 * g + 2] = l4.z; s[4 * g + 3] = l4.w;
                    }
                    if constexpr (BF) {
#pragma unroll
                        for (int m = 0; m < 2; ++m) {
                            const aw_bf16x8 kb = *reinterpret_cast<const aw_bf16x8 *>(kfrag + h * 64 + m * 16);
                            s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qb[h][m], kb, s, 0, 0, 0);
                        }
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const float4 k4 = *reinterpret_cast<const float4 *>(kfrag + h * 128 + j * 16);
                            s = __builtin_amdgcn_mfma_f32_32x32x2f32(qf[h][4 * j + 0], k4.x, s, 0, 0, 0);
                            s = __builtin_amdgcn_mfma_f32_32x32x2f32(qf[h][4 * j + 1], k4.y, s, 0, 0, 0);
                            s = __builtin_amdgcn_mfma_f32_32x32x2f32(qf[h][4 * j + 2], k4.z, s, 0, 0, 0);
                            s = __builtin_amdgcn_mfma_f32_32x32x2f32(qf[h][4 * j + 3], k4.w, s, 0, 0, 0);
                        }
                    }
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[r] += fast_exp2(s[r]);
                }
            }
        }
        const int key = tile * 32 + l31;
        if (key < a.S) {
            const bool valid = !MASK || ((kv >> l31) & 1u) != 0u;
            float *wp = a.W + ((long long)b * a.T + q0 + wave * 32) * a.ldw + key;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = krow(r, hi);
                if (q0 + wave * 32 + row < a.T) wp[(long long)row * a.ldw] = valid ? acc[r] * a.inv_h : 0.0f;
            }
        }
    }
}

// key tiles per workgroup: long runs amortise the Q fragments (1 KB per query, read per run), short ones fill the chip
static int aw_chunk(int B, int T, int ntiles) {
    int chunk = 16;
    while (chunk > 2 && (long long)B * cdiv(T, AW_QROWS) * cdiv(ntiles, chunk) < 1024) chunk >>= 1;
    return chunk;
}

}  // namespace detr

using namespace detr;

extern "C" int detr_hip_attention_weights(const detr_attn_desc *d, const uint32_t *key_valid, float *w, int64_t ldw, void *stream) {
    DETR_REQUIRE(d, "attention_weights: null descriptor");
    DETR_REQUIRE(d->q && d->k && d->lse && w, "attention_weights: null operand (q, k, lse, w)");
    DETR_REQUIRE(d->B > 0 && d->B <= 65535 && d->T > 0 && d->S > 0 && d->S <= 8192,
                 "attention_weights: bad shape B=%d T=%d S=%d (B 1..65535, T >= 1, S 1..8192)", d->B, d->T, d->S);
    DETR_REQUIRE(d->H > 0 && d->H <= AW_MAXH, "attention_weights: H=%d, 1..%d heads of 32 columns are supported", d->H, AW_MAXH);
    DETR_REQUIRE(ldw >= d->S, "attention_weights: ldw=%lld is smaller than S=%d", (long long)ldw, d->S);
    DETR_REQUIRE(d->dropout_p == 0.0f, "attention_weights: dropout_p=%f: the maps of a pass with attention dropout are not supported", d->dropout_p);
    DETR_REQUIRE(d->io_dtype == 0 || d->io_dtype == 1, "attention_weights: io_dtype=%d must be 0 (fp32) or 1 (bf16)", d->io_dtype);
    DETR_REQUIRE(d->compute >= 0 && d->compute <= 2, "attention_weights: compute=%d must be 0, 1 or 2", d->compute);
    DETR_REQUIRE(!(d->io_dtype == 0 && d->compute == 1), "attention_weights: bf16 compute (1) needs bf16 tensors (io_dtype = 1)");
    DETR_REQUIRE(!(d->io_dtype == 1 && d->compute != 1), "attention_weights: bf16 tensors (io_dtype = 1) need compute = 1");
    const int mult = d->io_dtype == 1 ? 8 : 4;
    DETR_REQUIRE(d->ldq >= (long long)d->H * 32 && d->ldq % mult == 0 && d->ldk >= (long long)d->H * 32 && d->ldk % mult == 0,
                 "attention_weights: row strides of q (%lld) and k (%lld) must be >= heads*32 and multiples of %d", (long long)d->ldq,
                 (long long)d->ldk, mult);
    DETR_REQUIRE(aligned16(d->q) && aligned16(d->k), "attention_weights: q and k must be 16-byte aligned");
    DETR_REQUIRE((reinterpret_cast<uintptr_t>(w) & 3) == 0 && (reinterpret_cast<uintptr_t>(d->lse) & 3) == 0,
                 "attention_weights: w and lse must be 4-byte aligned");
    DETR_REQUIRE(d->scale > 0.0f, "attention_weights: scale must be positive (1 = q already scaled)");
    AwArgs a{};
    a.Q = d->q; a.K = d->k; a.LSE = d->lse; a.W = w;
    a.B = d->B; a.H = d->H; a.T = d->T; a.S = d->S;
    a.ldq = d->ldq; a.ldk = d->ldk; a.ldw = ldw;
    a.qmul = d->scale * AT_LOG2E;
    a.inv_h = 1.0f / (float)d->H;
    a.key_valid = key_valid;
    a.kv_words = (d->S + 31) / 32;
    const int ntiles = a.kv_words;
    a.chunk = aw_chunk(d->B, d->T, ntiles);
    const dim3 grid(cdiv(d->T, AW_QROWS), cdiv(ntiles, a.chunk), d->B);
    hipStream_t s = (hipStream_t)stream;
    if (d->io_dtype == 1) {
        if (key_valid) attn_weights_kernel<true, true><<<grid, 256, 0, s>>>(a);
        else attn_weights_kernel<true, false><<<grid, 256, 0, s>>>(a);
    } else {
        if (key_valid) attn_weights_kernel<false, true><<<grid, 256, 0, s>>>(a);
        else attn_weights_kernel<false, false><<<grid, 256, 0, s>>>(a);
    }
    DETR_LAUNCH_CHECK("attention_weights");
    return 0;
}

// edgemlp_bf16.hip -- EdgeConv for a two-layer edge MLP over ANY grouped edge list with the per-edge products on the
// bf16 or fp16 matrix cores (gfx950), forward and backward.  Both operand types run the same two kernels, templates over
// the operand type (OpBf16, OpF16): the fp16 instances differ only in the rounding to 16 bits (v_cvt_f16_f32 /
// v_cvt_pk_f16_f32 instead of v_cvt_pk_bf16_f32) and the MFMA (v_mfma_f32_16x16x32_f16); what follows says bf16 for
// either.
//
// Replaces, for  nn = Sequential(Linear(2 Hin, H1), ELU, Linear(H1, H2)[, ELU][, BatchNorm1d(H2)])  and aggr in
// {max, add, mean}, the generic route under bf16 autocast (edge_features -> nn over E rows -> segment max / sum) and its
// autograd graph: the call shape of model/dynamic_reduction_network.py:59-73,86-87,94-95 (EdgeConv over
// to_undirected(knn_graph(...))) when the model runs under torch.autocast(dtype=torch.bfloat16).
//
// Only the two edge passes live here.  Everything at node level is the fp32 route's (edgemlp_f32.hip, which also owns
// the entry points and the host orchestration): the split of the first Linear PQ = [x (W1a - W1b)^T + b1 | x W1b^T],
// the BatchNorm finalize and apply kernels, the BatchNorm backward reduction, the gW2 partial sums and gx.  The plan is
// that route's plan:
//   forward edge pass: workgroup b owns the node range whose edges start at b E / nblk; it walks its edges in tiles of
//     T = 32 consecutive edges that may span targets: h1 = ELU(P_tgt + Q_src) in fp32 -> bf16 tile in LDS,
//     z2 = h1 W2^T + b2 on v_mfma_f32_16x16x32_bf16 (fp32 accumulation; W2 bf16 in LDS), m = ELU?(z2) in fp32, then
//     one thread per channel folds the tile in edge order into the current target's aggregate (max winners as int32
//     edge positions, lowest on ties) and keeps the BatchNorm partials sum m, sum m^2.
//   backward edge pass by target: per tile re-computes z2 as above, g_z2 in fp32 (fp32 route's formula), then on the
//     matrix cores g_h1 = g_z2 W2 and the gW2 accumulation gW2 += g_z2^T h1 (both operands bf16, fp32 accumulators that
//     live in registers across the workgroup's tiles); g_pre1 = g_h1 ELU'(h1) in fp32 is summed per target into gP in
//     edge order; gb2 is an fp32 sum of g_z2.  The same pass by source (EdgeList.by_source order) sums gQ.
// No [E, *] tensor in HBM, no atomics: every sum runs in a fixed order inside one workgroup; run to run bit-identical.
//
// MFMA operand maps (16x16x32 bf16): lane l holds A[row l & 15][k = 8 (l >> 4) + j] and B[k = 8 (l >> 4) + j][col l & 15],
// j = 0..7; C/D: col = l & 15, row = 4 (l >> 4) + reg.
//   z2    : A = h1 [t][c]  (edge-major bf16 tile, row pitch SH),  B[c][o] = W2[o][c] (W2 bf16 [H2][SH]); K = H1 padded to 32
//   g_h1  : A = g_z2 [t][o] (edge-major bf16 tile, pitch H2 + 8), B[o][c] = W2[o][c] (the same W2 image, read by column)
//   gW2   : A[o][t] = g_z2 (channel-major fp32 tile, rounded on the read), B[t][c] = h1 (channel-major fp32 tile); K = T
// The channel-major fp32 tiles also serve the fp32 parts: ELU'(h1), gb2, and (in place of h1) g_pre1 for the fold.
//
// Numerics: P, Q, ELU, the aggregation and the BatchNorm are fp32.  Forward: h1 and W2 rounded to bf16 (RNE), products
// exact, fp32 accumulation.  Backward: g_z2, h1 and W2 rounded to bf16 for g_h1 and gW2, fp32 accumulation; node-level
// products fp32.  Compared with the fp32 result at the R6 bar (rtol 2e-2 of the output scale).  fp16: the same, rounded
// to nearest even, overflow to +-inf (a GradScaler scale too large for g_z2 gives a non-finite gradient, never a
// saturated finite one), subnormals kept (the kernel's default fp16 denorm mode).
//
// Widths (dmet_edge_mlp_bf16_supported): H2 in {32, 64, 128}, H1 a multiple of 16 with H1 <= min(192, 2 H2),
// 1 <= Hin <= 128.  LDS per workgroup (T = 32): forward 2 SH (H2 + T) + 4 H2 (TS + 1) + 8 T bytes, backward
// 2 SH (H2 + T) + 4 TS (H1 + H2) + 2 T (H2 + 8) + 4 H2 + 12 T bytes, SH = roundup(H1, 32) + 8, TS = T + 4.
#include "edgemlp_fused.h"

namespace dmet {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

constexpr int kT = 32;          // edges per tile (the K of the gW2 product)
constexpr int kTS = kT + 4;     // row pitch of the channel-major fp32 tiles
constexpr int kWaves = kBlk / 64;

// The 16-bit operand type of the per-edge products: how an fp32 value is rounded to its 16 bits (kept as such in LDS),
// how 16 bits enter an MFMA operand, and the MFMA.  The kernels below are written once over it.
struct OpBf16 {
    typedef bf16x8 vec;
    static __device__ __forceinline__ unsigned short bits(float f)
    {
        const __bf16 b = (__bf16)f;     // RNE (v_cvt_pk_bf16_f32)
        return __builtin_bit_cast(unsigned short, b);
    }
    static __device__ __forceinline__ short elem(unsigned short u) { return (short)u; }
    static __device__ __forceinline__ f32x4 mfma(vec a, vec b, f32x4 c)
    {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
    }
};

struct OpF16 {
    typedef f16x8 vec;
    static __device__ __forceinline__ unsigned short bits(float f)
    {
        // v_cvt_f16_f32 in the kernel's default mode: RNE, beyond 65504 (after rounding) +-inf, subnormals kept -- not
        // the packed round-toward-zero v_cvt_pkrtz_f16_f32
        const _Float16 h = (_Float16)f;
        return __builtin_bit_cast(unsigned short, h);
    }
    static __device__ __forceinline__ _Float16 elem(unsigned short u) { return __builtin_bit_cast(_Float16, u); }
    static __device__ __forceinline__ f32x4 mfma(vec a, vec b, f32x4 c)
    {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
    }
};

__host__ __device__ __forceinline__ int h1_pad(int H1) { return (H1 + 31) & ~31; }
__host__ __device__ __forceinline__ int h1_pitch(int H1) { return h1_pad(H1) + 8; }

// 8 consecutive 16-bit operands from LDS (16-B aligned)
template <typename Op>
__device__ __forceinline__ typename Op::vec ld8(const unsigned short *p) { return *reinterpret_cast<const typename Op::vec *>(p); }

// 8 consecutive fp32 from LDS (16-B aligned), rounded to the operand type
template <typename Op>
__device__ __forceinline__ typename Op::vec ld8_f32(const float *p)
{
    const float4 a = *reinterpret_cast<const float4 *>(p), b = *reinterpret_cast<const float4 *>(p + 4);
    typename Op::vec r;
    r[0] = Op::elem(Op::bits(a.x)); r[1] = Op::elem(Op::bits(a.y)); r[2] = Op::elem(Op::bits(a.z)); r[3] = Op::elem(Op::bits(a.w));
    r[4] = Op::elem(Op::bits(b.x)); r[5] = Op::elem(Op::bits(b.y)); r[6] = Op::elem(Op::bits(b.z)); r[7] = Op::elem(Op::bits(b.w));
    return r;
}

// W2 as 16-bit [H2][SH] (columns H1 .. SH - 1 zero) and b2 fp32 [H2]
template <typename Op>
__device__ __forceinline__ void stage_w2(const float *__restrict__ W2, const float *__restrict__ b2, int H1, int H2,
                                         unsigned short *w2s, float *b2s)
{
    const int SH = h1_pitch(H1);
    for (int idx = threadIdx.x; idx < H2 * SH; idx += blockDim.x) {
        const int o = idx / SH, c = idx - o * SH;
        w2s[idx] = c < H1 ? Op::bits(W2[(int64_t)o * H1 + c]) : (unsigned short)0;
    }
    for (int o = threadIdx.x; o < H2; o += blockDim.x) b2s[o] = b2 ? b2[o] : 0.0f;
}

// h1 = ELU(P_tgt + Q_src) of the tile's cnt edges (beyond: 0): 16-bit edge-major [T][SH] (padding columns 0) and, when
// h1c is given, fp32 channel-major [H1][TS]
template <typename Op>
__device__ __forceinline__ void fill_h1(const float *__restrict__ PQ, int H1, const int32_t *tg, const int32_t *sr, int cnt,
                                        unsigned short *h1e, float *h1c)
{
    const int H1p = h1_pad(H1), SH = h1_pitch(H1);
    for (int idx = threadIdx.x; idx < kT * H1p; idx += blockDim.x) {
        const int t = idx / H1p, c = idx - t * H1p;
        float h = 0.0f;
        if (t < cnt && c < H1) h = elu1f(PQ[(int64_t)tg[t] * 2 * H1 + c] + PQ[(int64_t)sr[t] * 2 * H1 + H1 + c]);
        h1e[t * SH + c] = Op::bits(h);
        if (h1c && c < H1) h1c[c * kTS + t] = h;
    }
}

// z2 block (edge block eb, channel block ob) of the tile, before the bias: C[t][o], t = 16 eb + 4 (l >> 4) + r
template <typename Op>
__device__ __forceinline__ f32x4 z2_block(const unsigned short *h1e, const unsigned short *w2s, int H1, int eb, int ob, int lane)
{
    const int SH = h1_pitch(H1), ksteps = h1_pad(H1) / 32;
    const unsigned short *pa = h1e + (16 * eb + (lane & 15)) * SH + 8 * (lane >> 4);
    const unsigned short *pb = w2s + (16 * ob + (lane & 15)) * SH + 8 * (lane >> 4);
    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int ks = 0; ks < ksteps; ++ks) acc = Op::mfma(ld8<Op>(pa + 32 * ks), ld8<Op>(pb + 32 * ks), acc);
    return acc;
}

// aggr: 0 max, 1 add, 2 mean.  bn: 0 none, 1 training (keep the statistics partials), 2 eval.
template <typename Op, int H2>
__global__ __launch_bounds__(kBlk) void edge_mlp_fwd_mma_kernel(const float *__restrict__ PQ, const int32_t *__restrict__ rowptr,
                                                                 const int32_t *__restrict__ src, const int32_t *__restrict__ tgt,
                                                                 int64_t N, int64_t E, int H1, const float *__restrict__ W2,
                                                                 const float *__restrict__ b2, int act2, int aggr, int bn,
                                                                 float *__restrict__ agg, int32_t *__restrict__ win,
                                                                 float *__restrict__ partial)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const int SH = h1_pitch(H1);
    unsigned short *w2s = reinterpret_cast<unsigned short *>(lds_raw);   // [H2][SH]
    unsigned short *h1e = w2s + H2 * SH;                                 // [T][SH]
    float *b2s = reinterpret_cast<float *>(h1e + kT * SH);               // [H2]
    float *ms = b2s + H2;                                                // [H2][TS]
    int32_t *tg = reinterpret_cast<int32_t *>(ms + H2 * kTS);            // [T]
    int32_t *sr = tg + kT;                                               // [T]
    stage_w2<Op>(W2, b2, H1, H2, w2s, b2s);

    const int nblk = gridDim.x;
    const int64_t n0 = range_start(rowptr, N, E, blockIdx.x, nblk), n1 = range_start(rowptr, N, E, blockIdx.x + 1, nblk);
    const int64_t p0 = rowptr[n0], p1 = rowptr[n1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool maxa = aggr == 0, mins = maxa && bn != 0;
    // running aggregate of channel threadIdx.x (threads < H2)
    int64_t cur = -1;
    float s = 0.0f, mx = 0.0f, mn = 0.0f, st1 = 0.0f, st2 = 0.0f;
    int32_t amx = -1, amn = -1;
    auto flush = [&]() {
        if (cur < 0) return;
        const int64_t q = cur * H2 + threadIdx.x;
        if (maxa) {
            agg[q] = mx;
            win[q] = amx;
            if (mins) {
                agg[N * H2 + q] = mn;
                win[N * H2 + q] = amn;
            }
        } else {
            agg[q] = s;
        }
    };
    for (int64_t pt = p0; pt < p1; pt += kT) {
        const int cnt = (int)(p1 - pt < kT ? p1 - pt : kT);
        __syncthreads();       // the previous tile's readers of tg / sr / ms are done
        for (int t = threadIdx.x; t < kT; t += blockDim.x) {
            tg[t] = t < cnt ? tgt[pt + t] : 0;
            sr[t] = t < cnt ? src[pt + t] : 0;
        }
        __syncthreads();
        fill_h1<Op>(PQ, H1, tg, sr, cnt, h1e, nullptr);
        __syncthreads();
        for (int blk = wave; blk < 2 * (H2 / 16); blk += kWaves) {
            const int eb = blk & 1, ob = blk >> 1;
            const f32x4 acc = z2_block<Op>(h1e, w2s, H1, eb, ob, lane);
            const int o = 16 * ob + (lane & 15);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float z = acc[r] + b2s[o];
                ms[o * kTS + 16 * eb + 4 * (lane >> 4) + r] = act2 ? elu1f(z) : z;
            }
        }
        __syncthreads();
        if (threadIdx.x < H2) {
            const int c = threadIdx.x;
            for (int t = 0; t < cnt; ++t) {
                const int64_t own = tg[t];
                const float m = ms[c * kTS + t];
                const int32_t e = (int32_t)(pt + t);
                if (own != cur) {
                    flush();
                    cur = own;
                    s = m; mx = m; mn = m; amx = e; amn = e;
                } else {
                    s += m;
                    if (m > mx) { mx = m; amx = e; }
                    if (m < mn) { mn = m; amn = e; }
                }
                if (bn == 1) {
                    st1 += m;
                    st2 = __builtin_fmaf(m, m, st2);
                }
            }
        }
    }
    if (threadIdx.x < H2) {
        flush();
        if (bn == 1) {
            partial[(int64_t)blockIdx.x * 2 * H2 + threadIdx.x] = st1;
            partial[(int64_t)blockIdx.x * 2 * H2 + H2 + threadIdx.x] = st2;
        }
    }
}

// Backward edge pass.  BY_SRC = false: positions are grouped edges (owner = tgt), sums g_pre1 per target into
// gpq[:, 0:H1] and keeps gW2 / gb2 partials; BY_SRC = true: positions walk srcperm (owner = src), sums into gpq[:, H1:2H1].
template <typename Op, int H2, bool BY_SRC>
__global__ __launch_bounds__(kBlk) void edge_mlp_bwd_mma_kernel(const float *__restrict__ PQ, const int32_t *__restrict__ rowptr,
                                                                 const int32_t *__restrict__ optr, const int32_t *__restrict__ perm,
                                                                 const int32_t *__restrict__ src, const int32_t *__restrict__ tgt,
                                                                 int64_t N, int64_t E, int H1, const float *__restrict__ W2,
                                                                 const float *__restrict__ b2, int act2, int aggr, int bn,
                                                                 const float *__restrict__ g_out, const int32_t *__restrict__ win,
                                                                 const float *__restrict__ bnstat, const float *__restrict__ coef,
                                                                 float *__restrict__ gpq, float *__restrict__ partial)
{
    constexpr int H1MAX = 2 * H2 < 192 ? 2 * H2 : 192;
    constexpr int NGW = (H2 / 16) * (H1MAX / 16) / kWaves;     // gW2 blocks per wave at the widest H1
    constexpr int NGH = (2 * (H1MAX / 16) + kWaves - 1) / kWaves;  // g_h1 blocks per wave at the widest H1
    constexpr int SZ = H2 + 8;                                   // row pitch of the edge-major g_z2 tile
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const int SH = h1_pitch(H1);
    unsigned short *w2s = reinterpret_cast<unsigned short *>(lds_raw);   // [H2][SH]
    unsigned short *h1e = w2s + H2 * SH;                                 // [T][SH]
    unsigned short *gze = h1e + kT * SH;                                 // [T][SZ]   g_z2, 16-bit
    float *b2s = reinterpret_cast<float *>(gze + kT * SZ);               // [H2]
    float *h1c = b2s + H2;                                               // [H1][TS]  h1, then g_pre1
    float *gzc = h1c + H1 * kTS;                                         // [H2][TS]  g_z2, fp32
    int32_t *tg = reinterpret_cast<int32_t *>(gzc + H2 * kTS);           // [T]
    int32_t *sr = tg + kT;                                               // [T]
    int32_t *ep = sr + kT;                                               // [T] grouped edge position
    stage_w2<Op>(W2, b2, H1, H2, w2s, b2s);

    const int nblk = gridDim.x;
    const int64_t n0 = range_start(optr, N, E, blockIdx.x, nblk), n1 = range_start(optr, N, E, blockIdx.x + 1, nblk);
    const int64_t p0 = optr[n0], p1 = optr[n1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ngw = (H2 / 16) * (H1 / 16), ngh = 2 * (H1 / 16);
    f32x4 gw[BY_SRC ? 1 : NGW];
    if (!BY_SRC) {
#pragma unroll
        for (int j = 0; j < NGW; ++j) gw[j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    }
    float gb = 0.0f;
    int64_t cur = -1;
    float run = 0.0f;
    const int coff = BY_SRC ? H1 : 0;
    for (int64_t pt = p0; pt < p1; pt += kT) {
        const int cnt = (int)(p1 - pt < kT ? p1 - pt : kT);
        __syncthreads();
        load_tile_ids<kT, BY_SRC>(src, tgt, perm, pt, cnt, tg, sr, ep);
        __syncthreads();
        fill_h1<Op>(PQ, H1, tg, sr, cnt, h1e, h1c);
        __syncthreads();
        // g_z2 per (edge, channel) from the re-computed z2 (fp32), into both g_z2 tiles
        for (int blk = wave; blk < 2 * (H2 / 16); blk += kWaves) {
            const int eb = blk & 1, ob = blk >> 1;
            const f32x4 acc = z2_block<Op>(h1e, w2s, H1, eb, ob, lane);
            const int o = 16 * ob + (lane & 15);
            const Gz2<H2> gz2(coef, bnstat, win, N, aggr, bn, o);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int t = 16 * eb + 4 * (lane >> 4) + r;
                const float gzv = t < cnt ? gz2(acc[r] + b2s[o], g_out, rowptr, act2, aggr, bn, tg, ep, t, o) : 0.0f;
                gzc[o * kTS + t] = gzv;
                gze[t * SZ + o] = Op::bits(gzv);
            }
        }
        __syncthreads();
        if (!BY_SRC) {
            // gW2[o][c] += sum_t g_z2[t][o] h1[t][c]: blocks (ob, cb) of this wave, K = the tile's T edges
#pragma unroll
            for (int j = 0; j < NGW; ++j) {
                const int blk = wave + kWaves * j;
                if (blk < ngw) {
                    const int ob = blk % (H2 / 16), cb = blk / (H2 / 16);
                    const typename Op::vec a = ld8_f32<Op>(gzc + (16 * ob + (lane & 15)) * kTS + 8 * (lane >> 4));
                    const typename Op::vec b = ld8_f32<Op>(h1c + (16 * cb + (lane & 15)) * kTS + 8 * (lane >> 4));
                    gw[j] = Op::mfma(a, b, gw[j]);
                }
            }
            if (threadIdx.x < H2) {
                float a = 0.0f;
                for (int t = 0; t < cnt; ++t) a += gzc[threadIdx.x * kTS + t];
                gb += a;
            }
        }
        // g_h1[t][c] = sum_o g_z2[t][o] W2[o][c]: blocks (eb, cb), kept in registers until every h1c reader is done
        f32x4 gh[NGH];
#pragma unroll
        for (int j = 0; j < NGH; ++j) {
            gh[j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            const int blk = wave + kWaves * j;
            if (blk < ngh) {
                const int eb = blk & 1, cb = blk >> 1;
                const unsigned short *pa = gze + (16 * eb + (lane & 15)) * SZ + 8 * (lane >> 4);
                const unsigned short *pb = w2s + 8 * (lane >> 4) * SH + 16 * cb + (lane & 15);
                for (int ks = 0; ks < H2 / 32; ++ks) {
                    typename Op::vec b;
#pragma unroll
                    for (int q = 0; q < 8; ++q) b[q] = Op::elem(pb[(32 * ks + q) * SH]);
                    gh[j] = Op::mfma(ld8<Op>(pa + 32 * ks), b, gh[j]);
                }
            }
        }
        __syncthreads();
        // g_pre1 = g_h1 ELU'(h1) in place of h1 (each element read and written by its own lane)
#pragma unroll
        for (int j = 0; j < NGH; ++j) {
            const int blk = wave + kWaves * j;
            if (blk < ngh) {
                const int eb = blk & 1, c = 16 * (blk >> 1) + (lane & 15);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float *p = h1c + c * kTS + 16 * eb + 4 * (lane >> 4) + r;
                    const float h = *p;
                    *p = gh[j][r] * (h > 0.0f ? 1.0f : h + 1.0f);
                }
            }
        }
        __syncthreads();
        if (threadIdx.x < H1) {
            const int c = threadIdx.x;
            for (int t = 0; t < cnt; ++t) {
                const int64_t own = BY_SRC ? sr[t] : tg[t];
                const float v = h1c[c * kTS + t];
                if (own != cur) {
                    if (cur >= 0) gpq[cur * 2 * H1 + coff + c] = run;
                    cur = own;
                    run = v;
                } else {
                    run += v;
                }
            }
        }
    }
    if (threadIdx.x < H1 && cur >= 0) gpq[cur * 2 * H1 + coff + threadIdx.x] = run;
    if (!BY_SRC) {
        // partial[blk] = gW2 [H2][H1] | gb2 [H2]
        float *pb = partial + (int64_t)blockIdx.x * (H2 * H1 + H2);
#pragma unroll
        for (int j = 0; j < NGW; ++j) {
            const int blk = wave + kWaves * j;
            if (blk < ngw) {
                const int ob = blk % (H2 / 16), cb = blk / (H2 / 16);
                const int c = 16 * cb + (lane & 15);
#pragma unroll
                for (int r = 0; r < 4; ++r) pb[(16 * ob + 4 * (lane >> 4) + r) * H1 + c] = gw[j][r];
            }
        }
        if (threadIdx.x < H2) pb[H2 * H1 + threadIdx.x] = gb;
    }
}

inline size_t fwd_lds_bytes_mma(int H1, int H2)
{
    const size_t SH = h1_pitch(H1);
    return 2 * SH * (H2 + kT) + sizeof(float) * (size_t)H2 * (kTS + 1) + 2 * sizeof(int32_t) * kT;
}

inline size_t bwd_lds_bytes_mma(int H1, int H2)
{
    const size_t SH = h1_pitch(H1);
    return 2 * SH * (H2 + kT) + 2 * (size_t)kT * (H2 + 8) + sizeof(float) * ((size_t)H2 + (size_t)kTS * (H1 + H2)) +
           3 * sizeof(int32_t) * kT;
}

template <typename Op>
int fwd_pass(const EdgePassArgs &a, int nblk, float *partial, hipStream_t st)
{
    const size_t lds = fwd_lds_bytes_mma(a.H1, a.H2);
    int rc = 0;
    with_int<32, 64, 128>(a.H2, [&](auto h2) {
        constexpr int kH2 = decltype(h2)::value;
        static size_t granted = 0;
        rc = grant_lds(edge_mlp_fwd_mma_kernel<Op, kH2>, lds, granted, "hipFuncSetAttribute(edge_mlp_fwd_mma_kernel)");
        if (rc == 0)
            hipLaunchKernelGGL((edge_mlp_fwd_mma_kernel<Op, kH2>), dim3(nblk), dim3(kBlk), lds, st, a.pq, a.rowptr, a.src, a.tgt,
                               a.N, a.E, a.H1, a.W2, a.b2, a.act2, a.aggr, a.bn, a.agg, a.win, partial);
    });
    return rc;
}

template <typename Op>
int bwd_pass(const EdgePassArgs &a, bool by_src, int nblk, float *partial, hipStream_t st)
{
    const size_t lds = bwd_lds_bytes_mma(a.H1, a.H2);
    const int32_t *optr = by_src ? a.srcptr : a.rowptr, *perm = by_src ? a.srcperm : nullptr;
    int rc = 0;
    with_int<32, 64, 128>(a.H2, [&](auto h2) {
        with_flags([&](auto bs) {
            constexpr int kH2 = decltype(h2)::value;
            static size_t granted = 0;
            rc = grant_lds(edge_mlp_bwd_mma_kernel<Op, kH2, bs()>, lds, granted, "hipFuncSetAttribute(edge_mlp_bwd_mma_kernel)");
            if (rc == 0)
                hipLaunchKernelGGL((edge_mlp_bwd_mma_kernel<Op, kH2, bs()>), dim3(nblk), dim3(kBlk), lds, st, a.pq, a.rowptr, optr,
                                   perm, a.src, a.tgt, a.N, a.E, a.H1, a.W2, a.b2, a.act2, a.aggr, a.bn, a.g_out, a.cwin, a.bnstat,
                                   a.coef, a.gpq, partial);
        }, by_src);
    });
    return rc;
}

}  // namespace

int edge_mlp_fwd_pass_mma(const EdgePassArgs &a, EdgePrec prec, int nblk, float *partial, hipStream_t st)
{
    if (int rc = prec == EdgePrec::f16 ? fwd_pass<OpF16>(a, nblk, partial, st) : fwd_pass<OpBf16>(a, nblk, partial, st))
        return rc;
    DMET_LAUNCH_CHECK(prec == EdgePrec::f16 ? "edge_mlp_fwd_mma_kernel (f16)" : "edge_mlp_fwd_mma_kernel (bf16)");
    return 0;
}

int edge_mlp_bwd_pass_mma(const EdgePassArgs &a, EdgePrec prec, bool by_src, int nblk, float *partial, hipStream_t st)
{
    if (int rc = prec == EdgePrec::f16 ? bwd_pass<OpF16>(a, by_src, nblk, partial, st)
                                       : bwd_pass<OpBf16>(a, by_src, nblk, partial, st))
        return rc;
    DMET_LAUNCH_CHECK(by_src ? "edge_mlp_bwd_mma_kernel (by source)" : "edge_mlp_bwd_mma_kernel (by target)");
    return 0;
}

}  // namespace dmet

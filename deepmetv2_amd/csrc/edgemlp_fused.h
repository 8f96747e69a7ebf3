// edgemlp_fused.h -- what the fused edge-MLP routes over a grouped edge list share: the fp32 route (edgemlp_f32.hip),
// which owns the node-level kernels, every entry point and the host orchestration, and the bf16 / fp16 matrix-core
// routes (edgemlp_bf16.hip), which bring their own two edge passes.  The device pieces here are parts of the edge passes
// that do not depend on the tile geometry: the fp32 kernels (EdgeTile<H2>) and the matrix-core ones (kT) hand their T in.
// The two per-thread folds over a tile's edges (the forward's running aggregate, the backward's owner sums) stay written
// out in each kernel: behind a function (a struct with inline members, or free functions over references) their
// loop-carried state is promoted to registers one pass later and the tile loop comes out in another form (DESIGN.md,
// "K2 host path", has what was tried).
#pragma once

#include "common.h"

namespace dmet {
namespace {

constexpr int kBlk = 256;     // threads per workgroup of the edge passes
constexpr int kMaxBlocks = 512;

__device__ __forceinline__ float elu1f(float z) { return z > 0.0f ? z : expm1f(z); }

// first node of workgroup b's range: the first i with rowptr[i] >= b E / nblk (rowptr non-decreasing, rowptr[N] = E)
__device__ __forceinline__ int64_t range_start(const int32_t *__restrict__ rowptr, int64_t N, int64_t E, int b, int nblk)
{
    if (b >= nblk) return N;
    const int64_t target = (int64_t)b * E / nblk;
    int64_t lo = 0, hi = N;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)rowptr[mid] >= target) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// per-node g_y weight of an edge (sum 1, mean 1 / deg) and, for max, the winner array in use
__device__ __forceinline__ float gy_of(const float *__restrict__ g_out, const int32_t *__restrict__ rowptr,
                                       const int32_t *__restrict__ winsel, int aggr, int64_t tnode, int H2, int o, int32_t e)
{
    const int64_t q = tnode * H2 + o;
    const float go = g_out[q];
    if (aggr == 0) return winsel[q] == e ? go : 0.0f;
    if (aggr == 2) return go / (float)(rowptr[tnode + 1] - rowptr[tnode]);
    return go;
}

// Backward: ids of a tile's edges into LDS (beyond cnt: 0) -- the grouped position ep of each edge, which by source
// (BY_SRC) is perm[pt + t], and its target and source.  (The forward's two-line load of tgt / src at pt + t stays in its
// kernels: through this function its two address computations come out in the other order.)
template <int T, bool BY_SRC>
__device__ __forceinline__ void load_tile_ids(const int32_t *src, const int32_t *tgt, const int32_t *perm, int64_t pt, int cnt,
                                              int32_t *tg, int32_t *sr, int32_t *ep)
{
    for (int t = threadIdx.x; t < T; t += blockDim.x) {
        const int32_t e = t < cnt ? (BY_SRC ? perm[pt + t] : (int32_t)(pt + t)) : 0;
        ep[t] = e;
        tg[t] = t < cnt ? tgt[e] : 0;
        sr[t] = t < cnt ? src[e] : 0;
    }
}

// g_z2 of one (edge, channel o) from the re-computed pre-activation z: g_y through the BatchNorm backward (bn == 1: batch
// terms, bn == 2: the scale alone) and ELU'.  The constants are channel o's.
template <int H2>
struct Gz2 {
    float ka, k1, k2, bmean, binv;
    const int32_t *winsel;     // max: the winners in use (those of the min where the BatchNorm scale is < 0)

    __device__ __forceinline__ Gz2(const float *coef, const float *bnstat, const int32_t *win, int64_t N, int aggr, int bn, int o)
        : ka(coef[o]), k1(coef[H2 + o]), k2(coef[2 * H2 + o]), bmean(bnstat[2 * H2 + o]), binv(bnstat[3 * H2 + o]),
          winsel(win + ((aggr == 0 && bn != 0 && ka < 0.0f) ? N * H2 : 0)) {}

    // tg[t], ep[t]: the edge's target and grouped position, read from the tile's LDS ids after the ELU as the kernels did
    __device__ __forceinline__ float operator()(float z, const float *g_out, const int32_t *rowptr, int act2, int aggr, int bn,
                                                const int32_t *tg, const int32_t *ep, int t, int o) const
    {
        const float m = act2 ? elu1f(z) : z;
        const float gy = gy_of(g_out, rowptr, winsel, aggr, tg[t], H2, o, ep[t]);
        float gm = gy;
        if (bn == 1) gm = ka * (gy - k1 - (m - bmean) * binv * k2);
        else if (bn == 2) gm = ka * gy;
        return act2 ? gm * (z > 0.0f ? 1.0f : m + 1.0f) : gm;
    }
};

inline int edge_blocks(int64_t E)
{
    int64_t nb = (E + 2047) / 2048;
    if (nb < 1) nb = 1;
    return (int)(nb > kMaxBlocks ? kMaxBlocks : nb);
}

// dynamic LDS above 64 KB must be granted per kernel (hidden 128: up to 141 KB); remembered per instantiation
template <typename K>
int grant_lds(K kernel, size_t lds, size_t &granted, const char *what)
{
    if (lds <= 65536 || lds <= granted) return 0;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return hip_fail(e, what);
    granted = lds;
    return 0;
}

}  // namespace

// Arguments of one edge pass, filled once by the entry point (coef: by the backward, from its workspace); the forward
// pass reads the first block, the backward passes all of it.
struct EdgePassArgs {
    const float *pq;
    const int32_t *rowptr, *src, *tgt;
    int64_t N, E;
    int H1, H2;
    const float *W2, *b2;
    int act2, aggr, bn;
    // forward
    float *agg;
    int32_t *win;
    // backward
    const int32_t *srcptr, *srcperm;
    const float *g_out, *bnstat, *coef;
    const int32_t *cwin;
    float *gpq;
};

// operand type of the per-edge products: fp32 VALU (edgemlp_f32.hip), bf16 or fp16 matrix cores (edgemlp_bf16.hip)
enum class EdgePrec { f32, bf16, f16 };

// matrix-core edge passes (edgemlp_bf16.hip, prec bf16 or f16): launch on `st` over nblk workgroups; 0 or a dmet error code
int edge_mlp_fwd_pass_mma(const EdgePassArgs &a, EdgePrec prec, int nblk, float *partial, hipStream_t st);
int edge_mlp_bwd_pass_mma(const EdgePassArgs &a, EdgePrec prec, bool by_src, int nblk, float *partial, hipStream_t st);

}  // namespace dmet

// edgemlp_fused.h -- what the fused edge-MLP routes over a grouped edge list share: the fp32 route (edgemlp_f32.hip),
// which owns the node-level kernels and the host orchestration, and the bf16 / fp16 matrix-core routes
// (edgemlp_bf16.hip), which bring their own two edge passes.
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

// Arguments of one edge pass; the forward pass reads the first block, the backward passes all of it.
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

// host orchestration of every route (edgemlp_f32.hip): the entry points of include/dmet.h with the route chosen by prec
int edge_mlp_fwd(const char *fn, EdgePrec prec, const float *x, int64_t N, int Hin, const int32_t *rowptr, const int32_t *src,
                 const int32_t *tgt, int64_t E, const float *W1, const float *b1, int H1, const float *W2, const float *b2,
                 int H2, int act2, int aggr, int bn, const float *gamma, const float *beta, float eps, float momentum,
                 float *running_mean, float *running_var, int64_t *num_batches_tracked, float *out, float *pq, float *agg,
                 int32_t *win, float *bnstat, void *ws, size_t ws_bytes, dmet_stream_t stream);
int edge_mlp_bwd(const char *fn, EdgePrec prec, const float *x, int64_t N, int Hin, const int32_t *rowptr, const int32_t *src,
                 const int32_t *tgt, int64_t E, const int32_t *srcptr, const int32_t *srcperm, const float *W1, int H1,
                 const float *W2, const float *b2, int H2, int act2, int aggr, int bn, const float *pq, const float *agg,
                 const int32_t *win, const float *bnstat, const float *g_out, float *gx, float *gpq, float *gW2,
                 float *gb2, float *ggamma, float *gbeta, void *ws, size_t ws_bytes, dmet_stream_t stream);

}  // namespace dmet

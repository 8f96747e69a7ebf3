// bn_affine.h -- the BatchNorm transform of the per-node chain, written once:
//   y  = (raw - mean) * (gamma * invstd) + beta (+ res),   gx = gamma * invstd * (g - mean_g - (x - mean) * invstd * mean_gx)
// bn_apply_kernel / bn_bwd_apply_kernel (norm.hip) and every kernel that carries the transform for its consumer (the kNN
// prep launch, the node-level dense layer, the head's forward, the encoder's backward) call these functions, so all of
// them give the same bits by construction: with -ffp-contract=off the fp32 operations and their order are the ones below.
#pragma once
#include "common.h"

namespace dmet {
namespace {

// The operands of the forward transform; raw == nullptr: none.
struct BnAffine {
    const float *raw = nullptr, *res = nullptr, *gamma = nullptr, *beta = nullptr, *mean = nullptr, *invstd = nullptr;
};

// The six pointers and the output y are 16-byte aligned (a null res is accepted).
inline bool bn_affine_aligned16(const BnAffine &a, const void *y)
{
    return aligned16(a.raw) && aligned16(y) && aligned16(a.gamma) && aligned16(a.beta) && aligned16(a.mean) &&
           aligned16(a.invstd) && aligned16(a.res);
}

// The forward constants of the four channels 4 c4 .. 4 c4 + 3.
struct BnAffine4 { float4 mu, scale, beta; };

__device__ __forceinline__ BnAffine4 bn_affine_load4(const BnAffine &a, int c4)
{
    const float4 ga = reinterpret_cast<const float4 *>(a.gamma)[c4], is = reinterpret_cast<const float4 *>(a.invstd)[c4];
    return BnAffine4{reinterpret_cast<const float4 *>(a.mean)[c4], make_float4(ga.x * is.x, ga.y * is.y, ga.z * is.z, ga.w * is.w),
                     reinterpret_cast<const float4 *>(a.beta)[c4]};
}

__device__ __forceinline__ float4 bn_affine4(float4 v, float4 mu, float4 scale, float4 beta)
{
    return make_float4((v.x - mu.x) * scale.x + beta.x, (v.y - mu.y) * scale.y + beta.y, (v.z - mu.z) * scale.z + beta.z,
                       (v.w - mu.w) * scale.w + beta.w);
}

__device__ __forceinline__ float4 bn_add4(float4 v, float4 r) { return make_float4(v.x + r.x, v.y + r.y, v.z + r.z, v.w + r.w); }

// The backward transform of one element (training-mode batch statistics) and of four channels.
__device__ __forceinline__ float bn_bwd1(float g, float x, float gamma, float mean, float invstd, float mean_g, float mean_gx)
{
    return gamma * invstd * (g - mean_g - (x - mean) * invstd * mean_gx);
}

__device__ __forceinline__ float4 bn_bwd4(float4 g, float4 x, float4 ga, float4 mu, float4 is, float4 mg, float4 mx)
{
    return make_float4(bn_bwd1(g.x, x.x, ga.x, mu.x, is.x, mg.x, mx.x), bn_bwd1(g.y, x.y, ga.y, mu.y, is.y, mg.y, mx.y),
                       bn_bwd1(g.z, x.z, ga.z, mu.z, is.z, mg.z, mx.z), bn_bwd1(g.w, x.w, ga.w, mu.w, is.w, mg.w, mx.w));
}

}  // namespace
}  // namespace dmet

// knn_common.h -- what the kNN build (knn.hip) and the radius graph (radius.hip) share: the wavefront hand-off, the
// optional trailing argument pack of their kernels (periods, a second point set), its host-side choice and the check of
// a caller's periods.
#pragma once
#include <type_traits>

#include "common.h"

namespace dmet {
namespace {

typedef float f2 __attribute__((ext_vector_type(2)));

// LDS hand-off between the lanes of ONE wavefront: LDS requests of a wave execute in order, so only the compiler
// has to be kept from moving accesses across this point (no workgroup barrier: the group's waves are independent).
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Periodic coordinates (radius_graph / knn_graph(..., period=)): L[c] is the circumference of coordinate c, passed to
// the kernel BY VALUE (a captured graph replays the periods of its capture).  The host turns "not periodic" into L = +inf.
// The contract wraps the fp32 difference d as  a = |d|;  a = (a > L/2) ? L - a : a.  The kernels form the same value
// as  min(|d|, L - |d|):  for a > L/2, L - a < a so fp32(L - a) <= a; for a <= L/2, L - a >= L/2 >= a so fp32(L - a) >= a
// (rounding is monotone, L/2 is exact); NaN stays NaN, |d| = inf gives L - inf = -inf.  With L = +inf the result is
// |d| for every d (inf - inf = NaN loses to |d| = inf in min), so a plain coordinate keeps its bits.
struct RadPeriod { float L[8]; };

// the periods ride as an optional trailing kernel argument: an empty pack is the plain kernel (same arguments, same
// code as without periods), Per = RadPeriod wraps every coordinate c with L[c]
__device__ __forceinline__ RadPeriod rad_periods() { return RadPeriod{}; }
__device__ __forceinline__ RadPeriod rad_periods(const RadPeriod &p) { return p; }

// Two point sets (dmet_knn_xy_f32 / dmet_radius_xy_f32) ride the same way, after the periods: with a KnnQuerySet in the
// pack the QUERY rows and their events come from it and the kernel's x / ptr are the candidates alone; without one both
// sides are x / ptr, and the kernel is the one-set kernel, argument for argument and instruction for instruction.
struct KnnQuerySet { const float *qx; const int64_t *qptr; };
__device__ __forceinline__ RadPeriod rad_periods(const KnnQuerySet &) { return RadPeriod{}; }
__device__ __forceinline__ RadPeriod rad_periods(const RadPeriod &p, const KnnQuerySet &) { return p; }
__device__ __forceinline__ KnnQuerySet query_set(const float *x, const int64_t *ptr) { return KnnQuerySet{x, ptr}; }
__device__ __forceinline__ KnnQuerySet query_set(const float *x, const int64_t *ptr, const RadPeriod &) { return KnnQuerySet{x, ptr}; }
__device__ __forceinline__ KnnQuerySet query_set(const float *, const int64_t *, const KnnQuerySet &q) { return q; }
__device__ __forceinline__ KnnQuerySet query_set(const float *, const int64_t *, const RadPeriod &, const KnnQuerySet &q) { return q; }
template <typename T, typename... Pack>
constexpr bool pack_has = (std::is_same<T, Pack>::value || ...);

// Host side of the trailing pack: calls launch(pack...) with the pack that per / qs ask for -- (), (*per), (*qs) or
// (*per, *qs) -- so that a kernel's ladder over its pack is written once, as a generic lambda that names the kernel with
// decltype(pack)....  PER / QS = false: the kernel has no such instances, and none is made (the entries have refused the
// request before).
template <bool PER, bool QS, typename Launch>
inline void with_pack(const RadPeriod *per, const KnnQuerySet *qs, Launch &&launch)
{
    if (per) {
        if constexpr (PER) {
            if (!qs) launch(*per);
            else if constexpr (QS) launch(*per, *qs);
        }
    } else if (qs) {
        if constexpr (QS) launch(*qs);
    } else {
        launch();
    }
}

// Periodic coordinates (train.py:47-48: phi wraps at +-pi).  period[c] > 0: circumference of coordinate c; 0: plain.
// Host-side check of the D periods; *any = some coordinate is periodic.  per gets +inf for the plain ones (and for
// the padding coordinates c >= D), which the kernels' wrap turns into the identity.
inline int radius_periods(const char *who, int D, const float *period, RadPeriod *per, bool *any)
{
    DMET_REQUIRE(D >= 1 && D <= 8, "%s: D=%d not in [1,8]", who, D);
    DMET_REQUIRE(period, "%s: null period", who);
    *any = false;
    for (int c = 0; c < 8; ++c) per->L[c] = __builtin_inff();
    for (int c = 0; c < D; ++c) {
        const float L = period[c];
        DMET_REQUIRE(L == L && L >= 0.0f && L < __builtin_inff(), "%s: period[%d]=%g is not 0 or a positive finite number",
                     who, c, (double)L);
        if (L > 0.0f) { per->L[c] = L; *any = true; }
    }
    return 0;
}

}  // namespace
}  // namespace dmet

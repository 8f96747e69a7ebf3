// event_wg.h -- the skeleton of the kernels that give every event of a batch one workgroup and the whole batch one launch
// (select.hip topk_kernel, voxel.hip, edge_match.hip, components.hip, condense.hip): the event's node and edge ranges,
// the nodes no event owns, its state words in LDS or in the workspace, and the workgroup's count-and-rank scan.
#pragma once
#include "common.h"

namespace dmet {

// Event b's nodes [lo, hi), n = hi - lo of them, with ptr clamped to 0 <= lo <= hi <= N: whatever ptr holds, no node
// outside [0, N) is touched.  Uniform over the workgroup.
struct EventRange {
    int64_t lo, hi, n;
};

__device__ __forceinline__ EventRange event_range(const int64_t *__restrict__ ptr, int b, int64_t N)
{
    int64_t lo = ptr[b], hi = ptr[b + 1];
    lo = lo < 0 ? 0 : (lo > N ? N : lo);
    hi = hi < lo ? lo : (hi > N ? N : hi);
    return {lo, hi, hi - lo};
}

// f(i) for the nodes no event owns (ptr[0] > 0, ptr[B] < N): the first workgroup takes those before its event, the last
// those after its own, kThreads threads each.
template <int kThreads, typename F>
__device__ __forceinline__ void for_unowned(const EventRange &ev, int b, int B, int64_t N, F &&f)
{
    if (b == 0)
        for (int64_t i = threadIdx.x; i < ev.lo; i += kThreads) f(i);
    if (b == B - 1)
        for (int64_t i = ev.hi + threadIdx.x; i < N; i += kThreads) f(i);
}

// The positions e0 <= e1 of the event's rows in a by-target list of E entries, clamped to [0, E] like the nodes.
__device__ __forceinline__ void edge_range(const int32_t *__restrict__ rowptr, const EventRange &ev, int64_t E, int64_t &e0,
                                           int64_t &e1)
{
    int64_t lo = rowptr[ev.lo], hi = rowptr[ev.hi];
    lo = lo < 0 ? 0 : (lo > E ? E : lo);
    hi = hi < lo ? lo : (hi > E ? E : hi);
    e0 = lo, e1 = hi;
}

// ---- state words ---------------------------------------------------------------------------------------------------------
// One word per node (int32_t in components.hip and condense.hip; edge_match.hip's uint64_t words keep accessors of their
// own, DESIGN.md says why), read and written by any thread of the event's workgroup between barriers: relaxed atomics, so
// a word racing with its own update is the old or the new value.  In LDS (kGlobal false) workgroup scope: plain ds
// instructions.  In the workspace both sides must go to L2 (agent scope): the maxima, sums and swaps are formed there,
// and a load served by the CU's L1 could return the word as it was before another wavefront's store or atomic.
template <bool kGlobal, typename T>
__device__ __forceinline__ T state_load(const T *p)
{
    if (kGlobal) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
template <bool kGlobal, typename T>
__device__ __forceinline__ void state_store(T *p, T v)
{
    if (kGlobal) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
// true: *p was `expect` and is now `v`
template <bool kGlobal, typename T>
__device__ __forceinline__ bool state_cas(T *p, T expect, T v)
{
    if (kGlobal)
        return __hip_atomic_compare_exchange_strong(p, &expect, v, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                    __HIP_MEMORY_SCOPE_AGENT);
    return __hip_atomic_compare_exchange_strong(p, &expect, v, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                __HIP_MEMORY_SCOPE_WORKGROUP);
}
template <bool kGlobal, typename T>
__device__ __forceinline__ void state_max(T *p, T v)
{
    if (kGlobal) __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
template <bool kGlobal, typename T>
__device__ __forceinline__ void state_add(T *p, T v)
{
    if (kGlobal) __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// ---- lanes and wavefronts ------------------------------------------------------------------------------------------------
// The ballot bits of the lanes before `lane` (0 .. 63).
__device__ __forceinline__ uint64_t lanes_below(int lane) { return (1ull << lane) - 1ull; }

// LDS written by some lanes of a wavefront and read by others of the same one: the ds queue of a wavefront is in order,
// the fences keep the compiler from moving the accesses across.
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Count and rank over a workgroup of kWaves wavefronts, every thread calling: before = the flagged threads with a lower
// threadIdx.x, total = all of them.  One ballot per wavefront, its count in wsum[wave], one barrier.  The caller owns the
// barrier between this call's reads of wsum[kWaves] and the next write to it.
template <int kWaves>
__device__ __forceinline__ void wg_rank(bool flag, int *wsum, int &before, int &total)
{
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const uint64_t mask = __ballot(flag);
    if (lane == 0) wsum[wave] = __popcll(mask);
    __syncthreads();
    before = __popcll(mask & lanes_below(lane));
    total = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        const int c = wsum[w];
        before += w < wave ? c : 0;
        total += c;
    }
}

// Host: the largest event whose state words stay in LDS: lds_nodes, or the array's size `cap` for 0 and for more.
static inline int lds_limit(int lds_nodes, int cap) { return lds_nodes == 0 || lds_nodes > cap ? cap : lds_nodes; }

}  // namespace dmet

// edge_match.hip -- greedy edge contraction as a matching of locally dominant edges (torch_geometric's
// EdgePooling._merge_edges).  Semantics: include/dmet.h, section "Edge pooling".
#include "event_wg.h"
#include "score_key.h"

namespace dmet {
namespace {

constexpr int kMatchThreads = DMET_EDGE_MATCH_THREADS;

// Node state of one event (local indices), one 64-bit word per node: kFree between rounds, the largest key offered in
// the running round, or kClaimed for good.  Both small words lie below every key (score_key.h).
constexpr uint64_t kFree = 0ull, kClaimed = 1ull;

enum { kFlagRange = 0, kFlagCross = 1, kFlagRounds = 2 };

// The state words in LDS are plain ds accesses.  In the workspace they go to L2 (agent scope): the maxima are formed
// there by the atomics, and a load served by the CU's L1 could return the word as it was before them.
template <bool kGlobal>
__device__ __forceinline__ uint64_t st_load(const uint64_t *p)
{
    if (kGlobal) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return *p;
}
template <bool kGlobal>
__device__ __forceinline__ void st_store(uint64_t *p, uint64_t v)
{
    if (kGlobal) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else *p = v;
}
template <bool kGlobal>
__device__ __forceinline__ void st_max(uint64_t *p, uint64_t v)
{
    if (kGlobal) __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// The lists of live edges live in the workspace (either state form) and are read by other wavefronts than wrote them:
// both sides go to L2, as the state words of the workspace form do.
__device__ __forceinline__ int32_t list_load(const int32_t *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void list_store(int32_t *p, int32_t v)
{
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// All rounds of one event.  A round: (1) every live edge -- both ends free -- offers its key to both ends, an integer
// max per node, and is appended to the round's list; (2) an edge of that list that finds its own key at both ends is
// taken: it writes the outputs of its ends and claims them; (3) the words of the nodes still free are cleared.  Phase 1
// walks the list of the round before (round 0: the event's positions e0 .. e1), so an edge is visited while it is live
// and once more: the work is the sum of the live counts, not rounds x edges.  A wavefront reserves its list slots with
// one LDS add; the order of a list depends on which wavefront came first, the SET does not, and nothing reads the order.
// Keys are distinct, so at most one edge finds its key at a node, every output element has one writer per round, and
// nothing depends on the order lanes run in.  The largest live key of an event is the largest at both of its ends: every
// round with a live edge takes one, so the loop's bound of n + 1 rounds is never reached (a taken edge claims at least
// one of the n nodes).
template <bool kGlobal>
__device__ __forceinline__ void match_event(uint64_t *best, unsigned *cnt, int32_t *list_a, int32_t *list_b,
                                            const int32_t *__restrict__ src, const int32_t *__restrict__ tgt,
                                            const int32_t *__restrict__ perm, const float *__restrict__ score, int64_t e0,
                                            int64_t e1, int64_t lo, int64_t n, int64_t N, int64_t *__restrict__ cluster,
                                            int32_t *__restrict__ partner, int64_t *__restrict__ edge,
                                            int32_t *__restrict__ rounds, int32_t *__restrict__ flags, int b)
{
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    for (int64_t i = tid; i < n; i += kMatchThreads) {
        st_store<kGlobal>(best + i, kFree);
        cluster[lo + i] = lo + i;
        partner[lo + i] = -1;
        edge[lo + i] = -1;
    }
    if (tid < 2) cnt[tid] = 0;
    __syncthreads();

    int32_t *prev = nullptr, *next = list_a;        // prev == nullptr: the positions e0 .. e1 themselves
    int64_t m = e1 - e0;                            // entries of prev
    int cur = 0;
    int range = 0, cross = 0;                       // the edges that are no candidates, met in round 0
    int64_t r = 0;
    bool open = true;       // a live edge was left when the loop ended: only by its bound
    for (; r < n + 1; ++r) {
        for (int64_t i0 = 0; i0 < m; i0 += kMatchThreads) {         // uniform over the wavefront: the ballot below
            const int64_t i = i0 + tid;
            bool live = false;
            int64_t e = 0;
            if (i < m) {
                e = prev ? (int64_t)list_load(prev + i) : e0 + i;
                const int64_t sg = src[e], tg = tgt[e], s = sg - lo, t = tg - lo;
                if (s < 0 || s >= n || t < 0 || t >= n) {
                    if (sg < 0 || sg >= N || tg < 0 || tg >= N) range = 1;
                    else cross = 1;
                } else if (st_load<kGlobal>(best + s) != kClaimed && st_load<kGlobal>(best + t) != kClaimed) {
                    live = true;
                    const uint64_t key = select_key(score[e], (uint32_t)(perm ? perm[e] : (int32_t)e));
                    st_max<kGlobal>(best + s, key);
                    if (t != s) st_max<kGlobal>(best + t, key);
                }
            }
            const uint64_t mask = __ballot(live);
            if (mask) {
                const int leader = __ffsll((unsigned long long)mask) - 1;
                unsigned off = 0;
                if (lane == leader) off = atomicAdd(&cnt[cur], (unsigned)__popcll(mask));
                off = __shfl(off, leader, kWave);
                if (live) list_store(next + off + __popcll(mask & lanes_below(lane)), (int32_t)e);
            }
        }
        __syncthreads();
        const int64_t count = cnt[cur];
        if (count == 0) {                                           // uniform over the workgroup
            open = false;
            break;
        }
        for (int64_t i = tid; i < count; i += kMatchThreads) {
            const int64_t e = list_load(next + i);
            const int64_t s = (int64_t)src[e] - lo, t = (int64_t)tgt[e] - lo;
            // a reader may meet kClaimed here, written by the edge that took the node in this very phase: no key either
            const uint64_t bs = st_load<kGlobal>(best + s);
            if (bs <= kClaimed) continue;
            const int32_t id = perm ? perm[e] : (int32_t)e;
            const uint64_t key = select_key(score[e], (uint32_t)id);
            if (bs != key || st_load<kGlobal>(best + t) != key) continue;
            const int64_t u = lo + s, v = lo + t;
            edge[u] = id;
            st_store<kGlobal>(best + s, kClaimed);
            if (t != s) {
                edge[v] = id;
                partner[u] = (int32_t)v;
                partner[v] = (int32_t)u;
                cluster[u < v ? v : u] = u < v ? u : v;
                st_store<kGlobal>(best + t, kClaimed);
            }
        }
        if (tid == 0) cnt[cur ^ 1] = 0;         // the next round's counter: last read before this round's phase 1
        __syncthreads();
        for (int64_t i = tid; i < n; i += kMatchThreads)
            if (st_load<kGlobal>(best + i) != kClaimed) st_store<kGlobal>(best + i, kFree);
        __syncthreads();
        prev = next;
        next = next == list_a ? list_b : list_a;
        m = count;
        cur ^= 1;
    }
    if (range) atomicOr(&flags[kFlagRange], 1);
    if (cross) atomicOr(&flags[kFlagCross], 1);
    if (tid == 0) {
        if (rounds) rounds[b] = (int32_t)(r > INT32_MAX ? INT32_MAX : r);
        if (open) atomicOr(&flags[kFlagRounds], 1);
    }
}

// An event of up to lds_nodes <= DMET_EDGE_MATCH_LDS_NODES nodes keeps its state words in LDS (128 KiB); a larger one
// keeps them in the caller's workspace at ws[lo ..): the events' ranges are disjoint.  The two lists of live edges follow
// the N state words in the workspace, E entries each, an event's at its own positions e0 .. e1.  Nodes no event owns are
// clusters of their own, unclaimed.
__global__ __launch_bounds__(kMatchThreads) void edge_match_kernel(
    const int32_t *__restrict__ rowptr, const int32_t *__restrict__ src, const int32_t *__restrict__ tgt,
    const int32_t *__restrict__ perm, const float *__restrict__ score, const int64_t *__restrict__ ptr, int B, int64_t N,
    int64_t E, int64_t *__restrict__ cluster, int32_t *__restrict__ partner, int64_t *__restrict__ edge,
    int32_t *__restrict__ rounds, int32_t *__restrict__ flags, uint64_t *ws, int lds_nodes)
{
    __shared__ uint64_t lds[DMET_EDGE_MATCH_LDS_NODES];
    __shared__ unsigned cnt[2];
    const int b = blockIdx.x;
    const EventRange ev = event_range(ptr, b, N);
    for_unowned<kMatchThreads>(ev, b, B, N, [&](int64_t i) {
        cluster[i] = i;
        partner[i] = -1;
        edge[i] = -1;
    });
    const int64_t lo = ev.lo, n = ev.n;
    if (n <= 0) {                                           // uniform over the workgroup
        if (rounds && threadIdx.x == 0) rounds[b] = 0;
        return;
    }
    int64_t e0, e1;
    edge_range(rowptr, ev, E, e0, e1);
    int32_t *list_a = (int32_t *)(ws + N) + e0, *list_b = (int32_t *)(ws + N) + E + e0;
    if (n <= lds_nodes)
        match_event<false>(lds, cnt, list_a, list_b, src, tgt, perm, score, e0, e1, lo, n, N, cluster, partner, edge, rounds,
                           flags, b);
    else
        match_event<true>(ws + lo, cnt, list_a, list_b, src, tgt, perm, score, e0, e1, lo, n, N, cluster, partner, edge,
                          rounds, flags, b);
}

}  // namespace
}  // namespace dmet

using namespace dmet;

extern "C" size_t dmet_edge_match_workspace_bytes(int64_t N, int64_t E)
{
    if (N <= 0) return 0;
    return (size_t)N * sizeof(uint64_t) + 2 * (size_t)(E > 0 ? E : 0) * sizeof(int32_t);
}

extern "C" int dmet_edge_match_f32(const int32_t *rowptr, const int32_t *src, const int32_t *tgt, const int32_t *perm,
                                   const float *score, int64_t E, const int64_t *ptr, int B, int64_t N, int64_t *cluster,
                                   int32_t *partner, int64_t *edge, int32_t *rounds, int32_t *flags, void *ws,
                                   size_t ws_bytes, dmet_stream_t stream)
{
    DMET_REQUIRE(N >= 0 && N <= INT32_MAX, "dmet_edge_match_f32: N=%lld outside 0..2^31-1", (long long)N);
    DMET_REQUIRE(E >= 0 && E <= INT32_MAX, "dmet_edge_match_f32: E=%lld outside 0..2^31-1", (long long)E);
    DMET_REQUIRE(B >= 0, "dmet_edge_match_f32: B=%d < 0", B);
    DMET_REQUIRE(flags, "dmet_edge_match_f32: flags is NULL");
    const hipError_t me = hipMemsetAsync(flags, 0, 3 * sizeof(int32_t), as_stream(stream));
    if (me != hipSuccess) return hip_fail(me, "hipMemsetAsync(flags)");
    if (B == 0 || N == 0) {                                 // no event owns a node: no launch, every event ran 0 rounds
        if (rounds && B > 0) {
            const hipError_t re = hipMemsetAsync(rounds, 0, (size_t)B * sizeof(int32_t), as_stream(stream));
            if (re != hipSuccess) return hip_fail(re, "hipMemsetAsync(rounds)");
        }
        return 0;
    }
    DMET_REQUIRE(ws_bytes >= dmet_edge_match_workspace_bytes(N, E),
                 "dmet_edge_match_f32: ws_bytes=%zu, dmet_edge_match_workspace_bytes asks for %zu", ws_bytes,
                 dmet_edge_match_workspace_bytes(N, E));
    DMET_REQUIRE(rowptr, "dmet_edge_match_f32: rowptr is NULL");
    DMET_REQUIRE(ptr, "dmet_edge_match_f32: ptr is NULL");
    DMET_REQUIRE((src && tgt && score) || E == 0, "dmet_edge_match_f32: src, tgt or score is NULL");
    DMET_REQUIRE(cluster, "dmet_edge_match_f32: cluster is NULL");
    DMET_REQUIRE(partner, "dmet_edge_match_f32: partner is NULL");
    DMET_REQUIRE(edge, "dmet_edge_match_f32: edge is NULL");
    DMET_REQUIRE(ws, "dmet_edge_match_f32: ws is NULL");
    // DMET_EDGE_MATCH_STATE=workspace: every event through the workspace form (the tests hold both forms to the same bits)
    const int lds_nodes = env_is("DMET_EDGE_MATCH_STATE", "workspace") ? 0 : DMET_EDGE_MATCH_LDS_NODES;
    hipLaunchKernelGGL(edge_match_kernel, dim3((unsigned)B), dim3(kMatchThreads), 0, as_stream(stream), rowptr, src, tgt,
                       perm, score, ptr, B, N, E, cluster, partner, edge, rounds, flags, (uint64_t *)ws, lds_nodes);
    DMET_LAUNCH_CHECK("edge_match_kernel");
    return 0;
}

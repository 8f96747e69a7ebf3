// components.hip -- connected components and DBSCAN of every event of a batch as one union-find launch.
// Semantics: include/dmet.h, section "Components and DBSCAN".
#include "event_wg.h"

namespace dmet {
namespace {

constexpr int kCompThreads = DMET_COMPONENTS_THREADS;
constexpr int kCompWaves = kCompThreads / kWave;

// One parent word per node (event-local ids).  A word >= 0 is a node that takes part in the unions: its parent, itself
// for a root; a parent is never larger than its child, so the root of a finished component is its smallest id.  DBSCAN
// mode keeps the nodes that are not core below zero: kNoise, or -1 - r once the border pass met a core neighbour with
// root r (an integer max per node: the smallest root wins).
constexpr int32_t kNoise = INT32_MIN;

enum { kFlagRange = 0, kFlagCross = 1, kFlagBound = 2, kFlagFull = 3, kNumFlags = 4 };

// The parent words are the state words of event_wg.h: the hooks are formed by its compare-and-swap.

// The root of x, halving the path on the way.  A parent is smaller than its child, so x falls with every step and the n
// steps of the bound are never used up; should they be, `bound` is set and the caller stops.  The halving store writes
// an ancestor of x over an ancestor of x: whichever of two racing stores lands, the word stays one.  A root's word is
// only ever changed by the hook's compare-and-swap.
template <bool kGlobal, bool kHalve = true>
__device__ __forceinline__ int32_t uf_find(int32_t *p, int32_t x, int64_t n, bool &bound)
{
    for (int64_t step = 0; step < n; ++step) {
        const int32_t px = state_load<kGlobal>(p + x);
        if (px == x) return x;
        const int32_t gp = state_load<kGlobal>(p + px);
        if (kHalve && gp != px) state_store<kGlobal>(p + x, gp);
        x = gp;
    }
    bound = true;
    return x;
}

// Join the components of a and b: the larger root is hooked under the smaller by a compare-and-swap that only a root
// passes.  A failed swap means another lane hooked that root in between; an event has fewer than n successful hooks, so
// the n + 1 tries of the bound are never used up.
template <bool kGlobal>
__device__ __forceinline__ void uf_union(int32_t *p, int32_t a, int32_t b, int64_t n, bool &bound)
{
    for (int64_t t = 0; t < n + 1; ++t) {
        a = uf_find<kGlobal>(p, a, n, bound);
        b = uf_find<kGlobal>(p, b, n, bound);
        if (bound || a == b) return;
        const int32_t hi = a > b ? a : b, lo = a > b ? b : a;
        if (state_cas<kGlobal>(p + hi, hi, lo)) return;
        a = hi;
        b = lo;
    }
    bound = true;
}

// The graph of one event, in either form, as calls f(target, source, position): global ids as the operand holds them
// (the target of a table row is the row), position = the index an edge mask is read at.
//   table: nbr[N, k], row i = the sources of target i; the first min(cnt[i], k) slots with cnt, all k without; a slot
//          holding -1 is empty.  `lanes` (a power of two <= 64) lanes share a row.
//   list:  tgt[e], src[e] for the positions rowptr[lo] .. rowptr[hi] - 1 of the event's rows.
struct Graph {
    const int32_t *nbr;
    const int32_t *cnt;
    int k, lanes;
    const int32_t *src, *tgt;
    int64_t e0, e1;
};

template <bool kTable, typename F>
__device__ __forceinline__ void for_each_entry(const Graph &g, int64_t lo, int64_t n, F &&f)
{
    const int tid = threadIdx.x;
    if (kTable) {
        const int sub = tid & (g.lanes - 1), stride = kCompThreads / g.lanes;
        for (int64_t r = tid / g.lanes; r < n; r += stride) {
            int c = g.k;
            if (g.cnt) {
                c = g.cnt[lo + r];
                c = c < 0 ? 0 : (c > g.k ? g.k : c);
            }
            const int64_t row = (lo + r) * g.k;
            for (int s = sub; s < c; s += g.lanes) {
                const int32_t j = g.nbr[row + s];
                if (j != -1) f(lo + r, (int64_t)j, row + s);
            }
        }
    } else {
        for (int64_t e = g.e0 + tid; e < g.e1; e += kCompThreads) f((int64_t)g.tgt[e], (int64_t)g.src[e], e);
    }
}

// 0: both ends in the event; 1: an end outside [0, N); 2: the ends in two events (1 and 2 join nothing)
__device__ __forceinline__ int entry_kind(int64_t tg, int64_t sg, int64_t lo, int64_t n, int64_t N)
{
    const int64_t t = tg - lo, s = sg - lo;
    if (t >= 0 && t < n && s >= 0 && s < n) return 0;
    return tg < 0 || tg >= N || sg < 0 || sg >= N ? 1 : 2;
}

struct Outputs {
    int64_t *labels;
    uint8_t *core;
    int64_t *nclusters;
    int32_t *flags;
};

struct DbscanArgs {
    int min_samples, count_self;
    const int32_t *rowptr;
};

template <bool kGlobal, bool kTable, bool kDbscan>
__device__ __forceinline__ void components_event(int32_t *p, int *wsum, const Graph &g, const uint8_t *edge_mask,
                                                 const uint8_t *node_mask, const DbscanArgs &da, int64_t lo, int64_t n,
                                                 int64_t N, const Outputs &out, int b)
{
    const int tid = threadIdx.x;
    int range = 0, cross = 0, full = 0;
    bool bound = false;

    // ---- phase 1: the parent words (DBSCAN: the core test from the row counts) --------------------------------------------
    if (kDbscan) {
        const bool walk = kTable && !g.cnt;         // a -1-padded table: the count of a row is found by walking it
        if (walk) {
            for (int64_t i = tid; i < n; i += kCompThreads) state_store<kGlobal>(p + i, 0);
            __syncthreads();
            for_each_entry<kTable>(g, lo, n, [&](int64_t tg, int64_t, int64_t) { state_add<kGlobal>(p + (tg - lo), 1); });
            __syncthreads();
        }
        for (int64_t i = tid; i < n; i += kCompThreads) {
            int64_t c;
            if (walk) c = state_load<kGlobal>(p + i);
            else if (kTable) {
                c = g.cnt[lo + i];
                c = c < 0 ? 0 : (c > g.k ? g.k : c);
            } else {
                c = (int64_t)da.rowptr[lo + i + 1] - (int64_t)da.rowptr[lo + i];
                c = c < 0 ? 0 : c;
            }
            if (kTable && c >= g.k) ++full;
            const bool is_core = c + (da.count_self ? 1 : 0) >= (int64_t)da.min_samples;
            state_store<kGlobal>(p + i, is_core ? (int32_t)i : kNoise);
            out.core[lo + i] = is_core ? 1 : 0;
        }
    } else {
        for (int64_t i = tid; i < n; i += kCompThreads) state_store<kGlobal>(p + i, (int32_t)i);
    }
    __syncthreads();

    // ---- phase 2: the unions.  Every entry is visited once: the counts of the entries that join nothing are exact ---------
    for_each_entry<kTable>(g, lo, n, [&](int64_t tg, int64_t sg, int64_t pos) {
        const int kind = entry_kind(tg, sg, lo, n, N);
        range += kind == 1;
        cross += kind == 2;
        if (kind || bound) return;
        const int32_t t = (int32_t)(tg - lo), s = (int32_t)(sg - lo);
        if (t == s) return;
        if (kDbscan) {
            if (state_load<kGlobal>(p + t) < 0 || state_load<kGlobal>(p + s) < 0) return;    // core-core entries only
        } else {
            if (edge_mask && !edge_mask[pos]) return;
            if (node_mask && !(node_mask[tg] && node_mask[sg])) return;
        }
        uf_union<kGlobal>(p, t, s, n, bound);
    });
    __syncthreads();

    // ---- phase 3: full compression.  No hook is left to come, so a root stays one.  A first pass halves every path once
    // more; in the second only the owner of a word writes it (a halving store of another lane could land after the
    // owner's and leave an ancestor that is no root): after the barrier every word >= 0 is the root of its node -----------
    for (int64_t i = tid; i < n; i += kCompThreads)
        if (!kDbscan || state_load<kGlobal>(p + i) >= 0) uf_find<kGlobal>(p, (int32_t)i, n, bound);
    __syncthreads();
    for (int64_t i = tid; i < n; i += kCompThreads) {
        if (kDbscan && state_load<kGlobal>(p + i) < 0) continue;
        const int32_t r = uf_find<kGlobal, false>(p, (int32_t)i, n, bound);
        if (r != (int32_t)i) state_store<kGlobal>(p + i, r);
    }
    __syncthreads();

    if (!kDbscan) {
        for (int64_t i = tid; i < n; i += kCompThreads) {
            const bool in = !node_mask || node_mask[lo + i];
            out.labels[lo + i] = in ? lo + (int64_t)state_load<kGlobal>(p + i) : -1;
        }
    } else {
        // ---- phase 4: the border pass.  A node that is not core takes, over the core nodes of its own row, the smallest
        // root: an integer max of -1 - root --------------------------------------------------------------------------------
        for_each_entry<kTable>(g, lo, n, [&](int64_t tg, int64_t sg, int64_t) {
            const int64_t t = tg - lo, s = sg - lo;
            if (t < 0 || t >= n || s < 0 || s >= n) return;
            if (state_load<kGlobal>(p + t) >= 0) return;
            const int32_t rs = state_load<kGlobal>(p + s);
            if (rs >= 0) state_max<kGlobal>(p + t, -1 - rs);
        });
        __syncthreads();

        // ---- phase 5: the roots numbered in ascending id by a workgroup scan; a root's number is parked in its own label,
        // which the other nodes of its cluster read after the barrier (both sides through L2, as the workspace words) ------
        int64_t running = 0;
        for (int64_t i0 = 0; i0 < n; i0 += kCompThreads) {          // uniform over the workgroup: wg_rank and a barrier
            const int64_t i = i0 + tid;
            const bool root = i < n && state_load<kGlobal>(p + i) == (int32_t)i;
            int before, total;
            wg_rank<kCompWaves>(root, wsum, before, total);
            if (root) __hip_atomic_store(out.labels + lo + i, running + before, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            running += total;
            __syncthreads();
        }
        if (tid == 0) out.nclusters[b] = running;
        for (int64_t i = tid; i < n; i += kCompThreads) {
            const int32_t v = state_load<kGlobal>(p + i);
            if (v == (int32_t)i) continue;                          // a root: written above
            if (v == kNoise) {
                out.labels[lo + i] = -1;
                continue;
            }
            const int64_t r = v >= 0 ? v : -1 - (int64_t)v;
            out.labels[lo + i] = __hip_atomic_load(out.labels + lo + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (range) atomicAdd(&out.flags[kFlagRange], range);
    if (cross) atomicAdd(&out.flags[kFlagCross], cross);
    if (full) atomicAdd(&out.flags[kFlagFull], full);
    if (bound) atomicOr(&out.flags[kFlagBound], 1);
}

// An event of up to lds_nodes <= DMET_COMPONENTS_LDS_NODES nodes keeps its parent words in LDS (64 KiB); a larger one
// keeps them in the caller's workspace at ws[lo ..): the events' ranges are disjoint.  Nodes no event owns are components
// of their own; DBSCAN: noise, not core.
template <bool kTable, bool kDbscan>
__global__ __launch_bounds__(kCompThreads) void components_kernel(
    const int32_t *__restrict__ nbr, int k, int lanes, const int32_t *__restrict__ cnt, const int32_t *__restrict__ rowptr,
    const int32_t *__restrict__ src, const int32_t *__restrict__ tgt, int64_t E, const uint8_t *__restrict__ edge_mask,
    const uint8_t *__restrict__ node_mask, const int64_t *__restrict__ ptr, int B, int64_t N, int min_samples,
    int count_self, int64_t *labels, uint8_t *__restrict__ core, int64_t *__restrict__ nclusters,
    int32_t *__restrict__ flags, int32_t *ws, int lds_nodes)
{
    __shared__ int32_t lds[DMET_COMPONENTS_LDS_NODES];
    __shared__ int wsum[kCompWaves];
    const int b = blockIdx.x;
    const EventRange ev = event_range(ptr, b, N);
    for_unowned<kCompThreads>(ev, b, B, N, [&](int64_t i) {
        if (kDbscan) {
            labels[i] = -1;
            core[i] = 0;
        } else {
            labels[i] = !node_mask || node_mask[i] ? i : -1;
        }
    });
    const int64_t lo = ev.lo, n = ev.n;
    if (n <= 0) {                                           // uniform over the workgroup
        if (kDbscan && threadIdx.x == 0) nclusters[b] = 0;
        return;
    }
    Graph g{nbr, cnt, k, lanes, src, tgt, 0, 0};
    if (!kTable) edge_range(rowptr, ev, E, g.e0, g.e1);
    const DbscanArgs da{min_samples, count_self, rowptr};
    const Outputs out{labels, core, nclusters, flags};
    if (n <= lds_nodes)
        components_event<false, kTable, kDbscan>(lds, wsum, g, edge_mask, node_mask, da, lo, n, N, out, b);
    else
        components_event<true, kTable, kDbscan>(ws + lo, wsum, g, edge_mask, node_mask, da, lo, n, N, out, b);
}

}  // namespace
}  // namespace dmet

using namespace dmet;

extern "C" size_t dmet_components_workspace_bytes(int64_t N)
{
    return N > 0 ? (size_t)N * sizeof(int32_t) : 0;
}

extern "C" int dmet_components_i32(const int32_t *nbr, int k, const int32_t *cnt, const int32_t *rowptr, const int32_t *src,
                                   const int32_t *tgt, int64_t E, const uint8_t *edge_mask, const uint8_t *node_mask,
                                   const int64_t *ptr, int B, int64_t N, int mode, int min_samples, int count_self,
                                   int64_t *labels, uint8_t *core, int64_t *nclusters, int32_t *flags, int lds_nodes,
                                   void *ws, size_t ws_bytes, dmet_stream_t stream)
{
    DMET_REQUIRE(N >= 0 && N <= INT32_MAX, "dmet_components_i32: N=%lld outside 0..2^31-1", (long long)N);
    DMET_REQUIRE(B >= 0, "dmet_components_i32: B=%d < 0", B);
    DMET_REQUIRE(mode == DMET_COMPONENTS_CC || mode == DMET_COMPONENTS_DBSCAN, "dmet_components_i32: mode=%d is not 0 or 1",
                 mode);
    DMET_REQUIRE(lds_nodes >= 0, "dmet_components_i32: lds_nodes=%d < 0", lds_nodes);
    DMET_REQUIRE(flags, "dmet_components_i32: flags is NULL");
    const bool table = nbr != nullptr || rowptr == nullptr, dbscan = mode == DMET_COMPONENTS_DBSCAN;
    if (table) {
        DMET_REQUIRE(k >= 0, "dmet_components_i32: k=%d < 0", k);
        DMET_REQUIRE(nbr || k == 0 || N == 0, "dmet_components_i32: nbr and rowptr are both NULL");
    } else {
        DMET_REQUIRE(E >= 0 && E <= INT32_MAX, "dmet_components_i32: E=%lld outside 0..2^31-1", (long long)E);
        DMET_REQUIRE((src && tgt) || E == 0, "dmet_components_i32: src or tgt is NULL");
    }
    if (dbscan) {
        DMET_REQUIRE(!edge_mask && !node_mask, "dmet_components_i32: DBSCAN mode takes no edge_mask / node_mask");
        DMET_REQUIRE(min_samples >= 1, "dmet_components_i32: min_samples=%d < 1", min_samples);
    }
    const hipError_t me = hipMemsetAsync(flags, 0, kNumFlags * sizeof(int32_t), as_stream(stream));
    if (me != hipSuccess) return hip_fail(me, "hipMemsetAsync(flags)");
    if (B == 0 && N == 0) return 0;
    DMET_REQUIRE(B > 0, "dmet_components_i32: B=0 events for N=%lld nodes", (long long)N);
    DMET_REQUIRE(ptr, "dmet_components_i32: ptr is NULL");
    DMET_REQUIRE(labels || N == 0, "dmet_components_i32: labels is NULL");
    DMET_REQUIRE(!dbscan || ((core || N == 0) && nclusters), "dmet_components_i32: core or nclusters is NULL");
    DMET_REQUIRE(ws_bytes >= dmet_components_workspace_bytes(N),
                 "dmet_components_i32: ws_bytes=%zu, dmet_components_workspace_bytes asks for %zu", ws_bytes,
                 dmet_components_workspace_bytes(N));
    DMET_REQUIRE(ws || N == 0, "dmet_components_i32: ws is NULL");
    const int limit = lds_limit(lds_nodes, DMET_COMPONENTS_LDS_NODES);
    // lanes of a table row: the next power of two from the width, 64 at the most; a counted table's rows are taken as
    // shallow (a radius table is mostly padding) and get 16
    int lanes = 1;
    while (lanes < k && lanes < (cnt ? 16 : kWave)) lanes *= 2;
    with_flags(
        [&](auto t, auto d) {
            hipLaunchKernelGGL((components_kernel<decltype(t)::value, decltype(d)::value>), dim3((unsigned)B),
                               dim3(kCompThreads), 0, as_stream(stream), nbr, k, lanes, cnt, rowptr, src, tgt, E, edge_mask,
                               node_mask, ptr, B, N, min_samples, count_self, labels, core, nclusters, flags, (int32_t *)ws,
                               limit);
        },
        table, dbscan);
    DMET_LAUNCH_CHECK("components_kernel");
    return 0;
}

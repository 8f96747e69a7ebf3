// condense.hip -- object-condensation inference of every event of a batch as one windowed walk per workgroup.
// Semantics: include/dmet.h, section "Condensation clustering".
#include "event_wg.h"

namespace dmet {
namespace {

constexpr int kCondThreads = DMET_CONDENSE_THREADS;
constexpr int kWin = DMET_CONDENSE_WINDOW;
constexpr int kScan = 4;                    // chunks of 64 ranking entries wavefront 0 has in flight while it collects
static_assert(kWin == kWave, "a window is resolved by the lanes of one wavefront");

constexpr int32_t kFree = -1;               // a state word: the node's event-local number, or kFree

enum { kFlagRange = 0, kFlagBound = 1, kNumFlags = 2 };

// The state words (event_wg.h): a word written by wavefront 0 is read by the thread that owns the node.

// The window of one event: what wavefront 0 leaves for the workgroup.
struct Window {
    float px[DMET_CONDENSE_MAX_DIM * kWin];     // coordinate c of the window's point q at px[c * kWin + q], rank order
    int32_t pid[kWin];                          // its event-local id
    int32_t wid[kWin];                          // the collected candidates, before they are resolved
    int32_t npts, ncand;                        // points of this window; candidates collected (0: the walk is over)
};

struct Outputs {
    int64_t *local, *assoc, *nclusters;
    int32_t *flags;
};

// What wavefront 0 carries from window to window (uniform over its lanes).
struct Walk {
    int64_t cur;        // the next slot of the event's ranking
    bool over;          // an entry failed beta > t_beta, or the ranking is used up
    int range;          // entries outside the event met so far
};

// Wavefront 0: the next kWin still-unassigned candidates from the cursor, in rank order, into w.wid; returns their
// count.  An entry is compared against [lo, hi) before beta or the state word is read through it.
template <bool kGlobal>
__device__ __forceinline__ int collect(const int32_t *st, Window &w, Walk &wk, const float *__restrict__ beta,
                                       const int64_t *__restrict__ order, float t_beta, int64_t lo, int64_t n, int lane)
{
    int cnt = 0;
    while (cnt < kWin && !wk.over) {
        if (wk.cur >= n) {
            wk.over = true;
            break;
        }
        int64_t id[kScan];
        float bt[kScan];
#pragma unroll
        for (int u = 0; u < kScan; ++u) {
            const int64_t pos = wk.cur + u * kWave + lane;
            id[u] = pos < n ? order[lo + pos] - lo : -1;
        }
#pragma unroll
        for (int u = 0; u < kScan; ++u) bt[u] = id[u] >= 0 && id[u] < n ? beta[lo + id[u]] : 0.0f;
        const int64_t base0 = wk.cur;
#pragma unroll
        for (int u = 0; u < kScan; ++u) {
            const int64_t base = base0 + u * kWave;
            if (base >= n) {
                wk.over = true;
                break;
            }
            const int have = n - base < kWave ? (int)(n - base) : kWave;    // slots of this chunk inside the ranking
            const bool in = id[u] >= 0 && id[u] < n;
            const uint64_t failed = __ballot(lane < have && in && !(bt[u] > t_beta));
            const int stop = failed ? __builtin_ctzll(failed) : have;       // entries before `stop` are candidates
            const bool live = lane < stop;
            const bool take = live && in && state_load<kGlobal>(st + id[u]) == kFree;
            const uint64_t tm = __ballot(take);
            const int slot = cnt + __popcll(tm & lanes_below(lane));
            const bool put = take && slot < kWin;
            const uint64_t pm = __ballot(put);
            if (put) w.wid[slot] = (int32_t)id[u];
            const bool filled = pm != tm;                                   // the window took only a part of this chunk
            const int used = filled ? 64 - __builtin_clzll(pm) : stop;      // entries of the chunk the walk has passed
            wk.range += __popcll(__ballot(live && !in) & (used < kWave ? lanes_below(used) : ~0ull));
            cnt += __popcll(pm);
            wk.cur = base + used;
            if (!filled && stop < kWave) wk.over = true;                    // a failed entry, or the end of the ranking
            if (filled || wk.over || cnt == kWin) break;
        }
    }
    return cnt;
}

template <int D, bool kGlobal>
__device__ __forceinline__ void condense_event(int32_t *st, Window &w, const float *__restrict__ beta,
                                               const float *__restrict__ x, const int64_t *__restrict__ order,
                                               float t_beta, float td2, int64_t lo, int64_t n, const Outputs &out, int b)
{
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    for (int64_t i = tid; i < n; i += kCondThreads) state_store<kGlobal>(st + i, kFree);
    __syncthreads();

    Walk wk{0, false, 0};
    int64_t nfound = 0;         // condensation points of the earlier windows (uniform over the workgroup)
    bool bound = false;
    for (int64_t it = 0;; ++it) {
        if (it > n) {           // every window holds a point: there are at most n of them
            bound = true;
            break;
        }
        if (wave == 0) {
            const int cnt = collect<kGlobal>(st, w, wk, beta, order, t_beta, lo, n, lane);
            wave_sync();
            // ---- resolve the window among itself: lane t holds entry t ---------------------------------------------------
            const bool have = lane < cnt;
            const int32_t me = have ? w.wid[lane] : 0;
            float xs[D];
#pragma unroll
            for (int c = 0; c < D; ++c) xs[c] = have ? x[(lo + me) * D + c] : 0.0f;
            bool alive = have;
            int32_t mynum = 0, mypt = me;
            int np = 0;
            uint64_t rest = __ballot(alive);
            while (rest) {
                const int s = __builtin_ctzll(rest);                        // alive, and all before it settled: a point
                const int32_t sid = __builtin_amdgcn_readlane(me, s);
                float acc = 0.0f;
#pragma unroll
                for (int c = 0; c < D; ++c) {
                    const float a = xs[c] - __int_as_float(__builtin_amdgcn_readlane(__float_as_int(xs[c]), s));
                    acc = fmaf(a, a, acc);
                }
                const bool hit = alive && lane > s && acc < td2;
                if (hit || lane == s) {
                    mynum = (int32_t)nfound + np;
                    mypt = sid;
                }
                if (hit) alive = false;
                ++np;
                rest = __ballot(alive) & (s < kWave - 1 ? ~lanes_below(s + 1) : 0ull);
            }
            const uint64_t pts = __ballot(alive);
            if (alive) {
                const int q = __popcll(pts & lanes_below(lane));
                w.pid[q] = me;
#pragma unroll
                for (int c = 0; c < D; ++c) w.px[c * kWin + q] = xs[c];
            }
            if (have) {
                state_store<kGlobal>(st + me, mynum);
                out.local[lo + me] = mynum;
                out.assoc[lo + me] = lo + mypt;
            }
            if (lane == 0) {
                w.npts = np;
                w.ncand = cnt;
            }
        }
        __syncthreads();
        const int np = w.npts;
        if (w.ncand == 0) break;            // uniform: no candidate is left
        // ---- every thread: its own unassigned nodes against the window's points, in rank order ----------------------------
        for (int64_t j = tid; j < n; j += kCondThreads) {
            if (state_load<kGlobal>(st + j) != kFree) continue;
            float xj[D];
#pragma unroll
            for (int c = 0; c < D; ++c) xj[c] = x[(lo + j) * D + c];
            for (int q = 0; q < np; ++q) {
                float acc = 0.0f;
#pragma unroll
                for (int c = 0; c < D; ++c) {
                    const float a = xj[c] - w.px[c * kWin + q];
                    acc = fmaf(a, a, acc);
                }
                if (acc < td2) {
                    const int32_t num = (int32_t)nfound + q;
                    state_store<kGlobal>(st + j, num);
                    out.local[lo + j] = num;
                    out.assoc[lo + j] = lo + w.pid[q];
                    break;
                }
            }
        }
        nfound += np;
        __syncthreads();                    // the state words, before wavefront 0 collects over them and refills the window
    }

    for (int64_t j = tid; j < n; j += kCondThreads) {
        if (state_load<kGlobal>(st + j) != kFree) continue;
        out.local[lo + j] = -1;
        out.assoc[lo + j] = -1;
    }
    if (tid == 0) {
        out.nclusters[b] = nfound;
        if (wk.range) atomicAdd(&out.flags[kFlagRange], wk.range);
        if (bound) atomicOr(&out.flags[kFlagBound], 1);
    }
}

// An event of up to lds_nodes <= DMET_CONDENSE_LDS_NODES nodes keeps its state words in LDS (64 KiB); a larger one keeps
// them in the caller's workspace at ws[lo ..): the events' ranges are disjoint.  Nodes no event owns are noise.
template <int D>
__global__ __launch_bounds__(kCondThreads) void condense_kernel(
    const float *__restrict__ beta, const float *__restrict__ x, const int64_t *__restrict__ order,
    const int64_t *__restrict__ ptr, int B, int64_t N, float t_beta, float td2, int64_t *__restrict__ local,
    int64_t *__restrict__ assoc, int64_t *__restrict__ nclusters, int32_t *__restrict__ flags, int32_t *ws, int lds_nodes)
{
    __shared__ int32_t lds[DMET_CONDENSE_LDS_NODES];
    __shared__ Window w;
    const int b = blockIdx.x;
    const EventRange ev = event_range(ptr, b, N);
    for_unowned<kCondThreads>(ev, b, B, N, [&](int64_t i) {
        local[i] = -1;
        assoc[i] = -1;
    });
    const int64_t lo = ev.lo, n = ev.n;
    if (n <= 0) {                                           // uniform over the workgroup
        if (threadIdx.x == 0) nclusters[b] = 0;
        return;
    }
    const Outputs out{local, assoc, nclusters, flags};
    if (n <= lds_nodes) condense_event<D, false>(lds, w, beta, x, order, t_beta, td2, lo, n, out, b);
    else condense_event<D, true>(ws + lo, w, beta, x, order, t_beta, td2, lo, n, out, b);
}

}  // namespace
}  // namespace dmet

using namespace dmet;

extern "C" size_t dmet_condense_workspace_bytes(int64_t N)
{
    return N > 0 ? (size_t)N * sizeof(int32_t) : 0;
}

extern "C" int dmet_condense_f32(const float *beta, const float *x, const int64_t *order, const int64_t *ptr, int B,
                                 int64_t N, int D, float t_beta, float t_d, int64_t *local, int64_t *assoc,
                                 int64_t *nclusters, int32_t *flags, int lds_nodes, void *ws, size_t ws_bytes,
                                 dmet_stream_t stream)
{
    DMET_REQUIRE(N >= 0 && N <= INT32_MAX, "dmet_condense_f32: N=%lld outside 0..2^31-1", (long long)N);
    DMET_REQUIRE(B >= 0, "dmet_condense_f32: B=%d < 0", B);
    DMET_REQUIRE(D >= 1 && D <= DMET_CONDENSE_MAX_DIM, "dmet_condense_f32: D=%d outside 1..%d", D, DMET_CONDENSE_MAX_DIM);
    DMET_REQUIRE(__builtin_isfinite(t_beta), "dmet_condense_f32: t_beta=%g is not finite", (double)t_beta);
    DMET_REQUIRE(__builtin_isfinite(t_d) && t_d > 0.0f, "dmet_condense_f32: t_d=%g is not finite and > 0", (double)t_d);
    DMET_REQUIRE(lds_nodes >= 0, "dmet_condense_f32: lds_nodes=%d < 0", lds_nodes);
    DMET_REQUIRE(flags, "dmet_condense_f32: flags is NULL");
    const hipError_t me = hipMemsetAsync(flags, 0, kNumFlags * sizeof(int32_t), as_stream(stream));
    if (me != hipSuccess) return hip_fail(me, "hipMemsetAsync(flags)");
    if (B == 0 && N == 0) return 0;
    DMET_REQUIRE(B > 0, "dmet_condense_f32: B=0 events for N=%lld nodes", (long long)N);
    DMET_REQUIRE(ptr, "dmet_condense_f32: ptr is NULL");
    DMET_REQUIRE(nclusters, "dmet_condense_f32: nclusters is NULL");
    DMET_REQUIRE((beta && x && order) || N == 0, "dmet_condense_f32: beta, x or order is NULL");
    DMET_REQUIRE((local && assoc) || N == 0, "dmet_condense_f32: local or assoc is NULL");
    DMET_REQUIRE(ws_bytes >= dmet_condense_workspace_bytes(N),
                 "dmet_condense_f32: ws_bytes=%zu, dmet_condense_workspace_bytes asks for %zu", ws_bytes,
                 dmet_condense_workspace_bytes(N));
    DMET_REQUIRE(ws || N == 0, "dmet_condense_f32: ws is NULL");
    const int limit = lds_limit(lds_nodes, DMET_CONDENSE_LDS_NODES);
    const float td2 = t_d * t_d;
    with_int<1, 2, 3, 4, 5, 6, 7, 8>(D, [&](auto d) {
        hipLaunchKernelGGL(condense_kernel<decltype(d)::value>, dim3((unsigned)B), dim3(kCondThreads), 0, as_stream(stream),
                           beta, x, order, ptr, B, N, t_beta, td2, local, assoc, nclusters, flags, (int32_t *)ws, limit);
    });
    DMET_LAUNCH_CHECK("condense_kernel");
    return 0;
}

// radius.hip -- N1: the radius graph over ragged events (gfx950): radius_kernel, and the kernels windowed by the first
// coordinate (radius_order_kernel, radius_window_kernel).  Periods and a second point set ride as the optional trailing
// argument pack of knn_common.h, shared with the kNN build (knn.hip).
#include "common.h"
#include "knn_common.h"

namespace dmet {
namespace {

// ---- radius graph (N1): first max_nbr candidates in ascending index with d < r^2 ------------------------
// One lane per query, four independent wavefronts per workgroup (no workgroup barrier).  Candidates are staged per
// wavefront in LDS as [pair][feature][2] so that one broadcast read yields a feature of two candidates in adjacent
// registers: the R1 chain then runs on v_pk_add_f32 / v_pk_fma_f32 (each half an exact IEEE op in feature order, same
// bits as the scalar oracle).  The kernel only writes the hits; unused slots are -1 from a memset (dmet_radius_f32) or left unwritten (counted forms).
// `skip_self` reproduces upstream's loop=False: the search limit counts the node itself, the node is not stored.
constexpr int kRadTile = 64;   // candidates per LDS tile and wavefront

template <bool PER>
__device__ __forceinline__ f2 rad_wrap(f2 df, float L)
{
    if (!PER) return df;
    const float ax = fabsf(df.x), ay = fabsf(df.y);
    return f2{fminf(ax, L - ax), fminf(ay, L - ay)};
}

// With a KnnQuerySet after the periods (dmet_radius_xy_f32) the 64 queries of a wavefront are rows of qx (events qptr, N rows
// in all) and x / ptr hold the candidates of the same events; skip_self is then 0.
template <int DP, typename... Per>
__global__ __launch_bounds__(kWave * 4) void radius_kernel(const float *__restrict__ x,
                                                            const int64_t *__restrict__ ptr, int B, int64_t N, int D,
                                                            float r2, int max_nbr, int skip_self,
                                                            int32_t *__restrict__ nbr, int32_t *__restrict__ cntout,
                                                            Per... per_arg)
{
    constexpr bool PER = pack_has<RadPeriod, Per...>;
    const RadPeriod per = rad_periods(per_arg...);
    const KnnQuerySet qs = query_set(x, ptr, per_arg...);
    const float *__restrict__ qx = qs.qx;
    const int64_t *__restrict__ qptr = qs.qptr;
    __shared__ f2 tile_all[4][(kRadTile / 2) * DP];
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    f2 *tile = tile_all[wv];
    const int64_t q_first = ((int64_t)blockIdx.x * 4 + wv) * kWave;
    if (q_first >= N) return;
    const int64_t q_last = min(N, q_first + kWave) - 1;
    const int b_first = find_event(qptr, B, q_first);
    const int b_last = find_event(qptr, B, q_last);
    const int clo = (int)ptr[b_first];
    const int chi = (int)ptr[b_last + 1];
    const bool one_event = b_first == b_last;          // wave-uniform: no per-lane event window needed
    const int64_t qi = q_first + lane;
    const bool valid = qi < N;
    const int64_t qq = valid ? qi : q_last;
    int lo = clo, hi = chi;
    if (!one_event) { const int b = find_event(qptr, B, qq); lo = (int)ptr[b]; hi = (int)ptr[b + 1]; }
    f2 q[DP];
#pragma unroll
    for (int c = 0; c < DP; ++c) { const float v = (c < D) ? qx[qq * D + c] : 0.0f; q[c].x = v; q[c].y = v; }
    int stored = 0, seen = valid ? 0 : max_nbr;        // idle lanes are "full" from the start
    int32_t *row = nbr + qq * max_nbr;
    // hits are rare per lane (a few per thousand pairs): the sweep of a 64-candidate tile only records them as bits
    // of a lane-private 64-bit mask (compare + select + or per candidate, no branch, no memory traffic); the set
    // bits are turned into row entries after the tile, in ascending candidate order
    for (int c0 = clo; c0 < chi; c0 += kRadTile) {
        const int cntc = min(kRadTile, chi - c0);
        wave_sync();
        for (int e = lane; e < kRadTile * DP; e += kWave) {
            const int c = e / DP, dd = e - c * DP;
            // rows past the range get a coordinate that is farther than any radius from everything
            const float v = (c < cntc) ? ((dd < D) ? x[(int64_t)(c0 + c) * D + dd] : 0.0f) : 3.0e18f;
            reinterpret_cast<float *>(tile)[((c >> 1) * DP + dd) * 2 + (c & 1)] = v;
        }
        wave_sync();
        if (!__any(seen < max_nbr)) break;             // every query of the wavefront is full
        unsigned m0 = 0u, m1 = 0u;
#pragma unroll
        for (int cc = 0; cc < kRadTile; cc += 2) {
            f2 acc = {0.0f, 0.0f};
#pragma unroll
            for (int c = 0; c < DP; ++c) {
                const f2 df = rad_wrap<PER>(tile[(cc >> 1) * DP + c] - q[c], per.L[c]);
                acc = __builtin_elementwise_fma(df, df, acc);
            }
            if (cc < 32) {
                m0 |= (acc.x < r2) ? (1u << cc) : 0u;
                m0 |= (acc.y < r2) ? (1u << (cc + 1)) : 0u;
            } else {
                m1 |= (acc.x < r2) ? (1u << (cc - 32)) : 0u;
                m1 |= (acc.y < r2) ? (1u << (cc - 31)) : 0u;
            }
        }
        unsigned long long mask = ((unsigned long long)m1 << 32) | m0;
        if (!one_event) {                               // keep the candidates of the lane's own event only
            const int a0 = max(lo - c0, 0), a1 = min(hi - c0, 64);
            const unsigned long long keep = (a1 <= a0) ? 0ull
                : ((a1 >= 64 ? ~0ull : ((1ull << a1) - 1ull)) & ~((1ull << a0) - 1ull));
            mask &= keep;
        }
        while (__any(mask != 0ull)) {
            if (mask != 0ull) {
                const int bit = __ffsll((long long)mask) - 1;
                mask &= mask - 1ull;
                const int j = c0 + bit;
                if (seen < max_nbr) {
                    if (!(skip_self && j == (int)qq)) { row[stored] = j; ++stored; }
                    ++seen;
                }
            }
        }
    }
    if (valid) cntout[qi] = stored;
}

// ---- radius graph, windowed by the first coordinate --------------------------------------------------------------
// d(i,j) < r^2 needs |x0_i - x0_j| < r.  Queries are therefore PROCESSED in the order of their first coordinate (a
// wavefront = 64 neighbours in x0), and each wavefront walks its event's nodes in index order but only keeps those
// whose x0 lies in [min x0 - r, max x0 + r] of its queries (stream compaction: ballot + prefix count into a small
// index queue).  The kept candidates go through the same tile sweep as radius_kernel, still in ascending index
// order, so "the first max_nbr hits in index order" and the bits of every distance are unchanged -- only the
// candidates that cannot be hits are never multiplied out.  In (eta, phi) with r = 0.4 that is ~85 % of them.
constexpr int kRadBins = 1024;

// order[ptr[b] .. ptr[b+1]) = the node ids of event b grouped into kRadBins bins of x0 (ascending bins; the order
// inside a bin is arbitrary and does not influence any result, only which queries share a wavefront).
__global__ __launch_bounds__(kRadBins) void radius_order_kernel(const float *__restrict__ x,
                                                                const int64_t *__restrict__ ptr, int B, int D,
                                                                int32_t *__restrict__ order)
{
    constexpr int NT = kRadBins, NW = kRadBins / 64;
    __shared__ int hist[kRadBins];
    __shared__ float red_lo[NW], red_hi[NW];
    __shared__ int wave_tot[NW];
    const int b = blockIdx.x;
    if (b >= B) return;
    const int64_t lo = ptr[b], hi = ptr[b + 1];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    float mn = __builtin_inff(), mx = -__builtin_inff();
    for (int64_t i = lo + tid; i < hi; i += NT) {
        const float v = x[i * D];
        if (v == v && fabsf(v) < 3.0e38f) { mn = fminf(mn, v); mx = fmaxf(mx, v); }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { mn = fminf(mn, __shfl_xor(mn, off, 64)); mx = fmaxf(mx, __shfl_xor(mx, off, 64)); }
    if (lane == 0) { red_lo[wv] = mn; red_hi[wv] = mx; }
    hist[tid] = 0;
    __syncthreads();
    mn = red_lo[0]; mx = red_hi[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) { mn = fminf(mn, red_lo[w]); mx = fmaxf(mx, red_hi[w]); }
    const float scale = (mx > mn) ? (float)(kRadBins - 1) / (mx - mn) : 0.0f;
    auto bin_of = [&](float v) -> int {
        if (!(v == v)) return 0;
        const float t = (v - mn) * scale;
        if (!(t == t)) return 0;
        return t <= 0.0f ? 0 : (t >= (float)(kRadBins - 1) ? kRadBins - 1 : (int)t);
    };
    for (int64_t i = lo + tid; i < hi; i += NT) atomicAdd(&hist[bin_of(x[i * D])], 1);
    __syncthreads();
    // exclusive scan of the counters: one per thread, wavefront scan, then the wavefront totals
    const int mine = hist[tid];
    int incl = mine;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const int o = __shfl_up(incl, off, 64); if (lane >= off) incl += o; }
    if (lane == 63) wave_tot[wv] = incl;
    __syncthreads();
    int base = incl - mine;
    for (int w = 0; w < wv; ++w) base += wave_tot[w];
    hist[tid] = base;
    __syncthreads();
    for (int64_t i = lo + tid; i < hi; i += NT) {
        const int pos = atomicAdd(&hist[bin_of(x[i * D])], 1);
        order[lo + pos] = (int32_t)i;
    }
}

constexpr int kRadQueue = 128;   // pending candidate ids per wavefront (a compaction step adds at most 64)

// Per = RadPeriod wraps coordinates 1 .. DP-1 with L[c]; coordinate 0 must be plain (the window is not wrap-aware).
// The window stays exact: the coordinate-0 term is the first of the chain and the later terms are >= 0 or NaN.
template <int DP, typename... Per>
__global__ __launch_bounds__(kWave * 4) void radius_window_kernel(const float *__restrict__ x,
                                                                   const int64_t *__restrict__ ptr, int B, int64_t N,
                                                                   int D, float r2, int max_nbr, int skip_self,
                                                                   const int32_t *__restrict__ order,
                                                                   int32_t *__restrict__ nbr,
                                                                   int32_t *__restrict__ cntout,
                                                                   uint16_t *__restrict__ nbr16, int stride16,
                                                                   Per... per_arg)
{
    constexpr bool PER = sizeof...(Per) > 0;
    const RadPeriod per = rad_periods(per_arg...);
    __shared__ f2 tile_all[4][(kRadTile / 2) * DP];
    __shared__ int queue_all[4][kRadQueue];
    // hits leave the lane through 16-byte staging slots (4 int32 ids / 8 uint16 ids) and reach memory as one 16-byte
    // store per full slot: a wavefront's 64 scattered 2- or 4-byte stores per hit cost more than the distances
    __shared__ __attribute__((aligned(16))) int32_t stage32_all[4][kWave][4];
    __shared__ __attribute__((aligned(16))) uint16_t stage16_all[4][kWave][8];
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    f2 *tile = tile_all[wv];
    int *queue = queue_all[wv];
    int32_t *stage32 = stage32_all[wv][lane];
    uint16_t *stage16 = stage16_all[wv][lane];
    // wavefronts are aligned to events: event b owns the wavefront ids from (ptr[b] >> 6) + b on (strictly increasing
    // in b and at least ceil(n_b / 64) apart, so no prefix sum over the events is needed); surplus ids idle
    const int64_t w = (int64_t)blockIdx.x * 4 + wv;
    int b = 0;
    {
        int l = 0, h = B;                               // largest b with (ptr[b] >> 6) + b <= w
        while (h - l > 1) {
            const int mid = (l + h) >> 1;
            if ((ptr[mid] >> 6) + mid <= w) l = mid; else h = mid;
        }
        b = l;
    }
    const int clo = (int)ptr[b], chi = (int)ptr[b + 1];
    const int64_t p_first = clo + (w - ((int64_t)(clo >> 6) + b)) * kWave;   // positions in `order`
    if (p_first >= chi) return;
    const int64_t p_last = min((int64_t)chi, p_first + kWave) - 1;
    constexpr bool one_event = true;
    const int64_t pi = p_first + lane;
    const bool valid = pi < chi;
    const int64_t qq = order[valid ? pi : p_last];     // this lane's query (a node of event b)
    const int lo = clo, hi = chi;
    (void)N;
    f2 q[DP];
#pragma unroll
    for (int c = 0; c < DP; ++c) { const float v = (c < D) ? x[qq * D + c] : 0.0f; q[c].x = v; q[c].y = v; }
    // window of the first coordinate: a little wider than [min - r, max + r] so that rounding can only ADD candidates
    float wlo = -__builtin_inff(), whi = __builtin_inff();
    if (one_event) {
        float mn = q[0].x, mx = q[0].x;
        if (!(mn == mn)) { mn = __builtin_inff(); mx = -__builtin_inff(); }   // a NaN query has no hits anyway
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { mn = fminf(mn, __shfl_xor(mn, off, 64)); mx = fmaxf(mx, __shfl_xor(mx, off, 64)); }
        const float rr = __builtin_sqrtf(r2) * 1.00001f + 1e-30f;
        wlo = mn - rr - 1e-6f * fabsf(mn);
        whi = mx + rr + 1e-6f * fabsf(mx);
    }
    int stored = 0, seen = valid ? 0 : max_nbr;        // idle lanes are "full" from the start
    int32_t *row = nbr + qq * max_nbr;
    // optional second copy of the row as event-local uint16 ids (rows of stride16 ids, 16-byte aligned)
    uint16_t *row16 = nbr16 ? nbr16 + qq * stride16 : nullptr;
    int pending = 0;                                    // wave-uniform: ids waiting in the queue

    // sweep of one tile: the first `cntc` queue entries (ascending node ids)
    auto sweep = [&](const int cntc) {
        wave_sync();
        for (int e = lane; e < kRadTile * DP; e += kWave) {
            const int c = e / DP, dd = e - c * DP;
            // rows past the range get a coordinate that is farther than any radius from everything
            const float v = (c < cntc) ? ((dd < D) ? x[(int64_t)queue[c] * D + dd] : 0.0f) : 3.0e18f;
            reinterpret_cast<float *>(tile)[((c >> 1) * DP + dd) * 2 + (c & 1)] = v;
        }
        wave_sync();
        unsigned m0 = 0u, m1 = 0u;
#pragma unroll
        for (int cc = 0; cc < kRadTile; cc += 2) {
            f2 acc = {0.0f, 0.0f};
#pragma unroll
            for (int c = 0; c < DP; ++c) {
                // coordinate 0 is never periodic here (it is the window's coordinate)
                const f2 d = tile[(cc >> 1) * DP + c] - q[c];
                const f2 df = (c > 0) ? rad_wrap<PER>(d, per.L[c]) : d;
                acc = __builtin_elementwise_fma(df, df, acc);
            }
            if (cc < 32) {
                m0 |= (acc.x < r2) ? (1u << cc) : 0u;
                m0 |= (acc.y < r2) ? (1u << (cc + 1)) : 0u;
            } else {
                m1 |= (acc.x < r2) ? (1u << (cc - 32)) : 0u;
                m1 |= (acc.y < r2) ? (1u << (cc - 31)) : 0u;
            }
        }
        unsigned long long mask = ((unsigned long long)m1 << 32) | m0;
        while (__any(mask != 0ull)) {
            if (mask != 0ull) {
                const int bit = __ffsll((long long)mask) - 1;
                mask &= mask - 1ull;
                const int j = queue[bit];
                if (seen < max_nbr && j >= lo && j < hi) {   // own event only (wavefronts that straddle two events)
                    if (!(skip_self && j == (int)qq)) {
                        stage32[stored & 3] = j;
                        if (row16) stage16[stored & 7] = (uint16_t)(j - lo);
                        ++stored;
                        if ((stored & 3) == 0 && nbr) {   // rows are only 4-byte aligned (255-wide tables)
                            struct __attribute__((packed, aligned(4))) I4 { int32_t a, b, c, d; };
                            const int4 v = *reinterpret_cast<const int4 *>(stage32);
                            *reinterpret_cast<I4 *>(row + stored - 4) = I4{v.x, v.y, v.z, v.w};
                        }
                        if (row16 && (stored & 7) == 0)
                            *reinterpret_cast<uint4 *>(row16 + stored - 8) = *reinterpret_cast<const uint4 *>(stage16);
                    }
                    ++seen;
                }
            }
        }
    };

    // the walk over the event's nodes is a chain of dependent steps (load a first coordinate, ballot, append, maybe
    // sweep): with every wavefront of the grid resident at once the kernel lasts as long as ONE wavefront's chain, so
    // the first coordinates of kRadAhead groups of 64 nodes are fetched together (151 -> 128 us for the whole table at
    // 64 x 4500 nodes).  Carrying both coordinates with the queued ids (D = 2), so that a sweep needs no gather from
    // memory at all, was measured too: no further gain -- the kernel is then half vector-ALU time (7 000 instructions
    // per wavefront: the hit loop, the pair distances, the compaction), half latency.
    constexpr int kRadAhead = 4;
    bool full = false;
    for (int c0 = clo; c0 < chi && !full; c0 += kWave * kRadAhead) {
        float v4[kRadAhead];
#pragma unroll
        for (int u = 0; u < kRadAhead; ++u) {
            const int c = c0 + u * kWave + lane;
            v4[u] = (c < chi) ? x[(int64_t)c * D] : __builtin_nanf("");   // a NaN is outside every window
        }
#pragma unroll
        for (int u = 0; u < kRadAhead; ++u) {
            if (c0 + u * kWave >= chi) break;
            if (!__any(seen < max_nbr)) { pending = 0; full = true; break; }   // every query of the wavefront is full
            const int c = c0 + u * kWave + lane;
            const bool keep = c < chi && v4[u] >= wlo && v4[u] <= whi;
            const unsigned long long km = __ballot(keep);
            if (keep) queue[pending + __builtin_amdgcn_mbcnt_hi((unsigned)(km >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)km, 0u))] = c;
            pending += __popcll(km);
            if (pending >= kRadTile) {
                sweep(kRadTile);
                wave_sync();
                const int rest = pending - kRadTile;       // < 64: move it to the front
                int moved = 0;
                if (lane < rest) moved = queue[kRadTile + lane];
                wave_sync();
                if (lane < rest) queue[lane] = moved;
                pending = rest;
            }
        }
    }
    if (pending > 0 && __any(seen < max_nbr)) sweep(pending);
    if (valid) {
        cntout[qq] = stored;
        if (nbr)
            for (int s = stored & ~3; s < stored; ++s) row[s] = stage32[s & 3];     // the unfinished slots
        if (row16 && (stored & 7) != 0) {   // the last started chunk of 8 reads as "no neighbour" beyond the row's end
            for (int s = stored & 7; s < 8; ++s) stage16[s] = 0xFFFFu;
            *reinterpret_cast<uint4 *>(row16 + (stored & ~7)) = *reinterpret_cast<const uint4 *>(stage16);
        }
    }
}

}  // namespace
}  // namespace dmet

using namespace dmet;

enum class RadiusForm { AllPairs, Windowed };

// One radius build, as its entry asks for it.  radius_build works from this request alone.
struct RadiusBuild {
    const char *who;            // the entry that was called, for messages
    const float *x;             // candidate rows, cut into B events by ptr; the queries too unless qs is set
    const int64_t *ptr;
    int B;
    int64_t N;                  // number of QUERY rows: the rows of x, or of qs->qx when that is set
    int D;
    float r;
    int max_nbr, skip_self;
    bool fill;                  // slots from cnt on are -1 (one memset); false: left unwritten, consumers go by cnt
    int32_t *nbr, *cnt;
    hipStream_t st;
    RadiusForm form = RadiusForm::AllPairs;   // Windowed: candidates windowed by coordinate 0 (one point set, needs ws)
    void *ws = nullptr;
    size_t ws_bytes = 0;
    uint16_t *nbr16 = nullptr;                // Windowed: optional event-local copy of the rows, stride16 ids apart
    int stride16 = 0;
    const float *period = nullptr;            // D circumferences, 0 = a plain coordinate
    bool need_period = false;                 // a null period is an error
    const KnnQuerySet *qs = nullptr;          // non-null: two point sets (its entry has checked x; skip_self is 0)
};

extern "C" size_t dmet_radius_workspace_bytes(int64_t N)
{
    return N > 0 ? sizeof(int32_t) * (size_t)N + 512 : 0;
}

static int radius_build(const RadiusBuild &b)
{
    const bool windowed = b.form == RadiusForm::Windowed;
    RadPeriod per;
    bool any = false;
    if (b.period || b.need_period) {
        const int rc = radius_periods(b.who, b.D, b.period, &per, &any);
        if (rc) return rc;
        DMET_REQUIRE(!windowed || b.period[0] == 0.0f, "%s: coordinate 0 is periodic (period[0]=%g): the window runs on "
                     "coordinate 0; use dmet_radius_periodic_f32", b.who, (double)b.period[0]);
    }
    // all periods 0: the plain kernel (bit-identical to the entries without periods by construction)
    const RadPeriod *pp = any ? &per : nullptr;
    DMET_REQUIRE(!b.nbr16 || (b.stride16 >= b.max_nbr && b.stride16 % 8 == 0 && aligned16(b.nbr16)),
                 "%s: nbr16 rows need a 16-byte aligned stride of >= max_nbr ids (stride16=%d)", b.who, b.stride16);
    DMET_REQUIRE(b.N >= 0 && b.N < (int64_t)2147483647, "%s: N out of range", b.who);
    DMET_REQUIRE(b.D >= 1 && b.D <= 8, "%s: D=%d not in [1,8]", b.who, b.D);
    DMET_REQUIRE(b.max_nbr >= 1, "%s: max_nbr=%d", b.who, b.max_nbr);
    if (b.N == 0 || b.B == 0) return 0;
    // nbr == NULL: only the uint16 rows are written (a caller whose consumers read those: the 255-wide int32 table is 294 MB
    // of address space at 288 000 nodes, its ~36 used slots per row 41 MB of 16-byte pieces: 12 of the kernel's 130 us)
    DMET_REQUIRE((b.qs ? b.qs->qx && b.qs->qptr : b.x != nullptr) && b.ptr && b.cnt && (b.nbr || (b.nbr16 && !b.fill)) &&
                 (b.ws || !windowed), "%s: null pointer", b.who);
    int32_t *order = nullptr;
    if (windowed) {
        DMET_REQUIRE(b.ws_bytes >= dmet_radius_workspace_bytes(b.N), "%s: workspace too small", b.who);
        order = reinterpret_cast<int32_t *>((reinterpret_cast<uintptr_t>(b.ws) + 255u) & ~(uintptr_t)255u);
    }
    // empty slots are -1: one coalesced fill instead of per-lane tail stores (294 MB for 288 000 x 255: the counted
    // form leaves them unwritten, its consumers go by cnt)
    if (b.fill) {
        hipError_t me = hipMemsetAsync(b.nbr, 0xff, sizeof(int32_t) * (size_t)b.N * (size_t)b.max_nbr, b.st);
        if (me != hipSuccess) return hip_fail(me, "hipMemsetAsync(nbr)");
    }
    if (windowed) {
        hipLaunchKernelGGL(radius_order_kernel, dim3((unsigned)b.B), dim3(kRadBins), 0, b.st, b.x, b.ptr, b.B, b.D, order);
        DMET_LAUNCH_CHECK("radius_order_kernel");
    }
    const float r2 = b.r * b.r;
    // four wavefronts per workgroup: 64 queries each, or (windowed) event-aligned wavefront ids
    const int64_t blocks = windowed ? (b.N / kWave + b.B + 1 + 3) / 4 : (b.N + 4 * kWave - 1) / (4 * kWave);
    // the D ladder, then the per x query-set ladder of each kernel (the window kernel has no two-set instance)
    with_int<2, 4, 8>(b.D <= 2 ? 2 : b.D <= 4 ? 4 : 8, [&](auto dp) {
        constexpr int DP = decltype(dp)::value;
        if (windowed)
            with_pack<true, false>(pp, nullptr, [&](auto... pack) {
                hipLaunchKernelGGL((radius_window_kernel<DP, decltype(pack)...>), dim3((unsigned)blocks), dim3(kWave * 4), 0,
                                   b.st, b.x, b.ptr, b.B, b.N, b.D, r2, b.max_nbr, b.skip_self, order, b.nbr, b.cnt, b.nbr16,
                                   b.stride16, pack...);
            });
        else
            with_pack<true, true>(pp, b.qs, [&](auto... pack) {
                hipLaunchKernelGGL((radius_kernel<DP, decltype(pack)...>), dim3((unsigned)blocks), dim3(kWave * 4), 0, b.st,
                                   b.x, b.ptr, b.B, b.N, b.D, r2, b.max_nbr, b.skip_self, b.nbr, b.cnt, pack...);
            });
    });
    DMET_LAUNCH_CHECK(windowed ? "radius_window_kernel" : b.qs ? "radius_kernel (two sets)" : "radius_kernel");
    return 0;
}

// ---- entries: each fills a RadiusBuild and calls radius_build once --------------------------------------------------
extern "C" int dmet_radius_f32(const float *x, const int64_t *ptr, int B, int64_t N, int D, float r, int max_nbr,
                               int skip_self, int32_t *nbr, int32_t *cnt, dmet_stream_t stream)
{
    return radius_build({"dmet_radius_f32", x, ptr, B, N, D, r, max_nbr, skip_self, true, nbr, cnt, as_stream(stream)});
}

extern "C" int dmet_radius_counted_f32(const float *x, const int64_t *ptr, int B, int64_t N, int D, float r,
                                       int max_nbr, int skip_self, int32_t *nbr, int32_t *cnt, dmet_stream_t stream)
{
    return radius_build({"dmet_radius_counted_f32", x, ptr, B, N, D, r, max_nbr, skip_self, false, nbr, cnt,
                         as_stream(stream)});
}

extern "C" int dmet_radius_windowed_local_f32(const float *x, const int64_t *ptr, int B, int64_t N, int D, float r,
                                              int max_nbr, int skip_self, int fill, int32_t *nbr, int32_t *cnt,
                                              uint16_t *nbr16, int stride16, void *ws, size_t ws_bytes,
                                              dmet_stream_t stream)
{
    return radius_build({"dmet_radius_windowed_local_f32", x, ptr, B, N, D, r, max_nbr, skip_self, fill != 0, nbr, cnt,
                         as_stream(stream), RadiusForm::Windowed, ws, ws_bytes, nbr16, stride16});
}

extern "C" int dmet_radius_windowed_f32(const float *x, const int64_t *ptr, int B, int64_t N, int D, float r,
                                        int max_nbr, int skip_self, int fill, int32_t *nbr, int32_t *cnt, void *ws,
                                        size_t ws_bytes, dmet_stream_t stream)
{
    return radius_build({"dmet_radius_windowed_f32", x, ptr, B, N, D, r, max_nbr, skip_self, fill != 0, nbr, cnt,
                         as_stream(stream), RadiusForm::Windowed, ws, ws_bytes});
}

// Periodic coordinates (train.py:47-48: phi wraps at +-pi).  period[c] > 0: circumference of coordinate c; 0: plain.
extern "C" int dmet_radius_periodic_f32(const float *x, const int64_t *ptr, int B, int64_t N, int D, float r,
                                        int max_nbr, int skip_self, int fill, const float *period, int32_t *nbr,
                                        int32_t *cnt, dmet_stream_t stream)
{
    return radius_build({"dmet_radius_periodic_f32", x, ptr, B, N, D, r, max_nbr, skip_self, fill != 0, nbr, cnt,
                         as_stream(stream), RadiusForm::AllPairs, nullptr, 0, nullptr, 0, period, true});
}

extern "C" int dmet_radius_windowed_periodic_f32(const float *x, const int64_t *ptr, int B, int64_t N, int D, float r,
                                                 int max_nbr, int skip_self, int fill, const float *period,
                                                 int32_t *nbr, int32_t *cnt, uint16_t *nbr16, int stride16, void *ws,
                                                 size_t ws_bytes, dmet_stream_t stream)
{
    return radius_build({"dmet_radius_windowed_periodic_f32", x, ptr, B, N, D, r, max_nbr, skip_self, fill != 0, nbr, cnt,
                         as_stream(stream), RadiusForm::Windowed, ws, ws_bytes, nbr16, stride16, period, true});
}

// ---- two point sets: queries y against candidates x of the same events (torch_cluster.radius) -----------------------
extern "C" int dmet_radius_xy_f32(const float *x, const int64_t *ptr_x, int64_t Nx, const float *y, const int64_t *ptr_y,
                                  int64_t Ny, int B, int D, float r, int max_nbr, const float *period, int fill,
                                  int32_t *nbr, int32_t *cnt, dmet_stream_t stream)
{
    const char *who = "dmet_radius_xy_f32";
    DMET_REQUIRE(Nx >= 0 && Nx < (int64_t)2147483647 && Ny >= 0 && Ny < (int64_t)2147483647,
                 "%s: Nx=%lld / Ny=%lld out of range", who, (long long)Nx, (long long)Ny);
    DMET_REQUIRE(B >= 0, "%s: B=%d", who, B);
    if (period) {   // a bad period is reported ahead of the two checks below; radius_build reads it again for the kernel
        RadPeriod per;
        bool any = false;
        const int rc = radius_periods(who, D, period, &per, &any);
        if (rc) return rc;
    }
    if (Ny > 0) {   // (an empty query set still gets radius_build's checks of D and max_nbr)
        DMET_REQUIRE(B >= 1, "%s: %lld queries but no event", who, (long long)Ny);
        DMET_REQUIRE((x || Nx == 0) && ptr_x && y && ptr_y && nbr && cnt, "%s: null pointer", who);
    }
    const KnnQuerySet qs{y, ptr_y};
    return radius_build({who, x, ptr_x, B, Ny, D, r, max_nbr, 0, fill != 0, nbr, cnt, as_stream(stream),
                         RadiusForm::AllPairs, nullptr, 0, nullptr, 0, period, false, &qs});
}

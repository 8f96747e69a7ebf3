// segment.hip -- the rest of the scatter family over fp32 rows src[E, H] grouped by rowptr[rows + 1]: mean, min, softmax,
// log_softmax and logsumexp with their backward passes.  (segment_reduce_kernel of edgeconv.hip walks a row with one lane
// per channel: right for the 16 neighbours of a node, not for the 4500 nodes of an event.)
//
// Lane layout, all kernels: a team owns one (row, block of CL channels) pair.  Its lanes are CL channel lanes (lane % CL;
// adjacent lanes read adjacent channels) times entry lanes (adjacent entry lanes read adjacent entries, so a narrow src
// is read in contiguous runs too).  Two forms:
//   wavefront form  a team is one wavefront: 64 / CL entry lanes; a 256-thread workgroup holds four teams;
//   workgroup form  a team is one 256-thread workgroup: 4 * 64 / CL entry lanes; chosen by the host when the caller's
//                   max_len hint reaches kSegLongRow (an event of thousands of nodes), for every row of that call.
// CL is 1 for H == 1, 4 up to H = 4, 16 up to H = 16, then 32 and 64 in the wavefront form; the workgroup form stops at
// 16 (a wider src becomes more channel blocks, and so more workgroups for its few long rows).
//
// A row is taken in steps of seg_step(CL) entries per entry lane (4; 16 from CL = 32 on, where a wavefront has one or
// two entry lanes), loaded before the first is used.  With S entry lanes, entry lane g takes entries base + g + k*S
// (k < step); for H == 1 it takes base + 4*g + k instead, as one 16-byte load or store wherever the row's first
// position is 16-byte aligned (the entries a lane owns do not depend on the alignment).  A row that fits one step of
// its team -- the 16 neighbours of a node at any H -- stays in registers between the reducing and the writing pass.
// Each lane folds its entries in ascending order; the entry lanes of a wavefront combine by an xor butterfly (offsets 32
// down to CL) after which all hold the same bits; the four wavefronts of a workgroup team combine through LDS in
// wavefront order.  No float atomics, every output element is written once, and the order of every sum
// depends on H and the form only.  A span is clamped to [0, E] (row_span of row_softmax.h): a malformed rowptr gives
// wrong rows, never an access outside src.  Positions before the first row and after the last are written as zeros by
// the kernels with a per-entry output, so these outputs are fully written, each element once, whenever rowptr is
// non-decreasing.  A rowptr that is not leaves the positions of a gap between two rows unwritten and those two rows
// share written twice (by two teams, in no order): in bounds, but neither defined nor the same from run to run.
#include <math.h>

#include "common.h"

namespace dmet {
namespace {

constexpr int kSegThreads = 256;
constexpr int kSegWaves = kSegThreads / kWave;
constexpr int kSegMaxStep = 16;
// entries an entry lane loads before it uses the first
constexpr int seg_step(int CL) { return CL >= 32 ? kSegMaxStep : 4; }
constexpr int kSegLongRow = 1024;      // max_len hint from which a workgroup owns a row

struct Seg {
    int64_t row, lo;      // the row and its first position
    int n;                // its length
    int c;                // this lane's channel
    int ge;               // this lane's entry lane in the team
    bool on;              // c < H
};

template <int CL, bool BLOCK>
struct Team {
    static constexpr int EL = kWave / CL;                          // entry lanes of a wavefront
    static constexpr int S = BLOCK ? kSegWaves * EL : EL;          // entry lanes of the team
    static constexpr int kStep = seg_step(CL);
    static constexpr int kStride = kStep * S;                      // entries per step of the team
};

// false past the launch's teams; a whole team leaves together (a wavefront, or the workgroup before any barrier)
template <int CL, bool BLOCK>
__device__ __forceinline__ bool seg_take(const int32_t *__restrict__ rowptr, int64_t rows, int64_t E, int H, Seg &s)
{
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    const int nblk = (H + CL - 1) / CL;
    const int64_t unit = BLOCK ? (int64_t)blockIdx.x : (int64_t)blockIdx.x * kSegWaves + wave;
    if (unit >= rows * nblk) return false;
    s.row = unit / nblk;
    s.c = (int)(unit - s.row * nblk) * CL + lane % CL;
    s.on = s.c < H;
    s.ge = (BLOCK ? wave * Team<CL, BLOCK>::EL : 0) + lane / CL;
    s.lo = min(max((int64_t)rowptr[s.row], (int64_t)0), E);
    const int64_t hi = min(max((int64_t)rowptr[s.row + 1], s.lo), E);
    s.n = (int)(hi - s.lo);
    return true;
}

// entry k of entry lane ge in the step at base
template <int CL, int S>
__device__ __forceinline__ int seg_entry(int base, int ge, int k)
{
    return CL == 1 ? base + seg_step(CL) * ge + k : base + ge + k * S;
}

// p: the row's first position at this lane's channel; vec: p is 16-byte aligned (CL == 1 only)
template <int CL, int S>
__device__ __forceinline__ void seg_load(float (&v)[seg_step(CL)], const float *__restrict__ p, int H, const Seg &s, int base,
                                         bool vec, float fill)
{
    if constexpr (CL == 1) {
        const int t = base + 4 * s.ge;
        if (vec && t + 4 <= s.n) {
            const float4 q = *reinterpret_cast<const float4 *>(p + t);
            v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
            return;
        }
    }
#pragma unroll
    for (int k = 0; k < seg_step(CL); ++k) {
        const int t = seg_entry<CL, S>(base, s.ge, k);
        v[k] = (s.on && t < s.n) ? p[(int64_t)t * H] : fill;
    }
}

template <int CL, int S>
__device__ __forceinline__ void seg_store(const float (&v)[seg_step(CL)], float *__restrict__ p, int H, const Seg &s, int base,
                                          bool vec)
{
    if constexpr (CL == 1) {
        const int t = base + 4 * s.ge;
        if (vec && t + 4 <= s.n) {
            *reinterpret_cast<float4 *>(p + t) = make_float4(v[0], v[1], v[2], v[3]);
            return;
        }
    }
#pragma unroll
    for (int k = 0; k < seg_step(CL); ++k) {
        const int t = seg_entry<CL, S>(base, s.ge, k);
        if (s.on && t < s.n) p[(int64_t)t * H] = v[k];
    }
}

// zeros at the positions no row owns: before the first row and after the last
template <int S>
__device__ __forceinline__ void seg_fill_outside(float *__restrict__ out, const Seg &s, int64_t rows, int64_t E, int H)
{
    if (!s.on) return;
    if (s.row == 0)
        for (int64_t t = s.ge; t < s.lo; t += S) out[t * H + s.c] = 0.f;
    if (s.row == rows - 1)
        for (int64_t t = s.lo + s.n + s.ge; t < E; t += S) out[t * H + s.c] = 0.f;
}

// ---- what a lane folds, and how two partial results of one row combine (each commutative bit for bit) ----------------

struct SumOp {
    float v;
    __device__ __forceinline__ void merge(const SumOp &o) { v += o.v; }
};

// the running softmax of a row: m its maximum, l = sum expf(s - m); m == -inf: no finite entry yet, l == 0
struct SoftOp {
    float m, l;
    // one step of a lane: its maximum first, then one rescale of l (by exactly 1 when the maximum stays) and the step's
    // terms in ascending order -- N independent expf instead of a chain of N rescales
    template <int N>
    __device__ __forceinline__ void add(const float (&v)[N])
    {
        float mx = v[0];
#pragma unroll
        for (int k = 1; k < N; ++k) mx = fmaxf(mx, v[k]);
        const float mn = fmaxf(m, mx);
        if (mn == -INFINITY) return;
        float sum = 0.f;
#pragma unroll
        for (int k = 0; k < N; ++k) sum += expf(v[k] - mn);
        l = l * expf(m - mn) + sum;
        m = mn;
    }
    __device__ __forceinline__ void merge(const SoftOp &o)
    {
        const float mn = fmaxf(m, o.m);
        l = (mn == -INFINITY) ? 0.f : l * expf(m - mn) + o.l * expf(o.m - mn);
        m = mn;
    }
};

// the minimum and its position: a < 0 none yet; the lowest position wins a tie (R4; -0.0 and +0.0 tie)
struct MinOp {
    float v;
    int a;
    __device__ __forceinline__ void add(float x, int pos)
    {
        if (a < 0 || x < v) v = x, a = pos;
    }
    __device__ __forceinline__ void merge(const MinOp &o)
    {
        if (o.a >= 0 && (a < 0 || o.v < v || (o.v == v && o.a < a))) v = o.v, a = o.a;
    }
};

template <class Op>
__device__ __forceinline__ Op seg_shfl_xor(const Op &x, int off)
{
    static_assert(sizeof(Op) % 4 == 0 && sizeof(Op) <= 8, "one or two words");
    Op r;
    const int *src = reinterpret_cast<const int *>(&x);
    int *dst = reinterpret_cast<int *>(&r);
#pragma unroll
    for (int w = 0; w < (int)(sizeof(Op) / 4); ++w) dst[w] = __shfl_xor(src[w], off, kWave);
    return r;
}

// the team's result in every lane: the butterfly over a wavefront's entry lanes, then (workgroup form) the wavefronts in
// order through LDS.  Every thread of a workgroup team calls it, the same number of times.
template <int CL, bool BLOCK, class Op>
__device__ __forceinline__ void seg_combine(Op &x)
{
#pragma unroll
    for (int off = kWave / 2; off >= CL; off >>= 1) x.merge(seg_shfl_xor(x, off));
    if constexpr (BLOCK) {
        __shared__ Op part[kSegWaves][CL];
        const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
        if (lane < CL) part[wave][lane] = x;
        __syncthreads();
        x = part[0][lane % CL];
#pragma unroll
        for (int w = 1; w < kSegWaves; ++w) x.merge(part[w][lane % CL]);
        __syncthreads();        // the next combine of this kernel writes the same words
    }
}

static __device__ __forceinline__ bool seg_aligned(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// ---- kernels ----------------------------------------------------------------------------------------------------------

enum { kSoftmax = 0, kLogSoftmax = 1, kLogSumExp = 2, kMean = 3 };

// mean (arg NULL): out[i,c] = sum / max(n, 1).  min: out[i,c], arg[i,c] = the position in src, -1 and 0 for an empty row.
template <int CL, bool BLOCK, bool IS_MIN>
__global__ __launch_bounds__(kSegThreads) void seg_reduce_kernel(const float *__restrict__ src,
                                                                 const int32_t *__restrict__ rowptr, int64_t rows, int64_t E,
                                                                 int H, float *__restrict__ out, int32_t *__restrict__ arg)
{
    using T = Team<CL, BLOCK>;
    Seg s;
    if (!seg_take<CL, BLOCK>(rowptr, rows, E, H, s)) return;
    const float *p = src + s.lo * H + s.c;
    const bool vec = seg_aligned(p);
    SumOp sum{0.f};
    MinOp best{0.f, -1};
    for (int base = 0; base < s.n; base += T::kStride) {
        float v[T::kStep];
        seg_load<CL, T::S>(v, p, H, s, base, vec, 0.f);
#pragma unroll
        for (int k = 0; k < T::kStep; ++k) {
            if constexpr (IS_MIN) {
                const int t = seg_entry<CL, T::S>(base, s.ge, k);
                if (t < s.n) best.add(v[k], (int)(s.lo + t));
            } else {
                sum.v += v[k];
            }
        }
    }
    if constexpr (IS_MIN) {
        seg_combine<CL, BLOCK>(best);
        if (s.on && s.ge == 0) {
            out[s.row * H + s.c] = best.a < 0 ? 0.f : best.v;
            arg[s.row * H + s.c] = best.a;
        }
    } else {
        seg_combine<CL, BLOCK>(sum);
        if (s.on && s.ge == 0) out[s.row * H + s.c] = sum.v / (float)max(s.n, 1);
    }
}

// (m, l) of the row in one online pass, then one writing pass: y = expf(s - m) / l (kSoftmax) or (s - m) - logf(l)
// (kLogSoftmax); lse[i,c] = m + logf(l), 0 for an empty row.  kLogSumExp: lse only.
template <int CL, bool BLOCK, int MODE>
__global__ __launch_bounds__(kSegThreads) void seg_softmax_fwd_kernel(const float *__restrict__ src,
                                                                      const int32_t *__restrict__ rowptr, int64_t rows,
                                                                      int64_t E, int H, float *__restrict__ y,
                                                                      float *__restrict__ lse)
{
    using T = Team<CL, BLOCK>;
    Seg s;
    if (!seg_take<CL, BLOCK>(rowptr, rows, E, H, s)) return;
    const float *p = src + s.lo * H + s.c;
    const bool vec = seg_aligned(p);
    SoftOp ml{-INFINITY, 0.f};
    float v[T::kStep];
    for (int base = 0; base < s.n; base += T::kStride) {
        seg_load<CL, T::S>(v, p, H, s, base, vec, -INFINITY);      // -inf past the row: adds nothing
        ml.add(v);
    }
    seg_combine<CL, BLOCK>(ml);
    const float logl = logf(ml.l);
    if (s.on && s.ge == 0) lse[s.row * H + s.c] = s.n > 0 ? ml.m + logl : 0.f;
    if constexpr (MODE != kLogSumExp) {
        float *q = y + s.lo * H + s.c;
        const bool vecq = vec && seg_aligned(q);
        const bool kept = s.n <= T::kStride;       // the row's one step is still in v
        for (int base = 0; base < s.n; base += T::kStride) {
            if (!kept) seg_load<CL, T::S>(v, p, H, s, base, vecq, 0.f);
#pragma unroll
            for (int k = 0; k < T::kStep; ++k) v[k] = MODE == kSoftmax ? expf(v[k] - ml.m) / ml.l : (v[k] - ml.m) - logl;
            seg_store<CL, T::S>(v, q, H, s, base, vecq);
        }
        seg_fill_outside<T::S>(y, s, rows, E, H);
    }
}

// kSoftmax     a = y,   g[E,H]:            g_src = y * (g - sum_row y*g)
// kLogSoftmax  a = y,   g[E,H]:            g_src = g - expf(y) * sum_row g
// kLogSumExp   a = src, g[rows,H], o = out: g_src = g[i,c] * expf(s - out[i,c])
// kMean                 g[rows,H]:         g_src = g[i,c] / max(n, 1)
template <int CL, bool BLOCK, int MODE>
__global__ __launch_bounds__(kSegThreads) void seg_bwd_kernel(const float *__restrict__ a, const float *__restrict__ g,
                                                              const float *__restrict__ o,
                                                              const int32_t *__restrict__ rowptr, int64_t rows, int64_t E,
                                                              int H, float *__restrict__ g_src)
{
    using T = Team<CL, BLOCK>;
    Seg s;
    if (!seg_take<CL, BLOCK>(rowptr, rows, E, H, s)) return;
    constexpr bool kPerEntry = MODE == kSoftmax || MODE == kLogSoftmax;      // g is per entry and a row sum is needed
    const float *pa = MODE == kMean ? nullptr : a + s.lo * H + s.c;
    const float *pg = kPerEntry ? g + s.lo * H + s.c : nullptr;
    float *q = g_src + s.lo * H + s.c;
    const bool vec = seg_aligned(q) && (MODE == kMean || seg_aligned(pa)) && (!kPerEntry || seg_aligned(pg));
    float r = 0.f, ov = 0.f;       // the row's scalar: the sum, or the upstream gradient of the row
    float va[T::kStep], vg[T::kStep];
    const bool kept = kPerEntry && s.n <= T::kStride;       // the row's one step stays in va, vg
    if constexpr (kPerEntry) {
        SumOp sum{0.f};
        for (int base = 0; base < s.n; base += T::kStride) {
            seg_load<CL, T::S>(vg, pg, H, s, base, vec, 0.f);
            if constexpr (MODE == kSoftmax) {
                seg_load<CL, T::S>(va, pa, H, s, base, vec, 0.f);
#pragma unroll
                for (int k = 0; k < T::kStep; ++k) sum.v += va[k] * vg[k];
            } else {
                if (kept) seg_load<CL, T::S>(va, pa, H, s, base, vec, 0.f);
#pragma unroll
                for (int k = 0; k < T::kStep; ++k) sum.v += vg[k];
            }
        }
        seg_combine<CL, BLOCK>(sum);
        r = sum.v;
    } else if (s.on) {
        r = g[s.row * H + s.c];
        if constexpr (MODE == kLogSumExp) ov = o[s.row * H + s.c];
        if constexpr (MODE == kMean) r = r / (float)max(s.n, 1);
    }
    for (int base = 0; base < s.n; base += T::kStride) {
        if (!kept) {
            if constexpr (MODE != kMean) seg_load<CL, T::S>(va, pa, H, s, base, vec, 0.f);
            if constexpr (kPerEntry) seg_load<CL, T::S>(vg, pg, H, s, base, vec, 0.f);
        }
#pragma unroll
        for (int k = 0; k < T::kStep; ++k) {
            if constexpr (MODE == kSoftmax) vg[k] = va[k] * (vg[k] - r);
            else if constexpr (MODE == kLogSoftmax) vg[k] = vg[k] - expf(va[k]) * r;
            else if constexpr (MODE == kLogSumExp) vg[k] = r * expf(va[k] - ov);
            else vg[k] = r;
        }
        seg_store<CL, T::S>(vg, q, H, s, base, vec);
    }
    seg_fill_outside<T::S>(g_src, s, rows, E, H);
}

// ---- host side --------------------------------------------------------------------------------------------------------

int seg_check(const char *who, int64_t rows, int64_t E, int H, int max_len)
{
    DMET_REQUIRE(rows >= 0 && E >= 0 && H > 0 && max_len >= 0, "%s: bad sizes rows=%lld E=%lld H=%d max_len=%d", who,
                 (long long)rows, (long long)E, H, max_len);
    // a row's walk steps an int past its length by less than one stride of the team
    DMET_REQUIRE(E < (int64_t)2147483647 - kSegMaxStep * kSegThreads && rows < (int64_t)2147483647,
                 "%s: rows=%lld or E=%lld out of range", who, (long long)rows, (long long)E);
    // a launch covers rows * ceil(H / CL) teams, CL >= min(H, 16) in the workgroup form
    DMET_REQUIRE(rows * (int64_t)((H + 15) / 16 + 1) < (int64_t)2147483647, "%s: rows*H out of range", who);
    return 0;
}

// f(CL, BLOCK) as integral constants for a width and a max_len hint (0: unknown, the wavefront form)
template <class F>
void seg_dispatch(int H, int max_len, F &&f)
{
    using std::integral_constant;
    const bool block = max_len >= kSegLongRow;
    with_flags([&](auto b) {
        constexpr bool kBlockForm = decltype(b)::value;
        if (H == 1) f(integral_constant<int, 1>{}, b);
        else if (H <= 4) f(integral_constant<int, 4>{}, b);
        else if (H <= 16 || kBlockForm) f(integral_constant<int, 16>{}, b);
        else if constexpr (!kBlockForm) {
            if (H <= 32) f(integral_constant<int, 32>{}, b);
            else f(integral_constant<int, 64>{}, b);
        }
    }, block);
}

template <int CL, bool BLOCK>
dim3 seg_grid(int64_t rows, int H)
{
    const int64_t units = rows * ((H + CL - 1) / CL);
    return dim3((unsigned)(BLOCK ? units : (units + kSegWaves - 1) / kSegWaves));
}

}  // namespace
}  // namespace dmet

using namespace dmet;

extern "C" int dmet_segment_mean_f32(const float *src, const int32_t *rowptr, int64_t rows, int64_t E, int H, int max_len,
                                     float *out, dmet_stream_t stream)
{
    if (int rc = seg_check("dmet_segment_mean_f32", rows, E, H, max_len)) return rc;
    if (rows == 0) return 0;
    DMET_REQUIRE(rowptr && out && (src || E == 0), "dmet_segment_mean_f32: null pointer");
    seg_dispatch(H, max_len, [&](auto cl, auto b) {
        constexpr int CL = decltype(cl)::value;
        constexpr bool B = decltype(b)::value;
        hipLaunchKernelGGL((seg_reduce_kernel<CL, B, false>), (seg_grid<CL, B>(rows, H)),
                           dim3(kSegThreads), 0, as_stream(stream), src, rowptr, rows, E, H, out, (int32_t *)nullptr);
    });
    DMET_LAUNCH_CHECK("seg_reduce_kernel (mean)");
    return 0;
}

extern "C" int dmet_segment_min_f32(const float *src, const int32_t *rowptr, int64_t rows, int64_t E, int H, int max_len,
                                    float *out, int32_t *arg, dmet_stream_t stream)
{
    if (int rc = seg_check("dmet_segment_min_f32", rows, E, H, max_len)) return rc;
    if (rows == 0) return 0;
    DMET_REQUIRE(rowptr && out && arg && (src || E == 0), "dmet_segment_min_f32: null pointer");
    seg_dispatch(H, max_len, [&](auto cl, auto b) {
        constexpr int CL = decltype(cl)::value;
        constexpr bool B = decltype(b)::value;
        hipLaunchKernelGGL((seg_reduce_kernel<CL, B, true>), (seg_grid<CL, B>(rows, H)),
                           dim3(kSegThreads), 0, as_stream(stream), src, rowptr, rows, E, H, out, arg);
    });
    DMET_LAUNCH_CHECK("seg_reduce_kernel (min)");
    return 0;
}

extern "C" int dmet_segment_mean_bwd_f32(const float *g_out, const int32_t *rowptr, int64_t rows, int64_t E, int H,
                                         int max_len, float *g_src, dmet_stream_t stream)
{
    if (int rc = seg_check("dmet_segment_mean_bwd_f32", rows, E, H, max_len)) return rc;
    if (rows == 0 || E == 0) return 0;
    DMET_REQUIRE(g_out && rowptr && g_src, "dmet_segment_mean_bwd_f32: null pointer");
    seg_dispatch(H, max_len, [&](auto cl, auto b) {
        constexpr int CL = decltype(cl)::value;
        constexpr bool B = decltype(b)::value;
        hipLaunchKernelGGL((seg_bwd_kernel<CL, B, kMean>), (seg_grid<CL, B>(rows, H)),
                           dim3(kSegThreads), 0, as_stream(stream), (const float *)nullptr, g_out, (const float *)nullptr,
                           rowptr, rows, E, H, g_src);
    });
    DMET_LAUNCH_CHECK("seg_bwd_kernel (mean)");
    return 0;
}

extern "C" int dmet_segment_softmax_fwd_f32(const float *src, const int32_t *rowptr, int64_t rows, int64_t E, int H,
                                            int log, int max_len, float *y, float *lse, dmet_stream_t stream)
{
    if (int rc = seg_check("dmet_segment_softmax_fwd_f32", rows, E, H, max_len)) return rc;
    if (rows == 0) return 0;
    DMET_REQUIRE(rowptr && lse && ((src && y) || E == 0), "dmet_segment_softmax_fwd_f32: null pointer");
    seg_dispatch(H, max_len, [&](auto cl, auto b) {
        constexpr int CL = decltype(cl)::value;
        constexpr bool B = decltype(b)::value;
        if (log)
            hipLaunchKernelGGL((seg_softmax_fwd_kernel<CL, B, kLogSoftmax>), (seg_grid<CL, B>(rows, H)),
                               dim3(kSegThreads), 0, as_stream(stream), src, rowptr, rows, E, H, y, lse);
        else
            hipLaunchKernelGGL((seg_softmax_fwd_kernel<CL, B, kSoftmax>), (seg_grid<CL, B>(rows, H)),
                               dim3(kSegThreads), 0, as_stream(stream), src, rowptr, rows, E, H, y, lse);
    });
    DMET_LAUNCH_CHECK("seg_softmax_fwd_kernel");
    return 0;
}

extern "C" int dmet_segment_softmax_bwd_f32(const float *y, const float *g, const int32_t *rowptr, int64_t rows, int64_t E,
                                            int H, int log, int max_len, float *g_src, dmet_stream_t stream)
{
    if (int rc = seg_check("dmet_segment_softmax_bwd_f32", rows, E, H, max_len)) return rc;
    if (rows == 0 || E == 0) return 0;
    DMET_REQUIRE(y && g && rowptr && g_src, "dmet_segment_softmax_bwd_f32: null pointer");
    seg_dispatch(H, max_len, [&](auto cl, auto b) {
        constexpr int CL = decltype(cl)::value;
        constexpr bool B = decltype(b)::value;
        if (log)
            hipLaunchKernelGGL((seg_bwd_kernel<CL, B, kLogSoftmax>), (seg_grid<CL, B>(rows, H)),
                               dim3(kSegThreads), 0, as_stream(stream), y, g, (const float *)nullptr, rowptr, rows, E, H,
                               g_src);
        else
            hipLaunchKernelGGL((seg_bwd_kernel<CL, B, kSoftmax>), (seg_grid<CL, B>(rows, H)),
                               dim3(kSegThreads), 0, as_stream(stream), y, g, (const float *)nullptr, rowptr, rows, E, H,
                               g_src);
    });
    DMET_LAUNCH_CHECK("seg_bwd_kernel (softmax)");
    return 0;
}

extern "C" int dmet_segment_logsumexp_f32(const float *src, const int32_t *rowptr, int64_t rows, int64_t E, int H,
                                          int max_len, float *out, dmet_stream_t stream)
{
    if (int rc = seg_check("dmet_segment_logsumexp_f32", rows, E, H, max_len)) return rc;
    if (rows == 0) return 0;
    DMET_REQUIRE(rowptr && out && (src || E == 0), "dmet_segment_logsumexp_f32: null pointer");
    seg_dispatch(H, max_len, [&](auto cl, auto b) {
        constexpr int CL = decltype(cl)::value;
        constexpr bool B = decltype(b)::value;
        hipLaunchKernelGGL((seg_softmax_fwd_kernel<CL, B, kLogSumExp>), (seg_grid<CL, B>(rows, H)),
                           dim3(kSegThreads), 0, as_stream(stream), src, rowptr, rows, E, H, (float *)nullptr, out);
    });
    DMET_LAUNCH_CHECK("seg_softmax_fwd_kernel (logsumexp)");
    return 0;
}

extern "C" int dmet_segment_logsumexp_bwd_f32(const float *src, const float *out, const float *g_out,
                                              const int32_t *rowptr, int64_t rows, int64_t E, int H, int max_len,
                                              float *g_src, dmet_stream_t stream)
{
    if (int rc = seg_check("dmet_segment_logsumexp_bwd_f32", rows, E, H, max_len)) return rc;
    if (rows == 0 || E == 0) return 0;
    DMET_REQUIRE(src && out && g_out && rowptr && g_src, "dmet_segment_logsumexp_bwd_f32: null pointer");
    seg_dispatch(H, max_len, [&](auto cl, auto b) {
        constexpr int CL = decltype(cl)::value;
        constexpr bool B = decltype(b)::value;
        hipLaunchKernelGGL((seg_bwd_kernel<CL, B, kLogSumExp>), (seg_grid<CL, B>(rows, H)),
                           dim3(kSegThreads), 0, as_stream(stream), src, g_out, out, rowptr, rows, E, H, g_src);
    });
    DMET_LAUNCH_CHECK("seg_bwd_kernel (logsumexp)");
    return 0;
}

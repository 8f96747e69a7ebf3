// event_norm.hip -- per-event column statistics and the elementwise pass of the normalisation layers (GraphNorm,
// InstanceNorm, LayerNorm, PairNorm, GraphSizeNorm, MeanSubtractionNorm) over fp32 rows x[N, F] grouped by an int32
// rowptr[B + 1]: event b owns the rows [rowptr[b], rowptr[b+1]), each span clamped to [0, N] (as row_span / segment.hip).
//
// Reductions (event_moments, event_dots): a team owns one (event, block of CL channels) pair and is one workgroup:
//   wavefront form  64 threads;   workgroup form  1024 threads, chosen by the host when the caller's max_len hint reaches
//   kEvLongRow (an event of thousands of nodes), for every event of that call.
// CL is 1 for F == 1, 4 up to F = 4, else 16 (a wider x becomes more channel blocks).  The team's lanes are CL channel
// lanes (lane % CL: adjacent lanes read adjacent channels) times S = threads / CL entry lanes; entry lane ge takes the
// rows ge, ge + S, ge + 2S, ... of the event in ascending order, kEvStep of them loaded before the first is used.  The
// entry lanes of a wavefront combine by an xor butterfly (offsets 32 down to CL), the wavefronts of a workgroup team
// through LDS in wavefront order.  The variance is taken in a second walk over the same rows (in L2 by then), centred on
// the event's own rounded mean: never a difference of two means.  One event is never split over teams: the second walk
// needs the event's final mean, and there is no scratch and no float atomic to merge partial sums through.
//
// Elementwise pass (event_affine): a 256-thread workgroup owns a run of whole rows of about kAffPerBlock elements and
// finds the event of its first row by one binary search over rowptr (uniform over the workgroup); it then walks the
// events that reach into its run.  Lanes read and write consecutive floats.  The operation order is fixed
// (-ffp-contract=off): (x - shift) * k1 + k0, and with g: g * ka + that.
//
// Every output element is written exactly once when rowptr is non-decreasing, the order of every sum depends on F and
// the form only: the same bits from run to run and on unaligned views (no load is wider than a float).  A malformed rowptr
// gives wrong rows, never an access outside x.
#include <math.h>

#include "common.h"

namespace dmet {
namespace {

constexpr int kEvStep = 8;             // rows an entry lane loads before it uses the first
constexpr int kEvLongRow = 1024;       // max_len hint from which the 1024-thread form runs
constexpr int kEvBlockWaves = 16;      // wavefronts of that form
constexpr int kAffThreads = 256;
constexpr int kAffUnroll = 4;
constexpr int kAffPerBlock = 4096;     // elements a workgroup of event_affine owns, about

struct Ev {
    int64_t b, lo;        // the event and its first row
    int n;                // its length
    int c;                // this lane's channel
    int ge;               // this lane's entry lane in the team
    bool on;              // c < F
};

template <int CL, int W>
__device__ __forceinline__ void ev_take(const int32_t *__restrict__ rowptr, int64_t N, int F, Ev &s)
{
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    const int nblk = (F + CL - 1) / CL;
    s.b = (int64_t)blockIdx.x / nblk;
    s.c = (int)((int64_t)blockIdx.x - s.b * nblk) * CL + lane % CL;
    s.on = s.c < F;
    s.ge = wave * (kWave / CL) + lane / CL;
    s.lo = min(max((int64_t)rowptr[s.b], (int64_t)0), N);
    const int64_t hi = min(max((int64_t)rowptr[s.b + 1], s.lo), N);
    s.n = (int)(hi - s.lo);
}

// the team's sum in every lane; every thread of the workgroup calls it, the same number of times
template <int CL, int W>
__device__ __forceinline__ float ev_sum(float v)
{
#pragma unroll
    for (int off = kWave / 2; off >= CL; off >>= 1) v += __shfl_xor(v, off, kWave);
    if constexpr (W > 1) {
        __shared__ float part[W][CL];
        const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
        if (lane < CL) part[wave][lane] = v;
        __syncthreads();
        v = part[0][lane % CL];
#pragma unroll
        for (int w = 1; w < W; ++w) v += part[w][lane % CL];
        __syncthreads();        // the next sum of this kernel writes the same words
    }
    return v;
}

// v[k] = row base + ge + k*S of the event at this lane's channel, `ok[k]` whether there is such a row
template <int S>
__device__ __forceinline__ void ev_load(float (&v)[kEvStep], bool (&ok)[kEvStep], const float *__restrict__ p, int F,
                                        const Ev &s, int base)
{
#pragma unroll
    for (int k = 0; k < kEvStep; ++k) {
        const int t = base + s.ge + k * S;
        ok[k] = s.on && t < s.n;
        v[k] = ok[k] ? p[(int64_t)t * F] : 0.f;
    }
}

// mean[b,c] = fp32 sum / (float)n, var[b,c] = (sum of (x - mean)^2) / (float)n; 0 and 0 for an empty event
template <int CL, int W>
__global__ __launch_bounds__(kWave * W) void event_moments_kernel(const float *__restrict__ x,
                                                                  const int32_t *__restrict__ rowptr, int64_t N, int F,
                                                                  float *__restrict__ mean, float *__restrict__ var)
{
    constexpr int S = W * kWave / CL;
    Ev s;
    ev_take<CL, W>(rowptr, N, F, s);
    const float *p = x + s.lo * F + s.c;
    float v[kEvStep];
    bool ok[kEvStep];
    float sum = 0.f;
    for (int base = 0; base < s.n; base += kEvStep * S) {
        ev_load<S>(v, ok, p, F, s, base);
#pragma unroll
        for (int k = 0; k < kEvStep; ++k) sum += v[k];         // a missing row adds +0: no bit changes
    }
    sum = ev_sum<CL, W>(sum);
    const float m = s.n > 0 ? sum / (float)s.n : 0.f;
    float ss = 0.f;
    for (int base = 0; base < s.n; base += kEvStep * S) {
        ev_load<S>(v, ok, p, F, s, base);
#pragma unroll
        for (int k = 0; k < kEvStep; ++k) {
            const float d = ok[k] ? v[k] - m : 0.f;
            ss += d * d;
        }
    }
    ss = ev_sum<CL, W>(ss);
    if (s.on && s.ge == 0) {
        mean[s.b * F + s.c] = m;
        var[s.b * F + s.c] = s.n > 0 ? ss / (float)s.n : 0.f;
    }
}

// s1[b,c] = sum g;  DOTS: s2[b,c] = sum g * ((x - shift[b,c]) * scale[b,c])
template <int CL, int W, bool DOTS>
__global__ __launch_bounds__(kWave * W) void event_dots_kernel(const float *__restrict__ g, const float *__restrict__ x,
                                                               const int32_t *__restrict__ rowptr, int64_t N, int F,
                                                               const float *__restrict__ shift,
                                                               const float *__restrict__ scale, float *__restrict__ s1,
                                                               float *__restrict__ s2)
{
    constexpr int S = W * kWave / CL;
    Ev s;
    ev_take<CL, W>(rowptr, N, F, s);
    const float *pg = g + s.lo * F + s.c;
    const float *px = DOTS ? x + s.lo * F + s.c : nullptr;
    float sh = 0.f, sc = 0.f;
    if (DOTS && s.on) sh = shift[s.b * F + s.c], sc = scale[s.b * F + s.c];
    float vg[kEvStep], vx[kEvStep];
    bool ok[kEvStep];
    float a1 = 0.f, a2 = 0.f;
    for (int base = 0; base < s.n; base += kEvStep * S) {
        ev_load<S>(vg, ok, pg, F, s, base);
        if constexpr (DOTS) ev_load<S>(vx, ok, px, F, s, base);
#pragma unroll
        for (int k = 0; k < kEvStep; ++k) {
            a1 += vg[k];
            if constexpr (DOTS) {
                const float xh = (vx[k] - sh) * sc;
                a2 += ok[k] ? vg[k] * xh : 0.f;
            }
        }
    }
    a1 = ev_sum<CL, W>(a1);
    if constexpr (DOTS) a2 = ev_sum<CL, W>(a2);
    if (s.on && s.ge == 0) {
        s1[s.b * F + s.c] = a1;
        if constexpr (DOTS) s2[s.b * F + s.c] = a2;
    }
}

// out[n,c] = (x[n,c] - shift[b,c]) * k1[b,c] + k0[b,c];  WITH_G: out = g[n,c] * ka[b,c] + that.  Rows no event owns: 0.
template <bool WITH_G>
__global__ __launch_bounds__(kAffThreads) void event_affine_kernel(const float *__restrict__ x, const float *__restrict__ g,
                                                                   const int32_t *__restrict__ rowptr, int64_t B, int64_t N,
                                                                   int F, int64_t rows_per_block,
                                                                   const float *__restrict__ shift,
                                                                   const float *__restrict__ k1, const float *__restrict__ k0,
                                                                   const float *__restrict__ ka, float *__restrict__ out)
{
    const int tid = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
    const int64_t r1 = min(r0 + rows_per_block, N);
    const int64_t head = min(max((int64_t)rowptr[0], (int64_t)0), N);
    const int64_t tail = min(max((int64_t)rowptr[B], (int64_t)0), N);
    for (int64_t i = r0 * F + tid; i < min(r1, head) * F; i += kAffThreads) out[i] = 0.f;
    for (int64_t i = max(r0, tail) * F + tid; i < r1 * F; i += kAffThreads) out[i] = 0.f;
    // the last event that starts at or before r0 (uniform over the workgroup); empty events before it are skipped
    int64_t b = 0, top = B;
    while (top - b > 1) {
        const int64_t mid = (b + top) >> 1;
        if ((int64_t)rowptr[mid] <= r0) b = mid; else top = mid;
    }
    const int step = kAffThreads % F;        // how far a lane's channel moves from one of its elements to the next
    for (; b < B; ++b) {
        const int64_t lo = min(max((int64_t)rowptr[b], (int64_t)0), N);
        const int64_t hi = min(max((int64_t)rowptr[b + 1], lo), N);
        if (lo >= r1) break;
        const int64_t a = max(lo, r0), e = min(hi, r1);
        if (a >= e) continue;
        const int64_t cnt = (e - a) * F, base = a * F;      // base is a multiple of F: element i has channel i % F
        const float *cs = shift + b * F, *c1 = k1 + b * F, *c0 = k0 + b * F, *ca = WITH_G ? ka + b * F : nullptr;
        int c = tid % F, held = -1;
        float sh = 0.f, m1 = 0.f, m0 = 0.f, ma = 0.f;
        for (int64_t i = tid; i < cnt; i += kAffUnroll * kAffThreads) {
            float vx[kAffUnroll], vg[kAffUnroll];
#pragma unroll
            for (int u = 0; u < kAffUnroll; ++u) {
                const int64_t ii = i + (int64_t)u * kAffThreads;
                vx[u] = ii < cnt ? x[base + ii] : 0.f;
                if constexpr (WITH_G) vg[u] = ii < cnt ? g[base + ii] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < kAffUnroll; ++u) {
                const int64_t ii = i + (int64_t)u * kAffThreads;
                if (ii < cnt) {
                    if (c != held) {
                        sh = cs[c], m1 = c1[c], m0 = c0[c];
                        if constexpr (WITH_G) ma = ca[c];
                        held = c;
                    }
                    float o = (vx[u] - sh) * m1 + m0;
                    if constexpr (WITH_G) o = vg[u] * ma + o;
                    out[base + ii] = o;
                }
                c += step;
                if (c >= F) c -= F;
            }
        }
    }
}

// ---- host side --------------------------------------------------------------------------------------------------------

int ev_check(const char *who, int64_t B, int64_t N, int F, int max_len)
{
    DMET_REQUIRE(B >= 0 && N >= 0 && F > 0 && max_len >= 0, "%s: bad sizes B=%lld N=%lld F=%d max_len=%d", who,
                 (long long)B, (long long)N, F, max_len);
    // a walk steps an int past an event's length by less than one stride of the team
    DMET_REQUIRE(N < (int64_t)2147483647 - kEvStep * kWave * kEvBlockWaves && B < (int64_t)2147483647,
                 "%s: B=%lld or N=%lld out of range", who, (long long)B, (long long)N);
    // a launch covers B * ceil(F / CL) teams, CL >= min(F, 16)
    DMET_REQUIRE(B * (int64_t)((F + 15) / 16 + 1) < (int64_t)2147483647, "%s: B*F out of range", who);
    return 0;
}

// f(CL, W) as integral constants for a width and a max_len hint (0: unknown, the wavefront form)
template <class Fn>
void ev_dispatch(int F, int max_len, Fn &&f)
{
    using std::integral_constant;
    with_flags([&](auto blk) {
        using W = integral_constant<int, decltype(blk)::value ? kEvBlockWaves : 1>;
        if (F == 1) f(integral_constant<int, 1>{}, W{});
        else if (F <= 4) f(integral_constant<int, 4>{}, W{});
        else f(integral_constant<int, 16>{}, W{});
    }, max_len >= kEvLongRow);
}

template <int CL>
dim3 ev_grid(int64_t B, int F)
{
    return dim3((unsigned)(B * ((F + CL - 1) / CL)));
}

}  // namespace
}  // namespace dmet

using namespace dmet;

extern "C" int dmet_event_moments_f32(const float *x, const int32_t *rowptr, int64_t B, int64_t N, int F, int max_len,
                                      float *mean, float *var, dmet_stream_t stream)
{
    if (int rc = ev_check("dmet_event_moments_f32", B, N, F, max_len)) return rc;
    if (B == 0) return 0;
    DMET_REQUIRE(rowptr && mean && var && (x || N == 0), "dmet_event_moments_f32: null pointer");
    ev_dispatch(F, max_len, [&](auto cl, auto w) {
        constexpr int CL = decltype(cl)::value, W = decltype(w)::value;
        hipLaunchKernelGGL((event_moments_kernel<CL, W>), (ev_grid<CL>(B, F)), dim3(kWave * W), 0, as_stream(stream), x,
                           rowptr, N, F, mean, var);
    });
    DMET_LAUNCH_CHECK("event_moments_kernel");
    return 0;
}

extern "C" int dmet_event_dots_f32(const float *g, const float *x, const int32_t *rowptr, int64_t B, int64_t N, int F,
                                   int max_len, const float *shift, const float *scale, float *s1, float *s2,
                                   dmet_stream_t stream)
{
    if (int rc = ev_check("dmet_event_dots_f32", B, N, F, max_len)) return rc;
    const bool dots = s2 != nullptr;
    DMET_REQUIRE(dots ? (shift && scale) : (!x && !shift && !scale),
                 "dmet_event_dots_f32: x, shift, scale and s2 are given together or not at all");
    if (B == 0) return 0;
    DMET_REQUIRE(rowptr && s1 && ((g && (x || !dots)) || N == 0), "dmet_event_dots_f32: null pointer");
    ev_dispatch(F, max_len, [&](auto cl, auto w) {
        constexpr int CL = decltype(cl)::value, W = decltype(w)::value;
        if (dots)
            hipLaunchKernelGGL((event_dots_kernel<CL, W, true>), (ev_grid<CL>(B, F)), dim3(kWave * W), 0,
                               as_stream(stream), g, x, rowptr, N, F, shift, scale, s1, s2);
        else
            hipLaunchKernelGGL((event_dots_kernel<CL, W, false>), (ev_grid<CL>(B, F)), dim3(kWave * W), 0,
                               as_stream(stream), g, x, rowptr, N, F, shift, scale, s1, s2);
    });
    DMET_LAUNCH_CHECK("event_dots_kernel");
    return 0;
}

extern "C" int dmet_event_affine_f32(const float *x, const float *g, const int32_t *rowptr, int64_t B, int64_t N, int F,
                                     const float *shift, const float *k1, const float *k0, const float *ka, float *out,
                                     dmet_stream_t stream)
{
    if (int rc = ev_check("dmet_event_affine_f32", B, N, F, 0)) return rc;
    DMET_REQUIRE((g != nullptr) == (ka != nullptr), "dmet_event_affine_f32: g and ka are given together or not at all");
    if (B == 0 || N == 0) return 0;
    DMET_REQUIRE(x && rowptr && shift && k1 && k0 && out, "dmet_event_affine_f32: null pointer");
    const int64_t rows_per_block = F >= kAffPerBlock ? 1 : kAffPerBlock / F;
    const int64_t blocks = (N + rows_per_block - 1) / rows_per_block;
    DMET_REQUIRE(blocks < (int64_t)2147483647, "dmet_event_affine_f32: N*F out of range");
    if (g)
        hipLaunchKernelGGL((event_affine_kernel<true>), dim3((unsigned)blocks), dim3(kAffThreads), 0, as_stream(stream), x,
                           g, rowptr, B, N, F, rows_per_block, shift, k1, k0, ka, out);
    else
        hipLaunchKernelGGL((event_affine_kernel<false>), dim3((unsigned)blocks), dim3(kAffThreads), 0, as_stream(stream), x,
                           g, rowptr, B, N, F, rows_per_block, shift, k1, k0, ka, out);
    DMET_LAUNCH_CHECK("event_affine_kernel");
    return 0;
}

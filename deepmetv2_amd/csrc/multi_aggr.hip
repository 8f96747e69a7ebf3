// multi_aggr.hip -- several statistics of the same neighbour rows in one gather (torch_geometric.nn.PNAConv's
// aggregators under DegreeScalerAggregation, torch_scatter.scatter_std's variance): sum, mean, min, max, var, std over a
// fixed-width table or a grouped edge list.
//
// For target i with valid entries j_1..j_n (ascending slot / position order; -1 and ids outside [0, Ns) are skipped, a
// duplicate id counts once per slot), per feature f, fp32:
//   sum  = (((0 + x[j_1]) + x[j_2]) + ...)          mean = sum / (float)n
//   min / max over the candidates that are numbers (+-inf included), with the position (i*k + t, or the edge position)
//          of the winner, the lowest on ties (R4); a NaN never wins and never blocks, in any slot; a feature whose
//          candidates are all NaN gives NaN with position -1
//   var  = (((0 + d_1 d_1) + d_2 d_2) + ...) / (float)n,  d_e = x[j_e] - mean      a second walk over the row, centred on
//          the row's own mean: never a difference of two means
//   std  = s = sqrtf(var < 1e-5f ? 1e-5f : var), 0 where s <= sqrtf(1e-5f)           (PyG's StdAggregation; the clamp
//          keeps a NaN, as torch.clamp does: std is NaN where var is)
// n == 0: zeros everywhere (R3), count 0, positions -1.  out is [Nt, G, A, F/G]: the A requested statistics in request
// order inside each of G feature groups (PNA's towers).
//
// Backward: a per-target launch folds the sum, mean, var and std gradients into two coefficient rows,
//   c1 = (2 g_v) / n      c0 = (g_sum + g_mean / n) - c1 mean      g_v = g_var + g_std / (2 std) where var > 1e-5, std > 0
// and the by-source pass adds, over the positions p that hold source j (ascending), i = the position's row,
//   g_x[j] = sum_p ((c1_i x_j + c0_i) + [argmin_i == p] g_min_i) + [argmax_i == p] g_max_i
// Two launches, not one: formed on the fly every position would gather up to six rows of its target (four gradient
// slices, mean, var) where the folded form gathers two.
//
// Lane layout (the one of interpolate.hip / gravnet.hip): a group of LPT lanes (16, 32 or 64, inside one wavefront) owns
// one row; per chunk of LPT entries lane l forms the scalars of entry l once and the group takes them back by shuffle,
// keeps several row gathers in flight and adds in entry order.  A lane owns the units u = lane, lane + LPT, ... of a row;
// a unit is four floats (one 16-byte access) where F % 4 == 0, (F/G) % 4 == 0 and every row starts on a 16-byte boundary,
// else one float; the arithmetic per element is the same in both: the same bits.  No LDS, no barriers, no float atomics.
#include <math.h>

#include "common.h"

namespace dmet {
namespace {

constexpr int kMaBlock = 256;
constexpr int kMaInFlight = 4;       // row gathers in flight per group, forward
constexpr int kMaBwdInFlight = 2;    // positions in flight per group, backward: each gathers up to six rows
constexpr int kMaMaxF = 256;
constexpr int kMaMaxA = 6;
constexpr float kMaVarFloor = 1e-5f;     // PyG: var.clamp(min=1e-5).sqrt(), masked to 0 where <= sqrt(1e-5)

enum { kMaSum = 1, kMaMean = 2, kMaMin = 3, kMaMax = 4, kMaVar = 5, kMaStd = 6 };

template <typename T, int W>
struct alignas(sizeof(T) * W) Vec {
    T c[W];
};

struct MaArgs {
    const float *x;
    const int32_t *idx, *rowptr, *tgt, *rev_ptr, *rev_pos;
    int64_t Nt, Ns, M;      // M = Nt*k or E: the number of positions
    int k, F, G, A;
    int slot[kMaMaxA + 1];  // slot[kind]: where the statistic stands among the A of a group, -1: not requested
    // forward outputs / backward inputs
    float *out;
    int32_t *count;
    float *mean, *var;
    int32_t *amin, *amax;
    // backward
    const float *g_out;
    float *c0, *c1, *g_x;
};

__device__ __forceinline__ float ma_std(float var)
{
    const float s = sqrtf(var < kMaVarFloor ? kMaVarFloor : var);      // a comparison, not fmaxf: NaN stays NaN
    return s <= sqrtf(kMaVarFloor) ? 0.f : s;
}

// where unit p of a row (features p*W ..) starts inside a row of out / g_out [G, A, F/G], statistic slot 0
template <int W>
__device__ __forceinline__ int out_offset(int p, int Fg, int A)
{
    const int f0 = p * W;
    return (f0 / Fg) * A * Fg + f0 % Fg;
}

template <int LPT, int ITER, int W>
__global__ __launch_bounds__(kMaBlock) void multi_aggr_fwd_kernel(MaArgs a)
{
    using VF = Vec<float, W>;
    using VI = Vec<int32_t, W>;
    constexpr int TPB = kMaBlock / LPT;
    const int bid = xcd_swizzle(blockIdx.x, gridDim.x);
    const int64_t i = (int64_t)bid * TPB + threadIdx.x / LPT;
    const int lane = threadIdx.x % LPT;
    if (i >= a.Nt) return;        // whole groups leave: the shuffles below stay inside a group
    const int U = a.F / W;
    const VF *x = reinterpret_cast<const VF *>(a.x);

    int64_t lo;
    int len;
    if (a.rowptr == nullptr) {
        lo = i * a.k;
        len = a.k;
    } else {
        lo = min(max((int64_t)a.rowptr[i], (int64_t)0), a.M);
        len = (int)(min(max((int64_t)a.rowptr[i + 1], lo), a.M) - lo);
    }
    // the id of entry t of the row; -1 for an empty slot, an id outside [0, Ns) and anything past the row
    auto entry = [&](int t) -> int32_t {
        if (t >= len) return -1;
        const int32_t j = a.idx[lo + t];
        return (j >= 0 && (int64_t)j < a.Ns) ? j : -1;
    };
    const bool minmax = a.slot[kMaMin] >= 0 || a.slot[kMaMax] >= 0;
    const bool second = a.slot[kMaVar] >= 0 || a.slot[kMaStd] >= 0;

    float sum[ITER][W], mn[ITER][W], mx[ITER][W];
    int32_t pmn[ITER][W], pmx[ITER][W];
#pragma unroll
    for (int it = 0; it < ITER; ++it)
#pragma unroll
        for (int c = 0; c < W; ++c) {
            sum[it][c] = 0.f;
            mn[it][c] = mx[it][c] = NAN;        // NaN: no number among the candidates yet (min and max alike)
            pmn[it][c] = pmx[it][c] = -1;
        }
    int n = 0;
    int32_t jl = -1;
    for (int base = 0; base < len; base += LPT) {
        jl = entry(base + lane);        // lane l: the id of entry base + l
        const int m = min(LPT, len - base);
        for (int e0 = 0; e0 < m; e0 += kMaInFlight) {
            int32_t j[kMaInFlight];
            VF v[kMaInFlight][ITER];
#pragma unroll
            for (int u = 0; u < kMaInFlight; ++u) {
                j[u] = __shfl(jl, (e0 + u) & (LPT - 1), LPT);
                if (e0 + u >= m) j[u] = -1;
            }
#pragma unroll
            for (int u = 0; u < kMaInFlight; ++u)
#pragma unroll
                for (int it = 0; it < ITER; ++it) {
                    const int p = lane + it * LPT;
                    if (j[u] >= 0 && p < U) v[u][it] = x[(int64_t)j[u] * U + p];
                }
#pragma unroll
            for (int u = 0; u < kMaInFlight; ++u) {
                if (j[u] < 0) continue;        // the same for every lane of the group
                const int32_t pos = (int32_t)(lo + base + e0 + u);
#pragma unroll
                for (int it = 0; it < ITER; ++it) {
                    if (lane + it * LPT >= U) continue;
#pragma unroll
                    for (int c = 0; c < W; ++c) {
                        const float val = v[u][it].c[c];
                        sum[it][c] += val;
                        if (minmax) {
                            // strict: the lowest position keeps a tie (R4).  While the running value is NaN any
                            // candidate replaces it, so the first number is taken whatever it is (+-inf too); once it
                            // is a number a NaN fails the comparison: it never wins and never blocks, in any slot
                            const bool none = mn[it][c] != mn[it][c];      // mx is NaN exactly when mn is
                            if (val < mn[it][c] || none) {
                                mn[it][c] = val;
                                pmn[it][c] = pos;
                            }
                            if (val > mx[it][c] || none) {
                                mx[it][c] = val;
                                pmx[it][c] = pos;
                            }
                        }
                    }
                }
                ++n;
            }
        }
    }

    const float fn = (float)n;
    float mean[ITER][W], var[ITER][W];
#pragma unroll
    for (int it = 0; it < ITER; ++it)
#pragma unroll
        for (int c = 0; c < W; ++c) {
            mean[it][c] = n > 0 ? sum[it][c] / fn : 0.f;
            var[it][c] = 0.f;
        }
    if (second && n > 0) {
        // the second walk: the row's entries again (they are in L2), centred on the row's mean
        for (int base = 0; base < len; base += LPT) {
            if (len > LPT) jl = entry(base + lane);       // one chunk: the ids are still in registers
            const int m = min(LPT, len - base);
            for (int e0 = 0; e0 < m; e0 += kMaInFlight) {
                int32_t j[kMaInFlight];
                VF v[kMaInFlight][ITER];
#pragma unroll
                for (int u = 0; u < kMaInFlight; ++u) {
                    j[u] = __shfl(jl, (e0 + u) & (LPT - 1), LPT);
                    if (e0 + u >= m) j[u] = -1;
                }
#pragma unroll
                for (int u = 0; u < kMaInFlight; ++u)
#pragma unroll
                    for (int it = 0; it < ITER; ++it) {
                        const int p = lane + it * LPT;
                        if (j[u] >= 0 && p < U) v[u][it] = x[(int64_t)j[u] * U + p];
                    }
#pragma unroll
                for (int u = 0; u < kMaInFlight; ++u) {
                    if (j[u] < 0) continue;
#pragma unroll
                    for (int it = 0; it < ITER; ++it) {
                        if (lane + it * LPT >= U) continue;
#pragma unroll
                        for (int c = 0; c < W; ++c) {
                            const float d = v[u][it].c[c] - mean[it][c];
                            var[it][c] += d * d;
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int it = 0; it < ITER; ++it)
#pragma unroll
            for (int c = 0; c < W; ++c) var[it][c] = var[it][c] / fn;
    }

    const int Fg = a.F / a.G;
    float *orow = a.out + i * (int64_t)a.A * a.F;
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
        const int p = lane + it * LPT;
        if (p >= U) continue;
        VF s_sum, s_mean, s_min, s_max, s_var, s_std;
        VI s_pmn, s_pmx;
#pragma unroll
        for (int c = 0; c < W; ++c) {       // a row without a valid entry: zeros (R3), positions -1
            s_sum.c[c] = sum[it][c];
            s_mean.c[c] = mean[it][c];
            s_min.c[c] = n > 0 ? mn[it][c] : 0.f;       // still NaN: no number among the candidates
            s_max.c[c] = n > 0 ? mx[it][c] : 0.f;
            s_var.c[c] = var[it][c];
            s_std.c[c] = n > 0 ? ma_std(var[it][c]) : 0.f;
            s_pmn.c[c] = mn[it][c] != mn[it][c] ? -1 : pmn[it][c];       // a NaN that stood in for "none" is no winner
            s_pmx.c[c] = mx[it][c] != mx[it][c] ? -1 : pmx[it][c];
        }
        float *o = orow + out_offset<W>(p, Fg, a.A);
        auto put = [&](int kind, const VF &val) {
            if (a.slot[kind] >= 0) *reinterpret_cast<VF *>(o + a.slot[kind] * Fg) = val;
        };
        put(kMaSum, s_sum);
        put(kMaMean, s_mean);
        put(kMaMin, s_min);
        put(kMaMax, s_max);
        put(kMaVar, s_var);
        put(kMaStd, s_std);
        const int64_t at = i * U + p;
        if (a.mean != nullptr) reinterpret_cast<VF *>(a.mean)[at] = s_mean;
        if (a.var != nullptr) reinterpret_cast<VF *>(a.var)[at] = s_var;
        if (a.amin != nullptr) reinterpret_cast<VI *>(a.amin)[at] = s_pmn;
        if (a.amax != nullptr) reinterpret_cast<VI *>(a.amax)[at] = s_pmx;
    }
    if (lane == 0) a.count[i] = n;
}

// The coefficient rows of the backward, one thread per (target, feature): plain elementwise work, no row to share.
__global__ __launch_bounds__(kMaBlock) void multi_aggr_coef_kernel(MaArgs a)
{
    const int64_t e = (int64_t)blockIdx.x * kMaBlock + threadIdx.x;
    if (e >= a.Nt * a.F) return;
    const int64_t i = e / a.F;
    const int f = (int)(e - i * a.F);
    const int Fg = a.F / a.G;
    const float *g = a.g_out + i * (int64_t)a.A * a.F + out_offset<1>(f, Fg, a.A);
    const bool second = a.slot[kMaVar] >= 0 || a.slot[kMaStd] >= 0;
    const int n = a.count[i];
    float c0 = 0.f, c1 = 0.f;
    if (n > 0) {
        const float fn = (float)n;
        const float gs = a.slot[kMaSum] >= 0 ? g[a.slot[kMaSum] * Fg] : 0.f;
        const float gm = a.slot[kMaMean] >= 0 ? g[a.slot[kMaMean] * Fg] : 0.f;
        c0 = gs + gm / fn;
        if (second) {
            float gv = a.slot[kMaVar] >= 0 ? g[a.slot[kMaVar] * Fg] : 0.f;
            if (a.slot[kMaStd] >= 0) {
                const float v = a.var[e];
                const float s = ma_std(v);
                if (v > kMaVarFloor && s > 0.f) gv += g[a.slot[kMaStd] * Fg] / (2.f * s);
            }
            c1 = (2.f * gv) / fn;
            c0 = c0 - c1 * a.mean[e];
        }
    }
    a.c0[e] = c0;
    if (second) a.c1[e] = c1;
}

// Backward, by source: for source j over the positions that hold j (rev_pos, ascending; the span clamped to [0, M]).  A
// position outside [0, M) and a row outside [0, Nt) are no entries.  A hub's list is walked by its one group.
template <int LPT, int ITER, int W>
__global__ __launch_bounds__(kMaBlock) void multi_aggr_bwd_kernel(MaArgs a)
{
    using VF = Vec<float, W>;
    using VI = Vec<int32_t, W>;
    constexpr int TPB = kMaBlock / LPT;
    const int bid = xcd_swizzle(blockIdx.x, gridDim.x);
    const int64_t j = (int64_t)bid * TPB + threadIdx.x / LPT;
    const int lane = threadIdx.x % LPT;
    if (j >= a.Ns) return;
    const int U = a.F / W, Fg = a.F / a.G;
    const int64_t lo = min(max((int64_t)a.rev_ptr[j], (int64_t)0), a.M);
    const int64_t hi = min(max((int64_t)a.rev_ptr[j + 1], lo), a.M);
    const bool second = a.slot[kMaVar] >= 0 || a.slot[kMaStd] >= 0;
    const bool hasmin = a.slot[kMaMin] >= 0, hasmax = a.slot[kMaMax] >= 0;
    const VF *C0 = reinterpret_cast<const VF *>(a.c0), *C1 = reinterpret_cast<const VF *>(a.c1);
    const VI *AMIN = reinterpret_cast<const VI *>(a.amin), *AMAX = reinterpret_cast<const VI *>(a.amax);
    const int64_t gstride = (int64_t)a.A * a.F;       // floats per target row of g_out

    float acc[ITER][W];
    VF xj[ITER];
    int omin[ITER], omax[ITER];
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
        const int p = lane + it * LPT;
#pragma unroll
        for (int c = 0; c < W; ++c) acc[it][c] = xj[it].c[c] = 0.f;
        omin[it] = omax[it] = 0;
        if (p >= U) continue;
        if (second) xj[it] = reinterpret_cast<const VF *>(a.x)[j * U + p];
        const int off = out_offset<W>(p, Fg, a.A);
        omin[it] = off + (hasmin ? a.slot[kMaMin] * Fg : 0);
        omax[it] = off + (hasmax ? a.slot[kMaMax] * Fg : 0);
    }
    for (int64_t base = lo; base < hi; base += LPT) {
        // lane l: target and position of entry base + l
        int32_t il = -1, pl = -1;
        if (base + lane < hi) {
            const int64_t pos = a.rev_pos[base + lane];
            if (pos >= 0 && pos < a.M) {
                const int64_t i = a.tgt == nullptr ? pos / a.k : (int64_t)a.tgt[pos];
                if (i >= 0 && i < a.Nt) {
                    il = (int32_t)i;
                    pl = (int32_t)pos;
                }
            }
        }
        const int m = (int)min((int64_t)LPT, hi - base);
        for (int e0 = 0; e0 < m; e0 += kMaBwdInFlight) {
            int32_t i[kMaBwdInFlight], pos[kMaBwdInFlight];
            VF c0[kMaBwdInFlight][ITER], c1[kMaBwdInFlight][ITER], gmn[kMaBwdInFlight][ITER], gmx[kMaBwdInFlight][ITER];
            VI amn[kMaBwdInFlight][ITER], amx[kMaBwdInFlight][ITER];
#pragma unroll
            for (int u = 0; u < kMaBwdInFlight; ++u) {
                i[u] = __shfl(il, (e0 + u) & (LPT - 1), LPT);
                pos[u] = __shfl(pl, (e0 + u) & (LPT - 1), LPT);
                if (e0 + u >= m) i[u] = -1;
            }
#pragma unroll
            for (int u = 0; u < kMaBwdInFlight; ++u)
#pragma unroll
                for (int it = 0; it < ITER; ++it) {
                    const int p = lane + it * LPT;
                    if (i[u] < 0 || p >= U) continue;
                    const int64_t at = (int64_t)i[u] * U + p;
                    c0[u][it] = C0[at];
                    if (second) c1[u][it] = C1[at];
                    if (hasmin) {
                        amn[u][it] = AMIN[at];
                        gmn[u][it] = *reinterpret_cast<const VF *>(a.g_out + i[u] * gstride + omin[it]);
                    }
                    if (hasmax) {
                        amx[u][it] = AMAX[at];
                        gmx[u][it] = *reinterpret_cast<const VF *>(a.g_out + i[u] * gstride + omax[it]);
                    }
                }
#pragma unroll
            for (int u = 0; u < kMaBwdInFlight; ++u) {
                if (i[u] < 0) continue;        // the same for every lane of the group
#pragma unroll
                for (int it = 0; it < ITER; ++it) {
                    if (lane + it * LPT >= U) continue;
#pragma unroll
                    for (int c = 0; c < W; ++c) {
                        float t = c0[u][it].c[c];
                        if (second) t = c1[u][it].c[c] * xj[it].c[c] + t;
                        if (hasmin && amn[u][it].c[c] == pos[u]) t += gmn[u][it].c[c];
                        if (hasmax && amx[u][it].c[c] == pos[u]) t += gmx[u][it].c[c];
                        acc[it][c] += t;
                    }
                }
            }
        }
    }
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
        const int p = lane + it * LPT;
        if (p >= U) continue;
        VF o;
#pragma unroll
        for (int c = 0; c < W; ++c) o.c[c] = acc[it][c];
        reinterpret_cast<VF *>(a.g_x)[j * U + p] = o;        // a source nobody lists: zeros
    }
}

template <bool FWD, int LPT, int ITER, int W>
int launch(const MaArgs &a, hipStream_t st)
{
    constexpr int TPB = kMaBlock / LPT;
    const int64_t rows = FWD ? a.Nt : a.Ns;
    const int64_t blocks = (rows + TPB - 1) / TPB;
    if constexpr (FWD) {
        hipLaunchKernelGGL((multi_aggr_fwd_kernel<LPT, ITER, W>), dim3((unsigned)blocks), dim3(kMaBlock), 0, st, a);
        DMET_LAUNCH_CHECK("multi_aggr_fwd_kernel");
    } else {
        hipLaunchKernelGGL((multi_aggr_bwd_kernel<LPT, ITER, W>), dim3((unsigned)blocks), dim3(kMaBlock), 0, st, a);
        DMET_LAUNCH_CHECK("multi_aggr_bwd_kernel");
    }
    return 0;
}

// lanes per row and units per lane for a width F, as interpolate.hip: 16-byte units (vec), one per lane, 16 lanes up to
// F = 64, 32 up to 128, 64 up to 256; float units: 16 lanes up to F = 32 (two per lane), 32 up to 128 and 64 up to 256
// (four per lane).
template <bool FWD>
int dispatch(const MaArgs &a, bool vec, hipStream_t st)
{
    if (vec) {
        if (a.F <= 64) return launch<FWD, 16, 1, 4>(a, st);
        if (a.F <= 128) return launch<FWD, 32, 1, 4>(a, st);
        return launch<FWD, 64, 1, 4>(a, st);
    }
    if (a.F <= 32) return launch<FWD, 16, 2, 1>(a, st);
    if (a.F <= 128) return launch<FWD, 32, 4, 1>(a, st);
    return launch<FWD, 64, 4, 1>(a, st);
}

// aggrs: the requested statistics, four bits each from the lowest (1 sum, 2 mean, 3 min, 4 max, 5 var, 6 std), ended
// by the first zero nibble; each at most once
int check_args(const char *who, MaArgs &a, int64_t Nt, int64_t Ns, int64_t E, int width, int F, int G, int aggrs)
{
    DMET_REQUIRE(Nt >= 0 && Ns >= 0 && Nt < (int64_t)2147483647 && Ns < (int64_t)2147483647,
                 "%s: Nt=%lld, Ns=%lld out of range", who, (long long)Nt, (long long)Ns);
    DMET_REQUIRE(F >= 1 && F <= kMaMaxF, "%s: F=%d not in [1,%d]", who, F, kMaMaxF);
    DMET_REQUIRE(G >= 1 && F % G == 0, "%s: groups=%d must divide F=%d", who, G, F);
    DMET_REQUIRE(width >= 0 && width <= DMET_MAX_K, "%s: width=%d not in [1,%d] (0: an edge list)", who, width, DMET_MAX_K);
    if (width == 0)
        DMET_REQUIRE(E >= 0 && E < (int64_t)2147483647, "%s: E=%lld out of range", who, (long long)E);
    else
        DMET_REQUIRE(Nt * (int64_t)width < (int64_t)2147483647, "%s: Nt*width out of range", who);
    for (int kind = 0; kind <= kMaMaxA; ++kind) a.slot[kind] = -1;
    int A = 0;
    DMET_REQUIRE(aggrs > 0 && (aggrs >> (4 * kMaMaxA)) == 0, "%s: aggrs=0x%x names no or more than %d statistics", who,
                 (unsigned)aggrs, kMaMaxA);
    for (int rest = aggrs; rest != 0; rest >>= 4, ++A) {
        const int kind = rest & 15;
        DMET_REQUIRE(kind >= kMaSum && kind <= kMaStd, "%s: aggrs=0x%x: statistic %d of slot %d, supported 1..6", who,
                     (unsigned)aggrs, kind, A);
        DMET_REQUIRE(a.slot[kind] < 0, "%s: aggrs=0x%x names statistic %d twice", who, (unsigned)aggrs, kind);
        a.slot[kind] = A;
    }
    a.Nt = Nt; a.Ns = Ns; a.k = width; a.F = F; a.G = G; a.A = A;
    a.M = width == 0 ? E : Nt * (int64_t)width;
    return 0;
}

}  // namespace
}  // namespace dmet

using namespace dmet;

extern "C" int dmet_multi_aggr_fwd_f32(const float *x, const int32_t *idx, const int32_t *rowptr, int64_t Nt, int64_t Ns,
                                       int64_t E, int width, int F, int G, int aggrs, float *out, int32_t *count,
                                       float *mean, float *var, int32_t *argmin, int32_t *argmax, dmet_stream_t stream)
{
    const char *who = "dmet_multi_aggr_fwd_f32";
    MaArgs a{};
    if (int rc = check_args(who, a, Nt, Ns, E, width, F, G, aggrs)) return rc;
    if (Nt == 0) return 0;
    const bool list = width == 0;
    DMET_REQUIRE(out && count, "%s: null pointer", who);
    DMET_REQUIRE(!list || rowptr, "%s: an edge list (width 0) needs rowptr", who);
    DMET_REQUIRE(idx || (list && E == 0), "%s: null nbr / src", who);
    DMET_REQUIRE(Ns == 0 || x, "%s: null x with Ns=%lld", who, (long long)Ns);
    DMET_REQUIRE((a.slot[kMaVar] < 0 && a.slot[kMaStd] < 0) || (mean && var), "%s: var / std need the mean and var rows", who);
    DMET_REQUIRE(a.slot[kMaMin] < 0 || argmin, "%s: min needs argmin", who);
    DMET_REQUIRE(a.slot[kMaMax] < 0 || argmax, "%s: max needs argmax", who);
    a.x = x; a.idx = idx; a.rowptr = list ? rowptr : nullptr;
    a.out = out; a.count = count; a.mean = mean; a.var = var; a.amin = argmin; a.amax = argmax;
    const bool vec = F % 4 == 0 && (F / G) % 4 == 0 && aligned16(x) && aligned16(out) && aligned16(mean) && aligned16(var) &&
                     aligned16(argmin) && aligned16(argmax);
    return dispatch<true>(a, vec, as_stream(stream));
}

extern "C" int dmet_multi_aggr_bwd_f32(const float *x, const float *g_out, const int32_t *count, const float *mean,
                                       const float *var, const int32_t *argmin, const int32_t *argmax, const int32_t *tgt,
                                       const int32_t *rev_ptr, const int32_t *rev_pos, int64_t Nt, int64_t Ns, int64_t E,
                                       int width, int F, int G, int aggrs, float *c0, float *c1, float *g_x,
                                       dmet_stream_t stream)
{
    const char *who = "dmet_multi_aggr_bwd_f32";
    MaArgs a{};
    if (int rc = check_args(who, a, Nt, Ns, E, width, F, G, aggrs)) return rc;
    if (Ns == 0) return 0;      // no source: nothing to write
    DMET_REQUIRE(g_x, "%s: null g_x", who);
    hipStream_t st = as_stream(stream);
    if (Nt == 0) {      // no target: nothing reaches a source
        hipError_t e = hipMemsetAsync(g_x, 0, (size_t)Ns * F * sizeof(float), st);
        if (e != hipSuccess) return hip_fail(e, "dmet_multi_aggr_bwd_f32: memset");
        return 0;
    }
    const bool list = width == 0;
    const bool second = a.slot[kMaVar] >= 0 || a.slot[kMaStd] >= 0;
    DMET_REQUIRE(g_out && count && c0 && rev_ptr, "%s: null pointer", who);
    DMET_REQUIRE(a.M == 0 || (rev_pos && (!list || tgt)), "%s: null rev_pos / tgt", who);
    DMET_REQUIRE(!second || (x && mean && var && c1), "%s: var / std need x, mean, var and c1", who);
    DMET_REQUIRE(a.slot[kMaMin] < 0 || argmin, "%s: min needs argmin", who);
    DMET_REQUIRE(a.slot[kMaMax] < 0 || argmax, "%s: max needs argmax", who);
    a.x = x; a.g_out = g_out; a.count = const_cast<int32_t *>(count); a.mean = const_cast<float *>(mean);
    a.var = const_cast<float *>(var); a.amin = const_cast<int32_t *>(argmin); a.amax = const_cast<int32_t *>(argmax);
    a.tgt = list ? tgt : nullptr; a.rev_ptr = rev_ptr; a.rev_pos = rev_pos; a.c0 = c0; a.c1 = c1; a.g_x = g_x;
    const int64_t blocks = (Nt * (int64_t)F + kMaBlock - 1) / kMaBlock;
    hipLaunchKernelGGL(multi_aggr_coef_kernel, dim3((unsigned)blocks), dim3(kMaBlock), 0, st, a);
    DMET_LAUNCH_CHECK("multi_aggr_coef_kernel");
    const bool vec = F % 4 == 0 && (F / G) % 4 == 0 && aligned16(x) && aligned16(g_out) && aligned16(argmin) &&
                     aligned16(argmax) && aligned16(c0) && aligned16(c1) && aligned16(g_x);
    return dispatch<false>(a, vec, st);
}

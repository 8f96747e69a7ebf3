// weighted_sum.hip -- out_i = sum_e w_e x[src(e)] over a fixed-width table or a grouped edge list, with a free per-edge
// weight that takes a gradient of its own: torch_geometric's propagate(..., edge_weight=) under aggr='add' (GCNConv,
// GraphConv, SAGEConv, GINConv) and torch_sparse.spmm.
//
// Forward, for target i with valid entries e_1..e_n (ascending position order; -1 and ids outside [0, Ns) are skipped, and
// the weight of a skipped position is never read into a result), per feature f, fp32:
//   out[i,f] = fmaf(w_e, x[j_e,f], acc)  from acc = 0;  w == NULL: acc + x[j_e,f], the bits of w all ones
//   count[i] = n;  n == 0: zeros exactly (R3)
// Backward by source (g_x): for source j over the positions p that hold j (rev_pos, ascending), i = the position's row,
//   g_x[j,f] = fmaf(w_p, g_out[i,f], acc);  a source nobody lists: zeros.  A hub's list is walked by its one group.
// Backward by target (g_w): for every position p of row i with j = src(p),
//   g_w[p] = sum_f g_out[i,f] x[j,f]:  a lane owns four consecutive features per unit and adds its products in ascending
//   order from 0, then an xor butterfly runs over the group's lanes (the channel sum of gat.hip / row_softmax.h).  The
//   row g_out[i,:] is read once per group and kept in registers.  Every position is written, an empty slot gets 0.
//
// Lane layout (the one of multi_aggr.hip / interpolate.hip): a group of LPT lanes (16, 32 or 64, inside one wavefront) owns
// one row; per chunk of LPT entries lane l reads the id and the weight of entry l once and the group takes them back by
// shuffle, keeps several row gathers in flight and adds in entry order.  A lane owns the units u = lane, lane + LPT, ...
// of a row; a unit is four floats (one 16-byte access) where F % 4 == 0 and every row tensor starts on a 16-byte
// boundary, else one float; the arithmetic per element is the same in both: the same bits.  The g_w kernel sums over
// features, so there the element form keeps the 16-byte form's ownership (lane l: features 4l .. 4l+3) and only loads
// them one by one: the same partial sums, the same bits.  No LDS, no barriers, no float atomics.
#include <math.h>

#include "common.h"

namespace dmet {
namespace {

constexpr int kWsBlock = 256;
constexpr int kWsInFlight = 4;       // row gathers in flight per group
constexpr int kWsMaxF = 256;

template <typename T, int W>
struct alignas(sizeof(T) * W) Vec {
    T c[W];
};

struct WsArgs {
    const float *x, *w, *g_out;
    const int32_t *idx, *rowptr, *tgt, *rev_ptr, *rev_pos;
    int64_t Nt, Ns, M;      // M = Nt*k or E: the number of positions
    int k, F;
    float *out;
    int32_t *count;
    float *g_x, *g_w;
};

// the span [lo, lo + len) of row i's positions
__device__ __forceinline__ void row_span(const WsArgs &a, int64_t i, int64_t &lo, int &len)
{
    if (a.rowptr == nullptr) {
        lo = i * a.k;
        len = a.k;
    } else {
        lo = min(max((int64_t)a.rowptr[i], (int64_t)0), a.M);
        len = (int)(min(max((int64_t)a.rowptr[i + 1], lo), a.M) - lo);
    }
}

template <int LPT, int ITER, int W>
__global__ __launch_bounds__(kWsBlock) void weighted_sum_fwd_kernel(WsArgs a)
{
    using VF = Vec<float, W>;
    constexpr int TPB = kWsBlock / LPT;
    const int bid = xcd_swizzle(blockIdx.x, gridDim.x);
    const int64_t i = (int64_t)bid * TPB + threadIdx.x / LPT;
    const int lane = threadIdx.x % LPT;
    if (i >= a.Nt) return;        // whole groups leave: the shuffles below stay inside a group
    const int U = a.F / W;
    const VF *x = reinterpret_cast<const VF *>(a.x);
    int64_t lo;
    int len;
    row_span(a, i, lo, len);

    float acc[ITER][W];
#pragma unroll
    for (int it = 0; it < ITER; ++it)
#pragma unroll
        for (int c = 0; c < W; ++c) acc[it][c] = 0.f;
    int n = 0;
    for (int base = 0; base < len; base += LPT) {
        // lane l: the id and the weight of entry base + l; -1 for an empty slot, an id outside [0, Ns) and past the row
        int32_t jl = -1;
        float wl = 0.f;
        if (base + lane < len) {
            const int32_t j = a.idx[lo + base + lane];
            if (j >= 0 && (int64_t)j < a.Ns) {
                jl = j;
                wl = a.w != nullptr ? a.w[lo + base + lane] : 1.f;
            }
        }
        const int m = min(LPT, len - base);
        for (int e0 = 0; e0 < m; e0 += kWsInFlight) {
            int32_t j[kWsInFlight];
            float wv[kWsInFlight];
            VF v[kWsInFlight][ITER];
#pragma unroll
            for (int u = 0; u < kWsInFlight; ++u) {
                j[u] = __shfl(jl, (e0 + u) & (LPT - 1), LPT);
                wv[u] = __shfl(wl, (e0 + u) & (LPT - 1), LPT);
                if (e0 + u >= m) j[u] = -1;
            }
#pragma unroll
            for (int u = 0; u < kWsInFlight; ++u)
#pragma unroll
                for (int it = 0; it < ITER; ++it) {
                    const int p = lane + it * LPT;
                    if (j[u] >= 0 && p < U) v[u][it] = x[(int64_t)j[u] * U + p];
                }
#pragma unroll
            for (int u = 0; u < kWsInFlight; ++u) {
                if (j[u] < 0) continue;        // the same for every lane of the group
#pragma unroll
                for (int it = 0; it < ITER; ++it) {
                    if (lane + it * LPT >= U) continue;
#pragma unroll
                    for (int c = 0; c < W; ++c) acc[it][c] = fmaf(wv[u], v[u][it].c[c], acc[it][c]);
                }
                ++n;
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
        reinterpret_cast<VF *>(a.out)[i * U + p] = o;        // a row without a valid entry: zeros (R3)
    }
    if (lane == 0 && a.count != nullptr) a.count[i] = n;
}

// Backward, by source: for source j over the positions that hold j (rev_pos, ascending; the span clamped to [0, M]).  A
// position outside [0, M) and a row outside [0, Nt) are no entries.  A hub's list is walked by its one group.
template <int LPT, int ITER, int W>
__global__ __launch_bounds__(kWsBlock) void weighted_sum_bwd_x_kernel(WsArgs a)
{
    using VF = Vec<float, W>;
    constexpr int TPB = kWsBlock / LPT;
    const int bid = xcd_swizzle(blockIdx.x, gridDim.x);
    const int64_t j = (int64_t)bid * TPB + threadIdx.x / LPT;
    const int lane = threadIdx.x % LPT;
    if (j >= a.Ns) return;
    const int U = a.F / W;
    const VF *G = reinterpret_cast<const VF *>(a.g_out);
    const int64_t lo = min(max((int64_t)a.rev_ptr[j], (int64_t)0), a.M);
    const int64_t hi = min(max((int64_t)a.rev_ptr[j + 1], lo), a.M);

    float acc[ITER][W];
#pragma unroll
    for (int it = 0; it < ITER; ++it)
#pragma unroll
        for (int c = 0; c < W; ++c) acc[it][c] = 0.f;
    for (int64_t base = lo; base < hi; base += LPT) {
        // lane l: the target and the weight of entry base + l
        int32_t il = -1;
        float wl = 0.f;
        if (base + lane < hi) {
            const int64_t pos = a.rev_pos[base + lane];
            if (pos >= 0 && pos < a.M) {
                const int64_t i = a.tgt == nullptr ? pos / a.k : (int64_t)a.tgt[pos];
                if (i >= 0 && i < a.Nt) {
                    il = (int32_t)i;
                    wl = a.w != nullptr ? a.w[pos] : 1.f;
                }
            }
        }
        const int m = (int)min((int64_t)LPT, hi - base);
        for (int e0 = 0; e0 < m; e0 += kWsInFlight) {
            int32_t i[kWsInFlight];
            float wv[kWsInFlight];
            VF v[kWsInFlight][ITER];
#pragma unroll
            for (int u = 0; u < kWsInFlight; ++u) {
                i[u] = __shfl(il, (e0 + u) & (LPT - 1), LPT);
                wv[u] = __shfl(wl, (e0 + u) & (LPT - 1), LPT);
                if (e0 + u >= m) i[u] = -1;
            }
#pragma unroll
            for (int u = 0; u < kWsInFlight; ++u)
#pragma unroll
                for (int it = 0; it < ITER; ++it) {
                    const int p = lane + it * LPT;
                    if (i[u] >= 0 && p < U) v[u][it] = G[(int64_t)i[u] * U + p];
                }
#pragma unroll
            for (int u = 0; u < kWsInFlight; ++u) {
                if (i[u] < 0) continue;        // the same for every lane of the group
#pragma unroll
                for (int it = 0; it < ITER; ++it) {
                    if (lane + it * LPT >= U) continue;
#pragma unroll
                    for (int c = 0; c < W; ++c) acc[it][c] = fmaf(wv[u], v[u][it].c[c], acc[it][c]);
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

// the four features 4p .. 4p+3 of a row (those below F); VEC: one 16-byte access
template <bool VEC>
__device__ __forceinline__ Vec<float, 4> load4(const float *row, int p, int F)
{
    if constexpr (VEC) {
        return reinterpret_cast<const Vec<float, 4> *>(row)[p];
    } else {
        Vec<float, 4> v;
#pragma unroll
        for (int c = 0; c < 4; ++c) v.c[c] = 4 * p + c < F ? row[4 * p + c] : 0.f;
        return v;
    }
}

// Backward, by target: g_w[p] = <g_out[i,:], x[src(p),:]> for every position p of row i.  Lane l owns the features
// 4l .. 4l+3 in both forms (LPT * 4 >= F), so the partial sums and the butterfly see the same values in the same order.
template <int LPT, bool VEC>
__global__ __launch_bounds__(kWsBlock) void weighted_sum_bwd_w_kernel(WsArgs a)
{
    using VF = Vec<float, 4>;
    constexpr int TPB = kWsBlock / LPT;
    const int bid = xcd_swizzle(blockIdx.x, gridDim.x);
    const int64_t i = (int64_t)bid * TPB + threadIdx.x / LPT;
    const int lane = threadIdx.x % LPT;
    if (i >= a.Nt) return;
    const int F = a.F;
    const int nf = min(max(F - 4 * lane, 0), 4);        // how many of the lane's four features exist
    int64_t lo;
    int len;
    row_span(a, i, lo, len);
    if (a.rowptr != nullptr) {
        // positions no row lists (a rowptr that does not start at 0 or end at E): written too, by the outer rows' groups
        if (i == 0)
            for (int64_t p = lane; p < lo; p += LPT) a.g_w[p] = 0.f;
        if (i == a.Nt - 1)
            for (int64_t p = lo + len + lane; p < a.M; p += LPT) a.g_w[p] = 0.f;
    }
    VF g;
#pragma unroll
    for (int c = 0; c < 4; ++c) g.c[c] = 0.f;
    if (nf > 0) g = load4<VEC>(a.g_out + i * (int64_t)F, lane, F);

    for (int base = 0; base < len; base += LPT) {
        int32_t jl = -1;
        if (base + lane < len) {
            const int32_t j = a.idx[lo + base + lane];
            if (j >= 0 && (int64_t)j < a.Ns) jl = j;
        }
        const int m = min(LPT, len - base);
        float res = 0.f;        // lane l: the result of entry base + l; an empty slot keeps 0
        for (int e0 = 0; e0 < m; e0 += kWsInFlight) {
            int32_t j[kWsInFlight];
            VF v[kWsInFlight];
#pragma unroll
            for (int u = 0; u < kWsInFlight; ++u) {
                j[u] = __shfl(jl, (e0 + u) & (LPT - 1), LPT);
                if (e0 + u >= m) j[u] = -1;
            }
#pragma unroll
            for (int u = 0; u < kWsInFlight; ++u)
                if (j[u] >= 0 && nf > 0) v[u] = load4<VEC>(a.x + (int64_t)j[u] * F, lane, F);
#pragma unroll
            for (int u = 0; u < kWsInFlight; ++u) {
                float s = 0.f;
                if (j[u] >= 0) {
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        if (c < nf) s = s + g.c[c] * v[u].c[c];
                }
#pragma unroll
                for (int off = LPT / 2; off >= 1; off >>= 1) s += __shfl_xor(s, off, LPT);
                if (lane == e0 + u && j[u] >= 0) res = s;
            }
        }
        if (lane < m) a.g_w[lo + base + lane] = res;
    }
}

template <int KIND, int LPT, int ITER, int W>
int launch(const WsArgs &a, hipStream_t st)
{
    constexpr int TPB = kWsBlock / LPT;
    const int64_t rows = KIND == 1 ? a.Ns : a.Nt;
    const int64_t blocks = (rows + TPB - 1) / TPB;
    if constexpr (KIND == 0) {
        hipLaunchKernelGGL((weighted_sum_fwd_kernel<LPT, ITER, W>), dim3((unsigned)blocks), dim3(kWsBlock), 0, st, a);
        DMET_LAUNCH_CHECK("weighted_sum_fwd_kernel");
    } else if constexpr (KIND == 1) {
        hipLaunchKernelGGL((weighted_sum_bwd_x_kernel<LPT, ITER, W>), dim3((unsigned)blocks), dim3(kWsBlock), 0, st, a);
        DMET_LAUNCH_CHECK("weighted_sum_bwd_x_kernel");
    } else {
        hipLaunchKernelGGL((weighted_sum_bwd_w_kernel<LPT, W == 4>), dim3((unsigned)blocks), dim3(kWsBlock), 0, st, a);
        DMET_LAUNCH_CHECK("weighted_sum_bwd_w_kernel");
    }
    return 0;
}

// lanes per row and units per lane for a width F, as multi_aggr.hip: 16-byte units (vec), one per lane, 16 lanes up to
// F = 64, 32 up to 128, 64 up to 256; float units: 16 lanes up to F = 32 (two per lane), 32 up to 128 and 64 up to 256
// (four per lane).  KIND 0: forward, 1: backward by source, 2: backward by target, which keeps the vec form's lanes.
template <int KIND>
int dispatch(const WsArgs &a, bool vec, hipStream_t st)
{
    if (vec) {
        if (a.F <= 64) return launch<KIND, 16, 1, 4>(a, st);
        if (a.F <= 128) return launch<KIND, 32, 1, 4>(a, st);
        return launch<KIND, 64, 1, 4>(a, st);
    }
    if constexpr (KIND == 2) {
        if (a.F <= 64) return launch<KIND, 16, 1, 1>(a, st);
        if (a.F <= 128) return launch<KIND, 32, 1, 1>(a, st);
        return launch<KIND, 64, 1, 1>(a, st);
    } else {
        if (a.F <= 32) return launch<KIND, 16, 2, 1>(a, st);
        if (a.F <= 128) return launch<KIND, 32, 4, 1>(a, st);
        return launch<KIND, 64, 4, 1>(a, st);
    }
}

int check_args(const char *who, WsArgs &a, int64_t Nt, int64_t Ns, int64_t E, int width, int F)
{
    DMET_REQUIRE(Nt >= 0 && Ns >= 0 && Nt < (int64_t)2147483647 && Ns < (int64_t)2147483647,
                 "%s: Nt=%lld, Ns=%lld out of range", who, (long long)Nt, (long long)Ns);
    DMET_REQUIRE(F >= 1 && F <= kWsMaxF, "%s: F=%d not in [1,%d]", who, F, kWsMaxF);
    DMET_REQUIRE(width >= 0 && width <= DMET_MAX_K, "%s: width=%d not in [1,%d] (0: an edge list)", who, width, DMET_MAX_K);
    if (width == 0)
        DMET_REQUIRE(E >= 0 && E < (int64_t)2147483647, "%s: E=%lld out of range", who, (long long)E);
    else
        DMET_REQUIRE(Nt * (int64_t)width < (int64_t)2147483647, "%s: Nt*width out of range", who);
    a.Nt = Nt; a.Ns = Ns; a.k = width; a.F = F;
    a.M = width == 0 ? E : Nt * (int64_t)width;
    return 0;
}

}  // namespace
}  // namespace dmet

using namespace dmet;

extern "C" int dmet_weighted_sum_fwd_f32(const float *x, const float *w, const int32_t *idx, const int32_t *rowptr,
                                         int64_t Nt, int64_t Ns, int64_t E, int width, int F, float *out, int32_t *count,
                                         dmet_stream_t stream)
{
    const char *who = "dmet_weighted_sum_fwd_f32";
    WsArgs a{};
    if (int rc = check_args(who, a, Nt, Ns, E, width, F)) return rc;
    if (Nt == 0) return 0;
    const bool list = width == 0;
    DMET_REQUIRE(out, "%s: null out", who);
    DMET_REQUIRE(!list || rowptr, "%s: an edge list (width 0) needs rowptr", who);
    DMET_REQUIRE(idx || (list && E == 0), "%s: null nbr / src", who);
    DMET_REQUIRE(Ns == 0 || x, "%s: null x with Ns=%lld", who, (long long)Ns);
    a.x = x; a.w = w; a.idx = idx; a.rowptr = list ? rowptr : nullptr;
    a.out = out; a.count = count;
    const bool vec = F % 4 == 0 && aligned16(x) && aligned16(out);
    return dispatch<0>(a, vec, as_stream(stream));
}

extern "C" int dmet_weighted_sum_bwd_f32(const float *x, const float *w, const float *g_out, const int32_t *idx,
                                         const int32_t *rowptr, const int32_t *tgt, const int32_t *rev_ptr,
                                         const int32_t *rev_pos, int64_t Nt, int64_t Ns, int64_t E, int width, int F,
                                         float *g_x, float *g_w, dmet_stream_t stream)
{
    const char *who = "dmet_weighted_sum_bwd_f32";
    WsArgs a{};
    if (int rc = check_args(who, a, Nt, Ns, E, width, F)) return rc;
    DMET_REQUIRE(g_x || g_w, "%s: neither g_x nor g_w is asked for", who);
    hipStream_t st = as_stream(stream);
    if (Nt == 0) {      // no target: nothing reaches a source, and only a list can hold positions
        if (g_x != nullptr && Ns > 0) {
            hipError_t e = hipMemsetAsync(g_x, 0, (size_t)Ns * F * sizeof(float), st);
            if (e != hipSuccess) return hip_fail(e, "dmet_weighted_sum_bwd_f32: memset");
        }
        if (g_w != nullptr && a.M > 0) {
            hipError_t e = hipMemsetAsync(g_w, 0, (size_t)a.M * sizeof(float), st);
            if (e != hipSuccess) return hip_fail(e, "dmet_weighted_sum_bwd_f32: memset");
        }
        return 0;
    }
    const bool list = width == 0;
    DMET_REQUIRE(g_out, "%s: null g_out", who);
    DMET_REQUIRE(!list || rowptr, "%s: an edge list (width 0) needs rowptr", who);
    DMET_REQUIRE(idx || (list && E == 0), "%s: null nbr / src", who);
    DMET_REQUIRE(!list || tgt || E == 0, "%s: an edge list (width 0) needs tgt", who);
    a.x = x; a.w = w; a.g_out = g_out; a.idx = idx; a.rowptr = list ? rowptr : nullptr; a.tgt = list ? tgt : nullptr;
    a.rev_ptr = rev_ptr; a.rev_pos = rev_pos; a.g_x = g_x; a.g_w = g_w;
    if (g_x != nullptr) {
        DMET_REQUIRE(rev_ptr, "%s: g_x needs rev_ptr", who);
        DMET_REQUIRE(a.M == 0 || rev_pos, "%s: g_x needs rev_pos", who);
    }
    if (g_w != nullptr) DMET_REQUIRE(Ns == 0 || x, "%s: g_w needs x with Ns=%lld", who, (long long)Ns);
    if (g_x != nullptr && Ns > 0) {
        const bool vec = F % 4 == 0 && aligned16(g_out) && aligned16(g_x);
        if (int rc = dispatch<1>(a, vec, st)) return rc;
    }
    if (g_w != nullptr && a.M > 0) {
        const bool vec = F % 4 == 0 && aligned16(g_out) && aligned16(x);
        if (int rc = dispatch<2>(a, vec, st)) return rc;
    }
    return 0;
}

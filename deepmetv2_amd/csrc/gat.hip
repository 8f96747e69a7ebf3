// gat.hip -- additive-attention aggregation (torch_geometric.nn.GATConv / GATv2Conv: edge_update, utils.softmax and the
// 'add' aggregation) over a fixed-width table or a grouped edge list.
//
// For target i, head h and every valid entry e of row i, j = src(e), lrelu(t) = t > 0 ? t : slope t:
//   v2 (GATv2Conv):  score_e = sum_c att[h,c] lrelu(xl[j,h,c] + xr[i,h,c])
//   v1 (GATConv):    score_e = lrelu(s_src[j,h] + s_dst[i,h])
//   out[i,h,:] = sum_e softmax_e(score) xl[j,h,:]        lse[i,h] = max_e score_e + logf(sum_e expf(score_e - max))
// PyG adds 1e-16 to the softmax denominator; it is omitted here as in attention.hip: the denominator is at least 1 (the
// maximum's own term), so 1e-16 is below fp32 rounding.  Key and value are the same row: one head-row gather per edge
// and pass.  Nothing of message width is written per edge; the backward recomputes the scores and keeps two floats per
// (edge, head): alpha and g_score.
//
// self_loops (one node set, Nt == Ns): a written entry with j == i is skipped and one entry i -> i is taken after the
// row's own entries -- remove_self_loops + add_self_loops without rewriting the graph (the csrc/pointnet.hip
// convention).  The by-source pass adds the same entry for source i after its reverse list.
//
// Lane layout, all three kernels, is attention.hip's: a group of LPT lanes (16 for C <= 32, 32 beyond; inside one
// wavefront) owns one (row, head) pair, a row of any length is taken in chunks of LPT entries, lane l reads the id of
// entry l once, the group walks the chunk kGatInFlight gathers at a time over the channels c = lane, lane + LPT, a
// channel sum is each lane's partial sum in ascending c followed by the xor butterfly of the group, and lane e keeps
// the scalars of entry e.  The running (m, l, acc) is rescaled once per chunk that holds a valid entry; l and acc add
// their terms in ascending entry order, the implicit self entry last.  No LDS, no __syncthreads, no float atomics: the
// bits depend on LPT, never on the launch or the run, and a table and the edge list of the same entries in the same
// order give the same bits.  Every loop is bounded by a row length or a reverse-list length read once and clamped.
#include <math.h>

#include "common.h"

namespace dmet {
namespace {

constexpr int kGatMaxC = 64;
constexpr int kGatMaxH = 16;
constexpr int kGatMaxHC = 256;
constexpr int kGatBlock = 256;
constexpr int kGatInFlight = 4;    // head-row gathers in flight per group
constexpr int kGatV1 = 1, kGatV2 = 2;

template <int LPT>
__device__ __forceinline__ float gat_group_sum(float v)
{
    // xor butterfly inside the group: a fixed order, and every lane of the group ends with the same bits
#pragma unroll
    for (int off = LPT / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, LPT);
    return v;
}

template <int LPT>
__device__ __forceinline__ float gat_group_max(float v)
{
#pragma unroll
    for (int off = LPT / 2; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, LPT));
    return v;
}

template <int LPT, int ITER>
__device__ __forceinline__ float gat_group_dot(const float (&a)[ITER], const float (&b)[ITER])
{
    float part = 0.f;
#pragma unroll
    for (int it = 0; it < ITER; ++it) part += a[it] * b[it];
    return gat_group_sum<LPT>(part);
}

__device__ __forceinline__ float gat_lrelu(float t, float slope) { return t > 0.f ? t : slope * t; }
__device__ __forceinline__ float gat_dlrelu(float t, float slope) { return t > 0.f ? 1.f : slope; }   // slope at t == 0, as torch

// the v2 score: the one chain the forward and the backward form it with (channels past C hold zeros in all three rows)
template <int LPT, int ITER>
__device__ __forceinline__ float gat_score_v2(const float (&at)[ITER], const float (&xl)[ITER], const float (&xr)[ITER],
                                              float slope)
{
    float part = 0.f;
#pragma unroll
    for (int it = 0; it < ITER; ++it) part += at[it] * gat_lrelu(xl[it] + xr[it], slope);
    return gat_group_sum<LPT>(part);
}

// channels lane, lane + LPT, ... of the head row at p (zeros past C, and for a missing row)
template <int LPT, int ITER>
__device__ __forceinline__ void gat_load_row(float (&r)[ITER], const float *__restrict__ p, bool on, int lane, int C)
{
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
        const int c = lane + it * LPT;
        r[it] = (on && c < C) ? p[c] : 0.f;
    }
}

struct GatGraph {
    const int32_t *idx;       // nbr[Nt, k] (table) or src[E] (list)
    const int32_t *rowptr;    // NULL: table
    const int32_t *tgt;       // list, backward only
    const int32_t *rev_ptr, *rev_pos;
    int64_t Nt, Ns, M;        // M = Nt*k or E: the number of positions
    int k;
    int self_loops;
};

// positions [lo, lo + n) of row i, clamped to [0, M]
__device__ __forceinline__ void gat_row(const GatGraph &g, int64_t i, int64_t &lo, int &n)
{
    if (g.rowptr == nullptr) {
        lo = i * g.k;
        n = g.k;
    } else {
        lo = min(max((int64_t)g.rowptr[i], (int64_t)0), g.M);
        const int64_t hi = min(max((int64_t)g.rowptr[i + 1], lo), g.M);
        n = (int)(hi - lo);
    }
}

// the id of logical entry t of row i: the written entries [0, n), then (self_loops) the entry i -> i at t == n; -1 for
// an empty slot, an id outside [0, Ns), a written self loop under self_loops, and anything past the row
__device__ __forceinline__ int32_t gat_entry(const GatGraph &g, int64_t i, int64_t lo, int n, int t)
{
    if (t < n) {
        const int32_t j = g.idx[lo + t];
        if (j < 0 || (int64_t)j >= g.Ns) return -1;
        if (g.self_loops && (int64_t)j == i) return -1;
        return j;
    }
    return (g.self_loops && t == n) ? (int32_t)i : -1;
}

struct GatArgs {
    const float *xl, *xr, *att, *s_src, *s_dst, *out, *lse, *g_out;
    float slope;
    GatGraph g;
    int H, C;
    float *o, *l, *alpha, *alpha_w, *gs_w, *alpha_self, *gs_self, *g_xl, *g_xr, *g_att_rows, *g_ssrc, *g_sdst;
};

template <int LPT, int ITER, int MODE>
__global__ __launch_bounds__(kGatBlock) void gat_fwd_kernel(GatArgs a)
{
    constexpr int TPB = kGatBlock / LPT;
    const GatGraph &g = a.g;
    const int H = a.H, C = a.C;
    const int bid = xcd_swizzle(blockIdx.x, gridDim.x);
    const int64_t unit = (int64_t)bid * TPB + threadIdx.x / LPT;
    const int lane = threadIdx.x % LPT;
    if (unit >= g.Nt * H) return;        // whole groups leave: the shuffles below stay inside a group
    const int64_t i = unit / H;
    const int h = (int)(unit - i * H);
    const int HC = H * C;
    const float slope = a.slope;
    int64_t lo;
    int n;
    gat_row(g, i, lo, n);
    const int ne = n + (g.self_loops ? 1 : 0);      // logical entries: the self entry after the row's own

    float xr[ITER], at[ITER], acc[ITER];
    float sd = 0.f;
    if constexpr (MODE == kGatV2) {
        gat_load_row<LPT, ITER>(xr, a.xr + i * HC + h * C, true, lane, C);
        gat_load_row<LPT, ITER>(at, a.att + h * C, true, lane, C);
    } else {
        sd = a.s_dst[unit];
    }
#pragma unroll
    for (int it = 0; it < ITER; ++it) acc[it] = 0.f;
    float m = -INFINITY, l = 0.f;
    int cnt = 0;
    for (int base = 0; base < ne; base += LPT) {
        const int32_t jl = gat_entry(g, i, lo, n, base + lane);      // lane l: the id of entry base + l
        const int mch = min(LPT, ne - base);
        float sl = -INFINITY;           // lane e keeps the score of entry base + e
        if constexpr (MODE == kGatV2) {
            for (int e0 = 0; e0 < mch; e0 += kGatInFlight) {
                int32_t j[kGatInFlight];
                float xj[kGatInFlight][ITER];
#pragma unroll
                for (int u = 0; u < kGatInFlight; ++u) {
                    j[u] = __shfl(jl, (e0 + u) & (LPT - 1), LPT);
                    if (e0 + u >= mch) j[u] = -1;
                }
#pragma unroll
                for (int u = 0; u < kGatInFlight; ++u)
                    gat_load_row<LPT, ITER>(xj[u], a.xl + (int64_t)max(j[u], 0) * HC + h * C, j[u] >= 0, lane, C);
#pragma unroll
                for (int u = 0; u < kGatInFlight; ++u) {
                    if (j[u] < 0) continue;        // the same for every lane of the group
                    const float s = gat_score_v2<LPT, ITER>(at, xj[u], xr, slope);
                    if (lane == e0 + u) sl = s;
                }
            }
        } else if (jl >= 0) {
            sl = gat_lrelu(a.s_src[(int64_t)jl * H + h] + sd, slope);      // a scalar per entry: each lane forms its own
        }
        if (a.alpha != nullptr && base + lane < n) a.alpha[(lo + base + lane) * H + h] = sl;     // the score, until (m, l) is known
        if (gat_group_max<LPT>(jl >= 0 ? 1.f : 0.f) == 0.f) continue;      // a chunk of empty slots: the running state stays
        const float m_new = fmaxf(m, gat_group_max<LPT>(sl));
        const float scale = (cnt == 0) ? 0.f : expf(m - m_new);
        const float pl = jl >= 0 ? expf(sl - m_new) : 0.f;
        m = m_new;
        l *= scale;
#pragma unroll
        for (int it = 0; it < ITER; ++it) acc[it] *= scale;
        for (int e0 = 0; e0 < mch; e0 += kGatInFlight) {
            int32_t j[kGatInFlight];
            float p[kGatInFlight], xj[kGatInFlight][ITER];
#pragma unroll
            for (int u = 0; u < kGatInFlight; ++u) {
                j[u] = __shfl(jl, (e0 + u) & (LPT - 1), LPT);
                p[u] = __shfl(pl, (e0 + u) & (LPT - 1), LPT);
                if (e0 + u >= mch) j[u] = -1;
            }
#pragma unroll
            for (int u = 0; u < kGatInFlight; ++u)
                gat_load_row<LPT, ITER>(xj[u], a.xl + (int64_t)max(j[u], 0) * HC + h * C, j[u] >= 0, lane, C);
#pragma unroll
            for (int u = 0; u < kGatInFlight; ++u) {
                if (j[u] < 0) continue;
                l += p[u];
#pragma unroll
                for (int it = 0; it < ITER; ++it) acc[it] += p[u] * xj[u][it];
                ++cnt;
            }
        }
    }
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
        const int c = lane + it * LPT;
        if (c < C) a.o[i * HC + h * C + c] = cnt > 0 ? acc[it] / l : 0.f;     // a row without a valid entry: zeros (R3)
    }
    if (lane == 0) a.l[unit] = cnt > 0 ? m + logf(l) : 0.f;
    if (a.alpha != nullptr) {
        // each lane turns the scores it stored itself into weights; an empty slot is told by its id, not by the value
        for (int t = lane; t < n; t += LPT) {
            const int64_t pos = (lo + t) * H + h;
            a.alpha[pos] = gat_entry(g, i, lo, n, t) >= 0 ? expf(a.alpha[pos] - m) / l : 0.f;
        }
    }
}

// By-target pass: alpha and g_s of every position (0 in an empty slot; the self entry's pair goes to alpha_self / gs_self)
// and the target-side gradients.
//   delta = g_out[i,h,:] . out[i,h,:]    alpha_e = expf(score_e - lse)    g_s_e = alpha_e (g_out[i,h,:] . xl[j,h,:] - delta)
//   v2: g_xr[i,h,c] = sum_e (g_s_e att[h,c]) lrelu'(t_e[c]),  g_att_rows[i,h,c] = sum_e g_s_e lrelu(t_e[c]);  gs_w = g_s_e
//   v1: g_sdst[i,h] = sum_e g_s_e lrelu'(s_src[j,h] + s_dst[i,h]);  gs_w holds that product, the by-source pass sums it
template <int LPT, int ITER, int MODE>
__global__ __launch_bounds__(kGatBlock) void gat_bwd_target_kernel(GatArgs a)
{
    constexpr int TPB = kGatBlock / LPT;
    const GatGraph &g = a.g;
    const int H = a.H, C = a.C;
    const int bid = xcd_swizzle(blockIdx.x, gridDim.x);
    const int64_t unit = (int64_t)bid * TPB + threadIdx.x / LPT;
    const int lane = threadIdx.x % LPT;
    if (unit >= g.Nt * H) return;
    const int64_t i = unit / H;
    const int h = (int)(unit - i * H);
    const int HC = H * C;
    const float slope = a.slope;
    int64_t lo;
    int n;
    gat_row(g, i, lo, n);
    const int ne = n + (g.self_loops ? 1 : 0);

    float xr[ITER], at[ITER], go[ITER], o[ITER], gxr[ITER], gat[ITER];
    float sd = 0.f, gsd = 0.f;
    if constexpr (MODE == kGatV2) {
        gat_load_row<LPT, ITER>(xr, a.xr + i * HC + h * C, true, lane, C);
        gat_load_row<LPT, ITER>(at, a.att + h * C, true, lane, C);
    } else {
        sd = a.s_dst[unit];
    }
    gat_load_row<LPT, ITER>(go, a.g_out + i * HC + h * C, true, lane, C);
    gat_load_row<LPT, ITER>(o, a.out + i * HC + h * C, true, lane, C);
#pragma unroll
    for (int it = 0; it < ITER; ++it) gxr[it] = gat[it] = 0.f;
    const float delta = gat_group_dot<LPT, ITER>(go, o);
    const float ls = a.lse[unit];
    for (int base = 0; base < ne; base += LPT) {
        const int32_t jl = gat_entry(g, i, lo, n, base + lane);
        const int mch = min(LPT, ne - base);
        float al = 0.f, gl = 0.f;        // lane e keeps alpha and g_s of entry base + e for one store
        float dl = 0.f;                  // v1: lane e's lrelu' (and alpha in al) before the walk
        if (MODE == kGatV1 && jl >= 0) {
            const float t = a.s_src[(int64_t)jl * H + h] + sd;
            al = expf(gat_lrelu(t, slope) - ls);       // the forward's bits
            dl = gat_dlrelu(t, slope);
        }
        for (int e0 = 0; e0 < mch; e0 += kGatInFlight) {
            int32_t j[kGatInFlight];
            float av[kGatInFlight], dv[kGatInFlight], xj[kGatInFlight][ITER];
#pragma unroll
            for (int u = 0; u < kGatInFlight; ++u) {
                const int from = (e0 + u) & (LPT - 1);
                j[u] = __shfl(jl, from, LPT);
                if (MODE == kGatV1) {
                    av[u] = __shfl(al, from, LPT);
                    dv[u] = __shfl(dl, from, LPT);
                }
                if (e0 + u >= mch) j[u] = -1;
            }
#pragma unroll
            for (int u = 0; u < kGatInFlight; ++u)
                gat_load_row<LPT, ITER>(xj[u], a.xl + (int64_t)max(j[u], 0) * HC + h * C, j[u] >= 0, lane, C);
#pragma unroll
            for (int u = 0; u < kGatInFlight; ++u) {
                if (j[u] < 0) continue;        // the same for every lane of the group
                if constexpr (MODE == kGatV2) {
                    const float s = gat_score_v2<LPT, ITER>(at, xj[u], xr, slope);       // the forward's bits
                    const float al_e = expf(s - ls);
                    const float gs = al_e * (gat_group_dot<LPT, ITER>(go, xj[u]) - delta);
                    if (lane == e0 + u) {
                        al = al_e;
                        gl = gs;
                    }
#pragma unroll
                    for (int it = 0; it < ITER; ++it) {
                        const float t = xj[u][it] + xr[it];
                        gxr[it] += (gs * at[it]) * gat_dlrelu(t, slope);
                        gat[it] += gs * gat_lrelu(t, slope);
                    }
                } else {
                    const float gs = av[u] * (gat_group_dot<LPT, ITER>(go, xj[u]) - delta);
                    const float gp = gs * dv[u];
                    if (lane == e0 + u) gl = gp;
                    gsd += gp;
                }
            }
        }
        const int t = base + lane;
        if (t < n) {
            const int64_t pos = (lo + t) * H + h;
            a.alpha_w[pos] = al;
            a.gs_w[pos] = gl;
        } else if (t == n && g.self_loops) {
            a.alpha_self[unit] = al;
            a.gs_self[unit] = gl;
        }
    }
    if constexpr (MODE == kGatV2) {
#pragma unroll
        for (int it = 0; it < ITER; ++it) {
            const int c = lane + it * LPT;
            if (c < C) {
                a.g_xr[i * HC + h * C + c] = gxr[it];
                a.g_att_rows[i * HC + h * C + c] = gat[it];
            }
        }
    } else if (lane == 0) {
        a.g_sdst[unit] = gsd;
    }
}

// By-source pass: for source j and head h, over the positions that hold j (rev_pos, ascending), i = the position's row,
// then (self_loops) the implicit entry j -> j:
//   v2: g_xl[j,h,c] = sum alpha_e g_out[i,h,c] + (g_s_e att[h,c]) lrelu'(xl[j,h,c] + xr[i,h,c])
//   v1: g_xl[j,h,:] = sum alpha_e g_out[i,h,:]      g_ssrc[j,h] = sum gs_w
// A hub's list is walked by its one group, however long it is.
template <int LPT, int ITER, int MODE>
__global__ __launch_bounds__(kGatBlock) void gat_bwd_source_kernel(GatArgs a)
{
    constexpr int TPB = kGatBlock / LPT;
    const GatGraph &g = a.g;
    const int H = a.H, C = a.C;
    const int bid = xcd_swizzle(blockIdx.x, gridDim.x);
    const int64_t unit = (int64_t)bid * TPB + threadIdx.x / LPT;
    const int lane = threadIdx.x % LPT;
    if (unit >= g.Ns * H) return;
    const int64_t j = unit / H;
    const int h = (int)(unit - j * H);
    const int HC = H * C;
    const float slope = a.slope;
    const int64_t lo = min(max((int64_t)g.rev_ptr[j], (int64_t)0), g.M);
    const int64_t hi = min(max((int64_t)g.rev_ptr[j + 1], lo), g.M);

    float xj[ITER], at[ITER], gx[ITER];
    float gss = 0.f;
    if constexpr (MODE == kGatV2) {
        gat_load_row<LPT, ITER>(xj, a.xl + j * HC + h * C, true, lane, C);
        gat_load_row<LPT, ITER>(at, a.att + h * C, true, lane, C);
    }
#pragma unroll
    for (int it = 0; it < ITER; ++it) gx[it] = 0.f;
    for (int64_t base = lo; base < hi; base += LPT) {
        // lane l: target, alpha and g_s of entry base + l
        int32_t il = -1;
        float al = 0.f, gl = 0.f;
        if (base + lane < hi) {
            const int64_t pos = g.rev_pos[base + lane];
            if (pos >= 0 && pos < g.M) {
                const int64_t i = g.rowptr == nullptr ? pos / g.k : (int64_t)g.tgt[pos];
                if (i >= 0 && i < g.Nt && !(g.self_loops && i == j)) {      // a written self loop was skipped by target too
                    il = (int32_t)i;
                    al = a.alpha_w[pos * H + h];
                    gl = a.gs_w[pos * H + h];
                }
            }
        }
        const int mch = (int)min((int64_t)LPT, hi - base);
        for (int e0 = 0; e0 < mch; e0 += kGatInFlight) {
            int32_t i[kGatInFlight];
            float av[kGatInFlight], gs[kGatInFlight], gr[kGatInFlight][ITER], xi[kGatInFlight][ITER];
#pragma unroll
            for (int u = 0; u < kGatInFlight; ++u) {
                const int from = (e0 + u) & (LPT - 1);
                i[u] = __shfl(il, from, LPT);
                av[u] = __shfl(al, from, LPT);
                gs[u] = __shfl(gl, from, LPT);
                if (e0 + u >= mch) i[u] = -1;
            }
#pragma unroll
            for (int u = 0; u < kGatInFlight; ++u) {
                const int64_t row = (int64_t)max(i[u], 0) * HC + h * C;
                gat_load_row<LPT, ITER>(gr[u], a.g_out + row, i[u] >= 0, lane, C);
                if constexpr (MODE == kGatV2) gat_load_row<LPT, ITER>(xi[u], a.xr + row, i[u] >= 0, lane, C);
            }
#pragma unroll
            for (int u = 0; u < kGatInFlight; ++u) {
                if (i[u] < 0) continue;        // the same for every lane of the group
                if constexpr (MODE == kGatV2) {
#pragma unroll
                    for (int it = 0; it < ITER; ++it)
                        gx[it] += av[u] * gr[u][it] + (gs[u] * at[it]) * gat_dlrelu(xj[it] + xi[u][it], slope);
                } else {
#pragma unroll
                    for (int it = 0; it < ITER; ++it) gx[it] += av[u] * gr[u][it];
                    gss += gs[u];
                }
            }
        }
    }
    if (g.self_loops) {      // the implicit entry j -> j, after the reverse list (Nt == Ns)
        const float av = a.alpha_self[unit], gs = a.gs_self[unit];
        float gr[ITER], xi[ITER];
        gat_load_row<LPT, ITER>(gr, a.g_out + j * HC + h * C, true, lane, C);
        if constexpr (MODE == kGatV2) {
            gat_load_row<LPT, ITER>(xi, a.xr + j * HC + h * C, true, lane, C);
#pragma unroll
            for (int it = 0; it < ITER; ++it) gx[it] += av * gr[it] + (gs * at[it]) * gat_dlrelu(xj[it] + xi[it], slope);
        } else {
#pragma unroll
            for (int it = 0; it < ITER; ++it) gx[it] += av * gr[it];
            gss += gs;
        }
    }
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
        const int c = lane + it * LPT;
        if (c < C) a.g_xl[j * HC + h * C + c] = gx[it];
    }
    if (MODE == kGatV1 && lane == 0) a.g_ssrc[unit] = gss;
}

template <int LPT, int ITER, int MODE>
int launch_fwd(const GatArgs &a, hipStream_t st)
{
    constexpr int TPB = kGatBlock / LPT;
    const int64_t blocks = (a.g.Nt * a.H + TPB - 1) / TPB;
    hipLaunchKernelGGL((gat_fwd_kernel<LPT, ITER, MODE>), dim3((unsigned)blocks), dim3(kGatBlock), 0, st, a);
    DMET_LAUNCH_CHECK("gat_fwd_kernel");
    return 0;
}

template <int LPT, int ITER, int MODE>
int launch_bwd(const GatArgs &a, hipStream_t st)
{
    constexpr int TPB = kGatBlock / LPT;
    const int64_t tb = (a.g.Nt * a.H + TPB - 1) / TPB, sb = (a.g.Ns * a.H + TPB - 1) / TPB;    // sb = 0: empty rows only
    hipLaunchKernelGGL((gat_bwd_target_kernel<LPT, ITER, MODE>), dim3((unsigned)tb), dim3(kGatBlock), 0, st, a);
    DMET_LAUNCH_CHECK("gat_bwd_target_kernel");
    if (sb == 0) return 0;
    hipLaunchKernelGGL((gat_bwd_source_kernel<LPT, ITER, MODE>), dim3((unsigned)sb), dim3(kGatBlock), 0, st, a);
    DMET_LAUNCH_CHECK("gat_bwd_source_kernel");
    return 0;
}

// lanes per (row, head) pair and channels per lane for a head width C: 16 lanes up to 32 channels, 32 beyond
template <bool FWD, int MODE>
int dispatch_width(const GatArgs &a, hipStream_t st)
{
    if (a.C <= 16) return FWD ? launch_fwd<16, 1, MODE>(a, st) : launch_bwd<16, 1, MODE>(a, st);
    if (a.C <= 32) return FWD ? launch_fwd<16, 2, MODE>(a, st) : launch_bwd<16, 2, MODE>(a, st);
    return FWD ? launch_fwd<32, 2, MODE>(a, st) : launch_bwd<32, 2, MODE>(a, st);
}

template <bool FWD>
int dispatch(int mode, const GatArgs &a, hipStream_t st)
{
    return mode == kGatV2 ? dispatch_width<FWD, kGatV2>(a, st) : dispatch_width<FWD, kGatV1>(a, st);
}

bool supported(int H, int C) { return C >= 1 && C <= kGatMaxC && H >= 1 && H <= kGatMaxH && H * C <= kGatMaxHC; }

int check_shape(const char *who, int mode, bool list, int64_t Nt, int64_t Ns, int64_t E, int k, int H, int C, float slope,
                int self_loops)
{
    DMET_REQUIRE(mode == kGatV1 || mode == kGatV2, "%s: mode=%d, 1 (GATConv) or 2 (GATv2Conv)", who, mode);
    DMET_REQUIRE(Nt >= 0 && Ns >= 0 && Nt < (int64_t)2147483647 && Ns < (int64_t)2147483647,
                 "%s: Nt=%lld, Ns=%lld out of range", who, (long long)Nt, (long long)Ns);
    DMET_REQUIRE(supported(H, C), "%s: H=%d, C=%d not in 1 <= C <= %d, 1 <= H <= %d, H*C <= %d", who, H, C, kGatMaxC,
                 kGatMaxH, kGatMaxHC);
    DMET_REQUIRE(isfinite(slope) && slope >= 0.f, "%s: slope=%g must be finite and >= 0", who, (double)slope);
    DMET_REQUIRE(self_loops == 0 || self_loops == 1, "%s: self_loops=%d, 0 or 1", who, self_loops);
    DMET_REQUIRE(!self_loops || Nt == Ns, "%s: self_loops needs one node set, Nt=%lld Ns=%lld", who, (long long)Nt,
                 (long long)Ns);
    if (list)
        DMET_REQUIRE(E >= 0 && E < (int64_t)2147483647, "%s: E=%lld out of range", who, (long long)E);
    else
        DMET_REQUIRE(k >= 1 && k <= DMET_MAX_K, "%s: k=%d not in [1,%d] (table form: rowptr NULL)", who, k, DMET_MAX_K);
    DMET_REQUIRE(list || Nt * (int64_t)k < (int64_t)2147483647, "%s: Nt*k out of range", who);
    // a launch covers Nt*H (Ns*H) lane groups, at least 8 to a workgroup
    DMET_REQUIRE(Nt * (int64_t)H < (int64_t)2147483647 * 4 && Ns * (int64_t)H < (int64_t)2147483647 * 4,
                 "%s: Nt*H or Ns*H out of range", who);
    return 0;
}

}  // namespace
}  // namespace dmet

using namespace dmet;

extern "C" int dmet_gat_supported(int H, int C) { return supported(H, C) ? 1 : 0; }

extern "C" int dmet_gat_fwd_f32(int mode, const float *xl, const float *xr, const float *att, const float *s_src,
                                const float *s_dst, float slope, int self_loops, const int32_t *idx,
                                const int32_t *rowptr, int64_t Nt, int64_t Ns, int64_t E, int width, int H, int C,
                                float *out, float *lse, float *alpha, dmet_stream_t stream)
{
    const char *who = "dmet_gat_fwd_f32";
    const bool list = rowptr != nullptr;
    if (int rc = check_shape(who, mode, list, Nt, Ns, E, width, H, C, slope, self_loops)) return rc;
    if (Nt == 0) return 0;
    DMET_REQUIRE(out && lse, "%s: null pointer", who);
    DMET_REQUIRE(idx || (list && E == 0), "%s: null nbr / src", who);
    DMET_REQUIRE(Ns == 0 || xl, "%s: null xl with Ns=%lld", who, (long long)Ns);
    if (mode == kGatV2)
        DMET_REQUIRE(xr && att, "%s: mode 2 needs xr and att", who);
    else
        DMET_REQUIRE(s_dst && (Ns == 0 || s_src), "%s: mode 1 needs s_src and s_dst", who);
    GatArgs a{};
    a.xl = xl; a.xr = xr; a.att = att; a.s_src = s_src; a.s_dst = s_dst; a.slope = slope; a.H = H; a.C = C;
    a.o = out; a.l = lse; a.alpha = alpha;
    a.g.idx = idx; a.g.rowptr = rowptr; a.g.Nt = Nt; a.g.Ns = Ns; a.g.k = list ? 0 : width;
    a.g.M = list ? E : Nt * (int64_t)width; a.g.self_loops = self_loops;
    return dispatch<true>(mode, a, as_stream(stream));
}

extern "C" int dmet_gat_bwd_f32(int mode, const float *xl, const float *xr, const float *att, const float *s_src,
                                const float *s_dst, float slope, int self_loops, const float *out, const float *lse,
                                const float *g_out, const int32_t *idx, const int32_t *rowptr, const int32_t *tgt,
                                const int32_t *rev_ptr, const int32_t *rev_pos, int64_t Nt, int64_t Ns, int64_t E,
                                int width, int H, int C, float *alpha_w, float *gs_w, float *alpha_self, float *gs_self,
                                float *g_xl, float *g_xr, float *g_att_rows, float *g_ssrc, float *g_sdst,
                                dmet_stream_t stream)
{
    const char *who = "dmet_gat_bwd_f32";
    const bool list = rowptr != nullptr;
    if (int rc = check_shape(who, mode, list, Nt, Ns, E, width, H, C, slope, self_loops)) return rc;
    if (Ns > 0) DMET_REQUIRE(g_xl && (mode == kGatV2 || g_ssrc), "%s: null g_xl / g_ssrc", who);
    hipStream_t st = as_stream(stream);
    if (Nt == 0) {      // no target: nothing reaches a source
        if (Ns > 0) {
            hipError_t e = hipMemsetAsync(g_xl, 0, (size_t)Ns * H * C * sizeof(float), st);
            if (e == hipSuccess && mode == kGatV1) e = hipMemsetAsync(g_ssrc, 0, (size_t)Ns * H * sizeof(float), st);
            if (e != hipSuccess) return hip_fail(e, "dmet_gat_bwd_f32: memset");
        }
        return 0;
    }
    DMET_REQUIRE(out && lse && g_out, "%s: null pointer", who);
    if (mode == kGatV2)
        DMET_REQUIRE(xr && att && g_xr && g_att_rows, "%s: mode 2 needs xr, att, g_xr and g_att_rows", who);
    else
        DMET_REQUIRE(s_dst && g_sdst && (Ns == 0 || s_src), "%s: mode 1 needs s_src, s_dst and g_sdst", who);
    const bool none = list && E == 0;
    DMET_REQUIRE(none || (idx && alpha_w && gs_w && (!list || tgt)), "%s: null graph / work pointer", who);
    DMET_REQUIRE(!self_loops || (alpha_self && gs_self), "%s: self_loops needs alpha_self and gs_self", who);
    DMET_REQUIRE(Ns == 0 || (xl && rev_ptr && (none || rev_pos)), "%s: null source-side pointer", who);
    GatArgs a{};
    a.xl = xl; a.xr = xr; a.att = att; a.s_src = s_src; a.s_dst = s_dst; a.slope = slope; a.H = H; a.C = C;
    a.out = out; a.lse = lse; a.g_out = g_out;
    a.alpha_w = alpha_w; a.gs_w = gs_w; a.alpha_self = alpha_self; a.gs_self = gs_self;
    a.g_xl = g_xl; a.g_xr = g_xr; a.g_att_rows = g_att_rows; a.g_ssrc = g_ssrc; a.g_sdst = g_sdst;
    a.g.idx = idx; a.g.rowptr = rowptr; a.g.tgt = tgt; a.g.rev_ptr = rev_ptr; a.g.rev_pos = rev_pos;
    a.g.Nt = Nt; a.g.Ns = Ns; a.g.k = list ? 0 : width; a.g.M = list ? E : Nt * (int64_t)width;
    a.g.self_loops = self_loops;
    return dispatch<false>(mode, a, st);
}

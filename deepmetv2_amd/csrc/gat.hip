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
// The lane layout, the running softmax of a row and the walks of the two backward passes are row_softmax.h's; here are
// the two scores, the per-entry arithmetic of the backward and the entry points.
#include "row_softmax.h"

namespace dmet {
namespace {

constexpr int kGatV1 = 1, kGatV2 = 2;

__device__ __forceinline__ float gat_lrelu(float t, float slope) { return t > 0.f ? t : slope * t; }
__device__ __forceinline__ float gat_dlrelu(float t, float slope) { return t > 0.f ? 1.f : slope; }   // slope at t == 0, as torch

struct GatArgs {
    const float *xl, *xr, *att, *s_src, *s_dst, *out, *lse, *g_out;
    float slope;
    RowGraph g;
    int H, C;
    float *o, *l, *alpha, *alpha_w, *gs_w, *alpha_self, *gs_self, *g_xl, *g_xr, *g_att_rows, *g_ssrc, *g_sdst;
};

// the v2 score of an xl row: the one chain the forward and the backward form it with (channels past C hold zeros in all
// three rows)
template <int LPT, int ITER>
struct GatScoreV2 {
    static constexpr bool kGather = true;
    const float *rows;      // xl
    float xr[ITER], at[ITER], slope;
    __device__ __forceinline__ GatScoreV2(const GatArgs &a, const Unit &u) : rows(a.xl), slope(a.slope)
    {
        load_row<LPT, ITER>(xr, a.xr + u.row * a.H * a.C + u.h * a.C, true, u.lane, a.C);
        load_row<LPT, ITER>(at, a.att + u.h * a.C, true, u.lane, a.C);
    }
    __device__ __forceinline__ float operator()(const float (&xl)[ITER]) const
    {
        float part = 0.f;
#pragma unroll
        for (int it = 0; it < ITER; ++it) part += at[it] * gat_lrelu(xl[it] + xr[it], slope);
        return group_sum<LPT>(part);
    }
};

// the v1 score: a scalar per entry, each lane forms its own
struct GatScoreV1 {
    static constexpr bool kGather = false;
    const float *s_src;
    float sd, slope;
    int H, h;
    __device__ __forceinline__ GatScoreV1(const GatArgs &a, const Unit &u)
        : s_src(a.s_src), sd(a.s_dst[u.unit]), slope(a.slope), H(a.H), h(u.h)
    {
    }
    __device__ __forceinline__ float sum(int32_t j) const { return s_src[(int64_t)j * H + h] + sd; }
    __device__ __forceinline__ float operator()(int32_t j) const { return gat_lrelu(sum(j), slope); }
};

template <int LPT, int ITER, int MODE>
__global__ __launch_bounds__(kBlock) void gat_fwd_kernel(GatArgs a)
{
    Unit u;
    if (!take_unit<LPT>(a.g.Nt, a.H, u)) return;
    if constexpr (MODE == kGatV2)
        softmax_row_fwd<LPT, ITER>(a.g, u, a.H, a.C, GatScoreV2<LPT, ITER>(a, u), a.xl, a.o, a.l, a.alpha);
    else
        softmax_row_fwd<LPT, ITER>(a.g, u, a.H, a.C, GatScoreV1(a, u), a.xl, a.o, a.l, a.alpha);
}

// By-target pass: alpha and g_s of every position (0 in an empty slot; the self entry's pair goes to alpha_self / gs_self)
// and the target-side gradients.
//   delta = g_out[i,h,:] . out[i,h,:]    alpha_e = expf(score_e - lse)    g_s_e = alpha_e (g_out[i,h,:] . xl[j,h,:] - delta)
//   v2: g_xr[i,h,c] = sum_e (g_s_e att[h,c]) lrelu'(t_e[c]),  g_att_rows[i,h,c] = sum_e g_s_e lrelu(t_e[c]);  gs_w = g_s_e
//   v1: g_sdst[i,h] = sum_e g_s_e lrelu'(s_src[j,h] + s_dst[i,h]);  gs_w holds that product, the by-source pass sums it
template <int LPT, int ITER, int MODE>
__global__ __launch_bounds__(kBlock) void gat_bwd_target_kernel(GatArgs a)
{
    Unit u;
    if (!take_unit<LPT>(a.g.Nt, a.H, u)) return;
    const int C = a.C;
    const float slope = a.slope;
    float go[ITER], delta, ls;
    target_row<LPT, ITER>(a.g_out, a.out, a.lse, u, a.H, C, go, delta, ls);
    const float *const rows[1] = {a.xl};
    if constexpr (MODE == kGatV2) {
        const GatScoreV2<LPT, ITER> score(a, u);
        float gxr[ITER], gat[ITER];
#pragma unroll
        for (int it = 0; it < ITER; ++it) gxr[it] = gat[it] = 0.f;
        target_walk<LPT, ITER, 1>(
            a.g, u, a.H, C, rows, a.alpha_w, a.gs_w, a.alpha_self, a.gs_self, [](int32_t, float &, float &) {},
            [&](const float (&r)[1][ITER], float, float, float &al, float &gs) {
                al = expf(score(r[0]) - ls);       // the forward's bits
                gs = al * (group_dot<LPT, ITER>(go, r[0]) - delta);
#pragma unroll
                for (int it = 0; it < ITER; ++it) {
                    const float t = r[0][it] + score.xr[it];
                    gxr[it] += (gs * score.at[it]) * gat_dlrelu(t, slope);
                    gat[it] += gs * gat_lrelu(t, slope);
                }
            });
#pragma unroll
        for (int it = 0; it < ITER; ++it) {
            const int c = u.lane + it * LPT;
            if (c < C) {
                a.g_xr[u.row * a.H * C + u.h * C + c] = gxr[it];
                a.g_att_rows[u.row * a.H * C + u.h * C + c] = gat[it];
            }
        }
    } else {
        const GatScoreV1 score(a, u);
        float gsd = 0.f;
        target_walk<LPT, ITER, 1>(
            a.g, u, a.H, C, rows, a.alpha_w, a.gs_w, a.alpha_self, a.gs_self,
            [&](int32_t j, float &al, float &dl) {      // lane e's alpha and lrelu' of entry e, before the walk
                if (j < 0) return;
                const float t = score.sum(j);
                al = expf(gat_lrelu(t, slope) - ls);       // the forward's bits
                dl = gat_dlrelu(t, slope);
            },
            [&](const float (&r)[1][ITER], float av, float dv, float &al, float &gp) {
                const float gs = av * (group_dot<LPT, ITER>(go, r[0]) - delta);
                al = av;
                gp = gs * dv;
                gsd += gp;
            });
        if (u.lane == 0) a.g_sdst[u.unit] = gsd;
    }
}

// By-source pass: for source j and head h, over the positions that hold j, i = the position's row, then (self_loops) the
// implicit entry j -> j:
//   v2: g_xl[j,h,c] = sum alpha_e g_out[i,h,c] + (g_s_e att[h,c]) lrelu'(xl[j,h,c] + xr[i,h,c])
//   v1: g_xl[j,h,:] = sum alpha_e g_out[i,h,:]      g_ssrc[j,h] = sum gs_w
template <int LPT, int ITER, int MODE>
__global__ __launch_bounds__(kBlock) void gat_bwd_source_kernel(GatArgs a)
{
    Unit u;
    if (!take_unit<LPT>(a.g.Ns, a.H, u)) return;
    const int C = a.C;
    const float slope = a.slope;
    float gx[ITER];
#pragma unroll
    for (int it = 0; it < ITER; ++it) gx[it] = 0.f;
    if constexpr (MODE == kGatV2) {
        float xj[ITER], at[ITER];
        load_row<LPT, ITER>(xj, a.xl + u.row * a.H * C + u.h * C, true, u.lane, C);
        load_row<LPT, ITER>(at, a.att + u.h * C, true, u.lane, C);
        const float *const rows[2] = {a.g_out, a.xr};
        source_walk<LPT, ITER, 2>(a.g, u, a.H, C, rows, a.alpha_w, a.gs_w, a.alpha_self, a.gs_self,
                                  [&](const float (&r)[2][ITER], float av, float gs) {
#pragma unroll
                                      for (int it = 0; it < ITER; ++it)
                                          gx[it] += av * r[0][it] + (gs * at[it]) * gat_dlrelu(xj[it] + r[1][it], slope);
                                  });
    } else {
        float gss = 0.f;
        const float *const rows[1] = {a.g_out};
        source_walk<LPT, ITER, 1>(a.g, u, a.H, C, rows, a.alpha_w, a.gs_w, a.alpha_self, a.gs_self,
                                  [&](const float (&r)[1][ITER], float av, float gs) {
#pragma unroll
                                      for (int it = 0; it < ITER; ++it) gx[it] += av * r[0][it];
                                      gss += gs;
                                  });
        if (u.lane == 0) a.g_ssrc[u.unit] = gss;
    }
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
        const int c = u.lane + it * LPT;
        if (c < C) a.g_xl[u.row * a.H * C + u.h * C + c] = gx[it];
    }
}

template <bool FWD, int MODE>
int run(const GatArgs &a, hipStream_t st)
{
    return dispatch_width(a.C, [&](auto lpt, auto iter) {
        constexpr int LPT = decltype(lpt)::value, ITER = decltype(iter)::value;
        if constexpr (FWD) return launch<LPT>("gat_fwd_kernel", gat_fwd_kernel<LPT, ITER, MODE>, a.g.Nt, a.H, st, a);
        if (int rc = launch<LPT>("gat_bwd_target_kernel", gat_bwd_target_kernel<LPT, ITER, MODE>, a.g.Nt, a.H, st, a)) return rc;
        return launch<LPT>("gat_bwd_source_kernel", gat_bwd_source_kernel<LPT, ITER, MODE>, a.g.Ns, a.H, st, a);   // Ns == 0: no launch
    });
}

int check_shape(const char *who, int mode, bool list, int64_t Nt, int64_t Ns, int64_t E, int k, int H, int C, float slope,
                int self_loops)
{
    DMET_REQUIRE(mode == kGatV1 || mode == kGatV2, "%s: mode=%d, 1 (GATConv) or 2 (GATv2Conv)", who, mode);
    if (int rc = check_graph_shape(who, list, Nt, Ns, E, k, H, C)) return rc;
    DMET_REQUIRE(isfinite(slope) && slope >= 0.f, "%s: slope=%g must be finite and >= 0", who, (double)slope);
    DMET_REQUIRE(self_loops == 0 || self_loops == 1, "%s: self_loops=%d, 0 or 1", who, self_loops);
    DMET_REQUIRE(!self_loops || Nt == Ns, "%s: self_loops needs one node set, Nt=%lld Ns=%lld", who, (long long)Nt,
                 (long long)Ns);
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
    a.g = make_graph(idx, rowptr, nullptr, nullptr, nullptr, Nt, Ns, E, width, self_loops);
    return mode == kGatV2 ? run<true, kGatV2>(a, as_stream(stream)) : run<true, kGatV1>(a, as_stream(stream));
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
    a.g = make_graph(idx, rowptr, tgt, rev_ptr, rev_pos, Nt, Ns, E, width, self_loops);
    return mode == kGatV2 ? run<false, kGatV2>(a, st) : run<false, kGatV1>(a, st);
}

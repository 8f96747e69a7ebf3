// attention.hip -- softmax attention aggregation (torch_geometric.nn.TransformerConv's message + utils.softmax + the
// 'add' aggregation) over a fixed-width table or a grouped edge list.
//
// For target i, head h and every valid entry e of row i, j = src(e):
//   score_e = (q[i,h,:] . k[j,h,:]) / sqrtf(C)
//   out[i,h,:] = sum_e softmax_e(score) v[j,h,:]        lse[i,h] = max_e score_e + logf(sum_e expf(score_e - max))
// Nothing of message width is written per edge: the forward gathers one k and one v head row per edge, the backward
// recomputes the scores and keeps two floats per (edge, head): alpha and g_score.
//
// The lane layout, the running softmax of a row and the walks of the two backward passes are row_softmax.h's; here are
// the score, the per-entry arithmetic of the backward and the entry points.
#include "row_softmax.h"

namespace dmet {
namespace {

// score(k row) = (q[i,h,:] . k[j,h,:]) / sqrtf(C): the one chain the forward and the backward form a score with
template <int LPT, int ITER>
struct AttScore {
    static constexpr bool kGather = true;
    const float *rows;      // k
    float qr[ITER], rs;
    __device__ __forceinline__ AttScore(const float *q, const float *kx, const Unit &u, int H, int C)
        : rows(kx), rs(sqrtf((float)C))
    {
        load_row<LPT, ITER>(qr, q + u.row * H * C + u.h * C, true, u.lane, C);
    }
    __device__ __forceinline__ float operator()(const float (&kr)[ITER]) const { return group_dot<LPT, ITER>(qr, kr) / rs; }
};

template <int LPT, int ITER>
__global__ __launch_bounds__(kBlock) void attention_fwd_kernel(
    const float *__restrict__ q, const float *__restrict__ kx, const float *__restrict__ vx, RowGraph g, int H, int C,
    float *__restrict__ out, float *__restrict__ lse, float *__restrict__ alpha)
{
    Unit u;
    if (!take_unit<LPT>(g.Nt, H, u)) return;
    const AttScore<LPT, ITER> score(q, kx, u, H, C);
    softmax_row_fwd<LPT, ITER>(g, u, H, C, score, vx, out, lse, alpha);
}

// By-target pass: alpha and g_s of every position (0 in an empty slot) and g_q[i,h,:].
//   delta = g_out[i,h,:] . out[i,h,:]      alpha_e = expf(score_e - lse)      g_s_e = alpha_e (g_out[i,h,:] . v[j,h,:] - delta)
//   g_q[i,h,:] = (sum_e g_s_e k[j,h,:]) / sqrtf(C)      (ascending e)
template <int LPT, int ITER>
__global__ __launch_bounds__(kBlock) void attention_bwd_target_kernel(
    const float *__restrict__ q, const float *__restrict__ kx, const float *__restrict__ vx,
    const float *__restrict__ out, const float *__restrict__ lse, const float *__restrict__ g_out, RowGraph g, int H,
    int C, float *__restrict__ alpha_w, float *__restrict__ gs_w, float *__restrict__ g_q)
{
    Unit u;
    if (!take_unit<LPT>(g.Nt, H, u)) return;
    const AttScore<LPT, ITER> score(q, kx, u, H, C);
    float go[ITER], gq[ITER], delta, ls;
    target_row<LPT, ITER>(g_out, out, lse, u, H, C, go, delta, ls);
#pragma unroll
    for (int it = 0; it < ITER; ++it) gq[it] = 0.f;
    const float *const rows[2] = {kx, vx};
    target_walk<LPT, ITER, 2>(
        g, u, H, C, rows, alpha_w, gs_w, nullptr, nullptr, [](int32_t, float &, float &) {},
        [&](const float (&r)[2][ITER], float, float, float &a, float &gs) {
            a = expf(score(r[0]) - ls);       // the forward's bits
            gs = a * (group_dot<LPT, ITER>(go, r[1]) - delta);
#pragma unroll
            for (int it = 0; it < ITER; ++it) gq[it] += gs * r[0][it];
        });
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
        const int c = u.lane + it * LPT;
        if (c < C) g_q[u.row * H * C + u.h * C + c] = gq[it] / score.rs;
    }
}

// By-source pass: for source j and head h, over the positions that hold j, i = the position's row:
//   g_v[j,h,:] = sum alpha g_out[i,h,:]      g_k[j,h,:] = (sum g_s q[i,h,:]) / sqrtf(C)
template <int LPT, int ITER>
__global__ __launch_bounds__(kBlock) void attention_bwd_source_kernel(
    const float *__restrict__ q, const float *__restrict__ g_out, RowGraph g, int H, int C,
    const float *__restrict__ alpha_w, const float *__restrict__ gs_w, float *__restrict__ g_k, float *__restrict__ g_v)
{
    Unit u;
    if (!take_unit<LPT>(g.Ns, H, u)) return;
    const float rs = sqrtf((float)C);
    float gk[ITER], gv[ITER];
#pragma unroll
    for (int it = 0; it < ITER; ++it) gk[it] = gv[it] = 0.f;
    const float *const rows[2] = {g_out, q};
    source_walk<LPT, ITER, 2>(g, u, H, C, rows, alpha_w, gs_w, nullptr, nullptr,
                              [&](const float (&r)[2][ITER], float a, float gs) {
#pragma unroll
                                  for (int it = 0; it < ITER; ++it) {
                                      gv[it] += a * r[0][it];
                                      gk[it] += gs * r[1][it];
                                  }
                              });
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
        const int c = u.lane + it * LPT;
        if (c < C) {
            g_v[u.row * H * C + u.h * C + c] = gv[it];
            g_k[u.row * H * C + u.h * C + c] = gk[it] / rs;
        }
    }
}

}  // namespace
}  // namespace dmet

using namespace dmet;

extern "C" int dmet_attention_supported(int H, int C) { return supported(H, C) ? 1 : 0; }

extern "C" int dmet_attention_fwd_f32(const float *q, const float *k, const float *v, const int32_t *idx,
                                      const int32_t *rowptr, int64_t Nt, int64_t Ns, int64_t E, int width, int H, int C,
                                      float *out, float *lse, float *alpha, dmet_stream_t stream)
{
    const bool list = rowptr != nullptr;
    if (int rc = check_graph_shape("dmet_attention_fwd_f32", list, Nt, Ns, E, width, H, C)) return rc;
    if (Nt == 0) return 0;
    DMET_REQUIRE(q && out && lse, "dmet_attention_fwd_f32: null pointer");
    DMET_REQUIRE(idx || (list && E == 0), "dmet_attention_fwd_f32: null nbr / src");
    DMET_REQUIRE(Ns == 0 || (k && v), "dmet_attention_fwd_f32: null k / v with Ns=%lld", (long long)Ns);
    const RowGraph g = make_graph(idx, rowptr, nullptr, nullptr, nullptr, Nt, Ns, E, width, 0);
    return dispatch_width(C, [&](auto lpt, auto iter) {
        constexpr int LPT = decltype(lpt)::value, ITER = decltype(iter)::value;
        return launch<LPT>("attention_fwd_kernel", attention_fwd_kernel<LPT, ITER>, Nt, H, as_stream(stream), q, k, v, g, H,
                           C, out, lse, alpha);
    });
}

extern "C" int dmet_attention_bwd_f32(const float *q, const float *k, const float *v, const float *out, const float *lse,
                                      const float *g_out, const int32_t *idx, const int32_t *rowptr, const int32_t *tgt,
                                      const int32_t *rev_ptr, const int32_t *rev_pos, int64_t Nt, int64_t Ns, int64_t E,
                                      int width, int H, int C, float *alpha_w, float *gs_w, float *g_q, float *g_k,
                                      float *g_v, dmet_stream_t stream)
{
    const bool list = rowptr != nullptr;
    if (int rc = check_graph_shape("dmet_attention_bwd_f32", list, Nt, Ns, E, width, H, C)) return rc;
    if (Ns > 0) DMET_REQUIRE(g_k && g_v, "dmet_attention_bwd_f32: null g_k / g_v");
    hipStream_t st = as_stream(stream);
    if (Nt == 0) {      // no target: nothing reaches a source
        if (Ns > 0) {
            hipError_t e = hipMemsetAsync(g_k, 0, (size_t)Ns * H * C * sizeof(float), st);
            if (e == hipSuccess) e = hipMemsetAsync(g_v, 0, (size_t)Ns * H * C * sizeof(float), st);
            if (e != hipSuccess) return hip_fail(e, "dmet_attention_bwd_f32: memset");
        }
        return 0;
    }
    DMET_REQUIRE(q && out && lse && g_out && g_q, "dmet_attention_bwd_f32: null pointer");
    const bool none = list && E == 0;
    DMET_REQUIRE(none || (idx && alpha_w && gs_w && (!list || tgt)), "dmet_attention_bwd_f32: null graph / work pointer");
    DMET_REQUIRE(Ns == 0 || (k && v && rev_ptr && (none || rev_pos)), "dmet_attention_bwd_f32: null source-side pointer");
    const RowGraph g = make_graph(idx, rowptr, tgt, rev_ptr, rev_pos, Nt, Ns, E, width, 0);
    return dispatch_width(C, [&](auto lpt, auto iter) {
        constexpr int LPT = decltype(lpt)::value, ITER = decltype(iter)::value;
        if (int rc = launch<LPT>("attention_bwd_target_kernel", attention_bwd_target_kernel<LPT, ITER>, Nt, H, st, q, k, v,
                                 out, lse, g_out, g, H, C, alpha_w, gs_w, g_q))
            return rc;
        return launch<LPT>("attention_bwd_source_kernel", attention_bwd_source_kernel<LPT, ITER>, Ns, H, st, q, g_out, g, H,
                           C, alpha_w, gs_w, g_k, g_v);      // Ns == 0 (empty rows only): no launch
    });
}

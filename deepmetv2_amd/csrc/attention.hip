// attention.hip -- softmax attention aggregation (torch_geometric.nn.TransformerConv's message + utils.softmax + the
// 'add' aggregation) over a fixed-width table or a grouped edge list.
//
// For target i, head h and every valid entry e of row i, j = src(e):
//   score_e = (q[i,h,:] . k[j,h,:]) / sqrtf(C)
//   out[i,h,:] = sum_e softmax_e(score) v[j,h,:]        lse[i,h] = max_e score_e + logf(sum_e expf(score_e - max))
// Nothing of message width is written per edge: the forward gathers one k and one v head row per edge, the backward
// recomputes the scores and keeps two floats per (edge, head): alpha and g_score.
//
// Lane layout, all three kernels: a group of LPT lanes (16 for C <= 32, 32 beyond; inside one wavefront) owns one
// (row, head) pair -- a (target, head) in the forward and the by-target pass, a (source, head) in the by-source pass;
// the pairs of one node are neighbours in the grid, so a wavefront reads whole H*C rows.  A 256-thread workgroup holds
// 16 (LPT 16) or 8 (LPT 32) pairs.  A row of any length is taken in chunks of LPT entries: lane l reads the id of entry
// l once, the group walks the chunk kAttInFlight gathers at a time over the channels c = lane, lane + LPT of the
// contiguous head rows, a dot product is each lane's partial sum in ascending c followed by the xor butterfly of the
// group, and lane e keeps the scalars of entry e (score, then expf(score - m)) which the group takes back by shuffle.
// The running (m, l, acc) is rescaled once per chunk that holds a valid entry; l and acc add their terms in ascending
// entry order.  Sums run in slot / edge / reverse-index order with no float atomics: the bits depend on LPT (the chunk
// length), never on the launch or the run, and a table and the edge list of the same entries in the same order give
// the same bits.  Every loop is bounded by a row length or a reverse-list length read once and clamped.
#include <math.h>

#include "common.h"

namespace dmet {
namespace {

constexpr int kAttMaxC = 64;
constexpr int kAttMaxH = 16;
constexpr int kAttMaxHC = 256;
constexpr int kAttBlock = 256;
constexpr int kAttInFlight = 4;    // head-row gathers in flight per group

template <int LPT>
__device__ __forceinline__ float att_group_sum(float v)
{
    // xor butterfly inside the group: a fixed order, and every lane of the group ends with the same bits
#pragma unroll
    for (int off = LPT / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, LPT);
    return v;
}

template <int LPT>
__device__ __forceinline__ float att_group_max(float v)
{
#pragma unroll
    for (int off = LPT / 2; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, LPT));
    return v;
}

// a . b over the group's channels: the one chain the forward and the backward form a score with
template <int LPT, int ITER>
__device__ __forceinline__ float att_group_dot(const float (&a)[ITER], const float (&b)[ITER])
{
    float part = 0.f;
#pragma unroll
    for (int it = 0; it < ITER; ++it) part += a[it] * b[it];
    return att_group_sum<LPT>(part);
}

// channels lane, lane + LPT, ... of the head row at p (zeros past C, and for a missing row)
template <int LPT, int ITER>
__device__ __forceinline__ void att_load_row(float (&r)[ITER], const float *__restrict__ p, bool on, int lane, int C)
{
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
        const int c = lane + it * LPT;
        r[it] = (on && c < C) ? p[c] : 0.f;
    }
}

struct AttGraph {
    const int32_t *idx;       // nbr[Nt, k] (table) or src[E] (list)
    const int32_t *rowptr;    // NULL: table
    const int32_t *tgt;       // list, backward only
    const int32_t *rev_ptr, *rev_pos;
    int64_t Nt, Ns, M;        // M = Nt*k or E: the number of positions
    int k;
};

// positions [lo, lo + n) of row i, clamped to [0, M]
__device__ __forceinline__ void att_row(const AttGraph &g, int64_t i, int64_t &lo, int &n)
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

template <int LPT, int ITER>
__global__ __launch_bounds__(kAttBlock) void attention_fwd_kernel(
    const float *__restrict__ q, const float *__restrict__ kx, const float *__restrict__ vx, AttGraph g, int H, int C,
    float *__restrict__ out, float *__restrict__ lse, float *__restrict__ alpha)
{
    constexpr int TPB = kAttBlock / LPT;
    const int bid = xcd_swizzle(blockIdx.x, gridDim.x);
    const int64_t unit = (int64_t)bid * TPB + threadIdx.x / LPT;
    const int lane = threadIdx.x % LPT;
    if (unit >= g.Nt * H) return;        // whole groups leave: the shuffles below stay inside a group
    const int64_t i = unit / H;
    const int h = (int)(unit - i * H);
    const int HC = H * C;
    const float rs = sqrtf((float)C);
    int64_t lo;
    int n;
    att_row(g, i, lo, n);

    float qr[ITER], acc[ITER];
    att_load_row<LPT, ITER>(qr, q + i * HC + h * C, true, lane, C);
#pragma unroll
    for (int it = 0; it < ITER; ++it) acc[it] = 0.f;
    float m = -INFINITY, l = 0.f;
    int cnt = 0;
    for (int base = 0; base < n; base += LPT) {
        // lane l: the id of entry base + l
        int32_t jl = -1;
        if (base + lane < n) {
            const int32_t j = g.idx[lo + base + lane];
            if (j >= 0 && (int64_t)j < g.Ns) jl = j;
        }
        const int mch = min(LPT, n - base);
        float sl = -INFINITY;           // lane e keeps the score of entry base + e
        for (int e0 = 0; e0 < mch; e0 += kAttInFlight) {
            int32_t j[kAttInFlight];
            float kr[kAttInFlight][ITER];
#pragma unroll
            for (int u = 0; u < kAttInFlight; ++u) {
                j[u] = __shfl(jl, (e0 + u) & (LPT - 1), LPT);
                if (e0 + u >= mch) j[u] = -1;
            }
#pragma unroll
            for (int u = 0; u < kAttInFlight; ++u)
                att_load_row<LPT, ITER>(kr[u], kx + (int64_t)max(j[u], 0) * HC + h * C, j[u] >= 0, lane, C);
#pragma unroll
            for (int u = 0; u < kAttInFlight; ++u) {
                if (j[u] < 0) continue;        // the same for every lane of the group
                const float s = att_group_dot<LPT, ITER>(qr, kr[u]) / rs;
                if (lane == e0 + u) sl = s;
            }
        }
        if (alpha != nullptr && base + lane < n) alpha[(lo + base + lane) * H + h] = sl;     // the score, until the row's (m, l) is known
        if (att_group_max<LPT>(jl >= 0 ? 1.f : 0.f) == 0.f) continue;      // a chunk of empty slots: the running state stays
        const float m_new = fmaxf(m, att_group_max<LPT>(sl));
        const float scale = (cnt == 0) ? 0.f : expf(m - m_new);
        const float pl = jl >= 0 ? expf(sl - m_new) : 0.f;
        m = m_new;
        l *= scale;
#pragma unroll
        for (int it = 0; it < ITER; ++it) acc[it] *= scale;
        for (int e0 = 0; e0 < mch; e0 += kAttInFlight) {
            int32_t j[kAttInFlight];
            float p[kAttInFlight], vr[kAttInFlight][ITER];
#pragma unroll
            for (int u = 0; u < kAttInFlight; ++u) {
                j[u] = __shfl(jl, (e0 + u) & (LPT - 1), LPT);
                p[u] = __shfl(pl, (e0 + u) & (LPT - 1), LPT);
                if (e0 + u >= mch) j[u] = -1;
            }
#pragma unroll
            for (int u = 0; u < kAttInFlight; ++u)
                att_load_row<LPT, ITER>(vr[u], vx + (int64_t)max(j[u], 0) * HC + h * C, j[u] >= 0, lane, C);
#pragma unroll
            for (int u = 0; u < kAttInFlight; ++u) {
                if (j[u] < 0) continue;
                l += p[u];
#pragma unroll
                for (int it = 0; it < ITER; ++it) acc[it] += p[u] * vr[u][it];
                ++cnt;
            }
        }
    }
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
        const int c = lane + it * LPT;
        if (c < C) out[i * HC + h * C + c] = cnt > 0 ? acc[it] / l : 0.f;     // a row without a valid entry: zeros (R3)
    }
    if (lane == 0) lse[unit] = cnt > 0 ? m + logf(l) : 0.f;
    if (alpha != nullptr) {
        // each lane turns the scores it stored itself into weights; an empty slot is told by its id, not by the parked
        // value, so a valid entry whose score overflowed to -inf gets expf(-inf - m) / l like every other entry: 0
        // beside a finite m, and NaN in a row whose scores are all -inf, where out is NaN too (as torch's softmax)
        for (int t = lane; t < n; t += LPT) {
            const int64_t at = (lo + t) * H + h;
            const int32_t j = g.idx[lo + t];
            alpha[at] = (j >= 0 && (int64_t)j < g.Ns) ? expf(alpha[at] - m) / l : 0.f;
        }
    }
}

// By-target pass: alpha and g_s of every position (0 in an empty slot) and g_q[i,h,:].
//   delta = g_out[i,h,:] . out[i,h,:]      alpha_e = expf(score_e - lse)      g_s_e = alpha_e (g_out[i,h,:] . v[j,h,:] - delta)
//   g_q[i,h,:] = (sum_e g_s_e k[j,h,:]) / sqrtf(C)      (ascending e)
template <int LPT, int ITER>
__global__ __launch_bounds__(kAttBlock) void attention_bwd_target_kernel(
    const float *__restrict__ q, const float *__restrict__ kx, const float *__restrict__ vx,
    const float *__restrict__ out, const float *__restrict__ lse, const float *__restrict__ g_out, AttGraph g, int H,
    int C, float *__restrict__ alpha_w, float *__restrict__ gs_w, float *__restrict__ g_q)
{
    constexpr int TPB = kAttBlock / LPT;
    const int bid = xcd_swizzle(blockIdx.x, gridDim.x);
    const int64_t unit = (int64_t)bid * TPB + threadIdx.x / LPT;
    const int lane = threadIdx.x % LPT;
    if (unit >= g.Nt * H) return;
    const int64_t i = unit / H;
    const int h = (int)(unit - i * H);
    const int HC = H * C;
    const float rs = sqrtf((float)C);
    int64_t lo;
    int n;
    att_row(g, i, lo, n);

    float qr[ITER], go[ITER], o[ITER], gq[ITER];
    att_load_row<LPT, ITER>(qr, q + i * HC + h * C, true, lane, C);
    att_load_row<LPT, ITER>(go, g_out + i * HC + h * C, true, lane, C);
    att_load_row<LPT, ITER>(o, out + i * HC + h * C, true, lane, C);
#pragma unroll
    for (int it = 0; it < ITER; ++it) gq[it] = 0.f;
    const float delta = att_group_dot<LPT, ITER>(go, o);
    const float ls = lse[unit];
    for (int base = 0; base < n; base += LPT) {
        int32_t jl = -1;
        if (base + lane < n) {
            const int32_t j = g.idx[lo + base + lane];
            if (j >= 0 && (int64_t)j < g.Ns) jl = j;
        }
        const int mch = min(LPT, n - base);
        float al = 0.f, gl = 0.f;        // lane e keeps alpha and g_s of entry base + e for one store
        for (int e0 = 0; e0 < mch; e0 += kAttInFlight) {
            int32_t j[kAttInFlight];
            float kr[kAttInFlight][ITER], vr[kAttInFlight][ITER];
#pragma unroll
            for (int u = 0; u < kAttInFlight; ++u) {
                j[u] = __shfl(jl, (e0 + u) & (LPT - 1), LPT);
                if (e0 + u >= mch) j[u] = -1;
            }
#pragma unroll
            for (int u = 0; u < kAttInFlight; ++u) {
                const int64_t at = (int64_t)max(j[u], 0) * HC + h * C;
                att_load_row<LPT, ITER>(kr[u], kx + at, j[u] >= 0, lane, C);
                att_load_row<LPT, ITER>(vr[u], vx + at, j[u] >= 0, lane, C);
            }
#pragma unroll
            for (int u = 0; u < kAttInFlight; ++u) {
                if (j[u] < 0) continue;        // the same for every lane of the group
                const float s = att_group_dot<LPT, ITER>(qr, kr[u]) / rs;       // the forward's bits
                const float a = expf(s - ls);
                const float gs = a * (att_group_dot<LPT, ITER>(go, vr[u]) - delta);
                if (lane == e0 + u) {
                    al = a;
                    gl = gs;
                }
#pragma unroll
                for (int it = 0; it < ITER; ++it) gq[it] += gs * kr[u][it];
            }
        }
        if (base + lane < n) {
            const int64_t at = (lo + base + lane) * H + h;
            alpha_w[at] = al;
            gs_w[at] = gl;
        }
    }
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
        const int c = lane + it * LPT;
        if (c < C) g_q[i * HC + h * C + c] = gq[it] / rs;
    }
}

// By-source pass: for source j and head h, over the positions that hold j (rev_pos, ascending), i = the position's row:
//   g_v[j,h,:] = sum alpha g_out[i,h,:]      g_k[j,h,:] = (sum g_s q[i,h,:]) / sqrtf(C)
// A hub's list is walked by its one group, however long it is.
template <int LPT, int ITER>
__global__ __launch_bounds__(kAttBlock) void attention_bwd_source_kernel(
    const float *__restrict__ q, const float *__restrict__ g_out, AttGraph g, int H, int C,
    const float *__restrict__ alpha_w, const float *__restrict__ gs_w, float *__restrict__ g_k, float *__restrict__ g_v)
{
    constexpr int TPB = kAttBlock / LPT;
    const int bid = xcd_swizzle(blockIdx.x, gridDim.x);
    const int64_t unit = (int64_t)bid * TPB + threadIdx.x / LPT;
    const int lane = threadIdx.x % LPT;
    if (unit >= g.Ns * H) return;
    const int64_t j = unit / H;
    const int h = (int)(unit - j * H);
    const int HC = H * C;
    const float rs = sqrtf((float)C);
    const int64_t lo = min(max((int64_t)g.rev_ptr[j], (int64_t)0), g.M);
    const int64_t hi = min(max((int64_t)g.rev_ptr[j + 1], lo), g.M);

    float gk[ITER], gv[ITER];
#pragma unroll
    for (int it = 0; it < ITER; ++it) gk[it] = gv[it] = 0.f;
    for (int64_t base = lo; base < hi; base += LPT) {
        // lane l: target, alpha and g_s of entry base + l
        int32_t il = -1;
        float al = 0.f, gl = 0.f;
        if (base + lane < hi) {
            const int64_t pos = g.rev_pos[base + lane];
            if (pos >= 0 && pos < g.M) {
                const int64_t i = g.rowptr == nullptr ? pos / g.k : (int64_t)g.tgt[pos];
                if (i >= 0 && i < g.Nt) {
                    il = (int32_t)i;
                    al = alpha_w[pos * H + h];
                    gl = gs_w[pos * H + h];
                }
            }
        }
        const int mch = (int)min((int64_t)LPT, hi - base);
        for (int e0 = 0; e0 < mch; e0 += kAttInFlight) {
            int32_t i[kAttInFlight];
            float a[kAttInFlight], gs[kAttInFlight], gr[kAttInFlight][ITER], qr[kAttInFlight][ITER];
#pragma unroll
            for (int u = 0; u < kAttInFlight; ++u) {
                const int from = (e0 + u) & (LPT - 1);
                i[u] = __shfl(il, from, LPT);
                a[u] = __shfl(al, from, LPT);
                gs[u] = __shfl(gl, from, LPT);
                if (e0 + u >= mch) i[u] = -1;
            }
#pragma unroll
            for (int u = 0; u < kAttInFlight; ++u) {
                const int64_t at = (int64_t)max(i[u], 0) * HC + h * C;
                att_load_row<LPT, ITER>(gr[u], g_out + at, i[u] >= 0, lane, C);
                att_load_row<LPT, ITER>(qr[u], q + at, i[u] >= 0, lane, C);
            }
#pragma unroll
            for (int u = 0; u < kAttInFlight; ++u) {
                if (i[u] < 0) continue;        // the same for every lane of the group
#pragma unroll
                for (int it = 0; it < ITER; ++it) {
                    gv[it] += a[u] * gr[u][it];
                    gk[it] += gs[u] * qr[u][it];
                }
            }
        }
    }
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
        const int c = lane + it * LPT;
        if (c < C) {
            g_v[j * HC + h * C + c] = gv[it];
            g_k[j * HC + h * C + c] = gk[it] / rs;
        }
    }
}

struct AttArgs {
    const float *q, *k, *v, *out, *lse, *g_out;
    AttGraph g;
    int H, C;
    float *o, *l, *alpha, *alpha_w, *gs_w, *g_q, *g_k, *g_v;
};

template <int LPT, int ITER>
int launch_fwd(const AttArgs &a, hipStream_t st)
{
    constexpr int TPB = kAttBlock / LPT;
    const int64_t blocks = (a.g.Nt * a.H + TPB - 1) / TPB;
    hipLaunchKernelGGL((attention_fwd_kernel<LPT, ITER>), dim3((unsigned)blocks), dim3(kAttBlock), 0, st, a.q, a.k, a.v,
                       a.g, a.H, a.C, a.o, a.l, a.alpha);
    DMET_LAUNCH_CHECK("attention_fwd_kernel");
    return 0;
}

template <int LPT, int ITER>
int launch_bwd(const AttArgs &a, hipStream_t st)
{
    constexpr int TPB = kAttBlock / LPT;
    const int64_t tb = (a.g.Nt * a.H + TPB - 1) / TPB, sb = (a.g.Ns * a.H + TPB - 1) / TPB;    // sb = 0: empty rows only
    hipLaunchKernelGGL((attention_bwd_target_kernel<LPT, ITER>), dim3((unsigned)tb), dim3(kAttBlock), 0, st, a.q, a.k,
                       a.v, a.out, a.lse, a.g_out, a.g, a.H, a.C, a.alpha_w, a.gs_w, a.g_q);
    DMET_LAUNCH_CHECK("attention_bwd_target_kernel");
    if (sb == 0) return 0;
    hipLaunchKernelGGL((attention_bwd_source_kernel<LPT, ITER>), dim3((unsigned)sb), dim3(kAttBlock), 0, st, a.q,
                       a.g_out, a.g, a.H, a.C, a.alpha_w, a.gs_w, a.g_k, a.g_v);
    DMET_LAUNCH_CHECK("attention_bwd_source_kernel");
    return 0;
}

// lanes per (row, head) pair and channels per lane for a head width C: 16 lanes up to 32 channels, 32 beyond
template <bool FWD>
int dispatch(const AttArgs &a, hipStream_t st)
{
    if (a.C <= 16) return FWD ? launch_fwd<16, 1>(a, st) : launch_bwd<16, 1>(a, st);
    if (a.C <= 32) return FWD ? launch_fwd<16, 2>(a, st) : launch_bwd<16, 2>(a, st);
    return FWD ? launch_fwd<32, 2>(a, st) : launch_bwd<32, 2>(a, st);
}

bool supported(int H, int C) { return C >= 1 && C <= kAttMaxC && H >= 1 && H <= kAttMaxH && H * C <= kAttMaxHC; }

int check_shape(const char *who, bool list, int64_t Nt, int64_t Ns, int64_t E, int k, int H, int C)
{
    DMET_REQUIRE(Nt >= 0 && Ns >= 0 && Nt < (int64_t)2147483647 && Ns < (int64_t)2147483647,
                 "%s: Nt=%lld, Ns=%lld out of range", who, (long long)Nt, (long long)Ns);
    DMET_REQUIRE(supported(H, C), "%s: H=%d, C=%d not in 1 <= C <= %d, 1 <= H <= %d, H*C <= %d", who, H, C, kAttMaxC,
                 kAttMaxH, kAttMaxHC);
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

extern "C" int dmet_attention_supported(int H, int C) { return supported(H, C) ? 1 : 0; }

extern "C" int dmet_attention_fwd_f32(const float *q, const float *k, const float *v, const int32_t *idx,
                                      const int32_t *rowptr, int64_t Nt, int64_t Ns, int64_t E, int width, int H, int C,
                                      float *out, float *lse, float *alpha, dmet_stream_t stream)
{
    const bool list = rowptr != nullptr;
    if (int rc = check_shape("dmet_attention_fwd_f32", list, Nt, Ns, E, width, H, C)) return rc;
    if (Nt == 0) return 0;
    DMET_REQUIRE(q && out && lse, "dmet_attention_fwd_f32: null pointer");
    DMET_REQUIRE(idx || (list && E == 0), "dmet_attention_fwd_f32: null nbr / src");
    DMET_REQUIRE(Ns == 0 || (k && v), "dmet_attention_fwd_f32: null k / v with Ns=%lld", (long long)Ns);
    AttArgs a{};
    a.q = q; a.k = k; a.v = v; a.H = H; a.C = C; a.o = out; a.l = lse; a.alpha = alpha;
    a.g.idx = idx; a.g.rowptr = rowptr; a.g.Nt = Nt; a.g.Ns = Ns; a.g.k = list ? 0 : width;
    a.g.M = list ? E : Nt * (int64_t)width;
    return dispatch<true>(a, as_stream(stream));
}

extern "C" int dmet_attention_bwd_f32(const float *q, const float *k, const float *v, const float *out, const float *lse,
                                      const float *g_out, const int32_t *idx, const int32_t *rowptr, const int32_t *tgt,
                                      const int32_t *rev_ptr, const int32_t *rev_pos, int64_t Nt, int64_t Ns, int64_t E,
                                      int width, int H, int C, float *alpha_w, float *gs_w, float *g_q, float *g_k,
                                      float *g_v, dmet_stream_t stream)
{
    const bool list = rowptr != nullptr;
    if (int rc = check_shape("dmet_attention_bwd_f32", list, Nt, Ns, E, width, H, C)) return rc;
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
    AttArgs a{};
    a.q = q; a.k = k; a.v = v; a.out = out; a.lse = lse; a.g_out = g_out; a.H = H; a.C = C;
    a.alpha_w = alpha_w; a.gs_w = gs_w; a.g_q = g_q; a.g_k = g_k; a.g_v = g_v;
    a.g.idx = idx; a.g.rowptr = rowptr; a.g.tgt = tgt; a.g.rev_ptr = rev_ptr; a.g.rev_pos = rev_pos;
    a.g.Nt = Nt; a.g.Ns = Ns; a.g.k = list ? 0 : width; a.g.M = list ? E : Nt * (int64_t)width;
    return dispatch<false>(a, st);
}

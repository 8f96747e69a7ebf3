// gravnet.hip -- GravNet aggregation (torch_geometric.nn.GravNetConv's propagate step) over a fixed-width table.
//
// For target i and every valid slot t of its row, j = nbr[i,t]:
//   d = sum_c fmaf(a, a, acc), a = s_src[j,c] - s_tgt[i,c]   (the R1 chain: the bits of the kNN build's `dist`)
//   w = expf(-10 d)
//   out[i, 0:P] = (sum_t w h[j,:]) / cnt_i      out[i, P:2P] = max_t w h[j,:], arg = the winning slot (lowest on ties)
// The max runs over the messages that are numbers: a NaN never wins and never blocks; all NaN: NaN, arg 255.
// The [E, P] messages are never written: the forward gathers one h row per edge, the backward recomputes w.
//
// Lane layout, all three kernels: a group of LPT lanes (16 or 32, inside one wavefront) owns one row (a target in the
// forward and the by-target pass, a source in the by-source pass).  Per chunk of LPT entries of the row, lane l forms
// the scalars of entry l (id, w, ...) once; the group then walks the chunk, takes each entry's scalars from the lane
// that formed them (a shuffle inside the group) and runs over the channels p = lane, lane + LPT, ... of the contiguous
// h[j,:] / g_out[i,:] row.  P stays a run-time argument (ITER = ceil(P / LPT) is the compiled bound).
// Sums run in slot / reverse-index order with no float atomics: every run gives the same bits.
#include "common.h"

namespace dmet {
namespace {

constexpr int kGravMaxS = 16;        // coordinates of the learned space
constexpr int kGravBlock = 256;
constexpr int kGravInFlight = 4;   // row gathers in flight per group
constexpr uint8_t kGravNoWinner = 255;

// w of one (target row, source row) pair; the chain of dmet_knn_f32 (R1), then expf
__device__ __forceinline__ float grav_weight(const float *__restrict__ ss, const float *__restrict__ st, int S)
{
    float d = 0.f;
    for (int c = 0; c < S; ++c) {
        const float a = ss[c] - st[c];
        d = fmaf(a, a, d);
    }
    return expf(-10.0f * d);
}

template <int LPT>
__device__ __forceinline__ float group_sum(float v)
{
    // xor butterfly inside the group: a fixed order, and every lane of the group ends with the same bits
#pragma unroll
    for (int off = LPT / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, LPT);
    return v;
}

template <int LPT, int ITER>
__global__ __launch_bounds__(kGravBlock) void gravnet_fwd_kernel(
    const float *__restrict__ s_tgt, const float *__restrict__ s_src, const float *__restrict__ h,
    const int32_t *__restrict__ nbr, int64_t Nt, int64_t Ns, int k, int S, int P, float *__restrict__ out,
    uint8_t *__restrict__ arg, int32_t *__restrict__ cnt)
{
    constexpr int TPB = kGravBlock / LPT;
    const int bid = xcd_swizzle(blockIdx.x, gridDim.x);
    const int64_t i = (int64_t)bid * TPB + threadIdx.x / LPT;
    const int lane = threadIdx.x % LPT;
    if (i >= Nt) return;        // whole groups leave: the shuffles below stay inside a group
    const int32_t *row = nbr + i * k;
    const float *st = s_tgt + i * S;

    float sum[ITER], mx[ITER];
    int win[ITER];
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
        sum[it] = 0.f;
        mx[it] = NAN;       // NaN: no number among the messages yet
        win[it] = kGravNoWinner;
    }
    int n = 0;
    for (int base = 0; base < k; base += LPT) {
        // lane l: id and weight of slot base + l
        int32_t jl = -1;
        float wl = 0.f;
        if (base + lane < k) {
            const int32_t j = row[base + lane];
            if (j >= 0 && (int64_t)j < Ns) {
                jl = j;
                wl = grav_weight(s_src + (int64_t)j * S, st, S);
            }
        }
        const int m = min(LPT, k - base);
        for (int e0 = 0; e0 < m; e0 += kGravInFlight) {
            // kGravInFlight row gathers in flight, then the sums in slot order
            int32_t j[kGravInFlight];
            float w[kGravInFlight], v[kGravInFlight][ITER];
#pragma unroll
            for (int u = 0; u < kGravInFlight; ++u) {
                j[u] = __shfl(jl, (e0 + u) & (LPT - 1), LPT);
                w[u] = __shfl(wl, (e0 + u) & (LPT - 1), LPT);
                if (e0 + u >= m) j[u] = -1;
            }
#pragma unroll
            for (int u = 0; u < kGravInFlight; ++u)
#pragma unroll
                for (int it = 0; it < ITER; ++it) {
                    const int p = lane + it * LPT;
                    v[u][it] = (j[u] >= 0 && p < P) ? h[(int64_t)j[u] * P + p] : 0.f;
                }
#pragma unroll
            for (int u = 0; u < kGravInFlight; ++u) {
                if (j[u] < 0) continue;        // the same for every lane of the group
                const int t = base + e0 + u;
#pragma unroll
                for (int it = 0; it < ITER; ++it) {
                    const float m_ = w[u] * v[u][it];
                    sum[it] += m_;
                    // strict: ties keep the lower slot (R4).  While mx is NaN any message replaces it, so the first
                    // number is taken whatever it is (+-inf too); once mx is a number a NaN fails the comparison: it
                    // never wins and never blocks, in any slot
                    if (m_ > mx[it] || mx[it] != mx[it]) {
                        mx[it] = m_;
                        win[it] = t;
                    }
                }
                ++n;
            }
        }
    }
    const float fn = (float)n;
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
        const int p = lane + it * LPT;
        if (p < P) {
            out[i * 2 * P + p] = n > 0 ? sum[it] / fn : 0.f;         // a row without a valid slot: zeros (R3)
            // no number among the messages of a non-empty row: mx is still NaN, and arg is 255 (the backward routes
            // nothing)
            out[i * 2 * P + P + p] = n > 0 ? mx[it] : 0.f;
            arg[i * P + p] = mx[it] != mx[it] ? kGravNoWinner : (uint8_t)win[it];
        }
    }
    if (lane == 0) cnt[i] = n;
}

// By-target pass: g_d[i,t] for every slot (0 in an empty one) and g_s_tgt[i,:].
//   g_msg[i,t,p] = g_out[i,p] / cnt_i + (arg[i,p] == t ? g_out[i,P+p] : 0)
//   g_w = sum_p g_msg h[j,p]  (per lane in ascending p, then the butterfly),  g_d = -10 w g_w
//   g_s_tgt[i,c] = sum_t 2 g_d (s_tgt[i,c] - s_src[j,c])  (ascending t; lane c owns coordinate c, S <= 16 <= LPT)
template <int LPT, int ITER>
__global__ __launch_bounds__(kGravBlock) void gravnet_bwd_target_kernel(
    const float *__restrict__ s_tgt, const float *__restrict__ s_src, const float *__restrict__ h,
    const int32_t *__restrict__ nbr, const uint8_t *__restrict__ arg, const int32_t *__restrict__ cnt,
    const float *__restrict__ g_out, int64_t Nt, int64_t Ns, int k, int S, int P, float *__restrict__ g_d,
    float *__restrict__ g_s_tgt)
{
    constexpr int TPB = kGravBlock / LPT;
    const int bid = xcd_swizzle(blockIdx.x, gridDim.x);
    const int64_t i = (int64_t)bid * TPB + threadIdx.x / LPT;
    const int lane = threadIdx.x % LPT;
    if (i >= Nt) return;
    const int32_t *row = nbr + i * k;
    const float *st = s_tgt + i * S;
    const int n = cnt[i];
    const float fn = (float)max(n, 1);

    float gmean[ITER], gmax[ITER];
    int win[ITER];
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
        const int p = lane + it * LPT;
        gmean[it] = 0.f;
        gmax[it] = 0.f;
        win[it] = kGravNoWinner;
        if (p < P && n > 0) {
            gmean[it] = g_out[i * 2 * P + p] / fn;
            gmax[it] = g_out[i * 2 * P + P + p];
            win[it] = arg[i * P + p];
        }
    }
    const float stc = lane < S ? st[lane] : 0.f;
    float gs = 0.f;
    for (int base = 0; base < k; base += LPT) {
        int32_t jl = -1;
        float wl = 0.f;
        if (base + lane < k && n > 0) {
            const int32_t j = row[base + lane];
            if (j >= 0 && (int64_t)j < Ns) {
                jl = j;
                wl = grav_weight(s_src + (int64_t)j * S, st, S);
            }
        }
        const int m = min(LPT, k - base);
        float gdl = 0.f;        // lane e keeps g_d of slot base + e for one coalesced store
        for (int e0 = 0; e0 < m; e0 += kGravInFlight) {
            int32_t j[kGravInFlight];
            float w[kGravInFlight], v[kGravInFlight][ITER], sj[kGravInFlight];
#pragma unroll
            for (int u = 0; u < kGravInFlight; ++u) {
                j[u] = __shfl(jl, (e0 + u) & (LPT - 1), LPT);
                w[u] = __shfl(wl, (e0 + u) & (LPT - 1), LPT);
                if (e0 + u >= m) j[u] = -1;
            }
#pragma unroll
            for (int u = 0; u < kGravInFlight; ++u) {
#pragma unroll
                for (int it = 0; it < ITER; ++it) {
                    const int p = lane + it * LPT;
                    v[u][it] = (j[u] >= 0 && p < P) ? h[(int64_t)j[u] * P + p] : 0.f;
                }
                sj[u] = (j[u] >= 0 && lane < S) ? s_src[(int64_t)j[u] * S + lane] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < kGravInFlight; ++u) {
                if (j[u] < 0) continue;        // the same for every lane of the group
                const int t = base + e0 + u;
                float part = 0.f;
#pragma unroll
                for (int it = 0; it < ITER; ++it) {
                    const float gm = gmean[it] + (win[it] == t ? gmax[it] : 0.f);
                    part += gm * v[u][it];
                }
                const float gw = group_sum<LPT>(part);
                const float gd = (w[u] == 0.f) ? 0.f : -10.0f * w[u] * gw;     // an underflowed weight carries no gradient
                if (lane == e0 + u) gdl = gd;
                if (lane < S) gs += 2.0f * gd * (stc - sj[u]);
            }
        }
        if (base + lane < k) g_d[i * k + base + lane] = gdl;
    }
    if (lane < S) g_s_tgt[i * S + lane] = gs;
}

// By-source pass: for source j, over the table positions pos = i*k + t that hold j (rev_pos, ascending):
//   g_h[j,p] = sum w g_msg[i,t,p]      g_s_src[j,c] = sum 2 g_d[i,t] (s_src[j,c] - s_tgt[i,c])
// A hub's list is walked by its one group, however long it is.
template <int LPT, int ITER>
__global__ __launch_bounds__(kGravBlock) void gravnet_bwd_source_kernel(
    const float *__restrict__ s_tgt, const float *__restrict__ s_src, const int32_t *__restrict__ rev_ptr,
    const int32_t *__restrict__ rev_pos, const uint8_t *__restrict__ arg, const int32_t *__restrict__ cnt,
    const float *__restrict__ g_out, const float *__restrict__ g_d, int64_t Nt, int64_t Ns, int k, int S, int P,
    float *__restrict__ g_h, float *__restrict__ g_s_src)
{
    constexpr int TPB = kGravBlock / LPT;
    const int bid = xcd_swizzle(blockIdx.x, gridDim.x);
    const int64_t j = (int64_t)bid * TPB + threadIdx.x / LPT;
    const int lane = threadIdx.x % LPT;
    if (j >= Ns) return;
    const int64_t M = Nt * k;
    const float *ss = s_src + j * S;
    const float ssc = lane < S ? ss[lane] : 0.f;
    const int64_t lo = min(max((int64_t)rev_ptr[j], (int64_t)0), M);
    const int64_t hi = min(max((int64_t)rev_ptr[j + 1], lo), M);

    float acc[ITER];
#pragma unroll
    for (int it = 0; it < ITER; ++it) acc[it] = 0.f;
    float gs = 0.f;
    for (int64_t base = lo; base < hi; base += LPT) {
        // lane l: target, slot, weight, 1 / count divisor and g_d of entry base + l
        int32_t il = -1;
        int tl = 0;
        float wl = 0.f, fnl = 1.f, gdl = 0.f;
        if (base + lane < hi) {
            const int64_t pos = rev_pos[base + lane];
            if (pos >= 0 && pos < M) {
                il = (int32_t)(pos / k);
                tl = (int)(pos - (int64_t)il * k);
                wl = grav_weight(ss, s_tgt + (int64_t)il * S, S);
                fnl = (float)max(cnt[il], 1);
                gdl = g_d[pos];
            }
        }
        const int m = (int)min((int64_t)LPT, hi - base);
        for (int e0 = 0; e0 < m; e0 += kGravInFlight) {
            int32_t i[kGravInFlight];
            int t[kGravInFlight];
            float w[kGravInFlight], fn[kGravInFlight], gd[kGravInFlight];
            float ga[kGravInFlight][ITER], gb[kGravInFlight][ITER], si[kGravInFlight];
            int a[kGravInFlight][ITER];
#pragma unroll
            for (int u = 0; u < kGravInFlight; ++u) {
                const int src = (e0 + u) & (LPT - 1);
                i[u] = __shfl(il, src, LPT);
                t[u] = __shfl(tl, src, LPT);
                w[u] = __shfl(wl, src, LPT);
                fn[u] = __shfl(fnl, src, LPT);
                gd[u] = __shfl(gdl, src, LPT);
                if (e0 + u >= m) i[u] = -1;
            }
#pragma unroll
            for (int u = 0; u < kGravInFlight; ++u) {
#pragma unroll
                for (int it = 0; it < ITER; ++it) {
                    const int p = lane + it * LPT;
                    const bool on = i[u] >= 0 && p < P;
                    ga[u][it] = on ? g_out[(int64_t)i[u] * 2 * P + p] : 0.f;
                    gb[u][it] = on ? g_out[(int64_t)i[u] * 2 * P + P + p] : 0.f;
                    a[u][it] = on ? (int)arg[(int64_t)i[u] * P + p] : (int)kGravNoWinner;
                }
                si[u] = (i[u] >= 0 && lane < S) ? s_tgt[(int64_t)i[u] * S + lane] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < kGravInFlight; ++u) {
                if (i[u] < 0) continue;        // the same for every lane of the group
                if (w[u] != 0.f) {             // an underflowed weight carries no gradient
#pragma unroll
                    for (int it = 0; it < ITER; ++it) {
                        const float gm = ga[u][it] / fn[u] + (a[u][it] == t[u] ? gb[u][it] : 0.f);
                        acc[it] += w[u] * gm;
                    }
                }
                if (lane < S) gs += 2.0f * gd[u] * (ssc - si[u]);
            }
        }
    }
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
        const int p = lane + it * LPT;
        if (p < P) g_h[j * P + p] = acc[it];
    }
    if (lane < S) g_s_src[j * S + lane] = gs;
}

struct GravArgs {
    const float *s_tgt, *s_src, *h;
    const int32_t *nbr, *rev_ptr, *rev_pos;
    uint8_t *arg;
    int32_t *cnt;
    const float *g_out;
    int64_t Nt, Ns;
    int k, S, P;
    float *out, *g_d, *g_s_tgt, *g_s_src, *g_h;
};

template <int LPT, int ITER>
int launch_fwd(const GravArgs &a, hipStream_t st)
{
    constexpr int TPB = kGravBlock / LPT;
    const int64_t blocks = (a.Nt + TPB - 1) / TPB;
    hipLaunchKernelGGL((gravnet_fwd_kernel<LPT, ITER>), dim3((unsigned)blocks), dim3(kGravBlock), 0, st, a.s_tgt, a.s_src,
                       a.h, a.nbr, a.Nt, a.Ns, a.k, a.S, a.P, a.out, a.arg, a.cnt);
    DMET_LAUNCH_CHECK("gravnet_fwd_kernel");
    return 0;
}

template <int LPT, int ITER>
int launch_bwd(const GravArgs &a, hipStream_t st)
{
    constexpr int TPB = kGravBlock / LPT;
    const int64_t tb = (a.Nt + TPB - 1) / TPB, sb = (a.Ns + TPB - 1) / TPB;      // sb = 0: a table of empty rows only
    hipLaunchKernelGGL((gravnet_bwd_target_kernel<LPT, ITER>), dim3((unsigned)tb), dim3(kGravBlock), 0, st, a.s_tgt,
                       a.s_src, a.h, a.nbr, a.arg, a.cnt, a.g_out, a.Nt, a.Ns, a.k, a.S, a.P, a.g_d, a.g_s_tgt);
    DMET_LAUNCH_CHECK("gravnet_bwd_target_kernel");
    if (sb == 0) return 0;
    hipLaunchKernelGGL((gravnet_bwd_source_kernel<LPT, ITER>), dim3((unsigned)sb), dim3(kGravBlock), 0, st, a.s_tgt,
                       a.s_src, a.rev_ptr, a.rev_pos, a.arg, a.cnt, a.g_out, a.g_d, a.Nt, a.Ns, a.k, a.S, a.P, a.g_h,
                       a.g_s_src);
    DMET_LAUNCH_CHECK("gravnet_bwd_source_kernel");
    return 0;
}

// lanes per row and channels per lane for a width P: 16 lanes up to 32 channels (P = 22: two per lane), 32 beyond
template <bool FWD>
int dispatch(const GravArgs &a, hipStream_t st)
{
    if (a.P <= 16) return FWD ? launch_fwd<16, 1>(a, st) : launch_bwd<16, 1>(a, st);
    if (a.P <= 32) return FWD ? launch_fwd<16, 2>(a, st) : launch_bwd<16, 2>(a, st);
    if (a.P <= 64) return FWD ? launch_fwd<32, 2>(a, st) : launch_bwd<32, 2>(a, st);
    return FWD ? launch_fwd<32, 4>(a, st) : launch_bwd<32, 4>(a, st);
}

int check_shape(const char *who, int64_t Nt, int64_t Ns, int k, int S, int P)
{
    DMET_REQUIRE(Nt >= 0 && Ns >= 0 && Nt < (int64_t)2147483647 && Ns < (int64_t)2147483647,
                 "%s: Nt=%lld, Ns=%lld out of range", who, (long long)Nt, (long long)Ns);
    DMET_REQUIRE(k >= 1 && k <= DMET_MAX_K, "%s: k=%d not in [1,%d]", who, k, DMET_MAX_K);
    DMET_REQUIRE(S >= 1 && S <= kGravMaxS, "%s: S=%d not in [1,%d]", who, S, kGravMaxS);
    DMET_REQUIRE(P >= 1 && P <= DMET_MAX_H, "%s: P=%d not in [1,%d]", who, P, DMET_MAX_H);
    DMET_REQUIRE(Nt * (int64_t)k < (int64_t)2147483647, "%s: Nt*k out of range", who);
    DMET_REQUIRE(Nt * 2 * (int64_t)P < (int64_t)2147483647 * 4 && Ns * (int64_t)P < (int64_t)2147483647 * 4,
                 "%s: Nt*2P or Ns*P out of range", who);
    return 0;
}

}  // namespace
}  // namespace dmet

using namespace dmet;

extern "C" int dmet_gravnet_fwd_f32(const float *s_tgt, const float *s_src, const float *h, const int32_t *nbr, int64_t Nt,
                                    int64_t Ns, int k, int S, int P, float *out, uint8_t *arg, int32_t *cnt,
                                    dmet_stream_t stream)
{
    if (int rc = check_shape("dmet_gravnet_fwd_f32", Nt, Ns, k, S, P)) return rc;
    if (Nt == 0) return 0;
    DMET_REQUIRE(s_tgt && nbr && out && arg && cnt, "dmet_gravnet_fwd_f32: null pointer");
    DMET_REQUIRE(Ns == 0 || (s_src && h), "dmet_gravnet_fwd_f32: null s_src / h with Ns=%lld", (long long)Ns);
    GravArgs a{};
    a.s_tgt = s_tgt; a.s_src = s_src; a.h = h; a.nbr = nbr; a.Nt = Nt; a.Ns = Ns; a.k = k; a.S = S; a.P = P;
    a.out = out; a.arg = arg; a.cnt = cnt;
    return dispatch<true>(a, as_stream(stream));
}

extern "C" int dmet_gravnet_bwd_f32(const float *s_tgt, const float *s_src, const float *h, const int32_t *nbr,
                                    const int32_t *rev_ptr, const int32_t *rev_pos, const uint8_t *arg,
                                    const int32_t *cnt, const float *g_out, int64_t Nt, int64_t Ns, int k, int S, int P,
                                    float *g_d, float *g_s_tgt, float *g_s_src, float *g_h, dmet_stream_t stream)
{
    if (int rc = check_shape("dmet_gravnet_bwd_f32", Nt, Ns, k, S, P)) return rc;
    if (Ns > 0) DMET_REQUIRE(g_s_src && g_h, "dmet_gravnet_bwd_f32: null g_s_src / g_h");
    hipStream_t st = as_stream(stream);
    if (Nt == 0) {      // no target: nothing reaches a source
        if (Ns > 0) {
            hipError_t e = hipMemsetAsync(g_h, 0, (size_t)Ns * P * sizeof(float), st);
            if (e == hipSuccess) e = hipMemsetAsync(g_s_src, 0, (size_t)Ns * S * sizeof(float), st);
            if (e != hipSuccess) return hip_fail(e, "dmet_gravnet_bwd_f32: memset");
        }
        return 0;
    }
    DMET_REQUIRE(s_tgt && nbr && arg && cnt && g_out && g_d && g_s_tgt, "dmet_gravnet_bwd_f32: null pointer");
    DMET_REQUIRE(Ns == 0 || (s_src && h && rev_ptr && rev_pos), "dmet_gravnet_bwd_f32: null source-side pointer");
    GravArgs a{};
    a.s_tgt = s_tgt; a.s_src = s_src; a.h = h; a.nbr = nbr; a.rev_ptr = rev_ptr; a.rev_pos = rev_pos;
    a.arg = const_cast<uint8_t *>(arg); a.cnt = const_cast<int32_t *>(cnt); a.g_out = g_out;
    a.Nt = Nt; a.Ns = Ns; a.k = k; a.S = S; a.P = P; a.g_d = g_d; a.g_s_tgt = g_s_tgt; a.g_s_src = g_s_src; a.g_h = g_h;
    return dispatch<false>(a, as_stream(stream));
}

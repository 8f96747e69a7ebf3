// edgemlp_f32.hip -- fp32 EdgeConv for a two-layer edge MLP over ANY grouped edge list, forward and backward.
//
// Replaces, for  nn = Sequential(Linear(2 Hin, H1), ELU, Linear(H1, H2)[, ELU][, BatchNorm1d(H2)])  and aggr in
// {max, add, mean}, the generic route  edge_features -> nn over E rows -> segment max / sum  and its autograd graph:
// the call shape of /root/reference/model/dynamic_reduction_network.py:59-73,86-87,94-95 (EdgeConv over
// to_undirected(knn_graph(...))).
//
// Forward
//   1. node level: PQ[N][2 H1] = [x (W1a - W1b)^T + b1 | x W1b^T]  (rows_linear_kernel), so that per edge
//      h1 = ELU(P_tgt + Q_src): only the second Linear is per-edge work.
//   2. edge pass (edge_mlp_fwd_kernel): workgroup b owns the contiguous node range whose edges start at b E / nblk
//      (balanced by edges, hubs included).  It walks its edges in tiles of T = 2048 / H2 consecutive edges that may span
//      several targets: h1 tile -> LDS, z2 = W2 h1 + b2 (thread = one channel x 8 edges), m = ELU?(z2) -> LDS, then one
//      thread per channel folds the tile in edge order into the running aggregate of the current target and writes it
//      when the target changes: sum, or max / min with the winning edge position (lowest on ties: strict compares).
//      With a BatchNorm in training mode it also keeps sum m, sum m^2 per channel; one partial per workgroup.
//   3. (BatchNorm) one workgroup turns the partials into (a, b) in double, fixed order, and moves the running statistics
//      once; a node-level kernel applies the aggregate: sum a S + deg b, max a max + b (a >= 0) / a min + b, mean /deg,
//      0 for a node without in-edges (R3).
// Backward
//   1. (BatchNorm) sum_e g_y and sum_e g_y m per channel are node-level sums of g_out against deg, S or the winner's
//      value: two-stage fixed-order reduction (bn_bwd_reduce_kernel, bn_bwd_coef_kernel) -> g_gamma, g_beta and the
//      per-channel coefficients of g_m = a (g_y - mean(g_y) - xhat mean(g_y xhat)).
//   2. edge pass by target: re-computes h1, z2, m per tile, forms g_z2, g_h1 = W2^T g_z2 and g_pre1 = g_h1 ELU'(.);
//      sums g_pre1 per target into gP; accumulates gW2 / gb2 in registers -> one partial per workgroup.
//   3. the same edge pass by source (EdgeList.by_source order) sums g_pre1 per source into gQ.  No [E, *] tensor is
//      written and no atomic is used: both sums run in edge order inside one workgroup.
//   4. gW2 / gb2 = fixed-order sums of the partials; gx = [gP | gQ] [W1a - W1b ; W1b] (rows_linear_kernel).  gW1 and
//      gb1 follow from [gP | gQ]^T x on the caller's side (dmet_xty_f32).
// Numerics: fp32 throughout (fmaf chains), sums in edge order; BatchNorm statistics reduced in double.  Not bit-equal to
// the generic route (the split of the first Linear and the fused sums round differently); run to run bit-identical.
#include "edgemlp_fused.h"

namespace dmet {
namespace {

constexpr int kTpt = 8;       // edges per thread in the z2 / g_h1 products

// Y[n][m] = b[m] + sum_k X[n][k] Wt[k][m], 16 rows per workgroup; fixed summation order (ascending k)
__global__ __launch_bounds__(256) void rows_linear_kernel(const float *__restrict__ X, int64_t N, int K,
                                                          const float *__restrict__ Wt, const float *__restrict__ b, int M,
                                                          float *__restrict__ Y)
{
    __shared__ float xs[384][16];
    const int64_t n0 = (int64_t)blockIdx.x * 16;
    for (int idx = threadIdx.x; idx < 16 * K; idx += blockDim.x) {
        const int r = idx / K, k = idx - r * K;
        xs[k][r] = n0 + r < N ? X[(n0 + r) * K + k] : 0.0f;
    }
    __syncthreads();
    for (int m = threadIdx.x; m < M; m += blockDim.x) {
        const float bv = b ? b[m] : 0.0f;
        float acc[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = bv;
        for (int k = 0; k < K; ++k) {
            const float w = Wt[(int64_t)k * M + m];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 xv = *reinterpret_cast<const float4 *>(&xs[k][4 * q]);
                acc[4 * q] = __builtin_fmaf(xv.x, w, acc[4 * q]);
                acc[4 * q + 1] = __builtin_fmaf(xv.y, w, acc[4 * q + 1]);
                acc[4 * q + 2] = __builtin_fmaf(xv.z, w, acc[4 * q + 2]);
                acc[4 * q + 3] = __builtin_fmaf(xv.w, w, acc[4 * q + 3]);
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r)
            if (n0 + r < N) Y[(n0 + r) * M + m] = acc[r];
    }
}

// fwd: Wt[Hin][2 H1] = [(W1a - W1b)^T | W1b^T], bias [b1 | 0];  bwd: Wc[2 H1][Hin] = [W1a - W1b ; W1b]
__global__ void split_weights_kernel(const float *__restrict__ W1, const float *__restrict__ b1, int Hin, int H1,
                                     float *__restrict__ Wt, float *__restrict__ bias, float *__restrict__ Wc)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < 2 * H1 && bias) bias[t] = (t < H1 && b1) ? b1[t] : 0.0f;
    if (t >= H1 * Hin) return;
    const int c = t / Hin, k = t - c * Hin;
    const float wa = W1[(int64_t)c * 2 * Hin + k], wb = W1[(int64_t)c * 2 * Hin + Hin + k];
    if (Wt) {
        Wt[(int64_t)k * 2 * H1 + c] = wa - wb;
        Wt[(int64_t)k * 2 * H1 + H1 + c] = wb;
    }
    if (Wc) {
        Wc[(int64_t)c * Hin + k] = wa - wb;
        Wc[(int64_t)(H1 + c) * Hin + k] = wb;
    }
}

// W2^T image [H1][H2 + 1], rounded up to whole float4 so that the arrays after it stay 16-B aligned
__host__ __device__ __forceinline__ int w2t_floats(int H1, int H2) { return (H1 * (H2 + 1) + 3) & ~3; }

// LDS image shared by the edge passes.  [c][t] arrays use the row stride T + 4: conflict-free float4 reads along t
// with lanes along c, float4 broadcasts along t with lanes along the other channel.
template <int H2>
struct EdgeTile {
    static constexpr int T = 2048 / H2;      // edges per tile: kBlk threads x kTpt edges / H2 channels
    static constexpr int TS = T + 4;
};

// one z2 product: thread (o = tid % H2, edges 8 g .. 8 g + 7 of the tile, g = tid / H2) -> acc[8]
template <int H2>
__device__ __forceinline__ void tile_z2(const float *__restrict__ w2t, const float *__restrict__ h1s, const float *b2s,
                                        int H1, int o, int g, float acc[kTpt])
{
    constexpr int TS = EdgeTile<H2>::TS;
    const float bv = b2s[o];
#pragma unroll
    for (int u = 0; u < kTpt; ++u) acc[u] = bv;
    for (int c = 0; c < H1; ++c) {
        const float w = w2t[c * (H2 + 1) + o];
        const float4 h0 = *reinterpret_cast<const float4 *>(&h1s[c * TS + kTpt * g]);
        const float4 h1 = *reinterpret_cast<const float4 *>(&h1s[c * TS + kTpt * g + 4]);
        acc[0] = __builtin_fmaf(w, h0.x, acc[0]); acc[1] = __builtin_fmaf(w, h0.y, acc[1]);
        acc[2] = __builtin_fmaf(w, h0.z, acc[2]); acc[3] = __builtin_fmaf(w, h0.w, acc[3]);
        acc[4] = __builtin_fmaf(w, h1.x, acc[4]); acc[5] = __builtin_fmaf(w, h1.y, acc[5]);
        acc[6] = __builtin_fmaf(w, h1.z, acc[6]); acc[7] = __builtin_fmaf(w, h1.w, acc[7]);
    }
}

// stage W2^T (padded rows) and b2
template <int H2>
__device__ __forceinline__ void stage_weights(const float *__restrict__ W2, const float *__restrict__ b2, int H1, float *w2t,
                                              float *b2s)
{
    for (int idx = threadIdx.x; idx < H1 * H2; idx += blockDim.x) {
        const int o = idx / H1, c = idx - o * H1;
        w2t[c * (H2 + 1) + o] = W2[idx];
    }
    for (int o = threadIdx.x; o < H2; o += blockDim.x) b2s[o] = b2 ? b2[o] : 0.0f;
}

// h1 tile [H1][TS] = ELU(P_tgt + Q_src) for the tile's cnt edges (beyond: 0)
template <int H2>
__device__ __forceinline__ void fill_h1(const float *__restrict__ PQ, int H1, const int32_t *tg, const int32_t *sr, int cnt,
                                        float *h1s)
{
    constexpr int T = EdgeTile<H2>::T, TS = EdgeTile<H2>::TS;
    for (int idx = threadIdx.x; idx < T * H1; idx += blockDim.x) {
        const int t = idx / H1, c = idx - t * H1;
        float h = 0.0f;
        if (t < cnt) h = elu1f(PQ[(int64_t)tg[t] * 2 * H1 + c] + PQ[(int64_t)sr[t] * 2 * H1 + H1 + c]);
        h1s[c * TS + t] = h;
    }
}

// aggr: 0 max, 1 add, 2 mean.  bn: 0 none, 1 training (keep the statistics partials), 2 eval.
template <int H2>
__global__ __launch_bounds__(kBlk) void edge_mlp_fwd_kernel(const float *__restrict__ PQ, const int32_t *__restrict__ rowptr,
                                                            const int32_t *__restrict__ src, const int32_t *__restrict__ tgt,
                                                            int64_t N, int64_t E, int H1, const float *__restrict__ W2,
                                                            const float *__restrict__ b2, int act2, int aggr, int bn,
                                                            float *__restrict__ agg, int32_t *__restrict__ win,
                                                            float *__restrict__ partial)
{
    constexpr int T = EdgeTile<H2>::T, TS = EdgeTile<H2>::TS;
    extern __shared__ float lds[];
    float *w2t = lds;                              // [H1][H2 + 1]
    float *b2s = w2t + w2t_floats(H1, H2);         // [H2]
    float *h1s = b2s + H2;                         // [H1][TS]
    float *ms = h1s + H1 * TS;                     // [H2][TS]
    int32_t *tg = reinterpret_cast<int32_t *>(ms + H2 * TS);   // [T]
    int32_t *sr = tg + T;                                       // [T]
    stage_weights<H2>(W2, b2, H1, w2t, b2s);

    const int nblk = gridDim.x;
    const int64_t n0 = range_start(rowptr, N, E, blockIdx.x, nblk), n1 = range_start(rowptr, N, E, blockIdx.x + 1, nblk);
    const int64_t p0 = rowptr[n0], p1 = rowptr[n1];
    const int o = threadIdx.x % H2, g = threadIdx.x / H2;
    const bool maxa = aggr == 0, mins = maxa && bn != 0;
    // running aggregate of channel threadIdx.x (threads < H2)
    int64_t cur = -1;
    float s = 0.0f, mx = 0.0f, mn = 0.0f, st1 = 0.0f, st2 = 0.0f;
    int32_t amx = -1, amn = -1;
    auto flush = [&]() {
        if (cur < 0) return;
        const int64_t q = cur * H2 + threadIdx.x;
        if (maxa) {
            agg[q] = mx;
            win[q] = amx;
            if (mins) {
                agg[N * H2 + q] = mn;
                win[N * H2 + q] = amn;
            }
        } else {
            agg[q] = s;
        }
    };
    for (int64_t pt = p0; pt < p1; pt += T) {
        const int cnt = (int)(p1 - pt < T ? p1 - pt : T);
        __syncthreads();       // the previous tile's readers of tg / sr / ms are done
        for (int t = threadIdx.x; t < T; t += blockDim.x) {
            tg[t] = t < cnt ? tgt[pt + t] : 0;
            sr[t] = t < cnt ? src[pt + t] : 0;
        }
        __syncthreads();
        fill_h1<H2>(PQ, H1, tg, sr, cnt, h1s);
        __syncthreads();
        float acc[kTpt];
        tile_z2<H2>(w2t, h1s, b2s, H1, o, g, acc);
#pragma unroll
        for (int u = 0; u < kTpt; ++u) ms[o * TS + kTpt * g + u] = act2 ? elu1f(acc[u]) : acc[u];
        __syncthreads();
        if (threadIdx.x < H2) {
            const int c = threadIdx.x;
            for (int t = 0; t < cnt; ++t) {
                const int64_t own = tg[t];
                const float m = ms[c * TS + t];
                const int32_t e = (int32_t)(pt + t);
                if (own != cur) {
                    flush();
                    cur = own;
                    s = m; mx = m; mn = m; amx = e; amn = e;
                } else {
                    s += m;
                    if (m > mx) { mx = m; amx = e; }
                    if (m < mn) { mn = m; amn = e; }
                }
                if (bn == 1) {
                    st1 += m;
                    st2 = __builtin_fmaf(m, m, st2);
                }
            }
        }
    }
    if (threadIdx.x < H2) {
        flush();
        if (bn == 1) {
            partial[(int64_t)blockIdx.x * 2 * H2 + threadIdx.x] = st1;
            partial[(int64_t)blockIdx.x * 2 * H2 + H2 + threadIdx.x] = st2;
        }
    }
}

// bnstat[4][H2] = (a, b, mean, invstd): training -- batch statistics over the E messages (biased variance), running
// statistics moved once like torch.nn.BatchNorm1d; eval -- the running statistics.  No BatchNorm: a = 1, b = 0.
__global__ __launch_bounds__(128) void bn_fwd_finalize_kernel(const float *__restrict__ partial, int nblk, int64_t E, int H2,
                                                              int bn, const float *__restrict__ gamma,
                                                              const float *__restrict__ beta, float eps, float momentum,
                                                              float *__restrict__ running_mean, float *__restrict__ running_var,
                                                              int64_t *__restrict__ num_batches_tracked,
                                                              float *__restrict__ bnstat)
{
    const int c = threadIdx.x;
    if (c >= H2) return;
    if (bn == 0) {
        bnstat[c] = 1.0f; bnstat[H2 + c] = 0.0f; bnstat[2 * H2 + c] = 0.0f; bnstat[3 * H2 + c] = 1.0f;
        return;
    }
    double mean, var;
    if (bn == 1) {
        double s1 = 0.0, s2 = 0.0;
        for (int b = 0; b < nblk; ++b) {
            s1 += (double)partial[(int64_t)b * 2 * H2 + c];
            s2 += (double)partial[(int64_t)b * 2 * H2 + H2 + c];
        }
        const double n = (double)(E > 0 ? E : 1);
        mean = s1 / n;
        var = s2 / n - mean * mean;
        if (var < 0.0) var = 0.0;
        if (running_mean) {
            const double unbiased = n > 1.0 ? var * n / (n - 1.0) : var;
            running_mean[c] = (float)((1.0 - (double)momentum) * (double)running_mean[c] + (double)momentum * mean);
            running_var[c] = (float)((1.0 - (double)momentum) * (double)running_var[c] + (double)momentum * unbiased);
        }
        if (c == 0 && num_batches_tracked) *num_batches_tracked += 1;
    } else {
        mean = (double)running_mean[c];
        var = (double)running_var[c];
    }
    const double invstd = 1.0 / sqrt(var + (double)eps);
    const double a = (double)(gamma ? gamma[c] : 1.0f) * invstd;
    bnstat[c] = (float)a;
    bnstat[H2 + c] = (float)((double)(beta ? beta[c] : 0.0f) - mean * a);
    bnstat[2 * H2 + c] = (float)mean;
    bnstat[3 * H2 + c] = (float)invstd;
}

__global__ __launch_bounds__(256) void edge_mlp_apply_kernel(const float *__restrict__ agg, const int32_t *__restrict__ rowptr,
                                                             const float *__restrict__ bnstat, int64_t N, int H2, int aggr,
                                                             float *__restrict__ out)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= N * H2) return;
    const int64_t i = t / H2;
    const int c = (int)(t - i * H2);
    const int deg = rowptr[i + 1] - rowptr[i];
    float v = 0.0f;
    if (deg > 0) {
        const float a = bnstat[c], b = bnstat[H2 + c];
        if (aggr == 0) {
            v = __builtin_fmaf(a, a >= 0.0f ? agg[t] : agg[N * H2 + t], b);
        } else {
            v = __builtin_fmaf(a, agg[t], (float)deg * b);
            if (aggr == 2) v = v / (float)deg;
        }
    }
    out[t] = v;
}

// stage 1 of the BatchNorm backward sums: R1 = sum_i g_out w_i, R2 = sum_i g_out v_i (see the file comment); one partial
// per workgroup, threads (channel, row lane) reduced through LDS in a fixed order
__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(const float *__restrict__ g_out, const float *__restrict__ agg,
                                                            const int32_t *__restrict__ rowptr,
                                                            const float *__restrict__ bnstat, int64_t N, int H2, int aggr,
                                                            float *__restrict__ partial)
{
    __shared__ float red[2][256];
    const int o = threadIdx.x % H2, lanes = blockDim.x / H2, l = threadIdx.x / H2;
    const int64_t per = (N + gridDim.x - 1) / gridDim.x;
    const int64_t i0 = (int64_t)blockIdx.x * per, i1 = i0 + per < N ? i0 + per : N;
    const bool usemin = aggr == 0 && bnstat[o] < 0.0f;
    float r1 = 0.0f, r2 = 0.0f;
    for (int64_t i = i0 + l; i < i1; i += lanes) {
        const int deg = rowptr[i + 1] - rowptr[i];
        if (deg == 0) continue;
        const float go = g_out[i * H2 + o];
        const float v = agg[(usemin ? N * H2 : 0) + i * H2 + o];
        if (aggr == 0) { r1 += go; r2 = __builtin_fmaf(go, v, r2); }
        else if (aggr == 1) { r1 = __builtin_fmaf(go, (float)deg, r1); r2 = __builtin_fmaf(go, v, r2); }
        else { r1 += go; r2 = __builtin_fmaf(go, v / (float)deg, r2); }
    }
    red[0][threadIdx.x] = r1;
    red[1][threadIdx.x] = r2;
    __syncthreads();
    if (l == 0) {
        float a1 = 0.0f, a2 = 0.0f;
        for (int q = 0; q < lanes; ++q) { a1 += red[0][q * H2 + o]; a2 += red[1][q * H2 + o]; }
        partial[(int64_t)blockIdx.x * 2 * H2 + o] = a1;
        partial[(int64_t)blockIdx.x * 2 * H2 + H2 + o] = a2;
    }
}

// stage 2: g_beta = R1, g_gamma = invstd (R2 - mean R1); coef[3][H2] = (a, R1 / E, g_gamma / E) for the edge passes
// (eval: the batch terms are 0)
__global__ __launch_bounds__(128) void bn_bwd_coef_kernel(const float *__restrict__ partial, int nb, int64_t E, int H2, int bn,
                                                          const float *__restrict__ bnstat, float *__restrict__ ggamma,
                                                          float *__restrict__ gbeta, float *__restrict__ coef)
{
    const int c = threadIdx.x;
    if (c >= H2) return;
    double r1 = 0.0, r2 = 0.0;
    for (int b = 0; b < nb; ++b) {
        r1 += (double)partial[(int64_t)b * 2 * H2 + c];
        r2 += (double)partial[(int64_t)b * 2 * H2 + H2 + c];
    }
    const double mean = bnstat[2 * H2 + c], invstd = bnstat[3 * H2 + c];
    const double gg = invstd * (r2 - mean * r1);
    if (ggamma) ggamma[c] = (float)gg;
    if (gbeta) gbeta[c] = (float)r1;
    const double n = (double)(E > 0 ? E : 1);
    coef[c] = bnstat[c];
    coef[H2 + c] = bn == 1 ? (float)(r1 / n) : 0.0f;
    coef[2 * H2 + c] = bn == 1 ? (float)(gg / n) : 0.0f;
}

// Backward edge pass.  BY_SRC = false: positions are grouped edges (owner = tgt), sums g_pre1 per target into
// gpq[:, 0:H1] and keeps gW2 / gb2 partials; BY_SRC = true: positions walk srcperm (owner = src), sums into gpq[:, H1:2H1].
template <int H2, bool BY_SRC>
__global__ __launch_bounds__(kBlk) void edge_mlp_bwd_kernel(const float *__restrict__ PQ, const int32_t *__restrict__ rowptr,
                                                            const int32_t *__restrict__ optr, const int32_t *__restrict__ perm,
                                                            const int32_t *__restrict__ src, const int32_t *__restrict__ tgt,
                                                            int64_t N, int64_t E, int H1, const float *__restrict__ W2,
                                                            const float *__restrict__ b2, int act2, int aggr, int bn,
                                                            const float *__restrict__ g_out, const int32_t *__restrict__ win,
                                                            const float *__restrict__ bnstat, const float *__restrict__ coef,
                                                            float *__restrict__ gpq, float *__restrict__ partial)
{
    constexpr int T = EdgeTile<H2>::T, TS = EdgeTile<H2>::TS;
    constexpr int NP = (192 * H2 + kBlk - 1) / kBlk;     // gW2 entries per thread at the widest H1
    extern __shared__ float lds[];
    float *w2t = lds;                              // [H1][H2 + 1]
    float *b2s = w2t + w2t_floats(H1, H2);         // [H2]
    float *h1s = b2s + H2;                         // [H1][TS]
    float *gps = h1s + H1 * TS;                    // [H1][TS]  g_pre1
    float *gz = gps + H1 * TS;                     // [H2][TS]  g_z2
    int32_t *tg = reinterpret_cast<int32_t *>(gz + H2 * TS);   // [T]
    int32_t *sr = tg + T;                                       // [T]
    int32_t *ep = sr + T;                                       // [T] grouped edge position
    stage_weights<H2>(W2, b2, H1, w2t, b2s);

    const int nblk = gridDim.x;
    const int64_t n0 = range_start(optr, N, E, blockIdx.x, nblk), n1 = range_start(optr, N, E, blockIdx.x + 1, nblk);
    const int64_t p0 = optr[n0], p1 = optr[n1];
    const int o = threadIdx.x % H2, g = threadIdx.x / H2;
    const Gz2<H2> gz2(coef, bnstat, win, N, aggr, bn, o);
    float gw[BY_SRC ? 1 : NP];
    float gb = 0.0f;
    if (!BY_SRC) {
#pragma unroll
        for (int j = 0; j < NP; ++j) gw[j] = 0.0f;
    }
    int64_t cur = -1;
    float run = 0.0f;
    const int coff = BY_SRC ? H1 : 0;
    for (int64_t pt = p0; pt < p1; pt += T) {
        const int cnt = (int)(p1 - pt < T ? p1 - pt : T);
        __syncthreads();
        load_tile_ids<T, BY_SRC>(src, tgt, perm, pt, cnt, tg, sr, ep);
        __syncthreads();
        fill_h1<H2>(PQ, H1, tg, sr, cnt, h1s);
        __syncthreads();
        {
            float acc[kTpt], gbt = 0.0f;
            tile_z2<H2>(w2t, h1s, b2s, H1, o, g, acc);
#pragma unroll
            for (int u = 0; u < kTpt; ++u) {
                const int t = kTpt * g + u;
                const float gzv = t < cnt ? gz2(acc[u], g_out, rowptr, act2, aggr, bn, tg, ep, t, o) : 0.0f;
                gz[o * TS + t] = gzv;
                if (!BY_SRC) gbt += gzv;
            }
            if (!BY_SRC) gb += gbt;
        }
        __syncthreads();
        // g_h1 and g_pre1: items (c, group of 8 edges), lanes along c
        for (int it = threadIdx.x; it < H1 * (T / kTpt); it += blockDim.x) {
            const int q = it / H1, c = it - q * H1;
            float a[kTpt];
#pragma unroll
            for (int u = 0; u < kTpt; ++u) a[u] = 0.0f;
            for (int oo = 0; oo < H2; ++oo) {
                const float w = w2t[c * (H2 + 1) + oo];
                const float4 z0 = *reinterpret_cast<const float4 *>(&gz[oo * TS + kTpt * q]);
                const float4 z1 = *reinterpret_cast<const float4 *>(&gz[oo * TS + kTpt * q + 4]);
                a[0] = __builtin_fmaf(w, z0.x, a[0]); a[1] = __builtin_fmaf(w, z0.y, a[1]);
                a[2] = __builtin_fmaf(w, z0.z, a[2]); a[3] = __builtin_fmaf(w, z0.w, a[3]);
                a[4] = __builtin_fmaf(w, z1.x, a[4]); a[5] = __builtin_fmaf(w, z1.y, a[5]);
                a[6] = __builtin_fmaf(w, z1.z, a[6]); a[7] = __builtin_fmaf(w, z1.w, a[7]);
            }
#pragma unroll
            for (int u = 0; u < kTpt; ++u) {
                const float h = h1s[c * TS + kTpt * q + u];
                gps[c * TS + kTpt * q + u] = a[u] * (h > 0.0f ? 1.0f : h + 1.0f);
            }
        }
        if (!BY_SRC) {
            // gW2[o][c] += sum_t g_z2[t][o] h1[t][c]: thread keeps channel o and c = g, g + 256 / H2, ...
#pragma unroll
            for (int j = 0; j < NP; ++j) {
                const int c = g + j * (kBlk / H2);
                if (c < H1) {
                    // the tile's sum first, then into the running total: keeps the fp32 error of the long sum small
                    float a = 0.0f;
                    for (int t = 0; t < T; t += 4) {
                        const float4 z = *reinterpret_cast<const float4 *>(&gz[o * TS + t]);
                        const float4 h = *reinterpret_cast<const float4 *>(&h1s[c * TS + t]);
                        a = __builtin_fmaf(z.x, h.x, a); a = __builtin_fmaf(z.y, h.y, a);
                        a = __builtin_fmaf(z.z, h.z, a); a = __builtin_fmaf(z.w, h.w, a);
                    }
                    gw[j] += a;
                }
            }
        }
        __syncthreads();
        if (threadIdx.x < H1) {
            const int c = threadIdx.x;
            for (int t = 0; t < cnt; ++t) {
                const int64_t own = BY_SRC ? sr[t] : tg[t];
                const float v = gps[c * TS + t];
                if (own != cur) {
                    if (cur >= 0) gpq[cur * 2 * H1 + coff + c] = run;
                    cur = own;
                    run = v;
                } else {
                    run += v;
                }
            }
        }
    }
    if (threadIdx.x < H1 && cur >= 0) gpq[cur * 2 * H1 + coff + threadIdx.x] = run;
    if (!BY_SRC) {
        // partial[blk] = gW2 [H2][H1] | gb2 [H2]; gb2 of the kTpt-edge groups added in group order through LDS
        float *pb = partial + (int64_t)blockIdx.x * (H2 * H1 + H2);
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            const int c = g + j * (kBlk / H2);
            if (c < H1) pb[o * H1 + c] = gw[j];
        }
        __syncthreads();
        float *red = gz;
        red[threadIdx.x] = gb;
        __syncthreads();
        if (threadIdx.x < H2) {
            float a = 0.0f;
            for (int q = 0; q < kBlk / H2; ++q) a += red[q * H2 + threadIdx.x];
            pb[H2 * H1 + threadIdx.x] = a;
        }
    }
}

// gpq rows of nodes without in-edges (or out-edges) are never written by the passes above: zero them first
__global__ void zero_kernel(float *__restrict__ p, int64_t n)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) p[t] = 0.0f;
}

__global__ __launch_bounds__(256) void sum_partials_kernel(const float *__restrict__ partial, int nb, int64_t stride, int n,
                                                           float *__restrict__ outA, int nA, float *__restrict__ outB)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    double a = 0.0;
    for (int b = 0; b < nb; ++b) a += (double)partial[(int64_t)b * stride + t];
    if (t < nA) { if (outA) outA[t] = (float)a; }
    else if (outB) outB[t - nA] = (float)a;
}

inline size_t fwd_lds_bytes(int H1, int H2)
{
    const int T = 2048 / H2, TS = T + 4;
    return sizeof(float) * ((size_t)w2t_floats(H1, H2) + H2 + (size_t)H1 * TS + (size_t)H2 * TS) + 2 * sizeof(int32_t) * T;
}

inline size_t bwd_lds_bytes(int H1, int H2)
{
    const int T = 2048 / H2, TS = T + 4;
    return sizeof(float) * ((size_t)w2t_floats(H1, H2) + H2 + 2 * (size_t)H1 * TS + (size_t)H2 * TS) + 3 * sizeof(int32_t) * T;
}

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

constexpr int kBnReduceBlocks = 256;

// ---- K2 host path: every dmet_edge_mlp_{fwd,bwd}_{f32,bf16,f16} entry fills an EdgeMlp and calls edge_mlp_fwd or
// edge_mlp_bwd once ---------------------------------------------------------------------------------------------------

int supported(EdgePrec prec, int Hin, int H1, int H2)
{
    if (Hin < 1 || Hin > 128 || H1 < 1 || H1 > 192 || H1 > 2 * H2) return 0;
    if (prec == EdgePrec::f32) return H2 == 16 || H2 == 32 || H2 == 64 || H2 == 128;
    return (H2 == 32 || H2 == 64 || H2 == 128) && H1 % 16 == 0;     // whole 16 x 16 MFMA blocks
}

// The workspace of either call, the only place that knows its layout.  The forward's statistics partials and the
// backward's arrays share the bytes after the split weights; nothing is per node or per edge.
struct Workspace {
    float *w;           // fwd: Wt [Hin][2 H1], then its bias [2 H1];  bwd: Wc [2 H1][Hin]
    float *stat;        // fwd: sum m, sum m^2 [kMaxBlocks][2 H2]
    float *gw;          // bwd: gW2 | gb2 [kMaxBlocks][H2 H1 + H2]
    float *bnred;       // bwd: BatchNorm reduce partials [kBnReduceBlocks][2 H2]
    float *coef;        // bwd: [3][H2]
    size_t bytes;       // from `ws` on, with 256 bytes of slack to align it
};

Workspace carve(int64_t N, int64_t E, int Hin, int H1, int H2, void *ws)
{
    (void)N; (void)E;
    const size_t w = align256(sizeof(float) * ((size_t)2 * H1 * Hin + 2 * (size_t)H1));
    const size_t stat = align256(sizeof(float) * (size_t)kMaxBlocks * 2 * H2);
    const size_t gw = align256(sizeof(float) * (size_t)kMaxBlocks * ((size_t)H2 * H1 + H2));
    const size_t bnred = align256(sizeof(float) * (size_t)kBnReduceBlocks * 2 * H2);
    const size_t bwd = gw + bnred + align256(sizeof(float) * 3 * (size_t)H2);
    char *base = reinterpret_cast<char *>((reinterpret_cast<uintptr_t>(ws) + 255u) & ~(uintptr_t)255u);
    Workspace c;
    c.w = reinterpret_cast<float *>(base);
    c.stat = c.gw = reinterpret_cast<float *>(base + w);
    c.bnred = reinterpret_cast<float *>(base + w + gw);
    c.coef = reinterpret_cast<float *>(base + w + gw + bnred);
    c.bytes = 256 + w + (stat > bwd ? stat : bwd);
    return c;
}

size_t workspace_bytes(EdgePrec prec, int64_t N, int64_t E, int Hin, int H1, int H2)
{
    if (N < 0 || E < 0 || !supported(prec, Hin, H1, H2)) return 0;
    return carve(N, E, Hin, H1, H2, nullptr).bytes;
}

struct EdgeMlp {
    const char *entry;      // the exported function the caller called: every message names it
    EdgePrec prec;
    const float *x;
    int Hin;
    const float *W1;
    void *ws;
    size_t ws_bytes;
    dmet_stream_t stream;
    EdgePassArgs p;         // the graph, N, E, H1, H2, the second Linear, the modes and the state: what the edge passes take
    struct {
        const float *b1, *gamma, *beta;
        float eps, momentum;
        float *running_mean, *running_var;
        int64_t *num_batches_tracked;
        float *out, *pq, *bnstat;
    } fwd;
    struct {
        const float *agg;
        float *gx, *gW2, *gb2, *ggamma, *gbeta;
    } bwd;
};

// what the forward and the backward entries hand to the edge passes alike; each adds its own part by name
EdgePassArgs pass_args(const float *pq, const int32_t *rowptr, const int32_t *src, const int32_t *tgt, int64_t N, int64_t E,
                       int H1, int H2, const float *W2, const float *b2, int act2, int aggr, int bn)
{
    EdgePassArgs p{};
    p.pq = pq; p.rowptr = rowptr; p.src = src; p.tgt = tgt; p.N = N; p.E = E; p.H1 = H1; p.H2 = H2;
    p.W2 = W2; p.b2 = b2; p.act2 = act2; p.aggr = aggr; p.bn = bn;
    return p;
}

int check_common(const EdgeMlp &r, bool fwd)
{
    const char *fn = r.entry;
    const EdgePassArgs &p = r.p;
    DMET_REQUIRE(p.N >= 0 && p.N < (int64_t)2147483647 / 384, "%s: N out of range", fn);
    DMET_REQUIRE(p.E >= 0 && p.E < (int64_t)2147483647, "%s: E out of range", fn);
    DMET_REQUIRE(supported(r.prec, r.Hin, p.H1, p.H2), "%s: unsupported widths Hin=%d H1=%d H2=%d", fn, r.Hin, p.H1, p.H2);
    DMET_REQUIRE(p.aggr >= 0 && p.aggr <= 2, "%s: aggr must be 0 (max), 1 (add) or 2 (mean)", fn);
    DMET_REQUIRE(p.bn >= 0 && p.bn <= 2, "%s: bn must be 0 (none), 1 (training) or 2 (eval)", fn);
    if (fwd) {
        DMET_REQUIRE(p.bn != 2 || (r.fwd.running_mean && r.fwd.running_var), "%s: eval mode needs running statistics", fn);
        DMET_REQUIRE((r.fwd.running_mean == nullptr) == (r.fwd.running_var == nullptr), "%s: running_mean/var go together", fn);
    }
    DMET_REQUIRE(p.N > 0 || p.E == 0, "%s: E=%lld edges over no nodes", fn, (long long)p.E);
    if (p.N == 0) return 0;    // empty input: nothing is read, the entry points write only the weight gradients
    DMET_REQUIRE(r.x && p.rowptr && r.W1 && p.W2, "%s: null pointer", fn);
    DMET_REQUIRE(p.E == 0 || (p.src && p.tgt), "%s: null edge array", fn);
    DMET_REQUIRE(r.ws && r.ws_bytes >= carve(p.N, p.E, r.Hin, p.H1, p.H2, nullptr).bytes, "%s: workspace too small", fn);
    return 0;
}

// Forward: split weights -> P | Q -> edge pass (fp32 or matrix cores) -> BatchNorm finalize -> apply.
int edge_mlp_fwd(const EdgeMlp &r)
{
    const char *fn = r.entry;
    const EdgePassArgs &p = r.p;
    const int64_t N = p.N, E = p.E;
    const int Hin = r.Hin, H1 = p.H1, H2 = p.H2;
    if (int rc = check_common(r, true)) return rc;
    DMET_REQUIRE(p.bn != 1 || E > 0, "%s: batch statistics need at least one edge", fn);
    if (N == 0) return 0;      // out[0, H2]: nothing to write; running statistics do not move (bn != 1)
    DMET_REQUIRE(r.fwd.out && r.fwd.pq && p.agg && r.fwd.bnstat && (p.aggr != 0 || p.win), "%s: null output pointer", fn);
    hipStream_t st = as_stream(r.stream);
    const Workspace c = carve(N, E, Hin, H1, H2, r.ws);
    float *Wt = c.w, *bias = Wt + (size_t)Hin * 2 * H1;
    const int nw = H1 * Hin > 2 * H1 ? H1 * Hin : 2 * H1;
    hipLaunchKernelGGL(split_weights_kernel, dim3((nw + 255) / 256), dim3(256), 0, st, r.W1, r.fwd.b1, Hin, H1, Wt, bias,
                       (float *)nullptr);
    DMET_LAUNCH_CHECK("split_weights_kernel");
    hipLaunchKernelGGL(rows_linear_kernel, dim3((unsigned)((N + 15) / 16)), dim3(256), 0, st, r.x, N, Hin, (const float *)Wt,
                       (const float *)bias, 2 * H1, r.fwd.pq);
    DMET_LAUNCH_CHECK("rows_linear_kernel (P | Q)");
    const int nblk = edge_blocks(E);
    if (E > 0 && r.prec != EdgePrec::f32) {
        if (int rc = edge_mlp_fwd_pass_mma(p, r.prec, nblk, c.stat, st)) return rc;
    } else if (E > 0) {
        const size_t lds = fwd_lds_bytes(H1, H2);
        int rc = 0;
        with_int<16, 32, 64, 128>(H2, [&](auto h2) {
            constexpr int kH2 = decltype(h2)::value;
            static size_t granted = 0;
            rc = grant_lds(edge_mlp_fwd_kernel<kH2>, lds, granted, "hipFuncSetAttribute(edge_mlp_fwd_kernel)");
            if (rc == 0)
                hipLaunchKernelGGL((edge_mlp_fwd_kernel<kH2>), dim3(nblk), dim3(kBlk), lds, st, p.pq, p.rowptr, p.src, p.tgt, N, E,
                                   H1, p.W2, p.b2, p.act2, p.aggr, p.bn, p.agg, p.win, c.stat);
        });
        if (rc) return rc;
        DMET_LAUNCH_CHECK("edge_mlp_fwd_kernel");
    }
    hipLaunchKernelGGL(bn_fwd_finalize_kernel, dim3(1), dim3(128), 0, st, (const float *)c.stat, nblk, E, H2, p.bn, r.fwd.gamma,
                       r.fwd.beta, r.fwd.eps, r.fwd.momentum, r.fwd.running_mean, r.fwd.running_var,
                       r.fwd.num_batches_tracked, r.fwd.bnstat);
    DMET_LAUNCH_CHECK("bn_fwd_finalize_kernel");
    const int64_t total = N * H2;
    hipLaunchKernelGGL(edge_mlp_apply_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (const float *)p.agg,
                       p.rowptr, (const float *)r.fwd.bnstat, N, H2, p.aggr, r.fwd.out);
    DMET_LAUNCH_CHECK("edge_mlp_apply_kernel");
    return 0;
}

// Backward: split weights -> BatchNorm reduce -> coef -> zero gpq -> edge pass by target, then by source (fp32 or matrix
// cores) -> gW2 | gb2 from the partials -> gx.
int edge_mlp_bwd(EdgeMlp &r)
{
    const char *fn = r.entry;
    EdgePassArgs &p = r.p;
    const int64_t N = p.N, E = p.E;
    const int Hin = r.Hin, H1 = p.H1, H2 = p.H2, bn = p.bn;
    if (int rc = check_common(r, false)) return rc;
    hipStream_t st = as_stream(r.stream);
    if (N == 0) {
        // no nodes, no edges: every weight gradient is 0, and it is written like every other call's
        float *const zs[4] = {r.bwd.gW2, r.bwd.gb2, r.bwd.ggamma, r.bwd.gbeta};
        const int64_t ns[4] = {(int64_t)H2 * H1, H2, H2, H2};
        for (int q = 0; q < 4; ++q) {
            if (!zs[q]) continue;
            hipLaunchKernelGGL(zero_kernel, dim3((unsigned)((ns[q] + 255) / 256)), dim3(256), 0, st, zs[q], ns[q]);
            DMET_LAUNCH_CHECK("zero_kernel");
        }
        return 0;
    }
    DMET_REQUIRE(p.pq && r.bwd.agg && p.bnstat && p.g_out && p.gpq && (p.aggr != 0 || p.cwin), "%s: null pointer", fn);
    DMET_REQUIRE(E == 0 || (p.srcptr && p.srcperm), "%s: null by-source index", fn);
    const Workspace c = carve(N, E, Hin, H1, H2, r.ws);
    p.coef = c.coef;
    hipLaunchKernelGGL(split_weights_kernel, dim3((H1 * Hin + 255) / 256), dim3(256), 0, st, r.W1, (const float *)nullptr, Hin,
                       H1, (float *)nullptr, (float *)nullptr, c.w);
    DMET_LAUNCH_CHECK("split_weights_kernel");
    // BatchNorm sums over the nodes; without a BatchNorm coef = (1, 0, 0)
    const int nbr = bn ? (int)(N < kBnReduceBlocks ? N : kBnReduceBlocks) : 0;
    if (nbr > 0) {
        hipLaunchKernelGGL(bn_bwd_reduce_kernel, dim3(nbr), dim3(256), 0, st, p.g_out, r.bwd.agg, p.rowptr, p.bnstat, N, H2,
                           p.aggr, c.bnred);
        DMET_LAUNCH_CHECK("bn_bwd_reduce_kernel");
    }
    hipLaunchKernelGGL(bn_bwd_coef_kernel, dim3(1), dim3(128), 0, st, (const float *)c.bnred, nbr, E, H2, bn, p.bnstat,
                       bn ? r.bwd.ggamma : nullptr, bn ? r.bwd.gbeta : nullptr, c.coef);
    DMET_LAUNCH_CHECK("bn_bwd_coef_kernel");
    const int64_t npq = N * 2 * H1;
    hipLaunchKernelGGL(zero_kernel, dim3((unsigned)((npq + 255) / 256)), dim3(256), 0, st, p.gpq, npq);
    DMET_LAUNCH_CHECK("zero_kernel");
    const int nblk = edge_blocks(E);
    if (E > 0 && r.prec != EdgePrec::f32) {
        if (int rc = edge_mlp_bwd_pass_mma(p, r.prec, false, nblk, c.gw, st)) return rc;
        if (int rc = edge_mlp_bwd_pass_mma(p, r.prec, true, nblk, nullptr, st)) return rc;
    } else if (E > 0) {
        const size_t lds = bwd_lds_bytes(H1, H2);
        for (const bool by_src : {false, true}) {
            int rc = 0;
            with_int<16, 32, 64, 128>(H2, [&](auto h2) {
                with_flags([&](auto bs) {
                    constexpr int kH2 = decltype(h2)::value;
                    static size_t granted = 0;
                    rc = grant_lds(edge_mlp_bwd_kernel<kH2, bs()>, lds, granted, "hipFuncSetAttribute(edge_mlp_bwd_kernel)");
                    if (rc == 0)
                        hipLaunchKernelGGL((edge_mlp_bwd_kernel<kH2, bs()>), dim3(nblk), dim3(kBlk), lds, st, p.pq, p.rowptr,
                                           bs() ? p.srcptr : p.rowptr, bs() ? p.srcperm : (const int32_t *)nullptr, p.src, p.tgt,
                                           N, E, H1, p.W2, p.b2, p.act2, p.aggr, bn, p.g_out, p.cwin, p.bnstat, p.coef, p.gpq,
                                           bs() ? (float *)nullptr : c.gw);
                }, by_src);
            });
            if (rc) return rc;
            DMET_LAUNCH_CHECK(by_src ? "edge_mlp_bwd_kernel (by source)" : "edge_mlp_bwd_kernel (by target)");
        }
    }
    if (E > 0) {
        const int n = H2 * H1 + H2;
        hipLaunchKernelGGL(sum_partials_kernel, dim3((n + 255) / 256), dim3(256), 0, st, (const float *)c.gw, nblk,
                           (int64_t)n, n, r.bwd.gW2, H2 * H1, r.bwd.gb2);
        DMET_LAUNCH_CHECK("sum_partials_kernel");
    } else {
        if (r.bwd.gW2) hipLaunchKernelGGL(zero_kernel, dim3((H2 * H1 + 255) / 256), dim3(256), 0, st, r.bwd.gW2, (int64_t)H2 * H1);
        if (r.bwd.gb2) hipLaunchKernelGGL(zero_kernel, dim3(1), dim3(256), 0, st, r.bwd.gb2, (int64_t)H2);
        DMET_LAUNCH_CHECK("zero_kernel");
    }
    if (r.bwd.gx) {
        hipLaunchKernelGGL(rows_linear_kernel, dim3((unsigned)((N + 15) / 16)), dim3(256), 0, st, (const float *)p.gpq, N, 2 * H1,
                           (const float *)c.w, (const float *)nullptr, Hin, r.bwd.gx);
        DMET_LAUNCH_CHECK("rows_linear_kernel (gx)");
    }
    return 0;
}

}  // namespace
}  // namespace dmet

using namespace dmet;

// The entry points of the three routes (include/dmet.h has the contract) differ in their name and EdgePrec alone.

extern "C" int dmet_edge_mlp_f32_supported(int Hin, int H1, int H2) { return supported(EdgePrec::f32, Hin, H1, H2); }

extern "C" size_t dmet_edge_mlp_f32_workspace_bytes(int64_t N, int64_t E, int Hin, int H1, int H2)
{
    return workspace_bytes(EdgePrec::f32, N, E, Hin, H1, H2);
}

extern "C" int dmet_edge_mlp_fwd_f32(const float *x, int64_t N, int Hin, const int32_t *rowptr, const int32_t *src,
                                     const int32_t *tgt, int64_t E, const float *W1, const float *b1, int H1, const float *W2,
                                     const float *b2, int H2, int act2, int aggr, int bn, const float *gamma,
                                     const float *beta, float eps, float momentum, float *running_mean, float *running_var,
                                     int64_t *num_batches_tracked, float *out, float *pq, float *agg, int32_t *win,
                                     float *bnstat, void *ws, size_t ws_bytes, dmet_stream_t stream)
{
    EdgeMlp r{"dmet_edge_mlp_fwd_f32", EdgePrec::f32, x, Hin, W1, ws, ws_bytes, stream};
    r.p = pass_args(pq, rowptr, src, tgt, N, E, H1, H2, W2, b2, act2, aggr, bn);
    r.p.agg = agg; r.p.win = win;
    r.fwd = {b1, gamma, beta, eps, momentum, running_mean, running_var, num_batches_tracked, out, pq, bnstat};
    return edge_mlp_fwd(r);
}

extern "C" int dmet_edge_mlp_bwd_f32(const float *x, int64_t N, int Hin, const int32_t *rowptr, const int32_t *src,
                                     const int32_t *tgt, int64_t E, const int32_t *srcptr, const int32_t *srcperm,
                                     const float *W1, int H1, const float *W2, const float *b2, int H2, int act2, int aggr,
                                     int bn, const float *pq, const float *agg, const int32_t *win, const float *bnstat,
                                     const float *g_out, float *gx, float *gpq, float *gW2, float *gb2, float *ggamma,
                                     float *gbeta, void *ws, size_t ws_bytes, dmet_stream_t stream)
{
    EdgeMlp r{"dmet_edge_mlp_bwd_f32", EdgePrec::f32, x, Hin, W1, ws, ws_bytes, stream};
    r.p = pass_args(pq, rowptr, src, tgt, N, E, H1, H2, W2, b2, act2, aggr, bn);
    r.p.srcptr = srcptr; r.p.srcperm = srcperm; r.p.g_out = g_out; r.p.bnstat = bnstat; r.p.cwin = win; r.p.gpq = gpq;
    r.bwd = {agg, gx, gW2, gb2, ggamma, gbeta};
    return edge_mlp_bwd(r);
}

extern "C" int dmet_edge_mlp_bf16_supported(int Hin, int H1, int H2) { return supported(EdgePrec::bf16, Hin, H1, H2); }

extern "C" size_t dmet_edge_mlp_bf16_workspace_bytes(int64_t N, int64_t E, int Hin, int H1, int H2)
{
    return workspace_bytes(EdgePrec::bf16, N, E, Hin, H1, H2);
}

extern "C" int dmet_edge_mlp_fwd_bf16(const float *x, int64_t N, int Hin, const int32_t *rowptr, const int32_t *src,
                                      const int32_t *tgt, int64_t E, const float *W1, const float *b1, int H1, const float *W2,
                                      const float *b2, int H2, int act2, int aggr, int bn, const float *gamma,
                                      const float *beta, float eps, float momentum, float *running_mean, float *running_var,
                                      int64_t *num_batches_tracked, float *out, float *pq, float *agg, int32_t *win,
                                      float *bnstat, void *ws, size_t ws_bytes, dmet_stream_t stream)
{
    EdgeMlp r{"dmet_edge_mlp_fwd_bf16", EdgePrec::bf16, x, Hin, W1, ws, ws_bytes, stream};
    r.p = pass_args(pq, rowptr, src, tgt, N, E, H1, H2, W2, b2, act2, aggr, bn);
    r.p.agg = agg; r.p.win = win;
    r.fwd = {b1, gamma, beta, eps, momentum, running_mean, running_var, num_batches_tracked, out, pq, bnstat};
    return edge_mlp_fwd(r);
}

extern "C" int dmet_edge_mlp_bwd_bf16(const float *x, int64_t N, int Hin, const int32_t *rowptr, const int32_t *src,
                                      const int32_t *tgt, int64_t E, const int32_t *srcptr, const int32_t *srcperm,
                                      const float *W1, int H1, const float *W2, const float *b2, int H2, int act2, int aggr,
                                      int bn, const float *pq, const float *agg, const int32_t *win, const float *bnstat,
                                      const float *g_out, float *gx, float *gpq, float *gW2, float *gb2, float *ggamma,
                                      float *gbeta, void *ws, size_t ws_bytes, dmet_stream_t stream)
{
    EdgeMlp r{"dmet_edge_mlp_bwd_bf16", EdgePrec::bf16, x, Hin, W1, ws, ws_bytes, stream};
    r.p = pass_args(pq, rowptr, src, tgt, N, E, H1, H2, W2, b2, act2, aggr, bn);
    r.p.srcptr = srcptr; r.p.srcperm = srcperm; r.p.g_out = g_out; r.p.bnstat = bnstat; r.p.cwin = win; r.p.gpq = gpq;
    r.bwd = {agg, gx, gW2, gb2, ggamma, gbeta};
    return edge_mlp_bwd(r);
}

extern "C" int dmet_edge_mlp_f16_supported(int Hin, int H1, int H2) { return supported(EdgePrec::f16, Hin, H1, H2); }

extern "C" size_t dmet_edge_mlp_f16_workspace_bytes(int64_t N, int64_t E, int Hin, int H1, int H2)
{
    return workspace_bytes(EdgePrec::f16, N, E, Hin, H1, H2);
}

extern "C" int dmet_edge_mlp_fwd_f16(const float *x, int64_t N, int Hin, const int32_t *rowptr, const int32_t *src,
                                     const int32_t *tgt, int64_t E, const float *W1, const float *b1, int H1, const float *W2,
                                     const float *b2, int H2, int act2, int aggr, int bn, const float *gamma,
                                     const float *beta, float eps, float momentum, float *running_mean, float *running_var,
                                     int64_t *num_batches_tracked, float *out, float *pq, float *agg, int32_t *win,
                                     float *bnstat, void *ws, size_t ws_bytes, dmet_stream_t stream)
{
    EdgeMlp r{"dmet_edge_mlp_fwd_f16", EdgePrec::f16, x, Hin, W1, ws, ws_bytes, stream};
    r.p = pass_args(pq, rowptr, src, tgt, N, E, H1, H2, W2, b2, act2, aggr, bn);
    r.p.agg = agg; r.p.win = win;
    r.fwd = {b1, gamma, beta, eps, momentum, running_mean, running_var, num_batches_tracked, out, pq, bnstat};
    return edge_mlp_fwd(r);
}

extern "C" int dmet_edge_mlp_bwd_f16(const float *x, int64_t N, int Hin, const int32_t *rowptr, const int32_t *src,
                                     const int32_t *tgt, int64_t E, const int32_t *srcptr, const int32_t *srcperm,
                                     const float *W1, int H1, const float *W2, const float *b2, int H2, int act2, int aggr,
                                     int bn, const float *pq, const float *agg, const int32_t *win, const float *bnstat,
                                     const float *g_out, float *gx, float *gpq, float *gW2, float *gb2, float *ggamma,
                                     float *gbeta, void *ws, size_t ws_bytes, dmet_stream_t stream)
{
    EdgeMlp r{"dmet_edge_mlp_bwd_f16", EdgePrec::f16, x, Hin, W1, ws, ws_bytes, stream};
    r.p = pass_args(pq, rowptr, src, tgt, N, E, H1, H2, W2, b2, act2, aggr, bn);
    r.p.srcptr = srcptr; r.p.srcperm = srcperm; r.p.g_out = g_out; r.p.bnstat = bnstat; r.p.cwin = win; r.p.gpq = gpq;
    r.bwd = {agg, gx, gW2, gb2, ggamma, gbeta};
    return edge_mlp_bwd(r);
}

// edgeconv_sum.hip -- EdgeConv with nn = Linear(2 Hin -> Hout) and aggr in {'add', 'sum', 'mean'}, over any graph.
//
// The message W.[x_i || x_j - x_i] + b splits exactly into P_i + Q_j with P = x (W1-W2)^T + b, Q = x W2^T
// (dmet_node_linear_split_f32).  With deg_i the number of valid in-edges of node i:
//   add / sum: out_i = deg_i P_i + sum_j Q_j        mean: out_i = P_i + (sum_j Q_j) / deg_i        deg_i = 0: out_i = 0 (R3)
// so the layer reads one Q row per edge instead of forming the [E, 2 Hin] edge features and the [E, Hout] messages.
// Backward: gP_i = deg_i g_i (add) or [deg_i > 0] g_i (mean), gQ_j = sum over the edges j -> i of s_i g_i (s_i = 1 or
// 1 / deg_i), walked through a by-source index in ascending order: no float atomics, the same bits on every run.
#include "common.h"

namespace dmet {
namespace {

constexpr int kSumInFlight = 8;     // row gathers in flight per lane
// widest counted table: radius_table(loop=False) searches max_num_neighbors + 1 = 256 slots for the usual 255
constexpr int kSumMaxCountedK = 1024;

// Forward, L2-gather form: H/4 lanes per node, each lane owns 4 channels and gathers 16 bytes of every source's Q row,
// kSumInFlight rows at a time.  Sources in ascending slot (table) or edge (CSR) order; a skipped slot adds -0.0f, the
// exact identity of IEEE addition, so a table and the by-target edge list of the same graph give identical bits.
//   CSR = false: ids = nbr[N, k], the first min(k, cnt[i]) slots of row i (cnt may be NULL), -1 = no neighbour.
//   CSR = true:  ids = src[E], row i = src[rowptr[i] .. rowptr[i+1]-1].
template <int H, bool CSR>
__global__ __launch_bounds__(256) void gather_sum_kernel(const float *__restrict__ P, const float *__restrict__ Q,
                                                          const int32_t *__restrict__ ids,
                                                          const int32_t *__restrict__ cnt_or_rowptr, int64_t N, int k,
                                                          int mean, float *__restrict__ out, int32_t *__restrict__ deg)
{
    constexpr int LPN = H / 4;               // lanes per node
    constexpr int NPB = 256 / LPN;           // nodes per block
    const int bid = xcd_swizzle(blockIdx.x, gridDim.x);
    const int64_t node = (int64_t)bid * NPB + threadIdx.x / LPN;
    const int c4 = threadIdx.x % LPN;
    if (node >= N) return;
    const int32_t *row;
    int n;
    if (CSR) {
        const int lo = cnt_or_rowptr[node];
        row = ids + lo;
        n = cnt_or_rowptr[node + 1] - lo;
    } else {
        row = ids + node * k;
        n = cnt_or_rowptr ? min(k, max(cnt_or_rowptr[node], 0)) : k;
    }
    const float4 *Q4 = reinterpret_cast<const float4 *>(Q);
    const float nz = -0.0f;
    float4 acc = make_float4(nz, nz, nz, nz);
    int d = 0;
    for (int s0 = 0; s0 < n; s0 += kSumInFlight) {
        int32_t j[kSumInFlight];
        float4 v[kSumInFlight];
#pragma unroll
        for (int u = 0; u < kSumInFlight; ++u) j[u] = (s0 + u < n) ? row[s0 + u] : -1;
#pragma unroll
        for (int u = 0; u < kSumInFlight; ++u)
            v[u] = (j[u] >= 0) ? Q4[(int64_t)j[u] * LPN + c4] : make_float4(nz, nz, nz, nz);
#pragma unroll
        for (int u = 0; u < kSumInFlight; ++u) {
            d += (j[u] >= 0);
            acc.x += v[u].x;
            acc.y += v[u].y;
            acc.z += v[u].z;
            acc.w += v[u].w;
        }
    }
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    if (d > 0) {
        const float4 p = reinterpret_cast<const float4 *>(P)[node * LPN + c4];
        const float fd = (float)d;
        if (mean)
            o = make_float4(p.x + acc.x / fd, p.y + acc.y / fd, p.z + acc.z / fd, p.w + acc.w / fd);
        else
            o = make_float4(fd * p.x + acc.x, fd * p.y + acc.y, fd * p.z + acc.z, fd * p.w + acc.w);
    }
    reinterpret_cast<float4 *>(out)[node * LPN + c4] = o;
    if (c4 == 0) deg[node] = d;
}

// Backward: per node j, gP_j (row scale of g_j) and gQ_j = sum over the by-source entries t of j, ascending, of
// s_i g_i with i the entry's target: rev_idx[t] / k for a table (rev_idx = table positions i*k+s), tgt[rev_idx[t]] for
// a CSR list (rev_idx = edge positions).  Same lane layout and gathers in flight as the forward.
template <int H, bool CSR>
__global__ __launch_bounds__(256) void gather_sum_bwd_kernel(const float *__restrict__ g_out,
                                                              const int32_t *__restrict__ deg,
                                                              const int32_t *__restrict__ rev_ptr,
                                                              const int32_t *__restrict__ rev_idx,
                                                              const int32_t *__restrict__ tgt, int64_t N, int k,
                                                              int mean, float *__restrict__ gP, float *__restrict__ gQ)
{
    constexpr int LPN = H / 4;
    constexpr int NPB = 256 / LPN;
    const int bid = xcd_swizzle(blockIdx.x, gridDim.x);
    const int64_t node = (int64_t)bid * NPB + threadIdx.x / LPN;
    const int c4 = threadIdx.x % LPN;
    if (node >= N) return;
    const float4 *G4 = reinterpret_cast<const float4 *>(g_out);
    const int dn = deg[node];
    const float4 g = G4[node * LPN + c4];
    float4 gp = make_float4(0.f, 0.f, 0.f, 0.f);      // a node without in-edges produced 0: nothing reaches its P
    if (dn > 0) {
        const float fd = mean ? 1.0f : (float)dn;
        gp = make_float4(fd * g.x, fd * g.y, fd * g.z, fd * g.w);
    }
    reinterpret_cast<float4 *>(gP)[node * LPN + c4] = gp;

    const int lo = rev_ptr[node], hi = rev_ptr[node + 1];
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int t0 = lo; t0 < hi; t0 += kSumInFlight) {
        int32_t i[kSumInFlight];
        float4 v[kSumInFlight];
#pragma unroll
        for (int u = 0; u < kSumInFlight; ++u) {
            const int t = t0 + u;
            i[u] = -1;
            if (t < hi) i[u] = CSR ? tgt[rev_idx[t]] : rev_idx[t] / k;
        }
#pragma unroll
        for (int u = 0; u < kSumInFlight; ++u) {
            v[u] = (i[u] >= 0) ? G4[(int64_t)i[u] * LPN + c4] : make_float4(0.f, 0.f, 0.f, 0.f);
            if (mean && i[u] >= 0) {
                const float s = 1.0f / (float)deg[i[u]];   // >= 1: node i has this in-edge
                v[u] = make_float4(s * v[u].x, s * v[u].y, s * v[u].z, s * v[u].w);
            }
        }
#pragma unroll
        for (int u = 0; u < kSumInFlight; ++u) {
            acc.x += v[u].x;
            acc.y += v[u].y;
            acc.z += v[u].z;
            acc.w += v[u].w;
        }
    }
    reinterpret_cast<float4 *>(gQ)[node * LPN + c4] = acc;
}

template <int H>
int launch_gather_sum(const float *P, const float *Q, const int32_t *ids, const int32_t *aux, int64_t N, int k, int mean,
                      bool csr, float *out, int32_t *deg, hipStream_t st)
{
    constexpr int NPB = 256 / (H / 4);
    const int64_t blocks = (N + NPB - 1) / NPB;
    if (csr)
        hipLaunchKernelGGL((gather_sum_kernel<H, true>), dim3((unsigned)blocks), dim3(256), 0, st, P, Q, ids, aux, N, k,
                           mean, out, deg);
    else
        hipLaunchKernelGGL((gather_sum_kernel<H, false>), dim3((unsigned)blocks), dim3(256), 0, st, P, Q, ids, aux, N,
                           k, mean, out, deg);
    DMET_LAUNCH_CHECK("gather_sum_kernel");
    return 0;
}

template <int H>
int launch_gather_sum_bwd(const float *g_out, const int32_t *deg, const int32_t *rev_ptr, const int32_t *rev_idx,
                          const int32_t *tgt, int64_t N, int k, int mean, float *gP, float *gQ, hipStream_t st)
{
    constexpr int NPB = 256 / (H / 4);
    const int64_t blocks = (N + NPB - 1) / NPB;
    if (k == 0)
        hipLaunchKernelGGL((gather_sum_bwd_kernel<H, true>), dim3((unsigned)blocks), dim3(256), 0, st, g_out, deg,
                           rev_ptr, rev_idx, tgt, N, k, mean, gP, gQ);
    else
        hipLaunchKernelGGL((gather_sum_bwd_kernel<H, false>), dim3((unsigned)blocks), dim3(256), 0, st, g_out, deg,
                           rev_ptr, rev_idx, tgt, N, k, mean, gP, gQ);
    DMET_LAUNCH_CHECK("gather_sum_bwd_kernel");
    return 0;
}

}  // namespace
}  // namespace dmet

using namespace dmet;

extern "C" int dmet_gather_sum_table_f32(const float *P, const float *Q, const int32_t *nbr, const int32_t *cnt,
                                         int64_t N, int k, int H, int mean, float *out, int32_t *deg,
                                         dmet_stream_t stream)
{
    DMET_REQUIRE(N >= 0 && N < (int64_t)2147483647, "dmet_gather_sum_table_f32: N=%lld out of range", (long long)N);
    DMET_REQUIRE(k >= 1 && k <= (cnt ? kSumMaxCountedK : DMET_MAX_K),
                 "dmet_gather_sum_table_f32: k=%d not in [1,%d] (%s table)", k, cnt ? kSumMaxCountedK : DMET_MAX_K,
                 cnt ? "counted" : "fixed-width");
    DMET_REQUIRE(H == 32 || H == 64, "dmet_gather_sum_table_f32: unsupported H=%d (32/64)", H);
    DMET_REQUIRE(mean == 0 || mean == 1, "dmet_gather_sum_table_f32: mean=%d must be 0 or 1", mean);
    DMET_REQUIRE(N * (int64_t)k < (int64_t)2147483647, "dmet_gather_sum_table_f32: N*k out of range");
    if (N == 0) return 0;
    DMET_REQUIRE(P && Q && nbr && out && deg, "dmet_gather_sum_table_f32: null pointer");
    DMET_REQUIRE(aligned16(P) && aligned16(Q) && aligned16(out), "dmet_gather_sum_table_f32: P, Q, out must be 16-B aligned");
    hipStream_t st = as_stream(stream);
    return H == 32 ? launch_gather_sum<32>(P, Q, nbr, cnt, N, k, mean, false, out, deg, st)
                   : launch_gather_sum<64>(P, Q, nbr, cnt, N, k, mean, false, out, deg, st);
}

extern "C" int dmet_gather_sum_csr_f32(const float *P, const float *Q, const int32_t *rowptr, const int32_t *src,
                                       int64_t N, int H, int mean, float *out, int32_t *deg, dmet_stream_t stream)
{
    DMET_REQUIRE(N >= 0 && N < (int64_t)2147483647, "dmet_gather_sum_csr_f32: N=%lld out of range", (long long)N);
    DMET_REQUIRE(H == 32 || H == 64, "dmet_gather_sum_csr_f32: unsupported H=%d (32/64)", H);
    DMET_REQUIRE(mean == 0 || mean == 1, "dmet_gather_sum_csr_f32: mean=%d must be 0 or 1", mean);
    if (N == 0) return 0;
    // src may be NULL for a list without edges (a zero-size tensor): it is read only inside non-empty rows
    DMET_REQUIRE(P && Q && rowptr && out && deg, "dmet_gather_sum_csr_f32: null pointer");
    DMET_REQUIRE(aligned16(P) && aligned16(Q) && aligned16(out), "dmet_gather_sum_csr_f32: P, Q, out must be 16-B aligned");
    hipStream_t st = as_stream(stream);
    return H == 32 ? launch_gather_sum<32>(P, Q, src, rowptr, N, 0, mean, true, out, deg, st)
                   : launch_gather_sum<64>(P, Q, src, rowptr, N, 0, mean, true, out, deg, st);
}

extern "C" int dmet_gather_sum_bwd_f32(const float *g_out, const int32_t *deg, const int32_t *rev_ptr,
                                       const int32_t *rev_idx, const int32_t *tgt, int64_t N, int k, int H, int mean,
                                       float *gP, float *gQ, dmet_stream_t stream)
{
    DMET_REQUIRE(N >= 0 && N < (int64_t)2147483647, "dmet_gather_sum_bwd_f32: N=%lld out of range", (long long)N);
    DMET_REQUIRE(k >= 0 && k <= kSumMaxCountedK, "dmet_gather_sum_bwd_f32: k=%d not in [0,%d] (0 = CSR form)", k,
                 kSumMaxCountedK);
    DMET_REQUIRE(H == 32 || H == 64, "dmet_gather_sum_bwd_f32: unsupported H=%d (32/64)", H);
    DMET_REQUIRE(mean == 0 || mean == 1, "dmet_gather_sum_bwd_f32: mean=%d must be 0 or 1", mean);
    if (N == 0) return 0;
    DMET_REQUIRE(g_out && deg && rev_ptr && rev_idx && gP && gQ, "dmet_gather_sum_bwd_f32: null pointer");
    DMET_REQUIRE(aligned16(g_out) && aligned16(gP) && aligned16(gQ),
                 "dmet_gather_sum_bwd_f32: g_out, gP, gQ must be 16-B aligned");
    hipStream_t st = as_stream(stream);
    return H == 32 ? launch_gather_sum_bwd<32>(g_out, deg, rev_ptr, rev_idx, tgt, N, k, mean, gP, gQ, st)
                   : launch_gather_sum_bwd<64>(g_out, deg, rev_ptr, rev_idx, tgt, N, k, mean, gP, gQ, st);
}

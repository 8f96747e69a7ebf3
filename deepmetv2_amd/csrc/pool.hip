// pool.hip -- graclus matching, normalized-cut edge weights and pair pooling (the DynamicReductionNetwork's coarsening,
// model/dynamic_reduction_network.py:89-92,97-99).  Semantics: include/dmet.h, section "Graph coarsening".
#include "event_wg.h"

namespace dmet {
namespace {

constexpr int kGraclusThreads = 1024;
constexpr int kPoolThreads = 256;

__device__ __forceinline__ uint32_t lowbias32(uint32_t x)
{
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

__device__ __forceinline__ bool is_red(int64_t u, uint32_t rkey) { return (lowbias32((uint32_t)u ^ rkey) >> 31) != 0u; }

// Node state of one event (local indices i = u - lo):
//   st[i]: -1 unmatched, i singleton, else the local index of the partner
//   pr[i]: proposal of the round: -3 matched before the round, -2 no unmatched neighbour (becomes a singleton),
//          -1 nothing proposed, >= 0 the local index of the red node a blue node proposes to
constexpr int kMatched = -3, kLonely = -2, kNone = -1;

// The best candidate of row u: scan in CSR order, take the first candidate, replace it only by a strictly greater
// weight.  Candidates: local j != u inside the event with pred(j).
template <typename Pred>
__device__ __forceinline__ int best_in_row(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                           const float *__restrict__ weight, int64_t u, int64_t lo, int64_t n,
                                           Pred pred)
{
    int best = -1;
    float bw = 0.0f;
    const int64_t e1 = rowptr[u + 1];
    for (int64_t e = rowptr[u]; e < e1; ++e) {
        const int64_t j = (int64_t)col[e] - lo;
        if (j < 0 || j >= n || j + lo == u || !pred((int)j)) continue;
        if (best < 0) {
            best = (int)j;
            if (weight) bw = weight[e];
            if (!weight) break;             // unweighted: the first candidate
        } else if (weight[e] > bw) {
            best = (int)j;
            bw = weight[e];
        }
    }
    return best;
}

// One workgroup per block of nodes (an event): all rounds in one launch, state in LDS for blocks of up to
// DMET_GRACLUS_LDS_NODES nodes, in the caller's workspace above.  Every round has two phases separated by workgroup
// barriers; phase A only reads st and writes pr, phase B only reads pr and writes st (every entry by one lane), so the
// result does not depend on the order lanes run in.
__global__ __launch_bounds__(kGraclusThreads) void graclus_kernel(
    const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col, const float *__restrict__ weight,
    const int64_t *__restrict__ ptr, uint32_t skey, int max_rounds, int32_t *__restrict__ ws,
    int64_t *__restrict__ cluster, int32_t *__restrict__ partner, int32_t *__restrict__ rounds, int64_t N)
{
    __shared__ int32_t lds[2 * DMET_GRACLUS_LDS_NODES];
    const int b = blockIdx.x;
    const int64_t lo = ptr[b], n = ptr[b + 1] - lo;
    const int tid = threadIdx.x;
    if (n <= 0) {
        if (rounds && tid == 0) rounds[b] = 0;
        return;
    }
    int32_t *st = lds, *pr = lds + DMET_GRACLUS_LDS_NODES;
    if (n > DMET_GRACLUS_LDS_NODES) {
        st = ws + lo;
        pr = ws + N + lo;
    }
    for (int64_t i = tid; i < n; i += kGraclusThreads) st[i] = -1;
    __syncthreads();

    int r = 0;
    for (; r < max_rounds; ++r) {
        const uint32_t rkey = lowbias32(skey + 0x9E3779B9u * (uint32_t)r);
        int any = 0;
        // phase A: blue unmatched nodes propose to their best unmatched red neighbour; every unmatched node notes
        // whether it has an unmatched neighbour at all
        for (int64_t i = tid; i < n; i += kGraclusThreads) {
            int p = kMatched;
            if (st[i] < 0) {
                any = 1;
                const int64_t u = lo + i;
                const bool red = is_red(u, rkey);
                const int has = best_in_row(rowptr, col, nullptr, u, lo, n, [&](int j) { return st[j] < 0; });
                if (has < 0) {
                    p = kLonely;
                } else if (red) {
                    p = kNone;
                } else {
                    const int v = best_in_row(rowptr, col, weight, u, lo, n,
                                              [&](int j) { return st[j] < 0 && is_red(lo + j, rkey); });
                    p = v >= 0 ? v : kNone;
                }
            }
            pr[i] = p;
        }
        if (!__syncthreads_or(any)) break;
        // phase B: a red unmatched node accepts its best proposer; lonely nodes become singletons
        for (int64_t i = tid; i < n; i += kGraclusThreads) {
            const int p = pr[i];
            if (p == kLonely) {
                st[i] = (int32_t)i;
            } else if (p == kNone && is_red(lo + i, rkey)) {
                const int w = best_in_row(rowptr, col, weight, lo + i, lo, n, [&](int j) { return pr[j] == (int)i; });
                if (w >= 0) {
                    st[i] = w;
                    st[w] = (int32_t)i;
                }
            }
        }
        __syncthreads();
    }
    if (r == max_rounds) {
        // finisher: the nodes still unmatched in ascending order, each with its best unmatched neighbour
        if (tid == 0) {
            for (int64_t i = 0; i < n; ++i) {
                if (st[i] >= 0) continue;
                const int w = best_in_row(rowptr, col, weight, lo + i, lo, n, [&](int j) { return st[j] < 0; });
                if (w >= 0) {
                    st[i] = w;
                    st[w] = (int32_t)i;
                } else {
                    st[i] = (int32_t)i;
                }
            }
        }
        __syncthreads();
    }
    if (rounds && tid == 0) rounds[b] = r;
    for (int64_t i = tid; i < n; i += kGraclusThreads) {
        const int64_t s = st[i];
        cluster[lo + i] = lo + (s < i ? s : i);
        partner[lo + i] = s == i ? -1 : (int32_t)(lo + s);
    }
}

// ---- normalized cut ----------------------------------------------------------------------------------------------------
__global__ void in_degree_kernel(const int64_t *__restrict__ col, int64_t E, int64_t N, int32_t *__restrict__ deg)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const int64_t c = col[e];
    if (c >= 0 && c < N) atomicAdd(&deg[c], 1);
}

// w_e = attr_e * (1/deg(row_e) + 1/deg(col_e)); attr from `attr` or, when x is given, ||x[row_e] - x[col_e]||_2
// (squares summed in double in ascending channel order, one rounding to fp32).  Out-of-range endpoints give NaN.
__global__ void normalized_cut_kernel(const int64_t *__restrict__ row, const int64_t *__restrict__ col, int64_t E,
                                      int64_t N, const float *__restrict__ attr, const float *__restrict__ x, int D,
                                      const int32_t *__restrict__ deg, float *__restrict__ w)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const int64_t r = row[e], c = col[e];
    if (r < 0 || r >= N || c < 0 || c >= N) {
        w[e] = __builtin_nanf("");
        return;
    }
    float a;
    if (x) {
        double acc = 0.0;
        for (int d = 0; d < D; ++d) {
            const double t = (double)x[r * D + d] - (double)x[c * D + d];
            acc += t * t;
        }
        a = (float)sqrt(acc);
    } else {
        a = attr[e];
    }
    const float ir = 1.0f / (float)deg[r], ic = 1.0f / (float)deg[c];
    w[e] = a * (ir + ic);
}

// ---- pair pooling ----------------------------------------------------------------------------------------------------
// A node leads its cluster unless its partner is a valid lower index.
__device__ __forceinline__ int64_t leader_of(const int32_t *__restrict__ partner, int64_t u, int64_t N)
{
    const int64_t p = partner[u];
    return (p >= 0 && p < u && p < N) ? p : u;
}

// One workgroup per event: rank[u] = position of leader u among the leaders of its event, cnt[b] = their number.
__global__ __launch_bounds__(kPoolThreads) void leader_rank_kernel(const int32_t *__restrict__ partner,
                                                                  const int64_t *__restrict__ ptr, int64_t N,
                                                                  int32_t *__restrict__ rank, int32_t *__restrict__ cnt)
{
    __shared__ int wsum[kPoolThreads / kWave];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int64_t lo = ptr[b], hi = ptr[b + 1];
    int base = 0;
    for (int64_t c0 = lo; c0 < hi; c0 += kPoolThreads) {
        const int64_t u = c0 + tid;
        const bool lead = u < hi && leader_of(partner, u, N) == u;
        int before, total;
        wg_rank<kPoolThreads / kWave>(lead, wsum, before, total);
        if (lead) rank[u] = base + before;
        base += total;
        __syncthreads();
    }
    if (tid == 0) cnt[b] = base;
}

// One workgroup: pooled_ptr = exclusive prefix sum of cnt (B+1 entries).
__global__ __launch_bounds__(kPoolThreads) void count_scan_kernel(const int32_t *__restrict__ cnt, int B,
                                                                 int64_t *__restrict__ pooled_ptr)
{
    __shared__ int64_t part[kPoolThreads];
    const int tid = threadIdx.x;
    int64_t base = 0;
    if (tid == 0) pooled_ptr[0] = 0;
    for (int c0 = 0; c0 < B; c0 += kPoolThreads) {
        const int b = c0 + tid;
        part[tid] = b < B ? cnt[b] : 0;
        __syncthreads();
        for (int off = 1; off < kPoolThreads; off <<= 1) {     // inclusive Hillis-Steele scan
            const int64_t v = tid >= off ? part[tid - off] : 0;
            __syncthreads();
            part[tid] += v;
            __syncthreads();
        }
        if (b < B) pooled_ptr[b + 1] = base + part[tid];
        base += part[kPoolThreads - 1];
        __syncthreads();
    }
}

__global__ void cluster_id_kernel(const int32_t *__restrict__ partner, const int64_t *__restrict__ ptr, int B,
                                  int64_t N, const int32_t *__restrict__ rank, const int64_t *__restrict__ pooled_ptr,
                                  int64_t *__restrict__ cid)
{
    const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= N) return;
    const int64_t l = leader_of(partner, u, N);
    cid[u] = pooled_ptr[find_event(ptr, B, l)] + rank[l];
}

// Thread (leader u, channel f): the cluster row cid[u] from u and its partner.  Max ties go to u (the lower index).
__global__ void pool_pairs_kernel(const float *__restrict__ x, int64_t N, int F, const int32_t *__restrict__ partner,
                                  const int64_t *__restrict__ cid, const int64_t *__restrict__ ptr, int B, int64_t C,
                                  float *__restrict__ out_max, int32_t *__restrict__ arg, float *__restrict__ out_mean,
                                  int64_t *__restrict__ pooled_batch)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= N * F) return;
    const int64_t u = t / F;
    const int f = (int)(t - u * F);
    if (leader_of(partner, u, N) != u) return;
    const int64_t c = cid[u];
    if (c < 0 || c >= C) return;
    const int64_t p = partner[u];
    const bool pair = p > u && p < N;
    const float xu = x[u * F + f];
    float mx = xu, mean = xu;
    int32_t a = (int32_t)u;
    if (pair) {
        const float xv = x[p * F + f];
        if (xv > xu) {
            mx = xv;
            a = (int32_t)p;
        }
        mean = (xu + xv) * 0.5f;
    }
    if (out_max) out_max[c * F + f] = mx;
    if (arg) arg[c * F + f] = a;
    if (out_mean) out_mean[c * F + f] = mean;
    if (pooled_batch && f == 0) pooled_batch[c] = find_event(ptr, B, u);
}

__global__ void pool_pairs_bwd_kernel(const float *__restrict__ g_max, const int32_t *__restrict__ arg,
                                      const float *__restrict__ g_mean, const int32_t *__restrict__ partner,
                                      const int64_t *__restrict__ cid, int64_t N, int F, int64_t C, float *__restrict__ gx)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= N * F) return;
    const int64_t u = t / F;
    const int f = (int)(t - u * F);
    const int64_t c = cid[u];
    float g = 0.0f;
    if (c >= 0 && c < C) {
        if (g_max && arg[c * F + f] == (int32_t)u) g = g_max[c * F + f];
        if (g_mean) {
            const int64_t p = partner[u];
            const bool pair = p >= 0 && p < N && p != u;
            g += pair ? g_mean[c * F + f] * 0.5f : g_mean[c * F + f];
        }
    }
    gx[t] = g;
}

inline unsigned blocks_for(int64_t n, int t) { return (unsigned)((n + t - 1) / t); }

}  // namespace
}  // namespace dmet

using namespace dmet;

extern "C" size_t dmet_graclus_workspace_bytes(int64_t N)
{
    return N > 0 ? (size_t)(2 * N) * sizeof(int32_t) : 0;
}

extern "C" int dmet_graclus_f32(const int64_t *rowptr, const int32_t *col, const float *weight, const int64_t *ptr,
                                int B, int64_t N, uint64_t seed, int max_rounds, int64_t *cluster, int32_t *partner,
                                int32_t *rounds, void *ws, size_t ws_bytes, dmet_stream_t stream)
{
    DMET_REQUIRE(N >= 0 && B >= 0 && N <= INT32_MAX, "dmet_graclus_f32: bad sizes N=%lld B=%d", (long long)N, B);
    DMET_REQUIRE(max_rounds >= 0, "dmet_graclus_f32: max_rounds=%d < 0", max_rounds);
    if (N == 0 || B == 0) return 0;
    DMET_REQUIRE(rowptr && col && ptr && cluster && partner && ws, "dmet_graclus_f32: null pointer");
    DMET_REQUIRE(ws_bytes >= dmet_graclus_workspace_bytes(N), "dmet_graclus_f32: workspace too small");
    const uint32_t skey = (uint32_t)seed ^ (uint32_t)(seed >> 32);
    hipLaunchKernelGGL(graclus_kernel, dim3((unsigned)B), dim3(kGraclusThreads), 0, as_stream(stream), rowptr, col,
                       weight, ptr, skey, max_rounds == 0 ? DMET_GRACLUS_DEFAULT_ROUNDS : max_rounds,
                       (int32_t *)ws, cluster, partner, rounds, N);
    DMET_LAUNCH_CHECK("graclus_kernel");
    return 0;
}

extern "C" size_t dmet_normalized_cut_workspace_bytes(int64_t N)
{
    return N > 0 ? (size_t)N * sizeof(int32_t) : 0;
}

static int normalized_cut(const char *who, const int64_t *row, const int64_t *col, int64_t E, int64_t N,
                          const float *attr, const float *x, bool fused, int D, float *w, void *ws, size_t ws_bytes,
                          dmet_stream_t stream)
{
    DMET_REQUIRE(E >= 0 && N >= 0, "%s: bad sizes E=%lld N=%lld", who, (long long)E, (long long)N);
    DMET_REQUIRE(!fused || (D >= 1 && D <= DMET_MAX_CUT_DIM), "%s: D=%d outside 1..%d", who, D, DMET_MAX_CUT_DIM);
    if (E == 0) return 0;
    DMET_REQUIRE(N > 0, "%s: E=%lld edges on N=0 nodes", who, (long long)E);
    DMET_REQUIRE(row && col && (fused ? x != nullptr : attr != nullptr) && w && ws, "%s: null pointer", who);
    DMET_REQUIRE(ws_bytes >= dmet_normalized_cut_workspace_bytes(N), "%s: workspace too small", who);
    int32_t *deg = (int32_t *)ws;
    hipError_t e = hipMemsetAsync(deg, 0, (size_t)N * sizeof(int32_t), as_stream(stream));
    if (e != hipSuccess) return hip_fail(e, who);
    hipLaunchKernelGGL(in_degree_kernel, dim3(blocks_for(E, 256)), dim3(256), 0, as_stream(stream), col, E, N, deg);
    DMET_LAUNCH_CHECK("in_degree_kernel");
    hipLaunchKernelGGL(normalized_cut_kernel, dim3(blocks_for(E, 256)), dim3(256), 0, as_stream(stream), row, col, E, N,
                       attr, fused ? x : nullptr, D, deg, w);
    DMET_LAUNCH_CHECK("normalized_cut_kernel");
    return 0;
}

extern "C" int dmet_normalized_cut_f32(const int64_t *row, const int64_t *col, int64_t E, int64_t N, const float *attr,
                                       float *w, void *ws, size_t ws_bytes, dmet_stream_t stream)
{
    return normalized_cut("dmet_normalized_cut_f32", row, col, E, N, attr, nullptr, false, 0, w, ws, ws_bytes, stream);
}

extern "C" int dmet_normalized_cut_2d_f32(const int64_t *row, const int64_t *col, int64_t E, int64_t N, const float *x,
                                          int D, float *w, void *ws, size_t ws_bytes, dmet_stream_t stream)
{
    return normalized_cut("dmet_normalized_cut_2d_f32", row, col, E, N, nullptr, x, true, D, w, ws, ws_bytes, stream);
}

extern "C" size_t dmet_pool_pairs_workspace_bytes(int64_t N, int B)
{
    if (N <= 0 || B <= 0) return 0;
    return (size_t)(N + B) * sizeof(int32_t);
}

extern "C" int dmet_pool_pairs_index(const int32_t *partner, const int64_t *ptr, int B, int64_t N, int64_t *cid,
                                     int64_t *pooled_ptr, void *ws, size_t ws_bytes, dmet_stream_t stream)
{
    DMET_REQUIRE(N >= 0 && B >= 0 && N <= INT32_MAX, "dmet_pool_pairs_index: bad sizes N=%lld B=%d", (long long)N, B);
    DMET_REQUIRE(B > 0 || N == 0, "dmet_pool_pairs_index: N=%lld nodes in B=0 events", (long long)N);
    if (B == 0) return 0;
    DMET_REQUIRE(ptr && pooled_ptr && (N == 0 || (partner && cid && ws)), "dmet_pool_pairs_index: null pointer");
    DMET_REQUIRE(ws_bytes >= dmet_pool_pairs_workspace_bytes(N, B), "dmet_pool_pairs_index: workspace too small");
    int32_t *rank = (int32_t *)ws, *cnt = rank + N;
    hipLaunchKernelGGL(leader_rank_kernel, dim3((unsigned)B), dim3(kPoolThreads), 0, as_stream(stream), partner, ptr, N,
                       rank, cnt);
    DMET_LAUNCH_CHECK("leader_rank_kernel");
    hipLaunchKernelGGL(count_scan_kernel, dim3(1), dim3(kPoolThreads), 0, as_stream(stream), cnt, B, pooled_ptr);
    DMET_LAUNCH_CHECK("count_scan_kernel");
    if (N == 0) return 0;
    hipLaunchKernelGGL(cluster_id_kernel, dim3(blocks_for(N, 256)), dim3(256), 0, as_stream(stream), partner, ptr, B, N,
                       rank, pooled_ptr, cid);
    DMET_LAUNCH_CHECK("cluster_id_kernel");
    return 0;
}

extern "C" int dmet_pool_pairs_f32(const float *x, int64_t N, int F, const int32_t *partner, const int64_t *cid,
                                   const int64_t *ptr, int B, int64_t C, float *out_max, int32_t *arg, float *out_mean,
                                   int64_t *pooled_batch, dmet_stream_t stream)
{
    DMET_REQUIRE(N >= 0 && F >= 1 && C >= 0 && C <= N && B >= 0 && N <= INT32_MAX,
                 "dmet_pool_pairs_f32: bad sizes N=%lld F=%d C=%lld B=%d", (long long)N, F, (long long)C, B);
    DMET_REQUIRE(!pooled_batch || B > 0 || N == 0, "dmet_pool_pairs_f32: pooled_batch needs B > 0");
    if (N == 0) return 0;
    DMET_REQUIRE(x && partner && cid && (!pooled_batch || ptr), "dmet_pool_pairs_f32: null pointer");
    DMET_REQUIRE(!out_max == !arg, "dmet_pool_pairs_f32: out_max and arg go together");
    hipLaunchKernelGGL(pool_pairs_kernel, dim3(blocks_for(N * F, 256)), dim3(256), 0, as_stream(stream), x, N, F,
                       partner, cid, ptr, B, C, out_max, arg, out_mean, pooled_batch);
    DMET_LAUNCH_CHECK("pool_pairs_kernel");
    return 0;
}

extern "C" int dmet_pool_pairs_bwd_f32(const float *g_max, const int32_t *arg, const float *g_mean,
                                       const int32_t *partner, const int64_t *cid, int64_t N, int F, int64_t C,
                                       float *gx, dmet_stream_t stream)
{
    DMET_REQUIRE(N >= 0 && F >= 1 && C >= 0 && C <= N, "dmet_pool_pairs_bwd_f32: bad sizes N=%lld F=%d C=%lld",
                 (long long)N, F, (long long)C);
    if (N == 0) return 0;
    DMET_REQUIRE(partner && cid && gx && (!g_max || arg), "dmet_pool_pairs_bwd_f32: null pointer");
    hipLaunchKernelGGL(pool_pairs_bwd_kernel, dim3(blocks_for(N * F, 256)), dim3(256), 0, as_stream(stream), g_max, arg,
                       g_mean, partner, cid, N, F, C, gx);
    DMET_LAUNCH_CHECK("pool_pairs_bwd_kernel");
    return 0;
}

// select.hip -- score-based selection pooling (torch_geometric's topk / filter_adj, TopKPooling, SAGPooling,
// SortAggregation).  Semantics: include/dmet.h, section "Selection pooling".
#include "event_wg.h"
#include "score_key.h"

namespace dmet {
namespace {

constexpr int kSelThreads = DMET_SELECT_THREADS;
constexpr int kRowThreads = 256;                    // select_rows / filter_table: four waves, one row or node each
constexpr int kRowWaves = kRowThreads / kWave;
constexpr int kEdgeThreads = DMET_SELECT_EDGE_BLOCK;  // filter_edges: one edge per thread
constexpr int kEdgeWaves = kEdgeThreads / kWave;
static_assert(kEdgeWaves <= kWave, "the wave counts of an edge block are scanned by one wave");

// select_key (score_key.h) with the local index: keys of an event are distinct and > 0, the key of a padding slot.

// Descending bitonic network over key[0 .. P), P a power of two, by the whole workgroup: P / 2 compare-exchanges per
// stage, pair t of a stage with stride j is (i, i | j) with i = t's bits with a 0 inserted at bit log2(j); one barrier
// per stage.  Distinct keys (the padding zeros compare equal to each other only): the result does not depend on the
// network, so LDS and workspace give the same bits.
template <typename idx_t>
__device__ __forceinline__ void bitonic_desc(uint64_t *key, idx_t P)
{
    const idx_t half = P >> 1;
    for (idx_t k = 2; k <= P; k <<= 1) {
        for (idx_t j = k >> 1; j > 0; j >>= 1) {
            for (idx_t t = threadIdx.x; t < half; t += kSelThreads) {
                const idx_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const idx_t l = i | j;
                const uint64_t a = key[i], b = key[l];
                const bool desc = (i & k) == 0;
                if ((a < b) == desc && a != b) {
                    key[i] = b;
                    key[l] = a;
                }
            }
            __syncthreads();
        }
    }
}

template <typename idx_t>
__device__ __forceinline__ void topk_event(uint64_t *key, const float *__restrict__ score, int64_t lo, int64_t n, int64_t o0,
                                           int64_t r, int64_t M, int64_t *__restrict__ perm, int32_t *__restrict__ node_map)
{
    idx_t P = 1;
    while ((int64_t)P < n) P <<= 1;
    for (idx_t i = threadIdx.x; i < P; i += kSelThreads)
        key[i] = (int64_t)i < n ? select_key(score[lo + i], (uint32_t)i) : 0ull;
    __syncthreads();
    bitonic_desc<idx_t>(key, P);
    const int64_t m = r < n ? r : n;
    for (int64_t p = threadIdx.x; p < n; p += kSelThreads) {
        const int64_t i = (int64_t)(uint32_t)~(uint32_t)key[p];      // < n: the n real keys lead the padding
        const bool picked = p < m && o0 + p < M;
        if (picked) perm[o0 + p] = lo + i;
        if (i < n) node_map[lo + i] = picked ? (int32_t)(o0 + p) : -1;
    }
    for (int64_t p = m + threadIdx.x; p < r && o0 + p < M; p += kSelThreads) perm[o0 + p] = -1;
}

// An event of up to DMET_SELECT_LDS_NODES nodes keeps its keys in LDS (128 KiB); a larger one keeps them in the caller's
// workspace at ws[2 lo ..): the power of two above n is < 2 n, so the events' ranges are disjoint.  Nodes no event owns are
// not picked either.
__global__ __launch_bounds__(kSelThreads) void topk_kernel(const float *__restrict__ score, const int64_t *__restrict__ ptr,
                                                           const int64_t *__restrict__ out_ptr, int B, int64_t N, int64_t M,
                                                           int64_t *__restrict__ perm, int32_t *__restrict__ node_map,
                                                           uint64_t *ws)
{
    __shared__ uint64_t lds[DMET_SELECT_LDS_NODES];
    const int b = blockIdx.x;
    const EventRange ev = event_range(ptr, b, N);
    for_unowned<kSelThreads>(ev, b, B, N, [&](int64_t i) { node_map[i] = -1; });
    const int64_t lo = ev.lo, n = ev.n;
    int64_t o0 = out_ptr[b], r = out_ptr[b + 1] - o0;
    if (o0 < 0 || o0 > M) r = 0;
    if (r > M - o0) r = M - o0;
    if (r <= 0 || n <= 0) {                                 // uniform over the workgroup
        for (int64_t i = threadIdx.x; i < n; i += kSelThreads) node_map[lo + i] = -1;
        for (int64_t p = threadIdx.x; p < r; p += kSelThreads) perm[o0 + p] = -1;
        return;
    }
    if (n <= DMET_SELECT_LDS_NODES) topk_event<int>(lds, score, lo, n, o0, r, M, perm, node_map);
    else topk_event<int64_t>(ws + 2 * lo, score, lo, n, o0, r, M, perm, node_map);
}

// out[r, f] = x[perm[r], f] * s[perm[r]]; one thread per element.
template <bool kGate>
__global__ __launch_bounds__(kRowThreads) void select_rows_kernel(const float *__restrict__ x, const float *__restrict__ s,
                                                                  const int64_t *__restrict__ perm, int64_t N, int64_t M, int F,
                                                                  float *__restrict__ out)
{
    const int64_t e = (int64_t)blockIdx.x * kRowThreads + threadIdx.x;
    if (e >= M * F) return;
    const int64_t r = e / F;
    const int f = (int)(e - r * F);
    const int64_t p = perm[r];
    float v = 0.0f;
    if (p >= 0 && p < N) {
        v = x[p * F + f];
        if (kGate) v = v * s[p];
    }
    out[e] = v;
}

// One wave per node: gx[i, f] = g[r, f] * s[i], gs[i] = sum_f g[r, f] * x[i, f] with r = node_map[i]; lane l sums
// f = l, l + 64, ... in that order, then the xor butterfly of wave_sum.
template <bool kGate, bool kGx, bool kGs>
__global__ __launch_bounds__(kRowThreads) void select_rows_bwd_kernel(const float *__restrict__ g, const float *__restrict__ x,
                                                                      const float *__restrict__ s,
                                                                      const int32_t *__restrict__ node_map, int64_t N, int64_t M,
                                                                      int F, float *__restrict__ gx, float *__restrict__ gs)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t i = (int64_t)blockIdx.x * kRowWaves + threadIdx.x / kWave;
    if (i >= N) return;                                     // uniform over the wave
    const int64_t r = node_map[i];
    const bool picked = r >= 0 && r < M;
    float acc = 0.0f;
    const float si = kGate && picked ? s[i] : 1.0f;
    for (int f = lane; f < F; f += kWave) {
        const float gv = picked ? g[r * F + f] : 0.0f;
        if (kGx) gx[i * F + f] = picked ? (kGate ? gv * si : gv) : 0.0f;
        if (kGs && picked) acc += gv * x[i * F + f];
    }
    if (kGs) {
        acc = wave_sum(acc);
        if (lane == 0) gs[i] = picked ? acc : 0.0f;
    }
}

// One wave per output row: the kept entries of row perm[r], relabelled, packed to the left in slot order (a ballot and
// the count of the lanes below per chunk of 64 slots).
__global__ __launch_bounds__(kRowThreads) void filter_table_kernel(const int32_t *__restrict__ nbr, const int32_t *__restrict__ cnt,
                                                                   const int64_t *__restrict__ perm,
                                                                   const int32_t *__restrict__ node_map, int64_t N, int64_t M,
                                                                   int k, int32_t *__restrict__ out_nbr,
                                                                   int32_t *__restrict__ out_cnt)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t r = (int64_t)blockIdx.x * kRowWaves + threadIdx.x / kWave;
    if (r >= M) return;                                     // uniform over the wave
    const int64_t p = perm[r];
    int c = 0;
    if (p >= 0 && p < N) {
        c = k;
        if (cnt) {
            const int cp = cnt[p];
            c = cp < 0 ? 0 : (cp < k ? cp : k);
        }
    }
    int32_t *orow = out_nbr + r * k;
    int base = 0;
    for (int s0 = 0; s0 < c; s0 += kWave) {
        const int slot = s0 + lane;
        int32_t v = -1;
        if (slot < c) {
            const int32_t j = nbr[p * k + slot];
            if (j >= 0 && (int64_t)j < N) v = node_map[j];
        }
        const bool keep = v >= 0;
        const uint64_t mask = __ballot(keep);
        const int below = __popcll(mask & lanes_below(lane));
        if (keep) orow[base + below] = v;
        base += __popcll(mask);
    }
    for (int slot = base + lane; slot < k; slot += kWave) orow[slot] = -1;
    if (lane == 0) out_cnt[r] = base;
}

// 0: an end outside [0, N) (the id is compared before node_map is read); 1: in range, an end not picked; 2: kept.
__device__ __forceinline__ int edge_state(const int64_t *__restrict__ row, const int64_t *__restrict__ col,
                                          const int32_t *__restrict__ node_map, int64_t e, int64_t N, int32_t &a, int32_t &b)
{
    const int64_t u = row[e], v = col[e];
    if (u < 0 || u >= N || v < 0 || v >= N) return 0;
    a = node_map[u];
    b = node_map[v];
    return a >= 0 && b >= 0 ? 2 : 1;
}

// Block counts: kept[blk] = the block's kept edges, bad[blk] = its edges with an out-of-range end.
__global__ __launch_bounds__(kEdgeThreads) void filter_edges_count_kernel(const int64_t *__restrict__ row,
                                                                          const int64_t *__restrict__ col,
                                                                          const int32_t *__restrict__ node_map, int64_t E,
                                                                          int64_t N, int64_t *__restrict__ offs,
                                                                          int32_t *__restrict__ bad)
{
    __shared__ int wk[kEdgeWaves], wb[kEdgeWaves];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int64_t e = (int64_t)blockIdx.x * kEdgeThreads + threadIdx.x;
    int32_t a, b;
    const int st = e < E ? edge_state(row, col, node_map, e, N, a, b) : 1;
    const int nk = __popcll(__ballot(st == 2)), nb = __popcll(__ballot(st == 0));
    if (lane == 0) {
        wk[wave] = nk;
        wb[wave] = nb;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int sk = 0, sb = 0;
        for (int w = 0; w < kEdgeWaves; ++w) {
            sk += wk[w];
            sb += wb[w];
        }
        offs[blockIdx.x] = sk;
        bad[blockIdx.x] = sb;
    }
}

// One workgroup: offs[0 .. nblk] = exclusive prefix sums of the block counts (in place), total[0] = offs[nblk] = E',
// nbad[0] = the number of edges with an out-of-range end.  Integer sums: any order gives the same value.
__global__ __launch_bounds__(kSelThreads) void filter_edges_scan_kernel(int64_t *__restrict__ offs, const int32_t *__restrict__ bad,
                                                                        int64_t nblk, int64_t *__restrict__ total,
                                                                        int32_t *__restrict__ nbad)
{
    __shared__ int64_t part[kSelThreads];
    __shared__ int64_t partb[kSelThreads];
    const int tid = threadIdx.x;
    const int64_t per = (nblk + kSelThreads - 1) / kSelThreads;
    const int64_t lo = tid * per < nblk ? tid * per : nblk, hi = lo + per < nblk ? lo + per : nblk;
    int64_t sum = 0, sb = 0;
    for (int64_t i = lo; i < hi; ++i) {
        sum += offs[i];
        sb += bad[i];
    }
    part[tid] = sum;
    partb[tid] = sb;
    __syncthreads();
    if (tid == 0) {
        int64_t run = 0, runb = 0;
        for (int t = 0; t < kSelThreads; ++t) {
            const int64_t v = part[t];
            part[t] = run;
            run += v;
            runb += partb[t];
        }
        offs[nblk] = run;
        total[0] = run;
        nbad[0] = runb > INT32_MAX ? INT32_MAX : (int32_t)runb;
    }
    __syncthreads();
    int64_t run = part[tid];
    for (int64_t i = lo; i < hi; ++i) {
        const int64_t v = offs[i];
        offs[i] = run;
        run += v;
    }
}

// The writes: edge e of a block lands at offs[blk] + (kept edges of the block before e): the caller's order is kept.
__global__ __launch_bounds__(kEdgeThreads) void filter_edges_write_kernel(const int64_t *__restrict__ row,
                                                                          const int64_t *__restrict__ col,
                                                                          const int32_t *__restrict__ node_map, int64_t E,
                                                                          int64_t N, const int64_t *__restrict__ offs,
                                                                          int64_t Eout, int64_t *__restrict__ out_index,
                                                                          int64_t *__restrict__ kept)
{
    __shared__ int wk[kEdgeWaves];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int64_t e = (int64_t)blockIdx.x * kEdgeThreads + threadIdx.x;
    int32_t a = -1, b = -1;
    const bool keep = e < E && edge_state(row, col, node_map, e, N, a, b) == 2;
    const uint64_t mask = __ballot(keep);
    if (lane == 0) wk[wave] = __popcll(mask);
    __syncthreads();
    int before = __popcll(mask & lanes_below(lane));
    for (int w = 0; w < wave; ++w) before += wk[w];
    const int64_t o = offs[blockIdx.x] + before;
    if (keep && o >= 0 && o < Eout) {
        out_index[o] = a;
        out_index[Eout + o] = b;
        kept[o] = e;
    }
}

inline int64_t edge_blocks(int64_t E) { return (E + kEdgeThreads - 1) / kEdgeThreads; }

}  // namespace
}  // namespace dmet

using namespace dmet;

extern "C" size_t dmet_topk_workspace_bytes(int64_t N) { return N > 0 ? (size_t)N * 2 * sizeof(uint64_t) : 0; }

extern "C" int dmet_topk_f32(const float *score, const int64_t *ptr, int B, int64_t N, const int64_t *out_ptr, int64_t M,
                             int64_t *perm, int32_t *node_map, void *ws, size_t ws_bytes, dmet_stream_t stream)
{
    DMET_REQUIRE(N >= 0 && N <= INT32_MAX, "dmet_topk_f32: N=%lld outside 0..2^31-1", (long long)N);
    DMET_REQUIRE(B >= 0, "dmet_topk_f32: B=%d < 0", B);
    DMET_REQUIRE(M >= 0 && M <= INT32_MAX, "dmet_topk_f32: M=%lld outside 0..2^31-1", (long long)M);
    if (B == 0 || (N == 0 && M == 0)) return 0;
    DMET_REQUIRE(ws_bytes >= dmet_topk_workspace_bytes(N), "dmet_topk_f32: ws_bytes=%zu, dmet_topk_workspace_bytes asks for %zu",
                 ws_bytes, dmet_topk_workspace_bytes(N));
    DMET_REQUIRE(score || N == 0, "dmet_topk_f32: score is NULL");
    DMET_REQUIRE(ptr, "dmet_topk_f32: ptr is NULL");
    DMET_REQUIRE(out_ptr, "dmet_topk_f32: out_ptr is NULL");
    DMET_REQUIRE(perm || M == 0, "dmet_topk_f32: perm is NULL");
    DMET_REQUIRE(node_map || N == 0, "dmet_topk_f32: node_map is NULL");
    DMET_REQUIRE(ws || N == 0, "dmet_topk_f32: ws is NULL");
    hipLaunchKernelGGL(topk_kernel, dim3((unsigned)B), dim3(kSelThreads), 0, as_stream(stream), score, ptr, out_ptr, B, N, M,
                       perm, node_map, (uint64_t *)ws);
    DMET_LAUNCH_CHECK("topk_kernel");
    return 0;
}

extern "C" int dmet_select_rows_f32(const float *x, const float *s, const int64_t *perm, int64_t N, int64_t M, int F,
                                    float *out, dmet_stream_t stream)
{
    DMET_REQUIRE(F >= 1, "dmet_select_rows_f32: F=%d < 1", F);
    DMET_REQUIRE(N >= 0 && N <= INT32_MAX, "dmet_select_rows_f32: N=%lld outside 0..2^31-1", (long long)N);
    DMET_REQUIRE(M >= 0 && M <= INT32_MAX, "dmet_select_rows_f32: M=%lld outside 0..2^31-1", (long long)M);
    if (M == 0) return 0;
    DMET_REQUIRE(x || N == 0, "dmet_select_rows_f32: x is NULL");
    DMET_REQUIRE(perm, "dmet_select_rows_f32: perm is NULL");
    DMET_REQUIRE(out, "dmet_select_rows_f32: out is NULL");
    const int64_t blocks = (M * F + kRowThreads - 1) / kRowThreads;
    DMET_REQUIRE(blocks <= INT32_MAX, "dmet_select_rows_f32: M=%lld rows of F=%d are more than one grid", (long long)M, F);
    with_flags([&](auto gate) {
        hipLaunchKernelGGL(select_rows_kernel<decltype(gate)::value>, dim3((unsigned)blocks), dim3(kRowThreads), 0,
                           as_stream(stream), x, s, perm, N, M, F, out);
    }, s != nullptr);
    DMET_LAUNCH_CHECK("select_rows_kernel");
    return 0;
}

extern "C" int dmet_select_rows_bwd_f32(const float *g, const float *x, const float *s, const int32_t *node_map, int64_t N,
                                        int64_t M, int F, float *gx, float *gs, dmet_stream_t stream)
{
    DMET_REQUIRE(F >= 1, "dmet_select_rows_bwd_f32: F=%d < 1", F);
    DMET_REQUIRE(N >= 0 && N <= INT32_MAX, "dmet_select_rows_bwd_f32: N=%lld outside 0..2^31-1", (long long)N);
    DMET_REQUIRE(M >= 0 && M <= INT32_MAX, "dmet_select_rows_bwd_f32: M=%lld outside 0..2^31-1", (long long)M);
    if (N == 0 || (!gx && !gs)) return 0;
    DMET_REQUIRE(g || M == 0, "dmet_select_rows_bwd_f32: g is NULL");
    DMET_REQUIRE(node_map, "dmet_select_rows_bwd_f32: node_map is NULL");
    DMET_REQUIRE(x || !gs, "dmet_select_rows_bwd_f32: x is NULL and gs is asked for");
    const int64_t blocks = (N + kRowWaves - 1) / kRowWaves;
    with_flags([&](auto gate, auto wgx, auto wgs) {
        hipLaunchKernelGGL((select_rows_bwd_kernel<decltype(gate)::value, decltype(wgx)::value, decltype(wgs)::value>),
                           dim3((unsigned)blocks), dim3(kRowThreads), 0, as_stream(stream), g, x, s, node_map, N, M, F, gx, gs);
    }, s != nullptr, gx != nullptr, gs != nullptr);
    DMET_LAUNCH_CHECK("select_rows_bwd_kernel");
    return 0;
}

extern "C" int dmet_filter_table(const int32_t *nbr, const int32_t *cnt, const int64_t *perm, const int32_t *node_map,
                                 int64_t N, int64_t M, int k, int32_t *out_nbr, int32_t *out_cnt, dmet_stream_t stream)
{
    DMET_REQUIRE(k >= 1 && k <= DMET_SELECT_MAX_K, "dmet_filter_table: k=%d outside 1..%d", k, DMET_SELECT_MAX_K);
    DMET_REQUIRE(N >= 0 && N <= INT32_MAX, "dmet_filter_table: N=%lld outside 0..2^31-1", (long long)N);
    DMET_REQUIRE(M >= 0 && M <= INT32_MAX, "dmet_filter_table: M=%lld outside 0..2^31-1", (long long)M);
    if (M == 0) return 0;
    DMET_REQUIRE(nbr || N == 0, "dmet_filter_table: nbr is NULL");
    DMET_REQUIRE(perm, "dmet_filter_table: perm is NULL");
    DMET_REQUIRE(node_map || N == 0, "dmet_filter_table: node_map is NULL");
    DMET_REQUIRE(out_nbr, "dmet_filter_table: out_nbr is NULL");
    DMET_REQUIRE(out_cnt, "dmet_filter_table: out_cnt is NULL");
    const int64_t blocks = (M + kRowWaves - 1) / kRowWaves;
    hipLaunchKernelGGL(filter_table_kernel, dim3((unsigned)blocks), dim3(kRowThreads), 0, as_stream(stream), nbr, cnt, perm,
                       node_map, N, M, k, out_nbr, out_cnt);
    DMET_LAUNCH_CHECK("filter_table_kernel");
    return 0;
}

extern "C" size_t dmet_filter_edges_workspace_bytes(int64_t E)
{
    if (E <= 0) return 0;
    const size_t nblk = (size_t)edge_blocks(E);
    return align16((nblk + 1) * sizeof(int64_t)) + align16(nblk * sizeof(int32_t));
}

extern "C" int dmet_filter_edges_count(const int64_t *row, const int64_t *col, int64_t E, const int32_t *node_map, int64_t N,
                                       int64_t *total, int32_t *nbad, void *ws, size_t ws_bytes, dmet_stream_t stream)
{
    DMET_REQUIRE(E >= 0 && E <= INT32_MAX, "dmet_filter_edges_count: E=%lld outside 0..2^31-1", (long long)E);
    DMET_REQUIRE(N >= 0 && N <= INT32_MAX, "dmet_filter_edges_count: N=%lld outside 0..2^31-1", (long long)N);
    if (E == 0) return 0;
    DMET_REQUIRE(ws_bytes >= dmet_filter_edges_workspace_bytes(E),
                 "dmet_filter_edges_count: ws_bytes=%zu, dmet_filter_edges_workspace_bytes asks for %zu", ws_bytes,
                 dmet_filter_edges_workspace_bytes(E));
    DMET_REQUIRE(row, "dmet_filter_edges_count: row is NULL");
    DMET_REQUIRE(col, "dmet_filter_edges_count: col is NULL");
    DMET_REQUIRE(node_map || N == 0, "dmet_filter_edges_count: node_map is NULL");
    DMET_REQUIRE(total, "dmet_filter_edges_count: total is NULL");
    DMET_REQUIRE(nbad, "dmet_filter_edges_count: nbad is NULL");
    DMET_REQUIRE(ws, "dmet_filter_edges_count: ws is NULL");
    const int64_t nblk = edge_blocks(E);
    int64_t *offs = (int64_t *)ws;
    int32_t *bad = (int32_t *)((char *)ws + align16((size_t)(nblk + 1) * sizeof(int64_t)));
    hipLaunchKernelGGL(filter_edges_count_kernel, dim3((unsigned)nblk), dim3(kEdgeThreads), 0, as_stream(stream), row, col,
                       node_map, E, N, offs, bad);
    DMET_LAUNCH_CHECK("filter_edges_count_kernel");
    hipLaunchKernelGGL(filter_edges_scan_kernel, dim3(1), dim3(kSelThreads), 0, as_stream(stream), offs, bad, nblk, total, nbad);
    DMET_LAUNCH_CHECK("filter_edges_scan_kernel");
    return 0;
}

extern "C" int dmet_filter_edges_write(const int64_t *row, const int64_t *col, int64_t E, const int32_t *node_map, int64_t N,
                                       const void *ws, size_t ws_bytes, int64_t Eout, int64_t *out_index, int64_t *kept,
                                       dmet_stream_t stream)
{
    DMET_REQUIRE(E >= 0 && E <= INT32_MAX, "dmet_filter_edges_write: E=%lld outside 0..2^31-1", (long long)E);
    DMET_REQUIRE(N >= 0 && N <= INT32_MAX, "dmet_filter_edges_write: N=%lld outside 0..2^31-1", (long long)N);
    DMET_REQUIRE(Eout >= 0 && Eout <= E, "dmet_filter_edges_write: Eout=%lld outside 0..E=%lld", (long long)Eout, (long long)E);
    if (E == 0 || Eout == 0) return 0;
    DMET_REQUIRE(ws_bytes >= dmet_filter_edges_workspace_bytes(E),
                 "dmet_filter_edges_write: ws_bytes=%zu, dmet_filter_edges_workspace_bytes asks for %zu", ws_bytes,
                 dmet_filter_edges_workspace_bytes(E));
    DMET_REQUIRE(row, "dmet_filter_edges_write: row is NULL");
    DMET_REQUIRE(col, "dmet_filter_edges_write: col is NULL");
    DMET_REQUIRE(node_map, "dmet_filter_edges_write: node_map is NULL");
    DMET_REQUIRE(ws, "dmet_filter_edges_write: ws is NULL");
    DMET_REQUIRE(out_index, "dmet_filter_edges_write: out_index is NULL");
    DMET_REQUIRE(kept, "dmet_filter_edges_write: kept is NULL");
    const int64_t nblk = edge_blocks(E);
    hipLaunchKernelGGL(filter_edges_write_kernel, dim3((unsigned)nblk), dim3(kEdgeThreads), 0, as_stream(stream), row, col,
                       node_map, E, N, (const int64_t *)ws, Eout, out_index, kept);
    DMET_LAUNCH_CHECK("filter_edges_write_kernel");
    return 0;
}

// voxel.hip -- voxel clustering (torch_cluster's grid_cluster, PyG's voxel_grid) and the coarsening of its result
// (PyG's consecutive_cluster plus what the pooling operators derive from it).  Semantics: include/dmet.h, section
// "Voxel clustering".
#include "event_wg.h"

namespace dmet {
namespace {

constexpr int kVoxThreads = DMET_VOXEL_THREADS;     // workgroup of an event in the ranking
constexpr int kVoxWaves = kVoxThreads / kWave;
constexpr int kCellThreads = 256;                   // one node per thread
constexpr int kOutThreads = 256;                    // write-out: one workgroup per event
constexpr uint64_t kMaxCells = 0xFFFFFFFFull;       // cells of one event: the local cell id is a uint32

// One thread: nvox[d] = trunc((end_d - start_d) / size_d) + 1 in fp32, 1 for a NaN, infinite or negative quotient;
// nvox[D] = their product.  A product above 2^32 - 1 sets flags[0] and cuts the offending count so that it fits.
__global__ void voxel_setup_kernel(const float *__restrict__ grid, int D, int64_t *__restrict__ nvox, int32_t *__restrict__ flags)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    uint64_t prod = 1;
    int over = 0;
    for (int d = 0; d < D; ++d) {
        const float q = (grid[2 * D + d] - grid[D + d]) / grid[d];
        uint64_t nv;
        if (!(q >= 0.0f) || q == INFINITY) nv = 1;
        else if (q >= 4294967296.0f) nv = kMaxCells + 1;
        else nv = (uint64_t)q + 1;
        const uint64_t room = kMaxCells / prod;             // >= 1
        if (nv > room) {
            nv = room;
            over = 1;
        }
        prod *= nv;
        nvox[d] = (int64_t)nv;
    }
    nvox[D] = (int64_t)prod;
    flags[0] = over;
    flags[1] = 0;
}

// One node per thread.  The event of the workgroup's first node comes from one binary search over ptr (uniform over the
// workgroup); a thread walks on from there, at most B steps.  flags[1] = 1 (the same value from every thread that
// writes it) when batch[i] is not the event ptr gives.
__global__ __launch_bounds__(kCellThreads) void voxel_cells_kernel(const float *__restrict__ pos, int64_t N, int D,
                                                                   const float *__restrict__ grid,
                                                                   const int64_t *__restrict__ ptr, int B,
                                                                   const int64_t *__restrict__ batch,
                                                                   const int64_t *__restrict__ nvox, int32_t *__restrict__ flags,
                                                                   int64_t *__restrict__ id, uint32_t *__restrict__ cell)
{
    const int64_t r0 = (int64_t)blockIdx.x * kCellThreads;
    const int64_t i = r0 + threadIdx.x;
    int b = find_event(ptr, B, r0);
    if (i >= N) return;
    while (b + 1 < B && ptr[b + 1] <= i) ++b;
    uint64_t local = 0, mul = 1;
    for (int d = 0; d < D; ++d) {
        const uint64_t nv = (uint64_t)nvox[d];
        const float t = (pos[i * D + d] - grid[D + d]) / grid[d];       // one rounding each: -ffp-contract=off
        const double td = (double)t;
        uint64_t c;
        if (!(td > 0.0)) c = 0;                             // NaN, -inf, below start
        else if (td >= (double)nv) c = nv - 1;              // +inf, beyond end
        else c = (uint64_t)td;
        local += c * mul;
        mul *= nv;
    }
    id[i] = (int64_t)(local + (uint64_t)b * (uint64_t)nvox[D]);
    cell[i] = (uint32_t)local;
    if (batch && batch[i] != (int64_t)b) flags[1] = 1;
}

// Ascending bitonic network over key[0 .. P), P a power of two, by the whole workgroup: the network of select.hip's
// bitonic_desc with the comparison turned round.  Distinct keys except the padding ~0, which compares equal to itself
// only: the result does not depend on the network, so LDS and workspace give the same bits.
//
// S consecutive stages of a phase -- strides j, j / 2, ..., jl = j >> (S - 1) -- run as ONE pass over the keys: the 2^S
// keys base + q jl (base: a position with those S bits clear, group g's bits with S zeros inserted at bit log2(jl)) meet
// only each other in these stages, so a thread loads them, runs the S stages in registers and stores them; one barrier
// per pass.  All of a group lies on one side of bit k > j: one direction for the group.  A phase of m stages takes
// ceil(m / 3) passes instead of m, and the keys cross LDS (or L2) that many times.
//
// PAD (the LDS form): key i lives in slot i + i / 8.  The 64 lanes of a load then reach 64 different 8-byte slots of the
// 64 banks at every stride (two sweeps, the least a 64-bit access takes); unpadded, the groups of a stride of 1 to 16 keys
// start 64 jl bytes apart and pile up on 4 to 16 banks.
template <bool PAD, typename idx_t>
__device__ __forceinline__ idx_t slot(idx_t i)
{
    return PAD ? i + (i >> 3) : i;
}

template <typename idx_t, int S, bool PAD>
__device__ __forceinline__ void bitonic_pass(uint64_t *key, idx_t P, idx_t k, idx_t j)
{
    constexpr int G = 1 << S;
    const idx_t jl = j >> (S - 1);
    for (idx_t g = threadIdx.x; g < (P >> S); g += kVoxThreads) {
        const idx_t base = ((g & ~(jl - 1)) << S) | (g & (jl - 1));
        const bool asc = (base & k) == 0;
        uint64_t v[G];
#pragma unroll
        for (int q = 0; q < G; ++q) v[q] = key[slot<PAD>(base + (idx_t)q * jl)];
#pragma unroll
        for (int st = G >> 1; st > 0; st >>= 1) {
#pragma unroll
            for (int q = 0; q < G; ++q) {
                if ((q & st) == 0) {
                    const uint64_t a = v[q], b = v[q | st];
                    const bool swap = (a > b) == asc && a != b;
                    v[q] = swap ? b : a;
                    v[q | st] = swap ? a : b;
                }
            }
        }
#pragma unroll
        for (int q = 0; q < G; ++q) key[slot<PAD>(base + (idx_t)q * jl)] = v[q];
    }
    __syncthreads();
}

template <typename idx_t, bool PAD>
__device__ __forceinline__ void bitonic_asc(uint64_t *key, idx_t P)
{
    for (idx_t k = 2; k <= P; k <<= 1) {
        idx_t j = k >> 1;
        while (j > 0) {
            if (j >= 4) {
                bitonic_pass<idx_t, 3, PAD>(key, P, k, j);
                j >>= 3;
            } else if (j == 2) {
                bitonic_pass<idx_t, 2, PAD>(key, P, k, j);
                j = 0;
            } else {
                bitonic_pass<idx_t, 1, PAD>(key, P, k, j);
                j = 0;
            }
        }
    }
}

// The nodes of one event ranked by (cell, local index); a position whose cell differs from its predecessor's starts a
// cluster.  Writes order[lo + p] = the global node at sorted position p, node_map[lo + i] = the EVENT-LOCAL consecutive
// id of node i, first[lo + r] = the global position where local cluster r starts; returns the number of clusters.
template <typename idx_t, bool PAD>
__device__ __forceinline__ int64_t coarsen_event(uint64_t *key, int *wsum, const uint32_t *__restrict__ cell, int64_t lo,
                                                 int64_t n, int64_t *__restrict__ node_map, int64_t *__restrict__ order,
                                                 int32_t *__restrict__ first)
{
    idx_t P = 1;
    while ((int64_t)P < n) P <<= 1;
    for (idx_t i = threadIdx.x; i < P; i += kVoxThreads)
        key[slot<PAD>(i)] = (int64_t)i < n ? ((uint64_t)cell[lo + i] << 32) | (uint64_t)(uint32_t)i : ~0ull;
    __syncthreads();
    bitonic_asc<idx_t, PAD>(key, P);
    int64_t run = 0;                                        // clusters that start before this round (uniform)
    for (int64_t base = 0; base < n; base += kVoxThreads) {
        const int64_t p = base + threadIdx.x;
        uint64_t k = 0;
        bool head = false;
        if (p < n) {
            k = key[slot<PAD>((idx_t)p)];
            head = p == 0 || (uint32_t)(key[slot<PAD>((idx_t)(p - 1))] >> 32) != (uint32_t)(k >> 32);
        }
        int before, total;
        wg_rank<kVoxWaves>(head, wsum, before, total);
        if (p < n) {
            const int64_t r = run + before + (head ? 1 : 0) - 1;
            const int64_t i = (int64_t)(uint32_t)k;         // < n: the n real keys lead the padding
            order[lo + p] = lo + i;
            if (i < n) node_map[lo + i] = r;
            if (head) first[lo + r] = (int32_t)(lo + p);
        }
        run += total;
        __syncthreads();
    }
    return run;
}

// An event of up to DMET_SELECT_LDS_NODES nodes keeps its keys in LDS (144 KiB padded); a larger one keeps them in the
// caller's workspace at ws[2 lo ..): the power of two above n is < 2 n, so the events' ranges are disjoint.  Nodes no event
// owns belong to no cluster.
__global__ __launch_bounds__(kVoxThreads) void voxel_coarsen_kernel(const uint32_t *__restrict__ cell,
                                                                    const int64_t *__restrict__ ptr, int B, int64_t N,
                                                                    int64_t *__restrict__ node_map, int64_t *__restrict__ order,
                                                                    int32_t *__restrict__ first, int64_t *__restrict__ count,
                                                                    uint64_t *ws)
{
    __shared__ uint64_t lds[DMET_SELECT_LDS_NODES + DMET_SELECT_LDS_NODES / 8];        // 144 KiB: padded, see slot()
    __shared__ int wsum[kVoxWaves];
    const int b = blockIdx.x;
    const EventRange ev = event_range(ptr, b, N);
    const int64_t lo = ev.lo, hi = ev.hi, n = ev.n;
    // the nodes no event owns (ptr[0] > 0, ptr[B] < N), as for_unowned walks them
    if (b == 0)
        for (int64_t i = threadIdx.x; i < lo; i += kVoxThreads) node_map[i] = order[i] = -1;
    if (b == B - 1)
        for (int64_t i = hi + threadIdx.x; i < N; i += kVoxThreads) node_map[i] = order[i] = -1;
    int64_t c = 0;
    if (n > 0) {                                            // uniform over the workgroup
        if (n <= DMET_SELECT_LDS_NODES) c = coarsen_event<int, true>(lds, wsum, cell, lo, n, node_map, order, first);
        else c = coarsen_event<int64_t, false>(ws + 2 * lo, wsum, cell, lo, n, node_map, order, first);
    }
    if (threadIdx.x == 0) count[b] = c;
}

// One workgroup per event: the exclusive sum of the cluster counts before it (every workgroup adds up the B counts
// itself: B is small, integer sums have one value), then the event's part of every output.
__global__ __launch_bounds__(kOutThreads) void voxel_write_kernel(const int64_t *__restrict__ ptr, int B, int64_t N,
                                                                  const int64_t *__restrict__ count,
                                                                  const int32_t *__restrict__ first,
                                                                  int64_t *__restrict__ node_map, int32_t *__restrict__ rowptr,
                                                                  int64_t *__restrict__ out_batch, int64_t *__restrict__ out_ptr,
                                                                  int64_t *__restrict__ record)
{
    __shared__ int64_t part[4][kOutThreads];
    const int b = blockIdx.x, tid = threadIdx.x;
    int64_t before = 0, total = 0, mx = 0, mn = INT64_MAX;
    for (int e = tid; e < B; e += kOutThreads) {
        const int64_t v = count[e];
        before += e < b ? v : 0;
        total += v;
        mx = v > mx ? v : mx;
        mn = v < mn ? v : mn;
    }
    part[0][tid] = before, part[1][tid] = total, part[2][tid] = mx, part[3][tid] = mn;
    __syncthreads();
    for (int s = kOutThreads / 2; s > 0; s >>= 1) {
        if (tid < s) {
            part[0][tid] += part[0][tid + s];
            part[1][tid] += part[1][tid + s];
            part[2][tid] = part[2][tid + s] > part[2][tid] ? part[2][tid + s] : part[2][tid];
            part[3][tid] = part[3][tid + s] < part[3][tid] ? part[3][tid + s] : part[3][tid];
        }
        __syncthreads();
    }
    before = part[0][0], total = part[1][0];
    const EventRange ev = event_range(ptr, b, N);
    const int64_t lo = ev.lo, hi = ev.hi, n = ev.n;
    int64_t c = count[b];
    c = c < 0 ? 0 : (c > n ? n : c);
    for (int64_t i = tid; i < n; i += kOutThreads) node_map[lo + i] += before;
    for (int64_t r = tid; r < c && before + r < N; r += kOutThreads) {
        rowptr[before + r] = first[lo + r];
        out_batch[before + r] = b;
    }
    if (tid == 0) {
        out_ptr[b] = before;
        if (b == B - 1) {
            out_ptr[B] = total;
            if (total >= 0 && total <= N) rowptr[total] = (int32_t)hi;
            record[0] = total, record[1] = part[2][0], record[2] = part[3][0];
        }
    }
}

inline size_t keys_bytes(int64_t N) { return align16((size_t)N * 2 * sizeof(uint64_t)); }
inline size_t first_bytes(int64_t N) { return align16((size_t)N * sizeof(int32_t)); }

}  // namespace
}  // namespace dmet

using namespace dmet;

extern "C" int dmet_voxel_cells_f32(const float *pos, int64_t N, int D, const float *grid, const int64_t *ptr, int B,
                                    const int64_t *batch, int64_t *nvox, int32_t *flags, int64_t *id, uint32_t *cell,
                                    dmet_stream_t stream)
{
    DMET_REQUIRE(D >= 1 && D <= DMET_VOXEL_MAX_DIM, "dmet_voxel_cells_f32: D=%d outside 1..%d", D, DMET_VOXEL_MAX_DIM);
    DMET_REQUIRE(N >= 0 && N <= INT32_MAX, "dmet_voxel_cells_f32: N=%lld outside 0..2^31-1", (long long)N);
    DMET_REQUIRE(B >= 0, "dmet_voxel_cells_f32: B=%d < 0", B);
    DMET_REQUIRE(B >= 1 || N == 0, "dmet_voxel_cells_f32: B=0 with N=%lld nodes", (long long)N);
    DMET_REQUIRE(grid, "dmet_voxel_cells_f32: grid is NULL");
    DMET_REQUIRE(nvox, "dmet_voxel_cells_f32: nvox is NULL");
    DMET_REQUIRE(flags, "dmet_voxel_cells_f32: flags is NULL");
    hipLaunchKernelGGL(voxel_setup_kernel, dim3(1), dim3(kWave), 0, as_stream(stream), grid, D, nvox, flags);
    DMET_LAUNCH_CHECK("voxel_setup_kernel");
    if (N == 0) return 0;
    DMET_REQUIRE(pos, "dmet_voxel_cells_f32: pos is NULL");
    DMET_REQUIRE(ptr, "dmet_voxel_cells_f32: ptr is NULL");
    DMET_REQUIRE(id, "dmet_voxel_cells_f32: id is NULL");
    DMET_REQUIRE(cell, "dmet_voxel_cells_f32: cell is NULL");
    const int64_t blocks = (N + kCellThreads - 1) / kCellThreads;
    hipLaunchKernelGGL(voxel_cells_kernel, dim3((unsigned)blocks), dim3(kCellThreads), 0, as_stream(stream), pos, N, D, grid,
                       ptr, B, batch, nvox, flags, id, cell);
    DMET_LAUNCH_CHECK("voxel_cells_kernel");
    return 0;
}

extern "C" size_t dmet_voxel_coarsen_workspace_bytes(int64_t N, int B)
{
    if (N <= 0 || B <= 0) return 0;
    return keys_bytes(N) + first_bytes(N) + align16((size_t)B * sizeof(int64_t));
}

extern "C" int dmet_voxel_coarsen(const uint32_t *cell, const int64_t *ptr, int B, int64_t N, int64_t *node_map, int64_t *order,
                                  int32_t *rowptr, int64_t *out_batch, int64_t *out_ptr, int64_t *record, void *ws,
                                  size_t ws_bytes, dmet_stream_t stream)
{
    DMET_REQUIRE(N >= 0 && N <= INT32_MAX, "dmet_voxel_coarsen: N=%lld outside 0..2^31-1", (long long)N);
    DMET_REQUIRE(B >= 0, "dmet_voxel_coarsen: B=%d < 0", B);
    if (B == 0) return 0;
    DMET_REQUIRE(N > 0, "dmet_voxel_coarsen: N=0 with B=%d events: the caller fills the empty result", B);
    DMET_REQUIRE(ws_bytes >= dmet_voxel_coarsen_workspace_bytes(N, B),
                 "dmet_voxel_coarsen: ws_bytes=%zu, dmet_voxel_coarsen_workspace_bytes asks for %zu", ws_bytes,
                 dmet_voxel_coarsen_workspace_bytes(N, B));
    DMET_REQUIRE(cell, "dmet_voxel_coarsen: cell is NULL");
    DMET_REQUIRE(ptr, "dmet_voxel_coarsen: ptr is NULL");
    DMET_REQUIRE(node_map, "dmet_voxel_coarsen: node_map is NULL");
    DMET_REQUIRE(order, "dmet_voxel_coarsen: order is NULL");
    DMET_REQUIRE(rowptr, "dmet_voxel_coarsen: rowptr is NULL");
    DMET_REQUIRE(out_batch, "dmet_voxel_coarsen: out_batch is NULL");
    DMET_REQUIRE(out_ptr, "dmet_voxel_coarsen: out_ptr is NULL");
    DMET_REQUIRE(record, "dmet_voxel_coarsen: record is NULL");
    DMET_REQUIRE(ws, "dmet_voxel_coarsen: ws is NULL");
    uint64_t *keys = (uint64_t *)ws;
    int32_t *first = (int32_t *)((char *)ws + keys_bytes(N));
    int64_t *count = (int64_t *)((char *)ws + keys_bytes(N) + first_bytes(N));
    hipLaunchKernelGGL(voxel_coarsen_kernel, dim3((unsigned)B), dim3(kVoxThreads), 0, as_stream(stream), cell, ptr, B, N,
                       node_map, order, first, count, keys);
    DMET_LAUNCH_CHECK("voxel_coarsen_kernel");
    hipLaunchKernelGGL(voxel_write_kernel, dim3((unsigned)B), dim3(kOutThreads), 0, as_stream(stream), ptr, B, N, count, first,
                       node_map, rowptr, out_batch, out_ptr, record);
    DMET_LAUNCH_CHECK("voxel_write_kernel");
    return 0;
}

// fps.hip -- farthest point sampling (torch_cluster.fps).  Semantics: include/dmet.h, section "Farthest point sampling".
#include "common.h"

namespace dmet {
namespace {

constexpr int kFpsThreads = DMET_FPS_THREADS;
constexpr int kFpsWaves = kFpsThreads / kWave;
static_assert(kFpsWaves <= kWave && (kFpsWaves & (kFpsWaves - 1)) == 0, "the slot reduction is one butterfly of a wave");

__device__ __forceinline__ uint64_t umax64(uint64_t a, uint64_t b) { return a > b ? a : b; }

// "largest distance, lowest index" as one unsigned comparison: the distance's bits high (distances are never negative,
// so their bits order like unsigned integers), ~index low.  Every key of a real point is > 0, the key of no point.
__device__ __forceinline__ uint64_t fps_key(float d, uint32_t i)
{
    return ((uint64_t)__float_as_uint(d) << 32) | (uint64_t)(uint32_t)~i;
}

// The m picks of one event by one workgroup.  The event is held transposed, coordinate c of point i at cx[c * n + i], so
// that a wave's lanes read consecutive words; dist[i] is only ever touched by the thread that owns i (i mod
// kFpsThreads), and cx is read-only in the loop: the one exchange between threads is the per-wave (key) slot,
// double-buffered so that a wave writing the slots of iteration t + 1 cannot meet a wave still reading those of
// iteration t -- one workgroup barrier per iteration.
// DT: the number of coordinates at compile time (the pick's coordinates then sit in registers); 0 = any D <= 64: lane c
// of every wave holds coordinate c of the pick and the chain reads it with v_readlane.
// kLds: cx / dist are LDS (indexed in 32 bits), else global memory.
template <int DT, bool kLds>
__device__ __forceinline__ void fps_event(const float *cx, float *dist, uint64_t *slot, int64_t n, int D, int64_t m,
                                          int64_t s, int64_t lo, int64_t *__restrict__ out, int64_t o0, int64_t M)
{
    using idx_t = std::conditional_t<kLds, int, int64_t>;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const idx_t nn = (idx_t)n;
    // +inf: the first update then leaves d(p, start) itself (finite coordinates give no NaN), one loop for every pick
    for (idx_t i = tid; i < nn; i += kFpsThreads) dist[i] = __builtin_inff();
    int buf = 0;
    for (int64_t it = 0;; ++it) {
        if (tid == 0 && o0 + it < M) out[o0 + it] = lo + s;
        if (it + 1 >= m) break;                     // m is uniform over the workgroup
        float ps[DT > 0 ? DT : 1];
        if (DT > 0) {
#pragma unroll
            for (int c = 0; c < DT; ++c) ps[c] = cx[c * nn + (idx_t)s];
        } else {
            ps[0] = lane < D ? cx[lane * nn + (idx_t)s] : 0.0f;
        }
        uint64_t best = 0;
        for (idx_t i = tid; i < nn; i += kFpsThreads) {
            float acc = 0.0f;
            if (DT > 0) {
#pragma unroll
                for (int c = 0; c < DT; ++c) {
                    const float a = ps[c] - cx[c * nn + i];
                    acc = fmaf(a, a, acc);
                }
            } else {
                // eight loads in flight, then their eight links of the chain (one load per link is latency-bound)
                int c = 0;
                for (; c + 8 <= D; c += 8) {
                    float v[8];
#pragma unroll
                    for (int k = 0; k < 8; ++k) v[k] = cx[(c + k) * nn + i];
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        const float a = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ps[0]), c + k)) - v[k];
                        acc = fmaf(a, a, acc);
                    }
                }
                for (; c < D; ++c) {
                    const float a = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ps[0]), c)) - cx[c * nn + i];
                    acc = fmaf(a, a, acc);
                }
            }
            const float old = dist[i];
            const float d = acc < old ? acc : old;
            dist[i] = d;
            best = umax64(best, fps_key(d, (uint32_t)i));
        }
#pragma unroll
        for (int off = kWave / 2; off > 0; off >>= 1) best = umax64(best, __shfl_xor(best, off, kWave));
        if (lane == 0) slot[buf * kFpsWaves + wave] = best;
        __syncthreads();
        // every wave reduces the slots for itself
        uint64_t all = slot[buf * kFpsWaves + (lane & (kFpsWaves - 1))];
#pragma unroll
        for (int off = kFpsWaves / 2; off > 0; off >>= 1) all = umax64(all, __shfl_xor(all, off, kWave));
        const uint32_t win = ~(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)all);
        s = (int64_t)win < n ? (int64_t)win : 0;    // always a point of the event (n >= 1: some key was > 0)
        buf ^= 1;
    }
}

// xt[c * n + i] = xe[i * D + c] for the n points of an event, by the whole workgroup: consecutive threads read
// consecutive words, and (i, c) of word e = tid + k * kFpsThreads is stepped without a division.
template <typename idx_t>
__device__ __forceinline__ void fps_transpose(const float *__restrict__ xe, float *xt, idx_t n, int D)
{
    const int qs = kFpsThreads / D, rs = kFpsThreads % D;
    idx_t i = (int)threadIdx.x / D;
    int c = (int)threadIdx.x % D;
    while (i < n) {
        xt[c * n + i] = xe[i * D + c];
        c += rs;
        i += qs;
        if (c >= D) {
            c -= D;
            i += 1;
        }
    }
}

// One workgroup per event.  An event of up to DMET_FPS_LDS_NODES(D) nodes keeps its transposed coordinates and its
// running distances in LDS; a larger one keeps both in the caller's workspace (dist[N], then the events' transposed
// coordinates [N * D], read back through L2) and runs the same code.
template <int DT>
__global__ __launch_bounds__(kFpsThreads) void fps_kernel(const float *__restrict__ x, const int64_t *__restrict__ ptr,
                                                          const int64_t *__restrict__ out_ptr,
                                                          const int64_t *__restrict__ start, int64_t *__restrict__ out,
                                                          float *ws, int64_t N, int D, int64_t M)
{
    __shared__ float lds[DMET_FPS_LDS_FLOATS];
    __shared__ uint64_t slot[2 * kFpsWaves];
    const int b = blockIdx.x;
    const int64_t lo = ptr[b], n = ptr[b + 1] - lo;
    const int64_t o0 = out_ptr[b], m = out_ptr[b + 1] - o0;
    if (n <= 0 || m <= 0 || lo < 0 || lo + n > N || o0 < 0) return;     // uniform over the workgroup
    int64_t s = start ? start[b] : 0;
    s = s < 0 ? 0 : (s > n - 1 ? n - 1 : s);
    if (n <= DMET_FPS_LDS_NODES(D)) {
        float *xt = lds + n;        // dist[n] | coordinate 0 of every point | coordinate 1 | ...
        fps_transpose<int>(x + lo * D, xt, (int)n, D);
        __syncthreads();
        fps_event<DT, true>(xt, lds, slot, n, D, m, s, lo, out, o0, M);
    } else {
        float *xt = ws + N + lo * D;
        fps_transpose<int64_t>(x + lo * D, xt, n, D);
        __syncthreads();            // the workgroup's own global stores, read back by the same workgroup
        fps_event<DT, false>(xt, ws + lo, slot, n, D, m, s, lo, out, o0, M);
    }
}

}  // namespace
}  // namespace dmet

using namespace dmet;

extern "C" size_t dmet_fps_workspace_bytes(int64_t N, int B, int D)
{
    (void)B;
    return N > 0 && D > 0 ? (size_t)N * ((size_t)D + 1) * sizeof(float) : 0;
}

extern "C" int dmet_fps_f32(const float *x, const int64_t *ptr, int B, int64_t N, int D, const int64_t *out_ptr,
                            const int64_t *start, int64_t M, int64_t *out, void *ws, size_t ws_bytes,
                            dmet_stream_t stream)
{
    DMET_REQUIRE(D >= 1 && D <= DMET_MAX_KNN_DIM, "dmet_fps_f32: D=%d outside 1..%d", D, DMET_MAX_KNN_DIM);
    DMET_REQUIRE(N >= 0 && N <= INT32_MAX, "dmet_fps_f32: N=%lld outside 0..2^31-1", (long long)N);
    DMET_REQUIRE(B >= 0, "dmet_fps_f32: B=%d < 0", B);
    DMET_REQUIRE(M >= 0, "dmet_fps_f32: M=%lld < 0", (long long)M);
    if (B == 0 || N == 0 || M == 0) return 0;
    DMET_REQUIRE(ws_bytes >= dmet_fps_workspace_bytes(N, B, D),
                 "dmet_fps_f32: ws_bytes=%zu, dmet_fps_workspace_bytes asks for %zu", ws_bytes,
                 dmet_fps_workspace_bytes(N, B, D));
    DMET_REQUIRE(x, "dmet_fps_f32: x is NULL");
    DMET_REQUIRE(ptr, "dmet_fps_f32: ptr is NULL");
    DMET_REQUIRE(out_ptr, "dmet_fps_f32: out_ptr is NULL");
    DMET_REQUIRE(out, "dmet_fps_f32: out is NULL");
    DMET_REQUIRE(ws, "dmet_fps_f32: ws is NULL");
    const bool known = with_int<1, 2, 3, 4>(D, [&](auto dt) {
        hipLaunchKernelGGL(fps_kernel<decltype(dt)::value>, dim3((unsigned)B), dim3(kFpsThreads), 0, as_stream(stream), x,
                           ptr, out_ptr, start, out, (float *)ws, N, D, M);
    });
    if (!known)
        hipLaunchKernelGGL(fps_kernel<0>, dim3((unsigned)B), dim3(kFpsThreads), 0, as_stream(stream), x, ptr, out_ptr,
                           start, out, (float *)ws, N, D, M);
    DMET_LAUNCH_CHECK("fps_kernel");
    return 0;
}

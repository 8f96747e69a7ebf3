// interpolate.hip -- inverse-distance feature propagation (torch_geometric.nn.unpool.knn_interpolate after its kNN search)
// over a fixed-width table with the table's own distances.
//
// For target i and every valid slot t of its row, j = nbr[i,t]:
//   w_t = 1 / clamp(dist[i,t], 1e-16)   W_i = sum_t w_t     r_t = w_t / W_i     out[i,:] = sum_t r_t x[j,:]   (fma chain)
// and by source j over the reverse index: g_x[j,:] = sum_p r_p g_out[i,:], r_p recomputed from dist[p] and wsum[i] = W_i.
// The [E, F] messages are never written, there are no float atomics, both sums run in ascending slot / position order.
//
// Lane layout, both kernels (the one of gravnet.hip): a group of LPT lanes (16, 32 or 64, inside one wavefront) owns one
// row (a target in the forward, a source in the backward).  Per chunk of LPT entries of the row, lane l forms the scalars
// of entry l (id, w) once; the group takes them back by a shuffle inside the group, keeps kInFlight row gathers in
// flight and adds in entry order.  A lane owns the units u = lane, lane + LPT, ... of a row; a unit is a float4 where
// F % 4 == 0 and the rows start on 16-byte boundaries (VEC), else a float.  F stays a run-time argument.  No LDS, no
// barriers.  The arithmetic per element is the same in both unit types: the same bits.
#include "common.h"

namespace dmet {
namespace {

constexpr int kInterpBlock = 256;
constexpr int kInterpInFlight = 4;     // row gathers in flight per group
constexpr int kInterpMaxF = 256;
constexpr float kInterpMinD = 1e-16f;  // PyG: clamp(squared_distance, min=1e-16)

// the clamp is a comparison, not fmaxf: a NaN distance gives a NaN weight (torch.clamp keeps NaN), never 1e16
__device__ __forceinline__ float interp_weight(float d) { return 1.0f / (d < kInterpMinD ? kInterpMinD : d); }

__device__ __forceinline__ void zero_unit(float &a) { a = 0.f; }
__device__ __forceinline__ void zero_unit(float4 &a) { a = make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ void fma_unit(float &a, float r, const float &v) { a = fmaf(r, v, a); }
__device__ __forceinline__ void fma_unit(float4 &a, float r, const float4 &v)
{
    a.x = fmaf(r, v.x, a.x);
    a.y = fmaf(r, v.y, a.y);
    a.z = fmaf(r, v.z, a.z);
    a.w = fmaf(r, v.w, a.w);
}

// Forward.  U = units per row (F or F / 4).  Pass 1 forms W_i over all chunks (a serial sum over the group's lanes, the
// same in every lane), pass 2 the normalised weights and the gathers; with k <= LPT the one chunk stays in registers.
template <int LPT, int ITER, typename V>
__global__ __launch_bounds__(kInterpBlock) void interpolate_fwd_kernel(
    const V *__restrict__ x, const int32_t *__restrict__ nbr, const float *__restrict__ dist, int64_t Nt, int64_t Ns,
    int k, int U, V *__restrict__ out, float *__restrict__ wsum)
{
    constexpr int TPB = kInterpBlock / LPT;
    const int bid = xcd_swizzle(blockIdx.x, gridDim.x);
    const int64_t i = (int64_t)bid * TPB + threadIdx.x / LPT;
    const int lane = threadIdx.x % LPT;
    if (i >= Nt) return;        // whole groups leave: the shuffles below stay inside a group
    const int32_t *row = nbr + i * k;
    const float *drow = dist + i * k;

    // lane l: id and weight of slot base + l (validity comes from the id, never from the distance)
    int32_t jl = -1;
    float wl = 0.f;
    auto form = [&](int base) {
        jl = -1;
        wl = 0.f;
        if (base + lane < k) {
            const int32_t j = row[base + lane];
            if (j >= 0 && (int64_t)j < Ns) {
                jl = j;
                wl = interp_weight(drow[base + lane]);
            }
        }
    };
    float W = 0.f;
    int n = 0;
    for (int base = 0; base < k; base += LPT) {
        form(base);
        const int m = min(LPT, k - base);
        for (int e = 0; e < m; ++e) {
            const int32_t j = __shfl(jl, e, LPT);
            const float w = __shfl(wl, e, LPT);
            if (j >= 0) {       // the same for every lane of the group
                W += w;
                ++n;
            }
        }
    }

    V acc[ITER];
#pragma unroll
    for (int it = 0; it < ITER; ++it) zero_unit(acc[it]);
    if (n > 0) {
        for (int base = 0; base < k; base += LPT) {
            if (k > LPT) form(base);
            const float rl = wl / W;
            const int m = min(LPT, k - base);
            for (int e0 = 0; e0 < m; e0 += kInterpInFlight) {
                int32_t j[kInterpInFlight];
                float r[kInterpInFlight];
                V v[kInterpInFlight][ITER];
#pragma unroll
                for (int u = 0; u < kInterpInFlight; ++u) {
                    j[u] = __shfl(jl, (e0 + u) & (LPT - 1), LPT);
                    r[u] = __shfl(rl, (e0 + u) & (LPT - 1), LPT);
                    if (e0 + u >= m) j[u] = -1;
                }
#pragma unroll
                for (int u = 0; u < kInterpInFlight; ++u)
#pragma unroll
                    for (int it = 0; it < ITER; ++it) {
                        const int p = lane + it * LPT;
                        zero_unit(v[u][it]);
                        if (j[u] >= 0 && p < U) v[u][it] = x[(int64_t)j[u] * U + p];
                    }
#pragma unroll
                for (int u = 0; u < kInterpInFlight; ++u) {
                    if (j[u] < 0) continue;        // the same for every lane of the group
#pragma unroll
                    for (int it = 0; it < ITER; ++it) fma_unit(acc[it], r[u], v[u][it]);
                }
            }
        }
    }
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
        const int p = lane + it * LPT;
        if (p < U) out[i * U + p] = acc[it];        // a row without a valid slot: zeros (R3)
    }
    if (lane == 0) wsum[i] = n > 0 ? W : 0.f;
}

// Backward, by source: for source j, over the table positions pos = i*k + t that hold j (rev_pos, ascending):
//   g_x[j,:] = sum r_pos g_out[i,:],  r_pos = w(dist[pos]) / wsum[i]  (the forward's expression)
// A hub's list is walked by its one group, however long it is.
template <int LPT, int ITER, typename V>
__global__ __launch_bounds__(kInterpBlock) void interpolate_bwd_kernel(
    const V *__restrict__ g_out, const float *__restrict__ dist, const float *__restrict__ wsum,
    const int32_t *__restrict__ rev_ptr, const int32_t *__restrict__ rev_pos, int64_t Nt, int64_t Ns, int k, int U,
    V *__restrict__ g_x)
{
    constexpr int TPB = kInterpBlock / LPT;
    const int bid = xcd_swizzle(blockIdx.x, gridDim.x);
    const int64_t j = (int64_t)bid * TPB + threadIdx.x / LPT;
    const int lane = threadIdx.x % LPT;
    if (j >= Ns) return;
    const int64_t M = Nt * k;
    const int64_t lo = min(max((int64_t)rev_ptr[j], (int64_t)0), M);
    const int64_t hi = min(max((int64_t)rev_ptr[j + 1], lo), M);

    V acc[ITER];
#pragma unroll
    for (int it = 0; it < ITER; ++it) zero_unit(acc[it]);
    for (int64_t base = lo; base < hi; base += LPT) {
        // lane l: target and normalised weight of entry base + l
        int32_t il = -1;
        float rl = 0.f;
        if (base + lane < hi) {
            const int64_t pos = rev_pos[base + lane];
            if (pos >= 0 && pos < M) {
                il = (int32_t)(pos / k);
                rl = interp_weight(dist[pos]) / wsum[il];
            }
        }
        const int m = (int)min((int64_t)LPT, hi - base);
        for (int e0 = 0; e0 < m; e0 += kInterpInFlight) {
            int32_t i[kInterpInFlight];
            float r[kInterpInFlight];
            V g[kInterpInFlight][ITER];
#pragma unroll
            for (int u = 0; u < kInterpInFlight; ++u) {
                i[u] = __shfl(il, (e0 + u) & (LPT - 1), LPT);
                r[u] = __shfl(rl, (e0 + u) & (LPT - 1), LPT);
                if (e0 + u >= m) i[u] = -1;
            }
#pragma unroll
            for (int u = 0; u < kInterpInFlight; ++u)
#pragma unroll
                for (int it = 0; it < ITER; ++it) {
                    const int p = lane + it * LPT;
                    zero_unit(g[u][it]);
                    if (i[u] >= 0 && p < U) g[u][it] = g_out[(int64_t)i[u] * U + p];
                }
#pragma unroll
            for (int u = 0; u < kInterpInFlight; ++u) {
                if (i[u] < 0) continue;        // the same for every lane of the group
#pragma unroll
                for (int it = 0; it < ITER; ++it) fma_unit(acc[it], r[u], g[u][it]);
            }
        }
    }
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
        const int p = lane + it * LPT;
        if (p < U) g_x[j * U + p] = acc[it];        // a source nobody lists: zeros
    }
}

struct InterpArgs {
    const float *x, *dist, *wsum_in, *g_out;
    const int32_t *nbr, *rev_ptr, *rev_pos;
    int64_t Nt, Ns;
    int k, F;
    float *out, *wsum, *g_x;
};

template <bool FWD, int LPT, int ITER, typename V>
int launch(const InterpArgs &a, hipStream_t st)
{
    constexpr int TPB = kInterpBlock / LPT;
    const int U = a.F / (int)(sizeof(V) / sizeof(float));
    const int64_t rows = FWD ? a.Nt : a.Ns;
    const int64_t blocks = (rows + TPB - 1) / TPB;
    if constexpr (FWD) {
        hipLaunchKernelGGL((interpolate_fwd_kernel<LPT, ITER, V>), dim3((unsigned)blocks), dim3(kInterpBlock), 0, st,
                           reinterpret_cast<const V *>(a.x), a.nbr, a.dist, a.Nt, a.Ns, a.k, U,
                           reinterpret_cast<V *>(a.out), a.wsum);
        DMET_LAUNCH_CHECK("interpolate_fwd_kernel");
    } else {
        hipLaunchKernelGGL((interpolate_bwd_kernel<LPT, ITER, V>), dim3((unsigned)blocks), dim3(kInterpBlock), 0, st,
                           reinterpret_cast<const V *>(a.g_out), a.dist, a.wsum_in, a.rev_ptr, a.rev_pos, a.Nt, a.Ns, a.k,
                           U, reinterpret_cast<V *>(a.g_x));
        DMET_LAUNCH_CHECK("interpolate_bwd_kernel");
    }
    return 0;
}

// lanes per row and units per lane for a width F.  float4 units (vec): one per lane, 16 lanes up to F = 64, 32 up to 128,
// 64 up to 256.  float units: 16 lanes up to F = 32 (two per lane), 32 up to 128 and 64 up to 256 (four per lane).
template <bool FWD>
int dispatch(const InterpArgs &a, bool vec, hipStream_t st)
{
    if (vec) {
        if (a.F <= 64) return launch<FWD, 16, 1, float4>(a, st);
        if (a.F <= 128) return launch<FWD, 32, 1, float4>(a, st);
        return launch<FWD, 64, 1, float4>(a, st);
    }
    if (a.F <= 32) return launch<FWD, 16, 2, float>(a, st);
    if (a.F <= 128) return launch<FWD, 32, 4, float>(a, st);
    return launch<FWD, 64, 4, float>(a, st);
}

int check_shape(const char *who, int64_t Nt, int64_t Ns, int k, int F)
{
    DMET_REQUIRE(Nt >= 0 && Ns >= 0 && Nt < (int64_t)2147483647 && Ns < (int64_t)2147483647,
                 "%s: Nt=%lld, Ns=%lld out of range", who, (long long)Nt, (long long)Ns);
    DMET_REQUIRE(k >= 1 && k <= DMET_MAX_K, "%s: k=%d not in [1,%d]", who, k, DMET_MAX_K);
    DMET_REQUIRE(F >= 1 && F <= kInterpMaxF, "%s: F=%d not in [1,%d]", who, F, kInterpMaxF);
    DMET_REQUIRE(Nt * (int64_t)k < (int64_t)2147483647, "%s: Nt*k out of range", who);
    return 0;
}

}  // namespace
}  // namespace dmet

using namespace dmet;

extern "C" int dmet_interpolate_fwd_f32(const float *x, const int32_t *nbr, const float *dist, int64_t Nt, int64_t Ns, int k,
                                        int F, float *out, float *wsum, dmet_stream_t stream)
{
    if (int rc = check_shape("dmet_interpolate_fwd_f32", Nt, Ns, k, F)) return rc;
    if (Nt == 0) return 0;
    DMET_REQUIRE(nbr && dist && out && wsum, "dmet_interpolate_fwd_f32: null pointer");
    DMET_REQUIRE(Ns == 0 || x, "dmet_interpolate_fwd_f32: null x with Ns=%lld", (long long)Ns);
    InterpArgs a{};
    a.x = x; a.nbr = nbr; a.dist = dist; a.Nt = Nt; a.Ns = Ns; a.k = k; a.F = F; a.out = out; a.wsum = wsum;
    const bool vec = F % 4 == 0 && aligned16(x) && aligned16(out);
    return dispatch<true>(a, vec, as_stream(stream));
}

extern "C" int dmet_interpolate_bwd_f32(const float *g_out, const float *dist, const float *wsum, const int32_t *rev_ptr,
                                        const int32_t *rev_pos, int64_t Nt, int64_t Ns, int k, int F, float *g_x,
                                        dmet_stream_t stream)
{
    if (int rc = check_shape("dmet_interpolate_bwd_f32", Nt, Ns, k, F)) return rc;
    if (Ns == 0) return 0;      // no source: nothing to write
    DMET_REQUIRE(g_x, "dmet_interpolate_bwd_f32: null g_x");
    hipStream_t st = as_stream(stream);
    if (Nt == 0) {      // no target: nothing reaches a source
        hipError_t e = hipMemsetAsync(g_x, 0, (size_t)Ns * F * sizeof(float), st);
        if (e != hipSuccess) return hip_fail(e, "dmet_interpolate_bwd_f32: memset");
        return 0;
    }
    DMET_REQUIRE(g_out && dist && wsum && rev_ptr && rev_pos, "dmet_interpolate_bwd_f32: null pointer");
    InterpArgs a{};
    a.g_out = g_out; a.dist = dist; a.wsum_in = wsum; a.rev_ptr = rev_ptr; a.rev_pos = rev_pos;
    a.Nt = Nt; a.Ns = Ns; a.k = k; a.F = F; a.g_x = g_x;
    const bool vec = F % 4 == 0 && aligned16(g_out) && aligned16(g_x);
    return dispatch<false>(a, vec, st);
}

// Micro-benchmark: sorted insertion into the re-rank's KP-slot (distance bits, id) list, one candidate per lane and step.
//   form 0: one 64-bit unsigned compare per slot, two 64-bit selects on its condition (csrc/knn_filter.h before r07)
//   form 1: v_min_f64 / v_max_f64 on the words read as doubles (csrc/knn_key64.h)
// Both forms get the same word stream (a 32-bit xorshift per lane; one word in eight has distance bits 0, i.e. is a
// subnormal double, one in sixteen lies at or beyond the sentinel), and the final lists are compared word for word.
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off tools/key64_micro.hip -o key64_micro && ./key64_micro
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <algorithm>
#include <vector>
#include "../deepmetv2_amd/csrc/knn_key64.h"

using dmet::kKey64Empty;
typedef unsigned long long u64;

#define CHECK(e) do { hipError_t r_ = (e); if (r_ != hipSuccess) { printf("%s: %s\n", #e, hipGetErrorString(r_)); return 1; } } while (0)

__device__ __forceinline__ u64 next_word(unsigned &s, unsigned j)
{
    s ^= s << 13; s ^= s >> 17; s ^= s << 5;
    unsigned hi = s >> 2;                                   // < 2^30: below the sentinel's 0x501502F9
    if ((s & 7u) == 0u) hi = 0u;                            // zero distance
    if ((s & 15u) == 1u) hi = s | 0x60000000u;              // at or beyond the sentinel, NaN and negative patterns included
    return dmet::key64_word(hi, j);
}

template <int KP, int FORM>
__global__ __launch_bounds__(64) void k(u64 *__restrict__ out, int iters)
{
    const int lane = threadIdx.x;
    unsigned s = 0x9E3779B9u * (blockIdx.x * 64 + lane + 1);
    if constexpr (FORM == 0) {
        u64 kk[KP];
#pragma unroll
        for (int p = 0; p < KP; ++p) kk[p] = kKey64Empty;
        for (int it = 0; it < iters; ++it) {
            const u64 nk = next_word(s, (unsigned)it);
            bool g[KP];
#pragma unroll
            for (int p = 0; p < KP; ++p) g[p] = kk[p] > nk;
#pragma unroll
            for (int p = KP - 1; p >= 1; --p) kk[p] = g[p - 1] ? kk[p - 1] : (g[p] ? nk : kk[p]);
            kk[0] = g[0] ? nk : kk[0];
        }
#pragma unroll
        for (int p = 0; p < KP; ++p) out[((size_t)blockIdx.x * KP + p) * 64 + lane] = kk[p];
    } else {
        double kk[KP];
#pragma unroll
        for (int p = 0; p < KP; ++p) kk[p] = dmet::key64_as_double(kKey64Empty);
        for (int it = 0; it < iters; ++it) dmet::key64_insert<KP>(kk, next_word(s, (unsigned)it));
#pragma unroll
        for (int p = 0; p < KP; ++p) out[((size_t)blockIdx.x * KP + p) * 64 + lane] = dmet::key64_as_word(kk[p]);
    }
}

template <int KP, int FORM>
int run(int waves_per_simd, int cus, u64 *dout, std::vector<u64> &host, int reps)
{
    const int blocks = cus * 4 * waves_per_simd, iters = 20000;
    hipEvent_t a, b;
    CHECK(hipEventCreate(&a));
    CHECK(hipEventCreate(&b));
    hipLaunchKernelGGL((k<KP, FORM>), dim3(blocks), dim3(64), 0, 0, dout, iters);   // warm-up
    std::vector<float> ms(reps);
    for (int r = 0; r < reps; ++r) {
        CHECK(hipEventRecord(a));
        hipLaunchKernelGGL((k<KP, FORM>), dim3(blocks), dim3(64), 0, 0, dout, iters);
        CHECK(hipEventRecord(b));
        CHECK(hipEventSynchronize(b));
        CHECK(hipEventElapsedTime(&ms[r], a, b));
    }
    CHECK(hipGetLastError());
    host.resize((size_t)blocks * KP * 64);
    CHECK(hipMemcpy(host.data(), dout, host.size() * 8, hipMemcpyDeviceToHost));
    std::sort(ms.begin(), ms.end());
    const double ns = ms[reps / 2] * 1e6 / iters;           // per insertion and wavefront
    printf("KP=%2d %-12s waves/SIMD=%d  median %.3f ms  min %.3f  max %.3f  (%d runs)  %.1f ns = %.0f cycles at 2.4 GHz per insertion\n",
           KP, FORM ? "f64 min/max" : "cmp/select", waves_per_simd, ms[reps / 2], ms[0], ms[reps - 1], reps, ns, ns * 2.4);
    CHECK(hipEventDestroy(a));
    CHECK(hipEventDestroy(b));
    return 0;
}

template <int KP>
int both(int cus, u64 *dout)
{
    std::vector<u64> h0, h1;
    for (int w = 1; w <= 2; ++w) {
        if (run<KP, 0>(w, cus, dout, h0, 7)) return 1;
        if (run<KP, 1>(w, cus, dout, h1, 7)) return 1;
        size_t bad = 0;
        for (size_t i = 0; i < h0.size(); ++i) bad += h0[i] != h1[i];
        printf("KP=%2d waves/SIMD=%d  final lists: %zu of %zu words differ\n", KP, w, bad, h0.size());
        if (bad) return 1;
    }
    return 0;
}

int main()
{
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, 0));
    const int cus = prop.multiProcessorCount;
    printf("%s, %d CUs\n", prop.gcnArchName, cus);
    u64 *dout;
    CHECK(hipMalloc(&dout, (size_t)cus * 4 * 2 * 20 * 64 * 8));
    if (both<16>(cus, dout)) return 1;
    if (both<20>(cus, dout)) return 1;
    CHECK(hipFree(dout));
    return 0;
}

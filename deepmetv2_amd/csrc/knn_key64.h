// Sorted top-KP list of the kNN re-rank as 64-bit words, inserted into with f64 min / max.
//
// A word is (float bits of d) << 32 | j with d >= +0.  Read as IEEE doubles, non-negative finite doubles order exactly as
// their bit patterns do, so for a sorted list the compare / select insertion
//     new[p] = g[p-1] ? old[p-1] : (g[p] ? nk : old[p])        g[p] = old[p] > nk   (unsigned 64-bit)
// is
//     new[p] = max(old[p-1], min(old[p], nk)),   new[0] = min(old[0], nk):
// two instructions per slot, no condition in a scalar register pair and no wait state behind it.
//
// The domain is closed by key64_word(): the high word is clamped (unsigned) to the sentinel's bits.  +inf, every NaN
// pattern, every pattern with the sign bit set (a negative double would sort first) and the ~0 of an exhausted lane all
// become (sentinel, j) >= the empty slot (sentinel, 0), which min / max leaves alone exactly as the strict '>' does.
// After the clamp no operand has exponent field 0x7FF: IEEE mode has nothing to quiet.  Distance 0 gives high word 0,
// i.e. a subnormal double (+0.0 when j = 0): the kernels that use this keep f64 subnormals (.amdhsa_float_denorm_mode_16_64
// 3, hipcc's default), and tests/test_gpu_knn_rerank_keys.py (duplicates) fails if that ever stops holding.
//
// Host code (tests/test_knn_key64_host.py) takes the fmin / fmax path of the same network; the device path is one asm
// statement per instruction -- __builtin_fmin / __builtin_fmax canonicalise every operand with a v_max_f64 of its own.
#pragma once
#include <stdint.h>
#include <string.h>
#if !defined(__HIP_DEVICE_COMPILE__)
#include <math.h>
#endif

#if defined(__HIPCC__)
#define DMET_KEY64_FN __host__ __device__ __forceinline__
#else
#define DMET_KEY64_FN inline
#endif

namespace dmet {

constexpr unsigned kKey64SentinelBits = 0x501502F9u;                                  // float bits of 1e10f (kKnnSentinel)
constexpr unsigned long long kKey64Empty = (unsigned long long)kKey64SentinelBits << 32;   // (sentinel, 0)

// the word of a candidate: (min(dbits, sentinel bits), j)
DMET_KEY64_FN unsigned long long key64_word(unsigned dbits, unsigned j)
{
    const unsigned hi = dbits < kKey64SentinelBits ? dbits : kKey64SentinelBits;
    return ((unsigned long long)hi << 32) | j;
}

// the word of (dbits, j) when live, of an exhausted lane (never inserted) otherwise
DMET_KEY64_FN unsigned long long key64_word(unsigned dbits, unsigned j, bool live)
{
    return key64_word(live ? dbits : 0xFFFFFFFFu, j);
}

DMET_KEY64_FN double key64_as_double(unsigned long long w)
{
    double d;
    memcpy(&d, &w, 8);
    return d;
}

DMET_KEY64_FN unsigned long long key64_as_word(double d)
{
    unsigned long long w;
    memcpy(&w, &d, 8);
    return w;
}

// kk: sorted ascending, every word <= kKey64Empty; w: from key64_word()
template <int KP>
DMET_KEY64_FN void key64_insert(double (&kk)[KP], unsigned long long w)
{
    const double nk = key64_as_double(w);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
    for (int p = KP - 1; p >= 1; --p) {
        double t;
        asm("v_min_f64 %0, %1, %2" : "=v"(t) : "v"(kk[p]), "v"(nk));
        asm("v_max_f64 %0, %1, %2" : "=v"(kk[p]) : "v"(kk[p - 1]), "v"(t));
    }
    asm("v_min_f64 %0, %1, %2" : "=v"(kk[0]) : "v"(kk[0]), "v"(nk));
#else
    for (int p = KP - 1; p >= 1; --p) kk[p] = fmax(kk[p - 1], fmin(kk[p], nk));
    kk[0] = fmin(kk[0], nk);
#endif
}

}  // namespace dmet

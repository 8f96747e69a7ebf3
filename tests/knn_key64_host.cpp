// Host fuzz of csrc/knn_key64.h (built and run by tests/test_knn_key64_host.py): the f64 min / max insertion -- its
// host path, bit casts + fmin / fmax -- against the compare / select insertion on unsigned 64-bit words that the kNN
// re-rank used before, on lists of 8 / 16 / 20 slots, partly empty and full.  The final lists must be equal word for word.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "knn_key64.h"

typedef unsigned long long u64;
using namespace dmet;

static u64 rng_state = 0x243F6A8885A308D3ull;
static u64 rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return rng_state;
}

struct Cand { unsigned dbits, j; bool live; };

static const unsigned kEdgeHi[] = {0u, 0u, 0u, 1u, kKey64SentinelBits - 1u, kKey64SentinelBits, kKey64SentinelBits + 1u,
                                   0x7F800000u /* +inf */, 0x7FC00000u, 0xFFC00000u, 0x7FFFFFFFu, 0x80000000u, 0xFF800000u,
                                   0xFFFFFFFFu};
static const unsigned kEdgeJ[] = {0u, 1u, 0xFFFFFFFFu, 0x7FFFFFFFu, 0x80000000u, 4499u};

static Cand draw(const Cand *seen, int nseen)
{
    const unsigned r = (unsigned)(rnd() % 100);
    Cand c;
    c.live = true;
    if (r < 10 && nseen > 0) return seen[rnd() % nseen];                      // a repeated word
    if (r < 35) {
        c.dbits = kEdgeHi[rnd() % (sizeof(kEdgeHi) / sizeof(kEdgeHi[0]))];
        c.j = (rnd() & 1) ? kEdgeJ[rnd() % (sizeof(kEdgeJ) / sizeof(kEdgeJ[0]))] : (unsigned)rnd();
    } else if (r < 40) {
        c.dbits = (unsigned)rnd(); c.j = (unsigned)rnd(); c.live = false;        // an exhausted lane: ~0 before, never inserted
    } else if (r < 55) {
        c.dbits = (unsigned)rnd(); c.j = (unsigned)rnd();                        // any pattern (mostly beyond the sentinel)
    } else if (r < 70) {
        c.dbits = (unsigned)(rnd() % 4); c.j = (unsigned)(rnd() % 8);            // few distinct words: ties on d, on (d, j)
    } else {
        c.dbits = (unsigned)(rnd() % kKey64SentinelBits); c.j = (unsigned)rnd() % 70000u;
    }
    return c;
}

template <int KP>
static int fuzz(int trials)
{
    for (int t = 0; t < trials; ++t) {
        u64 ref[KP];
        double kk[KP];
        for (int p = 0; p < KP; ++p) { ref[p] = kKey64Empty; kk[p] = key64_as_double(kKey64Empty); }
        const int n = (int)(rnd() % (3 * KP + 1));       // 0 .. 3 KP candidates: empty, partly empty and full lists
        Cand seen[3 * KP + 1];
        for (int i = 0; i < n; ++i) {
            const Cand c = draw(seen, i);
            seen[i] = c;
            // the compare / select form, as it stood in csrc/knn_filter.h
            const u64 nk = c.live ? (((u64)c.dbits << 32) | c.j) : ~0ull;
            bool g[KP];
            for (int p = 0; p < KP; ++p) g[p] = ref[p] > nk;
            for (int p = KP - 1; p >= 1; --p) ref[p] = g[p - 1] ? ref[p - 1] : (g[p] ? nk : ref[p]);
            ref[0] = g[0] ? nk : ref[0];
            key64_insert<KP>(kk, key64_word(c.dbits, c.j, c.live));
            for (int p = 0; p < KP; ++p) {
                if (key64_as_word(kk[p]) != ref[p]) {
                    printf("KP=%d trial %d candidate %d (dbits %08x j %08x live %d): slot %d is %016llx, expected %016llx\n", KP, t,
                           i, c.dbits, c.j, (int)c.live, p, key64_as_word(kk[p]), ref[p]);
                    return 1;
                }
            }
        }
    }
    return 0;
}

int main(int argc, char **argv)
{
    const int trials = argc > 1 ? atoi(argv[1]) : 20000;
    if (fuzz<8>(trials) || fuzz<16>(trials) || fuzz<20>(trials)) return 1;
    printf("ok %d trials x 3 list lengths\n", trials);
    return 0;
}

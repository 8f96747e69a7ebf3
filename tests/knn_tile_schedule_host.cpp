// Host check of csrc/knn_tile_schedule.h (built and run by tests/test_knn_tile_schedule_host.py): the tile-index schedule of
// the second kNN filter form's sweeps, walked the way the kernel walks it (csrc/knn_filter.h).
//   four_set_sweep   f2_sweep4: the four first tiles are requested, the first tile's products are issued, and call i
//                    loads tile i + 4 into set i & 3 and then issues the products of tile i + 1 from set (i + 1) & 3
//   plain_sweep      f2_sweep with two sets: A = first tile, its products, A = second tile; call i loads tile i + 2 into
//                    the set that call i - 1 used and issues the products of tile i + 1 from the other
// For every range: each tile is loaded exactly once before the call that issues its products, into a set that is not
// waiting to be used; every tile lies in the range; only the sweep's last `lead` loads re-read its (clamped) last tile;
// the keys of consecutive tiles use different key blocks; the threshold is converted on the odd calls, as in the
// two-call loop.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "knn_tile_schedule.h"

static int g_fail = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            if (g_fail < 20) {                            \
                std::printf("FAIL %s: ", #cond);          \
                std::printf(__VA_ARGS__);                 \
                std::printf("\n");                        \
            }                                             \
            ++g_fail;                                     \
        }                                                 \
    } while (0)

struct Sets {
    int t_lo, t_hi, nsets;
    std::vector<int> holds;       // tile whose operands the set holds (or is receiving), -1: nothing of use
    std::vector<char> waiting;    // loaded, products not issued yet
    std::vector<int> loads, issued;
    long clamped = 0;

    Sets(int lo, int hi, int n) : t_lo(lo), t_hi(hi), nsets(n), holds(n, -1), waiting(n, 0), loads(hi - lo, 0), issued(hi - lo, 0) {}
    // `fresh`: the load is the first request of its tile (otherwise a clamped re-read of the last tile)
    void load(int set, int tile, bool fresh)
    {
        CHECK(set >= 0 && set < nsets, "set %d", set);
        CHECK(tile >= t_lo && tile < t_hi, "[%d, %d): tile %d", t_lo, t_hi, tile);
        CHECK(!waiting[set], "[%d, %d): tile %d overwrites set %d, which holds %d unused", t_lo, t_hi, tile, set, holds[set]);
        if (fresh) {
            ++loads[tile - t_lo];
            holds[set] = tile;
            waiting[set] = 1;
        } else {
            CHECK(tile == t_hi - 1, "[%d, %d): clamped load fetches tile %d", t_lo, t_hi, tile);
            ++clamped;
            holds[set] = -1;
        }
    }
    void issue(int set, int tile)
    {
        CHECK(holds[set] == tile, "[%d, %d): products of tile %d from set %d, which holds %d", t_lo, t_hi, tile, set, holds[set]);
        CHECK(loads[tile - t_lo] == 1, "[%d, %d): tile %d loaded %d times before its products", t_lo, t_hi, tile, loads[tile - t_lo]);
        ++issued[tile - t_lo];
        waiting[set] = 0;
    }
    void finish(int lead)
    {
        for (int i = 0; i < t_hi - t_lo; ++i) {
            CHECK(loads[i] == 1, "[%d, %d): tile %d loaded %d times", t_lo, t_hi, t_lo + i, loads[i]);
            CHECK(issued[i] == 1, "[%d, %d): products of tile %d issued %d times", t_lo, t_hi, t_lo + i, issued[i]);
        }
        CHECK(clamped == lead, "[%d, %d): %ld clamped loads", t_lo, t_hi, clamped);
    }
};

static void check_call(int i)
{
    CHECK(f2_call_converts(i) == ((i % 2) == 1), "call %d", i);
    CHECK(f2_tile_key_block(i) != f2_tile_key_block(i + 1), "tiles %d and %d share a key block", i, i + 1);
}

static void four_set_sweep(int t_lo, int t_hi)
{
    if (t_lo >= t_hi) return;
    Sets s(t_lo, t_hi, kF2Sets);
    const int len = t_hi - t_lo;
    for (int j = 0; j < kF2Sets; ++j) s.load(f2_tile_set(j), f2_load_tile(t_lo, j, t_hi), j < len);
    s.issue(f2_tile_set(0), t_lo);
    for (int i = 0; i < len; ++i) {
        check_call(i);
        s.load(f2_tile_set(i + kF2Sets), f2_load_tile(t_lo + i, kF2Sets, t_hi), i + kF2Sets < len);
        CHECK(f2_tile_set(i + kF2Sets) == f2_tile_set(i), "call %d loads into set %d", i, f2_tile_set(i + kF2Sets));
        if (i + 1 < len) s.issue(f2_tile_set(i + 1), t_lo + i + 1);
    }
    s.finish(kF2Sets);
}

static void plain_sweep(int t_lo, int t_hi)
{
    if (t_lo >= t_hi) return;
    Sets s(t_lo, t_hi, 2);
    const int len = t_hi - t_lo;
    s.load(0, f2_load_tile(t_lo, 0, t_hi), true);
    s.issue(0, t_lo);
    s.load(0, f2_load_tile(t_lo, 1, t_hi), 1 < len);
    for (int i = 0; i < len; ++i) {
        check_call(i);
        const int use = i & 1, ld = use ^ 1;      // even calls: use A, load B
        s.load(ld, f2_load_tile(t_lo + i, kF2PlainLead, t_hi), i + kF2PlainLead < len);
        if (i + 1 < len) s.issue(use, t_lo + i + 1);
    }
    s.finish(kF2PlainLead);
}

int main()
{
    const int lens[] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 25, 26, 27, 28, 32, 33, 37, 41, 109};
    const int defers[] = {32, 8, 2};     // kF2Defer and two smaller values: short main sweeps in front of short revisits
    long sweeps = 0;
    for (int lo : {0, 41}) {
        for (int n : lens) {
            // a first attempt: deferred / main / revisit, each sweep on its own
            for (int defer : defers) {
                const int nd = n < defer ? n : defer;
                plain_sweep(lo, lo + nd);
                four_set_sweep(lo + nd, lo + n);
                four_set_sweep(lo, lo + nd);
                sweeps += 3;
            }
            // a second attempt: one recording sweep over the range; and the range as a two-set sweep (64 features)
            four_set_sweep(lo, lo + n);
            plain_sweep(lo, lo + n);
            sweeps += 2;
        }
    }
    if (g_fail) {
        std::printf("%d checks failed\n", g_fail);
        return 1;
    }
    std::printf("ok %ld sweeps\n", sweeps);
    return 0;
}

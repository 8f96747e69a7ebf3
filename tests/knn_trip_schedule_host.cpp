// Host check of the trip arithmetic in csrc/knn_tile_schedule.h (built and run by tests/test_knn_trip_schedule_host.py):
// a four-set sweep of the second kNN filter form walked the way f2_sweep4 walks it (csrc/knn_filter.h) -- the first
// four tiles requested, the first tile's products issued, then f2_whole_trips(len) trips of four calls in a loop with
// no exit inside, then f2_remainder_calls(len) calls written out, remainder call r being call f2_remainder_trip_call(r)
// of a trip.  Call q of a trip selects from key block q & 1, loads into set f2_trip_load_set(q), issues the products
// of set f2_trip_use_set(q) and converts the threshold when q is odd.
// For every sweep length from 1 to 200 tiles, from tile 0 and from tile 41:
//   * every tile is visited exactly once and in order, by the call whose index in the sweep is the tile's;
//   * a set is never loaded before the call that issued its products (no load overwrites operands that wait to be
//     used), every tile is loaded exactly once before its products, and only the last four loads re-read the clamped
//     last tile;
//   * the remainder calls continue the set, key-block and conversion rotation of the trips: call i of the sweep, in a
//     trip or after them, uses set i & 3 / (i + 1) & 3, key block i & 1 and converts iff i is odd, as
//     f2_tile_set / f2_tile_key_block / f2_call_converts say for a sweep written as one call after another.
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

struct Walk {
    int t_lo, t_hi;
    int holds[kF2Sets];        // tile whose operands the set holds, -1: nothing of use
    bool waiting[kF2Sets];     // loaded, products not issued yet
    std::vector<int> loads, issued, visited;
    int clamped = 0, calls = 0, prev_key_block = -1;

    Walk(int lo, int hi) : t_lo(lo), t_hi(hi), loads(hi - lo, 0), issued(hi - lo, 0), visited(hi - lo, 0)
    {
        for (int j = 0; j < kF2Sets; ++j) {
            holds[j] = -1;
            waiting[j] = false;
        }
    }
    void load(int set, int tile, bool fresh)
    {
        CHECK(set >= 0 && set < kF2Sets, "set %d", set);
        CHECK(tile >= t_lo && tile < t_hi, "[%d, %d): tile %d", t_lo, t_hi, tile);
        if (set < 0 || set >= kF2Sets || tile < t_lo || tile >= t_hi) return;
        CHECK(!waiting[set], "[%d, %d): tile %d overwrites set %d, which holds %d unused", t_lo, t_hi, tile, set, holds[set]);
        if (fresh) {
            ++loads[tile - t_lo];
            holds[set] = tile;
            waiting[set] = true;
        } else {
            CHECK(tile == t_hi - 1, "[%d, %d): clamped load fetches tile %d", t_lo, t_hi, tile);
            ++clamped;
            holds[set] = -1;
        }
    }
    void issue(int set, int tile)
    {
        if (set < 0 || set >= kF2Sets || tile < t_lo || tile >= t_hi) {
            CHECK(false, "[%d, %d): products of tile %d from set %d", t_lo, t_hi, tile, set);
            return;
        }
        CHECK(holds[set] == tile, "[%d, %d): products of tile %d from set %d, which holds %d", t_lo, t_hi, tile, set, holds[set]);
        CHECK(loads[tile - t_lo] == 1, "[%d, %d): tile %d loaded %d times before its products", t_lo, t_hi, tile, loads[tile - t_lo]);
        ++issued[tile - t_lo];
        waiting[set] = false;
    }
    // call q of a trip at tile t, as f2_sweep4 writes it
    void call(int q, int t)
    {
        const int i = t - t_lo;     // the call's index in the sweep
        CHECK(q >= 0 && q < kF2Sets, "trip call %d", q);
        CHECK(t >= t_lo && t < t_hi, "[%d, %d): call at tile %d", t_lo, t_hi, t);
        if (t < t_lo || t >= t_hi) return;
        CHECK(i == calls, "[%d, %d): tile %d visited by call %d", t_lo, t_hi, t, calls);
        ++visited[i];
        ++calls;
        // the rotation of a sweep written as one call after another
        CHECK(f2_trip_load_set(q) == f2_tile_set(i), "call %d (trip call %d) loads into set %d", i, q, f2_trip_load_set(q));
        CHECK(f2_trip_use_set(q) == f2_tile_set(i + 1), "call %d (trip call %d) issues from set %d", i, q, f2_trip_use_set(q));
        CHECK(f2_tile_key_block(q) == f2_tile_key_block(i), "call %d (trip call %d): key block", i, q);
        CHECK(f2_call_converts(q) == ((i % 2) == 1), "call %d (trip call %d): conversion", i, q);
        CHECK(f2_tile_key_block(q) != prev_key_block, "calls %d and %d share a key block", i - 1, i);
        prev_key_block = f2_tile_key_block(q);
        // the keys this call selects from are tile t's: their products were issued by the call before (or the prologue)
        CHECK(issued[i] == 1, "[%d, %d): call at tile %d before its products", t_lo, t_hi, t);
        load(f2_trip_load_set(q), f2_load_tile(t, kF2Sets, t_hi), i + kF2Sets < t_hi - t_lo);
        if (t + 1 < t_hi) issue(f2_trip_use_set(q), t + 1);
    }
    void finish()
    {
        const int len = t_hi - t_lo;
        CHECK(calls == len, "[%d, %d): %d calls", t_lo, t_hi, calls);
        for (int i = 0; i < len; ++i) {
            CHECK(visited[i] == 1, "[%d, %d): tile %d visited %d times", t_lo, t_hi, t_lo + i, visited[i]);
            CHECK(loads[i] == 1, "[%d, %d): tile %d loaded %d times", t_lo, t_hi, t_lo + i, loads[i]);
            CHECK(issued[i] == 1, "[%d, %d): products of tile %d issued %d times", t_lo, t_hi, t_lo + i, issued[i]);
        }
        CHECK(clamped == kF2Sets, "[%d, %d): %d clamped loads", t_lo, t_hi, clamped);
    }
};

static void trip_sweep(int t_lo, int t_hi)
{
    const int len = t_hi - t_lo;
    Walk w(t_lo, t_hi);
    for (int j = 0; j < kF2Sets; ++j) w.load(f2_tile_set(j), f2_load_tile(t_lo, j, t_hi), j < len);
    w.issue(f2_tile_set(0), t_lo);
    const int trips = f2_whole_trips(len), rem = f2_remainder_calls(len);
    CHECK(trips >= 0 && rem >= 0 && rem < kF2Sets && trips * kF2Sets + rem == len, "len %d: %d trips + %d calls", len, trips, rem);
    int t = t_lo;
    for (int n = 0; n < trips; ++n, t += kF2Sets)
        for (int q = 0; q < kF2Sets; ++q) w.call(q, t + q);
    for (int r = 0; r < rem; ++r) w.call(f2_remainder_trip_call(r), t + r);
    w.finish();
}

int main()
{
    long sweeps = 0;
    CHECK(f2_whole_trips(0) == 0 && f2_remainder_calls(0) == 0, "an empty sweep");
    CHECK(f2_whole_trips(-3) == 0 && f2_remainder_calls(-3) == 0, "a sweep with t_hi < t_lo");
    for (int lo : {0, 41})
        for (int len = 1; len <= 200; ++len) {
            trip_sweep(lo, lo + len);
            ++sweeps;
        }
    if (g_fail) {
        std::printf("%d checks failed\n", g_fail);
        return 1;
    }
    std::printf("ok %ld sweeps\n", sweeps);
    return 0;
}

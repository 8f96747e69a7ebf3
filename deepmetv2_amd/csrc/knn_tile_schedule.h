// knn_tile_schedule.h -- which candidate tile every call of a sweep of the second filter form loads, and which operand
// set and key block a tile uses.  One definition for the kernel (knn_filter.h: f2_sweep, f2_sweep4) and for the host
// test (tests/knn_tile_schedule_host.cpp): plain C++, no device code, no other header.
//
// A sweep visits the tiles [t_lo, t_hi) in order; tile t_lo + i is its call i.  Call i selects from the keys of tile i,
// issues the matrix products of tile i + 1 and loads tile i + lead, clamped to the sweep's last tile: the last `lead`
// calls re-read that tile (never used).
//   * The recording sweeps at 32 features (main, revisit, second attempt; f2_sweep4) rotate FOUR operand sets: tile i
//     lives in set i & 3, lead = 4, and a sweep requests its first four tiles before its first call.  Call i therefore
//     loads into set i & 3, whose products the call before it issued: no set is overwritten while it waits to be used.
//     (The deferred pass too in a -DDMET_F2_DEFER_FOUR build: measured slower in r10, not the default.)
//   * Every other sweep (the deferred pass, 64 features; f2_sweep) has two sets and lead = 2.
// The keys of tile i go to key block i & 1, and the threshold is converted on the odd calls.
// A four-set sweep runs as whole TRIPS of four calls -- a loop with no exit inside a trip -- followed by its zero to
// three remaining calls, written out: f2_whole_trips, f2_remainder_calls, f2_remainder_trip_call.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DMET_SCHED_FN __host__ __device__ inline
#else
#define DMET_SCHED_FN inline
#endif

constexpr int kF2Sets = 4;    // operand sets of a recording sweep at 32 features; its calls load this many tiles ahead
constexpr int kF2PlainLead = 2;

// the tile that the call at tile t of the sweep [.., t_hi) loads (lead = 0 .. : also the tiles a sweep starts with)
DMET_SCHED_FN constexpr int f2_load_tile(int t, int lead, int t_hi) { return t + lead < t_hi - 1 ? t + lead : t_hi - 1; }

// tile i of a four-set sweep: its operand set, and (any sweep) the key block its keys go to
DMET_SCHED_FN constexpr int f2_tile_set(int i) { return i & (kF2Sets - 1); }
DMET_SCHED_FN constexpr int f2_tile_key_block(int i) { return i & 1; }
// call i converts the threshold it has just updated: every second one
DMET_SCHED_FN constexpr bool f2_call_converts(int i) { return (i & 1) != 0; }

// A four-set sweep of `len` tiles: its whole trips (kF2Sets calls each: calls 0 .. kF2Sets * trips - 1), the calls that
// remain after them, and the call of a trip -- its operand sets, key blocks and conversion -- that remainder call r
// (0 .. f2_remainder_calls - 1; call kF2Sets * trips + r of the sweep) is: the rotation goes on where the trips left it.
DMET_SCHED_FN constexpr int f2_whole_trips(int len) { return len > 0 ? len / kF2Sets : 0; }
DMET_SCHED_FN constexpr int f2_remainder_calls(int len) { return len > 0 ? len & (kF2Sets - 1) : 0; }
DMET_SCHED_FN constexpr int f2_remainder_trip_call(int r) { return r & (kF2Sets - 1); }
// call q of a trip (0 .. kF2Sets - 1): the set it loads into and the set whose products it issues
DMET_SCHED_FN constexpr int f2_trip_load_set(int q) { return f2_tile_set(q); }
DMET_SCHED_FN constexpr int f2_trip_use_set(int q) { return f2_tile_set(q + 1); }

// knn.hip -- K1: kNN graph build over ragged events (gfx950).  (The radius graph, N1, is radius.hip.)
//
// Replaces torch_cluster.knn_graph / knn (call sites /root/reference/model/graph_met_network.py:63,
// model/dynamic_reduction_network.py:86,94).  Results are bit-identical to oracle/dmet_oracle.c:
//   R1  d(i,j) = chain of fmaf(diff, diff, acc) over the feature index, fp32, diff = x[j,c]-x[i,c]
//   R2  top-k by (d, j) lexicographic order == upstream's strict-'>' insertion in ascending j
// R1 / R2 define the RESULT, not the work done on pairs that cannot win.  Three paths, one stream, no host sync:
//   * D = 32 (the model's shape) or 64 (the DRN's), k <= 20: a matrix-core FILTER ranks all pairs approximately
//     (key = |x_j|^2 - 2 x_i.x_j), keeps a certified superset of every query's neighbours, and only those go through
//     the exact R1 chain and the (d, j) order.  Second form (filter2_wave, events of 2048..65536 nodes): single-term
//     fp16 operands on v_mfma_f32_32x32x16_f16 (2 MFMAs per 32 x 32 block and 32 features; the certificate carries the
//     fp16 rounding), per-tile hit masks, threshold from tile minima, a second in-wavefront sweep for queries that
//     miss the certificate by the slack alone; first form (filter1_wave): bf16 split x = h + m on
//     v_mfma_f32_32x32x16_bf16 (6 MFMAs per block), per-key queue; one launch (knn_filter12_kernel), each wavefront
//     takes the form its event calls for.  A query whose certificate does not hold is recomputed exactly.
//   * everything else, and the recomputation: the exact kernel below (knn_kernel).
//
// The exact kernel is fp32-VALU bound (a subtract and an fma per (query, candidate, feature); the difference form
// cannot go to the matrix cores without changing the rounding).  Measured on MI355X (tools/valu_micro.hip) this
// instruction mix saturates at ~75-80 TFLOP/s (3 flop per element) and needs packed math plus >= 3 wavefronts per
// SIMD to get there, which shapes the design:
//   * a work item = one 64-lane wavefront (workgroups are 4 independent wavefronts); every lane OWNS 2 query nodes
//     whose features sit in registers as float2 pairs, so the inner loop is v_pk_add_f32 / v_pk_fma_f32 (each half
//     is an exact IEEE op: same bits);
//   * candidate rows are staged into LDS in tiles and read back as wave-uniform (broadcast) ds_read_b128; two
//     candidates are in flight per iteration (two independent fma chains per lane);
//   * selection is deferred: a lane whose distance beats its current k-th best appends (d, j) to its private LDS
//     queue; when any lane's queue is nearly full the whole wave drains its queues into the sorted top-k lists,
//     which live in an L2-resident global workspace between drains (keeps VGPRs for the distance loop);
//   * query tiles never straddle events (a straddling wavefront would sweep two events: a 2x straggler); the
//     tile -> event map is a device-side plan (no host sync), events ordered longest first;
//   * load balance: with T tiles on S SIMDs the last (T mod S) tiles would leave most of the chip idle for a whole
//     sweep.  Those tail tiles are split over the candidate range into `split` sub-sweeps (dispatched last) whose
//     partial top-k lists a small merge kernel combines.
#include <stdlib.h>

#include "common.h"
#include "knn_common.h"
#include "knn_key64.h"
#include "knn_tile_schedule.h"
#include "nls_body.h"

namespace dmet {
namespace {

constexpr int kTileC = 32;   // candidates per LDS tile
constexpr int kQMax = 8;     // per-lane pending queue capacity
constexpr int kMaxSplit = 8; // tail tiles are split into at most this many candidate sub-sweeps
constexpr int kWavesPerGroup = 4;  // independent wavefronts per workgroup (one per SIMD of the CU)

// Four features x two candidates (A, B) x the lane's two queries in ONE asm block of 8 v_pk_add_f32 + 8 v_pk_fma_f32.
//   v_pk_add_f32 t, cand_pair, q  op_sel -> (c, c) + (-q.x, -q.y): the candidate feature is the low or high half of a
//   register pair, broadcast to both result halves with op_sel/op_sel_hi; the query pair is negated with neg_lo/neg_hi
//   (c + (-q) is the same IEEE result as c - q).
// Why asm: hipcc materialises every broadcast pair with v_mov (49 extra VALU per 128 useful ones) and serialises the
// fma chains behind the packed-fp32 RAW wait state; here each accumulator's chain stays in feature order (R1) and
// dependent packed ops are always separated by an independent one.
#define DMET_PKSUB_LO " op_sel:[0,0] op_sel_hi:[0,1] neg_lo:[0,1] neg_hi:[0,1]\n\t"
#define DMET_PKSUB_HI " op_sel:[1,0] op_sel_hi:[1,1] neg_lo:[0,1] neg_hi:[0,1]\n\t"
__device__ __forceinline__ void pk_dist_step4(f2 &accA, f2 &accB, f2 vxy, f2 vzw, f2 wxy, f2 wzw, f2 q0, f2 q1, f2 q2,
                                              f2 q3)
{
    f2 t0, t1, t2, t3;
    asm("v_pk_add_f32 %[t0], %[vxy], %[q0]" DMET_PKSUB_LO
        "v_pk_add_f32 %[t1], %[wxy], %[q0]" DMET_PKSUB_LO
        "v_pk_add_f32 %[t2], %[vxy], %[q1]" DMET_PKSUB_HI
        "v_pk_add_f32 %[t3], %[wxy], %[q1]" DMET_PKSUB_HI
        "v_pk_fma_f32 %[a], %[t0], %[t0], %[a]\n\t"
        "v_pk_fma_f32 %[b], %[t1], %[t1], %[b]\n\t"
        "v_pk_add_f32 %[t0], %[vzw], %[q2]" DMET_PKSUB_LO
        "v_pk_add_f32 %[t1], %[wzw], %[q2]" DMET_PKSUB_LO
        "v_pk_fma_f32 %[a], %[t2], %[t2], %[a]\n\t"
        "v_pk_fma_f32 %[b], %[t3], %[t3], %[b]\n\t"
        "v_pk_add_f32 %[t2], %[vzw], %[q3]" DMET_PKSUB_HI
        "v_pk_add_f32 %[t3], %[wzw], %[q3]" DMET_PKSUB_HI
        "v_pk_fma_f32 %[a], %[t0], %[t0], %[a]\n\t"
        "v_pk_fma_f32 %[b], %[t1], %[t1], %[b]\n\t"
        "v_pk_fma_f32 %[a], %[t2], %[t2], %[a]\n\t"
        "v_pk_fma_f32 %[b], %[t3], %[t3], %[b]"
        : [a] "+v"(accA), [b] "+v"(accB), [t0] "=&v"(t0), [t1] "=&v"(t1), [t2] "=&v"(t2), [t3] "=&v"(t3)
        : [vxy] "v"(vxy), [vzw] "v"(vzw), [wxy] "v"(wxy), [wzw] "v"(wzw), [q0] "v"(q0), [q1] "v"(q1), [q2] "v"(q2),
          [q3] "v"(q3));
}

// The periodic kNN sweep (knn_kernel with Per = RadPeriod) takes one coordinate at a time: the candidate feature is
// broadcast and the query pair subtracted as in pk_dist_step4 (tA / tB: candidates A / B), a periodic coordinate is then
// wrapped half by half, and the squares enter the two chains in coordinate order (R1).
template <bool HI>
__device__ __forceinline__ void pk_sub2(f2 &tA, f2 &tB, f2 v, f2 w, f2 q)
{
    if (HI)
        asm("v_pk_add_f32 %[ta], %[v], %[q]" DMET_PKSUB_HI "v_pk_add_f32 %[tb], %[w], %[q]" DMET_PKSUB_HI
            : [ta] "=&v"(tA), [tb] "=&v"(tB) : [v] "v"(v), [w] "v"(w), [q] "v"(q));
    else
        asm("v_pk_add_f32 %[ta], %[v], %[q]" DMET_PKSUB_LO "v_pk_add_f32 %[tb], %[w], %[q]" DMET_PKSUB_LO
            : [ta] "=&v"(tA), [tb] "=&v"(tB) : [v] "v"(v), [w] "v"(w), [q] "v"(q));
}

__device__ __forceinline__ void pk_fma2(f2 &accA, f2 &accB, f2 tA, f2 tB)
{
    asm("v_pk_fma_f32 %[a], %[ta], %[ta], %[a]\n\t"
        "v_pk_fma_f32 %[b], %[tb], %[tb], %[b]"
        : [a] "+v"(accA), [b] "+v"(accB) : [ta] "v"(tA), [tb] "v"(tB));
}

// min(|d|, L - |d|) of one fp32 lane (RadPeriod above).  v_sub_f32 / v_min_f32 with abs source modifiers: gfx950 has
// no packed fp32 min, and fminf on an asm result would add canonicalising v_max_f32s.
__device__ __forceinline__ float wrap1(float d, float L)
{
    float a, t;
    asm("v_sub_f32 %[t], %[L], |%[d]|\n\t"
        "v_min_f32 %[a], |%[d]|, %[t]"
        : [a] "=v"(a), [t] "=&v"(t) : [d] "v"(d), [L] "s"(L));
    return a;
}

// One coordinate of the periodic sweep for candidates A (v) and B (w).  `wrap` (L < inf) is wave-uniform: a plain or
// padding coordinate branches around the 8 wrap instructions (the compiler adds two 64-bit moves on that side).
template <bool HI>
__device__ __forceinline__ void pk_dist_step1_per(f2 &accA, f2 &accB, f2 v, f2 w, f2 q, float L, bool wrap)
{
    f2 tA, tB;
    pk_sub2<HI>(tA, tB, v, w, q);
    if (wrap) {
        tA = f2{wrap1(tA.x, L), wrap1(tA.y, L)};
        tB = f2{wrap1(tB.x, L), wrap1(tB.y, L)};
    }
    pk_fma2(accA, accB, tA, tB);
}

template <int DP, int TQ>
struct KnnShared {
    float4 tile[(kTileC + 1) * DP / 4];  // +1 row kept at +inf: the paired sweep reads one row past the tile's last
    uint2 queue[TQ][kQMax][kWave];
};

// Drain a lane-private queue into the sorted list of the lane's query (list kept in ws between drains).
// Returns the lane's new admission threshold (its k-th best distance).
template <int KP>
__device__ __attribute__((noinline)) float drain_queue(const uint2 (*queue)[kWave], int lane, int cnt, bool fresh,
                                                       bool valid, float *__restrict__ ld,
                                                       int32_t *__restrict__ lj)
{
    float d[KP];
    int32_t j[KP];
    if (fresh || !valid) {
#pragma unroll
        for (int p = 0; p < KP; ++p) { d[p] = kKnnSentinel; j[p] = -1; }
    } else {
#pragma unroll
        for (int p = 0; p < KP; p += 4) {
            const float4 v = *reinterpret_cast<const float4 *>(ld + p);
            const int4 w = *reinterpret_cast<const int4 *>(lj + p);
            d[p] = v.x; d[p + 1] = v.y; d[p + 2] = v.z; d[p + 3] = v.w;
            j[p] = w.x; j[p + 1] = w.y; j[p + 2] = w.z; j[p + 3] = w.w;
        }
    }
    int maxcnt = cnt;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) maxcnt = max(maxcnt, __shfl_xor(maxcnt, off, 64));
    for (int s = 0; s < maxcnt; ++s) {
        if (s < cnt) {
            const uint2 e = queue[s][lane];
            const float nd = __uint_as_float(e.x);
            const int32_t nj = (int32_t)e.y;
            if (nd < d[KP - 1]) {
                // sorted insert; first position with d[p] > nd (strict) takes the new entry (R2)
#pragma unroll
                for (int p = KP - 1; p >= 1; --p) {
                    const bool mq = d[p - 1] > nd;
                    const bool mp = d[p] > nd;
                    const float dn = mq ? d[p - 1] : (mp ? nd : d[p]);
                    const int32_t jn = mq ? j[p - 1] : (mp ? nj : j[p]);
                    d[p] = dn;
                    j[p] = jn;
                }
                if (d[0] > nd) { d[0] = nd; j[0] = nj; }
            }
        }
    }
    if (valid) {
#pragma unroll
        for (int p = 0; p < KP; p += 4) {
            *reinterpret_cast<float4 *>(ld + p) = make_float4(d[p], d[p + 1], d[p + 2], d[p + 3]);
            *reinterpret_cast<int4 *>(lj + p) = make_int4(j[p], j[p + 1], j[p + 2], j[p + 3]);
        }
    }
    return d[KP - 1];
}

#ifdef DMET_KNN_STAMP
// experiment only (tools/knn_trace.hip): per-workgroup start/end realtime stamps and hardware placement
__device__ unsigned long long g_knn_stamps[1 << 16][4];
#endif

// events the second matrix-core filter form sweeps (filter2_wave); the plan counts the others
// Smaller events take the first form: the threshold of the second form is the M-th smallest of the event's tile minima (M = 22
// tiles = 704 nodes at least), and below ~800 nodes the first form is the faster one (tools/knn_small_events.py: 64 events
// of 704 nodes 155 us against 241, of 800 nodes 168 against 133, of 1000 nodes 188 against 109, of 2000 nodes 265 against 140).
// Until round 3 the boundary stood at 2048 -- twice the build time for events of 1000..2047 nodes.
#ifndef DMET_F2_MIN_NODES
#define DMET_F2_MIN_NODES 800
#endif
constexpr int kF2MinNodes = DMET_F2_MIN_NODES;
constexpr int kFilterMaxSplit = 2;  // tail balancing of the filter: at most 2 candidate sub-sweeps (the re-rank assumes 2).
#ifndef DMET_F2_SPLIT_MIN_NODES
#define DMET_F2_SPLIT_MIN_NODES 2560
#endif
constexpr int kF2SplitMinNodes = DMET_F2_SPLIT_MIN_NODES;   // smaller second-form events are never cut into candidate sub-sweeps (see filter2_wave)
constexpr int kF2MaxNodes = 65536;  // tile number must fit 11 bits

// Device-side launch plan (no host synchronisation): tiles never straddle events, so tile -> event needs a prefix.
struct KnnPlan {
    int total_tiles;   // sum_b ceil(n_b / tile_queries)
    int n_full;        // tiles 0..n_full-1 sweep their whole event in one workgroup
    int split;         // tiles n_full.. are cut into `split` candidate sub-sweeps each (tail balancing)
    int form1_events;  // non-empty events outside the second filter form's size range (its kernels exit at once if 0)
};

struct KnnArgs {
    const float *x;
    const int64_t *ptr;
    int B;
    int64_t N;
    int D, k;
    int32_t *nbr;
    float *dist;
    uint16_t *nbr16;       // optional [N][k]: the same table as event-local ids (0xFFFF = none; meaningful for events
                           // of at most 65535 nodes)
    float *wsd;            // [N][KP] running lists of whole-sweep tiles
    int32_t *wsj;
    const KnnPlan *plan;
    const int32_t *order;     // [B] events longest first
    const int32_t *tile_ptr;  // [B+1] exclusive prefix of per-position tile counts
    float *psd;            // [(tile-n_full)*tile_queries + slot][split][KP] partial lists of split tiles
    int32_t *psj;
    const int32_t *flags;  // optional [tiles] = number of uncertified queries per tile (matrix-core path): only
    int flag_min;          // tiles with flags[tile] >= flag_min are computed here
    const int32_t *any;    // optional: total number of uncertified queries (0: nothing to do for any workgroup)
    // per-query fallback of the matrix-core path, run by the first requery_groups workgroups of the same launch (32
    // features): the flagged queries in flagging order, the event -> position map of the plans, queries per exact tile
    const int32_t *qlist;
    const int32_t *pos_of;
    int requery_groups;
    int requery_tile_queries;
};

__device__ __forceinline__ uint16_t local_id16(int32_t j, int ev_lo)
{
    return (uint16_t)(j >= 0 ? (unsigned)(j - ev_lo) : 0xFFFFu);
}

// One workgroup: events ordered LONGEST FIRST (a tile of an n-node event costs n candidates, so big events go out
// first and the split tail consists of the smallest ones), per-position tile counts -> exclusive prefix, then the
// tail-splitting plan for `simds` SIMDs: whole sweeps for the largest multiple of the SIMD count, the remaining
// tiles cut into sub-sweeps.  order[p] = event at position p; tile_ptr is indexed by position.
constexpr int kMaxSortedEvents = 4096;  // beyond this the O(B^2) ranking is skipped (identity order)

struct KnnPlanOut {
    int tile_queries, simds, max_split;
    int32_t *order, *pos_of, *tile_ptr;
    KnnPlan *plan;
};

// Event order of the plans.  Ranks are by size, longest first.  Workgroups are dealt round-robin over the 8 XCDs
// (each with its own L2), and the matrix-core filter maps each XCD's workgroups to ONE contiguous eighth of the tile
// list so that the tiles of an event -- which all sweep the same candidate records -- run on one XCD and re-read them
// from its L2 (the records of a batch do not fit any L2: left to round-robin every sweep comes from the Infinity
// Cache).  For the eighths to carry equal work on ragged batches the ranks are dealt to 8 bins in snake order
// (0..7, 7..0, ...) and the bins concatenated: every bin, hence every XCD, gets the same mix of event sizes and still
// runs its own events longest first.  Small batches keep the plain order.
__device__ __forceinline__ int xcd_dealt_position(int rank, int B)
{
    if (B < 4 * kNumXcd) return rank;
    const int c = rank % (2 * kNumXcd), g = rank / (2 * kNumXcd);
    const int bin = c < kNumXcd ? c : 2 * kNumXcd - 1 - c;
    const int idx = 2 * g + (c >= kNumXcd ? 1 : 0);
    const int rem = B % (2 * kNumXcd), full = B / (2 * kNumXcd);
    int start = 0;
    for (int b = 0; b < bin; ++b)      // sizes of the earlier bins
        start += 2 * full + (b < min(rem, kNumXcd) ? 1 : 0) + ((rem > kNumXcd && b > 2 * kNumXcd - 1 - rem) ? 1 : 0);
    return start + idx;
}

// blockIdx.x selects one of up to two plans (exact kernel: 128-query tiles; matrix-core filter: 64-query tiles)
// XY (dmet_knn_xy_f32): `ptr` cuts the QUERIES into tiles and `cptr` holds the candidates of the same events.  A tile
// sweeps its event's nx candidates whatever number of queries it holds, so "longest first" ranks the events by nx
// (ties: more queries first); tiles (from ny) times sweep length (nx) is the event's pair count.  The tail is cut into
// sub-sweeps when the events that have queries hold 512 candidates on average.
template <bool XY = false>
__device__ __forceinline__ void knn_plan_body(const int64_t *__restrict__ ptr, int B, const KnnPlanOut &o,
                                              const int64_t *__restrict__ cptr = nullptr)
{
    const int tile_queries = o.tile_queries, simds = o.simds, max_split = o.max_split;
    int32_t *__restrict__ order = o.order, *__restrict__ pos_of = o.pos_of, *__restrict__ tile_ptr = o.tile_ptr;
    KnnPlan *__restrict__ plan = o.plan;
    __shared__ int part[256];
    const int tid = threadIdx.x;
    if (B <= kMaxSortedEvents) {
        for (int b = tid; b < B; b += 256) {
            const int64_t nb = ptr[b + 1] - ptr[b];
            int rank = 0;
            if constexpr (XY) {
                const int64_t xb = nb > 0 ? cptr[b + 1] - cptr[b] : -1;     // events without queries go last: no tiles
                for (int c = 0; c < B; ++c) {
                    const int64_t nc = ptr[c + 1] - ptr[c];
                    const int64_t xc = nc > 0 ? cptr[c + 1] - cptr[c] : -1;
                    rank += (xc > xb || (xc == xb && (nc > nb || (nc == nb && c < b)))) ? 1 : 0;
                }
            } else {
                for (int c = 0; c < B; ++c) {
                    const int64_t nc = ptr[c + 1] - ptr[c];
                    rank += (nc > nb || (nc == nb && c < b)) ? 1 : 0;
                }
            }
            const int p = xcd_dealt_position(rank, B);
            order[p] = b;
            pos_of[b] = p;
        }
    } else {
        for (int b = tid; b < B; b += 256) { order[b] = b; pos_of[b] = b; }
    }
    __syncthreads();
    const int chunk = (B + 255) / 256;
    const int lo = min(B, tid * chunk), hi = min(B, lo + chunk);
    int sum = 0, nf1 = 0;
    for (int p = lo; p < hi; ++p) {
        const int b = order[p];
        const int64_t nb = ptr[b + 1] - ptr[b];
        sum += (int)((nb + tile_queries - 1) / tile_queries);
        nf1 += (nb > 0 && !(nb >= kF2MinNodes && nb <= kF2MaxNodes)) ? 1 : 0;
    }
    // XY: candidates of the events that have queries, and the number of such events (for the tail rule below)
    __shared__ unsigned long long xy_cand;
    __shared__ int xy_events;
    if constexpr (XY) {
        if (tid == 0) { xy_cand = 0ull; xy_events = 0; }
        __syncthreads();
        unsigned long long cand = 0ull;
        int evs = 0;
        for (int p = lo; p < hi; ++p) {
            const int b = order[p];
            if (ptr[b + 1] > ptr[b]) { cand += (unsigned long long)(cptr[b + 1] - cptr[b]); ++evs; }
        }
        if (evs) { atomicAdd(&xy_cand, cand); atomicAdd(&xy_events, evs); }   // integer sums: order does not matter
    }
    // exclusive prefix of the per-thread tile counts and the number of first-form events: wavefront scans + four
    // wavefront totals (a serial walk of thread 0 over 256 LDS cells was a third of the prep launch: it sits on the
    // critical path of every build)
    __shared__ int wave_tot[4], wave_f1[4];
    const int lane = tid & 63, wv = tid >> 6;
    int incl = sum, f1 = nf1;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(incl, off, 64);
        if (lane >= off) incl += t;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) f1 += __shfl_xor(f1, off, 64);
    if (lane == 63) wave_tot[wv] = incl;
    if (lane == 0) wave_f1[wv] = f1;
    __syncthreads();
    int base = 0;
    for (int w = 0; w < wv; ++w) base += wave_tot[w];
    part[tid] = base + incl - sum;
    if (tid == 0) {
        const int form1_events = wave_f1[0] + wave_f1[1] + wave_f1[2] + wave_f1[3];
        const int tiles = wave_tot[0] + wave_tot[1] + wave_tot[2] + wave_tot[3];
        int n_full = tiles, split = 1;
        // the tiles beyond the last full round of `simds` -- ALL tiles when the batch is small -- are cut into
        // candidate sub-sweeps so that they still fill the chip (unless the events are so small that a sub-sweep
        // would be a handful of candidates)
        const int full = (tiles / simds) * simds;
        const int rem = tiles - full;
        bool cut = rem > 0;
        if constexpr (XY) cut = cut && xy_events > 0 && xy_cand >= 512ull * (unsigned long long)xy_events;
        else cut = cut && B > 0 && (ptr[B] - ptr[0]) >= (int64_t)512 * B;
        if (cut) {
            int f = simds / rem;
            if (f > max_split) f = max_split;
            if (f >= 2) { n_full = full; split = f; }
        }
        plan->total_tiles = tiles; plan->n_full = n_full; plan->split = split; plan->form1_events = form1_events;
        tile_ptr[B] = tiles;
    }
    __syncthreads();
    int run = part[tid];
    for (int p = lo; p < hi; ++p) {
        const int b = order[p];
        tile_ptr[p] = run;
        run += (int)((ptr[b + 1] - ptr[b] + tile_queries - 1) / tile_queries);
    }
    // When does cutting the tail's sweeps in two pay for SECOND-form events?  Each half has its own threshold from half
    // the tile minima (looser: more candidates to re-rank, a fixed cost per piece), so it pays only while the pieces
    // find idle SIMDs -- few tail tiles -- and the halves still have a threshold to speak of -- large events
    // (tools/knn_small_events.py, 2048 wavefront slots: 376 tiles of 3000-node events 106 us split / 154 whole, 568
    // tiles of 4500-node events 132 / 188, but 512 tiles of 2048-node events 115 / 106, 752 tiles of 3000-node events
    // 127 / 119, 1024 tiles of 2048-node events 140 / 118).  The tail holds the SMALLEST events (longest-first order),
    // so its first tile's event bounds them all.  First-form tails (events below kF2MinNodes) and the exact kernel's
    // plan keep the rule above.
    if (o.max_split == kFilterMaxSplit) {
        __syncthreads();
        if (tid == 0 && plan->split > 1) {
            const int first_tail = plan->n_full, rem = plan->total_tiles - plan->n_full;
            int plo = 0, phi = B;
            while (phi - plo > 1) {
                const int mid = (plo + phi) >> 1;
                if (tile_ptr[mid] <= first_tail) plo = mid; else phi = mid;
            }
            const int b = order[plo];
            const int64_t nb = ptr[b + 1] - ptr[b];
            // (the tile-count bound only for a batch that is ALL tail: behind full rounds -- 64 events of 3000 nodes, 960
            // tail tiles -- the halves still win, 248 us against 275)
#ifndef DMET_F2_SPLIT_REM16
#define DMET_F2_SPLIT_REM16 5
#endif
#ifndef DMET_F2_SPLIT_REM_ALLTAIL
#define DMET_F2_SPLIT_REM_ALLTAIL 1
#endif
            if (nb >= kF2MinNodes && (nb < kF2SplitMinNodes ||
                                      ((first_tail == 0 || !DMET_F2_SPLIT_REM_ALLTAIL) && rem * 16 > simds * DMET_F2_SPLIT_REM16))) {
                plan->n_full = plan->total_tiles;
                plan->split = 1;
            }
        }
    }
}

__global__ __launch_bounds__(256) void knn_plan_kernel(const int64_t *__restrict__ ptr, int B, KnnPlanOut o0, KnnPlanOut o1)
{
    knn_plan_body(ptr, B, blockIdx.x == 0 ? o0 : o1);
}

__global__ __launch_bounds__(256) void knn_plan_xy_kernel(const int64_t *__restrict__ qptr, const int64_t *__restrict__ cptr,
                                                          int B, KnnPlanOut o)
{
    knn_plan_body<true>(qptr, B, o, cptr);
}

// Position (in the longest-first order) that owns tile t: the p with tile_ptr[p] <= t < tile_ptr[p+1].
__device__ __forceinline__ int find_tile_event(const int32_t *__restrict__ tile_ptr, int B, int t)
{
    int lo = 0, hi = B;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (tile_ptr[mid] <= t) lo = mid; else hi = mid;
    }
    return lo;
}

// Global -> registers copy of one candidate tile (cntc rows of DP floats; missing rows become +inf).
template <int DP, bool EXACT_D, int NLD>
__device__ __forceinline__ void load_tile(float4 (&pf)[NLD], const float *__restrict__ x, int D, int c0, int cntc,
                                          int lane)
{
    const float inf = __builtin_inff();
    if (EXACT_D) {
        const float4 *g = reinterpret_cast<const float4 *>(x + (int64_t)c0 * DP);
        const int n4 = cntc * (DP / 4);
#pragma unroll
        for (int m = 0; m < NLD; ++m) {
            const int idx = lane + m * kWave;
            pf[m] = (idx < n4) ? g[idx] : make_float4(inf, inf, inf, inf);
        }
    } else {
#pragma unroll
        for (int m = 0; m < NLD; ++m) {
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int flat = (lane + m * kWave) * 4 + e;
                const int c = flat / DP, dd = flat - c * DP;
                v[e] = (c < cntc) ? ((dd < D) ? x[(int64_t)(c0 + c) * D + dd] : 0.0f) : inf;
            }
            pf[m] = make_float4(v[0], v[1], v[2], v[3]);
        }
    }
}

__device__ __forceinline__ float chain_dist32(const float *__restrict__ xj, const float (&q)[32])
{
    const float4 *g = reinterpret_cast<const float4 *>(xj);
    float acc = 0.0f;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const float4 v = g[c];
        float df;
        df = v.x - q[4 * c + 0]; acc = __builtin_fmaf(df, df, acc);
        df = v.y - q[4 * c + 1]; acc = __builtin_fmaf(df, df, acc);
        df = v.z - q[4 * c + 2]; acc = __builtin_fmaf(df, df, acc);
        df = v.w - q[4 * c + 3]; acc = __builtin_fmaf(df, df, acc);
    }
    return acc;
}

// Uncertified queries of sparsely flagged tiles (1..kRequeryMax per 128-query tile; denser tiles go to the exact
// tile kernel): ONE WORKGROUP PER FLAGGED QUERY, taken from the list the flagging sites append to (round 2: the
// tile's workgroup used to take its queries one after the other, and a single straggler cost the build ~90 us).  The
// 256 lanes stride over the event's candidates with the exact R1 chain (four rows in flight per lane; distances cached
// in LDS when the event fits), then k rounds of "smallest (d, j) above the previous pick" (R2) on 64-bit
// (distance bits, j) words with a wavefront + cross-wavefront reduction.
constexpr int kRequeryMax = 8;
constexpr int kRequeryGroups = 512;    // workgroups of the launch: they exit at once while nothing is flagged

__device__ __forceinline__ unsigned long long requery_word(float d, int j)
{
    // a candidate at d >= 1e10 (or NaN) is never a neighbour (upstream's initial best distance, dmet_oracle.c:62)
    return d < kKnnSentinel ? (((unsigned long long)__float_as_uint(d) << 32) | (unsigned)j) : ~0ull;
}

// Runs as the first kRequeryGroups workgroups of the exact kernel's launch (its own launch cost 4.7 us per build while
// nothing is flagged); `cache` / `red` alias that kernel's LDS.
__device__ __forceinline__ void knn_requery_body(const KnnArgs &a, float *__restrict__ cache, const int cache_floats,
                                                 unsigned long long *__restrict__ red, const int group, const int ngroups)
{
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    const int64_t nf64 = *a.any;
    const int nflag = (int)(nf64 < a.N ? nf64 : a.N);
    const int k = a.k;
    for (int it = group; it < nflag; it += ngroups) {   // block-uniform
        const int q = a.qlist[it];
        int lo = 0, hi = a.B;                // event of q: the last b with ptr[b] <= q (empty events share a ptr value
        while (hi - lo > 1) {                // with their successor and are skipped by taking the last)
            const int mid = (lo + hi) >> 1;
            if (a.ptr[mid] <= q) lo = mid; else hi = mid;
        }
        const int ev = lo;
        const int ev_lo = (int)a.ptr[ev], ev_hi = (int)a.ptr[ev + 1];
        const int n = ev_hi - ev_lo;
        const int xt = a.tile_ptr[a.pos_of[ev]] + (q - ev_lo) / a.requery_tile_queries;
        if (a.flags[xt] > kRequeryMax) continue;   // a densely flagged tile: the exact tile kernel recomputes it
        const bool cached = n <= cache_floats;
        float qrow[32];
        {
            const float4 *g = reinterpret_cast<const float4 *>(a.x + (int64_t)q * 32);
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const float4 v = g[c];
                qrow[4 * c] = v.x; qrow[4 * c + 1] = v.y; qrow[4 * c + 2] = v.z; qrow[4 * c + 3] = v.w;
            }
        }
        __syncthreads();   // the previous query's cache / reduction slots are free
        if (cached) {
            // four candidate rows in flight per lane (clamped re-reads past the end, results unused)
            for (int j0 = tid; j0 < n; j0 += 4 * 256) {
                float4 r[4][8];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const float4 *g = reinterpret_cast<const float4 *>(a.x + (int64_t)(ev_lo + min(j0 + 256 * u, n - 1)) * 32);
#pragma unroll
                    for (int c = 0; c < 8; ++c) r[u][c] = g[c];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    float dc = 0.0f;
#pragma unroll
                    for (int c = 0; c < 8; ++c) {
                        float df;
                        df = r[u][c].x - qrow[4 * c + 0]; dc = __builtin_fmaf(df, df, dc);
                        df = r[u][c].y - qrow[4 * c + 1]; dc = __builtin_fmaf(df, df, dc);
                        df = r[u][c].z - qrow[4 * c + 2]; dc = __builtin_fmaf(df, df, dc);
                        df = r[u][c].w - qrow[4 * c + 3]; dc = __builtin_fmaf(df, df, dc);
                    }
                    if (j0 + 256 * u < n) cache[j0 + 256 * u] = dc;
                }
            }
            __syncthreads();
        }
        unsigned long long last = 0ull;
        bool first = true;
        for (int r = 0; r < k; ++r) {
            unsigned long long best = ~0ull;
            for (int j = tid; j < n; j += 256) {
                const float d = cached ? cache[j] : chain_dist32(a.x + (int64_t)(ev_lo + j) * 32, qrow);
                const unsigned long long w = requery_word(d, ev_lo + j);
                if ((first || w > last) && w < best) best = w;
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const unsigned long long o = __shfl_xor(best, off, 64);
                if (o < best) best = o;
            }
            if (lane == 0) red[wv] = best;
            __syncthreads();
            best = red[0];
#pragma unroll
            for (int w = 1; w < 4; ++w) if (red[w] < best) best = red[w];
            __syncthreads();
            const bool found = best != ~0ull;   // block-uniform
            if (tid == 0) {
                const int bj = found ? (int)(unsigned)best : -1;
                a.nbr[(int64_t)q * k + r] = bj;
                if (a.nbr16) a.nbr16[(int64_t)q * k + r] = local_id16(bj, ev_lo);
                a.dist[(int64_t)q * k + r] = found ? __uint_as_float((unsigned)(best >> 32)) : kKnnSentinel;
            }
            if (!found) {
                if (tid == 0)
                    for (int rr = r + 1; rr < k; ++rr) {
                        a.nbr[(int64_t)q * k + rr] = -1;
                        a.dist[(int64_t)q * k + rr] = kKnnSentinel;
                        if (a.nbr16) a.nbr16[(int64_t)q * k + rr] = 0xFFFFu;
                    }
                break;
            }
            last = best;
            first = false;
        }
    }
}

// Per = RadPeriod (dmet_knn_periodic_f32): coordinate c is wrapped with L[c] when L[c] < inf; the host sets L = +inf on
// plain coordinates and on the padding coordinates c >= D, so those take the plain step.  An empty pack is the plain
// kernel.  Padded coordinates (0 - 0) and rows past a partial tile (+inf) behave as in the plain kernel: a periodic
// coordinate turns inf - q into |.| = inf, L - inf = -inf, squared +inf, so such a candidate is never admitted.
// XY (a KnnQuerySet after the periods, dmet_knn_xy_f32): the queries are the rows of qx cut into tiles by qptr, the
// candidates of a tile are the rows [ptr[ev], ptr[ev+1]) of a.x, and a.nbr / a.dist / a.wsd / a.wsj are indexed by query;
// everything else -- staging, sweep, lists, split tail -- is the same code.
template <int DP, int KP, int TQ, bool EXACT_D, typename... Per>
__global__ __launch_bounds__(kWave * kWavesPerGroup, 3) void knn_kernel(const KnnArgs a, Per... per_arg)
{
    constexpr bool PER = pack_has<RadPeriod, Per...>, XY = pack_has<KnnQuerySet, Per...>;
    static_assert(!PER || TQ == 2, "the periodic sweep is the packed two-query form (D <= 8)");
    const RadPeriod per = rad_periods(per_arg...);
    // A workgroup is kWavesPerGroup INDEPENDENT wavefronts (one work item each, no workgroup barrier): the hardware
    // spreads a workgroup's waves over the CU's 4 SIMDs, so each SIMD receives one item of every resident workgroup
    // and whole-sweep and sub-sweep items mix evenly per SIMD (single-wave workgroups left some SIMDs with 3 whole
    // sweeps: measured 3.1 ms stragglers against a 2.4 ms median).
    __shared__ KnnShared<DP, TQ> sh_all[kWavesPerGroup];
    // (wave-uniform, and said so: without readfirstlane the tile, the event and every derived address are per-lane math)
    const int wv_ = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    KnnShared<DP, TQ> &sh = sh_all[wv_];
    int first_group = 0;
    if constexpr (DP == 32 && !XY) {
        if (a.qlist) {    // (kernel-uniform) matrix-core path: the leading workgroups are the per-query fallback
            if (a.any && *a.any == 0) return;
            if ((int)blockIdx.x < a.requery_groups) {
                constexpr int kFloats = (int)((sizeof(sh_all) - 64) / sizeof(float));
                knn_requery_body(a, reinterpret_cast<float *>(sh_all), kFloats,
                                 reinterpret_cast<unsigned long long *>(reinterpret_cast<char *>(sh_all) + sizeof(sh_all) - 64),
                                 (int)blockIdx.x, a.requery_groups);
                return;
            }
            first_group = a.requery_groups;
        }
    }
    const int item = ((int)blockIdx.x - first_group) * kWavesPerGroup + wv_;
    const int lane = threadIdx.x & 63;
#ifdef DMET_KNN_STAMP
    if (lane == 0 && item < (1 << 16)) {
        g_knn_stamps[item][0] = __builtin_amdgcn_s_memrealtime();
        unsigned hwid, xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        g_knn_stamps[item][2] = hwid;
        g_knn_stamps[item][3] = xcc;
        g_knn_stamps[item][1] = 0;
    }
#endif
    const float *__restrict__ x = a.x;
    const int64_t *__restrict__ ptr = a.ptr;
    const KnnQuerySet qs = query_set(a.x, a.ptr, per_arg...);
    const float *__restrict__ qx = qs.qx;            // query rows and their events (x / ptr unless XY)
    const int64_t *__restrict__ qptr = qs.qptr;
    const int D = a.D;
    constexpr int QT = kWave * TQ;  // queries per tile

    // which (query tile, candidate sub-sweep) is this wavefront?  (plan lives in device memory)
    const int n_full = a.plan->n_full, split = a.plan->split, total = a.plan->total_tiles;
    int tile = item, sub = 0, nsub = 1;
    // as the fallback of the matrix-core path (flags given) every tile is swept whole: the few flagged tiles need no
    // balancing, and without partial lists the merge launch is not needed either
    if (item >= n_full && !a.flags) {
        const int r = item - n_full;
        tile = n_full + r / split;
        sub = r % split;
        nsub = split;
    }
    if (tile >= total) return;
    if (a.any && *a.any == 0) return;   // matrix-core path certified every query: nothing to recompute
    if (a.flags && a.flags[tile] < a.flag_min) return;
    const int pos = find_tile_event(a.tile_ptr, a.B, tile);
    const int ev = a.order[pos];
    const int ev_lo = (int)qptr[ev], ev_hi = (int)qptr[ev + 1];
    const int q_first = ev_lo + (tile - a.tile_ptr[pos]) * QT;

    // candidate range = the tile's own event (or one chunk of it for a split tile)
    int clo = XY ? (int)ptr[ev] : ev_lo, chi = XY ? (int)ptr[ev + 1] : ev_hi;
    if (nsub > 1) {
        const int chunk = (((chi - clo) + nsub - 1) / nsub + 1) & ~1;  // even: candidate pairs never straddle chunks
        clo = min(chi, clo + sub * chunk);
        chi = min(chi, clo + chunk);
    }

    int qi[TQ];
    bool valid[TQ];
    float tau[TQ];
    int cnt[TQ];
    float *ld[TQ];
    int32_t *lj[TQ];
    f2 q2[(TQ == 2) ? DP : 1];
    float q1[(TQ == 1) ? DP : 1];
#pragma unroll
    for (int t = 0; t < TQ; ++t) {
        qi[t] = q_first + t * kWave + lane;
        valid[t] = qi[t] < ev_hi;
        const int64_t qq = valid[t] ? qi[t] : ev_lo;
#pragma unroll
        for (int c = 0; c < DP; ++c) {
            float v;
            if (EXACT_D) v = qx[qq * DP + c]; else v = (c < D) ? qx[qq * D + c] : 0.0f;
            if (TQ == 2) { if (t == 0) q2[c].x = v; else q2[c].y = v; }
            else q1[c] = v;
        }
        tau[t] = valid[t] ? kKnnSentinel : -1.0f;  // a distance is never < -1: idle lanes admit nothing
        cnt[t] = 0;
        if (nsub == 1) {
            ld[t] = a.wsd + qq * KP;
            lj[t] = a.wsj + qq * KP;
        } else {
            const int64_t slot = (int64_t)(tile - n_full) * QT + t * kWave + lane;
            ld[t] = a.psd + (slot * nsub + sub) * KP;
            lj[t] = a.psj + (slot * nsub + sub) * KP;
        }
    }
    unsigned fresh = (1u << TQ) - 1u;  // wave-uniform: list of slot t not yet written to ws

    constexpr int kLd4 = kTileC * DP / 4;  // float4s per tile
    constexpr int kLdPerLane = (kLd4 + kWave - 1) / kWave;
    const float inf = __builtin_inff();
    const float4 inf4 = make_float4(inf, inf, inf, inf);
    // row kTileC is a permanent +inf row: the paired sweep may read one row past a full tile, and rows past a
    // partial tile are filled with +inf too, so such candidates get d = +inf and are never admitted
    for (int i = lane; i < DP / 4; i += kWave) sh.tile[kLd4 + i] = inf4;

    float4 pf[kLdPerLane];  // next tile, prefetched into registers while the current one is swept
#pragma unroll
    for (int m = 0; m < kLdPerLane; ++m) pf[m] = inf4;
    if (clo < chi) load_tile<DP, EXACT_D, kLdPerLane>(pf, x, D, clo, min(kTileC, chi - clo), lane);

    for (int c0 = clo; c0 < chi; c0 += kTileC) {
        const int cntc = min(kTileC, chi - c0);
        wave_sync();  // every lane is done reading the previous tile
#pragma unroll
        for (int m = 0; m < kLdPerLane; ++m) {
            const int idx = lane + m * kWave;
            if (idx < kLd4) sh.tile[idx] = pf[m];
        }
        wave_sync();
        if (c0 + kTileC < chi)
            load_tile<DP, EXACT_D, kLdPerLane>(pf, x, D, c0 + kTileC, min(kTileC, chi - c0 - kTileC), lane);

        for (int cc = 0; cc < cntc; cc += 2) {
            float dA[TQ], dB[TQ];
            if (TQ == 2) {
                f2 accA = {0.0f, 0.0f}, accB = {0.0f, 0.0f};
#pragma unroll
                for (int c4 = 0; c4 < DP / 4; ++c4) {
                    const float4 v = sh.tile[cc * (DP / 4) + c4];        // wave-uniform address: LDS broadcast
                    const float4 w = sh.tile[(cc + 1) * (DP / 4) + c4];
                    const f2 vxy = {v.x, v.y}, vzw = {v.z, v.w}, wxy = {w.x, w.y}, wzw = {w.z, w.w};
                    if constexpr (PER) {
                        const float *L = per.L + 4 * c4;
                        pk_dist_step1_per<false>(accA, accB, vxy, wxy, q2[4 * c4 + 0], L[0], L[0] < inf);
                        pk_dist_step1_per<true>(accA, accB, vxy, wxy, q2[4 * c4 + 1], L[1], L[1] < inf);
                        pk_dist_step1_per<false>(accA, accB, vzw, wzw, q2[4 * c4 + 2], L[2], L[2] < inf);
                        pk_dist_step1_per<true>(accA, accB, vzw, wzw, q2[4 * c4 + 3], L[3], L[3] < inf);
                    } else {
                        pk_dist_step4(accA, accB, vxy, vzw, wxy, wzw, q2[4 * c4 + 0], q2[4 * c4 + 1], q2[4 * c4 + 2],
                                      q2[4 * c4 + 3]);
                    }
                }
                dA[0] = accA.x; dB[0] = accB.x;
                dA[TQ - 1] = accA.y; dB[TQ - 1] = accB.y;
            } else {
                float accA = 0.0f, accB = 0.0f;
#pragma unroll
                for (int c4 = 0; c4 < DP / 4; ++c4) {
                    const float4 v = sh.tile[cc * (DP / 4) + c4];
                    const float4 w = sh.tile[(cc + 1) * (DP / 4) + c4];
                    float df;
                    df = v.x - q1[4 * c4 + 0]; accA = __builtin_fmaf(df, df, accA);
                    df = w.x - q1[4 * c4 + 0]; accB = __builtin_fmaf(df, df, accB);
                    df = v.y - q1[4 * c4 + 1]; accA = __builtin_fmaf(df, df, accA);
                    df = w.y - q1[4 * c4 + 1]; accB = __builtin_fmaf(df, df, accB);
                    df = v.z - q1[4 * c4 + 2]; accA = __builtin_fmaf(df, df, accA);
                    df = w.z - q1[4 * c4 + 2]; accB = __builtin_fmaf(df, df, accB);
                    df = v.w - q1[4 * c4 + 3]; accA = __builtin_fmaf(df, df, accA);
                    df = w.w - q1[4 * c4 + 3]; accB = __builtin_fmaf(df, df, accB);
                }
                dA[0] = accA; dB[0] = accB;
            }
#pragma unroll
            for (int t = 0; t < TQ; ++t) {
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const float dj = u ? dB[t] : dA[t];
                    bool pass = dj < tau[t];
#ifdef DMET_KNN_NOSELECT
                    pass = pass && (dj < -1.0f);   // experiment: distance sweep only
#endif
                    if (pass) {
                        sh.queue[t][cnt[t]][lane] = make_uint2(__float_as_uint(dj), (unsigned)(c0 + cc + u));
                        cnt[t]++;
                    }
                }
                if (__any(cnt[t] > kQMax - 2)) {
                    tau[t] = drain_queue<KP>(sh.queue[t], lane, cnt[t], (fresh >> t) & 1u, valid[t], ld[t], lj[t]);
                    if (!valid[t]) tau[t] = -1.0f;
                    cnt[t] = 0;
                    fresh &= ~(1u << t);
                }
            }
        }
    }
#ifdef DMET_KNN_STAMP
    if (lane == 0 && item < (1 << 16)) g_knn_stamps[item][1] = __builtin_amdgcn_s_memrealtime();
#endif
    // final drain; whole-sweep tiles also emit the first k entries
#pragma unroll
    for (int t = 0; t < TQ; ++t) {
        (void)drain_queue<KP>(sh.queue[t], lane, cnt[t], (fresh >> t) & 1u, valid[t], ld[t], lj[t]);
        if (valid[t] && nsub == 1) {
            const int64_t qq = qi[t];
            if (a.k == KP) {
#pragma unroll
                for (int p = 0; p < KP; p += 4) {
                    *reinterpret_cast<float4 *>(a.dist + qq * KP + p) = *reinterpret_cast<const float4 *>(ld[t] + p);
                    *reinterpret_cast<int4 *>(a.nbr + qq * KP + p) = *reinterpret_cast<const int4 *>(lj[t] + p);
                }
            } else {
                for (int p = 0; p < a.k; ++p) {
                    a.dist[qq * a.k + p] = ld[t][p];
                    a.nbr[qq * a.k + p] = lj[t][p];
                }
            }
            if (a.nbr16)
                for (int p = 0; p < a.k; ++p) a.nbr16[qq * a.k + p] = local_id16(lj[t][p], ev_lo);
        }
    }
}

// Merge the `split` sorted partial lists of every query of the split tiles: k steps of a `split`-way merge by
// (d, j); sentinels (1e10, -1) sort last.  One lane per query slot of the tail tiles (worst-case grid).
template <int KP, typename... Qs>
__global__ __launch_bounds__(256) void knn_merge_kernel(const KnnArgs a, int tile_queries, Qs... qs_arg)
{
    if (a.any && *a.any == 0) return;
    const int n_full = a.plan->n_full, split = a.plan->split, total = a.plan->total_tiles;
    if (split <= 1) return;
    const int64_t slot = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int tile = n_full + (int)(slot / tile_queries);
    if (tile >= total) return;
    if (a.flags && a.flags[tile] < a.flag_min) return;
    const int pos = find_tile_event(a.tile_ptr, a.B, tile);
    const int ev = a.order[pos];
    const int64_t *__restrict__ qptr = query_set(a.x, a.ptr, qs_arg...).qptr;     // the queries' events
    const int64_t qi = qptr[ev] + (int64_t)(tile - a.tile_ptr[pos]) * tile_queries + (slot % tile_queries);
    if (qi >= qptr[ev + 1]) return;
    const float *pd = a.psd + slot * split * KP;
    const int32_t *pj = a.psj + slot * split * KP;
    int head[kMaxSplit];
#pragma unroll
    for (int s = 0; s < kMaxSplit; ++s) head[s] = 0;
    for (int p = 0; p < a.k; ++p) {
        float bd = kKnnSentinel;
        int32_t bj = -1;
        int bs = -1;
#pragma unroll
        for (int s = 0; s < kMaxSplit; ++s) {
            if (s < split && head[s] < KP) {
                const float d = pd[s * KP + head[s]];
                const int32_t j = pj[s * KP + head[s]];
                if (j >= 0 && (bs < 0 || d < bd || (d == bd && j < bj))) { bd = d; bj = j; bs = s; }
            }
        }
#pragma unroll
        for (int s = 0; s < kMaxSplit; ++s) head[s] += (s == bs) ? 1 : 0;
        a.dist[qi * a.k + p] = bd;
        a.nbr[qi * a.k + p] = bj;
        if (a.nbr16) a.nbr16[qi * a.k + p] = local_id16(bj, (int)a.ptr[ev]);
    }
}

#include "knn_filter.h"

int num_simds()
{
    static int cached = 0;
    if (cached == 0) {
        int dev = 0, cus = 0;
        if (hipGetDevice(&dev) == hipSuccess &&
            hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cus > 0)
            cached = cus * 4;
        else
            cached = 1024;
    }
    return cached;
}

inline int padded_k(int k) { return k <= 8 ? 8 : k <= 16 ? 16 : k <= 32 ? 32 : 64; }
constexpr int kMaxSimds = 4096;  // workspace bound for the split (tail) tiles: fewer than `simds` tiles
// What the caller knows about the event sizes of a build (dmet_knn_size_hint; 0 = unknown).
struct KnnSizeHint {
    int min_nodes = 0, max_nodes = 0;
};

// One kNN build, as its entry asks for it.  Everything below the entries works from this request alone.
struct KnnBuild {
    const float *x;             // candidate rows, cut into B events by ptr; the queries too unless qs is set
    const int64_t *ptr;
    int64_t N;                  // number of QUERY rows: the rows of x, or of qs.qx when that is set
    KnnQuerySet qs;             // qx != nullptr: two point sets (exact sweep only)
    const RadPeriod *per;       // non-null: periodic coordinates (D <= 8)
    int B, D, k;
    int32_t *nbr;
    float *dist;
    uint16_t *nbr16;            // optional event-local copy of nbr
    void *ws;
    size_t ws_bytes;
    hipStream_t st;
    KnnRider rider;             // P != nullptr: the dense layer to carry if the build takes the second filter form
    BnAffine affine;            // raw != nullptr: the BatchNorm transform the prep launch has to apply (x is its output)
    KnnSizeHint hint;
};

// status of a build, and which of the request's options it carried out (a failed build carried out none: a bare status
// converts to an outcome with both flags false)
struct KnnOutcome {
    int rc = 0;
    bool rider_done = false, affine_done = false;
    KnnOutcome(int rc_ = 0) : rc(rc_) {}
};

struct KnnWorkspace {
    KnnPlan *plan;
    int32_t *order;
    int32_t *pos_of;
    int32_t *tile_ptr;
    float *wsd;
    int32_t *wsj;
    float *psd;
    int32_t *psj;
    // matrix-core filter path
    KnnPlan *fplan;
    int32_t *forder;
    int32_t *fpos_of;
    int32_t *ftile_ptr;
    float *nrm;
    uint8_t *rec;         // candidate tile records
    int64_t nrec;
    int32_t *flags;       // flags[...], any[4] and qflag[N] are one zero-filled region (any[1], any[2]: second attempts)
    int32_t *any;
    uint8_t *qflag;
    int32_t *qlist;       // [N] flagged queries (not cleared: `any` bounds it)
    size_t zero_bytes;
    size_t bytes;
};

inline int64_t exact_tiles_max(int64_t N, int B) { return (N + 63) / 64 + B + 1; }   // bound for 64- and 128-query tiles

// N query rows.  exact_only (the two-set build): the exact kernel's part alone -- plan, order, tile prefix, the running
// lists of the queries, the partial lists of the split tail; the filter's members stay null.
inline KnnWorkspace carve_workspace(void *ws, int64_t N, int B, int KP, bool exact_only = false)
{
    KnnWorkspace w{};
    uintptr_t p = (reinterpret_cast<uintptr_t>(ws) + 255u) & ~(uintptr_t)255u;
    auto take = [&](size_t nbytes) { uintptr_t r = p; p = (p + nbytes + 255u) & ~(uintptr_t)255u; return r; };
    // query slots of split (tail) tiles: fewer than kMaxSimds tiles, and never more than all tiles hold
    size_t split_q = (size_t)kMaxSimds * 128;
    if ((size_t)N + 128 * ((size_t)B + 1) < split_q) split_q = (size_t)N + 128 * ((size_t)B + 1);
    // the filter's split tiles use the same arrays: [slots][kFilterMaxSplit][KP + KP/4 + pad]
    size_t ps_elems = split_q * kMaxSplit * KP;
    if (!exact_only) {
        size_t fslots = (size_t)kMaxSimds * 2 * kFQ;
        if ((size_t)N + kFQ * ((size_t)B + 1) < fslots) fslots = (size_t)N + kFQ * ((size_t)B + 1);
        const size_t need = fslots * kFilterMaxSplit * (size_t)(2 * KP);
        if (need > ps_elems) ps_elems = need;
    }
    w.plan = reinterpret_cast<KnnPlan *>(take(sizeof(KnnPlan)));
    w.order = reinterpret_cast<int32_t *>(take(sizeof(int32_t) * ((size_t)B + 1)));
    w.pos_of = reinterpret_cast<int32_t *>(take(sizeof(int32_t) * ((size_t)B + 1)));
    w.tile_ptr = reinterpret_cast<int32_t *>(take(sizeof(int32_t) * ((size_t)B + 1)));
    w.wsd = reinterpret_cast<float *>(take(sizeof(float) * (size_t)N * KP));
    w.wsj = reinterpret_cast<int32_t *>(take(sizeof(int32_t) * (size_t)N * KP));
    w.psd = reinterpret_cast<float *>(take(sizeof(float) * ps_elems));
    w.psj = reinterpret_cast<int32_t *>(take(sizeof(int32_t) * ps_elems));
    if (!exact_only) {
        w.fplan = reinterpret_cast<KnnPlan *>(take(sizeof(KnnPlan)));
        w.forder = reinterpret_cast<int32_t *>(take(sizeof(int32_t) * ((size_t)B + 1)));
        w.fpos_of = reinterpret_cast<int32_t *>(take(sizeof(int32_t) * ((size_t)B + 1)));
        w.ftile_ptr = reinterpret_cast<int32_t *>(take(sizeof(int32_t) * ((size_t)B + 1)));
        w.nrm = reinterpret_cast<float *>(take(sizeof(float) * (size_t)N));
        w.nrec = (N >> 5) + B + 1;                               // event b owns records from (ptr[b] >> 5) + b
        w.rec = reinterpret_cast<uint8_t *>(take((size_t)w.nrec * kRecBytesMax));
        w.zero_bytes = sizeof(int32_t) * ((size_t)exact_tiles_max(N, B) + 4) + (size_t)N;
        w.flags = reinterpret_cast<int32_t *>(take(w.zero_bytes));
        w.any = w.flags + exact_tiles_max(N, B);
        w.qflag = reinterpret_cast<uint8_t *>(w.any + 4);
        w.qlist = reinterpret_cast<int32_t *>(take(sizeof(int32_t) * (size_t)N));
    }
    w.bytes = (size_t)(p - reinterpret_cast<uintptr_t>(ws));
    return w;
}

// DMET_KNN_PATH=exact disables the matrix-core filter (tests and A/B timing); =filter_only (experiment builds only)
// skips the exact fallback of uncertified tiles; anything else: filter when eligible + fallback
inline int filter_mode()
{
    const char *e = getenv("DMET_KNN_PATH");   // read per call: tests switch paths inside one process
    if (e && strcmp(e, "exact") == 0) return 0;
#if defined(DMET_KNN_EXPERIMENT) || defined(DMET_FILTER_ABL) || defined(DMET_F2_ABL) || defined(DMET_F2_SAMEREC)
    // timing builds only (tools/knn_budget*.sh): skipping the exact fallback can return uncertified neighbours, so
    // the product library does not honour it
    if (e && strcmp(e, "filter_only") == 0) return 2;
#endif
    return 1;
}

// DMET_KNN_FILTER=1: first form (per-key queue) for every event (A/B timing, tests); default: second form where it applies
inline int filter_form2()
{
    const char *e = getenv("DMET_KNN_FILTER");
    return (e && strcmp(e, "1") == 0) ? 0 : 1;
}

// DMET_KNN_CUT: the margin scale of the second form's final threshold (f2_cut).  Unset: kF2CutScale; "off" or "0": no cut, the
// threshold stays tk[M-1] (A/B against the cut in one library); any other finite value >= 0 is the scale itself, and a
// scale of zero ("0.0", "0e0") cuts at tk[k-1]: a query whose k nearest sit in k different tiles then fails its
// certificate and takes the second attempt (tests).
// Read per call, as DMET_KNN_PATH is.  Default 1.25: a scale of 1 is the certifying bound itself, the quarter on top is
// for the two-step estimate of the implicit slack; measured second attempts and flagged queries in
// profiles/r05_knn_cut.md.
constexpr float kF2CutScale = 1.25f;
inline float knn_cut_scale()
{
    const char *e = getenv("DMET_KNN_CUT");
    if (!e || !*e) return kF2CutScale;
    if (strcmp(e, "0") == 0 || strcmp(e, "off") == 0) return -1.0f;
    char *end = nullptr;
    const float v = strtof(e, &end);
    return (end != e && *end == '\0' && v >= 0.0f && v <= 1e6f) ? v : kF2CutScale;
}

// DMET_KNN_RUNCUT=0: the second form's main sweep records its hit masks against tk[M-1] alone and the cut is applied after
// the sweep only, as before the running cut (f2_running_tau): same tables and counters, A/B timing in one library.  Read
// per call.
inline int knn_run_cut() { return env_is("DMET_KNN_RUNCUT", "0") ? 0 : 1; }

// prep + filter (+ in-place re-rank) + re-rank of the split tail tiles, for result capacity KF >= k.  affine (32 features
// only): the transform the prep launch applies; rider (32 features, second form only): the dense layer the filter launch
// carries; nullptr: none.
template <int KF, int NH = 1>
int launch_filter(const KnnFilterArgs &f, const KnnWorkspace &w, int simds, const KnnPlanOut &px, const KnnPlanOut &pf,
                  hipStream_t st, const KnnRider *rider, const BnAffine *affine)
{
    const int slots = simds * kF2WavesPerSimd;   // filter wavefronts per SIMD
    if (affine) {
        if constexpr (NH == 1)
            hipLaunchKernelGGL((knn_prep_kernel<1, true>), dim3((unsigned)((w.nrec * kWave + 255) / 256 + 2)), dim3(256), 0, st, f.x,
                               f.ptr, f.B, f.N, w.nrm, w.rec, w.nrec, reinterpret_cast<uint32_t *>(w.flags), w.zero_bytes, px,
                               pf, f.form2, *affine, 0);
    } else {
        hipLaunchKernelGGL((knn_prep_kernel<NH>), dim3((unsigned)((w.nrec * kWave + 255) / 256 + 2)), dim3(256), 0, st, f.x,
                           f.ptr, f.B, f.N, w.nrm, w.rec, w.nrec, reinterpret_cast<uint32_t *>(w.flags), w.zero_bytes, px, pf,
                           f.form2, BnAffine{}, 0);
    }
    DMET_LAUNCH_CHECK("knn_prep_kernel");
    const int64_t ftiles_max = (f.N + kFQ - 1) / kFQ + f.B;
    const int64_t fblocks = (ftiles_max + slots + kWavesPerGroup - 1) / kWavesPerGroup;
    if (f.form2) {
        KnnFilterArgs fr = f;
        int64_t grid = fblocks;
        if (rider) {
            fr.rW = rider->W; fr.rb = rider->b; fr.rP = rider->P; fr.rQ = rider->Q; fr.r_sliced = rider->sliced;
            fr.first_rider = (int)fblocks;
            grid = fblocks + rider_groups();
        }
        hipLaunchKernelGGL((knn_filter12_kernel<KF, NH>), dim3((unsigned)grid), dim3(kWave * kWavesPerGroup), 0, st, fr);
        DMET_LAUNCH_CHECK("knn_filter12_kernel");
    } else {
        if constexpr (NH == 1) hipLaunchKernelGGL((knn_filter_kernel<KF>), dim3((unsigned)fblocks), dim3(kWave * kWavesPerGroup), 0, st, f);
        DMET_LAUNCH_CHECK("knn_filter_kernel");
    }
    constexpr int kRerankQpb = 4 * (kWave / filter_list_len(KF));
    constexpr int kRerankParts = (kFQ + kRerankQpb - 1) / kRerankQpb;
    // only the split tail tiles (fewer than `slots`) need the separate re-rank: whole sweeps re-rank in place
    const int64_t tail_max = ftiles_max < slots ? ftiles_max : slots;
    if constexpr (NH == 1) {    // tail tiles of the first form (32 features only)
        if (f.no_rerank) return 0;     // no first-form event in this batch (size hint): nothing to merge
        hipLaunchKernelGGL((knn_rerank_kernel<KF>), dim3((unsigned)(tail_max * kRerankParts)), dim3(256), 0, st, f);
        DMET_LAUNCH_CHECK("knn_rerank_kernel");
    }
    return 0;
}

// the per x query-set x EXACT_D ladder of knn_kernel (periodic instances exist for DP <= 8 only)
template <int DP, int KP, int TQ>
void launch_sweep(int64_t blocks, unsigned dyn, hipStream_t st, const KnnArgs &a, bool exact_d, const RadPeriod *per,
                  const KnnQuerySet *qs)
{
    const dim3 grid((unsigned)blocks), block(kWave * kWavesPerGroup);
    with_pack<DP <= 8, true>(per, qs, [&](auto... pack) {
        if (exact_d) hipLaunchKernelGGL((knn_kernel<DP, KP, TQ, true, decltype(pack)...>), grid, block, dyn, st, a, pack...);
        else hipLaunchKernelGGL((knn_kernel<DP, KP, TQ, false, decltype(pack)...>), grid, block, dyn, st, a, pack...);
    });
}

// the query-set ladder of knn_merge_kernel (the merge reads no coordinate: no periodic instance)
template <int KP>
void launch_merge(int64_t slots, hipStream_t st, const KnnArgs &a, int tile_queries, const KnnQuerySet *qs)
{
    with_pack<false, true>(nullptr, qs, [&](auto... pack) {
        hipLaunchKernelGGL((knn_merge_kernel<KP, decltype(pack)...>), dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, st, a,
                           tile_queries, pack...);
    });
}

template <int DP, int KP>
KnnOutcome launch_knn(const KnnBuild &r, const KnnWorkspace &w)
{
    KnnOutcome done;
    constexpr int TQ = (DP <= 32) ? 2 : 1;
    constexpr int QT = kWave * TQ;
    const KnnQuerySet *qs = r.qs.qx ? &r.qs : nullptr;
    int simds = num_simds();
    if (simds > kMaxSimds) simds = kMaxSimds;
    bool use_filter = false;   // one point set only; never with periods (their D <= 8)
    if constexpr ((DP == 32 || DP == 64) && KP <= 32)
        use_filter = !qs && r.D == DP && r.k <= 20 && aligned16(r.x) && filter_mode() != 0 && (DP == 32 || filter_form2());
    constexpr int NH = DP == 64 ? 2 : 1;   // 64 features (the DRN's hidden width): second filter form only
    const int slots = simds * kF2WavesPerSimd;   // filter wavefronts per SIMD
    const KnnPlanOut px{QT, simds, kMaxSplit, w.order, w.pos_of, w.tile_ptr, w.plan};
    const KnnPlanOut pf{kFQ, slots, kFilterMaxSplit, w.forder, w.fpos_of, w.ftile_ptr, w.fplan};
    if (qs) {
        hipLaunchKernelGGL(knn_plan_xy_kernel, dim3(1), dim3(256), 0, r.st, qs->qptr, r.ptr, r.B, px);
        DMET_LAUNCH_CHECK("knn_plan_xy_kernel");
    } else if (!use_filter) {   // the filter path computes both plans inside its prep launch
        hipLaunchKernelGGL(knn_plan_kernel, dim3(1), dim3(256), 0, r.st, r.ptr, r.B, px, pf);
        DMET_LAUNCH_CHECK("knn_plan_kernel");
    }
    KnnArgs a{r.x, r.ptr, r.B, r.N, r.D, r.k, r.nbr, r.dist, r.nbr16, w.wsd, w.wsj, w.plan, w.order, w.tile_ptr, w.psd, w.psj,
              nullptr, 0, nullptr, nullptr, nullptr, 0, QT};
    // uncertified-query counters: zero for every one-set call, so dmet_knn_fallback_stats is meaningful on any path (the
    // matrix-core path clears them in its prep kernel)
    if (!qs && !use_filter && hipMemsetAsync(w.flags, 0, w.zero_bytes, r.st) != hipSuccess)
        return hip_fail(hipGetLastError(), "hipMemsetAsync");

    // matrix-core filter + exact re-rank for the hot shapes (D = 32 or 64, k <= 20); the exact kernel then only recomputes
    // the tiles the re-rank could not certify
    if (use_filter) {
        KnnFilterArgs f{r.x, r.ptr, r.B, r.N, r.k, w.nrm, w.rec, w.fplan, w.forder, w.fpos_of, w.ftile_ptr,
                        w.psd, w.psj, r.nbr, r.dist, r.nbr16, w.flags, w.any, w.qflag, w.qlist, w.tile_ptr, QT, filter_form2(),
                        NH == 1 ? 1.0f : 1.5f, nullptr, nullptr, nullptr, nullptr, 0, 0,
                        (aligned16(r.nbr) && aligned16(r.dist) && aligned16(r.nbr16) && !env_is("DMET_KNN_EMIT", "lanes")) ? 1 : 0, 0,
                        knn_cut_scale(), w.any + 1, knn_run_cut()};
        // every event is a second-form event (the caller says so): the first form's tail merge has nothing to do
        f.no_rerank = (f.form2 && r.hint.min_nodes >= kF2MinNodes && r.hint.max_nodes >= r.hint.min_nodes &&
                       r.hint.max_nodes <= kF2MaxNodes) ? 1 : 0;
        // the affine rides in the prep launch and the rider in the second filter form, both at 32 features only
        const BnAffine *affine = (NH == 1 && r.affine.raw) ? &r.affine : nullptr;
        const KnnRider *rider = (NH == 1 && f.form2 && r.rider.P) ? &r.rider : nullptr;
        int rc = 0;
        if constexpr (DP == 32 || DP == 64) {
            if constexpr (KP == 8) rc = launch_filter<8, NH>(f, w, simds, px, pf, r.st, rider, affine);
            else if constexpr (KP == 16) rc = launch_filter<16, NH>(f, w, simds, px, pf, r.st, rider, affine);
            else if constexpr (KP == 32) rc = launch_filter<20, NH>(f, w, simds, px, pf, r.st, rider, affine);   // 16 < k <= 20 (checked above)
        }
        if (rc) return rc;
        done.affine_done = affine != nullptr;
        done.rider_done = rider != nullptr;
        if (filter_mode() == 2) return done;
        a.flags = w.flags;
        a.any = w.any;
        if constexpr (NH == 1) {
            a.qlist = w.qlist;             // the per-query fallback rides in front of the exact kernel's grid
            a.pos_of = w.pos_of;
            a.requery_groups = kRequeryGroups;
            a.flag_min = kRequeryMax + 1;
        } else {
            a.flag_min = 1;    // no per-query fallback at 64 features: the exact kernel takes every flagged tile
        }
    }

    // worst-case grid (the plan is on the device): every event adds at most one partial tile, and splitting the
    // fewer-than-`simds` tail tiles adds fewer than `simds` workgroups; surplus workgroups exit at once
    const int64_t tiles_max = (r.N + QT - 1) / QT + r.B;
    const int64_t blocks = (tiles_max + simds + kWavesPerGroup - 1) / kWavesPerGroup + a.requery_groups;
    unsigned dyn = 0;
#ifdef DMET_KNN_EXPERIMENT
    if (const char *e = getenv("DMET_KNN_EXTRA_LDS")) dyn = (unsigned)atoi(e);
#endif
    const bool exact_d = r.D == DP && aligned16(r.x) && (!qs || aligned16(qs->qx));
    launch_sweep<DP, KP, TQ>(blocks, dyn, r.st, a, exact_d, r.per, qs);
    DMET_LAUNCH_CHECK(qs ? "knn_kernel (two sets)" : "knn_kernel");
    if (!use_filter) {   // split tiles (the tail of a large batch, every tile of a small one) merge their partial lists
        int64_t mslots = (int64_t)simds * QT;
        if (tiles_max * QT < mslots) mslots = tiles_max * QT;
        launch_merge<KP>(mslots, r.st, a, QT, qs);
        DMET_LAUNCH_CHECK(qs ? "knn_merge_kernel (two sets)" : "knn_merge_kernel");
    }
    return done;
}

template <int DP>
KnnOutcome dispatch_k(const KnnBuild &r)
{
    const KnnWorkspace w = carve_workspace(r.ws, r.N, r.B, padded_k(r.k), r.qs.qx != nullptr);
    if (r.k <= 8) return launch_knn<DP, 8>(r, w);
    if (r.k <= 16) return launch_knn<DP, 16>(r, w);
    if (r.k <= 32) return launch_knn<DP, 32>(r, w);
    return launch_knn<DP, 64>(r, w);
}

// The build of a checked, non-empty request: status, and whether the rider and the affine were carried out.
KnnOutcome knn_build(const KnnBuild &r)
{
    if (r.D <= 4) return dispatch_k<4>(r);
    if (r.D <= 8) return dispatch_k<8>(r);
    if (r.D <= 16) return dispatch_k<16>(r);
    if (r.D <= 32) return dispatch_k<32>(r);
    return dispatch_k<64>(r);
}

}  // namespace
}  // namespace dmet

using namespace dmet;

// ---- entries: each checks its arguments, fills a KnnBuild and calls knn_build once ------------------------------------
// dmet_knn_size_hint is a per-thread contract (include/dmet.h); take_size_hint is the only reader of its storage.
static thread_local KnnSizeHint g_size_hint;

extern "C" int dmet_knn_size_hint(int min_nodes, int max_nodes)
{
    DMET_REQUIRE(min_nodes >= 0 && max_nodes >= 0, "dmet_knn_size_hint: negative size");
    g_size_hint.min_nodes = min_nodes;
    g_size_hint.max_nodes = max_nodes;
    return 0;
}

// The hint describes one batch: the build that takes it spends it, whatever its outcome.
static KnnSizeHint take_size_hint()
{
    const KnnSizeHint h = g_size_hint;
    g_size_hint = KnnSizeHint{};
    return h;
}

extern "C" size_t dmet_knn_workspace_bytes(int64_t N, int B, int D, int k)
{
    (void)D;
    if (N <= 0 || B < 0 || k <= 0 || k > DMET_MAX_K) return 0;
    return carve_workspace(nullptr, N, B, padded_k(k)).bytes + 512;
}

// The one-set entries share the arguments of dmet_knn_local_f32 and its checks.
static KnnBuild local_request(const float *x, const int64_t *ptr, int B, int64_t N, int D, int k, int32_t *nbr, float *dist,
                              uint16_t *nbr16, void *ws, size_t ws_bytes, dmet_stream_t stream)
{
    return KnnBuild{x, ptr, N, KnnQuerySet{nullptr, nullptr}, nullptr, B, D, k, nbr, dist, nbr16, ws, ws_bytes,
                    as_stream(stream), KnnRider{}, BnAffine{}, KnnSizeHint{}};
}

// 0: build it; 1: an empty problem, nothing to do; < 0: refused
static int local_checks(const KnnBuild &r)
{
    const char *who = "dmet_knn_f32/dmet_knn_local_f32";
    DMET_REQUIRE(r.N >= 0 && r.N < (int64_t)2147483647 - 4096, "%s: N=%lld out of range", who, (long long)r.N);
    DMET_REQUIRE(r.B >= 0, "%s: B=%d", who, r.B);
    DMET_REQUIRE(r.k >= 1 && r.k <= DMET_MAX_K, "%s: k=%d not in [1,%d]", who, r.k, DMET_MAX_K);
    DMET_REQUIRE(r.D >= 1 && r.D <= DMET_MAX_KNN_DIM, "%s: D=%d not in [1,%d]", who, r.D, DMET_MAX_KNN_DIM);
    if (r.N == 0 || r.B == 0) return 1;
    DMET_REQUIRE(r.x && r.ptr && r.nbr && r.dist && r.ws, "%s: null pointer", who);
    DMET_REQUIRE(r.ws_bytes >= dmet_knn_workspace_bytes(r.N, r.B, r.D, r.k), "%s: workspace too small", who);
    DMET_REQUIRE(!r.nbr16 || (reinterpret_cast<uintptr_t>(r.nbr16) & 3u) == 0, "dmet_knn_local_f32: nbr_local must be 4-byte aligned");
    return 0;
}

static KnnOutcome local_build(const KnnBuild &r)
{
    const int rc = local_checks(r);
    if (rc) return rc < 0 ? rc : 0;
    return knn_build(r);
}

extern "C" int dmet_knn_local_f32(const float *x, const int64_t *ptr, int B, int64_t N, int D, int k, int32_t *nbr,
                                  float *dist, uint16_t *nbr16, void *ws, size_t ws_bytes, dmet_stream_t stream)
{
    KnnBuild r = local_request(x, ptr, B, N, D, k, nbr, dist, nbr16, ws, ws_bytes, stream);
    r.hint = take_size_hint();
    return local_build(r).rc;
}

extern "C" int dmet_knn_f32(const float *x, const int64_t *ptr, int B, int64_t N, int D, int k, int32_t *nbr,
                            float *dist, void *ws, size_t ws_bytes, dmet_stream_t stream)
{
    KnnBuild r = local_request(x, ptr, B, N, D, k, nbr, dist, nullptr, ws, ws_bytes, stream);
    r.hint = take_size_hint();
    return local_build(r).rc;
}

// Periodic kNN (train.py:47: phi wraps at +-pi): the K1 contract with the radius graph's periodic difference.  D <= 8
// only, so the build is always the exact packed sweep; all-zero periods take the plain kernels.
extern "C" int dmet_knn_periodic_f32(const float *x, const int64_t *ptr, int B, int64_t N, int D, int k,
                                     const float *period, int32_t *nbr, float *dist, uint16_t *nbr16, void *ws,
                                     size_t ws_bytes, dmet_stream_t stream)
{
    KnnBuild r = local_request(x, ptr, B, N, D, k, nbr, dist, nbr16, ws, ws_bytes, stream);
    r.hint = take_size_hint();   // spent as by dmet_knn_local_f32, also when a period is refused
    RadPeriod per;
    bool any = false;
    const int rc = radius_periods("dmet_knn_periodic_f32", D, period, &per, &any);
    if (rc) return rc;
    if (any) r.per = &per;
    return local_build(r).rc;
}

// The checks of a dense layer that is to ride along, and the rider itself.  It rides in the matrix-core filter launch
// (32 features): any other build leaves the layer to the caller, so it is handed down for 32 aligned features only.
static int rider_checks(const float *W, int layout, const float *P, const void *Q)
{
    DMET_REQUIRE(W && P && Q, "dmet_knn_local_dense_f32: null pointer");
    DMET_REQUIRE(layout >= 0 && layout <= 2, "dmet_knn_local_dense_f32: layout=%d not in {0, 1, 2}", layout);
    DMET_REQUIRE(aligned16(P) && aligned16(Q), "dmet_knn_local_dense_f32: P / Q must be 16-byte aligned");
    return 0;
}

static KnnRider make_rider(const KnnBuild &r, const float *W, const float *bias, int layout, float *P, void *Q)
{
    if (!(r.D == 32 && r.N > 0 && r.B > 0 && aligned16(r.x))) return KnnRider{};
    return KnnRider{W, bias, P, reinterpret_cast<float *>(Q), layout};
}

extern "C" int dmet_knn_local_dense_f32(const float *x, const int64_t *ptr, int B, int64_t N, int D, int k, int32_t *nbr,
                                        float *dist, uint16_t *nbr16, const float *W, const float *bias, int layout,
                                        float *P, void *Q, int *dense_done, void *ws, size_t ws_bytes,
                                        dmet_stream_t stream)
{
    DMET_REQUIRE(dense_done, "dmet_knn_local_dense_f32: dense_done is null");
    *dense_done = 0;
    if (const int rc = rider_checks(W, layout, P, Q)) return rc;
    KnnBuild r = local_request(x, ptr, B, N, D, k, nbr, dist, nbr16, ws, ws_bytes, stream);
    r.hint = take_size_hint();
    r.rider = make_rider(r, W, bias, layout, P, Q);
    const KnnOutcome o = local_build(r);
    *dense_done = (o.rc == 0 && o.rider_done) ? 1 : 0;
    return o.rc;
}

extern "C" int dmet_bn_knn_local_dense_f32(const float *raw, const float *residual, const float *gamma, const float *beta,
                                           const float *mean, const float *invstd, float *y, const int64_t *ptr, int B,
                                           int64_t N, int D, int k, int32_t *nbr, float *dist, uint16_t *nbr16,
                                           const float *W, const float *bias, int layout, float *P, void *Q,
                                           int *dense_done, int *fused, void *ws, size_t ws_bytes, dmet_stream_t stream)
{
    DMET_REQUIRE(fused && dense_done, "dmet_bn_knn_local_dense_f32: fused / dense_done is null");
    *fused = 0;
    *dense_done = 0;
    DMET_REQUIRE(raw && gamma && beta && mean && invstd && y, "dmet_bn_knn_local_dense_f32: null pointer");
    // only the matrix-core path has the prep launch the transform rides in: any other build leaves everything to the
    // caller, the size hint included (the unfused build that the caller then runs needs it)
    const BnAffine affine{raw, residual, gamma, beta, mean, invstd};
    if (!(D == 32 && k >= 1 && k <= 20 && N > 0 && B > 0 && filter_mode() != 0 && bn_affine_aligned16(affine, y))) return 0;
    if (W) {
        if (const int rc = rider_checks(W, layout, P, Q)) return rc;
    }
    KnnBuild r = local_request(y, ptr, B, N, D, k, nbr, dist, nbr16, ws, ws_bytes, stream);
    r.hint = take_size_hint();
    r.affine = affine;
    if (W) r.rider = make_rider(r, W, bias, layout, P, Q);
    const KnnOutcome o = local_build(r);
    *dense_done = (o.rc == 0 && o.rider_done) ? 1 : 0;
    if (o.rc == 0 && !o.affine_done) {
        set_error("dmet_bn_knn_local_dense_f32: the build did not take the matrix-core path it was checked for");
        return -22;
    }
    *fused = (o.rc == 0) ? 1 : 0;
    return o.rc;
}

extern "C" int dmet_knn_fallback_stats(const void *ws, int64_t N, int B, int D, int k, int64_t *out, dmet_stream_t stream)
{
    (void)D;
    DMET_REQUIRE(N > 0 && B > 0 && k >= 1 && k <= DMET_MAX_K && ws && out, "dmet_knn_fallback_stats: bad arguments");
    const KnnWorkspace w = carve_workspace(const_cast<void *>(ws), N, B, padded_k(k));
    const int64_t n = exact_tiles_max(N, B);
    int32_t *host = static_cast<int32_t *>(malloc(sizeof(int32_t) * (size_t)n));
    DMET_REQUIRE(host != nullptr, "dmet_knn_fallback_stats: out of host memory");
    hipStream_t st = as_stream(stream);
    hipError_t e = hipMemcpyAsync(host, w.flags, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { free(host); return hip_fail(e, "dmet_knn_fallback_stats"); }
    out[0] = 0; out[1] = 0;
    for (int64_t i = 0; i < n; ++i) { out[0] += host[i] != 0; out[1] += host[i]; }
    free(host);
    if (getenv("DMET_KNN_LIST_FLAGGED") && out[1] > 0) {   // developer aid: the first flagged queries, to stderr
        int32_t ids[16];
        const int64_t m = out[1] < 16 ? out[1] : 16;
        if (hipMemcpy(ids, w.qlist, sizeof(int32_t) * (size_t)m, hipMemcpyDeviceToHost) == hipSuccess)
            for (int64_t i = 0; i < m; ++i) {
                uint8_t why = 0;
                (void)hipMemcpy(&why, w.qflag + ids[i], 1, hipMemcpyDeviceToHost);
                fprintf(stderr, "[dmet] flagged query %d (qflag %d)\n", ids[i], (int)why);
            }
    }
    return 0;
}

// Second attempts of the last build's second filter form (diagnostics): out[0] = wavefronts that swept their event a
// second time, out[1] = the queries those sweeps were for.  Zero for every build that did not take the matrix-core path.
extern "C" int dmet_knn_retry_stats(const void *ws, int64_t N, int B, int D, int k, int64_t *out, dmet_stream_t stream)
{
    (void)D;
    DMET_REQUIRE(N > 0 && B > 0 && k >= 1 && k <= DMET_MAX_K && ws && out, "dmet_knn_retry_stats: bad arguments");
    const KnnWorkspace w = carve_workspace(const_cast<void *>(ws), N, B, padded_k(k));
    int32_t host[2] = {0, 0};
    hipStream_t st = as_stream(stream);
    hipError_t e = hipMemcpyAsync(host, w.any + 1, sizeof(host), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return hip_fail(e, "dmet_knn_retry_stats");
    out[0] = host[0];
    out[1] = host[1];
    return 0;
}

// ---- two point sets: queries y against candidates x of the same events (torch_cluster.knn) --------------------------------
extern "C" size_t dmet_knn_xy_workspace_bytes(int64_t Nx, int64_t Ny, int B, int D, int k)
{
    (void)Nx; (void)D;
    if (Ny <= 0 || B < 0 || k <= 0 || k > DMET_MAX_K) return 0;
    return carve_workspace(nullptr, Ny, B, padded_k(k), true).bytes + 512;
}

// (the size hint is for the matrix-core filter, which the two-set build never takes: it is left alone)
extern "C" int dmet_knn_xy_f32(const float *x, const int64_t *ptr_x, int64_t Nx, const float *y, const int64_t *ptr_y,
                               int64_t Ny, int B, int D, int k, const float *period, int32_t *nbr, float *dist, void *ws,
                               size_t ws_bytes, dmet_stream_t stream)
{
    const int64_t kMaxRows = (int64_t)2147483647 - 4096;
    DMET_REQUIRE(Nx >= 0 && Nx < kMaxRows && Ny >= 0 && Ny < kMaxRows, "dmet_knn_xy_f32: Nx=%lld / Ny=%lld out of range",
                 (long long)Nx, (long long)Ny);
    DMET_REQUIRE(B >= 0, "dmet_knn_xy_f32: B=%d", B);
    DMET_REQUIRE(k >= 1 && k <= DMET_MAX_K, "dmet_knn_xy_f32: k=%d not in [1,%d]", k, DMET_MAX_K);
    DMET_REQUIRE(D >= 1 && D <= DMET_MAX_KNN_DIM, "dmet_knn_xy_f32: D=%d not in [1,%d]", D, DMET_MAX_KNN_DIM);
    RadPeriod per;
    bool any = false;
    if (period) {
        const int rc = radius_periods("dmet_knn_xy_f32", D, period, &per, &any);   // (D <= 8)
        if (rc) return rc;
    }
    if (Ny == 0) return 0;
    DMET_REQUIRE(B >= 1, "dmet_knn_xy_f32: %lld queries but no event", (long long)Ny);
    DMET_REQUIRE((x || Nx == 0) && ptr_x && y && ptr_y && nbr && dist && ws, "dmet_knn_xy_f32: null pointer");
    DMET_REQUIRE(ws_bytes >= dmet_knn_xy_workspace_bytes(Nx, Ny, B, D, k), "dmet_knn_xy_f32: workspace too small");
    return knn_build(KnnBuild{x, ptr_x, Ny, KnnQuerySet{y, ptr_y}, any ? &per : nullptr, B, D, k, nbr, dist, nullptr, ws,
                              ws_bytes, as_stream(stream), KnnRider{}, BnAffine{}, KnnSizeHint{}}).rc;
}

// row_softmax.h -- what the softmax aggregations over a graph share: attention.hip (a dot-product score, key and value
// rows) and gat.hip (an additive score, one row for both).  Here: the lane layout, the graph and its row and reverse-list
// spans, the forward's running softmax of a row, the walks of the two backward passes, and the host side's launch, width
// dispatch and shape checks.  A file brings its score (a policy of the forward walk) and the per-entry arithmetic of its
// backward passes (lambdas of the two walks).
//
// Lane layout, all kernels: a group of LPT lanes (16 for C <= 32, 32 beyond; inside one wavefront) owns one (row, head)
// pair -- a (target, head) in the forward and the by-target pass, a (source, head) in the by-source pass; the pairs of
// one node are neighbours in the grid, so a wavefront reads whole H*C rows.  A 256-thread workgroup holds 16 (LPT 16) or
// 8 (LPT 32) pairs.  A row of any length is taken in chunks of LPT entries: lane l reads the id of entry l once, the
// group walks the chunk kInFlight gathers at a time over the channels c = lane, lane + LPT of the contiguous head rows,
// a channel sum is each lane's partial sum in ascending c followed by the xor butterfly of the group, and lane e keeps
// the scalars of entry e (score, then expf(score - m)) which the group takes back by shuffle.  The running (m, l, acc)
// is rescaled once per chunk that holds a valid entry (by 0 while m is still -inf: nothing finite has been added); l and
// acc add their terms in ascending entry order, the implicit self entry last; a score of -inf adds exactly 0.  Sums run in slot / edge / reverse-index order with no LDS, no __syncthreads and no float atomics: the
// bits depend on LPT (the chunk length), never on the launch or the run, and a table and the edge list of the same
// entries in the same order give the same bits.  Every loop is bounded by a row length or a reverse-list length read
// once and clamped.
#pragma once

#include <math.h>

#include <type_traits>

#include "common.h"

namespace dmet {
namespace {

constexpr int kMaxC = 64;         // channels per head
constexpr int kMaxH = 16;         // heads
constexpr int kMaxHC = 256;       // heads * channels
constexpr int kBlock = 256;
constexpr int kInFlight = 4;      // entries whose head rows are gathered before the first is used

template <int LPT>
__device__ __forceinline__ float group_sum(float v)
{
    // xor butterfly inside the group: a fixed order, and every lane of the group ends with the same bits
#pragma unroll
    for (int off = LPT / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, LPT);
    return v;
}

template <int LPT>
__device__ __forceinline__ float group_max(float v)
{
#pragma unroll
    for (int off = LPT / 2; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, LPT));
    return v;
}

// a . b over the group's channels: the one chain the forward and the backward form a dot product with
template <int LPT, int ITER>
__device__ __forceinline__ float group_dot(const float (&a)[ITER], const float (&b)[ITER])
{
    float part = 0.f;
#pragma unroll
    for (int it = 0; it < ITER; ++it) part += a[it] * b[it];
    return group_sum<LPT>(part);
}

// channels lane, lane + LPT, ... of the head row at p (zeros past C, and for a missing row)
template <int LPT, int ITER>
__device__ __forceinline__ void load_row(float (&r)[ITER], const float *__restrict__ p, bool on, int lane, int C)
{
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
        const int c = lane + it * LPT;
        r[it] = (on && c < C) ? p[c] : 0.f;
    }
}

struct RowGraph {
    const int32_t *idx;       // nbr[Nt, k] (table) or src[E] (list)
    const int32_t *rowptr;    // NULL: table
    const int32_t *tgt;       // list, backward only
    const int32_t *rev_ptr, *rev_pos;
    int64_t Nt, Ns, M;        // M = Nt*k or E: the number of positions
    int k;
    int self_loops;           // one node set: a written entry j == i is skipped, one entry i -> i follows the row's own
};

// positions [lo, lo + n) of row i, clamped to [0, M]
__device__ __forceinline__ void row_span(const RowGraph &g, int64_t i, int64_t &lo, int &n)
{
    if (g.rowptr == nullptr) {
        lo = i * g.k;
        n = g.k;
    } else {
        lo = min(max((int64_t)g.rowptr[i], (int64_t)0), g.M);
        const int64_t hi = min(max((int64_t)g.rowptr[i + 1], lo), g.M);
        n = (int)(hi - lo);
    }
}

// the id of logical entry t of row i: the written entries [0, n), then (self_loops) the entry i -> i at t == n; -1 for
// an empty slot, an id outside [0, Ns), a written self loop under self_loops, and anything past the row
__device__ __forceinline__ int32_t row_entry(const RowGraph &g, int64_t i, int64_t lo, int n, int t)
{
    if (t < n) {
        const int32_t j = g.idx[lo + t];
        if (j < 0 || (int64_t)j >= g.Ns) return -1;
        if (g.self_loops && (int64_t)j == i) return -1;
        return j;
    }
    return (g.self_loops && t == n) ? (int32_t)i : -1;
}

// the (row, head) pair of this lane group
struct Unit {
    int64_t unit, row;
    int h, lane;
};

// false past the launch's rows * H pairs: whole groups leave, so the shuffles of the others stay inside a group
template <int LPT>
__device__ __forceinline__ bool take_unit(int64_t rows, int H, Unit &u)
{
    const int bid = xcd_swizzle(blockIdx.x, gridDim.x);
    u.unit = (int64_t)bid * (kBlock / LPT) + threadIdx.x / LPT;
    u.lane = threadIdx.x % LPT;
    if (u.unit >= rows * H) return false;
    u.row = u.unit / H;
    u.h = (int)(u.unit - u.row * H);
    return true;
}

// The first mch entries of a chunk, kInFlight at a time: entry e's id and lane e's two scalars come by shuffle, the NROW
// head rows of the id are gathered -- all kInFlight before the first is used -- and f(e, rows, a, b) runs for the valid
// entries in ascending e.  idl < 0: no entry; that is the same for every lane of the group.
template <int LPT, int ITER, int NROW, class F>
__device__ __forceinline__ void walk_chunk(int32_t idl, float al, float bl, int mch, const Unit &u, int H, int C,
                                           const float *const (&src)[NROW], F &&f)
{
    for (int e0 = 0; e0 < mch; e0 += kInFlight) {
        int32_t id[kInFlight];
        float a[kInFlight], b[kInFlight], r[kInFlight][NROW][ITER];
#pragma unroll
        for (int v = 0; v < kInFlight; ++v) {
            const int from = (e0 + v) & (LPT - 1);
            id[v] = __shfl(idl, from, LPT);
            a[v] = __shfl(al, from, LPT);
            b[v] = __shfl(bl, from, LPT);
            if (e0 + v >= mch) id[v] = -1;
        }
#pragma unroll
        for (int v = 0; v < kInFlight; ++v) {
            // the row stride zero-extended: one 32 x 32 -> 64 multiply-add.  Sign-extended, its high half goes through a
            // register pair whose other register may be the target of a gather still in flight, and the compiler then
            // waits for that gather before it issues the next one (seen in GAT v1's backward: 0.58 -> 0.63 ms)
            const int64_t at = (int64_t)max(id[v], 0) * (unsigned)(H * C) + u.h * C;
            // written out, not a loop over NROW: a loop nested here is unrolled a pass later, the arrays reach registers
            // a pass later, and the by-target and by-source kernels of 2 channels per lane then need 66..71 VGPRs for 62..64
            load_row<LPT, ITER>(r[v][0], src[0] + at, id[v] >= 0, u.lane, C);
            if constexpr (NROW == 2) load_row<LPT, ITER>(r[v][1], src[1] + at, id[v] >= 0, u.lane, C);
        }
#pragma unroll
        for (int v = 0; v < kInFlight; ++v) {
            if (id[v] >= 0) f(e0 + v, r[v], a[v], b[v]);      // (with `continue` three kernels lose a wave per SIMD)
        }
    }
}

// The forward of one (target, head) pair: out[i,h,:] = sum_e softmax_e(score) vx[j_e,h,:], lse[i,h] = max_e score_e +
// logf(sum_e expf(score_e - max)), and (alpha != NULL) the weights of the written entries.  Score: kGather says whether
// a score needs a head row of the source -- then score.rows holds the rows and score(row) is the group's score of one
// entry -- or is a scalar that each lane forms for its own entry, score(id).
template <int LPT, int ITER, class Score>
__device__ __forceinline__ void softmax_row_fwd(const RowGraph &g, const Unit &u, int H, int C, const Score &score,
                                                const float *__restrict__ vx, float *__restrict__ out,
                                                float *__restrict__ lse, float *__restrict__ alpha)
{
    const int64_t i = u.row;
    const int h = u.h, lane = u.lane, HC = H * C;
    int64_t lo;
    int n;
    row_span(g, i, lo, n);
    const int ne = n + (g.self_loops ? 1 : 0);      // logical entries: the self entry after the row's own

    float acc[ITER];
#pragma unroll
    for (int it = 0; it < ITER; ++it) acc[it] = 0.f;
    float m = -INFINITY, l = 0.f;
    int cnt = 0;
    for (int base = 0; base < ne; base += LPT) {
        const int32_t jl = row_entry(g, i, lo, n, base + lane);      // lane l: the id of entry base + l
        const int mch = min(LPT, ne - base);
        float sl = -INFINITY;           // lane e keeps the score of entry base + e
        if constexpr (Score::kGather) {
            const float *const rows[1] = {score.rows};
            walk_chunk<LPT, ITER, 1>(jl, 0.f, 0.f, mch, u, H, C, rows, [&](int e, const float (&r)[1][ITER], float, float) {
                const float s = score(r[0]);
                if (lane == e) sl = s;
            });
        } else if (jl >= 0) {
            sl = score(jl);
        }
        if (alpha != nullptr && base + lane < n) alpha[(lo + base + lane) * H + h] = sl;     // the score, until the row's (m, l) is known
        if (group_max<LPT>(jl >= 0 ? 1.f : 0.f) == 0.f) continue;      // a chunk of empty slots: the running state stays
        // Non-finite scores follow torch.softmax of the whole row, wherever the chunks fall.  A score of -inf weighs
        // exactly 0 and is never an operand of expf: beside m_new == -inf the difference would be NaN.  While m is -inf
        // nothing finite has been added, so the state is rescaled by 0, not by expf(-inf - m_new): a NaN that a NaN score
        // left in (l, acc) stays NaN through the product, zeros stay zeros.  A finite m gives the bits of expf(m - m_new).
        const float m_new = fmaxf(m, group_max<LPT>(sl));
        const float scale = (m == -INFINITY) ? 0.f : expf(m - m_new);
        const float pl = (jl >= 0 && sl != -INFINITY) ? expf(sl - m_new) : 0.f;
        m = m_new;
        l *= scale;
#pragma unroll
        for (int it = 0; it < ITER; ++it) acc[it] *= scale;
        const float *const rows[1] = {vx};
        walk_chunk<LPT, ITER, 1>(jl, pl, 0.f, mch, u, H, C, rows, [&](int, const float (&r)[1][ITER], float p, float) {
            l += p;
#pragma unroll
            for (int it = 0; it < ITER; ++it) acc[it] += p * r[0][it];
            ++cnt;
        });
    }
    if (m == -INFINITY) l = NAN;      // every score -inf (or NaN): the row has no softmax -- NaN in out, lse and alpha
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
        const int c = lane + it * LPT;
        if (c < C) out[i * HC + h * C + c] = cnt > 0 ? acc[it] / l : 0.f;     // a row without a valid entry: zeros (R3)
    }
    if (lane == 0) lse[u.unit] = cnt > 0 ? m + logf(l) : 0.f;
    if (alpha != nullptr) {
        // each lane turns the scores it stored itself into weights; an empty slot is told by its id, not by the parked
        // value, so a valid entry whose score overflowed to -inf gets expf(-inf - m) / l like every other entry: 0
        // beside a finite m, and NaN in a row whose scores are all -inf, where out is NaN too (as torch's softmax)
        for (int t = lane; t < n; t += LPT) {
            const int64_t at = (lo + t) * H + h;
            alpha[at] = row_entry(g, i, lo, n, t) >= 0 ? expf(alpha[at] - m) / l : 0.f;
        }
    }
}

// The by-target pass's own row of the upstream gradient and its two row scalars: delta = g_out[i,h,:] . out[i,h,:], lse
template <int LPT, int ITER>
__device__ __forceinline__ void target_row(const float *__restrict__ g_out, const float *__restrict__ out,
                                           const float *__restrict__ lse, const Unit &u, int H, int C, float (&go)[ITER],
                                           float &delta, float &ls)
{
    float o[ITER];
    load_row<LPT, ITER>(go, g_out + u.row * H * C + u.h * C, true, u.lane, C);
    load_row<LPT, ITER>(o, out + u.row * H * C + u.h * C, true, u.lane, C);
    delta = group_dot<LPT, ITER>(go, o);
    ls = lse[u.unit];
}

// The by-target walk of one (target, head) pair over the NROW head rows of every valid entry: init(id, a, b) sets lane
// e's two scalars of entry e before the chunk is walked (they reach entry() by shuffle), entry(rows, a, b, alpha, gs)
// does the file's arithmetic and answers the entry's pair, which lane e keeps for one store: to alpha_w / gs_w at the
// entry's position (0, 0 in an empty slot), the implicit self entry's to alpha_self / gs_self at the pair.
template <int LPT, int ITER, int NROW, class Init, class Entry>
__device__ __forceinline__ void target_walk(const RowGraph &g, const Unit &u, int H, int C, const float *const (&src)[NROW],
                                            float *__restrict__ alpha_w, float *__restrict__ gs_w,
                                            float *__restrict__ alpha_self, float *__restrict__ gs_self, Init &&init,
                                            Entry &&entry)
{
    int64_t lo;
    int n;
    row_span(g, u.row, lo, n);
    const int ne = n + (g.self_loops ? 1 : 0);
    for (int base = 0; base < ne; base += LPT) {
        const int32_t jl = row_entry(g, u.row, lo, n, base + u.lane);
        const int mch = min(LPT, ne - base);
        float al = 0.f, gl = 0.f;        // lane e keeps alpha and g_s of entry base + e for one store
        float bl = 0.f;
        init(jl, al, bl);
        walk_chunk<LPT, ITER, NROW>(jl, al, bl, mch, u, H, C, src, [&](int e, const float (&r)[NROW][ITER], float a, float b) {
            float a_e, gs_e;
            entry(r, a, b, a_e, gs_e);
            if (u.lane == e) {
                al = a_e;
                gl = gs_e;
            }
        });
        const int t = base + u.lane;
        if (t < n) {
            const int64_t pos = (lo + t) * H + u.h;
            alpha_w[pos] = al;
            gs_w[pos] = gl;
        } else if (t == n && g.self_loops) {
            alpha_self[u.unit] = al;
            gs_self[u.unit] = gl;
        }
    }
}

// The by-source walk of one (source, head) pair: over the positions that hold source j (rev_pos, ascending; the span
// clamped to [0, M]), i = the position's row, then (self_loops) the implicit entry j -> j.  entry(rows, alpha, gs) gets
// the NROW head rows of target i and the pair the by-target pass stored.  A position outside [0, M), a row outside
// [0, Nt) and a written self loop under self_loops (skipped by target too) are no entries.  A hub's list is walked by
// its one group, however long it is.
template <int LPT, int ITER, int NROW, class Entry>
__device__ __forceinline__ void source_walk(const RowGraph &g, const Unit &u, int H, int C, const float *const (&src)[NROW],
                                            const float *__restrict__ alpha_w, const float *__restrict__ gs_w,
                                            const float *__restrict__ alpha_self, const float *__restrict__ gs_self,
                                            Entry &&entry)
{
    const int64_t j = u.row;
    const int64_t lo = min(max((int64_t)g.rev_ptr[j], (int64_t)0), g.M);
    const int64_t hi = min(max((int64_t)g.rev_ptr[j + 1], lo), g.M);
    for (int64_t base = lo; base < hi; base += LPT) {
        // lane l: target, alpha and g_s of entry base + l
        int32_t il = -1;
        float al = 0.f, gl = 0.f;
        if (base + u.lane < hi) {
            const int64_t pos = g.rev_pos[base + u.lane];
            if (pos >= 0 && pos < g.M) {
                const int64_t i = g.rowptr == nullptr ? pos / g.k : (int64_t)g.tgt[pos];
                if (i >= 0 && i < g.Nt && !(g.self_loops && i == j)) {
                    il = (int32_t)i;
                    al = alpha_w[pos * H + u.h];
                    gl = gs_w[pos * H + u.h];
                }
            }
        }
        const int mch = (int)min((int64_t)LPT, hi - base);
        walk_chunk<LPT, ITER, NROW>(il, al, gl, mch, u, H, C, src,
                                    [&](int, const float (&r)[NROW][ITER], float a, float gs) { entry(r, a, gs); });
    }
    if (g.self_loops) {      // Nt == Ns
        float r[NROW][ITER];
        load_row<LPT, ITER>(r[0], src[0] + j * H * C + u.h * C, true, u.lane, C);
        if constexpr (NROW == 2) load_row<LPT, ITER>(r[1], src[1] + j * H * C + u.h * C, true, u.lane, C);
        entry(r, alpha_self[u.unit], gs_self[u.unit]);
    }
}

// ---- host side ----

// one launch over rows * H pairs, kBlock / LPT to a workgroup (the kernels undo the XCD deal themselves); no row: no launch
template <int LPT, class Kernel, class... Args>
int launch(const char *name, Kernel kernel, int64_t rows, int H, hipStream_t st, Args... args)
{
    constexpr int TPB = kBlock / LPT;
    const int64_t blocks = (rows * H + TPB - 1) / TPB;
    if (blocks == 0) return 0;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(kBlock), 0, st, args...);
    DMET_LAUNCH_CHECK(name);
    return 0;
}

// lanes per (row, head) pair and channels per lane for a head width C: 16 lanes up to 32 channels, 32 beyond;
// f(lpt, iter) gets them as integral constants
template <class F>
int dispatch_width(int C, F &&f)
{
    using std::integral_constant;
    if (C <= 16) return f(integral_constant<int, 16>{}, integral_constant<int, 1>{});
    if (C <= 32) return f(integral_constant<int, 16>{}, integral_constant<int, 2>{});
    return f(integral_constant<int, 32>{}, integral_constant<int, 2>{});
}

bool supported(int H, int C) { return C >= 1 && C <= kMaxC && H >= 1 && H <= kMaxH && H * C <= kMaxHC; }

int check_graph_shape(const char *who, bool list, int64_t Nt, int64_t Ns, int64_t E, int k, int H, int C)
{
    DMET_REQUIRE(Nt >= 0 && Ns >= 0 && Nt < (int64_t)2147483647 && Ns < (int64_t)2147483647,
                 "%s: Nt=%lld, Ns=%lld out of range", who, (long long)Nt, (long long)Ns);
    DMET_REQUIRE(supported(H, C), "%s: H=%d, C=%d not in 1 <= C <= %d, 1 <= H <= %d, H*C <= %d", who, H, C, kMaxC, kMaxH,
                 kMaxHC);
    if (list)
        DMET_REQUIRE(E >= 0 && E < (int64_t)2147483647, "%s: E=%lld out of range", who, (long long)E);
    else
        DMET_REQUIRE(k >= 1 && k <= DMET_MAX_K, "%s: k=%d not in [1,%d] (table form: rowptr NULL)", who, k, DMET_MAX_K);
    DMET_REQUIRE(list || Nt * (int64_t)k < (int64_t)2147483647, "%s: Nt*k out of range", who);
    // a launch covers Nt*H (Ns*H) lane groups, at least 8 to a workgroup
    DMET_REQUIRE(Nt * (int64_t)H < (int64_t)2147483647 * 4 && Ns * (int64_t)H < (int64_t)2147483647 * 4,
                 "%s: Nt*H or Ns*H out of range", who);
    return 0;
}

// the graph of a checked call: width is the table's k (rowptr NULL) and unused for a list
RowGraph make_graph(const int32_t *idx, const int32_t *rowptr, const int32_t *tgt, const int32_t *rev_ptr,
                    const int32_t *rev_pos, int64_t Nt, int64_t Ns, int64_t E, int width, int self_loops)
{
    const bool list = rowptr != nullptr;
    return RowGraph{idx, rowptr, tgt, rev_ptr, rev_pos, Nt, Ns, list ? E : Nt * (int64_t)width, list ? 0 : width, self_loops};
}

}  // namespace
}  // namespace dmet

// pointnet.hip -- PointNet set abstraction (torch_geometric.nn.PointNetConv's message and max aggregation) for
// local_nn = Linear(F + D, H1) - act - Linear(H1, H2) [- act] over a fixed-width table or a grouped edge list, forward
// and backward.
//
//   out[i, o] = max over the entries e of target i of m_e[o],   m_e = act2?(W2 act(A_src(e) - B_i) + b2)
//   A = x_src W1x^T + pos_src W1p^T + b1  (sources)     B = pos_dst W1p^T  (targets)     W1 = [W1x | W1p]
// so that only the second Linear and the max are per-entry work.  self_loop (one node set): entries with src == i are
// skipped and one implicit entry i -> i, h1 = act(S_i) with S = x W1x^T + b1 (a position difference of exactly 0), is
// taken after the row's own.  A target without an entry gives zeros, win -1.
//
// Forward
//   1. node level (pn_node_fwd_kernel, one launch): A, B and -- with self_loop -- S; with one node set A, B and S of a row
//      come from one pass over it.
//   2. entry pass (pn_fwd_kernel): a wavefront owns a target and walks its entries in tiles of 16.  h1 of the tile goes to
//      the wavefront's LDS, z2 = h1 W2^T + b2 runs on the fp32 matrix cores (v_mfma_f32_16x16x4_f32: tile entries x 16
//      channels per block, k in steps of 16), and the running (max, winner) of a channel is kept in registers in entry
//      order: strict compares, so the earliest entry wins a tie (R4); a NaN message never wins and never blocks, and a
//      channel whose messages are all NaN is NaN with win -1.  Nothing per entry is written.
// Backward (out and win are the forward's)
//   g_z2[i, o] = g_out[i, o] act2'(out[i, o]) belongs to the one entry win[i, o] names; the tile's routed g_z2 [16, H2]
//   goes to LDS and g_h1 = g_z2 W2 runs on the matrix cores, g_pre1 = g_h1 act'(h1) with h1 formed again.
//   1. by target (pn_bwd_target_kernel): gB[i] = -sum over the row's own entries of g_pre1 (entry order), gS[i] = g_pre1
//      of the implicit entry, gW2 += g_z2^T h1 (matrix cores, one accumulator set per wavefront) and gb2; the wavefronts
//      of a workgroup add up in wavefront order, one partial per workgroup, summed in workgroup order in double (chunks
//      of 32 workgroups, then the chunks).
//   2. by source (pn_bwd_source_kernel): a wavefront owns four consecutive sources and walks the positions that hold them
//      (one run of the reverse index, ascending) in tiles of 16, a tile's rows added to their own source:
//      gA[j] = sum g_pre1.  A source nobody lists gets zeros.
//   3. node level: gx = (gA + gS) W1x, gpos_src = gA W1p, gpos_dst = gB W1p.  gW1 and gb1 follow from gA, gS, gB on the
//      caller's side (dmet_xty_f32).
// No float atomics; every output element is written once; sums run in entry / reverse-index / workgroup order, so two
// runs give the same bits, and a table and the list of the same entries in the same order give the same bits (the tiles
// are cut from the row's own entry numbers in both forms).  Every loop is bounded by a row length read once and clamped.
#include <math.h>

#include "common.h"

namespace dmet {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kPnBlock = 256;        // four wavefronts, each with targets (sources) of its own
constexpr int kPnWaves = kPnBlock / kWave;
constexpr int kPnTile = 16;          // entries per tile: the M of a 16 x 16 x 4 product
constexpr int kPnMaxF = 128, kPnMaxD = 8, kPnMaxH1 = 128, kPnMaxH2 = 128;
constexpr int kPnMaxBlocks = 1024;   // entry-pass workgroups: the number of gW2 partials
constexpr int kPnNone = 0x7fffffff;  // "no entry yet" in the running winner
constexpr int kPnRows = 16;          // rows per workgroup of the node-level kernels
constexpr int kPnGroup = 4;          // consecutive sources a wavefront of the by-source pass owns: their lists share tiles
constexpr int kPnChunk = 32;         // gW2 partials per first-stage sum

__device__ __forceinline__ void pn_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__host__ __device__ __forceinline__ int pn_pad16(int h) { return (h + 15) & ~15; }
// LDS row stride of a [rows][h] image: whole 16-column blocks plus 4, an odd number of float4 -- the 16 rows a float4
// read of the matrix-core operands touches fall on distinct banks
__host__ __device__ __forceinline__ int pn_stride(int h) { return pn_pad16(h) + 4; }

// act: 0 ReLU, 1 ELU (alpha 1)
__device__ __forceinline__ float pn_act(float v, int act) { return v > 0.0f ? v : (act ? expm1f(v) : 0.0f); }
// the derivative, from the activation's output
__device__ __forceinline__ float pn_dact(float h, int act) { return h > 0.0f ? 1.0f : (act ? h + 1.0f : 0.0f); }

struct PnGraph {
    const int32_t *idx;       // nbr[Nt, width] (table) or src[E] (list)
    const int32_t *rowptr;    // NULL: table
    const int32_t *tgt;       // list, by-source pass only
    const int32_t *cnt;       // table: optional slot counts
    const int32_t *rev_ptr, *rev_pos;
    int64_t Nt, Ns, M;        // M = Nt*width or E: the number of positions
    int width;
    int self_loop;
};

// positions [lo, lo + n) of row i, clamped to [0, M]
__device__ __forceinline__ void pn_row(const PnGraph &g, int64_t i, int64_t &lo, int &n)
{
    if (g.rowptr == nullptr) {
        lo = i * g.width;
        n = g.width;
        if (g.cnt != nullptr) n = min(max(g.cnt[i], 0), g.width);
    } else {
        lo = min(max((int64_t)g.rowptr[i], (int64_t)0), g.M);
        const int64_t hi = min(max((int64_t)g.rowptr[i + 1], lo), g.M);
        n = (int)(hi - lo);
    }
}

// what win holds for entry t of a row that starts at lo with n own entries
__device__ __forceinline__ int32_t pn_code(const PnGraph &g, int64_t lo, int n, int t)
{
    if (g.self_loop && t == n) return -2;
    return g.rowptr == nullptr ? t : (int32_t)(lo + t);
}

// ---- node level ------------------------------------------------------------------------------------------------------
// Wt[k][c] = W1[c][k], k < F + D
__global__ void pn_transpose_kernel(const float *__restrict__ W1, int K, int H1, float *__restrict__ Wt)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= K * H1) return;
    const int c = t / K, k = t - c * K;
    Wt[(int64_t)k * H1 + c] = W1[t];
}

// Workgroups [0, nbs) take 16 source rows each: S = b1 + x W1x^T (ascending f), P = pos W1p^T (ascending d), A = S + P,
// and with one node set B = P.  Workgroups [nbs, ...) take 16 target rows: B = P.
__global__ __launch_bounds__(128) void pn_node_fwd_kernel(const float *__restrict__ x, int F, const float *__restrict__ pos_src,
                                                          const float *__restrict__ pos_dst, int D, int64_t Ns, int64_t Nt,
                                                          int one_set, int nbs, const float *__restrict__ Wt,
                                                          const float *__restrict__ b1, int H1, float *__restrict__ A,
                                                          float *__restrict__ B, float *__restrict__ S)
{
    __shared__ float xs[kPnMaxF + kPnMaxD][kPnRows];
    const bool src_rows = (int)blockIdx.x < nbs;
    const int64_t N = src_rows ? Ns : Nt;
    const int64_t n0 = (int64_t)(src_rows ? blockIdx.x : blockIdx.x - nbs) * kPnRows;
    const float *pos = src_rows ? pos_src : pos_dst;
    const int Fx = src_rows ? F : 0;
    for (int idx = threadIdx.x; idx < kPnRows * Fx; idx += blockDim.x) {
        const int r = idx / Fx, k = idx - r * Fx;
        xs[k][r] = n0 + r < N ? x[(n0 + r) * F + k] : 0.0f;
    }
    for (int idx = threadIdx.x; idx < kPnRows * D; idx += blockDim.x) {
        const int r = idx / D, k = idx - r * D;
        xs[kPnMaxF + k][r] = n0 + r < N ? pos[(n0 + r) * D + k] : 0.0f;
    }
    __syncthreads();
    const int m = threadIdx.x;
    if (m >= H1) return;
    float s[kPnRows], p[kPnRows];
    const float bv = (src_rows && b1) ? b1[m] : 0.0f;
#pragma unroll
    for (int r = 0; r < kPnRows; ++r) {
        s[r] = bv;
        p[r] = 0.0f;
    }
    for (int k = 0; k < Fx; ++k) {
        const float w = Wt[(int64_t)k * H1 + m];
#pragma unroll
        for (int r = 0; r < kPnRows; ++r) s[r] = __builtin_fmaf(xs[k][r], w, s[r]);
    }
    for (int k = 0; k < D; ++k) {
        const float w = Wt[(int64_t)(F + k) * H1 + m];
#pragma unroll
        for (int r = 0; r < kPnRows; ++r) p[r] = __builtin_fmaf(xs[kPnMaxF + k][r], w, p[r]);
    }
#pragma unroll
    for (int r = 0; r < kPnRows; ++r) {
        if (n0 + r >= N) continue;
        const int64_t at = (n0 + r) * H1 + m;
        if (src_rows) {
            A[at] = s[r] + p[r];
            if (S) S[at] = s[r];
            if (one_set) B[at] = p[r];
        } else {
            B[at] = p[r];
        }
    }
}

// Y[n][f] = sum_c (G[n][c] + G2[n][c]) W1[c][off + f], f < M, ascending c (G2 may be NULL); 16 rows per workgroup
__global__ __launch_bounds__(128) void pn_node_bwd_kernel(const float *__restrict__ G, const float *__restrict__ G2, int64_t N,
                                                          int H1, const float *__restrict__ W1, int ld, int off, int M,
                                                          float *__restrict__ Y)
{
    __shared__ float gs[kPnMaxH1][kPnRows];
    const int64_t n0 = (int64_t)blockIdx.x * kPnRows;
    for (int idx = threadIdx.x; idx < kPnRows * H1; idx += blockDim.x) {
        const int r = idx / H1, c = idx - r * H1;
        float v = 0.0f;
        if (n0 + r < N) {
            v = G[(n0 + r) * H1 + c];
            if (G2) v += G2[(n0 + r) * H1 + c];
        }
        gs[c][r] = v;
    }
    __syncthreads();
    const int f = threadIdx.x;
    if (f >= M) return;
    float acc[kPnRows];
#pragma unroll
    for (int r = 0; r < kPnRows; ++r) acc[r] = 0.0f;
    for (int c = 0; c < H1; ++c) {
        const float w = W1[(int64_t)c * ld + off + f];
#pragma unroll
        for (int r = 0; r < kPnRows; ++r) acc[r] = __builtin_fmaf(gs[c][r], w, acc[r]);
    }
#pragma unroll
    for (int r = 0; r < kPnRows; ++r)
        if (n0 + r < N) Y[(n0 + r) * M + f] = acc[r];
}

// ---- the entry passes ------------------------------------------------------------------------------------------------
// Every lane of the wavefront: the source id of entry base + (lane & 15) of target i's row, -1 for a slot that is no
// entry (empty, out of range, a written self loop under self_loop, beyond the row); the implicit entry is number n.
__device__ __forceinline__ int32_t pn_entry(const PnGraph &g, int64_t i, int64_t lo, int n, int t)
{
    if (t < n) {
        const int32_t v = g.idx[lo + t];
        if (v >= 0 && (int64_t)v < g.Ns && !(g.self_loop && (int64_t)v == i)) return v;
        return -1;
    }
    return (g.self_loop && t == n) ? (int32_t)i : -1;
}

// h1 tile of a target: row e = act(A[j_e] - B_i), or act(S_i) for the implicit entry; zeros for a row without an entry
// and in the padding columns [H1, pad16(H1))
__device__ __forceinline__ void pn_fill_h1_target(const float *__restrict__ A, const float *__restrict__ S, const float (&bi)[2],
                                                  int64_t i, int32_t jl, int self_at, int H1, int act, float *h1s, int lane)
{
    const int H1P = pn_pad16(H1), H1S = pn_stride(H1);
#pragma unroll 4
    for (int e = 0; e < kPnTile; ++e) {
        const int32_t j = __shfl(jl, e, kWave);
        const float *row = (e == self_at) ? S + i * H1 : A + (int64_t)max(j, 0) * H1;
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int k = lane + it * kWave;
            if (k >= H1P) continue;
            float h = 0.0f;
            if (j >= 0 && k < H1) h = pn_act(e == self_at ? row[k] : row[k] - bi[it], act);
            h1s[e * H1S + k] = h;
        }
    }
}

template <int H2>
__global__ __launch_bounds__(kPnBlock) void pn_fwd_kernel(const float *__restrict__ A, const float *__restrict__ B,
                                                          const float *__restrict__ S, PnGraph g, int H1,
                                                          const float *__restrict__ W2, const float *__restrict__ b2, int act,
                                                          int act2, float *__restrict__ out, int32_t *__restrict__ win)
{
    constexpr int NCB = H2 / 16;
    extern __shared__ float4 pn_lds4[];
    float *lds = reinterpret_cast<float *>(pn_lds4);
    const int H1P = pn_pad16(H1), H1S = pn_stride(H1);
    float *w2s = lds;                              // [H2][H1S]: W2 rows, zeros in the padding columns
    float *b2s = w2s + H2 * H1S;                   // [H2]
    const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
    float *h1s = b2s + H2 + wave * kPnTile * H1S;  // [16][H1S], the wavefront's own
    for (int idx = threadIdx.x; idx < H2 * H1P; idx += kPnBlock) {
        const int o = idx / H1P, c = idx - o * H1P;
        w2s[o * H1S + c] = c < H1 ? W2[o * H1 + c] : 0.0f;
    }
    for (int o = threadIdx.x; o < H2; o += kPnBlock) b2s[o] = b2 ? b2[o] : 0.0f;
    __syncthreads();

    const int m = lane & 15, q = lane >> 4;
    float bias[NCB];
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) bias[cb] = b2s[cb * 16 + m];
    const int64_t stride = (int64_t)gridDim.x * kPnWaves;
    for (int64_t i = (int64_t)blockIdx.x * kPnWaves + wave; i < g.Nt; i += stride) {
        int64_t lo;
        int n;
        pn_row(g, i, lo, n);
        const int total = n + (g.self_loop ? 1 : 0);
        float bi[2];
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int k = lane + it * kWave;
            bi[it] = k < H1 ? B[i * H1 + k] : 0.0f;
        }
        float rv[NCB];
        int rt[NCB];
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) {
            rv[cb] = 0.0f;
            rt[cb] = kPnNone;
        }
        bool seen = false;                     // the row has an entry
        for (int base = 0; base < total; base += kPnTile) {
            const int32_t jl = pn_entry(g, i, lo, n, base + m);
            const unsigned mask = (unsigned)(__ballot(jl >= 0) & 0xffffull);
            if (mask == 0u) continue;          // a tile of empty slots: the same for the whole wavefront
            seen = true;
            pn_wave_sync();                    // the previous tile's reads of h1s are done
            pn_fill_h1_target(A, S, bi, i, jl, g.self_loop ? n - base : -1, H1, act, h1s, lane);
            pn_wave_sync();
            f32x4 acc[NCB];
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb) acc[cb] = f32x4{bias[cb], bias[cb], bias[cb], bias[cb]};
            for (int kb = 0; kb < H1P; kb += 16) {
                const float4 a = *reinterpret_cast<const float4 *>(&h1s[m * H1S + kb + 4 * q]);
#pragma unroll
                for (int cb = 0; cb < NCB; ++cb) {
                    const float4 b = *reinterpret_cast<const float4 *>(&w2s[(cb * 16 + m) * H1S + kb + 4 * q]);
                    acc[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc[cb], 0, 0, 0);
                    acc[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc[cb], 0, 0, 0);
                    acc[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc[cb], 0, 0, 0);
                    acc[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc[cb], 0, 0, 0);
                }
            }
            // acc[cb][r]: entry base + 4 q + r, channel 16 cb + m
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb) {
                float bv = NAN;        // NaN: no number among this quarter's messages yet
                int bt = kPnNone;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int e = 4 * q + r;
                    if (!((mask >> e) & 1u)) continue;
                    const float v = act2 ? pn_act(acc[cb][r], act) : acc[cb][r];
                    // while bv is NaN any message replaces it, so the first number is taken whatever it is (+-inf too);
                    // once bv is a number a NaN fails the comparison: it never wins and never blocks, wherever in the
                    // row and in whichever quarter of the wavefront it stands
                    if (v > bv || bv != bv) {
                        bv = v;
                        bt = base + e;
                    }
                }
                // a NaN that stood in for "none" names no entry: a (value, entry) pair with an entry always holds a
                // number, and the two merges below need no more
                if (bv != bv) bt = kPnNone;
#pragma unroll
                for (int off = 16; off < kWave; off <<= 1) {
                    const float ov = __shfl_xor(bv, off, kWave);
                    const int ot = __shfl_xor(bt, off, kWave);
                    if (ot != kPnNone && (bt == kPnNone || ov > bv || (ov == bv && ot < bt))) {
                        bv = ov;
                        bt = ot;
                    }
                }
                if (bt != kPnNone && (rt[cb] == kPnNone || bv > rv[cb])) {
                    rv[cb] = bv;
                    rt[cb] = bt;
                }
            }
        }
        if (q == 0) {
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb) {
                const int64_t at = i * H2 + cb * 16 + m;
                // no entry: zeros (R3).  Entries, but no number among a channel's messages: NaN, win -1
                out[at] = rt[cb] == kPnNone ? (seen ? NAN : 0.0f) : rv[cb];
                win[at] = rt[cb] == kPnNone ? -1 : pn_code(g, lo, n, rt[cb]);
            }
        }
    }
}

// g_pre1 of the tile in the wavefront's LDS: gp[cb][r] belongs to entry 4 q + r and channel 16 cb + m.
// g_h1 = gzt [16][H2] . W2 (w2t[c][o] = W2[o][c]) on the matrix cores, times act'(h1).
template <int H2, int NCB1>
__device__ __forceinline__ void pn_gpre_tile(const float *gzt, const float *h1s, const float *w2t, int H1, int act, int m, int q,
                                             f32x4 (&gp)[NCB1])
{
    constexpr int H2S = H2 + 4;
    const int H1P = pn_pad16(H1), H1S = pn_stride(H1);
#pragma unroll
    for (int cb = 0; cb < NCB1; ++cb) gp[cb] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    for (int ob = 0; ob < H2; ob += 16) {
        const float4 a = *reinterpret_cast<const float4 *>(&gzt[m * H2S + ob + 4 * q]);
#pragma unroll
        for (int cb = 0; cb < NCB1; ++cb) {
            if (cb * 16 >= H1P) continue;
            const float4 b = *reinterpret_cast<const float4 *>(&w2t[(cb * 16 + m) * H2S + ob + 4 * q]);
            gp[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, gp[cb], 0, 0, 0);
            gp[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, gp[cb], 0, 0, 0);
            gp[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, gp[cb], 0, 0, 0);
            gp[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, gp[cb], 0, 0, 0);
        }
    }
#pragma unroll
    for (int cb = 0; cb < NCB1; ++cb) {
        if (cb * 16 >= H1P) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) gp[cb][r] *= pn_dact(h1s[(4 * q + r) * H1S + cb * 16 + m], act);
    }
}

// stage w2t[c][o] = W2[o][c] (zeros for c in [H1, pad16(H1)))
template <int H2>
__device__ __forceinline__ void pn_stage_w2t(const float *__restrict__ W2, int H1, float *w2t)
{
    constexpr int H2S = H2 + 4;
    const int H1P = pn_pad16(H1);
    for (int idx = threadIdx.x; idx < H2 * H1P; idx += kPnBlock) {
        const int o = idx / H1P, c = idx - o * H1P;
        w2t[c * H2S + o] = c < H1 ? W2[o * H1 + c] : 0.0f;
    }
}

// sum over the four lane groups of a wavefront, in a fixed order
__device__ __forceinline__ float pn_quad_sum(float v)
{
    v += __shfl_xor(v, 16, kWave);
    v += __shfl_xor(v, 32, kWave);
    return v;
}

template <int H2, int NCB1>
__global__ __launch_bounds__(kPnBlock) void pn_bwd_target_kernel(
    const float *__restrict__ A, const float *__restrict__ B, const float *__restrict__ S, PnGraph g, int H1,
    const float *__restrict__ W2, int act, int act2, const float *__restrict__ out, const int32_t *__restrict__ win,
    const float *__restrict__ g_out, float *__restrict__ gB, float *__restrict__ gS, float *__restrict__ partial)
{
    constexpr int NCB2 = H2 / 16, H2S = H2 + 4;
    extern __shared__ float4 pn_lds4[];
    float *lds = reinterpret_cast<float *>(pn_lds4);
    const int H1P = pn_pad16(H1), H1S = pn_stride(H1);
    const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
    float *w2t = lds;                                          // [H1P][H2S]
    float *h1all = w2t + H1P * H2S;                            // [4][16][H1S]
    float *h1s = h1all + wave * kPnTile * H1S;
    float *gzt = h1all + kPnWaves * kPnTile * H1S + wave * kPnTile * H2S;   // [4][16][H2S]
    pn_stage_w2t<H2>(W2, H1, w2t);
    __syncthreads();

    const int m = lane & 15, q = lane >> 4;
    f32x4 gw[NCB2][NCB1];        // gW2 block (ob, cb): rows o = 16 ob + 4 q + r, column c = 16 cb + m
#pragma unroll
    for (int ob = 0; ob < NCB2; ++ob)
#pragma unroll
        for (int cb = 0; cb < NCB1; ++cb) gw[ob][cb] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    float gb[2] = {0.0f, 0.0f};  // gb2 of channels lane, lane + 64
    const int64_t stride = (int64_t)gridDim.x * kPnWaves;
    for (int64_t i = (int64_t)blockIdx.x * kPnWaves + wave; i < g.Nt; i += stride) {
        int64_t lo;
        int n;
        pn_row(g, i, lo, n);
        const int total = n + (g.self_loop ? 1 : 0);
        float bi[2], gz[2];
        int32_t wn[2];
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int k = lane + it * kWave;
            bi[it] = k < H1 ? B[i * H1 + k] : 0.0f;
            gz[it] = 0.0f;
            wn[it] = -1;
            if (k < H2) {
                wn[it] = win[i * H2 + k];
                if (wn[it] != -1) gz[it] = g_out[i * H2 + k] * (act2 ? pn_dact(out[i * H2 + k], act) : 1.0f);
            }
            gb[it] += gz[it];
        }
        float sb[NCB1];
#pragma unroll
        for (int cb = 0; cb < NCB1; ++cb) sb[cb] = 0.0f;
        for (int base = 0; base < total; base += kPnTile) {
            const int32_t jl = pn_entry(g, i, lo, n, base + m);
            const unsigned mask = (unsigned)(__ballot(jl >= 0) & 0xffffull);
            if (mask == 0u) continue;
            pn_wave_sync();
            pn_fill_h1_target(A, S, bi, i, jl, g.self_loop ? n - base : -1, H1, act, h1s, lane);
            for (int e = 0; e < kPnTile; ++e) {
                const bool on = (mask >> e) & 1u;
                const int32_t code = pn_code(g, lo, n, base + e);
#pragma unroll
                for (int it = 0; it < 2; ++it) {
                    const int o = lane + it * kWave;
                    if (o < H2) gzt[e * H2S + o] = (on && wn[it] == code) ? gz[it] : 0.0f;
                }
            }
            pn_wave_sync();
            f32x4 gp[NCB1];
            pn_gpre_tile<H2, NCB1>(gzt, h1s, w2t, H1, act, m, q, gp);
            const int self_e = g.self_loop ? n - base : -1;      // the implicit entry's row in this tile, if it is here
#pragma unroll
            for (int cb = 0; cb < NCB1; ++cb) {
                const int c = cb * 16 + m;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (4 * q + r == self_e) {
                        if (c < H1) gS[i * H1 + c] = gp[cb][r];
                    } else {
                        sb[cb] += gp[cb][r];
                    }
                }
            }
            // gW2 += g_z2^T h1 over the tile's 16 entries: k = entry 4 q + s
            float hb[NCB1][4];
#pragma unroll
            for (int cb = 0; cb < NCB1; ++cb)
#pragma unroll
                for (int s = 0; s < 4; ++s) hb[cb][s] = cb * 16 < H1P ? h1s[(4 * q + s) * H1S + cb * 16 + m] : 0.0f;
#pragma unroll
            for (int ob = 0; ob < NCB2; ++ob) {
                float za[4];
#pragma unroll
                for (int s = 0; s < 4; ++s) za[s] = gzt[(4 * q + s) * H2S + ob * 16 + m];
#pragma unroll
                for (int cb = 0; cb < NCB1; ++cb) {
                    if (cb * 16 >= H1P) continue;
#pragma unroll
                    for (int s = 0; s < 4; ++s)
                        gw[ob][cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(za[s], hb[cb][s], gw[ob][cb], 0, 0, 0);
                }
            }
        }
#pragma unroll
        for (int cb = 0; cb < NCB1; ++cb) {
            const float v = pn_quad_sum(sb[cb]);
            const int c = cb * 16 + m;
            if (q == 0 && c < H1) gB[i * H1 + c] = -v;
        }
    }
    // one partial per workgroup: gW2 [H2][H1] | gb2 [H2], the wavefronts added in wavefront order through LDS
    __syncthreads();
    float *red = w2t;                    // [H2][H1] fits in [H1P][H2S]
    float *redb = h1all;                 // [4][128]
    for (int w = 0; w < kPnWaves; ++w) {
        if (wave == w) {
#pragma unroll
            for (int ob = 0; ob < NCB2; ++ob)
#pragma unroll
                for (int cb = 0; cb < NCB1; ++cb)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int o = ob * 16 + 4 * q + r, c = cb * 16 + m;
                        if (c < H1) red[o * H1 + c] = (w == 0 ? 0.0f : red[o * H1 + c]) + gw[ob][cb][r];
                    }
            redb[w * kPnMaxH2 + lane] = gb[0];
            redb[w * kPnMaxH2 + kWave + lane] = gb[1];
        }
        __syncthreads();
    }
    float *pb = partial + (int64_t)blockIdx.x * (H2 * H1 + H2);
    for (int idx = threadIdx.x; idx < H2 * H1; idx += kPnBlock) pb[idx] = red[idx];
    for (int o = threadIdx.x; o < H2; o += kPnBlock) {
        float a = 0.0f;
        for (int w = 0; w < kPnWaves; ++w) a += redb[w * kPnMaxH2 + o];
        pb[H2 * H1 + o] = a;
    }
}

template <int H2, int NCB1>
__global__ __launch_bounds__(kPnBlock) void pn_bwd_source_kernel(
    const float *__restrict__ A, const float *__restrict__ B, PnGraph g, int H1, const float *__restrict__ W2, int act,
    int act2, const float *__restrict__ out, const int32_t *__restrict__ win, const float *__restrict__ g_out,
    float *__restrict__ gA)
{
    constexpr int H2S = H2 + 4;
    extern __shared__ float4 pn_lds4[];
    float *lds = reinterpret_cast<float *>(pn_lds4);
    const int H1P = pn_pad16(H1), H1S = pn_stride(H1);
    const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
    float *w2t = lds;
    float *h1all = w2t + H1P * H2S;
    float *h1s = h1all + wave * kPnTile * H1S;
    float *gzt = h1all + kPnWaves * kPnTile * H1S + wave * kPnTile * H2S;
    pn_stage_w2t<H2>(W2, H1, w2t);
    __syncthreads();

    const int m = lane & 15, q = lane >> 4;
    const int64_t stride = (int64_t)gridDim.x * kPnWaves;
    const int64_t ngroups = (g.Ns + kPnGroup - 1) / kPnGroup;
    for (int64_t grp = (int64_t)blockIdx.x * kPnWaves + wave; grp < ngroups; grp += stride) {
        // the lists of kPnGroup consecutive sources are one run of the reverse index: [lo, ends[0]), [ends[0], ends[1]), ...
        const int64_t j0 = grp * kPnGroup;
        const int64_t lo = min(max((int64_t)g.rev_ptr[j0], (int64_t)0), g.M);
        int64_t ends[kPnGroup];
        int64_t prev = lo;
#pragma unroll
        for (int gi = 0; gi < kPnGroup; ++gi) {
            const int64_t jj = min(j0 + gi + 1, g.Ns);
            ends[gi] = min(max((int64_t)g.rev_ptr[jj], prev), g.M);
            prev = ends[gi];
        }
        const int64_t hi = prev;
        float sa[kPnGroup][NCB1];
#pragma unroll
        for (int gi = 0; gi < kPnGroup; ++gi)
#pragma unroll
            for (int cb = 0; cb < NCB1; ++cb) sa[gi][cb] = 0.0f;
        for (int64_t base = lo; base < hi; base += kPnTile) {
            // every lane: the source (as its number in the group), the target and the win code of position base + m of the
            // run; target -1 when the position is no entry of that source
            int32_t il = -1, code = -1, jl = 0;
            int gl = 0;
            if (base + m < hi) {
#pragma unroll
                for (int gi = 0; gi + 1 < kPnGroup; ++gi) gl += (base + m >= ends[gi]) ? 1 : 0;
                const int64_t j = j0 + gl;
                const int64_t p = g.rev_pos[base + m];
                if (j < g.Ns && p >= 0 && p < g.M && (int64_t)g.idx[p] == j) {
                    const int64_t i = g.rowptr == nullptr ? p / g.width : (int64_t)g.tgt[p];
                    if (i >= 0 && i < g.Nt && !(g.self_loop && i == j)) {
                        const int t = (int)(p - i * g.width);
                        if (g.rowptr != nullptr || g.cnt == nullptr || t < g.cnt[i]) {
                            il = (int32_t)i;
                            jl = (int32_t)j;
                            code = g.rowptr == nullptr ? t : (int32_t)p;
                        }
                    }
                }
            }
            const unsigned mask = (unsigned)(__ballot(il >= 0) & 0xffffull);
            if (mask == 0u) continue;
            pn_wave_sync();
#pragma unroll 4
            for (int e = 0; e < kPnTile; ++e) {
                const int32_t i = __shfl(il, e, kWave);
                const int32_t ce = __shfl(code, e, kWave);
                const int64_t jr = __shfl(jl, e, kWave);
                const int64_t ir = max(i, 0);
#pragma unroll
                for (int it = 0; it < 2; ++it) {
                    const int k = lane + it * kWave;
                    if (k < H1P)
                        h1s[e * H1S + k] = (i >= 0 && k < H1) ? pn_act(A[jr * H1 + k] - B[ir * H1 + k], act) : 0.0f;
                    if (k < H2) {
                        float z = 0.0f;
                        if (i >= 0 && win[ir * H2 + k] == ce)
                            z = g_out[ir * H2 + k] * (act2 ? pn_dact(out[ir * H2 + k], act) : 1.0f);
                        gzt[e * H2S + k] = z;
                    }
                }
            }
            pn_wave_sync();
            f32x4 gp[NCB1];
            pn_gpre_tile<H2, NCB1>(gzt, h1s, w2t, H1, act, m, q, gp);
            int gr[4];        // the group number of rows 4 q + r (lanes 0..15 hold entries 0..15)
#pragma unroll
            for (int r = 0; r < 4; ++r) gr[r] = __shfl(gl, 4 * q + r, kWave);
#pragma unroll
            for (int gi = 0; gi < kPnGroup; ++gi)
#pragma unroll
                for (int cb = 0; cb < NCB1; ++cb)
#pragma unroll
                    for (int r = 0; r < 4; ++r) sa[gi][cb] += gr[r] == gi ? gp[cb][r] : 0.0f;
        }
#pragma unroll
        for (int gi = 0; gi < kPnGroup; ++gi) {
            if (j0 + gi >= g.Ns) break;          // the same for the whole wavefront
#pragma unroll
            for (int cb = 0; cb < NCB1; ++cb) {
                const float v = pn_quad_sum(sa[gi][cb]);
                const int c = cb * 16 + m;
                if (q == 0 && c < H1) gA[(j0 + gi) * H1 + c] = v;
            }
        }
    }
}

// stage 1 (chunk = blockIdx.y): sums[chunk][t] = sum of partial[b][t] over the chunk's kPnChunk workgroups, ascending b;
// stage 2 (one chunk, from = sums): the chunks in ascending order.  double throughout.
template <typename T>
__global__ __launch_bounds__(256) void pn_sum_kernel(const T *__restrict__ from, int nb, int n, double *__restrict__ sums,
                                                     int H2H1, float *__restrict__ gW2, float *__restrict__ gb2)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const int b0 = blockIdx.y * kPnChunk, b1 = min(nb, b0 + kPnChunk);
    double a = 0.0;
    for (int b = b0; b < b1; ++b) a += (double)from[(int64_t)b * n + t];
    if (sums) {
        sums[(int64_t)blockIdx.y * n + t] = a;
    } else if (t < H2H1) {
        if (gW2) gW2[t] = (float)a;
    } else if (gb2) {
        gb2[t - H2H1] = (float)a;
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------
bool supported(int F, int D, int H1, int H2)
{
    return F >= 0 && F <= kPnMaxF && D >= 1 && D <= kPnMaxD && H1 >= 1 && H1 <= kPnMaxH1 &&
           (H2 == 16 || H2 == 32 || H2 == 64 || H2 == 128);
}

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// workspace: W1^T [F + D][H1] (forward) | gW2, gb2 partials [kPnMaxBlocks][H2 H1 + H2] (backward)
struct PnWorkspace {
    float *wt, *partial;
    double *sums;       // [kPnMaxBlocks / kPnChunk][H2 H1 + H2]
    size_t bytes;
};

PnWorkspace carve(int F, int D, int H1, int H2, void *ws)
{
    const size_t wt = align256(sizeof(float) * (size_t)(F + D) * H1);
    const size_t part = align256(sizeof(float) * (size_t)kPnMaxBlocks * ((size_t)H2 * H1 + H2));
    char *base = reinterpret_cast<char *>((reinterpret_cast<uintptr_t>(ws) + 255u) & ~(uintptr_t)255u);
    PnWorkspace c;
    c.wt = reinterpret_cast<float *>(base);
    c.partial = reinterpret_cast<float *>(base + wt);
    c.sums = reinterpret_cast<double *>(base + wt + part);
    c.bytes = 256 + wt + part + align256(sizeof(double) * (size_t)(kPnMaxBlocks / kPnChunk) * ((size_t)H2 * H1 + H2));
    return c;
}

inline size_t fwd_lds_bytes(int H1, int H2)
{
    return sizeof(float) * ((size_t)H2 * pn_stride(H1) + H2 + (size_t)kPnWaves * kPnTile * pn_stride(H1));
}

inline size_t bwd_lds_bytes(int H1, int H2)
{
    return sizeof(float) * ((size_t)pn_pad16(H1) * (H2 + 4) + (size_t)kPnWaves * kPnTile * (pn_stride(H1) + H2 + 4));
}

template <typename K>
int grant_lds(K kernel, size_t bytes, const char *what)
{
    if (bytes <= 64 * 1024) return 0;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)bytes);
    return e == hipSuccess ? 0 : hip_fail(e, what);
}

int entry_blocks(int64_t rows)
{
    const int64_t b = (rows + kPnWaves - 1) / kPnWaves;
    return (int)(b < kPnMaxBlocks ? b : kPnMaxBlocks);
}

// the smallest of 1, 2, 4, 8 blocks of 16 that hold H1
int ncb1_of(int H1) { return H1 <= 16 ? 1 : H1 <= 32 ? 2 : H1 <= 64 ? 4 : 8; }

struct PnShape {
    int64_t Nt, Ns, E;
    int width, F, D, H1, H2, act, act2, self_loop;
    bool list;
};

int check_shape(const char *who, const PnShape &s)
{
    DMET_REQUIRE(s.Nt >= 0 && s.Ns >= 0 && s.Nt < (int64_t)2147483647 / 128 && s.Ns < (int64_t)2147483647 / 128,
                 "%s: Nt=%lld, Ns=%lld out of range", who, (long long)s.Nt, (long long)s.Ns);
    DMET_REQUIRE(supported(s.F, s.D, s.H1, s.H2),
                 "%s: unsupported widths F=%d D=%d H1=%d H2=%d (0 <= F <= %d, 1 <= D <= %d, 1 <= H1 <= %d, H2 in {16, 32, 64, "
                 "128})", who, s.F, s.D, s.H1, s.H2, kPnMaxF, kPnMaxD, kPnMaxH1);
    DMET_REQUIRE((s.act == 0 || s.act == 1) && (s.act2 == 0 || s.act2 == 1), "%s: act must be 0 (ReLU) or 1 (ELU), act2 0 or 1",
                 who);
    DMET_REQUIRE(s.self_loop == 0 || s.self_loop == 1, "%s: self_loop must be 0 or 1", who);
    DMET_REQUIRE(!s.self_loop || s.Ns == s.Nt, "%s: self_loop needs one node set, got Ns=%lld, Nt=%lld", who, (long long)s.Ns,
                 (long long)s.Nt);
    if (s.list)
        DMET_REQUIRE(s.E >= 0 && s.E < (int64_t)2147483647, "%s: E=%lld out of range", who, (long long)s.E);
    else
        DMET_REQUIRE(s.width >= 1 && s.width <= DMET_POINTNET_MAX_WIDTH && s.Nt * (int64_t)s.width < (int64_t)2147483647,
                     "%s: width=%d not in [1,%d] or Nt*width out of range (table form: rowptr NULL)", who, s.width,
                     DMET_POINTNET_MAX_WIDTH);
    return 0;
}

PnGraph make_graph(const PnShape &s, const int32_t *idx, const int32_t *rowptr, const int32_t *tgt, const int32_t *cnt,
                   const int32_t *rev_ptr, const int32_t *rev_pos)
{
    PnGraph g{};
    g.idx = idx; g.rowptr = rowptr; g.tgt = tgt; g.cnt = s.list ? nullptr : cnt; g.rev_ptr = rev_ptr; g.rev_pos = rev_pos;
    g.Nt = s.Nt; g.Ns = s.Ns; g.M = s.list ? s.E : s.Nt * (int64_t)s.width; g.width = s.list ? 1 : s.width;
    g.self_loop = s.self_loop;
    return g;
}

int zero_async(float *p, int64_t n, hipStream_t st, const char *what)
{
    if (p == nullptr || n <= 0) return 0;
    const hipError_t e = hipMemsetAsync(p, 0, (size_t)n * sizeof(float), st);
    return e == hipSuccess ? 0 : hip_fail(e, what);
}

}  // namespace
}  // namespace dmet

using namespace dmet;

extern "C" int dmet_pointnet_supported(int F, int D, int H1, int H2) { return supported(F, D, H1, H2) ? 1 : 0; }

extern "C" size_t dmet_pointnet_workspace_bytes(int F, int D, int H1, int H2)
{
    if (!supported(F, D, H1, H2)) return 0;
    return carve(F, D, H1, H2, nullptr).bytes;
}

extern "C" int dmet_pointnet_fwd_f32(const float *x_src, const float *pos_src, const float *pos_dst, const int32_t *idx,
                                     const int32_t *rowptr, const int32_t *cnt, int64_t Nt, int64_t Ns, int64_t E, int width,
                                     int F, int D, const float *W1, const float *b1, int H1, const float *W2, const float *b2,
                                     int H2, int act, int act2, int self_loop, float *a, float *b, float *s, float *out,
                                     int32_t *win, void *ws, size_t ws_bytes, dmet_stream_t stream)
{
    const char *fn = "dmet_pointnet_fwd_f32";
    const PnShape sh{Nt, Ns, E, width, F, D, H1, H2, act, act2, self_loop, rowptr != nullptr};
    if (int rc = check_shape(fn, sh)) return rc;
    if (Nt == 0) return 0;
    DMET_REQUIRE(pos_dst && W1 && W2 && b && out && win, "%s: null pointer", fn);
    DMET_REQUIRE(idx || (sh.list && E == 0), "%s: null nbr / src", fn);
    DMET_REQUIRE(Ns == 0 || (pos_src && a && (F == 0 || x_src)), "%s: null source-side pointer with Ns=%lld", fn, (long long)Ns);
    DMET_REQUIRE(!self_loop || s, "%s: self_loop needs the s buffer", fn);
    DMET_REQUIRE(ws && ws_bytes >= carve(F, D, H1, H2, nullptr).bytes, "%s: workspace too small", fn);
    hipStream_t st = as_stream(stream);
    const PnWorkspace c = carve(F, D, H1, H2, ws);
    const int K = F + D;
    hipLaunchKernelGGL(pn_transpose_kernel, dim3((K * H1 + 255) / 256), dim3(256), 0, st, W1, K, H1, c.wt);
    DMET_LAUNCH_CHECK("pn_transpose_kernel");
    const int one_set = (Ns == Nt && pos_src == pos_dst) ? 1 : 0;
    const int nbs = (int)((Ns + kPnRows - 1) / kPnRows), nbt = one_set ? 0 : (int)((Nt + kPnRows - 1) / kPnRows);
    hipLaunchKernelGGL(pn_node_fwd_kernel, dim3(nbs + nbt), dim3(128), 0, st, x_src, F, pos_src, pos_dst, D, Ns, Nt, one_set, nbs,
                       (const float *)c.wt, b1, H1, a, b, self_loop ? s : (float *)nullptr);
    DMET_LAUNCH_CHECK("pn_node_fwd_kernel");
    const PnGraph g = make_graph(sh, idx, rowptr, nullptr, cnt, nullptr, nullptr);
    const size_t lds = fwd_lds_bytes(H1, H2);
    int rc = 0;
    with_int<16, 32, 64, 128>(H2, [&](auto h2) {
        constexpr int kH2 = decltype(h2)::value;
        rc = grant_lds(pn_fwd_kernel<kH2>, lds, "hipFuncSetAttribute(pn_fwd_kernel)");
        if (rc == 0)
            hipLaunchKernelGGL((pn_fwd_kernel<kH2>), dim3(entry_blocks(Nt)), dim3(kPnBlock), lds, st, (const float *)a,
                               (const float *)b, (const float *)s, g, H1, W2, b2, act, act2, out, win);
    });
    if (rc) return rc;
    DMET_LAUNCH_CHECK("pn_fwd_kernel");
    return 0;
}

extern "C" int dmet_pointnet_bwd_f32(const float *a, const float *b, const float *s, const float *out, const int32_t *win,
                                     const float *g_out, const int32_t *idx, const int32_t *rowptr, const int32_t *tgt,
                                     const int32_t *cnt, const int32_t *rev_ptr, const int32_t *rev_pos, int64_t Nt, int64_t Ns,
                                     int64_t E, int width, int F, int D, const float *W1, int H1, const float *W2, int H2,
                                     int act, int act2, int self_loop, float *g_a, float *g_b, float *g_s, float *g_x,
                                     float *g_pos_src, float *g_pos_dst, float *g_W2, float *g_b2, void *ws, size_t ws_bytes,
                                     dmet_stream_t stream)
{
    const char *fn = "dmet_pointnet_bwd_f32";
    const PnShape sh{Nt, Ns, E, width, F, D, H1, H2, act, act2, self_loop, rowptr != nullptr};
    if (int rc = check_shape(fn, sh)) return rc;
    DMET_REQUIRE(Ns == 0 || g_a, "%s: null g_a with Ns=%lld", fn, (long long)Ns);
    DMET_REQUIRE(Nt == 0 || g_b, "%s: null g_b with Nt=%lld", fn, (long long)Nt);
    DMET_REQUIRE(!self_loop || Nt == 0 || g_s, "%s: self_loop needs the g_s buffer", fn);
    hipStream_t st = as_stream(stream);
    const bool none = sh.list && E == 0;
    if (Nt > 0) {
        DMET_REQUIRE(b && out && win && g_out && W1 && W2, "%s: null pointer", fn);
        DMET_REQUIRE(none || (idx && (!sh.list || tgt)), "%s: null graph pointer", fn);
        DMET_REQUIRE(Ns == 0 || (a && rev_ptr && (none || rev_pos)), "%s: null source-side pointer", fn);
        DMET_REQUIRE(!self_loop || s, "%s: self_loop needs the s buffer", fn);
        DMET_REQUIRE(ws && ws_bytes >= carve(F, D, H1, H2, nullptr).bytes, "%s: workspace too small", fn);
    }
    // the source-side gradients are zero-filled first: a source nobody lists, and every source when there is no target
    if (int rc = zero_async(g_a, Ns * H1, st, "dmet_pointnet_bwd_f32: memset")) return rc;
    if (int rc = zero_async(g_x, Ns * F, st, "dmet_pointnet_bwd_f32: memset")) return rc;
    if (int rc = zero_async(g_pos_src, Ns * D, st, "dmet_pointnet_bwd_f32: memset")) return rc;
    if (Nt == 0) {
        if (int rc = zero_async(g_W2, (int64_t)H2 * H1, st, "dmet_pointnet_bwd_f32: memset")) return rc;
        return zero_async(g_b2, H2, st, "dmet_pointnet_bwd_f32: memset");
    }
    const PnWorkspace c = carve(F, D, H1, H2, ws);
    const PnGraph g = make_graph(sh, idx, rowptr, tgt, cnt, rev_ptr, rev_pos);
    const size_t lds = bwd_lds_bytes(H1, H2);
    const int nblk = entry_blocks(Nt), nsrc = entry_blocks((Ns + kPnGroup - 1) / kPnGroup);
    int rc = 0;
    with_int<16, 32, 64, 128>(H2, [&](auto h2) {
        with_int<1, 2, 4, 8>(ncb1_of(H1), [&](auto nc) {
            constexpr int kH2 = decltype(h2)::value, kNc = decltype(nc)::value;
            rc = grant_lds(pn_bwd_target_kernel<kH2, kNc>, lds, "hipFuncSetAttribute(pn_bwd_target_kernel)");
            if (rc == 0) rc = grant_lds(pn_bwd_source_kernel<kH2, kNc>, lds, "hipFuncSetAttribute(pn_bwd_source_kernel)");
            if (rc) return;
            hipLaunchKernelGGL((pn_bwd_target_kernel<kH2, kNc>), dim3(nblk), dim3(kPnBlock), lds, st, a, b, s, g, H1, W2, act,
                               act2, out, win, g_out, g_b, g_s, c.partial);
            if (nsrc > 0)
                hipLaunchKernelGGL((pn_bwd_source_kernel<kH2, kNc>), dim3(nsrc), dim3(kPnBlock), lds, st, a, b, g, H1, W2, act,
                                   act2, out, win, g_out, g_a);
        });
    });
    if (rc) return rc;
    DMET_LAUNCH_CHECK("pn_bwd_target_kernel / pn_bwd_source_kernel");
    const int n = H2 * H1 + H2;
    const int nchunk = (nblk + kPnChunk - 1) / kPnChunk;
    hipLaunchKernelGGL(pn_sum_kernel<float>, dim3((n + 255) / 256, nchunk), dim3(256), 0, st, (const float *)c.partial, nblk, n,
                       c.sums, H2 * H1, (float *)nullptr, (float *)nullptr);
    hipLaunchKernelGGL(pn_sum_kernel<double>, dim3((n + 255) / 256, 1), dim3(256), 0, st, (const double *)c.sums, nchunk, n,
                       (double *)nullptr, H2 * H1, g_W2, g_b2);
    DMET_LAUNCH_CHECK("pn_sum_kernel");
    const int K = F + D;
    if (g_x && F > 0 && Ns > 0) {
        hipLaunchKernelGGL(pn_node_bwd_kernel, dim3((unsigned)((Ns + kPnRows - 1) / kPnRows)), dim3(128), 0, st, (const float *)g_a,
                           self_loop ? (const float *)g_s : (const float *)nullptr, Ns, H1, W1, K, 0, F, g_x);
        DMET_LAUNCH_CHECK("pn_node_bwd_kernel (g_x)");
    }
    if (g_pos_src && Ns > 0) {
        hipLaunchKernelGGL(pn_node_bwd_kernel, dim3((unsigned)((Ns + kPnRows - 1) / kPnRows)), dim3(128), 0, st, (const float *)g_a,
                           (const float *)nullptr, Ns, H1, W1, K, F, D, g_pos_src);
        DMET_LAUNCH_CHECK("pn_node_bwd_kernel (g_pos_src)");
    }
    if (g_pos_dst) {
        hipLaunchKernelGGL(pn_node_bwd_kernel, dim3((unsigned)((Nt + kPnRows - 1) / kPnRows)), dim3(128), 0, st, (const float *)g_b,
                           (const float *)nullptr, Nt, H1, W1, K, F, D, g_pos_dst);
        DMET_LAUNCH_CHECK("pn_node_bwd_kernel (g_pos_dst)");
    }
    return 0;
}

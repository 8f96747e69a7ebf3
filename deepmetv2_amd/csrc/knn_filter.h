// knn_filter.h -- the matrix-core filter of the kNN build and its exact re-rank (D = 32 or 64, k <= 20).
// Part of knn.hip, which includes it inside namespace dmet::{anonymous} after the exact kernel the filter falls back to:
// it uses that file's plan, KnnArgs and distance steps.
// ---- matrix-core filter + exact re-rank (D = 32) ---------------------------------------------------------------
// The difference form of R1 cannot run on the matrix cores, but it does not have to run for every pair.  With
//   key(i,j) = |x_j|^2 - 2 x_i.x_j   ( = d(i,j) - |x_i|^2 in exact arithmetic )
// a matrix-core sweep ranks the candidates of every query approximately.  Each fp32 feature is split into two bf16
// terms x = h + m + r (h = bf16(x), m = bf16(x - h), |r| <= 2^-18 |x|) and x_i.x_j is taken as h.h' + h.m' + m.h' with
// v_mfma_f32_32x32x16_bf16 (exact bf16 products, fp32 accumulation): 6 MFMAs of 8 passes per 32x32 block instead of
// 16 fp32 MFMAs of 16 passes (measured on MI355X, tools/mfma_valu_micro.hip: MFMA passes and VALU instructions of a
// SIMD do NOT overlap, not even across wavefronts, so matrix-pipe time adds to the selection's VALU time).
// Error budget for a pair (a = |x_i|, b = |x_j|): dropped split terms 6.2 * 2^-18 a b, MFMA fp32 accumulation
// (<= 100 roundings) 3.3 * 2^-18 a b + 6e-6 b^2, squared norms 1.9e-6 (a^2 + b^2), the R1 chain itself 2.1e-6 (a + b)^2:
//   |d_chain(i,j) - (key(i,j) + |x_i|^2)|  <=  E(a, b) = 4e-5 a b + 1e-5 b^2 + 4e-6 a^2.
// Certification only has to rule out dropped candidates that could beat the k-th kept distance d_k: such a candidate
// has b <= R_i = a + sqrt(d_k) (otherwise d >= (b - a)^2 > d_k already), so the slack is e_i = 2 E(a, R_i) (2x margin)
// and depends on the query alone -- an outlier with a huge norm elsewhere in the event does not loosen it.
// R1/R2 stay the definition of the RESULT: every returned (d, j) comes from the exact fmaf chain and the (d, j) order;
// the expansion above only decides which pairs the exact chain is run for, under the proven bound.
//   1. knn_filter_kernel, sweep: every query (one lane) keeps the M = k + 4 smallest keys of its candidate range and
//      the candidates themselves (ties at the threshold included) in LDS.
//   2. exact re-rank: the R1 chain for the kept candidates, top-k by (d, j) (R2) -- in the tail of the filter kernel
//      for whole-sweep items, in knn_rerank_kernel for the tail tiles whose candidate range was split over two
//      work items.  It is THE exact answer iff nothing that could belong to the top k was dropped: a dropped
//      candidate has key >= the list's threshold tau, hence d >= tau + |x_i|^2 - e_i; if that exceeds the k-th
//      smallest exact distance among the kept candidates (for every partial list that saw at least M keys), the kept
//      top-k is the global top-k.
//   3. Queries that fail the test (exact ties beyond the list length, duplicates, lattices, events of more than
//      65535 nodes) are recomputed exactly: one workgroup per query when a 128-query tile has few of them, the exact
//      tile kernel above otherwise.
// Result: bit-identical output at a fraction of the VALU work.
constexpr int kFQ = 64;             // queries per filter work item: two 32-column MFMA blocks
// (4 sub-sweeps per tail tile were built and measured for the second form: every sub-sweep re-ranks its own ~27
// candidates and the 4-way merge took 60 us instead of 17: filter 452 -> 509 us, build 0.55 -> 0.65 ms.  Not kept.)

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

struct KnnFilterArgs {
    const float *x;
    const int64_t *ptr;
    int B;
    int64_t N;
    int k;
    float *nrm;                 // [N] squared norms
    uint8_t *rec;               // candidate tile records (kRecBytes each): the bf16 split of 32 rows in MFMA operand
                                // order + their squared norms; event b starts at record (ptr[b] >> 5) + b
    const KnnPlan *plan;        // filter plan (kFQ-query tiles)
    const int32_t *order;
    const int32_t *pos_of;
    const int32_t *tile_ptr;
    float *psd;                 // split tiles: [(tile-n_full)*kFQ + slot][split][MS], MS = M kept (key, id) + threshold slot
    int32_t *psj;
    int32_t *nbr;
    float *dist;
    uint16_t *nbr16;            // optional event-local copy of nbr (see KnnArgs)
    int32_t *flags;             // [exact tiles] number of uncertified queries of the tile
    int32_t *any;               // total number of uncertified queries: the fallback kernels exit at once while it is 0
    uint8_t *qflag;             // [N] 1 = uncertified query
    int32_t *qlist;             // [N] the uncertified queries in the order they were flagged (any = their number)
    const int32_t *xtile_ptr;   // tile prefix of the exact kernel's plan (same event order)
    int xtile_queries;
    int form2;                  // 1: events of kF2MinNodes..kF2MaxNodes nodes are swept by the second form
    float slack_scale;          // certificate slack relative to the 32-feature bound (1.5 at 64 features)
    // rider (dmet_knn_local_dense_f32): workgroups first_rider .. gridDim.x - 1 of the filter launch compute the
    // node-level dense layer of the EdgeConv that consumes this graph (nls_body.h; 32 -> 32 features), rP == nullptr: none
    const float *rW, *rb;
    float *rP, *rQ;
    int r_sliced;               // layout: 0 row-major fp32, 1 slice-major fp32, 2 row-major with Q as bf16 bits
    int first_rider;
    int emit_coalesced;         // 1: nbr / dist / nbr16 are 16-byte aligned: whole-sweep items write their rows as 16-byte pieces
    int no_rerank;              // 1: knn_rerank_kernel is not launched (dmet_knn_size_hint: no first-form event); a first-form
                                // tail item that shows up anyway hands its queries to the exact kernel
    float cut_scale;            // second form, final threshold min(tk[M-1], tk[k-1] + cut_scale x (what certifies the bound
                                // d_k <= tk[k-1] + |x|^2 + slack)): see f2_cut; < 0: no cut (DMET_KNN_CUT, knn_cut_scale)
    int32_t *retries;           // [2] second attempts of the second form: wavefronts that swept again, queries they carried
    int run_cut;                // second form: 1: the main sweep records its masks against the running cut (f2_tile, F2Lane::
                                // margin); 0: against tk[M-1] alone, the cut comes after the sweep only (DMET_KNN_RUNCUT=0)
};

// The dense layer a build may carry (dmet_knn_local_dense_f32); P == nullptr: none.
struct KnnRider {
    const float *W = nullptr, *b = nullptr;
    float *P = nullptr, *Q = nullptr;
    int sliced = 0;
};

// BatchNorm transform + residual fused into the prep launch (dmet_bn_knn_local_dense_f32): the build's input y is not
// there yet -- the prep kernel reads the rows it is made of, raw (the BatchNorm's input) and res, writes
//   y = (raw - mean) * (gamma * invstd) + beta + res      (bn_affine4 of bn_affine.h, as in bn_apply_kernel: same bits)
// and cuts its tile records from the values it just formed: one pass over the rows instead of two, one launch less.
// knn_prep_kernel takes the BnAffine and a never-read int kernarg_pad as its last arguments and the hidden kernel
// arguments follow them at the next multiple of 8: a change of this size moves them and with them the s_load offsets of
// every instance, so the device code would no longer be the verified one
static_assert(sizeof(BnAffine) == 48 && alignof(BnAffine) == 8,
              "BnAffine + the padded kernarg_pad are the 56-byte tail of knn_prep_kernel's argument block: keep its size");

// rider workgroups per launch (DMET_KNN_RIDER_GROUPS: experiments; 128..1024 measured within 1 % of each other at
// 64 x 4500 nodes: the last round leaves ~1150 of the 2048 wavefront slots empty)
inline int rider_groups()
{
    static int cached = 0;
    if (cached == 0) {
        const char *e = getenv("DMET_KNN_RIDER_GROUPS");
        const int v = e ? atoi(e) : 0;
        cached = (v >= 1 && v <= 4096) ? v : 512;
    }
    return cached;
}

// A query whose result is not certified: counted per exact-kernel tile (dense tiles go to the exact tile kernel) and
// appended to the list the per-query fallback walks.  Every query is flagged at most once per call.
__device__ __forceinline__ void flag_query(const KnnFilterArgs &a, int q, int xtile)
{
    a.qflag[q] = 1;
    atomicAdd(a.flags + xtile, 1);   // a count: order-independent
    const int slot = atomicAdd(a.any, 1);
    if (slot < a.N) a.qlist[slot] = q;
}

__device__ __forceinline__ unsigned bf16_rne_bits(float f)   // finite inputs
{
    const unsigned u = __float_as_uint(f);
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

// ---- candidate tile records ---------------------------------------------------------------------------------------
// The filter sweeps an event's candidates in tiles of 32 rows.  A tile's A operands are stored the way a wavefront
// consumes them: frag[m][lane] = the 8 bf16 values lane (col = lane & 31, hh = lane >> 5) feeds to MFMA operand m
// (m = 0,1: high terms of features 0-15 / 16-31; m = 2,3: middle terms), i.e. features 16 (m & 1) + 8 hh + 0..7 of row
// col -- so one load instruction of a wavefront is 1 KB of contiguous memory (8 full cache lines) instead of 32-byte
// pieces of 32 different rows -- followed by the 32 squared norms.  Rows past the end of an event are zero with
// norm = +inf (key = +inf: never admitted), so the sweep needs no range checks.  Event b owns the records
// [(ptr[b] >> 5) + b, ... + ceil(n_b / 32)): monotone and disjoint without a prefix sum over the events.
constexpr int kRecFragBytes = 4 * kWave * 16;           // 4096: the four operand fragments of 32 features
// NH = number of 32-feature halves per row (1: D = 32, 2: D = 64, the hidden width of the reference's DRN,
// model/dynamic_reduction_network.py:40,86): a record holds NH x 4 fragments, then the 32 squared norms
constexpr int rec_bytes(int NH) { return kRecFragBytes * NH + 32 * 4; }
constexpr int kRecBytes = rec_bytes(1);                 // 4224 (33 cache lines)
constexpr int kRecBytesMax = rec_bytes(2);              // the workspace is carved for either width

__device__ __forceinline__ int64_t rec_base_tile(const int64_t *__restrict__ ptr, int b) { return (ptr[b] >> 5) + b; }

// Second-form events (kF2MinNodes..kF2MaxNodes nodes, when the second form is enabled) get SINGLE-TERM fp16 records
// instead of the bf16 split: frag[m][lane], m = 0..2 NH - 1, = the 8 fp16 values (round to nearest even) of features
// 16 m + 8 hh + 0..7 of row col, then at byte kRec16FragBytes * NH one more fragment (1 KB) that carries the squared
// norms and the scales of the threshold (the record stride stays rec_bytes(NH)).  2 NH + 1 MFMAs per 32 x 32 block
// instead of six; the certificate of the second form carries the fp16 rounding (see f2_slack).  A row with a feature
// outside the range whose doubled value fits fp16 (|v| >= 16384, or not finite) is stored as zeros with the norm term
// -inf: its key is -inf for every query, so it is always a candidate of the exact re-rank and never dropped on the
// strength of an overflowed product (as a QUERY such a row is refused by the certificate through its true norm, kept
// in nrm[]).
constexpr int kRec16FragBytes = 2 * kWave * 16;         // 2048: the two fp16 operand fragments of 32 features
constexpr float kF16WideLimit = 16384.0f;
static_assert(kRec16FragBytes + kWave * 16 <= rec_bytes(1) && 2 * kRec16FragBytes + kWave * 16 <= rec_bytes(2),
              "the fold fragment fits the record");
// Fold of the squared norms and of the threshold into the matrix product (f2_block): the key block comes out as
// |x_j|^2 - 2 x_i.x_j - tau_rep(i).  Norm terms: N_i x kF2NormP[i], each scale chosen so that the residual of the term
// before (<= 2^-11 of it) fits fp16: N1 <= 65504 for s < kF2NormMax, N2..N4 <= 2^15.  Threshold terms: y x kF2TauC[i]
// with y the fp16 on the query side (f2_tau16).
constexpr float kF2NormP[4] = {0x1p15f, 0x1p5f, 0x1p-6f, 0x1p-17f};
constexpr float kF2NormInvP[4] = {0x1p-15f, 0x1p-5f, 0x1p6f, 0x1p17f};
constexpr float kF2NormMax = 65504.0f * 0x1p15f;
constexpr float kF2TauC[2] = {0x1p14f, 0x1p-15f};
constexpr float kF2TauRepMax = 65504.0f * 0x1p14f;   // the largest threshold the fold represents (f2_cert_T)

__device__ __forceinline__ bool f2_in_domain64(int64_t n) { return n >= kF2MinNodes && n <= kF2MaxNodes; }

// One wavefront per record: lane (col, hh) converts the 16 features of row col it will later feed to the MFMAs.
// Also writes the flat norm array (certificates) and clears the uncertified-query counters / flags (zero_bytes bytes
// at `zero`, 4-byte aligned) for the launches that follow, which saves a memset launch per call.
template <int NH, bool AFFINE = false>
__global__ __launch_bounds__(256) void knn_prep_kernel(const float *__restrict__ x, const int64_t *__restrict__ ptr,
                                                        int B, int64_t N, float *__restrict__ nrm,
                                                        uint8_t *__restrict__ rec, int64_t nrec,
                                                        uint32_t *__restrict__ zero, size_t zero_bytes, KnnPlanOut o0,
                                                        KnnPlanOut o1, int form2, BnAffine af, int /*kernarg_pad*/)
{
    static_assert(!AFFINE || NH == 1, "the fused BatchNorm transform is built for 32 features");
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    {
        const size_t words = zero_bytes >> 2, total = (size_t)gridDim.x * blockDim.x;
        for (size_t wd = (size_t)t; wd < words; wd += total) zero[wd] = 0u;
        if (t == 0)
            for (size_t bt = words << 2; bt < zero_bytes; ++bt) reinterpret_cast<uint8_t *>(zero)[bt] = 0;
    }
    // the last two workgroups compute the two launch plans (one launch less on the critical path of the build)
    if (blockIdx.x + 2 >= gridDim.x) {
        knn_plan_body(ptr, B, blockIdx.x + 2 == gridDim.x ? o0 : o1);
        return;
    }
    // wave-uniform, and said so: the search below then runs on the scalar unit (s_load through the constant cache)
    // instead of six dependent vector loads per wavefront
    const int64_t tile = (int64_t)blockIdx.x * (blockDim.x >> 6) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (tile >= nrec) return;
    const int lane = (int)(t & 63), col = lane & 31, hh = lane >> 5;
    // event that owns the record: the last b with (ptr[b] >> 5) + b <= tile.  A 64-ary search across the lanes (one
    // vector load + ballot per level: one memory round trip for B <= 64, two up to 4096) instead of a binary search of
    // log2(B) DEPENDENT scalar loads -- with every wavefront of the grid resident at once the kernel lasts as long as one
    // wavefront's chain of round trips (measured: 16.5 -> 16.0 us at 64 events; the chain was not what bounds the kernel)
    int lo = 0, hi = B;                      // invariant: base(lo) <= tile < base(hi) (base(B) = +inf)
    {
        const int ln = (int)(threadIdx.x & 63);
        while (hi - lo > 1) {
            const int span = hi - lo, step = (span + 63) >> 6;           // candidates lo + step * (ln + 1), ln = 0..63
            const int cand = lo + step * (ln + 1);
            const bool ok = cand < hi && rec_base_tile(ptr, cand) <= tile;
            const unsigned long long m = __ballot(ok);                   // monotone: a prefix of the lanes
            const int cnt = __popcll(m);                                 // wave-uniform
            const int nlo = lo + step * cnt;
            const int nhi = min(hi, lo + step * (cnt + 1));
            lo = __builtin_amdgcn_readfirstlane(nlo);
            hi = __builtin_amdgcn_readfirstlane(nhi);
        }
    }
    const int64_t ev_lo = ptr[lo], n = ptr[lo + 1] - ev_lo;
    const int64_t li0 = (tile - rec_base_tile(ptr, lo)) * 32;
    if (li0 >= n) return;                   // a slot between two events: never read
    const bool live = li0 + col < n;
    const int64_t r = ev_lo + (live ? li0 + col : 0);
    const bool rec16 = form2 != 0 && f2_in_domain64(n);    // wave-uniform: one event per record
    float s = 0.0f;
    uint8_t *recp = rec + tile * rec_bytes(NH);
    float f[NH][16];
    if constexpr (NH == 1) {
        // Coalesced tile loads (a wavefront instruction = 1 KB of consecutive bytes: lane l takes float4 64 j + l of the
        // 4 KB tile, i.e. feature group l & 7 of row 8 j + (l >> 3)), the optional BatchNorm transform applied right there
        // (one feature group per lane: its constants are loaded once) and y stored the same way; the values then change
        // to the record layout (lane (col, hh): features 16 kb + 8 hh .. + 7 of row col) through the wavefront's LDS tile.
        // Until the third session the rows were read as 32-byte pieces in the record layout: 4 instructions that each
        // touch all 32 cache lines of the tile.
        __shared__ __attribute__((aligned(16))) float prep_tile[4][32 * 36];
        float *T = prep_tile[threadIdx.x >> 6];
        const int fg = lane & 7;
        BnAffine4 c4;
        if constexpr (AFFINE) c4 = bn_affine_load4(af, fg);
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            const int rowj = 8 * jj + (lane >> 3);
            const bool livej = li0 + rowj < n;
            const int64_t rj = ev_lo + (livej ? li0 + rowj : 0);
            float4 v;
            if constexpr (AFFINE) {
                // x is the OUTPUT here: y = (raw - mean) * (gamma * invstd) + beta (+ res), written for the live rows
                v = bn_affine4(reinterpret_cast<const float4 *>(af.raw + rj * 32)[fg], c4.mu, c4.scale, c4.beta);
                if (af.res) v = bn_add4(v, reinterpret_cast<const float4 *>(af.res + rj * 32)[fg]);
                if (livej) reinterpret_cast<float4 *>(const_cast<float *>(x) + rj * 32)[fg] = v;
            } else {
                v = reinterpret_cast<const float4 *>(x + rj * 32)[fg];
            }
            *reinterpret_cast<float4 *>(&T[rowj * 36 + 4 * fg]) = v;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the wavefront's own LDS writes, in order
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            const float4 v0 = *reinterpret_cast<const float4 *>(&T[col * 36 + 16 * kb + 8 * hh]);
            const float4 v1 = *reinterpret_cast<const float4 *>(&T[col * 36 + 16 * kb + 8 * hh + 4]);
            f[0][8 * kb + 0] = v0.x; f[0][8 * kb + 1] = v0.y; f[0][8 * kb + 2] = v0.z; f[0][8 * kb + 3] = v0.w;
            f[0][8 * kb + 4] = v1.x; f[0][8 * kb + 5] = v1.y; f[0][8 * kb + 6] = v1.z; f[0][8 * kb + 7] = v1.w;
        }
    } else {
#pragma unroll
        for (int half = 0; half < NH; ++half) {
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) {
                const float4 *g = reinterpret_cast<const float4 *>(x + r * (32 * NH) + 32 * half + 16 * kb + 8 * hh);
                const float4 v0 = g[0], v1 = g[1];
                f[half][8 * kb + 0] = v0.x; f[half][8 * kb + 1] = v0.y; f[half][8 * kb + 2] = v0.z; f[half][8 * kb + 3] = v0.w;
                f[half][8 * kb + 4] = v1.x; f[half][8 * kb + 5] = v1.y; f[half][8 * kb + 6] = v1.z; f[half][8 * kb + 7] = v1.w;
            }
        }
    }
    bool wide = false;
#pragma unroll
    for (int half = 0; half < NH; ++half) {
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const float v = live ? f[half][u] : 0.0f;
            f[half][u] = v;
            s = __builtin_fmaf(v, v, s);
            wide = wide || !(__builtin_fabsf(v) < kF16WideLimit);
        }
    }
    s += __shfl_xor(s, 32, 64);             // the row's other features: fixed order, deterministic
    if (rec16) {
        wide = wide || (__shfl_xor(wide ? 1 : 0, 32, 64) != 0);
#pragma unroll
        for (int half = 0; half < NH; ++half) {
            uint4 *dst = reinterpret_cast<uint4 *>(recp + half * kRec16FragBytes);
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) {
                f16x8 hv;
#pragma unroll
                for (int u = 0; u < 8; ++u) hv[u] = wide ? (_Float16)0.0f : (_Float16)f[half][8 * kb + u];   // v_cvt_f16_f32: RNE
                dst[kb * 64 + lane] = __builtin_bit_cast(uint4, hv);
            }
        }
        // the fold fragment (see f2_block): lane (col, 0) = {0, 0, 0, 0, N1, N2, N3, N4}, the squared norm as four fp16
        // terms on the fixed scales kF2NormP (N1 = +inf for rows past the event's end, -inf for forced rows); lane
        // (col, 1) = {2^14, 2^-15, 0, ...}, the scales of the two threshold terms.  Each residual is exact (the
        // subtracted term is the rounded residual itself or a multiple of its ulp), so |s - sum N_i P_i| is the last
        // rounding alone: <= 2^-44 s + 2^-40 (f2_slack).  A norm at or beyond 65504 x 2^15 makes the row a forced
        // candidate (as a query it is refused by the certificate already: nx >= 2^28).
        // 64 features (NH = 2) keep the 32 fp32 squared norms there instead: the accumulator seed of f2_block.
        if constexpr (NH != 1) {
            if (hh == 0) {
                reinterpret_cast<float *>(recp + kRec16FragBytes * NH)[col] =
                    !live ? __builtin_inff() : (wide ? -__builtin_inff() : s);
                if (live) nrm[r] = s;
            }
            return;
        }
        f16x8 fv = {};
        if (hh == 0) {
            const float sn = !live ? __builtin_inff() : ((wide || !(s < kF2NormMax)) ? -__builtin_inff() : s);
            if (sn == sn && __builtin_fabsf(sn) < __builtin_inff()) {
                float rr = sn;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const _Float16 h = (_Float16)(rr * kF2NormInvP[i]);   // v_cvt_f16_f32: RNE
                    fv[4 + i] = h;
                    rr -= (float)h * kF2NormP[i];
                }
            } else {
                fv[4] = (_Float16)sn;
            }
            if (live) nrm[r] = s;
        } else {
            fv[0] = (_Float16)kF2TauC[0];
            fv[1] = (_Float16)kF2TauC[1];
        }
        reinterpret_cast<uint4 *>(recp + kRec16FragBytes * NH)[lane] = __builtin_bit_cast(uint4, fv);
        return;
    }
#pragma unroll
    for (int half = 0; half < NH; ++half) {
        unsigned h[16], m[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const float v = f[half][u];
            h[u] = bf16_rne_bits(v);
            m[u] = bf16_rne_bits(v - __uint_as_float(h[u] << 16));   // the subtraction is exact
        }
        uint4 *dst = reinterpret_cast<uint4 *>(recp + half * kRecFragBytes);
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            dst[kb * 64 + lane] = make_uint4(h[8 * kb] | (h[8 * kb + 1] << 16), h[8 * kb + 2] | (h[8 * kb + 3] << 16),
                                             h[8 * kb + 4] | (h[8 * kb + 5] << 16), h[8 * kb + 6] | (h[8 * kb + 7] << 16));
            dst[(2 + kb) * 64 + lane] = make_uint4(m[8 * kb] | (m[8 * kb + 1] << 16), m[8 * kb + 2] | (m[8 * kb + 3] << 16),
                                                   m[8 * kb + 4] | (m[8 * kb + 5] << 16), m[8 * kb + 6] | (m[8 * kb + 7] << 16));
        }
    }
    if (!live) s = __builtin_inff();
    if (hh == 0) {
        reinterpret_cast<float *>(recp + kRecFragBytes * NH)[col] = s;
        if (live) nrm[r] = s;
    }
}

// One 32(candidates) x 32(queries) block: acc = cinit + sum over both 16-feature k-blocks of  h.h' + h.m' + m.h'.
// Operand map of v_mfma_f32_32x32x16_bf16: lane (r = lane & 31, hh = lane >> 5) holds A[row r][k = 8 hh + 0..7].
// av / bv = {high k-block 0, high k-block 1, middle k-block 0, middle k-block 1}.
template <int NH = 1>
__device__ __forceinline__ f32x16 filter_block(const bf16x8 (&av)[4 * NH], const bf16x8 (&bv)[4 * NH], const f32x16 &cinit)
{
    f32x16 acc = cinit;
#pragma unroll
    for (int h = 0; h < NH; ++h) {
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av[4 * h + 0], bv[4 * h + 0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av[4 * h + 1], bv[4 * h + 1], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av[4 * h + 0], bv[4 * h + 2], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av[4 * h + 1], bv[4 * h + 3], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av[4 * h + 2], bv[4 * h + 0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av[4 * h + 3], bv[4 * h + 1], acc, 0, 0, 0);
    }
    return acc;
}

// one candidate tile record: the lane's 4 NH A operands and the squared norms of the 16 candidate rows it receives
// results for (accumulator seed; rows (e & 3) + 8 (e >> 2) + 4 hh)
template <int NH = 1>
__device__ __forceinline__ void filter_load(bf16x8 (&av)[4 * NH], f32x16 &cinit, const uint8_t *__restrict__ rec,
                                            int64_t tidx, int lane, int hh)
{
    const uint8_t *base = rec + tidx * rec_bytes(NH);
    const bf16x8 *g = reinterpret_cast<const bf16x8 *>(base);
#pragma unroll
    for (int m = 0; m < 4 * NH; ++m) av[m] = g[m * 64 + lane];
    const float4 *nr = reinterpret_cast<const float4 *>(base + kRecFragBytes * NH);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float4 v = nr[2 * q + hh];
        cinit[4 * q] = v.x; cinit[4 * q + 1] = v.y; cinit[4 * q + 2] = v.z; cinit[4 * q + 3] = v.w;
    }
}

// ---- selection state of one query (= one lane) ----------------------------------------------------------------
// After v_permlane32_swap of the two accumulators lane (c, hh) holds all 32 keys of query (block hh, column c), so
// a lane owns ONE query.  Per lane:
//   * tk[M]: the M smallest keys so far, sorted, in registers; inserting is a v_med3_f32 chain (one op per slot,
//     no payload to move);  tau = tk[M-1] is the admission threshold;
//   * an LDS queue of (key, j) pairs that doubles as the store of the kept candidates: admitted keys are appended;
//     when a lane runs out of room the wave drains: new entries update tk, then every lane compacts its queue in
//     place to the entries with key <= tau (at most M survive, ties aside).  No global-memory traffic until the end.
// A lane whose queue cannot be compacted below the refill mark (more than M candidates tied at tau) gives up
// (tau = -inf) and marks its list as overflowed: the re-rank flags such queries for the exact path.
template <int M>
struct FilterLane {
    float tk[M];
    float tau;
    int cnt;       // entries in the queue
    int kept;      // entries that survived the last compaction (already in tk)
    bool overflow;
};

constexpr int filter_list_len(int KP) { return KP + 4; }   // M = kept keys per list: result capacity KP (>= k) + 4
constexpr int filter_queue_len(int M) { return M + 28; }

// LDS queue of one wavefront: keys and 16-bit event-relative candidate ids in separate arrays (6 bytes per entry:
// QF = M + 28 slots per lane fit two wavefronts per SIMD).  Events of more than 65535 nodes do not fit the id and
// are handed to the exact kernel (every lane reports overflow).
template <int QF>
struct FilterQueue {
    unsigned key[QF][kWave];
    unsigned short id[QF][kWave];
};

template <int M>
__device__ __forceinline__ void filter_drain(FilterLane<M> &L, FilterQueue<filter_queue_len(M)> &Q, int lane)
{
    constexpr int QF = filter_queue_len(M);
    // 1. new entries -> sorted keys
    int maxnew = L.cnt - L.kept;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) maxnew = max(maxnew, __shfl_xor(maxnew, off, 64));
    for (int s = 0; s < maxnew; ++s) {
        const int idx = L.kept + s;
        if (idx < L.cnt) {
            const float key = __uint_as_float(Q.key[idx][lane]);
            if (key < L.tk[M - 1]) {
#pragma unroll
                for (int p = M - 1; p >= 1; --p) L.tk[p] = __builtin_amdgcn_fmed3f(L.tk[p - 1], key, L.tk[p]);
                L.tk[0] = fminf(L.tk[0], key);
            }
        }
    }
    const float tau = L.tk[M - 1];
    // 2. in-place compaction of every lane's queue to key <= tau
    int maxcnt = L.cnt;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) maxcnt = max(maxcnt, __shfl_xor(maxcnt, off, 64));
    int out = 0;
    for (int s = 0; s < maxcnt; ++s) {
        if (s < L.cnt) {
            const unsigned kb = Q.key[s][lane];
            const unsigned short id = Q.id[s][lane];
            if (__uint_as_float(kb) <= tau) { Q.key[out][lane] = kb; Q.id[out][lane] = id; ++out; }
        }
    }
    L.cnt = out;
    L.kept = out;
    if (out > QF - 8) {          // cannot make room: too many candidates tied at tau
        L.overflow = true;
        L.cnt = 0; L.kept = 0;
        L.tau = -__builtin_inff();
    } else if (!L.overflow) {
        L.tau = tau;
    }
}

// 16 keys of one accumulator.  The push is branch-free (a compare, a carry add, the slot address and the id: four VALU
// ops per key; per-key branches cost more in scalar work and pipeline bubbles than they skip): the slot is always
// written and only kept when the key is admitted.
template <int M>
__device__ __forceinline__ void filter_select(FilterLane<M> &L, const f32x16 &acc, int jrel,
                                              FilterQueue<filter_queue_len(M)> &Q, int lane)
{
    constexpr int QF = filter_queue_len(M);
#if defined(DMET_FILTER_ABL) && (DMET_FILTER_ABL == 1 || DMET_FILTER_ABL == 2)
    // cycle-budget experiment (tools/knn_budget.sh): keys computed (and swapped), never looked at
#pragma unroll
    for (int e = 0; e < 16; ++e) asm volatile("" ::"v"(acc[e]));
    return;
#endif
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        if (__any(L.cnt > QF - 8)) filter_drain<M>(L, Q, lane);
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int e = half * 8 + u;
            const float key = acc[e];
#if defined(DMET_FILTER_ABL) && DMET_FILTER_ABL == 3
            // experiment: the push's VALU work (compare, count, two slot addresses, id) without the LDS stores
            const unsigned ak = (unsigned)L.cnt * (kWave * 4u) + (unsigned)lane * 4u;
            const unsigned ai = (unsigned)L.cnt * (kWave * 2u) + (unsigned)lane * 2u;
            const unsigned idv = (unsigned)(jrel + (e & 3) + 8 * (e >> 2));
            asm volatile("" ::"v"(ak), "v"(ai), "v"(idv), "v"(key));
#else
            Q.key[L.cnt][lane] = __float_as_uint(key);
            Q.id[L.cnt][lane] = (unsigned short)(jrel + (e & 3) + 8 * (e >> 2));
#endif
            L.cnt += (key < L.tau) ? 1 : 0;
        }
#if defined(DMET_FILTER_ABL) && (DMET_FILTER_ABL == 3 || DMET_FILTER_ABL == 4)
        asm volatile("v_mov_b32 %0, 0" : "=v"(L.cnt) : "v"(L.cnt));   // experiment: queue never fills, no drains
#endif
    }
}


// events of the second form (filter2_wave below): kF2MinNodes .. kF2MaxNodes nodes (constants with the plan)
__device__ __forceinline__ bool f2_in_domain(int n) { return n >= kF2MinNodes && n <= kF2MaxNodes; }

// One wavefront's item of the first form (work item `group * kWavesPerGroup + wv` of the plan); Q is the wavefront's
// own LDS.  No workgroup barrier inside: wavefronts of one workgroup may run different forms (knn_filter12_kernel).
template <int KP>
__device__ __forceinline__ void filter1_wave(const KnnFilterArgs &a, FilterQueue<filter_queue_len(filter_list_len(KP))> &Q,
                                             int group, int wv, int lane)
{
    constexpr int M = filter_list_len(KP);
    constexpr int QF = filter_queue_len(M);
    constexpr int MS = (M + 1 + 3) & ~3;   // list stride in the workspace: M entries, then tau (d array) / overflow (j array)
    const int col = lane & 31, hh = lane >> 5;
    const int item = group * kWavesPerGroup + wv;
    const uint8_t *__restrict__ rec = a.rec;
    const int64_t *__restrict__ ptr = a.ptr;

    if (a.form2 && a.plan->form1_events == 0) return;      // every event is swept by the second form
    const int n_full = a.plan->n_full, split = a.plan->split, total = a.plan->total_tiles;
    int tile = item, sub = 0, nsub = 1;
    if (item >= n_full) {
        const int r = item - n_full;
        tile = n_full + r / split;
        sub = r % split;
        nsub = split;
    }
    if (tile >= total) return;
    const int pos = find_tile_event(a.tile_ptr, a.B, tile);
    const int ev = a.order[pos];
    const int ev_lo = (int)ptr[ev], ev_hi = (int)ptr[ev + 1];
    if (a.form2 && f2_in_domain(ev_hi - ev_lo)) return;   // swept by the second form
    const int q_first = ev_lo + (tile - a.tile_ptr[pos]) * kFQ;
    int clo = ev_lo, chi = ev_hi;
    if (nsub > 1) {
        const int chunk = (((chi - clo) + nsub - 1) / nsub + 31) & ~31;
        clo = min(chi, clo + sub * chunk);
        chi = min(chi, clo + chunk);
    }
    const bool fits = (ev_hi - ev_lo) <= 65535;   // 16-bit candidate ids

    // record of the event's first 32 candidates; the (32-aligned, event-relative) tile at c0 is rbase + (c0 - ev_lo) / 32
    const int64_t rbase = (ptr[ev] >> 5) + ev;
    const int64_t rlast = rbase + (ev_hi - ev_lo - 1) / 32;
    // B operands of both 32-query blocks: -2 * the query's bf16 terms (exact: sign flip and exponent + 1); the query
    // tiles are records too (a block past the end of the event reads the event's last record: idle lanes)
    bf16x8 bq[2][4];
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const int64_t qrec = min(rbase + (q_first - ev_lo) / 32 + b, rlast);
        const bf16x8 *g = reinterpret_cast<const bf16x8 *>(rec + qrec * kRecBytes);
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const bf16x8 v = g[m * 64 + lane];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const float f = -2.0f * __uint_as_float(((unsigned)(unsigned short)v[u]) << 16);
                bq[b][m][u] = (short)(__float_as_uint(f) >> 16);
            }
        }
    }
    // the query this lane selects for (after the half-wave swap): block hh, column col
    const int myq = q_first + hh * 32 + col;
    const bool valid = myq < ev_hi;
    FilterLane<M> L;
#pragma unroll
    for (int p = 0; p < M; ++p) L.tk[p] = kKnnSentinel;
    L.tau = (valid && fits) ? kKnnSentinel : -__builtin_inff();
    L.cnt = 0; L.kept = 0;
    L.overflow = !(valid && fits);   // idle lanes never admit; oversized events are left to the exact kernel

    if (clo < chi && fits) {
        bf16x8 av[4], an[4];
        f32x16 ci, cn;
        int64_t tidx = rbase + (clo - ev_lo) / 32;
        filter_load(av, ci, rec, tidx, lane, hh);
        for (int c0 = clo; c0 < chi; c0 += 32) {
            const bool more = c0 + 32 < chi;
            if (more) filter_load(an, cn, rec, ++tidx, lane, hh);
            f32x16 acc0 = filter_block(av, bq[0], ci);
            f32x16 acc1 = filter_block(av, bq[1], ci);
            // lanes 32..63 of block 0 <-> lanes 0..31 of block 1: afterwards acc0 = rows {0-3, 8-11, ..} and
            // acc1 = rows {4-7, 12-15, ..} of THIS lane's query
#if !(defined(DMET_FILTER_ABL) && DMET_FILTER_ABL == 2)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(acc0[e]), __float_as_uint(acc1[e]),
                                                                false, false);
                acc0[e] = __uint_as_float(r[0]);
                acc1[e] = __uint_as_float(r[1]);
            }
#endif
            filter_select<M>(L, acc0, c0 - ev_lo, Q, lane);
            filter_select<M>(L, acc1, c0 - ev_lo + 4, Q, lane);
            if (more) {
#pragma unroll
                for (int m = 0; m < 4; ++m) av[m] = an[m];
                ci = cn;
            }
        }
    }
    filter_drain<M>(L, Q, lane);
#if defined(DMET_FILTER_ABL) && DMET_FILTER_ABL == 5
    return;   // experiment: selection only, no exact re-rank / certificate
#endif
    if (nsub == 1) {
        // ---- whole-sweep items: exact re-rank right here, while the kept candidates still sit in LDS ----------------
        // Every lane owns one query and <= QF-8 kept candidates (all keys <= tau, ties included, so every dropped
        // candidate has key >= tau).  Round c handles candidate c of all 64 queries: the rows are fetched cooperatively
        // (8 lanes x 16 bytes per row: 8 cache lines per load instruction instead of 64) into the LDS space of the
        // keys (no longer needed), each lane runs the exact R1 chain on its row and inserts (d, j) into its sorted top-k.
        const int64_t qrow_id = valid ? myq : ev_lo;
        float qrow[32];
        {
            const float4 *g = reinterpret_cast<const float4 *>(a.x + qrow_id * 32);
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const float4 v = g[c];
                qrow[4 * c] = v.x; qrow[4 * c + 1] = v.y; qrow[4 * c + 2] = v.z; qrow[4 * c + 3] = v.w;
            }
        }
        float kd[KP];
        int32_t kj[KP];
#pragma unroll
        for (int p = 0; p < KP; ++p) { kd[p] = kKnnSentinel; kj[p] = -1; }
        constexpr int kRowPad = 36;
        static_assert(kWave * kRowPad <= QF * kWave, "row staging must fit the key array");
        float (*rows)[kRowPad] = reinterpret_cast<float (*)[kRowPad]>(&Q.key[0][0]);
        const int mycnt = valid ? L.cnt : 0;
        int maxcnt = mycnt;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) maxcnt = max(maxcnt, __shfl_xor(maxcnt, off, 64));
        // the loop is latency bound (load -> LDS -> chain per round): rows are fetched two rounds ahead into registers
        auto fetch = [&](int c, float4 (&pv)[8], int32_t &jout) {
            jout = (c < mycnt) ? ev_lo + (int32_t)Q.id[c < QF ? c : 0][lane] : -1;
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const int32_t jr = __shfl(jout, 8 * r + (lane >> 3), 64);
                pv[r] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (jr >= 0) pv[r] = reinterpret_cast<const float4 *>(a.x + (int64_t)jr * 32)[lane & 7];
            }
        };
        auto round = [&](const float4 (&pv)[8], int32_t j, bool have) {
            wave_sync();
#pragma unroll
            for (int r = 0; r < 8; ++r) *reinterpret_cast<float4 *>(&rows[8 * r + (lane >> 3)][4 * (lane & 7)]) = pv[r];
            wave_sync();
            if (have) {
                float dc = 0.0f;
#pragma unroll
                for (int c4 = 0; c4 < 8; ++c4) {
                    const float4 v = *reinterpret_cast<const float4 *>(&rows[lane][4 * c4]);
                    float df;
                    df = v.x - qrow[4 * c4 + 0]; dc = __builtin_fmaf(df, df, dc);
                    df = v.y - qrow[4 * c4 + 1]; dc = __builtin_fmaf(df, df, dc);
                    df = v.z - qrow[4 * c4 + 2]; dc = __builtin_fmaf(df, df, dc);
                    df = v.w - qrow[4 * c4 + 3]; dc = __builtin_fmaf(df, df, dc);
                }
                // sorted insert by (d, j) (R2)
#pragma unroll
                for (int p = KP - 1; p >= 1; --p) {
                    const bool gq = kd[p - 1] > dc || (kd[p - 1] == dc && kj[p - 1] > j);
                    const bool gp = kd[p] > dc || (kd[p] == dc && kj[p] > j);
                    const float dn = gq ? kd[p - 1] : (gp ? dc : kd[p]);
                    const int32_t jn = gq ? kj[p - 1] : (gp ? j : kj[p]);
                    kd[p] = dn; kj[p] = jn;
                }
                if (kd[0] > dc || (kd[0] == dc && kj[0] > j)) { kd[0] = dc; kj[0] = j; }
            }
        };
        float4 pa[8], pb[8];
        int32_t ja = -1, jb = -1;
        fetch(0, pa, ja);
        fetch(1, pb, jb);
        for (int c = 0; c < maxcnt; c += 2) {
            {
                float4 cur[8];
#pragma unroll
                for (int r = 0; r < 8; ++r) cur[r] = pa[r];
                const int32_t jc = ja;
                if (c + 2 < maxcnt) fetch(c + 2, pa, ja);
                round(cur, jc, c < mycnt);
            }
            if (c + 1 < maxcnt) {
                float4 cur[8];
#pragma unroll
                for (int r = 0; r < 8; ++r) cur[r] = pb[r];
                const int32_t jc = jb;
                if (c + 3 < maxcnt) fetch(c + 3, pb, jb);
                round(cur, jc, c + 1 < mycnt);
            }
        }
        if (valid) {
            const int k = a.k;
            float kth = -1.0f;
#pragma unroll
            for (int p = 0; p < KP; ++p) {
                if (p < k) {
                    a.nbr[(int64_t)myq * k + p] = kj[p];
                    a.dist[(int64_t)myq * k + p] = kd[p];
                }
                if (p == k - 1 && kj[p] >= 0) kth = kd[p];
            }
            if (a.nbr16) {
                uint16_t *r16 = a.nbr16 + (int64_t)myq * k;
                if ((k & 1) == 0) {   // two ids per dword store
#pragma unroll
                    for (int p = 0; p + 1 < KP; p += 2)
                        if (p < k)
                            reinterpret_cast<unsigned *>(r16)[p >> 1] =
                                (unsigned)local_id16(kj[p], ev_lo) | ((unsigned)local_id16(kj[p + 1], ev_lo) << 16);
                } else {
#pragma unroll
                    for (int p = 0; p < KP; ++p)
                        if (p < k) r16[p] = local_id16(kj[p], ev_lo);
                }
            }
            // certificate: a list that saw at least M keys dropped only keys >= tau
            const float tau = L.tk[M - 1];
            const float nx = a.nrm[myq];
            const float an = __builtin_sqrtf(nx) * 1.000001f;
            const float rn = an + __builtin_sqrtf(fmaxf(kth, 0.0f)) * 1.00002f;
            const float slack = 2.0f * (4e-5f * an * rn + 1e-5f * rn * rn + 4e-6f * an * an) + 1e-30f;
            const bool full = tau < kKnnSentinel;
            if (L.overflow || !fits || (full && !(tau + nx - slack > kth))) {
                flag_query(a, myq, a.xtile_ptr[pos] + (myq - ev_lo) / a.xtile_queries);
            }
        }
        return;
    }
    // ---- split (tail) items: hand the partial list to knn_rerank_kernel, which merges the sub-sweeps ---------------
    if (a.no_rerank) {   // the caller's size hint ruled this event out and the merge launch was dropped: exact path
        if (valid && sub == 0) flag_query(a, myq, a.xtile_ptr[pos] + (myq - ev_lo) / a.xtile_queries);
        return;
    }
    if (valid) {
        const int64_t slot = (int64_t)(tile - n_full) * kFQ + hh * 32 + col;
        float *ld = a.psd + (slot * nsub + sub) * MS;
        int32_t *lj = a.psj + (slot * nsub + sub) * MS;
        // keys below the threshold first, then ties at the threshold until the list is full (a dropped tie has
        // key == threshold, which is what the certification assumes of dropped candidates)
        const float tfin = L.tk[M - 1];
        int out = 0;
        for (int pass = 0; pass < 2; ++pass)
            for (int s = 0; s < L.cnt; ++s) {
                const float key = __uint_as_float(Q.key[s][lane]);
                if ((pass == 0 ? key < tfin : key == tfin) && out < M) {
                    ld[out] = key;
                    lj[out] = ev_lo + (int32_t)Q.id[s][lane];
                    ++out;
                }
            }
        for (; out < M; ++out) { ld[out] = kKnnSentinel; lj[out] = -1; }
        ld[M] = L.tk[M - 1];              // the list's admission threshold (sentinel while fewer than M keys were seen)
        lj[M] = (L.overflow || !fits) ? 1 : 0;
    }
}

// first form alone: DMET_KNN_FILTER=1 (every event), A/B timing
template <int KP>
__global__ __launch_bounds__(kWave * kWavesPerGroup, 2) void knn_filter_kernel(const KnnFilterArgs a)
{
    __shared__ FilterQueue<filter_queue_len(filter_list_len(KP))> queue_all[kWavesPerGroup];
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    filter1_wave<KP>(a, queue_all[wv], (int)blockIdx.x, wv, lane);
}


// ---- filter, second form ("tile masks"): events of kF2MinNodes .. 65536 nodes ------------------------------------------
// Budget of the first form at 64 x 4500 x 32 (tools/knn_budget.sh, ablation builds): once the operands arrive as
// contiguous records the kernel is bound by the per-key push -- two LDS stores per key on a 64 B/clk store path plus
// ~5 VALU ops -- and by the drains that re-read the queue.  This form keeps the per-key work to a compare and a carry
// add (a 32-bit hit mask per lane and tile) and touches LDS once per TILE:
//   * tau of a query = the M-th smallest TILE MINIMUM seen so far (a v_min3 tree over the lane's 32 keys, then the
//     v_med3 insertion chain once per tile): every one of those M tiles holds a key <= tau, so at least M >= k
//     candidates lie at or below it, and it is refreshed every tile instead of every drain;
//   * mask bit r = key of candidate row r < tau (the value before this tile's update); a tile with a non-zero mask
//     appends ONE 8-byte entry {mask, tile minimum | tile number};
//   * entries whose tile minimum exceeds the current tau are dropped when a lane runs out of slots and once at the
//     end: what survives are the ~M tiles that hold the list's keys.  Every dropped candidate -- an unset bit, a tile
//     that was never appended, a dropped entry -- had key >= the tau of its time >= the final tau: the same
//     certificate as the first form with T = tk[M-1];
//   * the first kF2Defer tiles only feed tau; they are swept again at the end against the final tau (their masks
//     would otherwise be nearly full: tau is still the sentinel there);
//   * the exact re-rank walks the set bits of the surviving entries.
#ifndef DMET_F2_DEFER
#define DMET_F2_DEFER 32
#endif
constexpr int kF2Defer = DMET_F2_DEFER;   // tiles that only feed tau in the main sweep
// DMET_F2_LEAN (experiment builds, tools/knn_lean.sh): THREE wavefronts per SIMD -- 26 entry slots, no row staging area
// (13 KB of LDS per wavefront, 12 wavefronts per CU), registers capped at 168 by the launch bounds
#ifdef DMET_F2_LEAN
constexpr int kF2Slots = 26;
constexpr int kF2StageRows = 4;
constexpr int kF2WavesPerSimd = 3;
#else
constexpr int kF2Slots = 30;        // entries per lane
constexpr int kF2StageRows = kWave;
constexpr int kF2WavesPerSimd = 2;
#endif
constexpr int kF2RowF = 16;         // features staged per re-rank half round
constexpr unsigned kF2TileBits = 11u, kF2TileMask = (1u << kF2TileBits) - 1u;

struct F2Wave {
    uint2 ent[kF2Slots][kWave];              // 15 360 B
    float rows[kF2StageRows][kF2RowF + 4];   //  5 120 B: half rows of the re-rank (16-byte aligned, conflict-free b128)
};
#ifndef DMET_F2_LEAN
static_assert(sizeof(F2Wave) == 20480, "two workgroups of four wavefronts fill the CU's 160 KB exactly");
#else
static_assert(sizeof(F2Wave) * 12 <= 163840, "three workgroups of four wavefronts per CU");
#endif

template <int M>
struct F2Lane {
    float tk[M];     // the M smallest tile minima, sorted
    float tau;       // admission threshold (= min(tk[M-1], tk[k-1] + margin); -inf for idle lanes / after an overflow)
    float margin;    // the running cut's distance above tk[k-1] (filter2_wave sets it before the main sweep); +inf: no cut
    unsigned tq;     // tau as the query side of the fold (f2_tau16; 0 while no mask is recorded)
    float rep;       // the threshold tq stands for (>= tau, or kF2TauRepMax)
    int cnt;         // entries in the lane's queue
    bool overflow;
};

// Drop the entries whose tile minimum is above tau.  The stored minimum carries the tile number in its low 11 mantissa
// bits; clearing them is monotone in the float order (x <= y => trunc(x) <= trunc(y)), so "trunc(stored) <= trunc(tau)"
// keeps every tile with minimum <= tau and at most the tiles within 2^-12 |tau| above it.  (Round 2, second session:
// the comparison used to allow 2^-10 |tau| on either side; with M = 22 one query per build of the benchmark's
// embeddings had five tile minima inside that window, ended with 27 entries and was handed to the fallback.)
// `limit`: entries a lane may keep -- during a sweep it needs room to append before the next compaction, at the end
// every slot may be in use.
template <int M>
__device__ __forceinline__ void f2_compact(F2Lane<M> &L, F2Wave &S, int lane, int limit)
{
    const float tauT = __uint_as_float(__float_as_uint(L.tau) & ~kF2TileMask);
    int maxcnt = L.cnt;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) maxcnt = max(maxcnt, __shfl_xor(maxcnt, off, 64));
    int out = 0;
    for (int s = 0; s < maxcnt; ++s) {
        if (s < L.cnt) {
            const uint2 e = S.ent[s][lane];
            if (!(__uint_as_float(e.y & ~kF2TileMask) > tauT)) { S.ent[out][lane] = e; ++out; }
        }
    }
    L.cnt = out;
    if (out > limit) {   // too many tiles tied at tau: leave the query to the exact path
        L.overflow = true;
        L.cnt = 0;
        L.tau = -__builtin_inff();
    }
}

// Query side of the fold block for one 32-query block, the same in every lane: {y_0, y_1, 0, 0, P1, P2, P3, P4} with
// tq = (y_0, y_1) packed (f2_tau16).  Lanes hh = 0 meet the zeros of the candidate side in slots 0, 1 and the norm
// terms in 4..7; lanes hh = 1 meet the threshold scales in 0, 1 and zeros in 4..7.
__device__ __forceinline__ f16x8 f2_fold(unsigned tq)
{
    const f16x8 pc = {(_Float16)0.0f, (_Float16)0.0f, (_Float16)0.0f, (_Float16)0.0f, (_Float16)kF2NormP[0],
                      (_Float16)kF2NormP[1], (_Float16)kF2NormP[2], (_Float16)kF2NormP[3]};
    uint4 u = __builtin_bit_cast(uint4, pc);
    u.x = tq;
    return __builtin_bit_cast(f16x8, u);
}

// The fold operands of both 32-query blocks live across a whole sweep (f2_sweep builds them, f2_tile reads them): only the
// threshold dword changes, and only where the threshold is converted.  v_permlane32_swap hands every lane the two
// thresholds of its lane pair (query (0, col), (1, col)); the constant dwords stay where they are.
__device__ __forceinline__ void f2_fold_tau(f16x8 (&fq)[2], unsigned tq)
{
    const auto tt = __builtin_amdgcn_permlane32_swap(tq, tq, false, false);
    uint4 u0 = __builtin_bit_cast(uint4, fq[0]), u1 = __builtin_bit_cast(uint4, fq[1]);
    u0.x = tt[0];
    u1.x = tt[1];
    fq[0] = __builtin_bit_cast(f16x8, u0);
    fq[1] = __builtin_bit_cast(f16x8, u1);
}

// Operands of one candidate tile: single-term fp16 records (see knn_prep_kernel).  32 features: the A fragments + the
// fold fragment.  64 features: the A fragments + the fp32 accumulator seed (the squared norms of the 16 candidate rows
// the lane receives results for, rows (e & 3) + 8 (e >> 2) + 4 hh) -- the fold's registers and conversions pushed the
// 64-feature kernels, which hold sixteen query fragments, into more scratch; their keys still need the subtract.
template <int NH = 1>
struct F2Ops {
    f16x8 a[2 * NH];
    f16x8 f;
};
template <>
struct F2Ops<2> {
    f16x8 a[4];
    f32x16 c;
};

// One 32(candidates) x 32(queries) block: acc = fold (or seed) + sum over the 16-feature k-blocks of h.h' (fp16
// operands, fp32 accumulate).  Operand map of v_mfma_f32_32x32x16_f16: lane (r = lane & 31, hh = lane >> 5) holds
// A[row r][k = 8 hh + 0..7].  32 features: 3 MFMAs, the first one from the inline constant 0 -- the fold block (o.f from
// the record, f2_fold(tq) on the query side) is  sum_k A[j][k] B[k][i] = N1 P1 + .. + N4 P4 + 2^14 y_0(i) +
// 2^-15 y_1(i) = |x_j|^2 - tau_rep(i) up to the norm's rounding: every product is exact in fp32 and the ones of the zero
// slots are 0 (every operand there is finite).  64 features: 4 MFMAs from the seed (keys, `fold` unused).
template <int NH = 1>
__device__ __forceinline__ f32x16 f2_block(const F2Ops<NH> &o, const f16x8 (&bv)[2 * NH], const f16x8 &fold)
{
    f32x16 acc;
    if constexpr (NH == 1) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(o.f, fold, f32x16{}, 0, 0, 0);
    else acc = o.c;
#pragma unroll
    for (int m = 0; m < 2 * NH; ++m) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(o.a[m], bv[m], acc, 0, 0, 0);
    return acc;
}

// one fp16 candidate tile record: the lane's 2 NH A operands and its part of the fold fragment (or its 16 norms)
// rofs: 16 x lane, the lane's byte offset inside a fragment (32 features)
template <int NH = 1>
__device__ __forceinline__ void f2_load(F2Ops<NH> &o, const uint8_t *__restrict__ rec, int64_t tidx, int lane, int hh,
                                        unsigned &rofs)
{
    if constexpr (NH == 1) {
        // the record number is wave-uniform (filter2_wave) but only readfirstlane tells the compiler: the three loads
        // then take a scalar base, one 32-bit lane offset and the immediates 0 / 1024 / 2048 instead of a 64-bit
        // multiply-add per lane and tile
        const uint64_t sb = reinterpret_cast<uint64_t>(rec + tidx * rec_bytes(NH));
        const uint64_t ub = ((uint64_t)(unsigned)__builtin_amdgcn_readfirstlane((int)(sb >> 32)) << 32) |
                            (unsigned)__builtin_amdgcn_readfirstlane((int)sb);
        // (a pointer made from an integer is a global-memory pointer only if its type says so)
        typedef const f16x8 __attribute__((address_space(1))) *GlobalFrag;
        // the lane's byte offset, made opaque at every load: left to itself hipcc widens it to 64 bits once, outside
        // the loop, and adds the base to it per lane and tile.  The copy is handed on (rofs is the caller's), so it
        // costs no move
        asm volatile("" : "+v"(rofs));
        const GlobalFrag g = (GlobalFrag)(ub + (uint64_t)rofs);
#pragma unroll
        for (int m = 0; m < 2; ++m) o.a[m] = g[m * 64];
        o.f = g[2 * 64];
    } else {
        const uint8_t *base = rec + tidx * rec_bytes(NH);
        const f16x8 *g = reinterpret_cast<const f16x8 *>(base);
#pragma unroll
        for (int m = 0; m < 2 * NH; ++m) o.a[m] = g[m * 64 + lane];
        const float4 *nr = reinterpret_cast<const float4 *>(base + kRec16FragBytes * NH);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 v = nr[2 * q + hh];
            o.c[4 * q] = v.x; o.c[4 * q + 1] = v.y; o.c[4 * q + 2] = v.z; o.c[4 * q + 3] = v.w;
        }
    }
}

// The threshold as the query side of the fold: returns (y_0, y_1) packed and sets rep = -(2^14 y_0 + 2^-15 y_1), a
// value >= tau (or kF2TauRepMax, see f2_cert_T), so that a key below tau has a negative fold result.  down(v) moves v
// down by 2^-9 |v| + 2^-24 (more than an fp16 ulp at |v|, normal or subnormal, and than the fp32 rounding of v) and
// rounds toward zero, i.e. down for v > 0 and up by less than the move for v < 0: down(v) <= v, within 2^-8 |v| + 2^-23.
// y_0 = x with x = -tau / 2^14 (clamped to +-65504: -inf, idle lanes, gives rep = -65376 x 2^14 and only forced
// candidates, key -inf, are admitted there; a tau beyond kF2TauRepMax gives rep = kF2TauRepMax) moved down by 2^-9 |x|
// and rounded toward zero: below x in the fp16 normal range, 0 for |x| < 2^-25 (|tau| < 2^-11), within one subnormal
// step of x between.  The remainder (x - y_0) 2^29 (> -32, rounded once) goes to the second term: y_1 = down(min(it,
// 65504)) <= it.  rep - tau stays within 2^-16 |tau| for 1 <= |tau| < 676; it reaches ~2^-11 |tau| for 676 <= |tau| <
// 2^10 (the remainder is clipped at 65504), ~2^-15 |tau| for 0.1 <= |tau| < 1 (y_0 is an fp16 subnormal there), and is
// never more than 2^-8 |tau| + 2^-38.  A looser tau_rep only admits more candidates.
__device__ __forceinline__ unsigned f2_tau16(float tau, float &rep)
{
    const float x = __builtin_amdgcn_fmed3f(-tau * (1.0f / kF2TauC[0]), -65504.0f, 65504.0f);
    float v = __builtin_amdgcn_fmed3f(__builtin_fmaf(__builtin_fabsf(x), -0x1p-9f, x), -65504.0f, 65504.0f);
    const float y0 = (float)__builtin_amdgcn_cvt_pkrtz(v, v)[0];
    const float w = __builtin_fmaf(-y0, kF2TauC[0] / kF2TauC[1], x * (kF2TauC[0] / kF2TauC[1]));
    v = fminf(__builtin_fmaf(__builtin_fabsf(w), -0x1p-9f, w - 0x1p-24f), 65504.0f);
    const auto y = __builtin_amdgcn_cvt_pkrtz(y0, v);   // y0 is an fp16 value already: converted exactly
    rep = -__builtin_fmaf(y0, kF2TauC[0], (float)y[1] * kF2TauC[1]);   // rounded once: f2_key_lower covers it
    return __builtin_bit_cast(unsigned, y);
}

// A key-space lower bound of the tile's keys from the minimum cmin of its fold results computed against rep: the fp32
// sum is moved down by more than its rounding, and by 2^-17 |rep| for the share of the MFMA's accumulation error that
// the threshold term brings (<= 79 x 2^-24 |rep| for the 80 products of a 64-feature block).  Entries store this
// value (f2_compact drops an entry only when it is above tau) and the threshold list is built from it.
__device__ __forceinline__ float f2_key_lower(float cmin, float rep)
{
    const float s = cmin + rep;
    return __builtin_fmaf(__builtin_fabsf(s), -0x1p-22f, __builtin_fmaf(__builtin_fabsf(rep), -0x1p-17f, s));
}

// The threshold a certificate may use for a lane whose masks were taken against tau (or any larger one): the fold
// applied rep >= min(tau, kF2TauRepMax), and a fold result >= 0 proves key >= rep - 2^-17 |rep| - (the share of the
// other terms, in f2_slack); t - 2^-17 |t| is increasing in t, so the bound holds with T = min(tau, kF2TauRepMax) in
// place of rep (2^-16 and the constant take the fp32 rounding of this expression).
// (64 features keep the subtract: their masks are exact against tau, T = tau, and a tau still at the sentinel dropped
// nothing -- kF2Full says whether such a lane needs the check at all)
template <int NH = 1>
__device__ __forceinline__ float f2_cert_T(float tau)
{
    if constexpr (NH != 1) return tau;
    const float T = fminf(tau, kF2TauRepMax);
    return __builtin_fmaf(__builtin_fabsf(T), -0x1p-16f, T) - 1e-16f;
}
template <int NH = 1>
__device__ __forceinline__ bool f2_full(float tau) { return NH == 1 || tau < kKnnSentinel; }

// Certificate slack of the second form (dropped candidates had key >= T; true d >= T + |x_i|^2 - slack).  an >= |x_i|,
// rn >= |x_i| + sqrt(d_k): a candidate with a larger norm than rn is farther than d_k by the triangle inequality, so the
// bound only has to hold for |x_j| <= rn.  Terms:
//   * the bound of the split form (fp32 accumulation inside the MFMAs, squared norms, the R1 chain itself), `scale` x
//     (1.5 at 64 features: twice the products per key), with its 2 x margin;
//   * fp16 operands: each rounds with relative error <= 2^-11 (normal range; |v| < 16384 is guaranteed by the record
//     writer), the products are exact in fp32, so |x.x' - h.h'| <= (2^-10 + 2^-22) sum_c |x_c||x'_c| <= 1.0003 x 2^-10
//     |x||x'| (Cauchy-Schwarz), twice that on the key: 2^-9 an rn, taken as 1.96e-3 (> 1.0003 x 2^-9 = 1.9537e-3);
//   * fp16 subnormals (|v| < 2^-14): absolute error <= 2^-25 per feature, on the key <= 2 x 2^-25 x sqrt(D) (|x|+|x'|)
//     <= 4.8e-7 (an + rn) at D <= 64; taken as 6e-7;
//   * the norm in the fold block (knn_prep_kernel): four fp16 terms, |s - sum| <= 2^-44 s + 2^-40 <= 6e-14 rn^2 + 1e-12.
//     The fold's longer sum (2 NH x 16 + 16 products) is still covered by the accumulation term above, which carried
//     the fp32 seed |x_j|^2 before; the threshold's own share of it is taken off tau itself (f2_cert_T).
__device__ __forceinline__ float f2_slack(float an, float rn, float scale)
{
    return 2.0f * scale * (4e-5f * an * rn + 1e-5f * rn * rn + 4e-6f * an * an) + 1.96e-3f * an * rn + 6e-7f * (an + rn) +
           6e-14f * rn * rn + 1e-12f;
}

// The smallest threshold that certifies the k-th distance kth of a query with squared norm nx under `slack`:
// kth - |x|^2 + slack, nudged up by f2_cert_T's margin and a few ulps of the largest term so that the certificate's own
// fp32 expression holds for it.
template <int NH = 1>
__device__ __forceinline__ float f2_cert_threshold(float kth, float nx, float slack)
{
    float ts = kth - nx + slack;
    ts += __builtin_fabsf(ts) * ((NH == 1 ? 0x1p-15f : 0.0f) + 4.8e-7f) + (nx + slack) * 4.8e-7f + (NH == 1 ? 2e-16f : 1e-30f);
    return ts;
}

// Final threshold of a first attempt, decoupled from the list length M.  tkk = tk[k-1] is the k-th smallest tile
// minimum: k tiles each hold a candidate with key <= tkk (up to the rounding-down of f2_key_lower), so the query's k-th
// distance is at most U = tkk + |x|^2 + slack(U), and every threshold from f2_cert_threshold(U) upwards certifies it.
// U is implicit (the slack grows with sqrt(U)): two substitutions from U_0 = tkk + |x|^2 settle it far inside the
// margin, slack / U being a few 1e-3.  `scale` stretches the distance of the cut from tkk: 1 is the bound itself, 0
// gives tkk, too tight wherever tkk is the k-th key itself (the certificate fails, the second attempt takes over: tests).
// Nothing rests on this bound: the certificate is evaluated with the threshold that was applied, and a lane whose cut
// was too tight fails it like any slack-only failure.  A NaN or infinite result (keys near the sentinel) leaves the
// caller's fminf() with today's threshold.
template <int NH = 1>
__device__ __forceinline__ float f2_cut(float tkk, float nx, float scale)
{
    const float sc = NH == 1 ? 1.0f : 1.5f;
    const float an = __builtin_sqrtf(nx) * 1.000001f;
    const float u0 = fmaxf(tkk + nx, 0.0f);
    float s = f2_slack(an, an + __builtin_sqrtf(u0) * 1.00002f, sc);
    s = f2_slack(an, an + __builtin_sqrtf(u0 + s) * 1.00002f, sc);
    const float U = u0 + s;
    const float ts = f2_cert_threshold<NH>(U, nx, f2_slack(an, an + __builtin_sqrtf(U) * 1.00002f, sc));
    return __builtin_fmaf(scale, ts - tkk, tkk);
}

// threshold list length of the second form: the fp16 slack needs the M-th smallest tile minimum two ranks further out
// than the split form did (measured on the model's embeddings at k = 16: uncertified queries per 4500-node event
// ~10 at KP + 4, ~2 at KP + 5, ~0.1 at KP + 6); a lane keeps kF2Slots = 30 entries, so the widest list stays at 24
constexpr int f2_list_len(int KP) { return KP <= 16 ? KP + 6 : KP + 4; }
// the result capacity KP a list of M belongs to (the instances are KP = 8, 16, 20: filter2_wave asserts the round trip)
constexpr int f2_list_cap(int M) { return M <= 22 ? M - 6 : M - 4; }

// The running cut.  The main sweep used to record its hit masks against tk[M-1] alone ("the parent" below), with the
// cut above tk[k-1] (f2_cut) applied once it was over: the cut drops whole entries, but every bit that was set
// between the final threshold and tk[M-1] inside a surviving entry still went through a re-rank round.  The main sweep
// therefore records against  tau = min(tk[M-1], tk[KP-1] + margin)  with `margin` = f2_cut(tk[k-1]) - tk[k-1] taken
// once per first attempt and lane after the deferred pass, padded upward by 1 % (filter2_wave).  Tables and counters
// stay the parent's:
//   * tk[] does not depend on the masks, so the lists are the parent's;
//   * fp addition of a constant is monotone and both tk[M-1] and tk[KP-1] only fall, so the thresholds the masks are
//     taken against (f2_tile: what a CONV tile converts at 32 features, tau in every tile at 64) are non-increasing over
//     the sweep, and the sweep leaves tau at min(tk[M-1], tk[k-1] + margin) of the final list, or at its tk[M-1];
//   * margin was taken at a larger tk[k-1]; f2_cut's margin grows with tk[k-1] (the slack grows with sqrt(tk[k-1] +
//     |x|^2)) up to its few-ulp nudges, which the pad covers: tk[k-1] + margin >= f2_cut(final tk[k-1]);
//   * so the final threshold, min(tau, f2_cut(final tk[k-1])), is the parent's min(tk[M-1], cut) bit for bit;
//   * every threshold applied on the way is at least that value: every dropped candidate had a key at or above it,
//     which is all the certificate asks -- same outcomes, same flagged queries, same second attempts.  Only stray bits
//     and entries disappear; a lane can only overflow more rarely;
//   * should the pad ever be too small, the final min() hands the certificate the smallest threshold that was applied:
//     that costs a second attempt, never a wrong row.
// "Same outcomes" holds for every certificate that passes, and for WHICH queries fail: a stray candidate has a key at
// or above the final threshold T, so where the certificate passes it is farther than d_k and never entered the list,
// and where it fails, it fails without the strays as well (the k-th distance of fewer candidates is no smaller).  A
// query that fails may see a larger k-th distance than it did with its strays, and starts its second attempt from a
// larger T*: still exact, admits more.  It also needs a margin > 0: k tiles hold a key <= tk[k-1] < T, so the first
// attempt always has its k candidates; at a margin of exactly zero (DMET_KNN_CUT=0.0: T = tk[k-1]) that count rested on
// the stray bits, and queries that used to retry were flagged instead (measured, one 2000-node event at 32 features,
// k = 16: 49 flagged / 616 retried against 20 / 649).  The running cut is therefore off at a zero margin.
// The slot is the compile-time KP - 1 (a runtime k would cost a KP-long select chain per tile): with k != KP the margin
// stays +inf, as it does without a cut (DMET_KNN_CUT=off), with DMET_KNN_RUNCUT=0, while tk[k-1] is the sentinel, and
// when the margin is not a finite number > 0.
template <int M>
__device__ __forceinline__ float f2_running_tau(const F2Lane<M> &L)
{
    float t = L.tk[f2_list_cap(M) - 1] + L.margin;     // (sentinel + inf = inf; no operand is a NaN)
    asm("v_min_f32 %0, %0, %1" : "+v"(t) : "v"(L.tk[M - 1]));
    return t;
}

// candidate row (0..31) of hit-mask position p (counted from the most significant bit), see f2_tile
__device__ __forceinline__ int f2_mask_row(int p) { return (p & 3) + 8 * ((p & 15) >> 2) + 4 * (p >> 4); }

// One tile of a sweep, software-pipelined inside the wavefront: the 12 MFMAs of tile t + 1 (operands `use`) are
// issued between the vector instructions that select from tile t's keys (c0, c1, computed one call earlier), and the
// operands of tile `t_load` -- two or four tiles ahead: f2_sweep, f2_sweep4 -- are loaded into `ld`.  On gfx950
// independent VALU work of the same wavefront hides under an MFMA (tools/mfma_overlap_micro.hip: 12 v_add per
// 32x32x16 MFMA interleaved cost 62 cycles per slot against 85 when the two run in phases), but only if it is in
// program order between the MFMAs: the scheduler is told to emit 1 MFMA + 11 VALU groups.  UPD: the tile minima feed tk / tau;  REC: hit masks are recorded.
// INS: this call inserts min(carry, its tile minimum) into the threshold list (every second tile: the list then holds the
// M smallest minima of tile PAIRS -- still M groups that each contain a key <= tau); otherwise it only updates `carry`.
// NH = 2 (64 features): `use` and `ld` are the SAME operand set (two sets of eight fragments next to the sixteen of
// the queries do not fit the register file at two wavefronts per SIMD), reloaded right after its MFMAs were issued.
template <int M, bool UPD, bool REC, bool INS, int NH = 1, bool CONV = true>
__device__ __forceinline__ void f2_tile(F2Lane<M> &L, F2Wave &S, const uint8_t *__restrict__ rec, int64_t rbase, int t,
                                        int t_load, f32x16 &c0, f32x16 &c1, f32x16 &n0, f32x16 &n1, float &rc, float &rn,
                                        const F2Ops<NH> &use, F2Ops<NH> &ld, const f16x8 (&bq)[2][2 * NH], f16x8 (&fq)[2],
                                        int lane, int hh, bool alive, float &carry, unsigned &rofs)
{
#if defined(DMET_F2_ABL) && DMET_F2_ABL >= 2
    constexpr bool kRec = false;     // cycle-budget experiment (tools/knn_budget2.sh)
#else
    constexpr bool kRec = REC;
#endif
#if defined(DMET_F2_ABL) && DMET_F2_ABL >= 3
    constexpr bool kUpd = false;
#else
    constexpr bool kUpd = UPD;
#endif
    if (kRec) {
        if (__any(L.cnt >= kF2Slots - 1)) f2_compact<M>(L, S, lane, kF2Slots - 3);
    }
#if defined(DMET_F2_SAMEREC)
    f2_load<NH>(ld, rec, rbase + (t & 1), lane, hh, rofs);   // experiment: operands always cache-resident
#else
    f2_load<NH>(ld, rec, rbase + t_load, lane, hh, rofs);   // clamped: the last calls re-read the last tile
#endif
    // the fold against the thresholds as they are now (tile t + 1's keys: stale by one update, i.e. larger -- a
    // superset): fq holds them since the last conversion (f2_sweep, or the CONV tile below).
    // Sweeps that record no masks fold threshold 0: their results are the keys themselves.
    n0 = f2_block<NH>(use, bq[0], fq[0]);     // (s_setprio 1 around these was measured: 10 % slower)
    n1 = f2_block<NH>(use, bq[1], fq[1]);
    rn = L.rep;
    // The accumulators stay where the MFMAs left them: lane (col, hh) holds, for candidate rows (e & 3) + 8 (e >> 2) + 4 hh,
    // the keys of query (0, col) in c0 and of query (1, col) in c1 -- 16 keys of each of the two queries the lane PAIR
    // (col, 0), (col, 1) owns.  Every lane reduces both halves it holds (hit mask against the owner's threshold, minimum)
    // and the pair exchanges the REDUCED values: v_permlane32_swap(V0, V1) trades V0 of lanes 32..63 for V1 of lanes
    // 0..31, so with V0 = "my part for query (0, col)" and V1 = "my part for query (1, col)" every lane ends up with
    // V0 = the hh = 0 rows' part and V1 = the hh = 1 rows' part of ITS OWN query.  Two swaps per tile (masks, minima;
    // a third for the thresholds where they are converted, f2_fold_tau) instead of the sixteen that moved the
    // accumulators themselves (second session of round 2; a swap costs two issue slots and sat between the MFMA results
    // and everything else).
    unsigned mask = 0u;
    unsigned ha = 0u, hb = 0u;     // the masks after element 0: see the v_min3 trees below
    if (kRec) {
        // One VALU op per key: the fold result is key - rep, v_alignbit shifts its sign bit into the mask (a -0 would
        // set a bit: admitted, never dropped).  Element e of a half ends up in bit 15 - e.
        // (64 features: the keys themselves, key - tau first, thresholds of query (0, col) / (1, col) from the swap)
        unsigned ma = 0u, mb = 0u;
        if constexpr (NH == 1) {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                ma = __builtin_amdgcn_alignbit(ma, __float_as_uint(c0[e]), 31);
                mb = __builtin_amdgcn_alignbit(mb, __float_as_uint(c1[e]), 31);
                if (e == 0) ha = ma, hb = mb;
            }
        } else {
            const auto tt = __builtin_amdgcn_permlane32_swap(__float_as_uint(L.tau), __float_as_uint(L.tau), false, false);
            const float t0 = __uint_as_float(tt[0]), t1 = __uint_as_float(tt[1]);
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                ma = __builtin_amdgcn_alignbit(ma, __float_as_uint(c0[e] - t0), 31);
                mb = __builtin_amdgcn_alignbit(mb, __float_as_uint(c1[e] - t1), 31);
                if (e == 0) ha = ma, hb = mb;
            }
        }
        const auto mm = __builtin_amdgcn_permlane32_swap(ma, mb, false, false);
        // bit 31 - p: p < 16 -> element p of the hh = 0 rows, else element p - 16 of the hh = 1 rows (f2_mask_row)
        mask = (mm[0] << 16) | mm[1];
    }
    float tmin = -__builtin_inff();   // deferred tiles: "never drop" (their tau is already final)
    if (kUpd) {
        // the trees start from the sentinel (the first operand also keeps a NaN key out of the v_med3 chain), taken as
        // a scalar source: a VOP3 encoding has no literal, and a "+v" start value costs a v_mov per tree and tile
        // v_min3_f32 by hand: fminf() makes hipcc canonicalise every MFMA output with a v_max first (twice the ops)
        // These statements read accumulators that MFMAs have just written, and hipcc pads the wait states an MFMA's
        // result needs before its first reader (12 after an 8-pass one) only for readers it knows: an asm statement
        // gets none, and one scheduled right behind its MFMA takes the minimum of stale registers -- a wrong threshold
        // (other flagged-query and second-attempt counts, never a wrong table).  So each tree hangs on an instruction
        // of hipcc's own that reads its accumulator block.  A recording call has one: the first v_alignbit of the
        // block's hit mask, named as an unused operand of the tree's first statement (no instruction).  The other
        // calls (deferred pass; the ablation builds) form the tree's sentinel with a v_med3 that reads a key and
        // returns the sentinel whatever the key is (median of S, S, x): one instruction per tree.
        // (profiles/r10_knn_counted_waits.md: the deferred pass as a four-call trip put a tree directly behind its
        // MFMA; tools/knn_mfma_asm_distance.py lists the distances, tests/test_knn_wait_counts_asm.py holds them.)
        float na, nb;
        if (kRec) {
            asm("v_min3_f32 %0, %1, %2, %3" : "=v"(na) : "s"(kKnnSentinel), "v"(c0[0]), "v"(c0[1]), "v"(ha));
            asm("v_min3_f32 %0, %1, %2, %3" : "=v"(nb) : "s"(kKnnSentinel), "v"(c1[0]), "v"(c1[1]), "v"(hb));
        } else {
            const float sa = __builtin_amdgcn_fmed3f(kKnnSentinel, kKnnSentinel, c0[0]);
            const float sb = __builtin_amdgcn_fmed3f(kKnnSentinel, kKnnSentinel, c1[0]);
            asm("v_min3_f32 %0, %1, %2, %3" : "=v"(na) : "v"(sa), "v"(c0[0]), "v"(c0[1]));
            asm("v_min3_f32 %0, %1, %2, %3" : "=v"(nb) : "v"(sb), "v"(c1[0]), "v"(c1[1]));
        }
#pragma unroll
        for (int e = 2; e < 16; e += 2) {
            asm("v_min3_f32 %0, %0, %1, %2" : "+v"(na) : "v"(c0[e]), "v"(c0[e + 1]));
            asm("v_min3_f32 %0, %0, %1, %2" : "+v"(nb) : "v"(c1[e]), "v"(c1[e + 1]));
        }
        const auto nn = __builtin_amdgcn_permlane32_swap(__float_as_uint(na), __float_as_uint(nb), false, false);
        tmin = __uint_as_float(nn[0]);
        asm("v_min_f32 %0, %0, %1" : "+v"(tmin) : "v"(__uint_as_float(nn[1])));
        if (NH == 1 && kRec) tmin = f2_key_lower(tmin, rc);   // back to key space, rounded down (the -inf of a forced row stays)
    }
    if (kRec) {
        // one 8-byte entry per tile and lane, kept only when the mask is non-zero (branch-free append)
        const unsigned packed = (__float_as_uint(tmin) & ~kF2TileMask) | (unsigned)t;
        S.ent[L.cnt][lane] = make_uint2(mask, packed);
        L.cnt += (mask != 0u) ? 1 : 0;
    }
    if (kUpd) {
        if (INS) {
            // a tile that holds a forced candidate (key -inf: a row outside the fp16 range, see knn_prep_kernel) does
            // not vote for the threshold: its -inf would take a list slot without standing for a real key below tau
            float v = tmin < -3.0e38f ? kKnnSentinel : tmin;
            asm("v_min_f32 %0, %0, %1" : "+v"(v) : "v"(carry));     // (both operands are clamped to the sentinel: no NaN)
            carry = kKnnSentinel;
#pragma unroll
            for (int p = M - 1; p >= 1; --p) L.tk[p] = __builtin_amdgcn_fmed3f(L.tk[p - 1], v, L.tk[p]);
            asm("v_min_f32 %0, %0, %1" : "+v"(L.tk[0]) : "v"(v));
            // The running cut where a mask threshold is taken from tau: every tile at 64 features, the CONV tiles at 32
            // (the tile between two conversions keeps tk[M-1], which only a compaction reads before the next CONV tile
            // lowers it again: it then drops less, never more; if that tile ends the sweep, the final cut is still
            // applied to tk[M-1], as it was before the running cut).  The deferred pass records nothing: tk[M-1].
            // Formed outside the condition: an asm statement under an `if` becomes an exec-masked branch in every tile,
            // not a select.
            constexpr bool kRun = kRec && (NH != 1 || CONV);
            const float tau = kRun ? f2_running_tau<M>(L) : L.tk[M - 1];
            if (alive && !L.overflow) L.tau = tau;
            if (NH == 1 && kRec && CONV) {   // (every second tile: see f2_sweep)
                L.tq = f2_tau16(L.tau, L.rep);
                f2_fold_tau(fq, L.tq);
            }
        } else {
            carry = tmin;
        }
    }
#ifdef DMET_F2_SCHED
    // experiment: force 1 MFMA + 11 VALU groups (measured 4 % SLOWER than hipcc's own order at two wavefronts per SIMD)
#pragma unroll
    for (int g = 0; g < 12; ++g) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x002, (kRec ? 11 : (kUpd ? 5 : 2)), 0);
    }
#endif
}

// Call Q (0..3) of a four-set trip at tile t: it selects from key block Q & 1, issues the MFMAs of set Q + 1 and loads
// tile t + 4 into set Q, whose MFMAs the call before it issued; the odd calls convert (knn_tile_schedule.h).
template <int M, bool UPD, bool REC, int Q>
__device__ __forceinline__ void f2_trip_call(F2Lane<M> &L, F2Wave &S, const uint8_t *__restrict__ rec, int64_t rbase, int t,
                                             int t_hi, f32x16 &c0, f32x16 &c1, f32x16 &n0, f32x16 &n1, float &rc, float &rn,
                                             F2Ops<1> (&s)[kF2Sets], const f16x8 (&bq)[2][2], f16x8 (&fq)[2], int lane, int hh,
                                             bool alive, float &carry, unsigned &rofs)
{
    static_assert(f2_tile_set(4) == 0 && f2_tile_key_block(2) == 0 && f2_tile_key_block(3) == 1 && !f2_call_converts(2) &&
                      f2_call_converts(3),
                  "the trip below is the schedule's, written out");
    static_assert(Q >= 0 && Q < kF2Sets && f2_remainder_trip_call(Q) == Q, "a remainder call is the same call of a trip");
    constexpr bool kConv = f2_call_converts(Q);
    if constexpr (f2_tile_key_block(Q) == 0)
        f2_tile<M, UPD, REC, true, 1, kConv>(L, S, rec, rbase, t, f2_load_tile(t, kF2Sets, t_hi), c0, c1, n0, n1, rc, rn,
                                             s[f2_trip_use_set(Q)], s[f2_trip_load_set(Q)], bq, fq, lane, hh, alive, carry, rofs);
    else
        f2_tile<M, UPD, REC, true, 1, kConv>(L, S, rec, rbase, t, f2_load_tile(t, kF2Sets, t_hi), n0, n1, c0, c1, rn, rc,
                                             s[f2_trip_use_set(Q)], s[f2_trip_load_set(Q)], bq, fq, lane, hh, alive, carry, rofs);
}

// A recording sweep at 32 features (main sweep, revisit, second attempt): FOUR tiles of operands in flight.  What the
// kernel's time per item holds beyond its own vector issue is waiting for operands (a loaded L2 round trip is ~2000
// cycles, a revisit tile ~250 cycles of work), so call t issues tile t + 1's MFMAs and loads tile t + 4, and the sweep
// requests its first four tiles at once instead of load, wait, MFMA, load.  Four calls per trip: the operand sets rotate
// with period 4, the key blocks (c, n) and the threshold conversions with period 2 (knn_tile_schedule.h, shared with the
// host tests).  Only WHEN operands are loaded differs from a sweep with two sets: the order of MFMAs, conversions,
// insertions and compactions does not.
// The sweep is a loop over WHOLE trips with no exit inside a trip, then its zero to three remaining calls written out.
// With an exit after every call (`for (;;) { call; if (++t >= t_hi) break; ... }`, r09) the loop header joins four
// paths that carry different numbers of loads in flight, and hipcc's wait insertion answers such a join with
// s_waitcnt vmcnt(0): once per trip every outstanding load was drained, the three requested one tile earlier included.
// In this form every tile block waits with a counted vmcnt(N) that leaves the three younger tiles in flight
// (tools/knn_tile_counts.py lists the waits; tests/test_knn_wait_counts_asm.py holds them).  The loads are plain loads
// that hipcc counts itself: no wait is placed by hand.  profiles/r10_knn_counted_waits.md.
// REC = false is the deferred pass on this trip (-DDMET_F2_DEFER_FOUR only): it folds threshold 0 and converts nothing,
// its results are the keys themselves.  As whole trips it does not spill (as a loop with exits it did, r09), its block
// of four tiles waits with counted vmcnt only, the tables and counters are the parent's -- and every one of six
// alternated runs was slower than with the two-set loop of f2_sweep (r10, -0.7 %): the deferred pass keeps two sets.
template <int M, bool UPD, bool REC>
__device__ __forceinline__ void f2_sweep4(F2Lane<M> &L, F2Wave &S, const uint8_t *__restrict__ rec, int64_t rbase, int t_lo,
                                          int t_hi, const f16x8 (&bq)[2][2], int lane, int hh, bool alive)
{
    F2Ops<1> s[kF2Sets];
    unsigned rofs = (unsigned)lane * 16u;
#pragma unroll
    for (int j = 0; j < kF2Sets; ++j) f2_load<1>(s[f2_tile_set(j)], rec, rbase + f2_load_tile(t_lo, j, t_hi), lane, hh, rofs);
    // query side of the fold for both 32-query blocks, built here once per sweep -- from the threshold the sweep starts
    // with (the running cut before the main sweep, the cut before the revisit, t_fix in a second attempt; threshold 0
    // in the deferred pass) -- and kept in registers: the tiles read them, a CONV tile rewrites their threshold dword.
    // Opaque, or hipcc rebuilds them (eight moves and the swap) in every tile rather than hold eight registers
    f16x8 fq[2] = {f2_fold(0u), f2_fold(0u)};
    if constexpr (REC) {
        L.tq = f2_tau16(L.tau, L.rep);
        f2_fold_tau(fq, L.tq);
        asm volatile("" : "+v"(fq[0]), "+v"(fq[1]));
    }
    float rc = L.rep, rn;
    f32x16 c0 = f2_block<1>(s[0], bq[0], fq[0]);      // prologue: the first tile's keys
    f32x16 c1 = f2_block<1>(s[0], bq[1], fq[1]);
    f32x16 n0, n1;
    float carry = kKnnSentinel;
#define F2_TRIP_CALL(Q, T) \
    f2_trip_call<M, UPD, REC, Q>(L, S, rec, rbase, T, t_hi, c0, c1, n0, n1, rc, rn, s, bq, fq, lane, hh, alive, carry, rofs)
    int t = t_lo;
    for (int n = f2_whole_trips(t_hi - t_lo); n > 0; --n, t += kF2Sets) {
        F2_TRIP_CALL(0, t);
        F2_TRIP_CALL(1, t + 1);
        F2_TRIP_CALL(2, t + 2);
        F2_TRIP_CALL(3, t + 3);
    }
    const int rem = f2_remainder_calls(t_hi - t_lo);
    if (rem > 0) {
        F2_TRIP_CALL(0, t);
        if (rem > 1) {
            F2_TRIP_CALL(1, t + 1);
            if (rem > 2) F2_TRIP_CALL(2, t + 2);
        }
    }
#undef F2_TRIP_CALL
}

// One pass over the tiles [t_lo, t_hi) of the event whose first record is rbase.
template <int M, bool UPD, bool REC, int NH = 1>
__device__ __forceinline__ void f2_sweep(F2Lane<M> &L, F2Wave &S, const uint8_t *__restrict__ rec, int64_t rbase,
                                         int t_lo, int t_hi, const f16x8 (&bq)[2][2 * NH], int lane, int hh, bool alive)
{
    if (t_lo >= t_hi) return;
#ifdef DMET_F2_DEFER_FOUR
    constexpr bool kFour = NH == 1;            // experiment: the deferred pass on four sets too (r10: slower in every run)
#else
    constexpr bool kFour = NH == 1 && REC;
#endif
    if constexpr (kFour) {
        f2_sweep4<M, UPD, REC>(L, S, rec, rbase, t_lo, t_hi, bq, lane, hh, alive);
        return;
    }
    // two operand sets (the deferred pass; 64 features: two sets of eight fragments next to the sixteen of the queries
    // are what fits): a cold start, and call t loads tile t + 2
    F2Ops<NH> A, B;
    unsigned rofs = (unsigned)lane * 16u;
    f2_load<NH>(A, rec, rbase + t_lo, lane, hh, rofs);
    // query side of the fold: threshold 0 (32 features: the deferred pass records no mask, its results are the keys
    // themselves; 64 features do not fold)
    f16x8 fq[2] = {f2_fold(0u), f2_fold(0u)};
    float rc = L.rep, rn;
    f32x16 c0 = f2_block<NH>(A, bq[0], fq[0]);      // prologue: the first tile's keys
    f32x16 c1 = f2_block<NH>(A, bq[1], fq[1]);
    f32x16 n0, n1;
    f2_load<NH>(A, rec, rbase + f2_load_tile(t_lo, 1, t_hi), lane, hh, rofs);
    float carry = kKnnSentinel;
    // every tile inserts its own minimum (INS = true).  Inserting the minimum of tile PAIRS instead (half the
    // v_med3 chains) was tried: the threshold then admits up to 2M tiles, more than the 26 entries a lane can keep
    // -> 3 761 overflowed queries per launch and twice the kernel time
    // the fold's threshold is converted after every second tile only (f2_tau16 is ~15 VALU ops): the masks of
    // the next two tiles are taken against a threshold older by one more update -- larger, a superset
    // (The same loop as whole pairs and an odd tile, without the exit between its two calls, was compiled in r10: its
    // waits still count down to vmcnt(0) -- with two sets the loads of the next use are the youngest in flight -- and
    // the 64-feature instances grow by 14 to 18 registers.  Not kept, not run.)
    for (int t = t_lo; t < t_hi; t += 2) {
        f2_tile<M, UPD, REC, true, NH, false>(L, S, rec, rbase, t, f2_load_tile(t, kF2PlainLead, t_hi), c0, c1, n0, n1, rc, rn,
                                              A, B, bq, fq, lane, hh, alive, carry, rofs);
        if (t + 1 < t_hi)
            f2_tile<M, UPD, REC, true, NH, true>(L, S, rec, rbase, t + 1, f2_load_tile(t + 1, kF2PlainLead, t_hi), n0, n1, c0,
                                                 c1, rn, rc, B, A, bq, fq, lane, hh, alive, carry, rofs);
    }
}

// Plan group of a workgroup.  Whole-sweep tiles: the workgroups of one XCD take one contiguous eighth of the tile list
// (see xcd_dealt_position); the split tail tiles that follow stay interleaved over the XCDs.
__device__ __forceinline__ int filter_group(const KnnFilterArgs &a)
{
    const int full_groups = a.plan->n_full / kWavesPerGroup;   // n_full is a multiple of the SIMD count
    return (int)blockIdx.x < full_groups ? xcd_swizzle((int)blockIdx.x, full_groups) : (int)blockIdx.x;
}

// One wavefront's item of the second form; S is the wavefront's own LDS (no workgroup barrier inside).
template <int KP, int NH = 1>
__device__ __forceinline__ void filter2_wave(const KnnFilterArgs &a, F2Wave &S, int *tickets, int group, int wv, int lane)
{
    constexpr int M = f2_list_len(KP);
    static_assert(f2_list_cap(M) == KP, "f2_running_tau reads slot KP - 1 of the list");
    constexpr int D = 32 * NH;
    constexpr int MS = (M + 1 + 3) & ~3;
    const int col = lane & 31, hh = lane >> 5;
    const uint8_t *__restrict__ rec = a.rec;
    const int64_t *__restrict__ ptr = a.ptr;

    const int n_full = a.plan->n_full, split = a.plan->split, total = a.plan->total_tiles;
    const int item = group * kWavesPerGroup + wv;
    int tile = item, sub = 0, nsub = 1;
    if (item >= n_full) {
        const int r = item - n_full;
        tile = n_full + r / split;
        sub = r % split;
        nsub = split;
    }
    if (tile >= total) return;
    const int pos = find_tile_event(a.tile_ptr, a.B, tile);
    const int ev = a.order[pos];
    const int ev_lo = (int)ptr[ev], ev_hi = (int)ptr[ev + 1];
    const int q_first = ev_lo + (tile - a.tile_ptr[pos]) * kFQ;
    if (!f2_in_domain(ev_hi - ev_lo)) {
        // the first form's events.  D = 64 has no first form: every query of such an event is handed to the exact
        // kernel (once per tile: a split tile comes by `split` times)
        if (NH != 1 && sub == 0) {
            const int q = q_first + lane;
            if (q < ev_hi) {
                flag_query(a, q, a.xtile_ptr[pos] + (q - ev_lo) / a.xtile_queries);
            }
        }
        return;
    }
    int clo = ev_lo, chi = ev_hi;
    if (nsub > 1) {
        if (ev_hi - ev_lo < kF2SplitMinNodes) {
            // a sub-sweep of fewer than ~2 M tiles has no threshold to speak of (it would hand most of its range to the
            // exact re-rank): the first piece takes the tile as a whole-sweep item -- rows written in place, second
            // attempt included, so a final threshold that was cut too tight has its safety net here as well -- and
            // the others have nothing to do (no list, no ticket: nobody merges)
            if (sub != 0) return;
            nsub = 1;
        } else {
            const int chunk = (((chi - clo) + nsub - 1) / nsub + 31) & ~31;
            clo = min(chi, clo + sub * chunk);
            chi = min(chi, clo + chunk);
        }
    }
    const int64_t rbase = (ptr[ev] >> 5) + ev;
    const int64_t rlast = rbase + (ev_hi - ev_lo - 1) / 32;
    const int t_lo = (clo - ev_lo) / 32, t_hi = (chi - ev_lo + 31) / 32;

    const int myq = q_first + hh * 32 + col;
    const bool valid = myq < ev_hi;
    // Second attempt (whole-sweep items only).  A query whose certificate fails by the slack alone -- enough candidates,
    // but the threshold T too close to its k-th distance: T + |x|^2 - slack <= d_k -- does not need the exact kernels:
    // the wavefront sweeps the event once more with the FIXED threshold T* = d_k - |x|^2 + slack for those lanes
    // (-inf, i.e. nothing recorded, for the others), re-ranks what that admits and certifies against T*: every candidate
    // dropped by that sweep has key >= T*, hence d >= d_k >= the new k-th distance.  With fp16 operands ~0.1 queries per
    // 4500-node event take this road (one wavefront in ~200 pays a second, masks-only sweep) instead of ~100 us of
    // per-query fallback per build.
    float t_fix = -__builtin_inff();
    bool act = valid;              // lanes whose result this attempt writes and certifies
    for (int attempt = 0;; ++attempt) {
    F2Lane<M> L;
#pragma unroll
    for (int p = 0; p < M; ++p) L.tk[p] = kKnnSentinel;
    L.tau = attempt == 0 ? -__builtin_inff() : t_fix;     // first attempt: nothing is recorded before tk is full
    L.margin = __builtin_inff();
    L.tq = 0u;
    L.rep = 0.0f;
    L.cnt = 0;
    L.overflow = false;
    {
        // the query operands live only as long as the sweeps (the re-rank needs the registers for the rows)
        f16x8 bq[2][2 * NH];      // -2 x the queries' fp16 fragments (exact: |h| <= 16384)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int64_t qrec = min(rbase + (q_first - ev_lo) / 32 + b, rlast);
            const f16x8 *g = reinterpret_cast<const f16x8 *>(rec + qrec * rec_bytes(NH));
#pragma unroll
            for (int m = 0; m < 2 * NH; ++m) bq[b][m] = g[m * 64 + lane] * (_Float16)-2.0f;
        }
        if (attempt == 0) {
            const int t_def = min(t_hi, t_lo + kF2Defer);
            f2_sweep<M, true, false, NH>(L, S, rec, rbase, t_lo, t_def, bq, lane, hh, valid);     // tau only
            // The running cut's margin (see f2_running_tau), from the list as the deferred pass left it; the main sweep
            // starts from the threshold it gives.  The norm is loaded here and again at the final cut: one more load
            // per item, no register held across the main sweep.
            if (a.run_cut && a.cut_scale >= 0.0f && a.k == KP && t_def < t_hi) {
                const float tkk = L.tk[KP - 1];
                int qi = valid ? myq : ev_lo;
                asm volatile("" : "+v"(qi));
                const float m = f2_cut<NH>(tkk, a.nrm[qi], a.cut_scale) - tkk;
                // (a NaN fails both comparisons; a zero margin, DMET_KNN_CUT=0.0, leaves the running cut off: see above)
                if (tkk < kKnnSentinel && m > 0.0f && m < __builtin_inff()) L.margin = __builtin_fmaf(m, 0.01f, m);
                L.tau = fminf(L.tau, tkk + L.margin);
            }
            f2_sweep<M, true, true, NH>(L, S, rec, rbase, t_def, t_hi, bq, lane, hh, valid);
            // The final threshold: tk[M-1], or the cut above tk[k-1] where that is lower (f2_cut).  The revisit below,
            // the compaction, the re-rank and the certificate all see the threshold that is applied here.  Lanes whose
            // list holds fewer than k minima keep tk[M-1]; idle and overflowed lanes stay at -inf.
            if (a.cut_scale >= 0.0f) {
                float tkk = kKnnSentinel;
#pragma unroll
                for (int p = 0; p < KP; ++p)
                    if (p == a.k - 1) tkk = L.tk[p];
                if (tkk < kKnnSentinel) {
                    int qi = valid ? myq : ev_lo;
                    asm volatile("" : "+v"(qi));   // (the address is formed here, not carried through the sweeps)
                    const float cut = f2_cut<NH>(tkk, a.nrm[qi], a.cut_scale);
                    L.tau = fminf(L.tau, cut);
                }
            }
            f2_sweep<M, false, true, NH>(L, S, rec, rbase, t_lo, t_def, bq, lane, hh, valid);     // against the final tau
        } else {
            f2_sweep<M, false, true, NH>(L, S, rec, rbase, t_lo, t_hi, bq, lane, hh, valid);      // against T*
        }
    }
    f2_compact<M>(L, S, lane, kF2Slots);
#if defined(DMET_F2_ABL) && DMET_F2_ABL >= 1
    return;
#endif

    // ---- exact re-rank of the set bits (R1 chain, top-k by (d, j)), candidates fetched cooperatively ----------------
    const int64_t qrow_id = valid ? myq : ev_lo;
    float qrow[D];
    {
        const float4 *g = reinterpret_cast<const float4 *>(a.x + qrow_id * D);
#pragma unroll
        for (int c = 0; c < D / 4; ++c) {
            const float4 v = g[c];
            qrow[4 * c] = v.x; qrow[4 * c + 1] = v.y; qrow[4 * c + 2] = v.z; qrow[4 * c + 3] = v.w;
        }
    }
    // sorted top-KP as 64-bit words (distance bits << 32 | j): distances are >= +0, so the unsigned order IS the (d, j)
    // order of R2 -- and, the words read as doubles, the f64 order: the insertion is one v_min_f64 + one v_max_f64 per
    // slot (knn_key64.h), no condition registers and no branches.  Empty slots are (sentinel, 0): a candidate at exactly
    // the sentinel distance (or NaN / inf: clamped to the sentinel by key64_word) is never inserted, like the oracle's
    // strict '>'.
    static_assert(__builtin_bit_cast(unsigned, kKnnSentinel) == kKey64SentinelBits, "knn_key64.h clamps to the sentinel");
    double kk[KP];
#pragma unroll
    for (int p = 0; p < KP; ++p) kk[p] = key64_as_double(kKey64Empty);
    const int nent = (act && !L.overflow) ? L.cnt : 0;
    int slot = 0;
    unsigned cmask = 0u;
    int ctile = 0;
    // The lane's next entry is read one call ahead, unconditionally (slot clamped to the last one: the value is not used
    // then), and swapped in when the mask runs out: no exec-masked branch around an LDS read and no wait directly behind
    // it inside a round.
    uint2 enext = S.ent[0][lane];
    // next candidate of this lane (tiles as appended, mask order inside a tile) as its row number INSIDE the event
    // (< ev_hi - ev_lo <= 65536: rows past the event's end have key = +inf and are never set), -1 when exhausted
    auto pop = [&]() __attribute__((always_inline)) -> int32_t {
        const bool take = cmask == 0u && slot < nent;
        cmask = take ? enext.x : cmask;
        ctile = take ? (int)(enext.y & kF2TileMask) : ctile;
        slot += take ? 1 : 0;
        enext = S.ent[min(slot, kF2Slots - 1)][lane];
        int32_t jl = -1;
        if (cmask != 0u) {
            const int r = __builtin_clz(cmask);
            cmask &= ~(0x80000000u >> r);
            jl = ctile * 32 + f2_mask_row(r);
        }
        return jl;
    };
    const float4 *x4 = reinterpret_cast<const float4 *>(a.x);
#ifdef DMET_RR_PRIO
    __builtin_amdgcn_s_setprio(DMET_RR_PRIO);   // experiment: the latency-bound phase issues ahead of the other wavefront's sweep
#endif
    if constexpr (NH != 1) {
        // D = 64: every lane fetches the row of its own candidate (sixteen 16-byte loads in flight) and runs the chain
        // on it -- none of the cooperative staging of the 32-wide form below, whose register budget (three rounds of
        // half rows in flight) does not carry over; the sweep, not this loop, is the larger part at this width
        for (;;) {
            const int32_t jl = pop();
            if (!__any(jl >= 0)) break;
            const int32_t j = ev_lo + jl;
            const float4 *row = x4 + (int64_t)(jl >= 0 ? j : ev_lo) * (D / 4);
            float4 v[D / 4];
#pragma unroll
            for (int c = 0; c < D / 4; ++c) v[c] = row[c];
            float dc = 0.0f;
#pragma unroll
            for (int c = 0; c < D / 4; ++c) {
                float df;
                df = v[c].x - qrow[4 * c + 0]; dc = __builtin_fmaf(df, df, dc);
                df = v[c].y - qrow[4 * c + 1]; dc = __builtin_fmaf(df, df, dc);
                df = v[c].z - qrow[4 * c + 2]; dc = __builtin_fmaf(df, df, dc);
                df = v[c].w - qrow[4 * c + 3]; dc = __builtin_fmaf(df, df, dc);
            }
            key64_insert<KP>(kk, key64_word(__float_as_uint(dc), (unsigned)j, jl >= 0));
        }
    } else {
    // rows are fetched half a row at a time (16 features = 64 bytes): load instruction 4 h + r brings half h of rows
    // 16 r + (lane >> 2), 16 bytes per lane; exhausted lanes re-read the event's first row (no branches, result unused)
    struct HalfRows { float4 v0, v1, v2, v3, v4, v5, v6, v7; };   // named members: stays in registers
#ifdef DMET_RR_FULLROW
    // experiment: one load instruction brings 8 WHOLE rows (8 lanes x 16 bytes = one 128-byte line per row) instead of 16
    // half rows -- half the line look-ups per round
    auto fetch = [&](int32_t jl) __attribute__((always_inline)) -> HalfRows {
        const int32_t jc = ev_lo + (jl >= 0 ? jl : 0);
        const int64_t o = lane & 7;
        const int sub = lane >> 3;
        HalfRows R;
        R.v0 = x4[(int64_t)__shfl(jc, 0 + sub, 64) * 8 + o];
        R.v1 = x4[(int64_t)__shfl(jc, 8 + sub, 64) * 8 + o];
        R.v2 = x4[(int64_t)__shfl(jc, 16 + sub, 64) * 8 + o];
        R.v3 = x4[(int64_t)__shfl(jc, 24 + sub, 64) * 8 + o];
        R.v4 = x4[(int64_t)__shfl(jc, 32 + sub, 64) * 8 + o];
        R.v5 = x4[(int64_t)__shfl(jc, 40 + sub, 64) * 8 + o];
        R.v6 = x4[(int64_t)__shfl(jc, 48 + sub, 64) * 8 + o];
        R.v7 = x4[(int64_t)__shfl(jc, 56 + sub, 64) * 8 + o];
        return R;
    };
#else
    // The rows of an item all lie in its event: the event's first row is a scalar base (readfirstlane of both halves,
    // as f2_load does for the records) and a half row is global_load_dwordx4 v, v_off, s[base:base+1] offset:0 / 64 with
    // the 32-bit offset 128 x (row inside the event) + 16 x (lane & 3), below 2^23 -- no sign extension and no 64-bit
    // vector arithmetic per row
    const uint64_t xb = reinterpret_cast<uint64_t>(a.x + (int64_t)ev_lo * D);
    const uint64_t xbs = ((uint64_t)(unsigned)__builtin_amdgcn_readfirstlane((int)(xb >> 32)) << 32) |
                         (unsigned)__builtin_amdgcn_readfirstlane((int)xb);
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    typedef const f32x4 __attribute__((address_space(1))) *GlobalRow;
    auto ld = [](GlobalRow g, int i) __attribute__((always_inline)) -> float4 {
        const f32x4 v = g[i];
        return make_float4(v.x, v.y, v.z, v.w);
    };
    auto fetch = [&](int32_t jl) __attribute__((always_inline)) -> HalfRows {
        const int32_t jc = jl >= 0 ? jl : 0;
        const unsigned o = 16u * (lane & 3);
        const GlobalRow r0 = (GlobalRow)(xbs + (uint64_t)(((unsigned)__shfl(jc, 0 + (lane >> 2), 64) << 7) + o));
        const GlobalRow r1 = (GlobalRow)(xbs + (uint64_t)(((unsigned)__shfl(jc, 16 + (lane >> 2), 64) << 7) + o));
        const GlobalRow r2 = (GlobalRow)(xbs + (uint64_t)(((unsigned)__shfl(jc, 32 + (lane >> 2), 64) << 7) + o));
        const GlobalRow r3 = (GlobalRow)(xbs + (uint64_t)(((unsigned)__shfl(jc, 48 + (lane >> 2), 64) << 7) + o));
        HalfRows R;
        R.v0 = ld(r0, 0); R.v1 = ld(r1, 0); R.v2 = ld(r2, 0); R.v3 = ld(r3, 0);
        R.v4 = ld(r0, 4); R.v5 = ld(r1, 4); R.v6 = ld(r2, 4); R.v7 = ld(r3, 4);
        return R;
    };
#endif
    auto chain16 = [&](float dc, int h) __attribute__((always_inline)) -> float {
#pragma unroll
        for (int c4 = 0; c4 < 4; ++c4) {
            const float4 v = *reinterpret_cast<const float4 *>(&S.rows[lane][4 * c4]);
            const int f0 = 16 * h + 4 * c4;
            float df;
            df = v.x - qrow[f0 + 0]; dc = __builtin_fmaf(df, df, dc);
            df = v.y - qrow[f0 + 1]; dc = __builtin_fmaf(df, df, dc);
            df = v.z - qrow[f0 + 2]; dc = __builtin_fmaf(df, df, dc);
            df = v.w - qrow[f0 + 3]; dc = __builtin_fmaf(df, df, dc);
        }
        return dc;
    };
    auto round = [&](const HalfRows &R, int32_t jl) __attribute__((always_inline)) {
#ifdef DMET_RR_FULLROW
        float4 *dst = reinterpret_cast<float4 *>(&S.rows[lane >> 3][4 * (lane & 3)]);   // + 8 r rows per register
        constexpr int kS8 = 8 * (kF2RowF + 4) / 4;                                        // float4s per 8 rows
        const bool lowhalf = (lane & 4) == 0;
        wave_sync();
        if (lowhalf) {
            dst[0] = R.v0; dst[kS8] = R.v1; dst[2 * kS8] = R.v2; dst[3 * kS8] = R.v3;
            dst[4 * kS8] = R.v4; dst[5 * kS8] = R.v5; dst[6 * kS8] = R.v6; dst[7 * kS8] = R.v7;
        }
        wave_sync();
        float dc = chain16(0.0f, 0);
        wave_sync();
        if (!lowhalf) {
            dst[0] = R.v0; dst[kS8] = R.v1; dst[2 * kS8] = R.v2; dst[3 * kS8] = R.v3;
            dst[4 * kS8] = R.v4; dst[5 * kS8] = R.v5; dst[6 * kS8] = R.v6; dst[7 * kS8] = R.v7;
        }
        wave_sync();
        dc = chain16(dc, 1);
#else
        float4 *dst = reinterpret_cast<float4 *>(&S.rows[lane >> 2][4 * (lane & 3)]);   // + 16 r rows per register
        constexpr int kStride = 16 * (kF2RowF + 4) / 4;                                    // float4s per 16 rows
        wave_sync();
        dst[0] = R.v0; dst[kStride] = R.v1; dst[2 * kStride] = R.v2; dst[3 * kStride] = R.v3;
        wave_sync();
        float dc = chain16(0.0f, 0);
        wave_sync();
        dst[0] = R.v4; dst[kStride] = R.v5; dst[2 * kStride] = R.v6; dst[3 * kStride] = R.v7;
        wave_sync();
        dc = chain16(dc, 1);
#endif
        key64_insert<KP>(kk, key64_word(__float_as_uint(dc), (unsigned)(ev_lo + jl), jl >= 0));   // the list keeps global ids
    };
    // Rounds of rows in flight: three (KP <= 16) were chosen in round 2 -- the kernel has since grown to 256 VGPRs + 56
    // bytes of scratch per lane with them (-Rpass-analysis=kernel-resource-usage), i.e. spill traffic inside this
    // latency-bound loop; with two it needs 237 registers and no scratch and the build is 8-10 us faster (second session
    // of round 3).  Measured again with the registers the opaque copies below freed (224 VGPRs at k = 16, no scratch,
    // profiles/r06_knn_operands.md): still slower, 48 213 against 48 519 events/s, every one of six runs below every run
    // with two rounds.  With the f64 insertion (knn_key64.h) the third round no longer fits at k = 16: 256 VGPRs + 140
    // bytes of scratch (profiles/r07_knn_rerank.md has the timing).  DMET_RR_THREE brings the third back for A/B
#ifdef DMET_RR_THREE
    constexpr bool kThreeRounds = KP <= 16;
#else
    constexpr bool kThreeRounds = false;
#endif
    if constexpr (kThreeRounds) {
        // three rounds of rows in flight: the loop is bound by the gathers' latency
        int32_t ja = pop(), jb, jc;
        HalfRows pa = fetch(ja), pb, pc;
        jb = pop();
        pb = fetch(jb);
        for (;;) {
            if (!__any(ja >= 0)) break;
            jc = pop(); pc = fetch(jc);
            round(pa, ja);
            if (!__any(jb >= 0)) break;
            ja = pop(); pa = fetch(ja);
            round(pb, jb);
            if (!__any(jc >= 0)) break;
            jb = pop(); pb = fetch(jb);
            round(pc, jc);
        }
    } else {
        // the 20-wide list leaves registers for two rounds in flight
        int32_t ja = pop(), jb;
        HalfRows pa = fetch(ja), pb;
        for (;;) {
            if (!__any(ja >= 0)) break;
            jb = pop(); pb = fetch(jb);
            round(pa, ja);
            if (!__any(jb >= 0)) break;
            ja = pop(); pa = fetch(ja);
            round(pb, jb);
        }
    }
    }
#ifdef DMET_RR_PRIO
    __builtin_amdgcn_s_setprio(0);
#endif
    float kd[KP];
    int32_t kj[KP];
#pragma unroll
    for (int p = 0; p < KP; ++p) {
        kd[p] = __uint_as_float((unsigned)(key64_as_word(kk[p]) >> 32));
        kj[p] = kd[p] == kKnnSentinel ? -1 : (int32_t)(unsigned)key64_as_word(kk[p]);
    }
    // Everything below addresses global memory and LDS by the lane and by the query.  Formed from `lane` and `myq` those
    // addresses are invariant in the attempt loop: the compiler computes them at the top of the kernel and carries them
    // through the sweeps, a dozen register pairs (the 64-feature instances spilled them).  Opaque copies keep them here.
    // What must go through the copies: every per-lane ADDRESS of this section -- the staging area (stg + elane ...), the
    // rows of nbr / dist / nbr16, nrm[eq], qflag / flag_query(eq).  Predicates and uniform values (valid, act, col, hh,
    // fslot) may keep the originals: they are a register or a mask each and were live anyway.  This only steers the
    // register allocation, never the result; the figures it buys are in profiles/r05_knn_cut.md and have to be read
    // again (-Rpass-analysis=kernel-resource-usage) when the compiler changes.
    // Every instance: at 64 features the carried addresses spilled; at 32 the sweep holds its two fold operands in
    // registers (f2_sweep) and only fits beside them without these pairs (at k = 16: 256 VGPRs + 20 bytes of scratch
    // against 223).
    int elane = lane, eq = myq;
    asm volatile("" : "+v"(elane), "+v"(eq));
    const int k = a.k;
    // the threshold that was applied: tk[M-1] or the cut (first attempt), t_fix (second).  -inf: an overflowed lane, which
    // fails whatever it is compared with, or a lane without a query
    const float tau = L.tau;
    // the query's rows of the three tables; returns its k-th distance (-1: fewer than k neighbours)
    // coop (whole-sweep items, called by ALL lanes): the 64 queries of the item own 64 consecutive rows of each table, i.e.
    // one contiguous block; written by the lanes themselves that is k 4-byte stores per lane and table, each instruction a
    // 4-byte piece of 64 different lines (switching the stores off measured 22 of the build's 420 us).  The rows go through
    // the wavefront's LDS (free by now) instead and leave as 16-byte pieces of consecutive addresses; rows_on masks the
    // rows that are written (lanes past the event's end; the second attempt rewrites only its own queries).
    auto emit = [&](const bool rows_on, const bool coop) __attribute__((always_inline)) -> float {
        float kth = -1.0f;
#pragma unroll
        for (int p = 0; p < KP; ++p)
            if (p == k - 1 && kj[p] >= 0) kth = kd[p];
        if constexpr (KP % 4 == 0 && KP <= 20) {
            if (coop && a.emit_coalesced && k == KP) {
                constexpr int RP = KP / 4;       // 16-byte pieces per row
                const unsigned long long on = __ballot(rows_on);
                unsigned *stg = reinterpret_cast<unsigned *>(&S);        // 64 rows x KP words <= 5 120 bytes per table
                const int64_t blk = (int64_t)q_first * KP;               // first word of the block in nbr / dist
                wave_sync();
#pragma unroll
                for (int q = 0; q < RP; ++q)
                    *reinterpret_cast<uint4 *>(stg + elane * KP + 4 * q) =
                        make_uint4((unsigned)kj[4 * q], (unsigned)kj[4 * q + 1], (unsigned)kj[4 * q + 2], (unsigned)kj[4 * q + 3]);
                wave_sync();
#pragma unroll
                for (int t = 0; t < RP; ++t) {
                    const int pi = t * 64 + elane;
                    const uint4 v = *reinterpret_cast<const uint4 *>(stg + 4 * pi);
                    if ((on >> (pi / RP)) & 1ull) *reinterpret_cast<uint4 *>(a.nbr + blk + 4 * pi) = v;
                }
                wave_sync();
#pragma unroll
                for (int q = 0; q < RP; ++q)
                    *reinterpret_cast<uint4 *>(stg + elane * KP + 4 * q) =
                        make_uint4(__float_as_uint(kd[4 * q]), __float_as_uint(kd[4 * q + 1]), __float_as_uint(kd[4 * q + 2]),
                                   __float_as_uint(kd[4 * q + 3]));
                wave_sync();
#pragma unroll
                for (int t = 0; t < RP; ++t) {
                    const int pi = t * 64 + elane;
                    const uint4 v = *reinterpret_cast<const uint4 *>(stg + 4 * pi);
                    if ((on >> (pi / RP)) & 1ull) *reinterpret_cast<uint4 *>(a.dist + blk + 4 * pi) = v;
                }
                if (a.nbr16) {
                    if constexpr (KP % 8 == 0) {
                        constexpr int RH = KP / 8;   // 16-byte pieces per uint16 row
                        wave_sync();
#pragma unroll
                        for (int q = 0; q < RH; ++q) {
                            uint4 w;
                            w.x = (unsigned)local_id16(kj[8 * q], ev_lo) | ((unsigned)local_id16(kj[8 * q + 1], ev_lo) << 16);
                            w.y = (unsigned)local_id16(kj[8 * q + 2], ev_lo) | ((unsigned)local_id16(kj[8 * q + 3], ev_lo) << 16);
                            w.z = (unsigned)local_id16(kj[8 * q + 4], ev_lo) | ((unsigned)local_id16(kj[8 * q + 5], ev_lo) << 16);
                            w.w = (unsigned)local_id16(kj[8 * q + 6], ev_lo) | ((unsigned)local_id16(kj[8 * q + 7], ev_lo) << 16);
                            *reinterpret_cast<uint4 *>(stg + elane * (KP / 2) + 4 * q) = w;
                        }
                        wave_sync();
#pragma unroll
                        for (int t = 0; t < RH; ++t) {
                            const int pi = t * 64 + elane;
                            const uint4 v = *reinterpret_cast<const uint4 *>(stg + 4 * pi);
                            if ((on >> (pi / RH)) & 1ull)
                                *reinterpret_cast<uint4 *>(reinterpret_cast<unsigned *>(a.nbr16 + blk) + 4 * pi) = v;
                        }
                    } else if (rows_on) {
                        uint16_t *r16 = a.nbr16 + (int64_t)eq * k;
#pragma unroll
                        for (int p = 0; p + 1 < KP; p += 2)
                            reinterpret_cast<unsigned *>(r16)[p >> 1] =
                                (unsigned)local_id16(kj[p], ev_lo) | ((unsigned)local_id16(kj[p + 1], ev_lo) << 16);
                    }
                }
                wave_sync();       // the staging area is the next attempt's entry list
                return kth;
            }
        }
        if (!rows_on) return kth;
#pragma unroll
        for (int p = 0; p < KP; ++p) {
            if (p < k) {
                a.nbr[(int64_t)eq * k + p] = kj[p];
                a.dist[(int64_t)eq * k + p] = kd[p];
            }
        }
        if (a.nbr16) {
            uint16_t *r16 = a.nbr16 + (int64_t)eq * k;
            if ((k & 1) == 0) {   // two ids per dword store
#pragma unroll
                for (int p = 0; p + 1 < KP; p += 2)
                    if (p < k)
                        reinterpret_cast<unsigned *>(r16)[p >> 1] =
                            (unsigned)local_id16(kj[p], ev_lo) | ((unsigned)local_id16(kj[p + 1], ev_lo) << 16);
            } else {
#pragma unroll
                for (int p = 0; p < KP; ++p)
                    if (p < k) r16[p] = local_id16(kj[p], ev_lo);
            }
        }
        return kth;
    };
    if (nsub == 1) {
        bool retry = false;
        const float kth = emit(act, true);
        if (act) {
            // certificate: every dropped candidate had key >= tau (see the header of this form).  Candidates were
            // dropped (tau below the sentinel) but fewer than k neighbours came back (kth < 0): not certified either
            const float nx = a.nrm[eq];
            const float an = __builtin_sqrtf(nx) * 1.000001f;
            const float rn = an + __builtin_sqrtf(fmaxf(kth, 0.0f)) * 1.00002f;
            const float slack = f2_slack(an, rn, NH == 1 ? 1.0f : 1.5f);
            // a query whose own row is outside the fp16 range (or not finite) swept with zero operands: never certified.
            // Every lane is checked, also one whose tau stayed at the sentinel: the fold drops keys above
            // kF2TauRepMax whatever tau is (f2_cert_T)
            const bool wideq = !(nx < kF16WideLimit * kF16WideLimit);
            const bool fail = L.overflow || wideq || (f2_full<NH>(tau) && !(kth >= 0.0f && f2_cert_T<NH>(tau) + nx - slack > kth));
            // slack-only failures (and cuts that came out too tight) get the second attempt: the smallest threshold
            // that certifies this k-th distance
            const float ts = f2_cert_threshold<NH>(kth, nx, slack);
            retry = fail && attempt == 0 && !L.overflow && !wideq && kth >= 0.0f && f2_cert_T<NH>(ts) + nx - slack > kth &&
                    ts < kKnnSentinel;
            if (fail && !retry) {
                flag_query(a, eq, a.xtile_ptr[pos] + (eq - ev_lo) / a.xtile_queries);
#ifdef DMET_KNN_WHY
                a.qflag[eq] = (uint8_t)(1 | (L.overflow ? 2 : 0) | (wideq ? 4 : 0) | (kth < 0.0f ? 8 : 0) | (attempt ? 16 : 0) |
                                         (!(ts < kKnnSentinel) ? 32 : 0) | (!(f2_cert_T<NH>(ts) + nx - slack > kth) ? 64 : 0));
                a.dist[(int64_t)eq * k + 0] = tau; a.dist[(int64_t)eq * k + 1] = kth; a.dist[(int64_t)eq * k + 2] = slack; a.dist[(int64_t)eq * k + 3] = (float)L.cnt;
#endif
            }
            t_fix = retry ? ts : -__builtin_inff();
        }
        if (!__any(retry)) return;
        const int nretry = __popcll(__ballot(retry));
        if (elane == 0) {   // diagnostics (dmet_knn_retry_stats): a retrying lane costs its whole wavefront a sweep
            atomicAdd(a.retries, 1);
            atomicAdd(a.retries + 1, nretry);
        }
        act = retry;
        continue;
    }
    // ---- split (tail) items: the exact top-KP of this candidate range + its threshold go to global memory; the two
    // sub-sweeps of a tile are neighbouring wavefronts of ONE workgroup (items 4g + {0,1} and 4g + {2,3}: n_full is a
    // multiple of 4 and the split is 2), and the one that finishes second merges the other's list into its own and
    // certifies against both thresholds -- a ticket in LDS and workgroup-scope fences, no launch of its own (the
    // separate merge kernel took 17 us per build behind the whole filter grid).
    static_assert(kFilterMaxSplit == 2 && kWavesPerGroup % 2 == 0, "pairs of sub-sweeps share a workgroup");
    const int64_t fslot = (int64_t)(tile - n_full) * kFQ + hh * 32 + col;
    if (valid) {
        float *ld = a.psd + (fslot * nsub + sub) * MS;
        int32_t *lj = a.psj + (fslot * nsub + sub) * MS;
#pragma unroll
        for (int p = 0; p < KP; ++p) { ld[p] = kd[p]; lj[p] = kj[p]; }
        ld[M] = tau;
        lj[M] = L.overflow ? 1 : 0;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    int arrived = 0;
    if (elane == 0) arrived = atomicAdd(&tickets[wv >> 1], 1);
    arrived = __builtin_amdgcn_readfirstlane(arrived);
    if (arrived == 0) return;                 // the other sub-sweep of this tile is still running: it will merge
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    float tau_o = kKnnSentinel;
    int of_o = 0;
    if (valid) {
        const float *ld = a.psd + (fslot * nsub + (sub ^ 1)) * MS;
        const int32_t *lj = a.psj + (fslot * nsub + (sub ^ 1)) * MS;
        tau_o = ld[M];
        of_o = lj[M];
#pragma unroll
        for (int p = 0; p < KP; ++p) {
            const float od = ld[p];
            const int32_t oj = lj[p];
            // (d, j) pairs of the two candidate ranges are distinct; empty slots are never inserted
            key64_insert<KP>(kk, key64_word(__float_as_uint(od), (unsigned)oj, oj >= 0));
        }
#pragma unroll
        for (int p = 0; p < KP; ++p) {
            kd[p] = __uint_as_float((unsigned)(key64_as_word(kk[p]) >> 32));
            kj[p] = kd[p] == kKnnSentinel ? -1 : (int32_t)(unsigned)key64_as_word(kk[p]);
        }
        const float kth = emit(true, false);      // (inside a divergent branch: every lane writes its own rows)
        const float nx = a.nrm[eq];
        const float an = __builtin_sqrtf(nx) * 1.000001f;
        const float rn = an + __builtin_sqrtf(fmaxf(kth, 0.0f)) * 1.00002f;
        const float slack = f2_slack(an, rn, NH == 1 ? 1.0f : 1.5f);
        const bool wideq = !(nx < kF16WideLimit * kF16WideLimit);
        const bool fail_a = f2_full<NH>(tau) && !(kth >= 0.0f && f2_cert_T<NH>(tau) + nx - slack > kth);
        const bool fail_b = f2_full<NH>(tau_o) && !(kth >= 0.0f && f2_cert_T<NH>(tau_o) + nx - slack > kth);
        if (L.overflow || of_o != 0 || wideq || fail_a || fail_b)
            flag_query(a, eq, a.xtile_ptr[pos] + (eq - ev_lo) / a.xtile_queries);
    }
    return;
    }   // attempts
}

// Both forms in ONE launch: a wavefront takes the form its item's event calls for.  Batches that mix event sizes
// (configs[4]: 500-8000 nodes) used to pay a second, nearly empty launch for their events below kF2MinNodes -- a few
// hundred long serial items on an otherwise idle chip (216 us at 64 events) -- which now run beside the second form's
// items.  The wavefront number is wave-uniform, but only readfirstlane tells the compiler: without it the tile, the
// event, the loop counters and every record address are computed per lane on the vector ALU.
template <int KP, int NH = 1>
__global__ __launch_bounds__(kWave * kWavesPerGroup, kF2WavesPerSimd) void knn_filter12_kernel(const KnnFilterArgs a)
{
    union WaveLds {
        F2Wave f2;
#ifndef DMET_F2_LEAN
        FilterQueue<filter_queue_len(filter_list_len(KP))> f1;
#endif
    };
    __shared__ WaveLds sh_all[kWavesPerGroup];
    if constexpr (NH == 1) {
        // rider workgroups (behind every filter workgroup of the grid: dispatched last, into the slots of the last round)
        if (a.rP != nullptr && (int)blockIdx.x >= a.first_rider) {
            static_assert(sizeof(WaveLds) >= sizeof(float) * kNlsLdsFloats, "a wavefront's LDS holds the transposition tiles");
            const int rwv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
            const int64_t wave = (int64_t)((int)blockIdx.x - a.first_rider) * kWavesPerGroup + rwv;
            const int64_t nwaves = (int64_t)((int)gridDim.x - a.first_rider) * kWavesPerGroup;
            float *tp = reinterpret_cast<float *>(&sh_all[rwv]);
            if (a.r_sliced == 2)
                node_linear_split_bf16_wave<32, 32>(a.x, a.N, a.rW, a.rb, a.rP, reinterpret_cast<unsigned short *>(a.rQ), wave,
                                                    nwaves, threadIdx.x & 63);
            else if (a.r_sliced == 1) node_linear_split_wave<32, 32, true>(a.x, a.N, a.rW, a.rb, a.rP, a.rQ, tp, wave, nwaves, threadIdx.x & 63);
            else node_linear_split_wave<32, 32, false>(a.x, a.N, a.rW, a.rb, a.rP, a.rQ, tp, wave, nwaves, threadIdx.x & 63);
            return;
        }
    }
    // arrival tickets of the sub-sweep pairs of split tiles: 4 x 20 480 bytes fill half the CU's LDS exactly, so they
    // live in the last two padding floats of wavefront 0's row staging area (bytes 20 472..20 479 of its block), which
    // neither the staging (features 0..15 of a row) nor the first form's queue (at most 19 968 bytes) ever touches;
    // cleared here, before any wavefront of the group can arrive
    static_assert(sizeof(WaveLds) == sizeof(F2Wave), "the union is sized by the second form");
#ifndef DMET_F2_LEAN
    static_assert(sizeof(FilterQueue<filter_queue_len(filter_list_len(KP))>) <= sizeof(F2Wave) - 8, "ticket bytes are free");
#endif
    static_assert(kWavesPerGroup / 2 <= 2, "two ticket words");
    int *tickets = reinterpret_cast<int *>(&sh_all[0].f2.rows[kF2StageRows - 1][kF2RowF + 2]);
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (threadIdx.x < kWavesPerGroup / 2) tickets[threadIdx.x] = 0;
    __syncthreads();
    const int group = filter_group(a);
    filter2_wave<KP, NH>(a, sh_all[wv].f2, tickets, group, wv, lane);   // returns at once unless the item's event is a second-form event
#ifndef DMET_F2_LEAN
    if constexpr (NH == 1) filter1_wave<KP>(a, sh_all[wv].f1, group, wv, lane);   // likewise (32 features only)
#endif
}

// Exact R1 chain for the kept candidates of one query, top-k by (d, j), certification.  M lanes per query (one kept
// candidate each; split tiles take a second round), 64 / M queries per wavefront; workgroups of one XCD walk one
// contiguous range of queries so the candidate rows they gather stay in that XCD's L2.
template <int KP>
__global__ __launch_bounds__(256) void knn_rerank_kernel(const KnnFilterArgs a)
{
    constexpr int M = filter_list_len(KP);
    constexpr int MS = (M + 1 + 3) & ~3;
    constexpr int QPW = kWave / M;                       // queries per wavefront (3 for M = 20)
    constexpr int QPB = 4 * QPW;                         // per workgroup
    constexpr int EMAX = kFilterMaxSplit * M;            // entries per query at most
    __shared__ float sc[QPB][EMAX];
    __shared__ int32_t sj[QPB][EMAX];
    __shared__ float skth[QPB];
    __shared__ int sfail[QPB];
    __shared__ float qbuf[QPB][32];
    constexpr int PARTS = (kFQ + QPB - 1) / QPB;         // workgroups per 64-query filter tile
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int qw = lane / M, l = lane - qw * M;          // query slot of the wavefront, lane within the query
    const int slot = wv * QPW + min(qw, QPW - 1);
    // workgroup -> (filter tile, part): the event lookup is per workgroup (wave-uniform: scalar loads), not per lane
    // no XCD remap here: the grid is a worst-case bound and the live tiles are its first few hundred workgroups,
    // which the round-robin dispatch already spreads over all XCDs
    const int bid = blockIdx.x;
    if (a.form2 && a.plan->form1_events == 0) return;
    const int n_full = a.plan->n_full, split = a.plan->split;
    const int ft = n_full + bid / PARTS, part = bid % PARTS;   // only the split (tail) tiles come here
    if (ft >= a.plan->total_tiles) return;
    const int pos = find_tile_event(a.tile_ptr, a.B, ft);
    const int ev = a.order[pos];
    const int64_t ev_lo = a.ptr[ev], ev_hi = a.ptr[ev + 1];
    if (a.form2 && f2_in_domain((int)(ev_hi - ev_lo))) return;   // merged inside the filter kernel
    const int qoff = part * QPB + wv * QPW + qw;         // query within the tile
    const int64_t q = ev_lo + (int64_t)(ft - a.tile_ptr[pos]) * kFQ + qoff;
    const bool active = qw < QPW && qoff < kFQ && q < ev_hi;
    const int64_t qq = active ? q : ev_lo;
    const int nsub = split;
    const int64_t fslot = (int64_t)(ft - n_full) * kFQ + (active ? qoff : 0);
    const float *bd = a.psd + fslot * nsub * MS;
    const int32_t *bj = a.psj + fslot * nsub * MS;
    const int E = nsub * M;

    // issue every independent load up front: the kernel is bound by its chain of dependent memory round trips
    int32_t myj[kFilterMaxSplit];
#pragma unroll
    for (int t = 0; t < kFilterMaxSplit; ++t) myj[t] = (active && t < nsub) ? bj[t * MS + l] : -1;
    float vtau = kKnnSentinel, vnx = 0.0f;
    bool voverflow = false;
    if (active && l < nsub) { vtau = bd[l * MS + M]; voverflow = bj[l * MS + M] != 0; vnx = a.nrm[qq]; }
    // the wavefront's query rows go through LDS (read back as broadcasts): 32 fewer VGPRs, twice the resident waves
    if (lane < QPW * 8) {
        const int w = lane >> 3;
        const int64_t qrow_id = min(ev_lo + (int64_t)(ft - a.tile_ptr[pos]) * kFQ + part * QPB + wv * QPW + w, ev_hi - 1);
        *reinterpret_cast<float4 *>(&qbuf[wv * QPW + w][4 * (lane & 7)]) =
            reinterpret_cast<const float4 *>(a.x + qrow_id * 32)[lane & 7];
    }
    float myc[kFilterMaxSplit];
    wave_sync();
#pragma unroll 1
    for (int t = 0; t < kFilterMaxSplit; ++t) {
        float ct = kKnnSentinel;
        int32_t j = (t == 0) ? myj[0] : myj[kFilterMaxSplit - 1];
        if (active && t < nsub) {
            const int idx = t * M + l;
            if (j >= 0) {
                const float4 *g = reinterpret_cast<const float4 *>(a.x + (int64_t)j * 32);
                float4 crow[8];
#pragma unroll
                for (int c = 0; c < 8; ++c) crow[c] = g[c];
                float acc = 0.0f;
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    const float4 v = crow[c];
                    const float4 qv = *reinterpret_cast<const float4 *>(&qbuf[slot][4 * c]);
                    float df;
                    df = v.x - qv.x; acc = __builtin_fmaf(df, df, acc);
                    df = v.y - qv.y; acc = __builtin_fmaf(df, df, acc);
                    df = v.z - qv.z; acc = __builtin_fmaf(df, df, acc);
                    df = v.w - qv.w; acc = __builtin_fmaf(df, df, acc);
                }
                ct = acc;
                // a candidate at or beyond the sentinel distance (or NaN) is never a neighbour (dmet_oracle.c:62: strict
                // '>' against the 1e10 the lists start from) -- it counts as a missing entry from here on
                if (!(ct < kKnnSentinel)) {
                    ct = kKnnSentinel;
                    j = -1;
                    if (t == 0) myj[0] = -1; else myj[kFilterMaxSplit - 1] = -1;
                }
            }
            sc[slot][idx] = ct;
            sj[slot][idx] = (j >= 0) ? j : (0x7fffffff - idx);   // missing entries sort last, all distinct
        }
        if (t == 0) myc[0] = ct; else myc[kFilterMaxSplit - 1] = ct;
    }
    if (active && l == 0) { skth[slot] = -1.0f; sfail[slot] = 0; }
    wave_sync();
    const int k = a.k;
#pragma unroll
    for (int t = 0; t < kFilterMaxSplit; ++t) {
        if (active && t < nsub) {
            const int idx = t * M + l;
            const float c = myc[t];
            const int32_t jj = (myj[t] >= 0) ? myj[t] : (0x7fffffff - idx);
            int rank = 0;
            for (int e = 0; e < E; ++e) {
                const float ce = sc[slot][e];
                const int32_t je = sj[slot][e];
                rank += (ce < c || (ce == c && je < jj)) ? 1 : 0;
            }
            if (rank < k) {
                a.nbr[q * k + rank] = myj[t];
                if (a.nbr16) a.nbr16[q * k + rank] = local_id16(myj[t], ev_lo);
                a.dist[q * k + rank] = (myj[t] >= 0) ? c : kKnnSentinel;
                if (rank == k - 1 && myj[t] >= 0) skth[slot] = c;
            }
        }
    }
    wave_sync();
    // certification (one lane per partial list): a list that saw at least M keys dropped only keys >= its threshold
    if (active && l < nsub) {
        const float kth = skth[slot];
        const float an = __builtin_sqrtf(vnx) * 1.000001f;
        const float rn = an + __builtin_sqrtf(fmaxf(kth, 0.0f)) * 1.00002f;
        const float slack = 2.0f * (4e-5f * an * rn + 1e-5f * rn * rn + 4e-6f * an * an) + 1e-30f;
        const bool full = vtau < kKnnSentinel;
        // kth < 0 (fewer than k kept candidates) cannot coincide with a full list (M >= k)
        if (voverflow || (full && !(vtau + vnx - slack > kth))) sfail[slot] = 1;
    }
    wave_sync();
    if (active && l == 0 && sfail[slot] != 0) {      // count the query once
        flag_query(a, (int)qq, a.xtile_ptr[pos] + (int)((qq - ev_lo) / a.xtile_queries));
    }
}

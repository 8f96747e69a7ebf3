/*
 * dmet.h -- C ABI of libdmet_hip.so: the MI355X (gfx950) implementation of the graph operators on the
 * DeepMETv2 DynamicEdgeConv hot path.
 *
 * The reference (DeepMETv2, /root/reference) is pure Python; the kernels it executes for this path live in
 * the torch_cluster / torch_geometric / torch_scatter wheels.  Each entry point below names the reference
 * call site (file:line, relative to /root/reference) whose third-party operator it replaces.  The reference
 * side binds this library with ctypes; deepmetv2_amd/_lib.py is that binding.
 *
 * Conventions
 *  - extern "C", plain pointers and sizes.  Every pointer is a DEVICE pointer unless it says "host".
 *  - every call is asynchronous on `stream` (a hipStream_t passed as void*), performs no host
 *    synchronisation, allocates nothing and keeps no global mutable state (re-entrant, graph-capturable).
 *    Scratch comes from the caller: ask dmet_*_workspace_bytes(), pass `ws`/`ws_bytes`.
 *  - return value: 0 = ok; < 0 = failure (-EINVAL = -22 for bad arguments, -(1000+hipError_t) for a HIP
 *    runtime error).  dmet_last_error() returns a thread-local message for the last failure.
 *  - events (graphs) are the ragged units: event b owns nodes ptr[b] .. ptr[b+1]-1 (int64, B+1 entries).
 *  - neighbour tables are fixed width: nbr[N, k] int32 GLOBAL node ids, -1 = no neighbour (short events).
 *  - all floating point is IEEE fp32 unless the name says otherwise.
 */
#ifndef DMET_H_
#define DMET_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void *dmet_stream_t; /* hipStream_t */

#define DMET_VERSION 1
#define DMET_MAX_K 64       /* upstream torch_cluster rejects k > 100; this build supports k <= 64   */
#define DMET_MAX_KNN_DIM 64 /* feature width of the kNN space (hot path: 32; (eta,phi) graph: 2)      */
#define DMET_MAX_H 128      /* feature width of EdgeConv inputs/outputs (hot path: 32)                */

int dmet_version(void);
const char *dmet_last_error(void);
/* 1 if a HIP device is usable by this process, 0 otherwise (never fails). */
int dmet_device_available(void);

/* ---- K1: kNN graph build -------------------------------------------------------------------------
 * replaces torch_cluster.knn_graph / torch_cluster.knn
 *   call sites: model/graph_met_network.py:63, model/dynamic_reduction_network.py:86,94; inside PyG
 *   DynamicEdgeConv.forward.
 * For every node i: the k nodes j of the same event with the smallest squared L2 distance
 *   d(i,j) = sum_c fmaf(x[j,c]-x[i,c], x[j,c]-x[i,c], acc)  (sequential in c, fp32; rule R1)
 * ordered by (d, j) ascending; ties keep the lower j (rule R2); candidates at d >= 1e10 are never
 * selected (upstream sentinel).  Self is a candidate like any other (loop handling is host-side).
 * nbr[N,k] int32 (required), dist[N,k] fp32 (required): the k neighbours and their R1 distances.
 * One launch for all ragged events.  1 <= k <= DMET_MAX_K, 1 <= D <= DMET_MAX_KNN_DIM. */
size_t dmet_knn_workspace_bytes(int64_t N, int B, int D, int k);
int dmet_knn_f32(const float *x, const int64_t *ptr, int B, int64_t N, int D, int k, int32_t *nbr,
                 float *dist, void *ws, size_t ws_bytes, dmet_stream_t stream);
/* Same call, additionally writing the table as event-local ids: nbr_local[N,k] uint16 = nbr - ptr[event], 0xFFFF
 * for an empty slot (4-byte aligned; may be NULL = dmet_knn_f32).  Written by the same kernels that write nbr, for
 * dmet_gather_max_lds16_f32.  Rows of events with more than 65535 nodes are unspecified. */
int dmet_knn_local_f32(const float *x, const int64_t *ptr, int B, int64_t N, int D, int k, int32_t *nbr,
                       float *dist, uint16_t *nbr_local, void *ws, size_t ws_bytes, dmet_stream_t stream);
/* Periodic coordinates, for a kNN graph in the reference's (eta, phi) space (train.py:47: phi is an angle; the plain
 * distance puts phi = +3.1 and -3.1 6.2 apart instead of 0.08).  The contract above (R1, R2, the 1e10 sentinel, self
 * a candidate like any other) with one change, the one dmet_radius_periodic_f32 makes: for a coordinate c with
 * period L = period[c] > 0 the fp32 difference is wrapped before it is squared into the chain,
 *     d = x[j,c] - x[i,c];  a = |d|;  a = (a > 0.5f * L) ? L - a : a;  acc = fmaf(a, a, acc)
 * Ordering stays (d, j) ascending; candidates at d >= 1e10 or NaN are never selected; dist holds the wrapped R1
 * distance.  Two nodes at phi = +pi_f32 and -pi_f32 are at distance 0 in phi, so a query's seam twin ties with the query
 * itself and R2 decides.  period: host array of D floats, 0 = a plain coordinate; read on the host and passed by value
 * (a captured graph replays the periods of its capture).  Arguments and workspace (dmet_knn_workspace_bytes) as
 * dmet_knn_local_f32, whose per-thread size hint it spends the same way.  Returns -EINVAL for D outside [1, 8], a NULL
 * period, or a period that is NaN, inf or negative, before any device work.  An all-zero period gives exactly the
 * result of dmet_knn_local_f32. */
int dmet_knn_periodic_f32(const float *x, const int64_t *ptr, int B, int64_t N, int D, int k, const float *period,
                          int32_t *nbr, float *dist, uint16_t *nbr_local, void *ws, size_t ws_bytes,
                          dmet_stream_t stream);
/* Two point sets (torch_cluster.knn(x, y, k, batch_x, batch_y)): for every row of y (a QUERY, Ny rows, events ptr_y[B+1])
 * the k rows of x (the CANDIDATES, Nx rows, events ptr_x[B+1]) of the same event with the smallest distance.  The
 * distance of query i and candidate j is the fp32 chain used everywhere here, in coordinate order:
 *     d = x[j,c] - y[i,c];  periodic coordinate (period[c] = L > 0): a = |d|; a = (a > 0.5f * L) ? L - a : a;  else a = d;
 *     acc = fmaf(a, a, acc)
 * Row i of nbr[Ny,k] / dist[Ny,k]: ascending (acc, j), ties to the lower j (R2); a candidate with acc >= 1e10 or NaN is
 * never selected; a query whose event holds fewer than k admissible candidates gets a short row (-1 / 1e10 in the
 * empty slots), a query of an event without candidates an empty one; an event without queries costs nothing.  nbr holds
 * GLOBAL row numbers of x.  There is no self to exclude: the two sets have separate index spaces, and a point present in
 * both finds its twin at distance 0 like any other candidate.  period: NULL (all plain), or a host array of D floats as
 * for dmet_knn_periodic_f32 (then D <= 8).  Always the exact vector-ALU sweep (the kernel of dmet_knn_f32's exact path
 * with the queries cut from ptr_y and the candidate range taken from ptr_x), so x = y, ptr_x = ptr_y gives the table of
 * dmet_knn_f32 / dmet_knn_periodic_f32 bit for bit.  1 <= k <= DMET_MAX_K, 1 <= D <= DMET_MAX_KNN_DIM.  Returns -EINVAL
 * on bad arguments before any device work, 0 at once for Ny == 0. */
size_t dmet_knn_xy_workspace_bytes(int64_t Nx, int64_t Ny, int B, int D, int k);
int dmet_knn_xy_f32(const float *x, const int64_t *ptr_x, int64_t Nx, const float *y, const int64_t *ptr_y, int64_t Ny,
                    int B, int D, int k, const float *period, int32_t *nbr, float *dist, void *ws, size_t ws_bytes,
                    dmet_stream_t stream);
/* dmet_knn_local_f32 for the DynamicEdgeConv call shape (model/graph_met_network.py:63: the graph is built in the
 * space of the rows the convolution then consumes): the node-level dense layer of the fused EdgeConv,
 *   P = x.(W1-W2)^T + b, Q = x.W2^T   (W[32,64], D = 32),
 * depends on x only, like the graph, and is computed by trailing workgroups of the matrix-core filter launch: they are
 * dispatched last and fill the wavefront slots the build's last round leaves empty.  layout = 0: P, Q fp32 [N,32]
 * (dmet_node_linear_split_f32), 1: slice-major [4][N][8] (dmet_node_linear_split_sliced_f32), 2: bf16 operands on
 * the bf16 matrix cores, P fp32 [N,32], Q as bf16 bits [N,32] (dmet_node_linear_split_bf16).  *dense_done = 1: P and
 * Q were written (same bits as the call named); 0: this build took another path (D != 32, k > 20, the matrix-core
 * path switched off) and the caller launches the dense layer itself.  nbr / dist / nbr_local as above. */
int dmet_knn_local_dense_f32(const float *x, const int64_t *ptr, int B, int64_t N, int D, int k, int32_t *nbr,
                             float *dist, uint16_t *nbr_local, const float *W, const float *bias, int layout,
                             float *P, void *Q, int *dense_done, void *ws, size_t ws_bytes, dmet_stream_t stream);
/* The block shape of model/graph_met_network.py:64-66, `emb = emb + bn(conv(emb))` followed by the next DynamicEdgeConv
 * on emb: the BatchNorm transform + residual add that PRODUCES the build's input is fused into the build's prep launch,
 *   y = (raw - mean) * (gamma * invstd) + beta (+ residual)     (the expression and bits of dmet_bn_fwd_f32's transform;
 *   mean / invstd from dmet_bn_stats_f32 or the running statistics),
 * which writes y[N,32] and cuts its tile records from the values it just formed: one pass over the rows instead of two
 * and one launch less per layer.  Then dmet_knn_local_dense_f32(y, ...) (W == NULL: dmet_knn_local_f32).  *fused = 1:
 * y, the graph (and P / Q when *dense_done) were written; *fused = 0: NOTHING was launched (the build would not take the
 * matrix-core path: D != 32, k > 20, switched off, misaligned) and the caller runs the transform and the build itself. */
int dmet_bn_knn_local_dense_f32(const float *raw, const float *residual, const float *gamma, const float *beta,
                                const float *mean, const float *invstd, float *y, const int64_t *ptr, int B, int64_t N,
                                int D, int k, int32_t *nbr, float *dist, uint16_t *nbr_local, const float *W,
                                const float *bias, int layout, float *P, void *Q, int *dense_done, int *fused, void *ws,
                                size_t ws_bytes, dmet_stream_t stream);

/* What the caller knows about the event sizes of the NEXT dmet_knn*_f32 call on this thread (a data loader has the sizes
 * on the host; ptr lives on the device): every event of that batch has min_nodes .. max_nodes nodes; 0 = unknown.  The
 * hint is spent by that one call.  Today it saves one launch: when every event takes the second filter form (800 ..
 * 65536 nodes) the merge launch of the first form's tail items is dropped.  A hint that is WRONG costs time, never
 * results: an event the hint ruled out sends the queries concerned through the exact kernel. */
int dmet_knn_size_hint(int min_nodes, int max_nodes);

/* Diagnostics of the matrix-core kNN path (D = 32 or 64, k <= 20): dmet_knn_f32 first ranks candidates with an MFMA
 * filter (fp16 operands for events of 800..65536 nodes, a bf16 split for smaller ones), re-ranks the kept ones with
 * the exact R1 chain and certifies every query; uncertified queries are recomputed exactly (one workgroup per query
 * when their 128-query tile has at most 8 of them, by the exact tile kernel otherwise).  Rows with a feature of
 * magnitude >= 16384 (or not finite) in an event of 2048..65536 nodes are outside the fp16 operand range: they stay
 * candidates of every query and are themselves recomputed exactly -- same results, slower.  For the LAST dmet_knn_f32 call on this workspace: out[0] = tiles holding an uncertified query,
 * out[1] = uncertified queries (both 0 when the exact kernel ran alone).  Synchronises the stream.
 * Environment: DMET_KNN_PATH=exact forces the exact kernel for everything. */
int dmet_knn_fallback_stats(const void *ws, int64_t N, int B, int D, int k, int64_t *out, dmet_stream_t stream);
/* Second attempts of the last build in `ws` (matrix-core filter, second form): out[0] = wavefronts that swept their
 * event a second time because a query's certificate failed by the slack or its final threshold was cut too tight,
 * out[1] = the queries those sweeps were for.  Same arguments and synchronisation as dmet_knn_fallback_stats. */
int dmet_knn_retry_stats(const void *ws, int64_t N, int B, int D, int k, int64_t *out, dmet_stream_t stream);

/* ---- N1: radius graph build ----------------------------------------------------------------------
 * replaces torch_cluster.radius_graph   call sites: train.py:48, evaluate.py:88, plt_weight.py:122
 * For every node i: the FIRST max_nbr nodes j (ascending j) of the same event with d(i,j) < r*r
 * (strict, r*r formed in fp32).  nbr[N,max_nbr] int32 (-1 padded), cnt[N] int32 = entries stored in the row.
 * skip_self != 0 reproduces upstream's loop=False (call it with max_nbr = max_num_neighbors + 1): node i counts
 * towards the search limit when it is met but is not stored. */
int dmet_radius_f32(const float *x, const int64_t *ptr, int B, int64_t N, int D, float r, int max_nbr, int skip_self,
                    int32_t *nbr, int32_t *cnt, dmet_stream_t stream);
/* Same, but slots >= cnt[i] of row i are left UNWRITTEN (no -1 fill of the max_nbr-wide table: the reference's
 * max_num_neighbors=255 rows are ~36 deep, so the fill is most of the table's bytes).  For consumers that go by cnt:
 * dmet_gather_max_counted_f32, dmet_table_degree / dmet_table_edges, the arg-addressed backward. */
int dmet_radius_counted_f32(const float *x, const int64_t *ptr, int B, int64_t N, int D, float r, int max_nbr,
                            int skip_self, int32_t *nbr, int32_t *cnt, dmet_stream_t stream);
/* The same table (bit-identical: same candidates in the same order, same distance arithmetic) without multiplying out
 * all n^2 pairs of an event: queries are processed in the order of their FIRST coordinate, and a wavefront only keeps
 * the candidates whose first coordinate lies within r of its 64 queries' range (stream compaction in index order).
 * In (eta, phi) with r = 0.4 about 85 % of the pairs are never formed.  fill != 0: -1 fill as dmet_radius_f32,
 * fill == 0: as dmet_radius_counted_f32.  ws: dmet_radius_workspace_bytes(N) bytes (the processing order). */
size_t dmet_radius_workspace_bytes(int64_t N);
int dmet_radius_windowed_f32(const float *x, const int64_t *ptr, int B, int64_t N, int D, float r, int max_nbr,
                             int skip_self, int fill, int32_t *nbr, int32_t *cnt, void *ws, size_t ws_bytes,
                             dmet_stream_t stream);
/* Same, and optionally a second copy of every row as EVENT-LOCAL uint16 ids (nbr16 != NULL: rows of stride16 ids,
 * stride16 % 8 == 0, stride16 >= max_nbr, 16-byte aligned; slots cnt[i] .. roundup8(cnt[i]) - 1 hold 0xFFFF, the rest
 * of the row is unwritten; meaningful for events of at most 65534 nodes) for dmet_gather_max_local_j16_f32.
 * With nbr16 given and fill == 0, nbr may be NULL: the int32 table is then not written at all (for callers whose
 * consumers read the uint16 rows -- 288 000 x 255 int32 slots are 294 MB of address space, the ~36 used slots per row
 * 41 MB of 16-byte pieces). */
int dmet_radius_windowed_local_f32(const float *x, const int64_t *ptr, int B, int64_t N, int D, float r, int max_nbr,
                                   int skip_self, int fill, int32_t *nbr, int32_t *cnt, uint16_t *nbr16, int stride16,
                                   void *ws, size_t ws_bytes, dmet_stream_t stream);
/* Periodic coordinates, for the reference's (eta, phi) graph (train.py:47-48: phi is an angle, and the plain distance
 * puts phi = +3.1 and phi = -3.1 6.2 apart instead of 0.08).  period: host array of D floats; period[c] > 0 is the
 * circumference of coordinate c, 0 leaves it plain.  The only change to the contract above is the per-coordinate
 * difference of a periodic coordinate c with period L (fp32; exact by Sterbenz for a <= 2L):
 *     d = x[j,c] - x[i,c];  a = |d|;  a = (a > 0.5f * L) ? L - a : a;  acc = fmaf(a, a, acc)
 * This is the circular distance whenever |d| <= 1.5 L, i.e. when every value of a periodic coordinate lies within one
 * period (atan2 output in [-pi_f32, pi_f32] does); outside that the formula still defines the result.  Non-finite
 * coordinates give no hit, as in the plain form.  Returns -EINVAL for D outside [1, 8], a NULL period, or a period that
 * is NaN, inf or negative.  An all-zero period gives exactly the table of the plain entry.  The periods are read on the
 * host and passed by value: a captured graph replays the periods of its capture.
 * dmet_radius_periodic_f32: all pairs of an event (the arguments of dmet_radius_f32, fill != 0: its -1 fill, fill == 0:
 * the counted form of dmet_radius_counted_f32). */
int dmet_radius_periodic_f32(const float *x, const int64_t *ptr, int B, int64_t N, int D, float r, int max_nbr,
                             int skip_self, int fill, const float *period, int32_t *nbr, int32_t *cnt,
                             dmet_stream_t stream);
/* The windowed form of the same table (arguments of dmet_radius_windowed_local_f32 plus period), bit-identical to
 * dmet_radius_periodic_f32.  The window runs on coordinate 0, so period[0] must be 0 (-EINVAL otherwise): the
 * reference's [eta, phi] layout qualifies, a [phi, eta] layout must take the slower all-pairs entry (train.py:47-48). */
int dmet_radius_windowed_periodic_f32(const float *x, const int64_t *ptr, int B, int64_t N, int D, float r, int max_nbr,
                                      int skip_self, int fill, const float *period, int32_t *nbr, int32_t *cnt,
                                      uint16_t *nbr16, int stride16, void *ws, size_t ws_bytes, dmet_stream_t stream);
/* Two point sets (torch_cluster.radius(x, y, r, batch_x, batch_y, max_num_neighbors)): for every row of y the FIRST
 * max_nbr rows j of x (ascending j) of the same event with acc(i, j) < r * r (strict, fp32 product), acc the chain of
 * dmet_knn_xy_f32 (period: NULL or D floats).  nbr[Ny,max_nbr] int32 global row numbers of x, cnt[Ny] int32; fill != 0:
 * slots >= cnt[i] are -1, fill == 0: they are left unwritten (the counted form).  All pairs of an event (the kernel of
 * dmet_radius_f32 / dmet_radius_periodic_f32 with a second operand; no self to skip).  1 <= D <= 8.  Returns -EINVAL on
 * bad arguments before any device work, 0 at once for Ny == 0. */
int dmet_radius_xy_f32(const float *x, const int64_t *ptr_x, int64_t Nx, const float *y, const int64_t *ptr_y, int64_t Ny,
                       int B, int D, float r, int max_nbr, const float *period, int fill, int32_t *nbr, int32_t *cnt,
                       dmet_stream_t stream);

/* ---- K2+K3 fused: EdgeConv with nn = Linear(2*Hin -> Hout), aggr = 'max', fixed-width table ---------
 * replaces torch_geometric.nn.EdgeConv(nn=Sequential(Linear(2H,H)), aggr='max').forward
 *   constructed model/graph_met_network.py:36-38, invoked :65 (static graph) / :63 (dynamic kNN).
 *   out[i] = max_{s: nbr[i,s]>=0} ( W . [x_i || x_j - x_i] + b ),  j = nbr[i,s];  no neighbour -> 0 (R3)
 * computed through the exact split  W.[x_i || x_j-x_i] + b = (W1-W2).x_i + b + W2.x_j :
 *   step 1 (fp32 MFMA):  P[i] = (W1-W2).x_i + b,  Q[i] = W2.x_i           (tables [N,Hout] in ws)
 *   step 2 (gather+max): out[i] = P[i] + max_s Q[nbr[i,s]],  arg[i,c] = winning slot s (lowest on ties, R4)
 * W is torch Linear.weight layout [Hout, 2*Hin] row-major; arg[N,Hout] uint8 may be NULL (inference);
 * arg = 255 marks a node without neighbours.  Hin, Hout multiples of 32, <= DMET_MAX_H; k <= DMET_MAX_K. */
size_t dmet_edgeconv_linear_workspace_bytes(int64_t N, int Hout);
int dmet_edgeconv_linear_max_fwd_f32(const float *x, const int32_t *nbr, const int64_t *ptr, int B,
                                     int64_t N, int k, int Hin, int Hout, const float *W,
                                     const float *b, float *out, uint8_t *arg, void *ws,
                                     size_t ws_bytes, dmet_stream_t stream);
/* The same operator in ONE launch for events of up to 5119 nodes (Hin = Hout = 32, k in {8,16,32}): one workgroup
 * per (event, 8-channel slice) computes [Q slice | P slice] on the fp32 matrix cores (v_mfma_f32_16x16x4_f32),
 * keeps the Q slice of the whole event in LDS and gathers the k neighbour rows from there -- neighbour gather +
 * edge MLP + max with no P/Q round trip through memory.  Larger events are evaluated edge by edge (correct, slow). */
int dmet_edgeconv_fused_lds_f32(const float *x, const int32_t *nbr, const int64_t *ptr, int B, int64_t N, int k,
                                int Hin, int Hout, const float *W, const float *b, float *out, uint8_t *arg,
                                dmet_stream_t stream);
/* The two steps individually (step 2 is "the gather + scatter_max kernel" of BASELINE.json).
 * The contract of step 2, shared by every dmet_gather_max_* forward entry below and by dmet_edgeconv_fused_lds_f32 (stated
 * exactly by gather_max_ref in tests/gather_max_reference.py, to which all of them are held bit for bit):
 *   - row i examines its slots in ascending order (the first min(k, cnt[i]) of them where a cnt is given); a slot holding
 *     -1 (0xFFFF in uint16 rows) is empty and may stand anywhere in the row;
 *   - per channel the running maximum starts at -inf and is replaced on strict `>` only: the lowest slot wins exact ties
 *     (R4), +0 and -0 are equal, +inf wins, NaN and -inf candidates never win;
 *   - whether a row has neighbours is decided by its IDS, never by the values: a row with at least one non-empty slot gives
 *     out = P + max in every channel -- P + (-inf) = -inf, with arg 255, in a channel whose candidates are all -inf or NaN
 *     (an overflowed fp16 activation) while the other channels keep their maxima and winners;
 *   - a row without one gives out = 0 and arg = 255 (0xFFFF as a winner id) in every channel, whatever P holds (R3).
 * One deviation: for the events that gather_max_lds_kernel keeps in its LDS image (dmet_gather_max_lds_f32, _lds16_f32,
 * _lds_sliced_f32, _lds_sliced_cap_f32 and _mixed_f32; events of at most 5119 nodes, 2559 under a max_nodes hint) the result
 * is unspecified where every candidate of a channel is non-finite: there the kernel takes a finite maximum in the first of
 * a lane's four channels for "has neighbours", so a row whose candidates are all -inf / NaN in a channel c % 4 == 0 comes
 * out as 0 / 255 in those four channels.  Larger events in the same calls, and the L2, counted, winner-id and fused entries,
 * follow the id rule.  (Two ways of deciding it from the ids were measured at +4 % and +6 % on that kernel:
 * profiles/NOTES.md, "K3 empty-row rule".) */
int dmet_node_linear_split_f32(const float *x, int64_t N, int Hin, int Hout, const float *W,
                               const float *b, float *P, float *Q, dmet_stream_t stream);
int dmet_gather_max_f32(const float *P, const float *Q, const int32_t *nbr, const int64_t *ptr, int B,
                        int64_t N, int k, int H, float *out, uint8_t *arg, dmet_stream_t stream);
/* Slice-major pair: step 1 writes P and Q as [Hout/8][N][8] (the 8-channel slice of every node contiguous) and the
 * LDS-resident gather reads them that way -- its (event, slice) workgroups then stage Q and stream P as contiguous
 * bytes instead of 32-byte pieces of 128-byte rows.  out / arg stay row-major; nbr_local may be NULL; k in {8,16,20,32},
 * H % 8 == 0.  Same results as dmet_node_linear_split_f32 + dmet_gather_max_lds_f32. */
int dmet_node_linear_split_sliced_f32(const float *x, int64_t N, int Hin, int Hout, const float *W,
                                      const float *b, float *P, float *Q, dmet_stream_t stream);
/* The same dense layer with its input rows FORMED on the fly as y = residual + BatchNorm(raw) -- the block shape
 * `emb = emb + bn(conv(emb, edge_index))` of model/graph_met_network.py:65-66 followed by the next EdgeConv over the SAME
 * static graph (the reference's active flow, train.py:48: no kNN build whose prep launch could carry the transform):
 * y[N,H] is written (the block's output), P / Q are computed from the registers; y has the bits of dmet_bn_fwd_f32's
 * transform, P / Q those of dmet_node_linear_split[_sliced]_f32 on that y.  mean / invstd: dmet_bn_stats_f32 (training)
 * or dmet_bn_eval_stats_f32.  residual may be NULL.  H = 32 -> 32 only; sliced != 0: slice-major P / Q. */
int dmet_bn_node_linear_split_f32(const float *raw, const float *residual, const float *gamma, const float *beta,
                                  const float *mean, const float *invstd, float *y, int64_t N, int H, const float *W,
                                  const float *b, int sliced, float *P, float *Q, dmet_stream_t stream);
int dmet_gather_max_lds_sliced_f32(const float *P, const float *Q, const int32_t *nbr, const uint16_t *nbr_local,
                                   const int64_t *ptr, int B, int64_t N, int k, int H, float *out, uint8_t *arg,
                                   dmet_stream_t stream);
/* Same with a HINT on the batch's largest event (max_nodes; 0 = unknown = the entry above).  The kernel above is one
 * workgroup per CU whatever the event size -- by its 160 KB image and by its registers -- so its staging phase overlaps with
 * nothing.  For batches whose largest event fits 2 559 rows -- what model/data_loader.py:67-90 yields on real data -- and
 * uint16 ids given, workgroups of 512 threads on 80 KB images run two to a CU (one stages while the other gathers).  An
 * event beyond the hint takes the in-kernel L2 path: slower, never wrong.  Same bits. */
int dmet_gather_max_lds_sliced_cap_f32(const float *P, const float *Q, const int32_t *nbr, const uint16_t *nbr_local,
                                       const int64_t *ptr, int B, int64_t N, int k, int H, float *out, uint8_t *arg,
                                       int64_t max_nodes, dmet_stream_t stream);
/* Same contract with a per-node slot count: only the first cnt[i] slots of row i are examined (radius tables are
 * max_num_neighbors wide but a few dozen deep).  cnt may be NULL (= k for every node). */
int dmet_gather_max_counted_f32(const float *P, const float *Q, const int32_t *nbr, const int32_t *cnt, int64_t N,
                                int k, int H, float *out, uint8_t *arg, dmet_stream_t stream);
/* Same contract, LDS-resident form: one workgroup per (event, 8-channel slice) stages that slice of Q for the
 * whole event in the CU's 160 KB LDS (events up to 5120 nodes; larger events gather from global memory inside the
 * same kernel).  Needs ptr/B and H % 8 == 0.  The faster form for events of a few thousand nodes. */
int dmet_gather_max_lds_f32(const float *P, const float *Q, const int32_t *nbr, const int64_t *ptr, int B,
                            int64_t N, int k, int H, float *out, uint8_t *arg, dmet_stream_t stream);
/* LDS-resident form of dmet_gather_max_counted_f32 (radius tables: kmax slots per row, the first cnt[i] used): the
 * (event, 8-channel slice) workgroups and LDS image of dmet_gather_max_lds_f32; events that do not fit gather from
 * global memory inside the same kernel.  Identical results. */
int dmet_gather_max_counted_lds_f32(const float *P, const float *Q, const int32_t *nbr, const int32_t *cnt,
                                    const int64_t *ptr, int B, int64_t N, int k, int H, int pq_sliced, float *out,
                                    uint8_t *arg, dmet_stream_t stream);   /* pq_sliced != 0: P / Q are the slice-major
                                    tables of dmet_node_linear_split_sliced_f32 */
/* Winner-id form of dmet_gather_max_counted_lds_f32 for the reference's active flow (one 255-wide radius table per
 * batch, train.py:48): instead of the winning slot it stores, per (node, channel), the winner's EVENT-LOCAL node id
 * (argj[N,H] uint16, 0xFFFF = no neighbour; events of at most 65534 nodes), so that the backward scatter
 * (dmet_gather_max_bwd_j16_f32) needs no look-up in the wide table; `order` (optional, from dmet_table_order_by_count:
 * the event's local node indices grouped by slot count) makes the lane pairs of a wavefront walk rows of similar depth.
 * out is identical to dmet_gather_max_counted_f32.
 * dmet_table_order_by_count writes all of order[N]: per event a permutation of its local indices, deepest rows first.
 * The order inside a group of equal count is unspecified and may differ between runs (a counting sort with integer
 * atomics in LDS); it influences no result, every node is computed independently. */
int dmet_table_order_by_count(const int32_t *cnt, const int64_t *ptr, int B, int64_t N, int32_t *order,
                              dmet_stream_t stream);
int dmet_gather_max_counted_lds_j16_f32(const float *P, const float *Q, const int32_t *nbr, const int32_t *cnt,
                                        const int32_t *order, const int64_t *ptr, int B, int64_t N, int k, int H,
                                        int pq_sliced, float *out, uint16_t *argj, dmet_stream_t stream);
/* Second form of the ids for the same gather: rows of event-local uint16 ids written by the radius kernel itself
 * (dmet_radius_windowed_local_f32: nbr16[N][stride16], stride16 a multiple of 8 and >= max_nbr, 16-byte aligned; the
 * last started chunk of 8 of every row is padded with 0xFFFF; events of at most 65534 nodes): one aligned 16-byte
 * load per 8 slots, no packing pass.  Identical out / argj.  argj == NULL (inference): the maximum alone. */
int dmet_gather_max_local_j16_f32(const float *P, const float *Q, const uint16_t *nbr16, int stride16,
                                  const int32_t *cnt, const int32_t *order, const int64_t *ptr, int B, int64_t N,
                                  int kmax, int H, int pq_sliced, float *out, uint16_t *argj, dmet_stream_t stream);
/* gQ[j,c] = sum of g_out[i,c] over the (i,c) whose winner is j = ptr[event] + argj[i,c]: the per-event LDS scatter
 * with exact integer sums of dmet_gather_max_bwd_lds_f32 (bitwise reproducible), H = 32. */
int dmet_gather_max_bwd_j16_f32(const float *g_out, const uint16_t *argj, const int64_t *ptr, int B, int64_t N, int H,
                                float *gQ, dmet_stream_t stream);
/* Same again with the table ALSO given as event-local uint16 ids (nbr_local from dmet_knn_local_f32; k in {8,16,20,32},
 * 16-byte aligned): events that fit the LDS image read their ids from it -- half the id bytes, and every one of the
 * H/8 slice workgroups of an event re-reads the ids, so this is a third of the kernel's L2 requests.  Larger events
 * read nbr as before.  Results are identical to dmet_gather_max_lds_f32. */
int dmet_gather_max_lds16_f32(const float *P, const float *Q, const int32_t *nbr, const uint16_t *nbr_local,
                              const int64_t *ptr, int B, int64_t N, int k, int H, float *out, uint8_t *arg,
                              dmet_stream_t stream);
/* Ragged batches (BASELINE configs[4]: events of 500..8000 nodes): the gather form is chosen PER EVENT inside one call.
 * Events whose Q slice fits the LDS image (<= 5119 nodes) take the LDS-resident kernel, larger ones the L2-form kernel
 * (8 lanes per node, 16 row gathers in flight); both read the row-major P / Q tables and each skips the other's
 * events.  nbr_local may be NULL.  H = 32 and k in {8,16,20,32}; anything else is dmet_gather_max_f32.  Results are
 * identical to dmet_gather_max_f32.  Replaces the same reference lines as dmet_gather_max_f32
 * (model/graph_met_network.py:63,65 through torch_geometric.nn.EdgeConv / torch_scatter.scatter(max)). */
int dmet_gather_max_mixed_f32(const float *P, const float *Q, const int32_t *nbr, const uint16_t *nbr_local,
                              const int64_t *ptr, int B, int64_t N, int k, int H, float *out, uint8_t *arg,
                              dmet_stream_t stream);
/* Two-layer edge MLP on the bf16 matrix cores, fused with the aggregation (BASELINE configs[2]; the DRN call shape
 * model/dynamic_reduction_network.py:59-73,86-87): for nn = Linear(2 Hin, H1) - ELU - Linear(H1, H2) [- ELU] (act2 != 0)
 * over a fixed-width table nbr[N,k] (-1 = empty slot):
 *   out[i,:] = aggr_{s: nbr[i,s] >= 0} nn([x_i || x_{nbr[i,s]} - x_i]),  aggr = 0: max (0 for a node without neighbours,
 *   rule R3), 1: add.   W1[H1, 2 Hin], W2[H2, H1] row-major as torch.nn.Linear.weight; b1 / b2 may be NULL.
 * Inputs and weights are rounded to bf16, products accumulate in fp32, ELU and the aggregation are fp32: the bf16 bar
 * of rule R6 (rtol 2e-2) against the fp32 operators.  Nothing per-edge is written to memory.
 * Built for (Hin, H1, H2) in {(32, <= 64, 32 | 64), (64, <= 128, 64)} and k in {8, 16, 32}: dmet_edge_mlp2_supported.
 * Replaces torch_geometric.nn.EdgeConv.forward (index_select x2 -> cat -> nn -> scatter) for that `nn`. */
int dmet_edge_mlp2_supported(int Hin, int H1, int H2, int k);
int dmet_edge_mlp2_bf16(const float *x, int64_t N, int Hin, const int32_t *nbr, int k, const float *W1, const float *b1,
                        int H1, const float *W2, const float *b2, int H2, int act2, int aggr, float *out,
                        dmet_stream_t stream);
/* The same edge MLP followed by the BatchNorm1d(H2) that ends the DRN's `nn` (model/dynamic_reduction_network.py:59-70;
 * it normalises the per-edge MESSAGES, before the aggregation).  One pass over the edges: the affine map of the norm
 * commutes with the aggregation (sum: a S + cnt b; max: a max + b for a >= 0, a min + b otherwise), so the kernel writes
 * un-normalised aggregates plus per-wavefront partial sums of m and m^2 over the valid edges, a one-workgroup kernel turns
 * them into the per-channel (a, b) -- training != 0: batch statistics over the E valid edges (biased variance;
 * running_mean / running_var / num_batches_tracked, all optional, updated like torch.nn.BatchNorm1d); training == 0:
 * running statistics -- and a node-level kernel applies them.  Nodes without any neighbour give 0 (R3).
 * ws: dmet_edge_mlp2_bn_workspace_bytes(N, H2). */
size_t dmet_edge_mlp2_bn_workspace_bytes(int64_t N, int H2);
int dmet_edge_mlp2_bn_bf16(const float *x, int64_t N, int Hin, const int32_t *nbr, int k, const float *W1, const float *b1,
                           int H1, const float *W2, const float *b2, int H2, int act2, int aggr, const float *gamma,
                           const float *beta, float eps, float momentum, float *running_mean, float *running_var,
                           int64_t *num_batches_tracked, int training, float *out, void *ws, size_t ws_bytes,
                           dmet_stream_t stream);
/* ---- fp32 edge MLP over any grouped edge list, forward and backward (csrc/edgemlp_f32.hip) ----------------------
 * replaces torch_geometric.nn.EdgeConv.forward (edge features -> nn over E rows -> scatter) and its autograd graph for
 *   nn = Sequential(Linear(2 Hin, H1), ELU, Linear(H1, H2)[, ELU][, BatchNorm1d(H2)]), aggr in {max, add, mean}:
 *   model/dynamic_reduction_network.py:59-73 (the edge MLP), :86-87 and :94-95 (edgeconv1 / edgeconv2 over
 *   to_undirected(knn_graph(...))).
 * Graph: the grouped edge list of the K2/K3 section below: rowptr[N+1], src[E], tgt[E] int32 (edge e = src -> tgt,
 *   tgt[e] == i for rowptr[i] <= e < rowptr[i+1]); in-degrees are unbounded.  The backward also takes the by-source
 *   index srcptr[N+1], srcperm[E] (dmet_reverse_index of src).
 * W1[H1, 2 Hin], W2[H2, H1] row-major as torch.nn.Linear.weight; b1 / b2 may be NULL.  act2: ELU after the second
 *   Linear.  aggr: 0 max, 1 add, 2 mean.  bn: 0 none, 1 BatchNorm1d in training mode (batch statistics over the E
 *   messages, biased variance to normalise; running_mean / running_var (unbiased) / num_batches_tracked, all optional,
 *   moved once like torch), 2 eval (running statistics, required).  gamma / beta may be NULL (1 / 0).
 * dmet_edge_mlp_fwd_f32 writes out[N, H2] and the state the backward needs: pq[N, 2 H1] = [x (W1a - W1b)^T + b1 |
 *   x W1b^T], agg[2 N H2] (sum, or max then min), win[2 N H2] int32 (max only: grouped position of the winning edge of
 *   the max, then of the min, lowest on ties; defined only for nodes with in-edges), bnstat[4 H2] = (a, b, mean,
 *   invstd) of the per-channel map m -> a m + b.  A node without in-edges gives 0 (R3).  bn == 1 needs E >= 1.
 *   agg, like win, is defined only for nodes with in-edges: the rows of a node without one are left unwritten (every
 *   reader -- the apply launch, the BatchNorm backward sums -- skips a node whose rowptr says it has no in-edge).
 * dmet_edge_mlp_bwd_f32 takes g_out[N, H2] and writes gx[N, Hin] (may be NULL), gpq[N, 2 H1] = [gP | gQ] (the
 *   gradients of P and Q; the caller forms gW1 = [gP^T x | (gQ - gP)^T x] and gb1 = sum gP), gW2, gb2, and with a
 *   BatchNorm ggamma, gbeta (each may be NULL).  Every gradient is written, not accumulated.
 * N = 0 (then E = 0) is legal and reads no pointer: the forward writes nothing, the backward writes zero gW2, gb2,
 *   ggamma and gbeta.
 * Numerics: fp32 with fmaf chains; per-node and per-edge sums in edge order, partial sums in workgroup order, BatchNorm
 *   statistics in double: bit-identical from run to run, no atomics.  Not bit-equal to the generic route (the first
 *   Linear is split per node): within 1e-4 of the output and gradient scales.
 * Widths: H2 in {16, 32, 64, 128}, 1 <= H1 <= min(192, 2 H2), 1 <= Hin <= 128 (dmet_edge_mlp_f32_supported): the DRN
 *   at hidden 16 ... 128 (Hin = H2 = h, H1 = 3h/2).
 * ws: dmet_edge_mlp_f32_workspace_bytes(N, E, Hin, H1, H2), for either call (0 for unsupported widths). */
int dmet_edge_mlp_f32_supported(int Hin, int H1, int H2);
size_t dmet_edge_mlp_f32_workspace_bytes(int64_t N, int64_t E, int Hin, int H1, int H2);
int dmet_edge_mlp_fwd_f32(const float *x, int64_t N, int Hin, const int32_t *rowptr, const int32_t *src, const int32_t *tgt,
                          int64_t E, const float *W1, const float *b1, int H1, const float *W2, const float *b2, int H2,
                          int act2, int aggr, int bn, const float *gamma, const float *beta, float eps, float momentum,
                          float *running_mean, float *running_var, int64_t *num_batches_tracked, float *out, float *pq,
                          float *agg, int32_t *win, float *bnstat, void *ws, size_t ws_bytes, dmet_stream_t stream);
int dmet_edge_mlp_bwd_f32(const float *x, int64_t N, int Hin, const int32_t *rowptr, const int32_t *src, const int32_t *tgt,
                          int64_t E, const int32_t *srcptr, const int32_t *srcperm, const float *W1, int H1, const float *W2,
                          const float *b2, int H2, int act2, int aggr, int bn, const float *pq, const float *agg,
                          const int32_t *win, const float *bnstat, const float *g_out, float *gx, float *gpq, float *gW2,
                          float *gb2, float *ggamma, float *gbeta, void *ws, size_t ws_bytes, dmet_stream_t stream);
/* --- bf16 matrix-core edge MLP over any grouped edge list (entries csrc/edgemlp_f32.hip, kernels csrc/edgemlp_bf16.hip) --
 * The same layer, arguments, state and outputs as dmet_edge_mlp_fwd_f32 / dmet_edge_mlp_bwd_f32 above (it replaces the
 * same reference lines, model/dynamic_reduction_network.py:59-73,86-87,94-95, as the DRN runs them under bf16
 * autocast), with the per-edge products on the bf16 matrix cores (v_mfma_f32_16x16x32_bf16):
 *   forward: P, Q, ELU, aggregation and BatchNorm fp32; h1 and W2 rounded to bf16 (RNE), fp32 accumulation.
 *   backward: g_z2, h1 and W2 rounded to bf16 for g_h1 = g_z2 W2 and gW2 = g_z2^T h1, fp32 accumulation; node-level
 *   products (gx, and gW1 / gb1 on the caller's side) fp32.
 * Within rtol 2e-2 of the output and gradient scales of the fp32 layer (R6); bit-identical from run to run, no atomics,
 * no per-edge tensor in memory.  The state (pq, agg, win, bnstat) is interchangeable with the fp32 route's.
 * Widths: H2 in {32, 64, 128}, H1 a multiple of 16 with 16 <= H1 <= min(192, 2 H2), 1 <= Hin <= 128
 *   (dmet_edge_mlp_bf16_supported): the DRN at hidden 32, 64, 128 (Hin = H2 = h, H1 = 3h/2).
 * ws: dmet_edge_mlp_bf16_workspace_bytes(N, E, Hin, H1, H2), for either call (0 for unsupported widths). */
int dmet_edge_mlp_bf16_supported(int Hin, int H1, int H2);
size_t dmet_edge_mlp_bf16_workspace_bytes(int64_t N, int64_t E, int Hin, int H1, int H2);
int dmet_edge_mlp_fwd_bf16(const float *x, int64_t N, int Hin, const int32_t *rowptr, const int32_t *src, const int32_t *tgt,
                           int64_t E, const float *W1, const float *b1, int H1, const float *W2, const float *b2, int H2,
                           int act2, int aggr, int bn, const float *gamma, const float *beta, float eps, float momentum,
                           float *running_mean, float *running_var, int64_t *num_batches_tracked, float *out, float *pq,
                           float *agg, int32_t *win, float *bnstat, void *ws, size_t ws_bytes, dmet_stream_t stream);
int dmet_edge_mlp_bwd_bf16(const float *x, int64_t N, int Hin, const int32_t *rowptr, const int32_t *src, const int32_t *tgt,
                           int64_t E, const int32_t *srcptr, const int32_t *srcperm, const float *W1, int H1, const float *W2,
                           const float *b2, int H2, int act2, int aggr, int bn, const float *pq, const float *agg,
                           const int32_t *win, const float *bnstat, const float *g_out, float *gx, float *gpq, float *gW2,
                           float *gb2, float *ggamma, float *gbeta, void *ws, size_t ws_bytes, dmet_stream_t stream);
/* --- fp16 matrix-core edge MLP over any grouped edge list (entries csrc/edgemlp_f32.hip, kernels csrc/edgemlp_bf16.hip) --
 * The bf16 entries above with fp16 in place of bf16 (v_mfma_f32_16x16x32_f16; the route of the DRN under fp16 autocast,
 * torch.autocast("cuda") without a dtype, with torch.amp.GradScaler).  Same arguments, argument checks, widths,
 * workspace and state; the same kernels, instantiated for the other operand type.
 *   forward: P, Q, ELU, aggregation and BatchNorm fp32; h1 and W2 rounded to fp16, fp32 accumulation.
 *   backward: g_z2, h1 and W2 rounded to fp16 for g_h1 = g_z2 W2 and gW2 = g_z2^T h1, fp32 accumulation; node-level
 *   products fp32.
 * Rounding is round-to-nearest-even (as torch's .half()), never the packed round-toward-zero conversion.  A value whose
 * magnitude rounds beyond 65504 becomes +-inf (no saturation), so a gradient scaled past the fp16 range comes out
 * non-finite and GradScaler skips the step; fp16 subnormals are kept, so a scaled-up tiny g_z2 keeps its bits.
 * ws: dmet_edge_mlp_f16_workspace_bytes(N, E, Hin, H1, H2) (equal to the bf16 size). */
int dmet_edge_mlp_f16_supported(int Hin, int H1, int H2);
size_t dmet_edge_mlp_f16_workspace_bytes(int64_t N, int64_t E, int Hin, int H1, int H2);
int dmet_edge_mlp_fwd_f16(const float *x, int64_t N, int Hin, const int32_t *rowptr, const int32_t *src, const int32_t *tgt,
                          int64_t E, const float *W1, const float *b1, int H1, const float *W2, const float *b2, int H2,
                          int act2, int aggr, int bn, const float *gamma, const float *beta, float eps, float momentum,
                          float *running_mean, float *running_var, int64_t *num_batches_tracked, float *out, float *pq,
                          float *agg, int32_t *win, float *bnstat, void *ws, size_t ws_bytes, dmet_stream_t stream);
int dmet_edge_mlp_bwd_f16(const float *x, int64_t N, int Hin, const int32_t *rowptr, const int32_t *src, const int32_t *tgt,
                          int64_t E, const int32_t *srcptr, const int32_t *srcperm, const float *W1, int H1, const float *W2,
                          const float *b2, int H2, int act2, int aggr, int bn, const float *pq, const float *agg,
                          const int32_t *win, const float *bnstat, const float *g_out, float *gx, float *gpq, float *gW2,
                          float *gb2, float *ggamma, float *gbeta, void *ws, size_t ws_bytes, dmet_stream_t stream);
/* bf16 variant (BASELINE configs[2]): x and the split weights rounded to bf16 (RNE), multiplied on the bf16 matrix
 * cores with fp32 accumulation; P stays fp32, Q is stored as bf16 (raw bits) and gathered as 64-B rows.
 * Built for Hin = Hout = 32, k in {8,16,32}.  Backward is shared with the fp32 path (arg-based, fp32). */
int dmet_node_linear_split_bf16(const float *x, int64_t N, int Hin, int Hout, const float *W, const float *b,
                                float *P, uint16_t *Qh, dmet_stream_t stream);
int dmet_gather_max_bf16q(const float *P, const uint16_t *Qh, const int32_t *nbr, int64_t N, int k, int H,
                          float *out, uint8_t *arg, dmet_stream_t stream);
/* Backward of step 2 w.r.t. Q:  gQ[j,c] = sum over (i,s) with nbr[i,s]==j and arg[i,c]==s of g_out[i,c].
 * Deterministic (no float atomics): walks the reverse index rev_ptr[N+1] (int32), rev_slot[E] (int32,
 * entry = i*k+s, ascending inside a row) built by dmet_reverse_index(nbr, N*k, N, ...). */
int dmet_gather_max_bwd_f32(const float *g_out, const uint8_t *arg, const int32_t *rev_ptr,
                            const int32_t *rev_slot, int64_t N, int k, int H, float *gQ,
                            dmet_stream_t stream);
/* The same gQ without a reverse index (H = 32, node-sorted events as in ptr[B+1]; every nbr entry of a node lies in
 * the node's own event): a workgroup per (event, 4 channels) scatter-adds into LDS with 64-bit fixed-point integer
 * atomics -- integer sums are order-independent, hence bitwise reproducible; each term is rounded once to 2^-30 of the
 * slice's max |g_out|, the sums are exact.  Replaces the radix sort + L2 gather of the route above on the hot path. */
int dmet_gather_max_bwd_lds_f32(const float *g_out, const uint8_t *arg, const int32_t *nbr, const int64_t *ptr, int B,
                                int64_t N, int k, int H, float *gQ, dmet_stream_t stream);
/* Same, reading the winning neighbour's id from the event-local uint16 table of dmet_knn_local_f32 (nbr_local, may
 * be NULL) for events of at most 65535 nodes -- 32-byte instead of 64-byte rows under the scattered 2-byte reads. */
int dmet_gather_max_bwd_lds16_f32(const float *g_out, const uint8_t *arg, const int32_t *nbr,
                                  const uint16_t *nbr_local, const int64_t *ptr, int B, int64_t N, int k, int H,
                                  float *gQ, dmet_stream_t stream);
/* The same two scatters with a HINT on the batch's largest event (max_nodes; 0 = unknown = the entries above): a
 * workgroup's accumulators are (event nodes) x 4 channels x 8 bytes of LDS, so for batches of small events -- what
 * model/data_loader.py:67-90 yields on real data, 1 000-2 500 candidates per event -- the workgroups are sized down
 * (<= 1 152 nodes: 256 threads, 36 KB; <= 2 304: 512 threads, 72 KB) and several share a CU.  Events larger than the
 * hint take more passes: slower, never wrong.  Same bits as the unhinted entries (integer sums). */
int dmet_gather_max_bwd_lds16_cap_f32(const float *g_out, const uint8_t *arg, const int32_t *nbr,
                                      const uint16_t *nbr_local, const int64_t *ptr, int B, int64_t N, int k, int H,
                                      float *gQ, int64_t max_nodes, dmet_stream_t stream);
int dmet_gather_max_bwd_j16_cap_f32(const float *g_out, const uint16_t *argj, const int64_t *ptr, int B, int64_t N, int H,
                                    float *gQ, int64_t max_nodes, dmet_stream_t stream);
/* The pair scatter -> node-level kernel with gQ handed over SLICE-MAJOR, gQs[8][N][4] floats: a scatter workgroup owns 4
 * channels of one event, so in this layout it writes ONE contiguous run instead of a 16-byte piece of every 128-byte
 * row (13 of the scatter's 46 us at 64 x 4500 nodes were that write-out), and the node-level kernel's loads stay whole
 * 128-byte lines either way.  Same sums, same bits; only the layout of the intermediate differs.  arg_is_j16: `arg` holds
 * uint16 winner ids (dmet_gather_max_bwd_j16_sliced_f32) instead of uint8 slots. */
int dmet_gather_max_bwd_sliced_f32(const float *g_out, const uint8_t *arg, const int32_t *nbr, const uint16_t *nbr_local,
                                   const int64_t *ptr, int B, int64_t N, int k, int H, float *gQs, int64_t max_nodes,
                                   dmet_stream_t stream);
int dmet_gather_max_bwd_j16_sliced_f32(const float *g_out, const uint16_t *argj, const int64_t *ptr, int B, int64_t N,
                                       int H, float *gQs, int64_t max_nodes, dmet_stream_t stream);
int dmet_edgeconv_linear_bwd_sliced_f32(const float *x, const float *W, const float *g_out, const void *arg,
                                        int arg_is_j16, const float *gQs, const float *g_add, int64_t N, int H, float *gx,
                                        float *gW, float *gb, void *ws, size_t ws_bytes, dmet_stream_t stream);
/* ---- K2+K3 fused: EdgeConv with nn = Linear(2*Hin -> Hout), aggr = 'add' / 'sum' / 'mean', any graph -----------
 * replaces torch_geometric.nn.EdgeConv(nn=Sequential(Linear(2H,H')), aggr='add'|'mean').forward
 *   the layer constructed at model/graph_met_network.py:36-38 with aggr switched from 'max'.
 * With P, Q from dmet_node_linear_split_f32 and deg[i] the number of valid in-edges of node i:
 *   add / sum (mean = 0): out[i] = deg[i] P[i] + sum_j Q[j]
 *   mean      (mean = 1): out[i] = P[i] + (sum_j Q[j]) / deg[i]
 *   deg[i] = 0: out[i] = 0 exactly, also where P[i] is not finite (R3).
 * sum_j runs in ascending slot / edge order in fp32, no float atomics: a table and the by-target edge list of the same
 * graph give identical bits, and every run gives the same bits.  deg[N] int32 is written for the backward.
 * H = Hout in {32, 64} (Hin in {32, 64} is dmet_node_linear_split_f32's); P, Q, out 16-B aligned.
 * Table form: nbr[N, k] int32, -1 = no neighbour; cnt NULL: k <= DMET_MAX_K; cnt[N] given (radius tables): only the
 * first cnt[i] slots of row i are read, k <= 1024 (radius_graph with loop=False is max_num_neighbors + 1 = 256 wide).  CSR form: rowptr[N+1], src[E] grouped by target (see K2 / K3
 * un-fused below), any in-degree; src may be NULL when E = 0. */
int dmet_gather_sum_table_f32(const float *P, const float *Q, const int32_t *nbr, const int32_t *cnt, int64_t N, int k,
                              int H, int mean, float *out, int32_t *deg, dmet_stream_t stream);
int dmet_gather_sum_csr_f32(const float *P, const float *Q, const int32_t *rowptr, const int32_t *src, int64_t N, int H,
                            int mean, float *out, int32_t *deg, dmet_stream_t stream);
/* Backward of the two entries above, w.r.t. P and Q (g_out[N,H], deg from the forward):
 *   gP[i] = deg[i] g_out[i] (add) or [deg[i] > 0] g_out[i] (mean);  0 where deg[i] = 0 (R3)
 *   gQ[j] = sum over the edges j -> i of s_i g_out[i],  s_i = 1 (add) or 1 / deg[i] (mean)
 * walked through a by-source index rev_ptr[N+1], rev_idx[] in ascending order (deterministic, no float atomics):
 *   k >= 1 (table): rev_idx = table positions i*k+s of NeighborTable.reverse() (dmet_reverse_index of nbr), k <= 1024,
 *                   tgt unused;
 *   k == 0 (CSR):   rev_idx = edge positions of dmet_reverse_index(src), the target of entry t is tgt[rev_idx[t]]
 *                   (tgt may be NULL when E = 0).
 * gx, gW, gb follow from gP, gQ through dmet_edgeconv_linear_bwd_f32 with g_out = gP and arg = NULL (H = 32). */
int dmet_gather_sum_bwd_f32(const float *g_out, const int32_t *deg, const int32_t *rev_ptr, const int32_t *rev_idx,
                            const int32_t *tgt, int64_t N, int k, int H, int mean, float *gP, float *gQ,
                            dmet_stream_t stream);
/* ---- Non-finite values in the fused aggregations ---------------------------------------------------------------------
 * One contract for dmet_gravnet_*, dmet_attention_*, dmet_gat_*, dmet_interpolate_*, dmet_multi_aggr_*,
 * dmet_weighted_sum_* and dmet_pointnet_* (the sections below name their lanes); tests/nonfinite_contract.py holds them to it.
 *   Sum lanes follow IEEE: a non-finite term makes its channel non-finite.
 *   Softmax lanes follow torch.softmax of the row's scores wherever in the row an entry stands and however the row falls
 *     into chunks: -inf beside a finite score weighs exactly 0; a row holding only -inf, or any +inf or NaN, is NaN in out,
 *     lse and all its alpha; an empty slot is told by its id.
 *   Max / min lanes give the max / min over the candidates that are numbers; +-inf are numbers and can win; ties go to the
 *     lowest position (R4); a NaN candidate never wins and never blocks, in any slot; a channel of a non-empty row whose
 *     candidates are all NaN gives NaN with winner "none" (255 / -1), so the backward routes nothing for it.  The result
 *     does not depend on the order of the row's entries except through R4.  (Gather-max, above, reports -inf there; PyG's
 *     amax propagates a NaN.)
 *   Clamp lanes keep a NaN, as torch.clamp does: they are written as a comparison, never as fmaxf.
 *   Locality, forward and backward: a non-finite value in source row j changes the outputs of the rows that list j and
 *     nothing else; every other output row, and every gradient row of a source or target that shares no row with j, has
 *     the bits of the run without it. */
/* ---- GravNet aggregation --------------------------------------------------------------------------------------
 * replaces the propagate step of torch_geometric.nn.GravNetConv (message x_j * exp(-10 d^2), aggr ['mean', 'max']) and
 * its autograd graph, which index_select the [E, P] messages twice and scatter them twice (csrc/gravnet.hip).
 * Inputs: a fixed-width table nbr[Nt, k] int32 of ids into the SOURCE set (-1 = empty slot, anywhere in a row; an id
 *   outside [0, Ns) is treated as empty), s_tgt[Nt, S] and s_src[Ns, S] the learned coordinates of the targets (the
 *   table's rows) and of the sources, h[Ns, P] the features that are propagated.  The one-set form passes
 *   s_src == s_tgt and Ns == Nt.  1 <= k <= DMET_MAX_K, 1 <= S <= 16, 1 <= P <= DMET_MAX_H (any P: 22 is the usual one).
 * dmet_gravnet_fwd_f32, for target i and every valid slot t, j = nbr[i,t]:
 *   d = sum_c fmaf(a, a, acc), a = s_src[j,c] - s_tgt[i,c], in coordinate order (R1: on a table of dmet_knn_f32 /
 *       dmet_knn_xy_f32 built in the same space d has the bits of that table's dist);  w = expf(-10.0f * d)
 *   out[i, 0:P]  = (sum_t w h[j,:]) / cnt_i   slots added in ascending t, cnt_i = the number of valid slots (PyG's mean)
 *   out[i, P:2P] = max_t w h[j,p]             arg[Nt, P] uint8 = the winning slot, ties to the lowest slot (R4)
 *   cnt[Nt] int32 = cnt_i.  A row without a valid slot gives zeros in both halves (R3), cnt 0 and arg = 255 ("no winner").
 *   Non-finite values: the mean half is a sum lane, the max half a max lane over the messages w h[j,p] that are numbers; a
 *   channel whose messages are all NaN gives NaN with arg 255.
 *   Nothing per edge is written.
 * dmet_gravnet_bwd_f32, with g_msg[i,t,p] = g_out[i,p] / cnt_i + (arg[i,p] == t ? g_out[i,P+p] : 0):
 *   g_h[j,p]     = sum over the (i,t) with nbr[i,t] == j of w g_msg[i,t,p]
 *   g_w[i,t]     = sum_p g_msg[i,t,p] h[j,p],   g_d[i,t] = -10 w g_w   (0 in an empty slot)
 *   g_s_tgt[i,c] = sum_t 2 g_d (s_tgt[i,c] - s_src[j,c]),   g_s_src[j,c] = sum over (i,t) of 2 g_d (s_src[j,c] - s_tgt[i,c])
 *   in two launches: by target (g_d, g_s_tgt; ascending t), then by source over the reverse index rev_ptr[Ns+1],
 *   rev_pos[] of dmet_reverse_index(nbr, Nt*k, Ns) (g_h, g_s_src; positions ascending).  g_d[Nt, k] fp32, 4 B per slot,
 *   is the only per-edge buffer (caller's scratch, every slot written).  w is recomputed, never stored; an underflowed
 *   w == 0 gives zero gradients, never NaN.  Every gradient is written, not accumulated; the caller of the one-set
 *   form adds g_s = g_s_tgt + g_s_src.  No float atomics: sums run in a fixed order, two runs give identical bits.
 * Both return -EINVAL on bad arguments before any device work.  Nt == 0: the forward returns 0 at once; the backward
 * zero-fills g_h and g_s_src (Ns > 0) and returns. */
int dmet_gravnet_fwd_f32(const float *s_tgt, const float *s_src, const float *h, const int32_t *nbr, int64_t Nt,
                         int64_t Ns, int k, int S, int P, float *out, uint8_t *arg, int32_t *cnt, dmet_stream_t stream);
int dmet_gravnet_bwd_f32(const float *s_tgt, const float *s_src, const float *h, const int32_t *nbr,
                         const int32_t *rev_ptr, const int32_t *rev_pos, const uint8_t *arg, const int32_t *cnt,
                         const float *g_out, int64_t Nt, int64_t Ns, int k, int S, int P, float *g_d, float *g_s_tgt,
                         float *g_s_src, float *g_h, dmet_stream_t stream);
/* ---- Attention aggregation ------------------------------------------------------------------------------------
 * replaces torch_geometric.nn.TransformerConv.message (alpha = (query_i * key_j).sum(-1) / sqrt(out_channels),
 * alpha = softmax(alpha, index, ptr, size_i), out = value_j * alpha.view(-1, heads, 1)), torch_geometric.utils.softmax
 * (scatter max, exp, scatter sum, divide) and the 'add' aggregation, with their autograd graph: three [E, H*C] gathers,
 * two scatters for the softmax and one for the sum, all kept for the backward (csrc/attention.hip).
 * Inputs: q[Nt, H, C] of the targets, k[Ns, H, C] and v[Ns, H, C] of the sources, fp32, contiguous.  The graph in one of
 * two forms:
 *   table (rowptr == NULL): idx = nbr[Nt, width] int32, -1 or any id outside [0, Ns) = an empty slot, anywhere in a row;
 *     position pos = i*width + t belongs to target i; 1 <= width <= DMET_MAX_K; E is ignored.
 *   list  (rowptr != NULL): the grouped edge list of the K2 / K3 section below: rowptr[Nt+1], idx = src[E], tgt[E] int32,
 *     any in-degree; width is ignored; src / tgt may be NULL when E == 0.
 * 1 <= C <= 64, 1 <= H <= 16, H*C <= 256: dmet_attention_supported(H, C) returns 1 for these and 0 otherwise.
 * dmet_attention_fwd_f32, for target i, head h and every valid entry e of row i, j = src(e):
 *   score_e = (sum_c q[i,h,c] k[j,h,c]) / sqrtf(C)     a division, as PyG writes it
 *   m = max_e score_e,  l = sum_e expf(score_e - m),  alpha_e = expf(score_e - m) / l
 *   out[i,h,:] = sum_e alpha_e v[j,h,:]                  lse[Nt, H]: lse[i,h] = m + logf(l)
 *   A row is taken in chunks of 16 (C <= 32) or 32 entries with a running (m, l, acc) rescaled once per chunk; the terms
 *   of l and acc are added in ascending entry order and out = acc / l.  A dot product is the sum of each lane's
 *   channels c = lane, lane + 16|32 in ascending order, then an xor butterfly over the lanes.  The bits depend on that
 *   chunking, never on the launch or on the run; a table and a list that hold the same entries in the same order give
 *   the same bits.  A row with no valid entry gives out = 0 (R3) and lse = 0.
 *   alpha[E or Nt*width, H] (may be NULL): the weights, 0 in an empty slot (told by its id).  Nothing else per edge is
 *   written.  Non-finite scores: a softmax lane.  An entry whose score is -inf weighs exactly 0 beside a finite score,
 *   wherever it stands -- a first chunk (or any run of chunks) of nothing but such entries leaves l = 0 and acc = 0, and a
 *   state with m == -inf is rescaled by 0, never by expf(-inf - m); a NaN score makes l NaN and the product with 0 keeps
 *   it.  A row whose scores are all -inf (or hold +inf or NaN) gives NaN in out, lse and alpha, as torch's softmax does.
 *   The value sum is a sum lane: a weight of exactly 0 times a non-finite v[j,h,c] is NaN in that channel, as in
 *   alpha.unsqueeze(-1) * v[src].
 * dmet_attention_bwd_f32, two launches.  By target, with delta[i,h] = sum_c g_out[i,h,c] out[i,h,c]:
 *   alpha_e = expf(score_e - lse[i,h])  (recomputed with the forward's chain),
 *   g_s_e = alpha_e (sum_c g_out[i,h,c] v[j,h,c] - delta[i,h]),   g_q[i,h,:] = (sum_e g_s_e k[j,h,:]) / sqrtf(C)
 *   alpha_w, gs_w [E or Nt*width, H] fp32: the caller's scratch, every position written (0 in an empty slot); they are
 *   the only per-edge buffers.  By source, over the by-source index rev_ptr[Ns+1], rev_pos[] in ascending order --
 *   dmet_reverse_index(nbr, Nt*width, Ns) for a table (i = pos / width), dmet_reverse_index(src, E, Ns) for a list
 *   (i = tgt[pos]):
 *   g_v[j,h,:] = sum alpha_e g_out[i,h,:]       g_k[j,h,:] = (sum g_s_e q[i,h,:]) / sqrtf(C)
 *   A hub's list is walked by its one owner.  Every gradient is written, not accumulated; rows and sources without
 *   entries get zeros.  No float atomics: two runs give identical bits.
 * Both return -EINVAL on anything outside these limits and on NULL or negative arguments, before any device work.
 * Nt == 0: the forward returns 0 at once; the backward zero-fills g_k and g_v (Ns > 0) and returns. */
int dmet_attention_supported(int H, int C);
int dmet_attention_fwd_f32(const float *q, const float *k, const float *v, const int32_t *idx, const int32_t *rowptr,
                           int64_t Nt, int64_t Ns, int64_t E, int width, int H, int C, float *out, float *lse,
                           float *alpha, dmet_stream_t stream);
int dmet_attention_bwd_f32(const float *q, const float *k, const float *v, const float *out, const float *lse,
                           const float *g_out, const int32_t *idx, const int32_t *rowptr, const int32_t *tgt,
                           const int32_t *rev_ptr, const int32_t *rev_pos, int64_t Nt, int64_t Ns, int64_t E, int width,
                           int H, int C, float *alpha_w, float *gs_w, float *g_q, float *g_k, float *g_v,
                           dmet_stream_t stream);
/* ---- GAT aggregation: additive attention ---------------------------------------------------------------------------
 * replaces torch_geometric.nn.GATv2Conv.edge_update (x = x_i + x_j; x = F.leaky_relu(x, negative_slope);
 * alpha = (x * self.att).sum(dim=-1); alpha = softmax(alpha, index, ptr, dim_size)) and GATConv.edge_update
 * (alpha = alpha_j + alpha_i; alpha = F.leaky_relu(alpha, negative_slope); alpha = softmax(...)), the message
 * x_j * alpha.unsqueeze(-1) of both, the 'add' aggregation, remove_self_loops + add_self_loops on the edge index, and
 * their autograd graph: two [E, H*C] gathers and their sum, two scatters for the softmax and one for the sum
 * (csrc/gat.hip).
 * mode 2 (GATv2Conv): xl[Ns, H, C] of the sources, xr[Nt, H, C] of the targets, att[H, C]; s_src / s_dst are ignored.
 * mode 1 (GATConv):   xl[Ns, H, C], s_src[Ns, H], s_dst[Nt, H] (the caller's (x * att_src).sum(-1) and
 *   (x * att_dst).sum(-1)); xr / att are ignored.  fp32, contiguous.  slope: the LeakyReLU's, finite and >= 0.
 * The graph is the attention section's: a table (rowptr == NULL, idx = nbr[Nt, width], 1 <= width <= DMET_MAX_K, an id
 * outside [0, Ns) = an empty slot) or a grouped list (rowptr[Nt+1], idx = src[E], tgt[E]; any in-degree).
 * self_loops = 1 (legal only with Nt == Ns, one node set): a written entry with src == i is skipped and one implicit
 *   entry i -> i is taken after the row's own entries -- remove_self_loops + add_self_loops without rewriting the graph.
 * 1 <= C <= 64, 1 <= H <= 16, H*C <= 256: dmet_gat_supported(H, C) returns 1 for these and 0 otherwise.
 * dmet_gat_fwd_f32, for target i, head h and every valid entry e of row i, j = src(e), lrelu(t) = t > 0 ? t : slope t:
 *   mode 2: score_e = sum_c att[h,c] lrelu(xl[j,h,c] + xr[i,h,c])        mode 1: score_e = lrelu(s_src[j,h] + s_dst[i,h])
 *   m = max_e score_e,  l = sum_e expf(score_e - m),  alpha_e = expf(score_e - m) / l
 *   out[i,h,:] = sum_e alpha_e xl[j,h,:]                 lse[Nt, H]: lse[i,h] = m + logf(l)
 *   PyG's softmax divides by l + 1e-16; l >= 1 (the maximum's own term), so the 1e-16 is below fp32 rounding and is
 *   omitted, as in the attention section.  A row is taken in chunks of 16 (C <= 32) or 32 entries with a running
 *   (m, l, acc) rescaled once per chunk; the terms of l and acc are added in ascending entry order, the implicit self
 *   entry last, and out = acc / l.  A sum over channels is each lane's channels c = lane, lane + 16|32 in ascending
 *   order, then an xor butterfly over the lanes.  The bits depend on that chunking, never on the launch or on the run; a
 *   table and a list that hold the same entries in the same order give the same bits.  A row with no valid entry gives
 *   out = 0 (R3) and lse = 0; with self_loops a row with no other entry gives out[i,h,:] = xl[i,h,:] exactly.
 *   Non-finite scores: a softmax lane, as in the attention section; with self_loops a row whose written entries all score
 *   -inf gives out[i,h,:] = xl[i,h,:] exactly, the self weight 1 and lse = the self score.
 *   alpha[E or Nt*width, H] (may be NULL): the weights of the written entries, 0 in an empty slot and in a skipped
 *   written self loop; the implicit entry's weight is not returned.  Nothing else per edge is written.
 * dmet_gat_bwd_f32, two launches.  By target, with delta[i,h] = sum_c g_out[i,h,c] out[i,h,c] and the score recomputed
 *   with the forward's chain:  alpha_e = expf(score_e - lse[i,h]),  g_s_e = alpha_e (sum_c g_out[i,h,c] xl[j,h,c] - delta).
 *   mode 2, t_e[c] = xl[j,h,c] + xr[i,h,c], d_e[c] = (g_s_e att[h,c]) (t_e[c] > 0 ? 1 : slope) (the slope at t == 0, as
 *     torch's leaky_relu backward):  g_xr[i,h,:] = sum_e d_e,  g_att_rows[Nt, H, C]: g_att_rows[i,h,c] = sum_e g_s_e
 *     lrelu(t_e[c]), both in ascending e; the caller sums g_att_rows over i in a fixed order for g_att.  gs_w = g_s_e.
 *   mode 1, d_e = g_s_e (s_src[j,h] + s_dst[i,h] > 0 ? 1 : slope):  g_sdst[i,h] = sum_e d_e, ascending e.  gs_w = d_e.
 *   alpha_w, gs_w [E or Nt*width, H] fp32: the caller's scratch, every position written (0 in an empty slot); they are
 *   the only per-edge buffers.  alpha_self, gs_self [Nt, H]: the same pair for the implicit entry (self_loops; may be
 *   NULL otherwise).  By source, over the by-source index rev_ptr[Ns+1], rev_pos[] in ascending order (as in the
 *   attention section), then the implicit entry j -> j; a written self loop is skipped here too:
 *   mode 2: g_xl[j,h,:] = sum (alpha_e g_out[i,h,:] + d_e)        mode 1: g_xl[j,h,:] = sum alpha_e g_out[i,h,:],
 *                                                                          g_ssrc[j,h] = sum gs_w
 *   A hub's list is walked by its one owner.  Every gradient is written, not accumulated; rows and sources without
 *   entries get zeros.  No float atomics: two runs give identical bits.  Pointers of the other mode may be NULL.
 * Both return -EINVAL on anything outside these limits, on NULL or negative arguments, on self_loops with Nt != Ns and on
 * a non-finite or negative slope, before any device work.  Nt == 0: the forward returns 0 at once; the backward
 * zero-fills g_xl (and g_ssrc in mode 1) when Ns > 0 and returns. */
int dmet_gat_supported(int H, int C);
int dmet_gat_fwd_f32(int mode, const float *xl, const float *xr, const float *att, const float *s_src, const float *s_dst,
                     float slope, int self_loops, const int32_t *idx, const int32_t *rowptr, int64_t Nt, int64_t Ns,
                     int64_t E, int width, int H, int C, float *out, float *lse, float *alpha, dmet_stream_t stream);
int dmet_gat_bwd_f32(int mode, const float *xl, const float *xr, const float *att, const float *s_src, const float *s_dst,
                     float slope, int self_loops, const float *out, const float *lse, const float *g_out,
                     const int32_t *idx, const int32_t *rowptr, const int32_t *tgt, const int32_t *rev_ptr,
                     const int32_t *rev_pos, int64_t Nt, int64_t Ns, int64_t E, int width, int H, int C, float *alpha_w,
                     float *gs_w, float *alpha_self, float *gs_self, float *g_xl, float *g_xr, float *g_att_rows,
                     float *g_ssrc, float *g_sdst, dmet_stream_t stream);
/* ---- Interpolation: inverse-distance feature propagation ------------------------------------------------------------
 * replaces the body of torch_geometric.nn.unpool.knn_interpolate(x, pos_x, pos_y, batch_x, batch_y, k) after its kNN
 * search (squared_distance = (pos_x[x_idx] - pos_y[y_idx]).pow(2).sum(-1), weights = 1 / clamp(squared_distance,
 * min=1e-16), y = scatter(x[x_idx] * weights, y_idx, 'sum') / scatter(weights, y_idx, 'sum')) and its autograd graph: a
 * [2, E] edge index sized by a host sync, two index_selects, the [E, F] messages and two scatters with float atomics
 * (csrc/interpolate.hip).
 * Inputs: a fixed-width table nbr[Nt, k] int32 of ids into the SOURCE set (-1 = empty slot, anywhere in a row; an id
 *   outside [0, Ns) is treated as empty), dist[Nt, k] fp32 the table's own R1 squared distances (dmet_knn_xy_f32 /
 *   dmet_knn_f32, periodic or not; the value in an empty slot is ignored), x[Ns, F] fp32 the source features.
 *   1 <= k <= DMET_MAX_K, 1 <= F <= 256.
 * dmet_interpolate_fwd_f32, for target i and every valid slot t, j = nbr[i,t]:
 *   w_t = 1.0f / (dist[i,t] < 1e-16f ? 1e-16f : dist[i,t])     torch.clamp(min=1e-16): a NaN distance stays NaN (a clamp
 *                                                              lane), so W_i, r and the whole row of out are NaN
 *   W_i = sum_t w_t                         valid slots in ascending t, fp32
 *   r_t = w_t / W_i
 *   out[i,f] = fmaf(r_t, x[j,f], acc)       valid slots in ascending t, acc from 0
 *   wsum[Nt] fp32: wsum[i] = W_i.  A row without a valid slot gives out[i,:] = 0 exactly (R3) and wsum[i] = 0.
 *   The weights are normalised before the sum (upstream divides the sum): nothing overflows at w = 1e16, the backward
 *   needs r anyway, and the two forms differ by rounding only.  Nothing per edge is written.  out is a sum lane: a
 *   non-finite x[j,f] shows in feature f of the rows that list j and nowhere else.
 * dmet_interpolate_bwd_f32, by source j over the reverse index rev_ptr[Ns+1], rev_pos[] of
 *   dmet_reverse_index(nbr, Nt*k, Ns), positions p = i*k + t in ascending order:
 *   g_x[j,f] = fmaf(r_p, g_out[i,f], acc)   r_p = w_p / wsum[i] with w_p the forward's expression of dist[p], clamp
 *   included: the same bits, NaN where the forward's was.  A source nobody lists gets g_x[j,:] = 0.  A long list is walked by its one owner.
 *   There is no gradient into dist (upstream forms the weights under no_grad).
 * No float atomics: sums run in a fixed order, two runs give identical bits.  Every element of out, wsum and g_x is
 * written, not accumulated.  Rows are read and written 16 bytes at a time where F % 4 == 0 and x / out (g_out / g_x)
 * start on a 16-byte boundary, element by element otherwise, with the same bits.
 * Both return -EINVAL on bad arguments (NULL pointers, negative sizes, k or F out of range) before any device work.
 * Nt == 0: the forward returns 0 at once; the backward zero-fills g_x (Ns > 0) and returns. */
int dmet_interpolate_fwd_f32(const float *x, const int32_t *nbr, const float *dist, int64_t Nt, int64_t Ns, int k, int F,
                             float *out, float *wsum, dmet_stream_t stream);
int dmet_interpolate_bwd_f32(const float *g_out, const float *dist, const float *wsum, const int32_t *rev_ptr,
                             const int32_t *rev_pos, int64_t Nt, int64_t Ns, int k, int F, float *g_x, dmet_stream_t stream);
/* ---- Multi-aggregation: sum, mean, min, max, var and std of the same neighbour rows ----------------------------------
 * replaces the aggregators of torch_geometric.nn.PNAConv (aggr.SumAggregation ... aggr.StdAggregation under
 * aggr.DegreeScalerAggregation), one scatter each over the same [E, F] messages, and supplies the variance of
 * torch_scatter.scatter_std (csrc/multi_aggr.hip): every source row is gathered once per walk and all requested
 * statistics are formed from it in registers.
 * The graph: width >= 1 is a table idx = nbr[Nt, width] (1 <= width <= DMET_MAX_K, position p = i*width + t belongs to
 *   target i, E and rowptr are ignored); width == 0 is an edge list grouped by target, idx = src[E], rowptr[Nt+1]
 *   (clamped to [0, E]), any in-degree.  -1 and an id outside [0, Ns) are no entry; a duplicate id counts once per slot.
 * x[Ns, F] fp32, 1 <= F <= 256; G >= 1 feature groups with F % G == 0.
 * aggrs: the A requested statistics in request order, four bits each from the lowest: 1 sum, 2 mean, 3 min, 4 max,
 *   5 var, 6 std; the first zero nibble ends the list; 1 <= A <= 6, each statistic at most once.
 * dmet_multi_aggr_fwd_f32, for target i with valid entries j_1..j_n in ascending position order, per feature f:
 *   sum  = ((0 + x[j_1,f]) + x[j_2,f]) + ...          mean = sum / (float)n
 *   min, max: over the candidates that are numbers; the first is taken whatever it is (+-inf too), then the first strictly
 *          smaller / larger value wins, so the lowest position keeps a tie (R4); a NaN never wins and never blocks
 *   var  = (((0 + d_1*d_1) + d_2*d_2) + ...) / (float)n with d_e = x[j_e,f] - mean: a second walk over the row, centred
 *          on the row's own mean (error at most (2n+8) u var + ((n+2) u mean|x|)^2, u = 2^-24)
 *   std  = s = sqrtf(var < 1e-5f ? 1e-5f : var), 0 where s <= sqrtf(1e-5f): the clamp keeps a NaN, so std is NaN where var
 *          is (a clamp lane); sum, mean and var are sum lanes
 *   out[Nt, G, A, F/G]: statistic a of feature f at out[i, f / (F/G), a, f % (F/G)].  count[Nt] int32 = n.  n == 0: every
 *   statistic 0 exactly (R3).  mean[Nt, F], var[Nt, F] (required with var or std, optional else), argmin[Nt, F] int32
 *   (required with min), argmax[Nt, F] (required with max): the winner's position, -1 in an empty row.  A feature of a
 *   non-empty row whose candidates are all NaN gives min / max = NaN with position -1.
 * dmet_multi_aggr_bwd_f32: one launch per target forms c1[i,f] = (2 g_v) / n and c0[i,f] = (g_sum + g_mean / n) -
 *   c1 mean, g_v = g_var + g_std / (2 std) where var > 1e-5 and std > 0, g_v = g_var otherwise, 0 and 0 for n == 0 (c0,
 *   c1: caller's work rows [Nt, F]; c1 only with var or std); then by source j over the positions p of the by-source
 *   index rev_ptr[Ns+1], rev_pos[] (dmet_reverse_index over idx) in ascending order, i = p / width or tgt[p]:
 *   g_x[j,f] = acc + ((((c1[i,f] * x[j,f]) + c0[i,f]) + [argmin[i,f] == p] g_min[i,f]) + [argmax[i,f] == p] g_max[i,f])
 *   g_out has out's layout.  A source nobody lists gets 0.  A long list is walked by its one owner.
 * No float atomics; sums run in a fixed order, two runs give identical bits; every element of every output is written.
 * Rows are read and written 16 bytes at a time where F % 4 == 0, (F/G) % 4 == 0 and every row tensor starts on a 16-byte
 * boundary, element by element otherwise, with the same bits.
 * Both return -EINVAL on bad arguments before any device work.  Nt == 0: the forward returns 0 at once; the backward
 * zero-fills g_x (Ns > 0) and returns. */
int dmet_multi_aggr_fwd_f32(const float *x, const int32_t *idx, const int32_t *rowptr, int64_t Nt, int64_t Ns, int64_t E,
                            int width, int F, int G, int aggrs, float *out, int32_t *count, float *mean, float *var,
                            int32_t *argmin, int32_t *argmax, dmet_stream_t stream);
int dmet_multi_aggr_bwd_f32(const float *x, const float *g_out, const int32_t *count, const float *mean, const float *var,
                            const int32_t *argmin, const int32_t *argmax, const int32_t *tgt, const int32_t *rev_ptr,
                            const int32_t *rev_pos, int64_t Nt, int64_t Ns, int64_t E, int width, int F, int G, int aggrs,
                            float *c0, float *c1, float *g_x, dmet_stream_t stream);
/* ---- Weighted aggregation: out_i = sum_e w_e x[src(e)] with a gradient into the edge weights ---------------------------
 * replaces torch_geometric's propagate(edge_index, x=x, edge_weight=edge_weight) under aggr='add' -- message
 * (return x_j if edge_weight is None else edge_weight.view(-1, 1) * x_j) and the scatter sum, in GCNConv, GraphConv,
 * SAGEConv and GINConv -- and torch_sparse.spmm(index, value, m, n, matrix) (out = matrix[col] * value.unsqueeze(-1);
 * scatter_add(out, row, dim=0, dim_size=m)), with their autograd graph: the index_select, the [E, F] product, an
 * index_add_ with float atomics and a host read of E (csrc/weighted_sum.hip).
 * The graph is the multi-aggregation section's: width >= 1 is a table idx = nbr[Nt, width] (1 <= width <= DMET_MAX_K,
 *   position p = i*width + t belongs to target i, E and rowptr are ignored); width == 0 is an edge list grouped by
 *   target, idx = src[E], rowptr[Nt+1] (clamped to [0, E]), any in-degree; the backward also takes tgt[E].  -1 and an id
 *   outside [0, Ns) are no entry; a duplicate id counts once per slot.
 * x[Ns, F] fp32, 1 <= F <= 256.  w[Nt*width] or w[E] fp32, one scalar per position, or NULL: weight 1.  The value of w in
 *   an empty slot is never read into a result: a NaN there changes nothing.
 * dmet_weighted_sum_fwd_f32, for target i with valid entries e_1..e_n in ascending position order, per feature f:
 *   out[i,f] = fmaf(w_e, x[j_e,f], acc) from acc = 0; with w == NULL the step is acc + x[j_e,f], the bits of w all ones.
 *   count[Nt] int32 = n (may be NULL).  n == 0: out[i,:] = 0 exactly (R3), count 0.  out is a sum lane: a non-finite
 *   x[j,f] or w_e shows in the rows that hold it (feature f, or every feature) and nowhere else.
 * dmet_weighted_sum_bwd_f32 runs up to two launches:
 *   by source, when g_x != NULL: for source j over the positions p of the by-source index rev_ptr[Ns+1], rev_pos[]
 *     (dmet_reverse_index over idx) in ascending order, i = p / width or tgt[p]:
 *     g_x[j,f] = fmaf(w_p, g_out[i,f], acc).  A source nobody lists gets 0.  A long list is walked by its one owner.
 *   by target, when g_w != NULL: for every position p of row i with j = src(p):  g_w[p] = sum_f g_out[i,f] x[j,f] -- a
 *     lane adds the products of its four consecutive features in ascending order from 0, then an xor butterfly runs over
 *     the row's 16, 32 or 64 lanes (F <= 64, <= 128, <= 256): one product rounding, at most 4 + 6 additions.  Every
 *     position is written; an empty slot gets 0.
 *   g_x and g_w are each optional (rev_ptr / rev_pos are read only for g_x, x only for g_w); both NULL is -EINVAL.
 * No float atomics: sums run in a fixed order, two runs give identical bits.  Every element of out, count, g_x and g_w is
 * written, not accumulated.  Rows are read and written 16 bytes at a time where F % 4 == 0 and every row tensor starts
 * on a 16-byte boundary, element by element otherwise, with the same bits.
 * Both return -EINVAL on bad arguments (NULL pointers, negative sizes, F or width out of range, a list without rowptr or,
 * in the backward, without tgt) before any device work.  Nt == 0: the forward returns 0 at once; the backward zero-fills
 * g_x (Ns > 0) and returns. */
int dmet_weighted_sum_fwd_f32(const float *x, const float *w, const int32_t *idx, const int32_t *rowptr, int64_t Nt,
                              int64_t Ns, int64_t E, int width, int F, float *out, int32_t *count, dmet_stream_t stream);
int dmet_weighted_sum_bwd_f32(const float *x, const float *w, const float *g_out, const int32_t *idx, const int32_t *rowptr,
                              const int32_t *tgt, const int32_t *rev_ptr, const int32_t *rev_pos, int64_t Nt, int64_t Ns,
                              int64_t E, int width, int F, float *g_x, float *g_w, dmet_stream_t stream);
/* ---- PointNet convolution: fused set abstraction -------------------------------------------------------------------
 * replaces torch_geometric.nn.PointNetConv.forward for local_nn = Sequential(Linear(F + D, H1), act, Linear(H1, H2)
 * [, act]) and aggr = 'max': remove_self_loops + add_self_loops on the edge index, message
 * (msg = pos_j - pos_i; msg = torch.cat([x_j, msg], dim=1); return self.local_nn(msg)) and the scatter max, with their
 * autograd graph: the [E, F + D] features, the [E, H1] and [E, H2] activations and a host read of E
 * (csrc/pointnet.hip).
 * Inputs: x_src[Ns, F] (NULL when F == 0), pos_src[Ns, D], pos_dst[Nt, D], W1[H1, F + D] = [W1x | W1p], b1[H1] or NULL,
 *   W2[H2, H1], b2[H2] or NULL; fp32, contiguous, row-major as torch.nn.Linear.weight.  0 <= F <= 128, 1 <= D <= 8,
 *   1 <= H1 <= 128, H2 in {16, 32, 64, 128}: dmet_pointnet_supported(F, D, H1, H2) returns 1 for these, 0 otherwise.
 *   act: 0 ReLU, 1 ELU (alpha 1; expm1f below 0), used in both places; act2: 1 applies it after the second Linear too.
 * The graph in one of two forms:
 *   table (rowptr == NULL): idx = nbr[Nt, width] int32, 1 <= width <= DMET_POINTNET_MAX_WIDTH; an id outside [0, Ns) is
 *     an empty slot, anywhere in a row; with cnt[Nt] (may be NULL) the slots at or beyond cnt[i] are never read; E is
 *     ignored.
 *   list  (rowptr != NULL): rowptr[Nt+1], idx = src[E], tgt[E] int32 grouped by target, any in-degree; width and cnt are
 *     ignored; src / tgt may be NULL when E == 0.
 *   self_loop = 1 (legal only with Ns == Nt, one node set): entries with src == i are skipped and one implicit entry
 *     i -> i is taken after the row's own entries -- remove_self_loops + add_self_loops without rewriting the graph.
 * dmet_pointnet_fwd_f32, in evaluation order:
 *   s[j,c] = fmaf chain over f ascending from b1[c] of x_src[j,f] W1[c,f]            (written only with self_loop)
 *   p[n,c] = fmaf chain over d ascending from 0 of pos[n,d] W1[c,F+d]
 *   a[Ns,H1] = s + p over the sources,  b[Nt,H1] = p over the targets            (the caller's buffers, kept for backward)
 *   h1_e = act(a[src(e)] - b[i]) for an entry e of target i;  h1 = act(s[i]) for the implicit entry: a position
 *     difference of exactly 0
 *   z2_e[o] = b2[o] + sum_c h1_e[c] W2[o,c]   on v_mfma_f32_16x16x4_f32, c in the order 16 B + 4 q + t for B, then t = 0..3,
 *     then the matrix core's own q = 0..3;  m_e = act(z2_e) when act2 else z2_e
 *   out[i,o] = max_e m_e[o] over the row's entries in entry order, strict compares: the earliest entry wins a tie (R4).
 *     A max lane: over the messages that are numbers, wherever in the row and in whichever quarter of the wavefront an
 *     entry stands; a channel of a target with entries whose messages are all NaN gives NaN with win -1.  (ReLU is
 *     v > 0 ? v : 0, so it turns a NaN pre-activation into 0; ELU carries it on.)
 *   win[Nt,H2] int32: the winning table slot t (table) or grouped list position (list), -2 for the implicit entry, -1
 *     for a target without an entry, whose out row is exactly 0 (R3).  Nothing per edge is written.
 * dmet_pointnet_bwd_f32, with g_z2[i,o] = g_out[i,o] act'(out[i,o]) (act2; else g_out[i,o]) routed to entry win[i,o]:
 *   g_pre1_e = (sum_o g_z2_e[o] W2[o,:]) act'(h1_e), h1_e formed again as above.
 *   by target: g_b[i] = -sum_e g_pre1_e over the row's own entries, g_s[i] = g_pre1 of the implicit entry (self_loop),
 *     g_W2 = sum g_z2_e^T h1_e and g_b2 = sum g_z2 as one partial per workgroup, added in workgroup order in double.
 *   by source, over the by-source index rev_ptr[Ns+1], rev_pos[] in ascending order -- dmet_reverse_index(nbr, Nt*width,
 *     Ns) for a table (i = pos / width), dmet_reverse_index(src, E, Ns) for a list (i = tgt[pos]):  g_a[j] = sum g_pre1_e.
 *     Four consecutive sources share a wavefront and its tiles of 16 positions; a long list is walked by its one owner.
 *   node level: g_x = (g_a + g_s) W1x, g_pos_src = g_a W1p, g_pos_dst = g_b W1p (g_x, g_pos_src, g_pos_dst, g_W2, g_b2
 *     may each be NULL: not wanted).  g_a[Ns,H1], g_b[Nt,H1], g_s[Nt,H1] are the caller's buffers and outputs:
 *     g_W1 = [(g_a + g_s)^T x_src | g_a^T pos_src + g_b^T pos_dst] and g_b1 = column sums of g_a + g_s follow through
 *     dmet_xty_f32 on the caller's side.
 *   Every gradient element is written, not accumulated; the backward zero-fills the source-side gradients (g_a, g_x,
 *   g_pos_src) first, so a source nobody lists gets exact zeros.  No float atomics: two runs give identical bits, and a
 *   table and a list holding the same entries in the same order give identical bits (the tiles of 16 are cut from the
 *   entry numbers of a row: a table's valid slots come first, as in every table this library builds).
 * ws: dmet_pointnet_workspace_bytes(F, D, H1, H2) bytes (0 for unsupported widths).
 * Both return -EINVAL before any device work on NULL or negative arguments, unsupported widths, a width outside the
 * limit and self_loop with Ns != Nt.  Nt == 0: the forward returns 0 at once; the backward zero-fills the source-side
 * gradients, g_W2 and g_b2 and returns. */
#define DMET_POINTNET_MAX_WIDTH 1024
int dmet_pointnet_supported(int F, int D, int H1, int H2);
size_t dmet_pointnet_workspace_bytes(int F, int D, int H1, int H2);
int dmet_pointnet_fwd_f32(const float *x_src, const float *pos_src, const float *pos_dst, const int32_t *idx,
                          const int32_t *rowptr, const int32_t *cnt, int64_t Nt, int64_t Ns, int64_t E, int width, int F,
                          int D, const float *W1, const float *b1, int H1, const float *W2, const float *b2, int H2, int act,
                          int act2, int self_loop, float *a, float *b, float *s, float *out, int32_t *win, void *ws,
                          size_t ws_bytes, dmet_stream_t stream);
int dmet_pointnet_bwd_f32(const float *a, const float *b, const float *s, const float *out, const int32_t *win,
                          const float *g_out, const int32_t *idx, const int32_t *rowptr, const int32_t *tgt,
                          const int32_t *cnt, const int32_t *rev_ptr, const int32_t *rev_pos, int64_t Nt, int64_t Ns,
                          int64_t E, int width, int F, int D, const float *W1, int H1, const float *W2, int H2, int act,
                          int act2, int self_loop, float *g_a, float *g_b, float *g_s, float *g_x, float *g_pos_src,
                          float *g_pos_dst, float *g_W2, float *g_b2, void *ws, size_t ws_bytes, dmet_stream_t stream);
/* Reverse index: a stable sort of the positions 0..M-1 of an int32 key array by key value.
 *   rev_ptr[num_keys+1]: rev_pos[rev_ptr[j] .. rev_ptr[j+1]-1] = the positions holding key j, ascending.
 * Keys outside [0, num_keys) (the -1 "no neighbour" entries) sort last and are not indexed.
 * For a neighbour table pass keys = nbr, M = N*k, num_keys = N (position = i*k+s). */
size_t dmet_reverse_index_workspace_bytes(int64_t M, int64_t num_keys);
int dmet_reverse_index(const int32_t *keys, int64_t M, int64_t num_keys, int32_t *rev_ptr,
                       int32_t *rev_pos, void *ws, size_t ws_bytes, dmet_stream_t stream);

/* ---- K2 / K3 un-fused: arbitrary `nn`, arbitrary edge lists ------------------------------------------
 * replaces the PyG MessagePassing.propagate pieces around a user `nn`
 *   (model/dynamic_reduction_network.py:59-73,86-87: Linear-ELU-Linear-ELU-BN, aggr in {'add','max'}).
 * Edges are (src[e] -> tgt[e]) int32, grouped by target: rowptr[N+1] int32 with tgt[e]==i for
 * rowptr[i] <= e < rowptr[i+1], and 0 <= src[e] < N for every e: these entry points, and the edge-MLP ones above that
 * take the same list, index x / P / Q with src unchecked.  A table's -1 slots must not reach them (build the list with
 * the rowptr of dmet_table_degree, which drops them).
 *   edge_features: feat[e] = [ x[tgt[e]] || x[src[e]] - x[tgt[e]] ]                      ([E, 2H])
 *   segment_max  : out[i,c] = max_e msg[e,c] (empty -> 0), arg[i,c] = winning e (lowest on ties), -1 if empty
 *   segment_sum  : out[i,c] = sum_e msg[e,c] in ascending e (deterministic)
 *   segment_max_bwd: g_msg[e,c] = (arg[tgt(e),c]==e) ? g_out[tgt(e),c] : 0
 *   edge_features_bwd: gx[i] = sum_{e in in(i)} (g_feat[e,:H] - g_feat[e,H:]) + sum_{e in out(i)} g_feat[e,H:]
 *                      out(i) walked through the by-source index srcptr[N+1], srcperm[E] (ascending e). */
int dmet_edge_features_f32(const float *x, const int32_t *src, const int32_t *tgt, int64_t E, int H,
                           float *feat, dmet_stream_t stream);
int dmet_segment_max_f32(const float *msg, const int32_t *rowptr, int64_t N, int H, float *out,
                         int32_t *arg, dmet_stream_t stream);
int dmet_segment_sum_f32(const float *msg, const int32_t *rowptr, int64_t N, int H, float *out,
                         dmet_stream_t stream);
int dmet_segment_max_bwd_f32(const float *g_out, const int32_t *arg, const int32_t *rowptr, int64_t N,
                             int H, float *g_msg, dmet_stream_t stream);
int dmet_segment_sum_bwd_f32(const float *g_out, const int32_t *rowptr, int64_t N, int H, float *g_msg,
                             dmet_stream_t stream);
int dmet_edge_features_bwd_f32(const float *g_feat, const int32_t *rowptr, const int32_t *srcptr,
                               const int32_t *srcperm, int64_t N, int H, float *gx,
                               dmet_stream_t stream);

/* ---- segment reductions over long and short rows (csrc/segment.hip) -------------------------------------
 * The rest of the scatter family over fp32 rows src[E,H] (a 1-D src: H = 1) grouped by rowptr[rows+1] int32: row i owns
 * the positions [rowptr[i], rowptr[i+1]), each span clamped to [0, E].  A wavefront owns a (row, block of channels) pair;
 * max_len is a hint of the longest row: from 1024 on a 256-thread workgroup owns the pair instead, 0 means unknown and
 * selects the wavefront form.  Either form takes rows of any length; the two agree to rounding, not in bits.  No float
 * atomics, every output element written once, sums in an order fixed by H and the form: same bits run to run.
 *   mean         : out[i,c] = (sum_e src[e,c]) / max(n_i, 1)                              (empty -> 0)
 *   mean_bwd     : g_src[e,c] = g_out[i,c] / max(n_i, 1)
 *   min          : out[i,c] = min_e src[e,c] (empty -> 0), arg[i,c] = winning e (lowest on ties), -1 if empty; the
 *                  backward is dmet_segment_max_bwd_f32 (the same arg convention)
 *   softmax_fwd  : m = max_e s, l = sum_e expf(s - m) in one online pass; then y[e,c] = expf(s - m) / l, or with log != 0
 *                  y = (s - m) - logf(l); lse[i,c] = m + logf(l) (empty -> 0).  A row of -inf alone gives NaN, a -inf
 *                  beside finite scores exactly 0 (softmax).
 *   softmax_bwd  : g_src = y * (g - sum_row y*g), or with log != 0 g_src = g - expf(y) * sum_row g     (g is [E,H])
 *   logsumexp    : out[i,c] = m + logf(l)                                                  (empty -> 0)
 *   logsumexp_bwd: g_src[e,c] = g_out[i,c] * expf(src[e,c] - out[i,c])
 * The per-entry outputs (y, g_src) are zero at positions before rowptr[0] and from rowptr[rows] on.  rowptr must be
 * non-decreasing for them to be fully written: where it is not, positions in a gap between two rows are left as the
 * caller allocated them and positions two rows share are written by both (in bounds; not defined, not reproducible). */
int dmet_segment_mean_f32(const float *src, const int32_t *rowptr, int64_t rows, int64_t E, int H, int max_len,
                          float *out, dmet_stream_t stream);
int dmet_segment_mean_bwd_f32(const float *g_out, const int32_t *rowptr, int64_t rows, int64_t E, int H, int max_len,
                              float *g_src, dmet_stream_t stream);
int dmet_segment_min_f32(const float *src, const int32_t *rowptr, int64_t rows, int64_t E, int H, int max_len,
                         float *out, int32_t *arg, dmet_stream_t stream);
int dmet_segment_softmax_fwd_f32(const float *src, const int32_t *rowptr, int64_t rows, int64_t E, int H, int log,
                                 int max_len, float *y, float *lse, dmet_stream_t stream);
int dmet_segment_softmax_bwd_f32(const float *y, const float *g, const int32_t *rowptr, int64_t rows, int64_t E, int H,
                                 int log, int max_len, float *g_src, dmet_stream_t stream);
int dmet_segment_logsumexp_f32(const float *src, const int32_t *rowptr, int64_t rows, int64_t E, int H, int max_len,
                               float *out, dmet_stream_t stream);
int dmet_segment_logsumexp_bwd_f32(const float *src, const float *out, const float *g_out, const int32_t *rowptr,
                                   int64_t rows, int64_t E, int H, int max_len, float *g_src, dmet_stream_t stream);
/* ---- event normalisation: per-event column statistics and one elementwise pass (csrc/event_norm.hip) ----
 * fp32 rows x[N,F] grouped by rowptr[B+1] int32: event b owns the rows [rowptr[b], rowptr[b+1]), each span clamped to
 * [0, N]; n_b is its length.  Any F >= 1 and any event length.  moments and dots: a team owns an (event, block of
 * channels) pair; it is one wavefront, and from a max_len hint (the longest event; 0 = unknown) of 1024 on a 1024-thread
 * workgroup, for every event of the call.  Either form takes events of any length; the two agree to rounding, not in
 * bits.  No float atomics, no scratch, every output element written once, sums in an order fixed by F and the form: same
 * bits run to run and on unaligned pointers.
 *   moments: mean[b,c] = (fp32 sum_n x[n,c]) / (float)n_b  (one division);
 *            var[b,c] = (sum_n d*d) / (float)n_b with d = x[n,c] - mean[b,c], taken in a second walk over the event's rows
 *            centred on its own rounded mean (never a difference of two means).  Empty event: mean = var = 0.
 *   dots   : s1[b,c] = sum_n g[n,c];  s2[b,c] = sum_n g[n,c] * ((x[n,c] - shift[b,c]) * scale[b,c]), every operation
 *            rounded once.  Empty event: 0.  x, shift, scale and s2 may be NULL together: s1 alone.
 *   affine : out[n,c] = (x[n,c] - shift[b,c]) * k1[b,c] + k0[b,c]; with g and ka (NULL together or neither):
 *            out[n,c] = g[n,c] * ka[b,c] + ((x[n,c] - shift[b,c]) * k1[b,c] + k0[b,c]); every operation rounded once, in
 *            that order.  Rows before rowptr[0] and from rowptr[B] on are written as zeros.  A workgroup owns a run of
 *            rows and finds the event of its first row by one search.
 * B == 0 (all three) and N == 0 (affine) return without a launch; bad sizes and NULL pointers return -22 before any
 * launch.  rowptr must be non-decreasing: a row whose end lies before its start is empty to moments and dots; affine leaves
 * the rows in a gap between two events as the caller allocated them and writes rows two events share twice (in bounds; not
 * defined, not reproducible).  A malformed rowptr never causes an access outside x, g or out. */
int dmet_event_moments_f32(const float *x, const int32_t *rowptr, int64_t B, int64_t N, int F, int max_len, float *mean,
                           float *var, dmet_stream_t stream);
int dmet_event_dots_f32(const float *g, const float *x, const int32_t *rowptr, int64_t B, int64_t N, int F, int max_len,
                        const float *shift, const float *scale, float *s1, float *s2, dmet_stream_t stream);
int dmet_event_affine_f32(const float *x, const float *g, const int32_t *rowptr, int64_t B, int64_t N, int F,
                          const float *shift, const float *k1, const float *k0, const float *ka, float *out,
                          dmet_stream_t stream);
/* The same two pieces for TWO node sets (EdgeConv((x_src, x_dst), edge_index)): src[e] indexes x_src[N_src,H], tgt[e]
 * indexes x_dst[N_dst,H], edges grouped by target (rowptr[N_dst+1]); both ids unchecked, so 0 <= src[e] < N_src and
 * 0 <= tgt[e] < N_dst must hold for every e (a table's -1 slots are dropped before, dmet_table_degree).  Any H > 0.
 *   edge_features_xy: feat[e] = [ x_dst[tgt[e]] || x_src[src[e]] - x_dst[tgt[e]] ]          ([E, 2H])
 *   edge_features_xy_bwd: g_x_dst[i] = sum_{e in in(i)} (g_feat[e,:H] - g_feat[e,H:])   (by rowptr, ascending e)
 *                         g_x_src[j] = sum_{e in out(j)} g_feat[e,H:]   (by srcptr[N_src+1], srcperm[E]: ascending e)
 *   either output may be NULL (not wanted).  Same bits run to run. */
int dmet_edge_features_xy_f32(const float *x_src, const float *x_dst, const int32_t *src, const int32_t *tgt, int64_t E,
                              int H, float *feat, dmet_stream_t stream);
int dmet_edge_features_xy_bwd_f32(const float *g_feat, const int32_t *rowptr, const int32_t *srcptr,
                                  const int32_t *srcperm, int64_t N_src, int64_t N_dst, int H, float *g_x_src,
                                  float *g_x_dst, dmet_stream_t stream);

/* ---- K4: per-event MET reduction -------------------------------------------------------------------
 * replaces the two torch_scatter.scatter_add calls at model/net.py:55-56 (and :132-133):
 *   met[b,0] = sum_{i in event b} w[i]*x[i*x_stride+0],  met[b,1] = sum w[i]*x[i*x_stride+1]
 * Deterministic fixed-shape tree (one workgroup per event; lane-strided partials, wavefront shuffle
 * tree, then waves in order).  bwd: g_w[i] = g_met[b,0]*px_i + g_met[b,1]*py_i. */
int dmet_met_reduce_f32(const float *w, const float *x, int64_t x_stride, const int64_t *ptr, int B,
                        float *met, dmet_stream_t stream);
int dmet_met_reduce_bwd_f32(const float *g_met, const float *x, int64_t x_stride, const int64_t *ptr,
                            int B, int64_t N, float *g_w, dmet_stream_t stream);
/* H1: torch.optim.AdamW's step (train.py:52,75; decoupled weight decay, no amsgrad) on one flat fp32 tensor, one launch.
 * Device-side step state, advanced by the launch (replayable in a hipGraph): step[0] = number of steps taken (float),
 * bias_pow[2] = beta1^step, beta2^step as running products in double (both 1.0 before the first step).
 * Hyper-parameters are doubles (python floats): 1 - beta is formed before the rounding to fp32, as torch does. */
int dmet_adamw_f32(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, float *step, double *bias_pow,
                   int64_t n, double lr, double beta1, double beta2, double eps, double weight_decay,
                   dmet_stream_t stream);
/* Same with the learning rate read from device memory (lr_dev[0], double): the reference drives it with
 * ReduceLROnPlateau (train.py:76, stepped at train.py:58), and a launch captured in a hipGraph must see the change. */
int dmet_adamw_lr_f32(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, float *step, double *bias_pow,
                      int64_t n, const double *lr_dev, double beta1, double beta2, double eps, double weight_decay,
                      dmet_stream_t stream);
/* loss[0] = 0.5 * mean_b((met[b,0] + truth[b,0])^2 + (met[b,1] + truth[b,1])^2)  (model/net.py:58-61) and
 * g_met[B,2] = d loss / d met, one launch, fixed summation order. */
int dmet_met_loss_f32(const float *met, const float *truth, int B, float *loss, float *g_met, dmet_stream_t stream);
/* The same two entries for the fused loss of model/net.py:49-62 (deepmetv2_amd.scatter.met_loss_from_weights): truth rows
 * of truth_stride floats (px, py in columns 0, 1 of the [B,11] target: no [B,2] copy), and the backward with g_met
 * multiplied by one device float first (the upstream gradient of the scalar loss: no separate multiply). */
int dmet_met_loss_strided_f32(const float *met, const float *truth, int64_t truth_stride, int B, float *loss,
                              float *g_met, dmet_stream_t stream);
int dmet_met_reduce_bwd_scaled_f32(const float *g_met, const float *scale, const float *x, int64_t x_stride,
                                   const int64_t *ptr, int B, int64_t N, float *g_w, dmet_stream_t stream);
/* Generic sorted-index form used by the scatter_add(src, batch) drop-in: out[b] = sum_{i in b} src[i]. */
int dmet_segment_sum_1d_f32(const float *src, const int64_t *ptr, int B, float *out,
                            dmet_stream_t stream);
/* Neighbour table -> edge list (what knn_graph / radius_graph return): deg[i] = valid entries of row i (among the
 * first cnt[i] slots when cnt is given); with rowptr = exclusive prefix sum of deg, dmet_table_edges writes the edges
 * grouped by target i in slot order: first/second [E] int64 = (source, target), or (target, source) when swap != 0,
 * and/or src32/tgt32 [E] int32.  A row given exactly k edges by rowptr is copied slot for slot, -1 slots included (the
 * sync-free rowptr = i k of a table expected to be full); such a list is no input of the edge-list entry points. */
int dmet_table_degree(const int32_t *nbr, const int32_t *cnt, int64_t N, int k, int32_t *deg, dmet_stream_t stream);
int dmet_table_edges(const int32_t *nbr, const int32_t *cnt, const int32_t *rowptr, int64_t N, int k, int swap,
                     int64_t *first, int64_t *second, int32_t *src32, int32_t *tgt32, dmet_stream_t stream);
/* ptr[B+1] from a SORTED int64 batch vector with values in [0, B) (ptr[b] = first i with batch[i] >= b).  Safe for any
 * int64 input: only ptr[0..B] is written, and all of it; for an unsorted vector or values outside [0, B) the content
 * is unspecified (and may differ between runs), so the caller validates the vector before using ptr. */
int dmet_batch_to_ptr(const int64_t *batch, int64_t N, int B, int64_t *ptr, dmet_stream_t stream);

/* ---- N3 (first piece): weight gradients of the per-node dense layers ----------------------------------
 * The layers around the graph operators (model/graph_met_network.py:15-32,41-44) are tiny per-node Linear /
 * Embedding modules over N ~ 3e5 nodes; autograd's weight gradients for them are tall-skinny reductions
 *   C[Ha,Hb] = A^T B,  A = grad_out[N,Ha], B = input[N,Hb]        (torch Linear.weight layout [out,in])
 *   C[R,Hb]  = onehot(index[N])^T B                                (torch Embedding.weight gradient)
 * computed deterministically (fixed row ranges per wavefront, partials summed in order), Ha,Hb,R <= 64. */
size_t dmet_xty_workspace_bytes(int64_t N, int Ha, int Hb);
int dmet_xty_f32(const float *A, const float *B, int64_t N, int Ha, int Hb, float *C, void *ws,
                 size_t ws_bytes, dmet_stream_t stream);
int dmet_onehot_xty_f32(const int64_t *index, const float *B, int64_t N, int R, int Hb, float *C, void *ws,
                        size_t ws_bytes, dmet_stream_t stream);

/* ---- N3 (second piece): the per-node encoder as one kernel each way ---------------------------------------
 * model/graph_met_network.py:48-58 up to (not including) bn_all:
 *   h = ELU(Wa [ELU(Wk [Echg[chg+1] | Epdg[remap(|pdg|)] | Epv[pv]] + bk) | ELU(Wc x[:, :8] + bc)] + ba)
 * x[N,8] fp32 continuous columns with row stride x_stride floats (a view into the 11-column feature matrix is
 * fine); x_cat[N,3] int64 = (pdgId, charge, fromPV), the arguments of GraphMETNetwork.forward -- or x_cat == NULL:
 * the three columns are columns 8..10 of the same rows of x (x_stride >= 11), still as floats, and the `.long()` of
 * train.py:43 (truncation toward zero) happens inside the kernel.  Torch layouts
 * for the weights (Linear.weight [out,in], Embedding.weight [rows,8]).  Backward takes the forward output h and g_h = dL/dh and
 * writes (not accumulates) all nine parameter gradients, reduced over the nodes deterministically. */
int dmet_encode_fwd_f32(const float *x, int64_t x_stride, const int64_t *x_cat, int64_t N, const float *Wc, const float *bc,
                        const float *Wk, const float *bk, const float *Wa, const float *ba, const float *Echg,
                        const float *Epdg, const float *Epv, float *h, dmet_stream_t stream);
size_t dmet_encode_bwd_workspace_bytes(int64_t N);
int dmet_encode_bwd_f32(const float *x, int64_t x_stride, const int64_t *x_cat, int64_t N, const float *Wc, const float *bc,
                        const float *Wk, const float *bk, const float *Wa, const float *ba, const float *Echg,
                        const float *Epdg, const float *Epv, const float *h, const float *g_h, float *gWc,
                        float *gbc, float *gWk, float *gbk, float *gWa, float *gba, float *gEchg, float *gEpdg,
                        float *gEpv, void *ws, size_t ws_bytes, dmet_stream_t stream);
/* dmet_encode_bwd_f32 behind bn_all (model/graph_met_network.py:58): g_y is the gradient with respect to the
 * BatchNorm's OUTPUT and the BatchNorm's backward transform g = gamma * invstd * (g_y - mean_g - (h - mean) * invstd *
 * mean_gx) (statistics from dmet_bn_bwd_stats_f32; h, the BatchNorm's input, is the encoder's own output) is applied
 * as the rows are loaded: the transform pass of dmet_bn_bwd_f32 disappears.  *fused = 0: nothing was launched
 * (DMET_ENCODER_BWD=valu, misaligned operands) and the caller keeps the two steps. */
int dmet_encode_bn_bwd_f32(const float *x, int64_t x_stride, const int64_t *xcat, int64_t N, const float *Wc,
                           const float *bc, const float *Wk, const float *bk, const float *Wa, const float *ba,
                           const float *Echg, const float *Epdg, const float *Epv, const float *h, const float *g_y,
                           const float *bn_gamma, const float *bn_mean, const float *bn_invstd, const float *bn_mean_g,
                           const float *bn_mean_gx, float *gWc, float *gbc, float *gWk, float *gbk, float *gWa,
                           float *gba, float *gEchg, float *gEpdg, float *gEpv, int *fused, void *ws, size_t ws_bytes,
                           dmet_stream_t stream);

/* ---- K5 (node level): backward of the fused EdgeConv dense layer, H = 32 -------------------------------------
 * With P = x (W1-W2)^T + b, Q = x W2^T, out_i = P_i + max_s Q[nbr[i,s]] (dmet_node_linear_split_f32 +
 * dmet_gather_max_f32) and gQ from dmet_gather_max_bwd_f32:
 *   gx = gP (W1-W2) + gQ W2,   gW[H,2H] = [gP^T x | gQ^T x - gP^T x],   gb = sum_i gP_i,
 * gP = g_out masked to 0 where arg == 255 (node without neighbour; arg may be NULL for dense tables).
 * One pass over the rows, fp32 MFMA, deterministic (fixed node ranges per wavefront, ordered partial sums). */
size_t dmet_edgeconv_linear_bwd_workspace_bytes(int64_t N, int H);
int dmet_edgeconv_linear_bwd_f32(const float *x, const float *W, const float *g_out, const uint8_t *arg,
                                 const float *gQ, int64_t N, int H, float *gx, float *gW, float *gb, void *ws,
                                 size_t ws_bytes, dmet_stream_t stream);
/* Same with gx += g_add[N,H] fused into the store (g_add may be NULL): the gradient that reaches x through the
 * residual connection of the block (graph_met_network.py:66: emb = emb + norm(conv(emb))), instead of a separate
 * elementwise add over the node table. */
int dmet_edgeconv_linear_bwd_add_f32(const float *x, const float *W, const float *g_out, const uint8_t *arg,
                                     const float *gQ, const float *g_add, int64_t N, int H, float *gx, float *gW,
                                     float *gb, void *ws, size_t ws_bytes, dmet_stream_t stream);
/* Same for the winner-id form of the counted radius gather (dmet_gather_max_local_j16_f32 / _counted_lds_j16_f32:
 * train.py:48's radius graph feeding model/graph_met_network.py:65): argj[N,H] uint16 event-local winner ids,
 * 0xFFFF = the node had no neighbour at all (a query with a NaN / inf coordinate finds nobody, not even itself);
 * gP is masked to 0 there exactly as for arg == 255 above.  argj may be NULL (no masking). */
int dmet_edgeconv_linear_bwd_add_j16_f32(const float *x, const float *W, const float *g_out, const uint16_t *argj,
                                         const float *gQ, const float *g_add, int64_t N, int H, float *gx, float *gW,
                                         float *gb, void *ws, size_t ws_bytes, dmet_stream_t stream);

/* ---- N3 (third piece): BatchNorm1d over the nodes, optionally fused with the residual add ---------------
 * model/graph_met_network.py:32,39,58,66: bn_all(...) and emb + bn(conv(...)).  x[N,H] row-major, H a multiple of 4
 * up to 64.  training != 0: batch statistics (biased variance for the normalisation, unbiased for running_var, like
 * torch.nn.BatchNorm1d); running_mean/var (optional pair) are updated in place with `momentum`.  training == 0:
 * running statistics.  y = (x - mean) * gamma / sqrt(var + eps) + beta (+ residual when not NULL).
 * save_mean / save_invstd [H] are written for the backward.  Column sums use fixed row ranges per workgroup and are
 * combined in order: bitwise reproducible.  Backward (training statistics): g_x, g_gamma, g_beta (written). */
size_t dmet_bn_workspace_bytes(int64_t N, int H);
int dmet_bn_fwd_f32(const float *x, const float *residual, int64_t N, int H, const float *gamma, const float *beta,
                    float eps, float momentum, float *running_mean, float *running_var, int training, float *y,
                    float *save_mean, float *save_invstd, void *ws, size_t ws_bytes, dmet_stream_t stream);
/* Same; in training mode *num_batches_tracked (optional, int64 on the device: nn.BatchNorm1d's buffer) is incremented by
 * the statistics kernel instead of by a kernel launch of its own. */
int dmet_bn_fwd_tracked_f32(const float *x, const float *residual, int64_t N, int H, const float *gamma,
                            const float *beta, float eps, float momentum, float *running_mean, float *running_var,
                            int64_t *num_batches_tracked, int training, float *y, float *save_mean, float *save_invstd,
                            void *ws, size_t ws_bytes, dmet_stream_t stream);
/* The statistics half of dmet_bn_bwd_f32 (column sums + finalize): g_gamma, g_beta and the two means the element
 * transform needs, for a caller that applies the transform elsewhere (dmet_encode_bn_bwd_f32). */
int dmet_bn_bwd_stats_f32(const float *x, const float *g_y, int64_t N, int H, const float *save_mean,
                          const float *save_invstd, float *g_gamma, float *g_beta, float *mean_g, float *mean_gx,
                          void *ws, size_t ws_bytes, dmet_stream_t stream);
/* Eval mode: save_mean = running_mean, save_invstd = 1 / sqrt(running_var + eps) (the constants dmet_bn_fwd_f32 uses with
 * training == 0), for callers that apply the transform elsewhere (dmet_bn_knn_local_dense_f32, dmet_bn_head_fwd_f32). */
int dmet_bn_eval_stats_f32(const float *running_mean, const float *running_var, int H, float eps, float *save_mean,
                           float *save_invstd, dmet_stream_t stream);
/* The transform half of dmet_bn_fwd_f32 with the statistics given (dmet_bn_stats_f32 / dmet_bn_eval_stats_f32):
 * y = (x - mean) * (gamma * invstd) + beta (+ residual when not NULL), the same kernel and therefore the same bits as
 * dmet_bn_fwd_f32 -- for a caller whose fused consumer (dmet_bn_knn_local_dense_f32, dmet_bn_head_fwd_f32) declined
 * after the statistics were computed (model/graph_met_network.py:58,66).  All pointers 16-byte aligned. */
int dmet_bn_apply_f32(const float *x, const float *residual, int64_t N, int H, const float *gamma, const float *beta,
                      const float *mean, const float *invstd, float *y, dmet_stream_t stream);
/* The statistics half of dmet_bn_fwd_tracked_f32 in training mode (column sums + finalize: save_mean, save_invstd,
 * running statistics, num_batches_tracked), for a caller that applies the transform elsewhere
 * (dmet_bn_knn_local_dense_f32 fuses it into the next layer's graph build). */
int dmet_bn_stats_f32(const float *x, int64_t N, int H, float eps, float momentum, float *running_mean, float *running_var,
                      int64_t *num_batches_tracked, float *save_mean, float *save_invstd, void *ws, size_t ws_bytes,
                      dmet_stream_t stream);
int dmet_bn_bwd_f32(const float *x, const float *g_y, int64_t N, int H, const float *gamma, const float *save_mean,
                    const float *save_invstd, float *g_x, float *g_gamma, float *g_beta, void *ws, size_t ws_bytes,
                    dmet_stream_t stream);

/* ---- N3 (fourth piece): the output head with its sigmoid ---------------------------------------------------
 * model/graph_met_network.py:41-44,67 + model/net.py:46:  out_i = sigmoid(W2 . ELU(W1 . emb_i + b1) + b2) with
 * emb[N,32], W1[16,32], b1[16], W2[1,16], b2[1] (torch layouts).  Backward takes the forward output and g_out[N] and
 * writes g_emb[N,32] and the four parameter gradients (reduced over the nodes deterministically). */
int dmet_head_fwd_f32(const float *emb, int64_t N, const float *W1, const float *b1, const float *W2, const float *b2,
                      float *out, dmet_stream_t stream);
/* The last block of the model, `emb = emb + bn(conv(emb))` followed by the head (model/graph_met_network.py:66-67): the
 * BatchNorm transform + residual add is formed inside the head's forward launch (expression and bits of
 * dmet_bn_fwd_f32's transform; statistics from dmet_bn_stats_f32), emb[N,32] is written for the backward.  *fused = 0:
 * nothing was launched (misaligned operands, DMET_HEAD_FWD=valu) and the caller keeps the two steps. */
int dmet_bn_head_fwd_f32(const float *raw, const float *residual, const float *gamma, const float *beta,
                         const float *mean, const float *invstd, float *emb, int64_t N, const float *W1,
                         const float *b1, const float *W2, const float *b2, float *out, int *fused,
                         dmet_stream_t stream);
size_t dmet_head_bwd_workspace_bytes(int64_t N);
int dmet_head_bwd_f32(const float *emb, int64_t N, const float *W1, const float *b1, const float *W2, const float *out,
                      const float *g_out, float *g_emb, float *gW1, float *gb1, float *gW2, float *gb2, void *ws,
                      size_t ws_bytes, dmet_stream_t stream);

/* ---- K5 / N3: the weight-gradient sums of a whole backward pass in one launch -----------------------------------
 * train.py:51-52 (`loss.backward(); optimizer.step()`): dmet_edgeconv_linear_bwd*_f32, dmet_encode_bwd_f32 /
 * dmet_encode_bn_bwd_f32 and dmet_head_bwd_f32 each end in a small second launch that adds the per-workgroup partials
 * of their parameter gradients in a fixed order; only the optimizer reads the results.  After
 * dmet_finalize_defer_begin() those calls -- from ANY thread of the process: an autograd engine runs them on a thread of
 * its own -- queue that step instead of launching it -- up to 8; a ninth
 * launches its own as before -- and dmet_finalize_flush(stream) forms every queued sum in ONE launch (the same
 * additions in the same order: same bits) and ends the deferral.  Contract: the gradient outputs and the workspaces of
 * the queued calls must stay allocated and untouched until the flush has been enqueued on the same stream; the outputs
 * hold garbage before it.  dmet_finalize_pending(): queued steps, -1 outside a deferral.  Beginning a deferral while sums
 * of an earlier one are still queued is refused (-22): they would never be formed. */
int dmet_finalize_defer_begin(void);
int dmet_finalize_pending(void);
int dmet_finalize_flush(dmet_stream_t stream);

/* ---- Graph coarsening: graclus matching, normalized-cut weights, pair pooling (csrc/pool.hip) -----------------------
 * replaces torch_cluster.graclus, torch_geometric.utils.normalized_cut and the cluster pooling of
 * torch_geometric.nn.max_pool / max_pool_x / avg_pool_x
 *   call sites: model/dynamic_reduction_network.py:89-92 (normalized_cut_2d, graclus, max_pool) and :97-99
 *   (normalized_cut_2d, graclus, max_pool_x).
 *
 * dmet_graclus_f32: greedy matching of torch_cluster's GPU algorithm (colour, propose, respond), deterministic.
 *   Graph: CSR rowptr[N+1] int64, col[E] int32 (row u lists its neighbours in ascending (row, col) order), optional
 *   weight[E] (NULL = unweighted).  Blocks: ptr[B+1] (events); one workgroup per block.  Edges whose endpoints lie in
 *   different blocks, or outside 0..N-1, are ignored; self loops (col == u) are ignored.
 *   All nodes start unmatched.  Round r = 0, 1, ... of a block, for every node u unmatched at the round's start:
 *     colour: s = (uint32)seed ^ (uint32)(seed >> 32), key_r = lowbias32(s + 0x9E3779B9u * r),
 *             red(u) = lowbias32((uint32)u ^ key_r) >> 31   (1 = red, 0 = blue), where
 *             lowbias32(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16.
 *     "best" of a candidate set in row u: scan the row in CSR order, take the first candidate and replace it only by a
 *             candidate of strictly greater weight (IEEE >); unweighted: the first candidate.
 *     a node with no unmatched neighbour (other than itself) becomes a singleton;
 *     propose: a blue node proposes to its best unmatched red neighbour (if any);
 *     respond: a red node accepts its best neighbour among the blue nodes that proposed to it: the two are matched.
 *   Rounds end when the block has no unmatched node at the start of a round.  After max_rounds rounds (0 = the default
 *   DMET_GRACLUS_DEFAULT_ROUNDS) the unmatched nodes are finished sequentially in ascending index: each is matched to
 *   its best unmatched neighbour, or made a singleton.  The kernel loops over a bounded number of rounds only.
 *   Outputs: cluster[N] int64 = min(u, v) for a matched pair (u, v), u for a singleton (torch_cluster's convention: u
 *   leads its cluster iff cluster[u] == u); partner[N] int32 = v, -1 for a singleton; rounds[B] int32 (may be NULL) =
 *   colour rounds the block ran (max_rounds when the finisher ran).  The result depends on (graph, weights, seed) only:
 *   colours are keyed by the global node id and the block's own round count, so one block per event and one block for
 *   a whole graph without edges across events give the same bits.  Block state is kept in LDS for blocks of up to
 *   DMET_GRACLUS_LDS_NODES nodes and in the workspace above that.
 *
 * dmet_normalized_cut_f32: w[e] = attr[e] * (1/deg(row[e]) + 1/deg(col[e])) in fp32, deg = in-degree counted over col
 *   (torch_geometric.utils.normalized_cut).  dmet_normalized_cut_2d_f32: the same with attr[e] = ||x[row[e]] -
 *   x[col[e]]||_2 for x[N,D], D <= DMET_MAX_CUT_DIM (the DRN's normalized_cut_2d, :89,97); squares summed in double,
 *   one rounding to fp32.  row / col: the two rows of an int64 edge_index; an out-of-range endpoint gives NaN.
 *
 * Pair pooling of a graclus result (partner[N] as written by dmet_graclus_f32; a node leads its cluster unless its
 *   partner is a lower index).  dmet_pool_pairs_index: cid[N] int64 = pooled row of every node, pooled_ptr[B+1] int64 =
 *   exclusive prefix sum over events b of the leaders in ptr[b] .. ptr[b+1]-1 (clusters are numbered in ascending leader
 *   index, so pooled rows stay grouped by event; a cluster belongs to its leader's event).  dmet_pool_pairs_f32 with
 *   C = pooled_ptr[B]: out_max[C,F] = the larger member row channel-wise, arg[C,F] int32 = its node (the leader on
 *   ties), out_mean[C,F] = (x_u + x_v) * 0.5 (x_u for a singleton), pooled_batch[C] int64 = event of the leader; any of
 *   the outputs may be NULL (out_max and arg together).  dmet_pool_pairs_bwd_f32: gx[u,f] = (arg[cid[u],f] == u ?
 *   g_max[cid[u],f] : 0) + g_mean[cid[u],f] * (1/2 for a pair, 1 for a singleton); g_max / g_mean may be NULL. */
#define DMET_GRACLUS_LDS_NODES 16384    /* blocks up to this size keep their matching state in LDS (128 KiB) */
#define DMET_GRACLUS_DEFAULT_ROUNDS 64
#define DMET_MAX_CUT_DIM 64
size_t dmet_graclus_workspace_bytes(int64_t N);
int dmet_graclus_f32(const int64_t *rowptr, const int32_t *col, const float *weight, const int64_t *ptr, int B,
                     int64_t N, uint64_t seed, int max_rounds, int64_t *cluster, int32_t *partner, int32_t *rounds,
                     void *ws, size_t ws_bytes, dmet_stream_t stream);
size_t dmet_normalized_cut_workspace_bytes(int64_t N);
int dmet_normalized_cut_f32(const int64_t *row, const int64_t *col, int64_t E, int64_t N, const float *attr, float *w,
                            void *ws, size_t ws_bytes, dmet_stream_t stream);
int dmet_normalized_cut_2d_f32(const int64_t *row, const int64_t *col, int64_t E, int64_t N, const float *x, int D,
                               float *w, void *ws, size_t ws_bytes, dmet_stream_t stream);
size_t dmet_pool_pairs_workspace_bytes(int64_t N, int B);
int dmet_pool_pairs_index(const int32_t *partner, const int64_t *ptr, int B, int64_t N, int64_t *cid,
                          int64_t *pooled_ptr, void *ws, size_t ws_bytes, dmet_stream_t stream);
int dmet_pool_pairs_f32(const float *x, int64_t N, int F, const int32_t *partner, const int64_t *cid, const int64_t *ptr,
                        int B, int64_t C, float *out_max, int32_t *arg, float *out_mean, int64_t *pooled_batch,
                        dmet_stream_t stream);
int dmet_pool_pairs_bwd_f32(const float *g_max, const int32_t *arg, const float *g_mean, const int32_t *partner,
                            const int64_t *cid, int64_t N, int F, int64_t C, float *gx, dmet_stream_t stream);

/* ---- Farthest point sampling: replaces torch_cluster.fps (csrc/fps.hip) ----------------------------------------------
 * dmet_fps_f32: greedy farthest point sampling of every event, one workgroup per event, all picks in one launch.
 *   Arguments: x[N,D] fp32; event b owns the nodes lo = ptr[b] .. ptr[b+1]-1, n = ptr[b+1] - ptr[b], and writes
 *   m = out_ptr[b+1] - out_ptr[b] GLOBAL node ids (int64) to out[out_ptr[b] .. out_ptr[b+1]).  M = out_ptr[B] as the
 *   caller knows it = the size of out (nothing is written at or beyond out[M]).  start[b] = the event-local index of the
 *   first sample; NULL = 0 for every event; the kernel clamps it into [0, n-1].  An event with n == 0 or m == 0 writes
 *   nothing.
 *   Distance: the fp32 chain of rule R1 in coordinate order, d(p, s): a = x[s,c] - x[p,c]; acc = fmaf(a, a, acc) from
 *   acc = 0.  The chain is bit-symmetric in s and p (a and -a square to the same bits).
 *   Selection: out[0] = lo + start; dist[p] = d(p, start) for every p of the event; for i = 1 .. m-1: s = the LOWEST
 *   event-local index whose dist is the maximum, out[i] = lo + s, and every p is updated,
 *   dist[p] = (d(p,s) < dist[p]) ? d(p,s) : dist[p].  m > n is legal: once every distinct point is taken all distances
 *   are 0 and the lowest index repeats.
 *   Numerics: finite coordinates never produce NaN; an overflow gives +inf, which orders normally.  With non-finite
 *   coordinates the chosen nodes are unspecified, but every id written lies inside its event and the loop ends after m
 *   iterations.
 *   Limits: 1 <= D <= DMET_MAX_KNN_DIM, N <= 2^31-1, any n.  An event of up to DMET_FPS_LDS_NODES(D) nodes keeps its
 *   coordinates (transposed, [D][n]) and running distances in LDS; a larger one keeps the same two arrays in the
 *   workspace, N (D + 1) floats, and reads them back through L2 (same code, same bits).  Returns -EINVAL with a dmet_last_error() message naming the argument for a bad D, negative
 *   sizes, a workspace smaller than dmet_fps_workspace_bytes(N, B, D) (monotone in N), or a NULL x / ptr / out_ptr / out
 *   / ws with N, M > 0; returns 0 at once when B == 0, N == 0 or M == 0.  Asynchronous on `stream`: no host sync, no
 *   allocation, no global state, capturable in a graph; bit-identical from run to run. */
#define DMET_FPS_THREADS 1024           /* workgroup size: node p of an event is owned by thread p mod this */
#define DMET_FPS_LDS_FLOATS 36864       /* 144 KiB: the running distances [n] and the coordinates [D][n] of one event */
#define DMET_FPS_LDS_NODES(D) (DMET_FPS_LDS_FLOATS / ((D) + 1))
size_t dmet_fps_workspace_bytes(int64_t N, int B, int D);
int dmet_fps_f32(const float *x, const int64_t *ptr, int B, int64_t N, int D, const int64_t *out_ptr,
                 const int64_t *start, int64_t M, int64_t *out, void *ws, size_t ws_bytes, dmet_stream_t stream);

/* ---- Selection pooling: torch_geometric's topk / filter_adj under TopKPooling, SAGPooling, SortAggregation
 *      (csrc/select.hip) ----------------------------------------------------------------------------------------------------
 * dmet_topk_f32: the ranked selection of every event, one workgroup per event, all events in one launch.
 *   Arguments: score[N] fp32; event b owns the nodes lo = ptr[b] .. ptr[b+1]-1 (n_b of them; ptr must be non-decreasing,
 *   the caller's precondition as for every ptr of this header; its values are clamped to [0, N]) and
 *   the slots out_ptr[b] .. out_ptr[b+1]-1 of perm (r_b of them, the caller's choice).  M = the size of perm: nothing is
 *   written at or beyond perm[M] (a slot range is cut there).
 *   Order within an event: descending canonical score, ties to the lower index.  Canonical score: -0.0 counts as +0.0,
 *   every NaN (either sign, any payload) ranks above +inf -- where torch.sort(descending=True) puts it --, +-inf order
 *   normally.  Realised as one unsigned 64-bit key per node: high word = the order-preserving map of the canonical fp32
 *   bits (NaN -> 0xFFFFFFFF first; then sign set: ~bits, else bits | 0x80000000), low word = ~local index.  The keys of an
 *   event are distinct and key 0, the padding to a power of two, lies below all of them, so the descending bitonic
 *   network that sorts them has one answer.
 *   Event b writes m_b = min(r_b, n_b) GLOBAL node ids, best first, to perm[out_ptr[b] ..), then -1 to the remaining
 *   r_b - m_b slots.  node_map[i] (int32) = the position of node i in perm, -1 if it was not picked; it is written for
 *   all N nodes, those of events that pick nothing and those before ptr[0] or from ptr[B] on included.
 *   An event of up to DMET_SELECT_LDS_NODES nodes keeps its keys in LDS (128 KiB); a larger one keeps the same array in the
 *   workspace, 2 N keys, at ws[2 lo ..) (the power of two above n_b is below 2 n_b), and runs the same code (same bits).
 *   Limits: any n_b, 0 included; N, M <= 2^31-1.
 *
 * dmet_select_rows_f32: out[r, f] = x[perm[r], f] * s[perm[r]] for x[N,F], perm[M]; s == NULL: the plain gather; a row with
 *   perm[r] outside [0, N) is zeros.  dmet_select_rows_bwd_f32, for g[M,F], by node through node_map, no memset and no
 *   scatter: r = node_map[i] outside [0, M): gx[i,:] = 0, gs[i] = 0; else gx[i,f] = g[r,f] * s[i] (g[r,f] for s == NULL)
 *   and gs[i] = sum_f g[r,f] * x[i,f], lane l of the node's wavefront adding f = l, l + 64, ... in that order, then the xor
 *   butterfly over the 64 lanes.  gx or gs may be NULL: only the gradients somebody needs are formed (x may be NULL
 *   without gs).  Any F >= 1.  No transcendental: the activation of the score is the caller's.
 *
 * dmet_filter_table: the induced subgraph of a neighbour table.  nbr[N,k] int32, cnt[N] or NULL (only the first cnt[i] slots
 *   of row i are read), perm[M], node_map[N] -> out_nbr[M,k], out_cnt[M].  Row r = row perm[r] of nbr: its entries j with
 *   0 <= j < N and node_map[j] >= 0, in slot order, relabelled to node_map[j] and packed to the left; every remaining slot
 *   -1; out_cnt[r] = the number kept.  perm[r] outside [0, N): all -1, count 0.  1 <= k <= DMET_SELECT_MAX_K.
 *
 * dmet_filter_edges_count / dmet_filter_edges_write: the induced subgraph of an int64 edge index (row[E], col[E]), as a
 *   stable compaction in two calls with one workspace.  An edge is kept when both ends lie in [0, N) -- compared before
 *   node_map is read -- and both are picked.  _count leaves per-block counts (blocks of DMET_SELECT_EDGE_BLOCK edges) and
 *   their exclusive scan in ws, total[0] (int64) = E' and nbad[0] (int32) = the number of edges with an out-of-range end
 *   (those are dropped).  The caller reads E' (the one host read: upstream returns exact-size tensors too), sizes
 *   out_index[2,E'] and kept[E'], and calls _write with the same operands and workspace: kept edge number q in the
 *   caller's order gets out_index[0,q] = node_map[row[e]], out_index[1,q] = node_map[col[e]], kept[q] = e.  Nothing is
 *   written at or beyond column Eout.
 *
 *   All entries: -EINVAL with a dmet_last_error() message naming the argument, before any HIP call, for a bad size, a
 *   small workspace or a NULL operand of a non-empty problem; 0 at once for an empty problem (dmet_topk_f32: B == 0, or
 *   N == 0 and M == 0; the others: no output element).  Asynchronous on `stream`, no allocation, no float atomics, no
 *   global state; bit-identical from run to run. */
#define DMET_SELECT_THREADS 1024        /* workgroup of an event */
#define DMET_SELECT_LDS_NODES 16384     /* events up to this size sort their 64-bit keys in LDS (128 KiB) */
#define DMET_SELECT_MAX_K 1024          /* widest table dmet_filter_table takes */
#define DMET_SELECT_EDGE_BLOCK 1024     /* edges per block of the compaction */
size_t dmet_topk_workspace_bytes(int64_t N);
int dmet_topk_f32(const float *score, const int64_t *ptr, int B, int64_t N, const int64_t *out_ptr, int64_t M,
                  int64_t *perm, int32_t *node_map, void *ws, size_t ws_bytes, dmet_stream_t stream);
int dmet_select_rows_f32(const float *x, const float *s, const int64_t *perm, int64_t N, int64_t M, int F, float *out,
                         dmet_stream_t stream);
int dmet_select_rows_bwd_f32(const float *g, const float *x, const float *s, const int32_t *node_map, int64_t N, int64_t M,
                             int F, float *gx, float *gs, dmet_stream_t stream);
int dmet_filter_table(const int32_t *nbr, const int32_t *cnt, const int64_t *perm, const int32_t *node_map, int64_t N,
                      int64_t M, int k, int32_t *out_nbr, int32_t *out_cnt, dmet_stream_t stream);
size_t dmet_filter_edges_workspace_bytes(int64_t E);
int dmet_filter_edges_count(const int64_t *row, const int64_t *col, int64_t E, const int32_t *node_map, int64_t N,
                            int64_t *total, int32_t *nbad, void *ws, size_t ws_bytes, dmet_stream_t stream);
int dmet_filter_edges_write(const int64_t *row, const int64_t *col, int64_t E, const int32_t *node_map, int64_t N,
                            const void *ws, size_t ws_bytes, int64_t Eout, int64_t *out_index, int64_t *kept,
                            dmet_stream_t stream);

/* ---- Voxel clustering: torch_cluster's grid_cluster, PyG's voxel_grid and consecutive_cluster (csrc/voxel.hip) -----------
 * dmet_voxel_cells_f32 replaces torch_cluster.grid_cluster(pos, size, start, end) and, with events, PyG's
 *   voxel_grid(pos, size, batch, start, end).  pos[N,D] fp32, 1 <= D <= DMET_VOXEL_MAX_DIM.  grid[3,D] fp32 in DEVICE
 *   memory: row 0 the cell sizes, row 1 start, row 2 end (the caller fills in pos.min(0) / pos.max(0) where upstream
 *   would).  Event b owns the nodes ptr[b] .. ptr[b+1]-1 (non-decreasing, ptr[0] = 0, ptr[B] = N: the caller's
 *   precondition; a node's event is found from ptr, one binary search per workgroup and a walk of at most B steps).
 *   Two launches.  The first, one thread, writes nvox[0..D): nvox_d = trunc((end_d - start_d) / size_d) + 1 in fp32, 1 when
 *   that quotient is NaN, infinite or negative; nvox[D] = cells = their product, and flags[0] = 1 when the product would pass
 *   2^32 - 1: the count that passes it is cut so that cells fits (B cells <= 2^63 - 1 follows from B <= 2^31 - 1).
 *   The second, one node per thread: c_d = trunc((pos_d - start_d) / size_d), the subtraction and the correctly rounded
 *   division one fp32 rounding each, clamped to [0, nvox_d - 1] (NaN and -inf: 0, +inf: nvox_d - 1);
 *   cell[i] = sum_d c_d prod_{d' < d} nvox_d' (uint32, event-local) and id[i] = cell[i] + b cells (int64): upstream's value
 *   for every finite pos inside [start, end], the event being the most significant digit as PyG's appended batch
 *   coordinate makes it.  batch (int64 [N], may be NULL): flags[1] = 1 when some batch[i] differs from the event ptr
 *   gives, else 0.  N = 0: only the first launch.
 *
 * dmet_voxel_coarsen replaces PyG's consecutive_cluster and what the pooling operators derive from it (a global stable
 *   sort, unique, scatter, searchsorted) for ids of the form above.  Two launches.  The first, one workgroup per event: the
 *   event's nodes ranked ascending by the 64-bit key (cell << 32 | local index) -- distinct keys, padded with ~0 to a power
 *   of two, so the bitonic network has one answer, the stable order -- a mark on each position whose cell differs from its
 *   predecessor's, the marks prefix-summed by wavefront ballots.  An event of up to DMET_SELECT_LDS_NODES nodes keeps its
 *   keys in LDS (128 KiB of keys, 144 KiB with one spare slot per eight against bank conflicts; one workgroup per CU); a
 *   larger one keeps the same array, unpadded, in the workspace at ws[2 lo ..) and runs the same code (same bits).  Three
 *   stages of the network run as one pass over the keys, in registers.  The second, one workgroup per event, adds up the B cluster counts (exclusive for its own offset) and writes:
 *   node_map[N] int64, the consecutive cluster id of every node (= unique(id, sorted, return_inverse)[1]);
 *   order[N] int64, the nodes grouped by cluster, ascending node index inside one (= sort(id, stable)[1]);
 *   rowptr[0..C] int32, cluster c is order[rowptr[c] .. rowptr[c+1]), rowptr[C] = ptr[B]; out_batch[0..C) int64, the event
 *   of every cluster; out_ptr[B+1] int64, the clusters of event b are out_ptr[b] .. out_ptr[b+1]-1;
 *   record[3] int64 = (C, the largest and the smallest number of clusters in one event).  rowptr holds N + 1 entries and
 *   out_batch N; entries beyond C + 1 and C are not written.  Nodes no event owns get node_map = order = -1.
 *   No atomics, integer arithmetic only: bit-identical from run to run whatever the buffers held.
 *   Limits: N <= 2^31-1, any n_b.  B == 0: returns 0 at once; N == 0 with B > 0 is refused (the caller fills the empty
 *   result).
 *
 *   Both entries: -EINVAL with a dmet_last_error() message naming the argument, before any HIP call, for a bad size, a
 *   small workspace or a NULL operand of a non-empty problem.  Asynchronous on `stream`, no allocation, no global state. */
#define DMET_VOXEL_MAX_DIM 8            /* D of dmet_voxel_cells_f32 */
#define DMET_VOXEL_THREADS 1024         /* workgroup of an event in dmet_voxel_coarsen */
int dmet_voxel_cells_f32(const float *pos, int64_t N, int D, const float *grid, const int64_t *ptr, int B,
                         const int64_t *batch, int64_t *nvox, int32_t *flags, int64_t *id, uint32_t *cell,
                         dmet_stream_t stream);
size_t dmet_voxel_coarsen_workspace_bytes(int64_t N, int B);
int dmet_voxel_coarsen(const uint32_t *cell, const int64_t *ptr, int B, int64_t N, int64_t *node_map, int64_t *order,
                       int32_t *rowptr, int64_t *out_batch, int64_t *out_ptr, int64_t *record, void *ws, size_t ws_bytes,
                       dmet_stream_t stream);

/* ---- Edge pooling: the greedy edge contraction of torch_geometric.nn.pool.EdgePooling (csrc/edge_match.hip) --------------
 * dmet_edge_match_f32 replaces torch_geometric.nn.pool.EdgePooling._merge_edges, which copies the edge index to the host
 *   and walks the sorted edges in a Python loop.  One workgroup per event, every round in one launch.
 *   The rule (the result is defined by this sequential form): take the candidate edges of an event in descending
 *   canonical score, ties to the lower edge id in the CALLER's order; an edge (s, t) is taken when s and t are both still
 *   free, and claims both.  A self loop s == t claims its one node, which becomes a one-node cluster carrying that edge (as
 *   upstream).  Canonical score: the order of dmet_topk_f32 -- -0.0 counts as +0.0, every NaN ranks above +inf -- as the
 *   same 64-bit key, (order-preserving map of the fp32 bits << 32) | ~edge id.  Keys are distinct: a strict total order.
 *   The parallel form: in a round every live edge (both ends free) offers its key to both ends, an integer max per node;
 *   a live edge that holds the largest key at both of its ends is taken; rounds repeat until no live edge is left.  For a
 *   strict total order this takes exactly the edges of the sequential rule (the locally dominant edges of the live graph
 *   are the ones the sequential walk reaches with both ends free, by induction over the rounds), and the largest live key
 *   is always taken, so there are at most n_b rounds; the kernel's loop is bounded by n_b + 1 and sets flags[2] should it
 *   ever get there.  Typical counts: 13 to 16 rounds for the events of a 64 x 4 500 batch under a k = 16 kNN graph with
 *   the layer's softmax scores; n_b / 2 for a path with monotone scores, the worst case.
 *   Arguments: the edges grouped by target -- rowptr[N+1] int32, src[E], tgt[E] int32 (tgt[e] == i for rowptr[i] <= e <
 *   rowptr[i+1]) --, perm[E] int32 = the caller-order id of every grouped position (NULL = the position itself),
 *   score[E] fp32 by grouped position, ptr[B+1] (values clamped to [0, N]).  Event b owns the nodes ptr[b] .. ptr[b+1]-1
 *   and the positions rowptr[ptr[b]] .. rowptr[ptr[b+1]]-1.
 *   An edge with an end outside [0, N) is no candidate and sets flags[0]; one whose ends lie in different events is no
 *   candidate and sets flags[1].  flags[3] int32 is cleared by the call (a memset node on the stream) and written 0 / 1.
 *   Outputs, every element written by the kernel: cluster[N] int64 = min(u, v) for a pair (u, v), u otherwise (the
 *   convention of dmet_graclus_f32); partner[N] int32 = v, -1 for a one-node cluster (what dmet_pool_pairs_index /
 *   dmet_pool_pairs_f32 read); edge[N] int64 = the caller-order id of the claiming edge, -1 for a node nobody claimed;
 *   rounds[B] int32 (may be NULL) = the rounds of event b that had a live edge.  Nodes no event owns are unclaimed.
 *   An event of up to DMET_EDGE_MATCH_LDS_NODES nodes keeps one 64-bit state word per node in LDS (128 KiB of the CU's
 *   160); a larger one keeps the same words in the workspace, N words, at ws[ptr[b] ..), and runs the same code (same
 *   bits).  Behind the N words the workspace holds two lists of E positions each (dmet_edge_match_workspace_bytes(N, E)
 *   = 8 N + 8 E bytes): a round appends its live edges to one list while it walks the other, so an edge is visited
 *   while it is live and once more, not once per round; the order inside a list depends on the run, the set does not, and
 *   nothing reads the order (DMET_EDGE_MATCH_STATE=workspace in the environment, read on every call, sends every event
 *   through the workspace form, for tests).  Integer atomic max only (LDS, or L2 for the workspace form), no float
 *   atomics: the result is a function of the input alone, whatever the buffers and the workspace held.
 *   Limits: N, E <= 2^31-1, any n_b.  Events without edges, E == 0 and N == 0 are valid; B == 0 or N == 0 returns 0 after
 *   clearing flags and rounds and writes nothing else (no event owns a node).  -EINVAL with a dmet_last_error() message naming the
 *   argument, before any HIP call, for a bad size, a small workspace or a NULL operand of a non-empty problem.
 *   Asynchronous on `stream`, no allocation, no global state. */
#define DMET_EDGE_MATCH_THREADS 1024    /* workgroup of an event */
#define DMET_EDGE_MATCH_LDS_NODES 16384 /* events up to this size keep their 64-bit state words in LDS (128 KiB) */
size_t dmet_edge_match_workspace_bytes(int64_t N, int64_t E);
int dmet_edge_match_f32(const int32_t *rowptr, const int32_t *src, const int32_t *tgt, const int32_t *perm,
                        const float *score, int64_t E, const int64_t *ptr, int B, int64_t N, int64_t *cluster,
                        int32_t *partner, int64_t *edge, int32_t *rounds, int32_t *flags, void *ws, size_t ws_bytes,
                        dmet_stream_t stream);

/* ---- Components and DBSCAN: connected components and density clustering of every event (csrc/components.hip) -------------
 * dmet_components_i32 replaces scipy.sparse.csgraph.connected_components (PyG's LargestConnectedComponents runs it on the
 *   host) and sklearn.cluster.DBSCAN over a given neighbourhood graph.  One workgroup per event, one launch for the batch.
 *   The graph, one of two forms:
 *     table (nbr != NULL): nbr[N, k] int32, row i lists the neighbours of node i; with cnt[N] int32 the first
 *       min(cnt[i], k) slots of row i are read and nothing beyond them, without it all k; a slot holding -1 is empty.
 *     list  (nbr == NULL, rowptr != NULL): rowptr[N+1], src[E], tgt[E] int32, the entries grouped by target (tgt[e] == i
 *       for rowptr[i] <= e < rowptr[i+1]); event b owns the positions rowptr[ptr[b]] .. rowptr[ptr[b+1]] - 1.
 *   Event b owns the nodes ptr[b] .. ptr[b+1]-1 (ptr[B+1] int64, values clamped to [0, N]).  An entry (i, j) joins i and j
 *   whichever way round it is listed (weak connectivity); duplicates and self entries are harmless.  An entry with an end
 *   outside [0, N) joins nothing and adds 1 to flags[0]; one whose ends lie in two events joins nothing and adds 1 to
 *   flags[1].  flags[4] int32 is cleared by the call (a memset node on the stream); flags[2] is set should a loop of the
 *   union-find ever reach its bound (a defect of the kernel: see below); flags[3] counts, in DBSCAN mode over a table, the
 *   rows that fill all k slots (a radius table that may have cut a neighbourhood).
 *
 *   mode = DMET_COMPONENTS_CC: labels[i] int64 = the smallest global id of the component of node i: canonical, the same
 *   for every order of the entries, every launch and every run.  node_mask[N] (uint8, may be NULL): a node with 0 gets -1
 *   and every entry that touches it joins nothing.  edge_mask (uint8, may be NULL): one value per position -- [N k] for a
 *   table, where the value of an empty slot (-1, or beyond cnt) is never read, [E] in grouped order for a list --, an
 *   entry with 0 joins nothing.  core and nclusters are not touched.
 *
 *   mode = DMET_COMPONENTS_DBSCAN (no masks): n_i = the non-empty slots of row i (table: min(cnt[i], k), or the slots
 *   != -1; list: rowptr[i+1] - rowptr[i]), plus 1 with count_self -- the caller's statement that rows list no self entry.
 *   Node i is core when n_i >= min_samples (>= 1); core[i] uint8 = 1 / 0.  Core nodes joined by an entry form clusters, the
 *   components of the core-core subgraph; the root of a cluster is its smallest core id.  A node that is not core takes
 *   the cluster of the core node IN ITS OWN ROW whose cluster has the smallest root, and is noise, -1, with no core node
 *   in its row: the graph is taken as symmetric, as a radius graph is (an entry (i, j) without its mirror makes j no
 *   border node of i's cluster).  labels[i] int64 = the EVENT-LOCAL number of i's cluster, 0, 1, ... in ascending root id
 *   (sklearn's discovery order), or -1; nclusters[b] int64 = the clusters of event b (0 for an event without nodes).  The
 *   batch-wide number is labels + the exclusive sum of nclusters, left to the caller.  Whenever flags is all zero the
 *   labels and the core mask are those of sklearn.cluster.DBSCAN(metric='precomputed') on the same symmetric entry set.
 *
 *   The kernel: one parent word (int32, event-local) per node; an event of up to lds_nodes nodes keeps the words in LDS,
 *   a larger one in the workspace at ws[ptr[b] ..) (dmet_components_workspace_bytes(N) = 4 N bytes) through agent-scope
 *   atomics, and runs the same code (same labels).  lds_nodes: 0 = DMET_COMPONENTS_LDS_NODES (64 KiB of the CU's 160,
 *   two workgroups per CU), larger values are cut to it, 1 .. sends larger events through the workspace (for tests).
 *   Union-find: an entry finds the roots of its ends, halving the paths, and hooks the larger root under the smaller with
 *   a compare-and-swap that only a root passes: a parent is never larger than its child, so a find walks at most n_b
 *   steps and the root of a finished component is its smallest id; a failed swap means some other hook succeeded, and an
 *   event has fewer than n_b of those, so a hook is retried at most n_b + 1 times.  Both loops carry those bounds and set
 *   flags[2] there; neither is reached.  After a barrier the paths are compressed in full.  DBSCAN mode runs core test,
 *   unions over core-core entries, compression, border pass (an integer max per node) and a workgroup scan over the roots,
 *   with barriers between them.  Integer atomics only: the result is a function of the input alone, whatever lane ran
 *   first and whatever labels, core, nclusters and the workspace held; every output element is written exactly once.
 *   Nodes no event owns (ptr[0] > 0, ptr[B] < N) are components of their own (CC; -1 when masked) or noise, not core.
 *   Limits: N, E <= 2^31-1, any n_b, any k >= 0.  B == 0 with N == 0 returns 0 after clearing flags; B == 0 with N > 0 is
 *   refused.  -EINVAL with a dmet_last_error() message naming the argument, before any HIP call, for a bad size or mode, a
 *   small workspace, a mask in DBSCAN mode or a NULL operand of a non-empty problem.  Asynchronous on `stream`, no
 *   allocation, no global state. */
#define DMET_COMPONENTS_THREADS 1024    /* workgroup of an event */
#define DMET_COMPONENTS_LDS_NODES 16384 /* events up to this size keep their int32 parent words in LDS (64 KiB) */
#define DMET_COMPONENTS_CC 0
#define DMET_COMPONENTS_DBSCAN 1
size_t dmet_components_workspace_bytes(int64_t N);
int dmet_components_i32(const int32_t *nbr, int k, const int32_t *cnt, const int32_t *rowptr, const int32_t *src,
                        const int32_t *tgt, int64_t E, const uint8_t *edge_mask, const uint8_t *node_mask,
                        const int64_t *ptr, int B, int64_t N, int mode, int min_samples, int count_self, int64_t *labels,
                        uint8_t *core, int64_t *nclusters, int32_t *flags, int lds_nodes, void *ws, size_t ws_bytes,
                        dmet_stream_t stream);

/* ---- Condensation clustering: object-condensation inference of every event (csrc/condense.hip) ---------------------------
 * dmet_condense_f32 collects the nodes of every event around its condensation points (Kieseler 2020), the step upstream
 *   runs as a host loop with one device read per point.  One workgroup per event, one launch for the batch.
 *   Arguments: beta[N] fp32, the condensation weights; x[N, D] fp32 row-major, the cluster coordinates, 1 <= D <=
 *   DMET_CONDENSE_MAX_DIM; event b owns the nodes ptr[b] .. ptr[b+1]-1 (ptr[B+1] int64, non-decreasing, values clamped to
 *   [0, N]); order[N] int64, the ranking: order[ptr[b] .. ptr[b+1]) lists GLOBAL node ids of event b, best first, as
 *   dmet_topk_f32 writes perm for out_ptr = ptr, M = N over the score (beta > t_beta ? beta : -inf); t_beta finite;
 *   t_d finite and > 0.
 *   The rule, per event:
 *     1. Candidates are the nodes with beta[i] > t_beta, compared in fp32 and strictly: a NaN is never one, +inf is.
 *     2. They are walked in the order of `order`: descending canonical beta (-0.0 = +0.0), ties to the lower index.  The
 *        walk reads order from the event's first slot and ends at the first entry that fails beta > t_beta.
 *     3. A candidate that is still unassigned becomes the event's next condensation point c, numbered 0, 1, ... in the
 *        order found, and takes its own number.
 *     4. Every still-unassigned node j of the event, candidate or not, with d2(j, c) < t_d2 takes that number.
 *        d2 is the fp32 chain of rule R1 over the D coordinates in order: a = x[j,c] - x[p,c]; acc = fmaf(a, a, acc) from
 *        0 (d2(a, b) and d2(b, a) are the same bits); t_d2 = t_d * t_d, one fp32 rounding, as dmet_radius_f32 forms r2;
 *        the comparison is strict, as there.  A NaN distance is below nothing: a candidate with a NaN coordinate becomes
 *        a condensation point of itself alone.
 *     5. Nodes left unassigned are noise.
 *   So a candidate is a condensation point iff no condensation point of a higher rank lies within t_d of it, and a node's
 *   point is the highest-ranked condensation point within t_d of it.
 *   Outputs, every element written exactly once: local[N] int64 = the EVENT-LOCAL number of the node's condensation
 *   point, -1 for noise; assoc[N] int64 = the GLOBAL id of that point (a point holds itself), -1 for noise; nclusters[B]
 *   int64 = the points of event b (0 for an event without nodes).  The batch-wide number is local + the exclusive sum of
 *   nclusters, left to the caller.  Nodes no event owns (ptr[0] > 0, ptr[B] < N) are noise.  Unwritten regions: none.
 *   flags[2] int32 is cleared by the call (a memset node on the stream).  flags[0] counts the entries of `order` the walk
 *   met that lie outside their event: such an entry is compared against the event's range BEFORE anything is read
 *   through it, and skipped.  flags[1] is set should the walk reach its bound of n_b + 1 windows (a defect of the kernel:
 *   every window holds a condensation point, so there are at most n_b).  A ranking that lists a node twice or leaves one
 *   out is the caller's error beyond that: no access leaves the buffers, the labels are then not the rule's.
 *
 *   The kernel: one state word (int32: the node's number, or -1) per node; an event of up to lds_nodes nodes keeps the
 *   words in LDS, a larger one in the workspace at ws[ptr[b] ..) (ws_bytes, the size of ws, at least
 *   dmet_condense_workspace_bytes(N) = 4 N bytes) through agent-scope accesses, and runs the same code (same outputs).
 *   lds_nodes: 0 = DMET_CONDENSE_LDS_NODES, larger values
 *   are cut to it, 1 .. sends larger events through the workspace (for tests).  The walk is windowed: wavefront 0
 *   compacts the next DMET_CONDENSE_WINDOW still-unassigned candidates from its cursor in `order`, resolves them among
 *   themselves in rank order (entry s, if still alive, is a point and the alive entries behind it within t_d take its
 *   number: a dead entry suppresses nobody), and after a workgroup barrier every thread holds its own unassigned nodes
 *   against the window's points in rank order and takes the first within t_d.  A node within t_d of a point of an earlier
 *   window was assigned there and is never collected, so the windows give exactly the sequential rule.  No float
 *   atomics; the result is a function of the inputs alone, whatever local, assoc, nclusters and the workspace held.
 *   Limits: N <= 2^31-1, any n_b.  B == 0 with N == 0 returns 0 after clearing flags; B == 0 with N > 0 is refused.
 *   -EINVAL with a dmet_last_error() message naming the argument, before any HIP call, for N < 0, B < 0, D outside
 *   1..DMET_CONDENSE_MAX_DIM, a t_beta that is not finite, a t_d that is not finite and > 0, lds_nodes < 0, a small
 *   workspace or a NULL operand of a non-empty problem.  Asynchronous on `stream`, no allocation, no global state. */
#define DMET_CONDENSE_THREADS 1024      /* workgroup of an event */
#define DMET_CONDENSE_LDS_NODES 16384   /* events up to this size keep their int32 state words in LDS (64 KiB) */
#define DMET_CONDENSE_WINDOW 64         /* candidates resolved per window: one wavefront */
#define DMET_CONDENSE_MAX_DIM 8
size_t dmet_condense_workspace_bytes(int64_t N);
int dmet_condense_f32(const float *beta, const float *x, const int64_t *order, const int64_t *ptr, int B, int64_t N, int D,
                      float t_beta, float t_d, int64_t *local, int64_t *assoc, int64_t *nclusters, int32_t *flags,
                      int lds_nodes, void *ws, size_t ws_bytes, dmet_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DMET_H_ */

"""CPU restatement (numpy / plain Python) of the graph-coarsening contract of include/dmet.h: the graclus matching of
dmet_graclus_f32 (colour function, propose / respond rounds, best-candidate rule, sequential finisher), the CSR order
deepmetv2_amd.graclus builds, the consecutive numbering of the pooled clusters, the pair-pool index, pair pooling forward
and backward, and the normalized-cut weights.  Every function restates the header, not the kernels of csrc/pool.hip."""
from __future__ import annotations

import numpy as np

M32 = 0xFFFFFFFF
DEFAULT_ROUNDS = 64


def lowbias32(x: int) -> int:
    x &= M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x


def is_red(u: int, key: int) -> bool:
    return (lowbias32((u & M32) ^ key) >> 31) == 1


def to_csr(edge_index: np.ndarray, N: int, weight=None):
    """Ascending (row, col), stable among duplicates: rowptr[N+1], col[E], weight[E] (or None)."""
    row, col = np.asarray(edge_index[0], np.int64), np.asarray(edge_index[1], np.int64)
    order = np.lexsort((col, row))          # stable; primary key row
    row, col = row[order], col[order]
    w = None if weight is None else np.asarray(weight, np.float32)[order]
    rowptr = np.searchsorted(row, np.arange(N + 1), side="left").astype(np.int64)
    return rowptr, col, w


def _best(cands, ws):
    """First candidate, replaced only by a strictly greater weight (IEEE >); unweighted: the first one."""
    if not cands:
        return -1
    if ws is None:
        return cands[0]
    b, bw = cands[0], ws[0]
    for c, w in zip(cands[1:], ws[1:]):
        if w > bw:
            b, bw = c, w
    return b


def graclus(rowptr, col, weight, ptr, seed: int, max_rounds: int = 0):
    """(cluster[N] int64, partner[N] int64 (-1 = singleton), rounds[B]) exactly as dmet_graclus_f32 defines them."""
    N = len(rowptr) - 1
    R = max_rounds or DEFAULT_ROUNDS
    s = (seed & M32) ^ ((seed >> 32) & M32)
    cluster = np.arange(N, dtype=np.int64)
    partner = np.full(N, -1, dtype=np.int64)
    rounds = []
    w32 = None if weight is None else np.asarray(weight, np.float32)
    for b in range(len(ptr) - 1):
        lo, hi = int(ptr[b]), int(ptr[b + 1])
        n = hi - lo
        if n <= 0:
            rounds.append(0)
            continue
        # every row once: (local neighbour, weight) in CSR order, self loops and out-of-block endpoints dropped
        rows = []
        for i in range(n):
            u = lo + i
            e0, e1 = int(rowptr[u]), int(rowptr[u + 1])
            c = col[e0:e1].astype(np.int64)
            keep = (c >= lo) & (c < hi) & (c != u)
            rows.append((list((c[keep] - lo).tolist()), None if w32 is None else list(w32[e0:e1][keep])))
        st = [-1] * n

        def best_of(i, pred):
            cs, ws = rows[i]
            idx = [t for t, j in enumerate(cs) if pred(j)]
            return _best([cs[t] for t in idx], None if ws is None else [ws[t] for t in idx])

        r = 0
        while r < R:
            if all(v >= 0 for v in st):
                break
            key = lowbias32((s + 0x9E3779B9 * r) & M32)
            red = [is_red(lo + i, key) for i in range(n)]
            pr = [-3] * n
            for i in range(n):
                if st[i] >= 0:
                    continue
                if not any(st[j] < 0 for j in rows[i][0]):
                    pr[i] = -2
                elif red[i]:
                    pr[i] = -1
                else:
                    v = best_of(i, lambda j: st[j] < 0 and red[j])
                    pr[i] = v
            for i in range(n):
                if pr[i] == -2:
                    st[i] = i
                elif pr[i] == -1 and red[i]:
                    w = best_of(i, lambda j, i=i: pr[j] == i)
                    if w >= 0:
                        st[i], st[w] = w, i
            r += 1
        if r == R:
            for i in range(n):
                if st[i] >= 0:
                    continue
                w = best_of(i, lambda j: st[j] < 0)
                if w >= 0:
                    st[i], st[w] = w, i
                else:
                    st[i] = i
        rounds.append(r)
        for i in range(n):
            cluster[lo + i] = lo + min(i, st[i])
            partner[lo + i] = -1 if st[i] == i else lo + st[i]
    return cluster, partner, np.asarray(rounds, np.int64)


def check_matching(cluster, partner, edge_index, ptr):
    """Assert the matching is valid (clusters of <= 2 nodes joined by an edge, inside one event, cluster = min) and
    maximal for a symmetric graph (no edge joins two singletons; self loops do not count)."""
    N = len(cluster)
    edges = set(zip(edge_index[0].tolist(), edge_index[1].tolist()))
    event = np.searchsorted(np.asarray(ptr), np.arange(N), side="right") - 1
    for u in range(N):
        v = int(partner[u])
        if v < 0:
            assert cluster[u] == u
            continue
        assert partner[v] == u and v != u
        assert cluster[u] == min(u, v) == cluster[v]
        assert (u, v) in edges or (v, u) in edges
        assert event[u] == event[v]
    single = partner < 0
    for a, b in edges:
        if a != b:
            assert not (single[a] and single[b]), f"edge ({a},{b}) joins two singletons"


def consecutive(cluster: np.ndarray):
    """PyG consecutive_cluster: ids ranked by sorted unique value -> inverse[N]."""
    _u, inv = np.unique(cluster, return_inverse=True)
    return inv


# ---- pair pooling of a matching (include/dmet.h, "Pair pooling of a graclus result") -----------------------------------
def ptr_of(sizes) -> np.ndarray:
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, np.int64))]).astype(np.int64)


def event_of(ptr, nodes) -> np.ndarray:
    """The event that holds each node: the one with ptr[b] <= u < ptr[b+1], so never an empty one."""
    return np.searchsorted(np.asarray(ptr, np.int64), np.asarray(nodes, np.int64), side="right") - 1


def leaders(partner) -> np.ndarray:
    """leader[u]: u itself unless its partner is a valid lower index."""
    partner = np.asarray(partner, np.int64)
    u = np.arange(len(partner), dtype=np.int64)
    return np.where((partner >= 0) & (partner < u), partner, u)


def pair_index(partner, ptr):
    """(cid[N] int64, pooled_ptr[B+1] int64): clusters numbered in ascending leader index, pooled_ptr the exclusive prefix
    sum of the leaders per event."""
    ptr = np.asarray(ptr, np.int64)
    lead = leaders(partner)
    is_lead = lead == np.arange(len(lead))
    number = np.cumsum(is_lead) - 1                       # ascending leader index, over the whole node range
    cid = number[lead].astype(np.int64) if len(lead) else np.zeros(0, np.int64)
    cnt = [int(is_lead[int(a):int(b)].sum()) for a, b in zip(ptr[:-1], ptr[1:])]
    return cid, ptr_of(cnt)


def pool_pairs(x, partner, cid, ptr, C):
    """(out_max[C,F] f32, arg[C,F] int32, out_mean[C,F] f32, pooled_batch[C] int64) in float32 arithmetic: the partner's
    value wins only when strictly greater (IEEE >), so the leader keeps ties (and -0.0 against +0.0);
    out_mean = (x_u + x_v) * 0.5f, x_u for a singleton."""
    x = np.asarray(x, np.float32)
    partner = np.asarray(partner, np.int64)
    cid = np.asarray(cid, np.int64)
    N, F = x.shape
    out_max = np.zeros((C, F), np.float32)
    arg = np.zeros((C, F), np.int32)
    out_mean = np.zeros((C, F), np.float32)
    pooled_batch = np.zeros(C, np.int64)
    u = np.flatnonzero(leaders(partner) == np.arange(N))
    p = partner[u]
    pair = p > u
    xu = x[u]
    xv = x[np.where(pair, p, u)]                          # a singleton meets itself: never strictly greater
    with np.errstate(invalid="ignore"):                   # inf + -inf
        take = xv > xu
        mean = np.where(pair[:, None], (xu + xv) * np.float32(0.5), xu).astype(np.float32)
    out_max[cid[u]] = np.where(take, xv, xu)
    arg[cid[u]] = np.where(take, p[:, None], u[:, None]).astype(np.int32)
    out_mean[cid[u]] = mean
    pooled_batch[cid[u]] = event_of(ptr, u)
    return out_max, arg, out_mean, pooled_batch


def pool_pairs_bwd(g_max, arg, g_mean, partner, cid, F):
    """gx[u,f] = (arg[cid[u],f] == u ? g_max[cid[u],f] : 0) + g_mean[cid[u],f] * (1/2 for a pair, 1 for a singleton) in
    float32, in this order; a NULL (None) gradient leaves its term out."""
    partner = np.asarray(partner, np.int64)
    cid = np.asarray(cid, np.int64)
    N = len(partner)
    u = np.arange(N, dtype=np.int64)
    gx = np.zeros((N, F), np.float32)
    if g_max is not None:
        hit = np.asarray(arg, np.int64)[cid] == u[:, None]
        gx = np.where(hit, np.asarray(g_max, np.float32)[cid], np.float32(0)).astype(np.float32)
    if g_mean is not None:
        pair = (partner >= 0) & (partner != u)
        half = np.where(pair, np.float32(0.5), np.float32(1.0)).astype(np.float32)[:, None]
        gx = (gx + np.asarray(g_mean, np.float32)[cid] * half).astype(np.float32)
    return gx


def random_matching(ptr, rng, single_share):
    """partner[N] int64 of a valid matching: partner[partner[u]] == u inside one event, -1 for singletons.  Each event
    is permuted and the permutation cut into consecutive couples, so pairs straddle any fixed chunk of node indices;
    a couple stays two singletons with probability single_share (0: all pairs, 1: all singletons)."""
    ptr = np.asarray(ptr, np.int64)
    partner = np.full(int(ptr[-1]), -1, np.int64)
    for lo, hi in zip(ptr[:-1], ptr[1:]):
        perm = int(lo) + rng.permutation(int(hi - lo))
        a, b = perm[0:len(perm) - 1:2], perm[1::2]
        keep = rng.random(len(a)) >= single_share
        partner[a[keep]] = b[keep]
        partner[b[keep]] = a[keep]
    return partner


def tie_grid(rng, shape) -> np.ndarray:
    """float32 values from a small grid: multiples of 0.5, both zeros and both infinities, so that many pairs tie and
    some meet -0.0 against +0.0 or an infinity.  No NaN: the header does not define it."""
    grid = np.array([-2.0, -1.5, -1.0, -0.5, 0.5, 1.0, 1.5, 2.0, -0.0, 0.0, np.inf, -np.inf], np.float32)
    return grid[rng.integers(0, len(grid), shape)]


def index_cases():
    """name -> event sizes: where the pair-pool index can go wrong.  Events past one 256-node chunk (the leader rank is
    carried across chunks), 255 / 256 / 257 and 700 events (the count scan is carried across chunks of 256 events), empty
    events at the front, inside and at the end (pooled_ptr repeats)."""
    rng = np.random.default_rng(2024)
    cases = {"chunk_edges": [0, 255, 256, 257, 0, 513, 1, 1025, 0], "one_event": [5000]}
    for B in (255, 256, 257):
        cases[f"events_{B}"] = rng.integers(0, 9, B).tolist()
    s = rng.integers(0, 9, 700)
    s[[0, 1, 255, 256, 349, 698, 699]] = 0
    s[350] = 300
    # the carry across the first 256 events must matter: leaders exist on both sides of it
    cases["scan_carry"] = s.tolist()
    return cases


# ---- normalized cut (include/dmet.h, dmet_normalized_cut_f32 / dmet_normalized_cut_2d_f32) -----------------------------
def normalized_cut(row, col, N, attr=None, x=None):
    """w[E] float32 = a * (1/deg[row] + 1/deg[col]) in float32, deg = in-degree counted over the in-range entries of col;
    a = attr, or ||x[row] - x[col]||_2 with the squares summed in float64 in ascending channel order and one rounding
    to float32.  An out-of-range endpoint gives NaN."""
    row, col = np.asarray(row, np.int64), np.asarray(col, np.int64)
    E = len(row)
    col_ok = (col >= 0) & (col < N)
    ok = col_ok & (row >= 0) & (row < N)
    deg = np.bincount(col[col_ok], minlength=N).astype(np.float32)
    r, c = row[ok], col[ok]
    if x is not None:
        x64 = np.asarray(x, np.float32).astype(np.float64)
        acc = np.zeros(len(r), np.float64)
        for d in range(x64.shape[1]):                     # a loop, not np.sum: np.sum adds pairwise
            t = x64[r, d] - x64[c, d]
            acc = acc + t * t
        a = np.sqrt(acc).astype(np.float32)
    else:
        a = np.asarray(attr, np.float32).reshape(-1)[ok]
    w = np.full(E, np.nan, np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):  # 1/0 = inf, 0 * inf = NaN
        ir = np.float32(1.0) / deg[r]
        ic = np.float32(1.0) / deg[c]
        w[ok] = a * (ir + ic)
    return w

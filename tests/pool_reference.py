"""CPU restatement (numpy / plain Python) of the graph-coarsening contract of include/dmet.h: the graclus matching of
dmet_graclus_f32 (colour function, propose / respond rounds, best-candidate rule, sequential finisher), the CSR order
deepmetv2_amd.graclus builds, and the consecutive numbering of the pooled clusters."""
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

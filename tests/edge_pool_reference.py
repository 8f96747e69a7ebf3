"""References of the edge pooling (deepmetv2_amd/edge_pool.py, csrc/edge_match.hip; include/dmet.h, "Edge pooling").

  * the canonical score order and the 64-bit key (numpy);
  * `sequential_match`: the rule the header defines the result by, a plain-Python sort and loop;
  * `round_match`: the kernel's parallel form, rounds of locally dominant edges, emulated with integer maxima;
  * `upstream_forward` / `upstream_unpool`: torch_geometric's EdgePooling per edge as published (float64 by default), and
    `layer_tensors`: the same formulas evaluated on a GIVEN partition, in float64 (the reference) or float32 (the torch
    composition on the CPU whose own error sets the tolerances of tests/test_gpu_edge_pool.py);
  * `FakeNative`: CPU stand-ins for the _native entries the layer runs, for the host-logic tests;
  * the case builders.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np
import torch

import pool_reference as pr

LDS_NODES = 16384       # DMET_EDGE_MATCH_LDS_NODES


# ---- the order ---------------------------------------------------------------------------------------------------------
def order_bits(score) -> np.ndarray:
    """uint32 whose unsigned order is the canonical score order: -0.0 = +0.0, every NaN above +inf."""
    u = np.ascontiguousarray(np.asarray(score, np.float32)).view(np.uint32).copy()
    nan = (u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    u[u == np.uint32(0x80000000)] = 0
    hi = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    hi[nan] = np.uint32(0xFFFFFFFF)
    return hi


def keys(score, ids) -> np.ndarray:
    """(order bits << 32) | ~edge id: larger key = taken earlier; distinct ids give distinct keys."""
    low = (~np.asarray(ids, np.int64).astype(np.uint32)).astype(np.uint64)
    return (order_bits(score).astype(np.uint64) << np.uint64(32)) | low


def _candidates(src, tgt, ptr, N):
    """(mask of the candidate edges, their event): both ends in [0, N) and in one event."""
    src, tgt, ptr = np.asarray(src, np.int64), np.asarray(tgt, np.int64), np.asarray(ptr, np.int64)
    inside = (src >= 0) & (src < N) & (tgt >= 0) & (tgt < N)
    if len(ptr) < 2:
        return inside & False, np.zeros(len(src), np.int64), inside
    es = pr.event_of(ptr, np.clip(src, 0, max(N - 1, 0)))
    et = pr.event_of(ptr, np.clip(tgt, 0, max(N - 1, 0)))
    owned = (np.clip(src, 0, max(N - 1, 0)) >= ptr[0]) & (np.clip(src, 0, max(N - 1, 0)) < ptr[-1]) & \
            (np.clip(tgt, 0, max(N - 1, 0)) >= ptr[0]) & (np.clip(tgt, 0, max(N - 1, 0)) < ptr[-1])
    return inside & owned & (es == et), et, inside


def sequential_match(src, tgt, score, ids, ptr, N):
    """(cluster[N], partner[N], edge[N]) int64 of the sequential rule: the candidate edges in descending canonical score,
    ties to the lower id; an edge is taken when both ends are free."""
    src, tgt, ids = np.asarray(src, np.int64), np.asarray(tgt, np.int64), np.asarray(ids, np.int64)
    cand, _ev, _inside = _candidates(src, tgt, ptr, N)
    key = keys(score, ids)
    order = sorted((int(e) for e in np.flatnonzero(cand)), key=lambda e: int(key[e]), reverse=True)
    cluster, partner, edge = list(range(N)), [-1] * N, [-1] * N
    free = [True] * N
    for e in order:
        s, t = int(src[e]), int(tgt[e])
        if not (free[s] and free[t]):
            continue
        free[s] = free[t] = False
        edge[s] = edge[t] = int(ids[e])
        if s != t:
            partner[s], partner[t] = t, s
            cluster[max(s, t)] = min(s, t)
    return np.asarray(cluster, np.int64), np.asarray(partner, np.int64), np.asarray(edge, np.int64)


def round_match(src, tgt, score, ids, ptr, N):
    """The parallel form: (cluster, partner, edge, rounds[B], flags[3]).  Every event runs its own rounds; a round of an
    event is counted when the event had a live edge at its start."""
    src, tgt, ids = np.asarray(src, np.int64), np.asarray(tgt, np.int64), np.asarray(ids, np.int64)
    ptr = np.asarray(ptr, np.int64)
    B = max(len(ptr) - 1, 0)
    cand, ev, inside = _candidates(src, tgt, ptr, N)
    flags = np.array([int((~inside).any()), int((inside & ~cand).any()), 0], np.int32)
    key = keys(score, ids)
    s, t = np.clip(src, 0, max(N - 1, 0)), np.clip(tgt, 0, max(N - 1, 0))
    cluster, partner, edge = np.arange(N, dtype=np.int64), np.full(N, -1, np.int64), np.full(N, -1, np.int64)
    claimed = np.zeros(N, bool)
    rounds = np.zeros(B, np.int32)
    for _ in range(N + 1):
        live = cand & ~claimed[s] & ~claimed[t] if N else cand
        if not live.any():
            break
        rounds[np.unique(ev[live])] += 1
        best = np.zeros(N, np.uint64)
        np.maximum.at(best, s[live], key[live])
        np.maximum.at(best, t[live], key[live])
        take = np.flatnonzero(live & (best[s] == key) & (best[t] == key))
        assert len(take), "a round with a live edge took none"
        a, b = s[take], t[take]
        claimed[a] = claimed[b] = True
        edge[a] = edge[b] = ids[take]
        pair = a != b
        partner[a[pair]], partner[b[pair]] = b[pair], a[pair]
        cluster[np.maximum(a, b)] = np.minimum(a, b)
    else:
        flags[2] = 1
    return cluster, partner, edge, rounds, flags


def group_by_target(edge_index, N):
    """(rowptr[N+1] int32, src[E] int32, tgt[E] int32, perm[E] int32) of a caller-order [2, E] index whose targets lie in
    [0, N): the stable grouping the package's edge-list path makes."""
    ei = np.asarray(edge_index, np.int64)
    perm = np.argsort(ei[1], kind="stable")
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(ei[1], minlength=N))]).astype(np.int32)
    return rowptr, ei[0][perm].astype(np.int32), ei[1][perm].astype(np.int32), perm.astype(np.int32)


def pooled_rows(cluster):
    """(cid[N], leaders[C]): pooled rows numbered in ascending leader index (events are ranges of nodes, so this is event by
    event)."""
    cluster = np.asarray(cluster, np.int64)
    leaders, cid = np.unique(cluster, return_inverse=True)
    return cid.astype(np.int64), leaders.astype(np.int64)


# ---- upstream, per edge as published --------------------------------------------------------------------------------------
def _softmax_by_target(raw, tgt, N):
    """torch_geometric.utils.softmax(raw, index=tgt, num_nodes=N)."""
    mx = torch.full((N,), float("-inf"), dtype=raw.dtype).scatter_reduce(0, tgt, raw.detach(), "amax", include_self=True)
    out = (raw - mx[tgt]).exp()
    den = torch.zeros(N, dtype=raw.dtype).index_add(0, tgt, out)
    return out / (den[tgt] + 1e-16)


METHODS = {"softmax": _softmax_by_target, "tanh": lambda raw, tgt, N: torch.tanh(raw),
           "sigmoid": lambda raw, tgt, N: torch.sigmoid(raw)}


def edge_scores(x, edge_index, weight, bias, method, add):
    """e[E] in the caller's order: lin(cat([x[src], x[tgt]])) through the score method, plus add_to_edge_score."""
    raw = torch.nn.functional.linear(torch.cat([x[edge_index[0]], x[edge_index[1]]], dim=-1), weight, bias).view(-1)
    return METHODS[method](raw, edge_index[1], x.shape[0]) + add


def upstream_merge(e, edge_index, N):
    """EdgePooling._merge_edges as published, with a stable descending sort (ties to the lower edge id): (cluster[N] in
    upstream's numbering -- the order the edges are taken, then the remaining nodes --, the taken edge ids)."""
    order = sorted(range(len(e)), key=lambda i: (-float(e[i]), i))
    cluster, remaining, taken = [None] * N, set(range(N)), []
    for i in order:
        s, t = int(edge_index[0][i]), int(edge_index[1][i])
        if s not in remaining or t not in remaining:
            continue
        cluster[s] = cluster[t] = len(taken)
        remaining -= {s, t}
        taken.append(i)
    n = len(taken)
    for node in sorted(remaining):
        cluster[node] = n
        n += 1
    return np.asarray(cluster, np.int64), np.asarray(taken, np.int64)


def upstream_forward(x, edge_index, weight, bias, method, add):
    """(new_x, new_edge_index, cluster, new_edge_score) of upstream's forward in x's dtype, upstream's numbering."""
    N = x.shape[0]
    e = edge_scores(x, edge_index, weight, bias, method, add)
    cluster, taken = upstream_merge(e.detach().numpy(), edge_index.numpy(), N)
    cluster = torch.from_numpy(cluster)
    C = int(cluster.max()) + 1 if N else 0
    score = torch.cat([e[torch.from_numpy(taken)], torch.ones(C - len(taken), dtype=x.dtype)])
    new_x = torch.zeros(C, x.shape[1], dtype=x.dtype).index_add(0, cluster, x) * score.view(-1, 1)
    pooled = cluster[edge_index]
    key = torch.unique(pooled[0] * max(C, 1) + pooled[1])
    return new_x, torch.stack([key // max(C, 1), key % max(C, 1)]), cluster, score


def upstream_unpool(x, cluster, score):
    return (x / score.view(-1, 1))[cluster]


def layer_tensors(dtype, x, edge_index, weight, bias, method, add, cluster, edge, gout):
    """[(name, tensor)] of the layer on the GIVEN partition (cluster[N] = the leader of every node, edge[N] = the claiming
    edge or -1, as edge_matching returns them), pooled rows in ascending leader index: scores, new_edge_score, new_x, and
    the gradients of sum(new_x * gout) to x, lin.weight and lin.bias."""
    x = x.detach().to(dtype).requires_grad_(True)
    w, b = weight.detach().to(dtype).requires_grad_(True), bias.detach().to(dtype).requires_grad_(True)
    cid, leaders = pooled_rows(cluster)
    cid, leaders = torch.from_numpy(cid), torch.from_numpy(leaders)
    e = edge_scores(x, edge_index, w, b, method, add)
    claim = torch.as_tensor(np.asarray(edge, np.int64))[leaders]
    score = torch.where(claim >= 0, e[claim.clamp(min=0)], torch.ones(len(leaders), dtype=dtype))
    new_x = torch.zeros(len(leaders), x.shape[1], dtype=dtype).index_add(0, cid, x) * score.view(-1, 1)
    gx, gw, gb = torch.autograd.grad((new_x * gout.to(dtype)).sum(), [x, w, b])
    return [("scores", e.detach()), ("new_edge_score", score.detach()), ("new_x", new_x.detach()), ("g_x", gx),
            ("g_weight", gw), ("g_bias", gb)]


def coalesced(cid, edge_index):
    """coalesce(cid[edge_index]): the sorted unique pooled edges, self loops kept."""
    cid = np.asarray(cid, np.int64)
    C = int(cid.max()) + 1 if len(cid) else 1
    key = np.unique(cid[edge_index[0]] * C + cid[edge_index[1]])
    return np.stack([key // C, key % C])


# ---- CPU stand-ins ------------------------------------------------------------------------------------------------------------
class FakeNative:
    """Stand-ins for deepmetv2_amd._native._edge_match and the pair-pooling entries on CPU tensors (the matching through
    the round emulation); with fake_native, segment_reference and knn_xy_reference's stand-ins the whole layer runs on the
    CPU.  `calls` counts them by name."""

    def __init__(self):
        self.calls = {}

    def _note(self, name):
        self.calls[name] = self.calls.get(name, 0) + 1

    def edge_match(self, rowptr, src, tgt, perm, score, ptr, want_rounds=False):
        self._note("edge_match")
        assert rowptr.dtype == src.dtype == tgt.dtype == torch.int32 and ptr.dtype == torch.int64
        assert score.dtype == torch.float32 and score.numel() == src.numel() == tgt.numel()
        assert perm is None or (perm.dtype == torch.int32 and perm.numel() == src.numel())
        N = rowptr.numel() - 1
        assert torch.equal(torch.repeat_interleave(torch.arange(N), rowptr.long().diff()).int(), tgt), "not grouped by target"
        ids = np.arange(src.numel()) if perm is None else perm.numpy()
        cluster, partner, edge, rounds, flags = round_match(src.numpy(), tgt.numpy(), score.detach().numpy(), ids,
                                                            ptr.numpy(), N)
        return (torch.from_numpy(cluster), torch.from_numpy(partner).int(), torch.from_numpy(edge),
                torch.from_numpy(rounds) if want_rounds else None, torch.from_numpy(flags))

    def pool_pairs_index(self, partner, ptr):
        self._note("pool_pairs_index")
        cid, pooled_ptr = pr.pair_index(partner.numpy(), ptr.numpy())
        return torch.from_numpy(cid), torch.from_numpy(pooled_ptr)

    def pool_pairs(self, x, partner, cid, ptr, C, want_max, want_mean, want_batch):
        self._note("pool_pairs")
        mx, arg, mean, pb = pr.pool_pairs(x.detach().numpy(), partner.numpy(), cid.numpy(), ptr.numpy(), C)
        return (torch.from_numpy(mx) if want_max else None, torch.from_numpy(arg) if want_max else None,
                torch.from_numpy(mean) if want_mean else None, torch.from_numpy(pb) if want_batch else None)

    def pool_pairs_bwd(self, g_max, arg, g_mean, partner, cid, F, C):
        self._note("pool_pairs_bwd")
        return torch.from_numpy(pr.pool_pairs_bwd(None if g_max is None else g_max.numpy(),
                                                  None if arg is None else arg.numpy(),
                                                  None if g_mean is None else g_mean.numpy(), partner.numpy(), cid.numpy(), F))

    def install(self, monkeypatch):
        import deepmetv2_amd._native as nat
        import knn_xy_reference
        import segment_reference
        knn_xy_reference.install(monkeypatch)           # fake_native's stand-ins and the two-set edge gather
        segment_reference.install(monkeypatch)          # the by-target softmax
        monkeypatch.setattr(nat, "_require_device", lambda *t: torch.device("cpu"))
        monkeypatch.setattr(nat, "_edge_match", self.edge_match)
        for name in ("pool_pairs_index", "pool_pairs", "pool_pairs_bwd"):
            monkeypatch.setattr(nat, name, getattr(self, name))
        return self


# ---- cases ------------------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "name sizes edge_index score")      # edge_index int64 [2, E] and score fp32 [E], caller's order

RAGGED = [0, 1, 2, 33, 130]


def ptr_of(sizes):
    return pr.ptr_of(sizes)


def _table_edges(sizes, width, rng):
    """The edges of a width-`width` table: every node of an event of n > 2 nodes lists min(width, n) random nodes of its
    event (itself possibly among them: a self loop)."""
    src, tgt, lo = [], [], 0
    for n in sizes:
        if n > 2:
            for i in range(n):
                nb = rng.choice(n, size=min(width, n), replace=False)
                src += list(lo + nb)
                tgt += [lo + i] * len(nb)
        lo += n
    return src, tgt


def _mixed_edges(sizes, width, rng):
    """A table's edges plus written self loops, duplicate edges and antiparallel pairs in the large events, and -- the two
    cases every mixed graph must show -- the two-node event (a, b) holding a self loop on a and the edge b -> a alone (with
    the loop scored highest a is a self-loop singleton and b stays unclaimed), the one-node event without an edge."""
    src, tgt = _table_edges(sizes, width, rng)
    ptr = ptr_of(sizes)
    for b, n in enumerate(sizes):
        if n > 2:
            lo = int(ptr[b])
            pick = lo + rng.choice(n, size=6, replace=False)
            src += [pick[0], pick[1], pick[1], pick[2], pick[3], pick[4]]          # a self loop, a duplicate pair of edges,
            tgt += [pick[0], pick[2], pick[2], pick[1], pick[4], pick[3]]          # their antiparallel edge, one more couple
    a = int(ptr[RAGGED.index(2)])
    two = len(src)
    src += [a, a + 1]
    tgt += [a, a]
    ei = np.array([src, tgt], np.int64)
    shuffle = rng.permutation(ei.shape[1])                 # the list arrives ungrouped
    where = np.empty_like(shuffle)
    where[shuffle] = np.arange(len(shuffle))
    return ei[:, shuffle], int(where[two]), int(where[two + 1])


def _mixed(name, width, scores, seed):
    rng = np.random.default_rng(seed)
    ei, loop, weak = _mixed_edges(RAGGED, width, rng)
    E = ei.shape[1]
    if scores == "distinct":
        s = rng.permutation(E).astype(np.float32) / np.float32(E) - np.float32(0.5)
        s[loop], s[weak] = 2.0, -2.0
    elif scores == "ties":
        s = np.array([1.0, 2.0, 3.0], np.float32)[rng.integers(0, 3, E)]
        s[loop], s[weak] = 3.0, 1.0
    else:
        grid = np.array([np.nan, -np.nan, np.inf, -np.inf, -0.0, 0.0, 1.0, -1.0, 1e-45, -1e-45, 3e38], np.float32)
        s = grid[rng.integers(0, len(grid), E)]
        s[loop], s[weak] = np.nan, -np.inf
    return Case(name, RAGGED, ei, s.astype(np.float32))


def path_case():
    """One 130-node path, edge i = (i, i + 1), strictly descending scores: 65 rounds, one edge each."""
    n = 130
    ei = np.array([np.arange(n - 1), np.arange(1, n)], np.int64)
    return Case("path130", [n], ei, (n - np.arange(n - 1)).astype(np.float32))


def big_case():
    """One event one node past the LDS limit, about three edges a node: the workspace form of the state."""
    rng = np.random.default_rng(77)
    n = LDS_NODES + 1
    tgt = np.repeat(np.arange(n), 3)
    src = np.clip(tgt + rng.integers(-40, 41, tgt.size), 0, n - 1)       # local neighbourhoods: chains of dependent edges
    ei = np.array([src, tgt], np.int64)[:, rng.permutation(tgt.size)]
    return Case("lds_plus_one", [n], ei, rng.permutation(tgt.size).astype(np.float32))


def mixed_cases():
    return [_mixed("w3_distinct", 3, "distinct", 1), _mixed("w16_distinct", 16, "distinct", 2),
            _mixed("w16_ties", 16, "ties", 3), _mixed("w3_nonfinite", 3, "nonfinite", 4)]


def empty_cases():
    none = np.zeros((2, 0), np.int64)
    z = np.zeros(0, np.float32)
    return [Case("no_edges", [3, 0, 2], none, z), Case("no_nodes", [], none, z), Case("empty_events", [0, 0], none, z),
            Case("one_event_without_edges", [4, 5], np.array([[0, 1], [1, 2]], np.int64), np.array([1.0, 2.0], np.float32))]


def all_cases():
    return mixed_cases() + [path_case(), big_case()] + empty_cases()


def bad_edge_cases():
    """w3_distinct with one more edge each: one joining two events, one whose source id is >= N (the target stays in
    range: a by-target list cannot hold any other).  (name, case, the flag it must set)."""
    base = mixed_cases()[0]
    N = sum(base.sizes)
    ptr = ptr_of(base.sizes)
    lo33, lo130 = int(ptr[3]), int(ptr[4])
    out = []
    for name, edge, flag in (("crossing", (lo33 + 5, lo130 + 7), 1), ("out_of_range", (N + 3, lo130 + 9), 0)):
        ei = np.concatenate([base.edge_index, np.array([[edge[0]], [edge[1]]], np.int64)], axis=1)
        score = np.concatenate([base.score, np.array([9.0], np.float32)])        # it would be taken first if it counted
        out.append((name, Case(name, base.sizes, ei, score), flag))
    return out


def layer_cases():
    """(name, case, score method, add_to_edge_score) for the layer: the table graphs, their scores replaced by the layer's."""
    m = mixed_cases()
    return [("w3_softmax", m[0], "softmax", 0.5), ("w16_softmax", m[1], "softmax", 0.5), ("w16_tanh", m[1], "tanh", 0.5),
            ("w3_sigmoid", m[0], "sigmoid", 0.0)]


LAYER_F = 5


def layer_inputs(case, seed=5):
    """(x[N, F], weight[1, 2F], bias[1], gout[N, F] -- cut to the pooled rows by the caller) fp32."""
    g = torch.Generator().manual_seed(seed)
    N = sum(case.sizes)
    return (torch.randn(N, LAYER_F, generator=g), torch.randn(1, 2 * LAYER_F, generator=g) * 0.7,
            torch.randn(1, generator=g) * 0.1, torch.randn(N, LAYER_F, generator=g))

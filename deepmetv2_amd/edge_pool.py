"""Edge-contraction pooling with the torch_geometric signature: `EdgePooling` (Diehl 2019) and, on its own, the matching
under it, `edge_matching`.

The kernel is in csrc/edge_match.hip (include/dmet.h, section "Edge pooling"): the greedy contraction of upstream's
`EdgePooling._merge_edges` -- edges in descending score, an edge is taken when both ends are still free -- as rounds of
locally dominant edges, one workgroup per event, every round in one launch, the same bits every run.  This file is
argument checking, the edge scores and the plumbing around the matching; everything differentiable runs through
autograd Functions the package already has (the by-target softmax, the two-set edge gather, pair pooling) and torch
operators.  PyG is not installed next to this package: names and formulas follow its published source, **unpinned**.
"""
from __future__ import annotations

from typing import Callable, NamedTuple, Optional, Tuple

import torch

from . import _native
from .conv import _EdgeFeaturesXY
from .graph import EdgeList, _deferred, _registry_put, batch_info, edge_list_from_edge_index, lookup_graph
from .pool import _Coarsening, _graclus_registry, _num_nodes, pool_edge
from .scatter import softmax


class UnpoolInfo(NamedTuple):
    """What `EdgePooling.unpool` needs: the input's edge_index and batch, `cluster` [N] = the pooled row of every node,
    `new_edge_score` [C] = the factor every pooled row was multiplied by."""
    edge_index: torch.Tensor
    cluster: torch.Tensor
    batch: Optional[torch.Tensor]
    new_edge_score: torch.Tensor


class _Grouped:
    """An edge_index as the matching reads it: `edges`, grouped by target, every id of it in range (what the gathers go
    through); `src` as the tensor holds it (a short row of a kNN table carries -1 there: no candidate)."""
    __slots__ = ("edges", "src")

    def __init__(self, edges: EdgeList, src: torch.Tensor):
        self.edges, self.src = edges, src


def _check(edge_index: torch.Tensor, who: str) -> None:
    if not torch.is_tensor(edge_index) or edge_index.dim() != 2 or edge_index.shape[0] != 2:
        raise ValueError(f"{who}: edge_index must be an int64 [2, E] tensor")
    if edge_index.dtype != torch.int64:
        raise TypeError(f"{who}: edge_index must be int64 (torch.long), got {edge_index.dtype}")


def _group(edge_index: torch.Tensor, N: int) -> _Grouped:
    """By target.  A knn_graph / radius_graph tensor is grouped as its table wrote it (no sort, no host read); any other
    tensor goes through edge_list_from_edge_index (a stable sort and one host read, which also checks the ids)."""
    hit = lookup_graph(edge_index)
    if hit is not None and hit[1] == "source_to_target" and hit[0].num_nodes == N:
        table = hit[0]
        rowptr, E = table._rowptr()
        if E == edge_index.shape[1]:
            src = edge_index[0].to(torch.int32)
            # only the [2, E] view of a full_rows table can hold -1 (graph.NeighborTable): keep the gathers in range
            safe = src.clamp(min=0) if table.full_rows and not table.dense else src
            return _Grouped(EdgeList(safe, edge_index[1].to(torch.int32), rowptr, N), src)
    edges = edge_list_from_edge_index(edge_index, N, "source_to_target")
    return _Grouped(edges, edges.src)


def _match(g: _Grouped, score: torch.Tensor, ptr: torch.Tensor, who: str, want_rounds: bool = False):
    """The launch and its deferred checks; score [E] fp32 by grouped position."""
    edges = g.edges
    cluster, partner, edge, rounds, flags = _native._edge_match(edges.rowptr, g.src, edges.tgt, edges.perm, score, ptr,
                                                                want_rounds)
    if flags.is_cuda and not torch.cuda.is_current_stream_capturing():       # a captured graph cannot report
        _deferred.post(flags[0:1], f"{who}: an edge_index node id lies outside [0, {edges.num_nodes}): its edge was no "
                                   "candidate")
        _deferred.post(flags[1:2], f"{who}: an edge joins nodes of two events: it was no candidate")
        _deferred.post(flags[2:3], f"{who}: the matching reached its round bound with live edges left (a defect of the "
                                   "kernel): nodes were left unmatched")
    _registry_put(_graclus_registry, cluster, partner)
    return cluster, partner, edge, rounds


def _score_vector(edge_score: torch.Tensor, E: int, who: str) -> torch.Tensor:
    if not torch.is_tensor(edge_score) or not edge_score.is_floating_point():
        raise TypeError(f"{who}: edge_score must be a floating-point tensor of one score per edge")
    if edge_score.dtype == torch.float64:
        raise TypeError(f"{who}: edge_score must be float32, bfloat16 or float16: rounding a float64 score would merge "
                        "distinct scores")
    if edge_score.dim() != 1 or edge_score.numel() != E:
        raise ValueError(f"{who}: edge_score must be [{E}], one score per edge, got {tuple(edge_score.shape)}")
    return edge_score.detach().float()


def edge_matching(edge_index: torch.Tensor, edge_score: torch.Tensor, batch: Optional[torch.Tensor] = None,
                  num_nodes: Optional[int] = None, *, return_rounds: bool = False):
    """The greedy edge contraction of torch_geometric's `EdgePooling._merge_edges` on its own: (cluster, edge).

    The edges of every event are taken in descending canonical score (NaN above +inf, -0.0 = +0.0, as `topk`), ties to the
    lower position in `edge_index`; an edge is taken when both of its ends are still free, and claims them.  A self loop
    claims its one node.  cluster: int64 [N], min(u, v) for a contracted pair, u otherwise (graclus's convention), and
    registered with its partners as a `graclus` result is, so max_pool, avg_pool, max_pool_x and avg_pool_x pool it
    through the pair route.  edge: int64 [N], the position in `edge_index` of the edge that claimed the node, -1 for a
    node nobody claimed.  return_rounds=True: (cluster, edge, rounds int32 [B]), the rounds every event ran.

    edge_index: int64 [2, E] in any order (a knn_graph / radius_graph tensor keeps its table's grouping: no sort, no host
    read; any other tensor is grouped by target with one host read, where an id outside [0, N) is a ValueError).
    edge_score: [E] in the order of edge_index, fp32 (bf16 / fp16 are upcast exactly; float64 is a TypeError).
    batch: the events, one workgroup each (None: one event); N = batch.numel(), else num_nodes, else the largest id + 1
    (one host read).  An edge between two events, and a -1 of a short kNN row, is no candidate and is reported by a
    deferred check (the next operator call or raise_deferred_errors()).  One launch (include/dmet.h,
    dmet_edge_match_f32), the same bits every run.  No host sync with a registered batch and a table's tensor.  Not
    differentiable."""
    _check(edge_index, "edge_matching")
    score = _score_vector(edge_score, edge_index.shape[1], "edge_matching")
    dev = _native._require_device(edge_index, edge_score, batch)
    N = batch.numel() if batch is not None and num_nodes is None else _num_nodes(edge_index, num_nodes)
    ptr = batch_info(batch, N, dev).ptr
    g = _group(edge_index, N)
    if g.edges.perm is not None:
        score = score.index_select(0, g.edges.perm.long())
    _deferred.poll()
    cluster, _partner, edge, rounds = _match(g, score, ptr, "edge_matching", return_rounds)
    return (cluster, edge, rounds) if return_rounds else (cluster, edge)


class EdgePooling(torch.nn.Module):
    """torch_geometric.nn.EdgePooling(in_channels, edge_score_method=None, dropout=0.0, add_to_edge_score=0.5) (unpinned:
    the published source; the parameter is `lin` = Linear(2 * in_channels, 1)):

        raw_e  = lin([x_src(e) || x_dst(e)])                 dropout on raw_e in training
        e      = edge_score_method(raw_e, edge_index, N) + add_to_edge_score        (default: softmax over the edges
                                                                                     of one target; tanh, sigmoid)
        the edges are contracted greedily in descending e (edge_matching)
        new_x_c = (sum of the members of cluster c) * e(the contracted edge of c)   (factor 1 for an unclaimed node)
        forward(x, edge_index, batch) -> (new_x, new_edge_index, new_batch, unpool_info)
        unpool(x, unpool_info)        -> (x / factor gathered back to the nodes, edge_index, batch)

    No [E, 2 F] tensor: lin.weight is split into its source and target halves, two scalars per node are formed, and
    raw_e = a[src] + b[dst] + bias.  The softmax is this package's by-target softmax over the grouped list.  The member sum is
    pair pooling's mean times the member count (exact wherever x_u + x_v is normal), the factor one gathered score per
    pooled row, so every gradient has the same bits every run.  Gradients reach x and lin through the factor and the
    sum, not through the choice of the edges.  new_edge_index is coalesce(cluster[edge_index]), self loops kept, as
    upstream; new_batch comes back registered.

    Deviations from upstream: pooled rows are numbered event by event, in ascending index of the cluster's lowest node
    (upstream numbers them in the order the edges were taken, which interleaves the events and leaves the pooled batch
    unsorted) -- the partition and every per-cluster value are upstream's; score ties go to the lower edge position
    (upstream's unstable argsort leaves them unspecified).  `edge_attr` is not supported.

    Host reads of forward: the pooled size with the largest / smallest pooled event (one read, as graclus + max_pool) and
    the coalesced edge count (torch.unique); plus one for the grouping of an edge_index that is no knn_graph /
    radius_graph tensor, and those of an unregistered batch.  scores(x, edge_index, batch) returns the [E] vector forward
    matches on, in the order of edge_index."""

    def __init__(self, in_channels: int, edge_score_method: Optional[Callable] = None, dropout: float = 0.0,
                 add_to_edge_score: float = 0.5):
        super().__init__()
        self.in_channels = int(in_channels)
        self.compute_edge_score = edge_score_method if edge_score_method is not None else self.compute_edge_score_softmax
        if not callable(self.compute_edge_score):
            raise TypeError("EdgePooling: edge_score_method must be callable (raw_edge_score, edge_index, num_nodes)")
        self.add_to_edge_score = float(add_to_edge_score)
        self.dropout = float(dropout)
        self.lin = torch.nn.Linear(2 * self.in_channels, 1)
        self.reset_parameters()

    def reset_parameters(self):
        self.lin.reset_parameters()

    @staticmethod
    def compute_edge_score_softmax(raw_edge_score: torch.Tensor, edge_index: torch.Tensor, num_nodes: int) -> torch.Tensor:
        """softmax over the edges that share a target (edge_index[1])."""
        return softmax(raw_edge_score, edge_index[1], num_nodes=num_nodes)

    @staticmethod
    def compute_edge_score_tanh(raw_edge_score: torch.Tensor, edge_index: Optional[torch.Tensor] = None,
                                num_nodes: Optional[int] = None) -> torch.Tensor:
        return torch.tanh(raw_edge_score)

    @staticmethod
    def compute_edge_score_sigmoid(raw_edge_score: torch.Tensor, edge_index: Optional[torch.Tensor] = None,
                                   num_nodes: Optional[int] = None) -> torch.Tensor:
        return torch.sigmoid(raw_edge_score)

    # ---- scores ----------------------------------------------------------------------------------------------------------
    def _grouped_scores(self, x: torch.Tensor, edge_index: torch.Tensor, g: _Grouped) -> torch.Tensor:
        """e [E] fp32 by grouped position."""
        edges, N, F = g.edges, x.shape[0], self.in_channels
        w = self.lin.weight.float().view(2, F)
        ab = x @ w.t()                                  # [N, 2]: the source and the target scalar of every node
        zero = torch.zeros_like(ab[:, 0])
        # [0 | b[tgt] | a[src] - 0 | 0 - b[tgt]] per edge: both gathers exact, their backward the by-row / by-source sums of
        # the edge list (no float atomics)
        feat = _EdgeFeaturesXY.apply(torch.stack([ab[:, 0], zero], 1), torch.stack([zero, ab[:, 1]], 1), edges)
        raw = feat[:, 2] + feat[:, 1] + self.lin.bias.float()
        raw = torch.nn.functional.dropout(raw, p=self.dropout, training=self.training)
        fn = self.compute_edge_score
        if fn is EdgePooling.compute_edge_score_softmax:
            e = softmax(raw, ptr=edges.rowptr)
        elif fn in (EdgePooling.compute_edge_score_tanh, EdgePooling.compute_edge_score_sigmoid):
            e = fn(raw)
        else:                                           # a caller's method sees the caller's order
            e = self._to_grouped(fn(self._to_caller(raw, edges), edge_index, N).float(), edges)
        return e + self.add_to_edge_score

    @staticmethod
    def _to_caller(v: torch.Tensor, edges: EdgeList) -> torch.Tensor:
        return v if edges.perm is None else torch.zeros_like(v).index_copy(0, edges.perm.long(), v)

    @staticmethod
    def _to_grouped(v: torch.Tensor, edges: EdgeList) -> torch.Tensor:
        return v if edges.perm is None else v.index_select(0, edges.perm.long())

    def _inputs(self, x: torch.Tensor, edge_index: torch.Tensor, batch: Optional[torch.Tensor]):
        _check(edge_index, "EdgePooling")
        if not torch.is_tensor(x) or not x.is_floating_point() or x.dtype == torch.float64:
            raise TypeError("EdgePooling: x must be a float32, bfloat16 or float16 tensor")
        x = x.unsqueeze(-1) if x.dim() == 1 else x
        if x.dim() != 2 or x.shape[1] != self.in_channels:
            raise ValueError(f"EdgePooling: x must be [N, {self.in_channels}], got {tuple(x.shape)}")
        dev = _native._require_device(x, edge_index, batch)
        binfo = batch_info(batch, x.shape[0], dev)
        return x, binfo

    def scores(self, x: torch.Tensor, edge_index: torch.Tensor, batch: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The fp32 score [E] that forward matches on (forward's partition is a pure function of it), in the order of
        edge_index.  In training with dropout > 0 every call draws its own mask."""
        x, _binfo = self._inputs(x, edge_index, batch)
        if edge_index.shape[1] == 0:
            return torch.zeros(0, dtype=torch.float32, device=x.device)
        g = _group(edge_index, x.shape[0])
        return self._to_caller(self._grouped_scores(x.float(), edge_index, g), g.edges)

    # ---- the layer ---------------------------------------------------------------------------------------------------------
    def forward(self, x: torch.Tensor, edge_index: torch.Tensor, batch: Optional[torch.Tensor] = None
                ) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor], UnpoolInfo]:
        x, binfo = self._inputs(x, edge_index, batch)
        N, dev = x.shape[0], x.device
        if N == 0:
            ones = torch.ones(0, dtype=torch.float32, device=dev)
            return x, edge_index, batch, UnpoolInfo(edge_index, torch.zeros(0, dtype=torch.int64, device=dev), batch, ones)
        xf = x.float()
        g = _group(edge_index, N)
        if edge_index.shape[1]:
            e = self._grouped_scores(xf, edge_index, g)
        else:
            e = torch.zeros(0, dtype=torch.float32, device=dev)
        _deferred.poll()
        cluster, partner, edge, _rounds = _match(g, e.detach(), binfo.ptr, "EdgePooling")
        co = _Coarsening(cluster, batch, N)             # the pair route: pooled rows in ascending leader index
        C = co.C
        # per pooled row: its leader (the lowest member), through which the member count and the claiming edge are read
        leader = torch.zeros(C, dtype=torch.int64, device=dev).scatter_reduce_(
            0, co.node_map, torch.arange(N, dtype=torch.int64, device=dev), "amin", include_self=False)
        members = 1 + (partner.index_select(0, leader) >= 0).to(torch.float32)
        claimed = edge.index_select(0, leader)
        if edge_index.shape[1]:
            picked = self._to_caller(e, g.edges).index_select(0, claimed.clamp(min=0))      # one read per taken edge
            new_edge_score = torch.where(claimed >= 0, picked, torch.ones_like(picked))
        else:
            new_edge_score = torch.ones(C, dtype=torch.float32, device=dev)
        summed = co.pool(xf, "mean") * members.unsqueeze(1)       # (x_u + x_v) * 0.5 * 2
        new_x = summed * new_edge_score.unsqueeze(1)
        new_edge_index, _attr = pool_edge(co.node_map, edge_index, None, C, self_loops=True)
        new_batch = co.pooled_batch()
        info = UnpoolInfo(edge_index=edge_index, cluster=co.node_map, batch=batch, new_edge_score=new_edge_score)
        return (new_x if x.dtype == torch.float32 else new_x.to(x.dtype)), new_edge_index, new_batch, info

    def unpool(self, x: torch.Tensor, unpool_info: UnpoolInfo) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
        """Upstream's unpool: every node gets its pooled row divided by the row's factor."""
        new_x = x / unpool_info.new_edge_score.view(-1, 1).to(x.dtype)
        return new_x.index_select(0, unpool_info.cluster), unpool_info.edge_index, unpool_info.batch

    def __repr__(self):
        return f"{type(self).__name__}({self.in_channels})"

"""Score-based selection pooling with the torch_geometric signatures: `topk`, `filter_adj`, `TopKPooling`, `SAGPooling`,
`SortAggregation` / `global_sort_pool`, plus `filter_table` for this package's neighbour tables.

The kernels are in csrc/select.hip (include/dmet.h, section "Selection pooling"): one ranked selection per event in one
launch (descending canonical score, ties to the lower index, NaN above +inf, -0.0 = +0.0; the same bits every run), the
gather-and-gate of the kept rows with its whole backward, and the induced subgraph of a table or of an edge index.  This
file is argument checking, the m_b rules and the autograd plumbing.  The activations (tanh, sigmoid, softmax) are applied to
the [N] score vector by torch / this package's softmax before the kernels see it.
"""
from __future__ import annotations

import math
import numbers
import struct
from typing import Callable, Optional, Tuple, Union

import torch
from torch.autograd.function import once_differentiable

from . import _native
from .gcn import GraphConv
from .graph import BipartiteTable, GraphFuture, NeighborTable, _deferred, batch_info, register_batch
from .scatter import scatter_max, softmax


def _fp32(v: float) -> float:
    return struct.unpack("f", struct.pack("f", v))[0]


def _check_ratio(ratio) -> Union[int, float]:
    if isinstance(ratio, bool) or not isinstance(ratio, numbers.Real):
        raise ValueError(f"ratio must be a float in (0, 1] or an int >= 1, got {ratio!r}")
    if isinstance(ratio, numbers.Integral):
        if ratio < 1:
            raise ValueError(f"an int ratio must be >= 1, got {ratio!r}")
        return int(ratio)
    if not 0.0 < float(ratio) <= 1.0:
        raise ValueError(f"a float ratio must lie in (0, 1], got {ratio!r}")
    return float(ratio)


def _m_host(n: int, ratio) -> int:
    """m_b of an event of n nodes, on the host: the fp32 product and ceil of the device rule, or min(ratio, n)."""
    if isinstance(ratio, int):
        return min(ratio, int(n))
    return int(math.ceil(_fp32(_fp32(float(n)) * _fp32(ratio))))


def _m_device(deg: torch.Tensor, ratio) -> torch.Tensor:
    if isinstance(ratio, int):
        return deg.clamp(max=ratio)
    return torch.ceil(deg.to(torch.float32) * ratio).to(torch.int64)


class Selection:
    """What a ranked selection leaves behind: perm[M] int64 (grouped by event, best first), node_map[N] int32 (position in
    perm or -1), the pooled ptr[B+1], B, and the largest / smallest pooled event as far as the host knows them."""
    __slots__ = ("perm", "node_map", "ptr", "num_events", "max_nodes", "min_nodes")

    def __init__(self, perm, node_map, ptr, num_events, max_nodes, min_nodes):
        self.perm, self.node_map, self.ptr, self.num_events = perm, node_map, ptr, num_events
        self.max_nodes, self.min_nodes = max_nodes, min_nodes

    def batch(self) -> torch.Tensor:
        """The pooled batch vector (= batch[perm]: perm is grouped by event), registered with the pooled ptr and sizes
        where the host knows the sizes (the min_score rule leaves them unknown and the vector unregistered)."""
        M = self.perm.numel()
        b = torch.repeat_interleave(torch.arange(self.num_events, device=self.perm.device), self.ptr.diff(), output_size=M)
        if self.max_nodes is not None:
            register_batch(b, self.ptr, self.num_events, max_nodes=self.max_nodes, min_nodes=self.min_nodes)
        return b


def _events(x: torch.Tensor, batch, ptr, batch_size):
    N, dev = x.shape[0], x.device
    if ptr is not None:
        if not torch.is_tensor(ptr) or ptr.dtype != torch.int64 or ptr.dim() != 1 or ptr.numel() < 1:
            raise TypeError("ptr must be a 1-D int64 (torch.long) tensor of B + 1 event offsets")
        if ptr.device != dev:
            raise RuntimeError("deepmetv2_amd: all tensors must live on the same device")
        return ptr, ptr.numel() - 1, None, None
    info = batch_info(batch, N, dev, batch_size)
    return info.ptr, info.num_events, info.max_nodes, info.min_nodes


def _select(score: torch.Tensor, ratio, batch=None, ptr=None, batch_size=None) -> Selection:
    """The ranked selection of every event of `score` [N] (fp32 on the device).  M is formed on the host, with no sync,
    when the registered batch has equal event sizes, or `ratio` is an int and the registered min_nodes >= ratio; else it
    costs one read (which then also brings the pooled sizes if the batch's own are unknown)."""
    ptr, B, mx, mn = _events(score, batch, ptr, batch_size)
    dev = score.device
    if B == 0:
        z = torch.zeros(1, dtype=torch.int64, device=dev)
        return Selection(torch.zeros(0, dtype=torch.int64, device=dev),
                         torch.full((score.numel(),), -1, dtype=torch.int32, device=dev), z, 0, 0, 0)
    m = _m_device(ptr[1:] - ptr[:-1], ratio)
    out_ptr = torch.nn.functional.pad(torch.cumsum(m, 0), (1, 0))
    pmx = _m_host(mx, ratio) if mx is not None else None        # m_b is monotone in n_b: the largest event's is the largest
    pmn = _m_host(mn, ratio) if mn is not None else None
    if mx is not None and mn is not None and mx == mn:
        M = B * pmx
    elif isinstance(ratio, int) and mn is not None and mn >= ratio:
        M = B * ratio
    elif mx is not None and mn is not None:
        M = int(out_ptr[-1].item())
    else:
        M, pmx, pmn = (int(v) for v in torch.stack([out_ptr[-1], m.max(), m.min()]).tolist())
    perm, node_map = _native._topk(score, ptr, out_ptr, M)
    return Selection(perm, node_map, out_ptr, B, pmx, pmn)


def _score_vector(x: torch.Tensor) -> torch.Tensor:
    if not torch.is_tensor(x) or not x.is_floating_point():
        raise TypeError("topk: x must be a floating-point tensor of one score per node")
    if x.dim() == 2 and x.shape[1] == 1:
        x = x.view(-1)
    if x.dim() != 1:
        raise ValueError(f"topk: x must be [N] (or [N, 1]), got {tuple(x.shape)}")
    return x.detach().float()


def _select_min_score(score: torch.Tensor, min_score: float, tol: float, batch, ptr, batch_size) -> Selection:
    """Upstream's other rule, composed from scatter_max and torch operators (no kernel of its own): keep
    x > min(min_score, max_b - tol), in index order.  One host sync, the size of the result (nonzero); the pooled event sizes
    stay on the device, so the pooled batch is not registered on this path."""
    p, B, _mx, _mn = _events(score, batch, ptr, batch_size)
    N, dev = score.numel(), score.device
    deg = p[1:] - p[:-1]
    bvec = batch if (batch is not None and ptr is None) else torch.repeat_interleave(
        torch.arange(B, device=dev), deg, output_size=N)
    smax = scatter_max(score.view(-1, 1), bvec, 0, dim_size=B)[0].view(-1)
    smin = (smax - tol).clamp(max=min_score)
    keep = score > smin.index_select(0, bvec)
    perm = keep.nonzero().view(-1)
    M = perm.numel()
    node_map = torch.full((N,), -1, dtype=torch.int32, device=dev)
    node_map[perm] = torch.arange(M, dtype=torch.int32, device=dev)
    m = torch.zeros(B, dtype=torch.int64, device=dev).index_add_(0, bvec, keep.to(torch.int64))
    out_ptr = torch.nn.functional.pad(torch.cumsum(m, 0), (1, 0))
    return Selection(perm, node_map, out_ptr, B, None, None)


def topk(x: torch.Tensor, ratio=0.5, batch: Optional[torch.Tensor] = None, min_score: Optional[float] = None,
         tol: float = 1e-7, *, ptr: Optional[torch.Tensor] = None, batch_size: Optional[int] = None, return_map: bool = False):
    """torch_geometric's `topk` (nn.pool.select.topk): perm, int64 [M], grouped by event, best first -- descending score,
    ties to the lower index, NaN above +inf, -0.0 = +0.0 (include/dmet.h, dmet_topk_f32; one launch, the same bits every
    run).  Not differentiable.

    ratio: a float in (0, 1] keeps m_b = ceil(fp32(n_b) * fp32(ratio)) of the n_b nodes of event b (upstream's rule, and
    fps's); an int >= 1 keeps min(ratio, n_b).  Anything else, a bool included, raises ValueError.
    M is formed on the host, without a sync, when `batch` is registered (register_batch) with equal event sizes, or when
    `ratio` is an int and the registered min_nodes >= ratio; otherwise it costs one read, as in fps.
    min_score: upstream's other rule -- keep x > min(min_score, max_b - tol), in index order.  That path is NOT a kernel:
    it is composed from scatter_max and torch operators and costs one host sync (the layers then return the pooled batch
    unregistered: its event sizes are not read).
    ptr: int64 [B+1] event offsets, non-decreasing from 0 to N and taken on trust, as upstream; when given, `batch` is
    ignored.  return_map=True: (perm, node_map), node_map int32 [N]
    = the position of every node in perm, -1 if it was not picked."""
    score = _score_vector(x)
    _deferred.poll()
    if min_score is not None:
        sel = _select_min_score(score, float(min_score), float(tol), batch, ptr, batch_size)
    else:
        sel = _select(score, _check_ratio(ratio), batch, ptr, batch_size)
    return (sel.perm, sel.node_map) if return_map else sel.perm


def _inverse(node_index: torch.Tensor, num_nodes: int) -> torch.Tensor:
    node_map = torch.full((num_nodes,), -1, dtype=torch.int32, device=node_index.device)
    node_map[node_index] = torch.arange(node_index.numel(), dtype=torch.int32, device=node_index.device)
    return node_map


def filter_adj(edge_index: torch.Tensor, edge_attr: Optional[torch.Tensor], node_index: torch.Tensor,
               num_nodes: Optional[int] = None, *, node_map: Optional[torch.Tensor] = None
               ) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """torch_geometric's `filter_adj`: the subgraph induced by the nodes `node_index` (a perm), relabelled to their
    positions in it: (edge_index' int64 [2, E'], edge_attr[kept] or None).  Kept edges keep the caller's order (a stable
    compaction; include/dmet.h, dmet_filter_edges_count / _write).  One host read, of E' (upstream's result is exact-size
    too).  node_map: the inverse of node_index as topk(..., return_map=True) returns it; without it the inverse is built
    by one scatter over `num_nodes` entries (num_nodes None: the largest id of edge_index and node_index + 1, one more
    read).  An edge with an end
    outside [0, num_nodes) is dropped and a deferred check reports it (the next operator call or
    raise_deferred_errors() raises)."""
    if edge_index.dim() != 2 or edge_index.shape[0] != 2:
        raise ValueError(f"edge_index must be [2, E], got {tuple(edge_index.shape)}")
    _deferred.poll()
    if node_map is None:
        if num_nodes is None:
            tops = [t.max() for t in (edge_index, node_index) if t.numel()]
            num_nodes = int(torch.stack(tops).max().item()) + 1 if tops else 0
        node_map = _inverse(node_index, int(num_nodes))
    out, kept, nbad = _native._filter_edges(edge_index, node_map)
    if edge_index.shape[1] and nbad.is_cuda and not torch.cuda.is_current_stream_capturing():
        _deferred.post(nbad, f"filter_adj: an edge_index node id lies outside [0, {node_map.numel()}): its edge was dropped")
    return out, (edge_attr.index_select(0, kept) if edge_attr is not None else None)


def filter_table(table: NeighborTable, perm: torch.Tensor, node_map: torch.Tensor, ptr: Optional[torch.Tensor], *,
                 max_nodes: Optional[int] = None) -> NeighborTable:
    """The subgraph of a NeighborTable induced by the picked nodes, as a NeighborTable over them: row r is row perm[r],
    its picked entries relabelled through node_map and packed to the left, -1 behind them (include/dmet.h,
    dmet_filter_table).  No edge list, no host sync.  The result is counted (cnt = the entries kept per row), not dense,
    and carries the pooled `ptr`.  max_nodes: the largest pooled event as the caller knows it.  Every consumer of a
    table's max_nodes only compares it against an upper limit or sizes work by it, so an upper BOUND is safe (the layers
    pass m(max_nodes) of the batch's registered largest event, which is exact when that one is)."""
    if isinstance(table, GraphFuture):
        table = table.result()
    if isinstance(table, BipartiteTable):
        raise ValueError("filter_table: a BipartiteTable has two node sets; selection pooling needs a one-set NeighborTable")
    if not isinstance(table, NeighborTable):
        raise TypeError(f"filter_table: expected a NeighborTable, got {type(table).__name__}")
    table.join()
    out_nbr, out_cnt = _native._filter_table(table.nbr, table.cnt, perm, node_map)
    return NeighborTable(out_nbr, ptr, dense=False, max_nodes=max_nodes, cnt=out_cnt)


class _SelectRows(torch.autograd.Function):
    """out = x[perm] * s[perm][:, None] (s None: x[perm]); rows with perm < 0 are zeros.  fp32.  `once_differentiable`."""

    @staticmethod
    def forward(ctx, x, s, perm, node_map):
        # x is needed for the gradient of s alone
        ctx.save_for_backward(x if s is not None and ctx.needs_input_grad[1] else None, s, node_map)
        return _native._select_rows(x, s, perm)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, s, node_map = ctx.saved_tensors
        need_gx = ctx.needs_input_grad[0]
        need_gs = s is not None and ctx.needs_input_grad[1]
        if not (need_gx or need_gs):
            return None, None, None, None
        gx, gs = _native._select_rows_bwd(g, x, s, node_map, need_gx, need_gs)
        return gx, gs, None, None


def select_rows(x: torch.Tensor, s: Optional[torch.Tensor], perm: torch.Tensor, node_map: torch.Tensor) -> torch.Tensor:
    """x[perm] * s[perm][:, None] for x [N, F] (s None: the gather alone), differentiable through x and s; a row with
    perm < 0 is zeros.  bf16 / fp16 operands are gated in fp32 and returned in x's dtype."""
    out = _SelectRows.apply(x.float(), None if s is None else s.float(), perm, node_map)
    return out if x.dtype == torch.float32 else out.to(x.dtype)


def _activation(nonlinearity) -> Callable:
    if callable(nonlinearity):
        return nonlinearity
    fn = getattr(torch, str(nonlinearity), None)
    if not callable(fn):
        raise ValueError(f"unknown nonlinearity {nonlinearity!r}")
    return fn


class _ScorePooling(torch.nn.Module):
    """What TopKPooling and SAGPooling share: everything after the raw score."""

    def _setup(self, in_channels, ratio, min_score, multiplier, nonlinearity):
        self.in_channels = in_channels
        self.ratio = _check_ratio(ratio) if min_score is None else ratio
        self.min_score = min_score
        self.multiplier = multiplier
        self.nonlinearity = _activation(nonlinearity)

    def _raw_score(self, attn, graph):
        raise NotImplementedError

    @staticmethod
    def _resolve(edge_index, edge_attr, who):
        if isinstance(edge_index, GraphFuture):
            edge_index = edge_index.result()
        if isinstance(edge_index, BipartiteTable):
            raise ValueError(f"{who}: a BipartiteTable has two node sets; selection pooling needs a one-set graph")
        if isinstance(edge_index, NeighborTable):
            if edge_attr is not None:
                raise ValueError(f"{who}: edge_attr over a NeighborTable is not supported; pass the [2, E] edge_index")
            return edge_index
        if not torch.is_tensor(edge_index) or edge_index.dim() != 2 or edge_index.shape[0] != 2:
            raise ValueError(f"{who}: edge_index must be an int64 [2, E] tensor, a NeighborTable or a GraphFuture")
        return edge_index

    def scores(self, x: torch.Tensor, edge_index, batch: Optional[torch.Tensor] = None,
               attn: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The full activated fp32 score [N] that forward ranks (forward's perm is a pure function of it)."""
        graph = self._resolve(edge_index, None, type(self).__name__)
        return self._scores(x, graph, batch, attn)

    def _scores(self, x, graph, batch, attn):
        attn = x if attn is None else attn
        attn = attn.unsqueeze(-1) if attn.dim() == 1 else attn
        raw = self._raw_score(attn.float(), graph)
        if self.min_score is None:
            return self.nonlinearity(raw)
        if batch is None:
            batch = torch.zeros(raw.numel(), dtype=torch.int64, device=raw.device)
            register_batch(batch, torch.tensor([0, raw.numel()], dtype=torch.int64, device=raw.device), 1,
                           max_nodes=raw.numel(), min_nodes=raw.numel())
        return softmax(raw, batch)

    def forward(self, x: torch.Tensor, edge_index, edge_attr: Optional[torch.Tensor] = None,
                batch: Optional[torch.Tensor] = None, attn: Optional[torch.Tensor] = None):
        graph = self._resolve(edge_index, edge_attr, type(self).__name__)
        x = x.unsqueeze(-1) if x.dim() == 1 else x
        score = self._scores(x, graph, batch, attn)
        _deferred.poll()
        if self.min_score is None:
            sel = _select(score.detach(), self.ratio, batch)
        else:
            sel = _select_min_score(score.detach(), float(self.min_score), 1e-7, batch, None, None)
        out = select_rows(x, score, sel.perm, sel.node_map)
        if self.multiplier != 1:
            out = self.multiplier * out
        kept_score = select_rows(score.view(-1, 1), None, sel.perm, sel.node_map).view(-1).to(x.dtype)
        pooled_batch = sel.batch()
        if isinstance(graph, NeighborTable):
            new_graph, new_attr = filter_table(graph, sel.perm, sel.node_map, sel.ptr, max_nodes=sel.max_nodes), None
        else:
            new_graph, new_attr = filter_adj(graph, edge_attr, sel.perm, score.numel(), node_map=sel.node_map)
        return out, new_graph, new_attr, pooled_batch, sel.perm, kept_score


class _SelectWeight(torch.nn.Module):
    """Holds `weight` [1, in_channels] under the name upstream publishes since 2.3 (`select.weight`)."""

    def __init__(self, in_channels: int):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.zeros(1, in_channels))


class TopKPooling(_ScorePooling):
    """torch_geometric.nn.TopKPooling(in_channels, ratio=0.5, min_score=None, multiplier=1.0, nonlinearity='tanh')
    (unpinned: the published source; the parameter is `select.weight` [1, in_channels] as there since 2.3, and a
    state_dict with the older bare `weight` loads too).

        score = nonlinearity((x . w) / ||w||_2)              min_score None
        score = softmax(x . w, batch)                        with min_score (this package's softmax)
        perm  = topk(score, ratio, batch, min_score)
        forward(x, edge_index, edge_attr=None, batch=None, attn=None)
            -> (x[perm] * score[perm] * multiplier, edge_index', edge_attr', batch[perm], perm, score[perm])

    edge_index: an int64 [2, E] tensor gives a tensor out (filter_adj: one host read, of E'); a NeighborTable or
    GraphFuture gives a NeighborTable out (filter_table: no edge list and no sync; edge_attr is refused there).  A
    BipartiteTable is refused.  The pooled batch comes back registered (register_batch with the pooled ptr and sizes), so
    the next knn_graph on the kept nodes needs no sync.  bf16 / fp16 x is ranked and gated in fp32 and returned in its own
    dtype.  Gradients reach x and select.weight through the gate (not through the ranking).  scores(...) returns the [N]
    score forward ranks."""

    def __init__(self, in_channels: int, ratio=0.5, min_score: Optional[float] = None, multiplier: float = 1.0,
                 nonlinearity="tanh"):
        super().__init__()
        self._setup(in_channels, ratio, min_score, multiplier, nonlinearity)
        self.select = _SelectWeight(in_channels)
        self._register_load_state_dict_pre_hook(self._legacy_weight)
        self.reset_parameters()

    @staticmethod
    def _legacy_weight(state_dict, prefix, *_args):
        old = prefix + "weight"
        if old in state_dict and prefix + "select.weight" not in state_dict:
            state_dict[prefix + "select.weight"] = state_dict.pop(old)

    def reset_parameters(self):
        bound = 1.0 / math.sqrt(self.in_channels)         # upstream's `uniform(in_channels, weight)`
        with torch.no_grad():
            self.select.weight.uniform_(-bound, bound)

    def _raw_score(self, attn, graph):
        w = self.select.weight.float()
        raw = (attn * w).sum(dim=-1)
        return raw / w.norm(p=2, dim=-1) if self.min_score is None else raw

    def __repr__(self):
        what = f"ratio={self.ratio}" if self.min_score is None else f"min_score={self.min_score}"
        return f"{type(self).__name__}({self.in_channels}, {what}, multiplier={self.multiplier})"


class SAGPooling(_ScorePooling):
    """torch_geometric.nn.SAGPooling(in_channels, ratio=0.5, GNN=GraphConv, min_score=None, multiplier=1.0,
    nonlinearity='tanh', **kwargs) (unpinned): self.gnn = GNN(in_channels, 1, **kwargs) from this package (GraphConv,
    GCNConv, SAGEConv, GATConv, ...),

        score = nonlinearity(gnn(attn or x, graph).view(-1))        (softmax(., batch) with min_score)

    and the rest as TopKPooling.  This is the formula of the paper and of upstream before 2.3; newer upstream passes the
    GNN output through a [1, 1] select weight, which only contributes a sign, and is not followed here."""

    def __init__(self, in_channels: int, ratio=0.5, GNN=GraphConv, min_score: Optional[float] = None, multiplier: float = 1.0,
                 nonlinearity="tanh", **kwargs):
        super().__init__()
        self._setup(in_channels, ratio, min_score, multiplier, nonlinearity)
        self.gnn = GNN(in_channels, 1, **kwargs)

    def reset_parameters(self):
        self.gnn.reset_parameters()

    def _raw_score(self, attn, graph):
        return self.gnn(attn, graph).view(-1).float()

    def __repr__(self):
        what = f"ratio={self.ratio}" if self.min_score is None else f"min_score={self.min_score}"
        return f"{type(self).__name__}({type(self.gnn).__name__}, {self.in_channels}, {what}, multiplier={self.multiplier})"


def global_sort_pool(x: torch.Tensor, batch: Optional[torch.Tensor], k: int, *, ptr: Optional[torch.Tensor] = None,
                     batch_size: Optional[int] = None) -> torch.Tensor:
    """torch_geometric.nn.global_sort_pool: every event's rows ranked by their LAST channel (descending, ties to the lower
    index), the first k of them side by side as [B, k * F], zero-padded for events shorter than k.  One dmet_topk_f32 with
    k slots per event -- M = B k is known on the host, so there is no sync once the batch is registered -- and one
    dmet_select_rows_f32; short events end in -1 slots, which come out as zero rows.  Differentiable through x."""
    if isinstance(k, bool) or not isinstance(k, numbers.Integral) or k < 1:
        raise ValueError(f"k must be an int >= 1, got {k!r}")
    if x.dim() != 2 or x.shape[1] < 1:
        raise ValueError(f"x must be [N, F] with F >= 1, got {tuple(x.shape)}")
    _deferred.poll()
    p, B, _mx, _mn = _events(x, batch, ptr, batch_size)
    out_ptr = torch.arange(0, (B + 1) * int(k), int(k), dtype=torch.int64, device=x.device)
    perm, node_map = _native._topk(x[:, -1].detach().float().contiguous(), p, out_ptr, B * int(k))
    return select_rows(x, None, perm, node_map).view(B, int(k) * x.shape[1])


class SortAggregation(torch.nn.Module):
    """torch_geometric.nn.aggr.SortAggregation(k): global_sort_pool as a module; forward(x, index=None, ptr=None,
    dim_size=None) -> [B, k * F]."""

    def __init__(self, k: int):
        super().__init__()
        if isinstance(k, bool) or not isinstance(k, numbers.Integral) or k < 1:
            raise ValueError(f"k must be an int >= 1, got {k!r}")
        self.k = int(k)

    def forward(self, x: torch.Tensor, index: Optional[torch.Tensor] = None, ptr: Optional[torch.Tensor] = None,
                dim_size: Optional[int] = None, dim: int = -2) -> torch.Tensor:
        if dim not in (-2, 0):
            raise NotImplementedError("SortAggregation: only dim=-2 of [N, F] rows is implemented")
        return global_sort_pool(x, index, self.k, ptr=ptr, batch_size=dim_size)

    def __repr__(self):
        return f"{type(self).__name__}(k={self.k})"

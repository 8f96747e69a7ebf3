"""GCNConv, GraphConv, SAGEConv and GINConv (torch_geometric.nn) over this package's graphs, and gcn_norm.

All four aggregate with csrc/weighted_sum.hip through propagate.weighted_aggregate: out_i = sum_e w_e x_j over a
NeighborTable, a BipartiteTable or a grouped edge list, differentiable in x and in the edge weights, without an [E, F]
tensor and without float atomics.  GCNConv runs fused: the symmetric normalisation D^-1/2 (A + I) D^-1/2 is applied at
node level on both sides of the aggregation, so no normalised [E] weight is written and the graph is never rewritten to
add self loops.  The Linears stay torch modules with PyG's attribute names.

PyG is not installed next to this package: the parameter names and shapes follow PyG's published source and are
**unpinned** -- no PyG checkpoint has been loaded against them.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _native
from ._softmax_conv import SoftmaxConv
from .graph import BipartiteTable, EdgeList, GraphFuture, NeighborTable, edge_list_from_edge_index, lookup_graph
from .pna import multi_aggregate
from .propagate import _aggregate, _sizes

MAX_FEATURES = _native.WEIGHTED_SUM_MAX_F


def gcn_norm(graph, edge_weight: Optional[torch.Tensor], num_nodes: int, improved: bool = False,
             add_self_loops: bool = True) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """(dinv [N], self_weight [N] or None) of GCN's symmetric normalisation over a one-set graph (a -1-padded
    NeighborTable or an EdgeList), edge_weight per position as weighted_aggregate takes it (None: ones).

    deg_i = sum_e w_e over row i -- weighted_aggregate of a ones column, so the gradient reaches edge_weight through the
    degree.  With add_self_loops every node without a written i -> i entry gets one implicit loop of weight fill = 2 if
    improved else 1: self_weight_i = fill there and 0 where a loop is written, and deg_i includes it.  dinv = deg^-1/2,
    0 where deg == 0.  This is torch_geometric.utils.add_remaining_self_loops' meaning: a written self loop stays as
    written.  One deviation: several written loops on one node all count (upstream keeps one of them).  The mask of
    written loops is node-level torch work over nbr or (src, tgt); the graph itself is never rewritten.

    The normalised operator is  out = dinv * weighted_aggregate(dinv * h, graph, w) + self_weight * dinv^2 * h."""
    if isinstance(graph, NeighborTable) and graph.cnt is not None:
        graph = graph.edge_list()
    if isinstance(graph, BipartiteTable) or not isinstance(graph, (NeighborTable, EdgeList)):
        raise ValueError("gcn_norm: the symmetric normalisation needs a one-set graph (a NeighborTable or an EdgeList)")
    Nt, Ns, _width = _sizes(graph)
    if Nt != num_nodes or Ns != num_nodes:
        raise ValueError(f"gcn_norm: the graph has {Nt} rows over {Ns} sources, num_nodes={num_nodes}")
    if isinstance(graph, NeighborTable):
        graph.join()
        dev = graph.nbr.device
    else:
        dev = graph.rowptr.device
    ones = torch.ones((num_nodes, 1), dtype=torch.float32, device=dev)
    deg = _aggregate("gcn_norm", ones, graph, edge_weight, "sum")[0].view(-1)
    self_weight = None
    if add_self_loops:
        if isinstance(graph, NeighborTable):
            rows = torch.arange(num_nodes, dtype=graph.nbr.dtype, device=dev).view(-1, 1)
            written = (graph.nbr == rows).any(dim=1)
        else:
            loops = (graph.src == graph.tgt).to(torch.int32)
            written = torch.zeros(num_nodes, dtype=torch.int32, device=dev).scatter_add_(0, graph.tgt.long(), loops) > 0
        self_weight = (~written).to(deg.dtype) * (2.0 if improved else 1.0)
        deg = deg + self_weight
    zero = deg == 0
    dinv = torch.where(zero, torch.zeros_like(deg), torch.where(zero, torch.ones_like(deg), deg).pow(-0.5))
    return dinv, self_weight


class _PropagateConv(SoftmaxConv):
    """The layer plumbing the four convolutions share (x split and messages as SoftmaxConv): what becomes of `edge_index`
    and `edge_weight`, and the refusals."""

    def _refuse(self, kwargs: dict, aggrs) -> str:
        """The constructor's refusals: edge features, an aggregation outside `aggrs`, unknown options.  Returns aggr."""
        who = self.__class__.__name__
        kwargs = dict(kwargs)
        if kwargs.pop("edge_dim", None) is not None:
            raise ValueError(f"{who}: edge features (edge_dim) are not supported")
        aggr = kwargs.pop("aggr", aggrs[0])
        if aggr not in aggrs:
            raise ValueError(f"{who}: aggr={aggr!r} is not supported, one of {list(aggrs)}")
        if kwargs:
            raise TypeError(f"{who}: unknown arguments {sorted(kwargs)}")
        return "add" if aggr == "sum" else aggr

    def _width(self, F: int) -> None:
        if not 1 <= F <= MAX_FEATURES:
            raise ValueError(f"{self.__class__.__name__}: the aggregated rows have {F} features, supported 1..{MAX_FEATURES}")

    def _graph(self, edge_index, edge_weight, num_src: int, num_dst: int, pair: bool):
        """(graph, edge_weight in the graph's position order)."""
        who = self.__class__.__name__
        if edge_weight is not None and not torch.is_tensor(edge_weight):
            raise TypeError(f"{who}: edge_weight must be a tensor or None, got {type(edge_weight).__name__}")
        if isinstance(edge_index, GraphFuture):
            edge_index = edge_index.peek() if isinstance(edge_index.peek(), NeighborTable) else edge_index.result()
        if isinstance(edge_index, EdgeList):        # grouped already: edge_weight is in its order
            if (edge_index.num_nodes, edge_index.num_src) != (num_dst, num_src):
                raise ValueError(f"{who}: the edge list has {edge_index.num_nodes} rows over {edge_index.num_src} sources, x "
                                 f"has {num_dst} and {num_src} rows")
            return edge_index, edge_weight
        if isinstance(edge_index, (NeighborTable, BipartiteTable)):
            if isinstance(edge_index, NeighborTable) and pair:
                raise ValueError(f"{who}: an (x_src, x_dst) pair goes with a BipartiteTable or an edge_index tensor")
            if isinstance(edge_index, BipartiteTable) and not pair:
                raise ValueError(f"{who}: a BipartiteTable needs an (x_src, x_dst) pair")
            nt, ns, _k = _sizes(edge_index)
            if nt != num_dst or ns != num_src:
                raise ValueError(f"{who}: the table has {nt} rows over {ns} sources, x has {num_dst} and {num_src} rows")
            if edge_index.cnt is not None:       # a counted radius table: its valid slots as a list (one host read)
                return edge_index.edge_list(), edge_weight
            return edge_index, edge_weight
        if not torch.is_tensor(edge_index):
            raise TypeError(f"{who}: edge_index must be a graph object or an int64 [2, E] tensor, got "
                            f"{type(edge_index).__name__}")
        hit = None if pair else lookup_graph(edge_index)
        if hit is not None and hit[1] == "source_to_target" and hit[0].num_nodes == num_dst and hit[0].cnt is None:
            table = hit[0]
            # with weights: only a tensor that lists the table's slots in position order (sized Nt*k) runs over the table
            if edge_weight is None or edge_index.shape[1] == table.num_nodes * table.k:
                return table, edge_weight
        edges = edge_list_from_edge_index(edge_index, num_dst, "source_to_target", num_src=num_src if pair else None)
        if edge_weight is not None:
            if tuple(edge_weight.shape) != (edge_index.shape[1],):
                raise ValueError(f"{who}: edge_weight must be [{edge_index.shape[1]}], one scalar per edge, got "
                                 f"{tuple(edge_weight.shape)}")
            if edges.perm is not None:       # into the grouped order; autograd carries the gradient back through it
                edge_weight = edge_weight.index_select(0, edges.perm.long())
        return edges, edge_weight

    def _channels(self, in_channels):
        if isinstance(in_channels, (tuple, list)):
            return int(in_channels[0]), int(in_channels[1])
        return int(in_channels), int(in_channels)


class GCNConv(_PropagateConv):
    """torch_geometric.nn.GCNConv(in_channels, out_channels, improved=False, cached=False, add_self_loops=True,
    normalize=True, bias=True):

        out = D^-1/2 (A + fill I) D^-1/2 (x W^T) + b,    A_ij = w_e of the edge j -> i,  D_ii = sum_j (A + fill I)_ij

    run fused as  h = lin(x),  out = dinv * weighted_aggregate(dinv * h, graph, w) + self_weight * dinv^2 * h + bias  with
    (dinv, self_weight) = gcn_norm(...): no [E] normalised weight and no [E, F] tensor is made, and the self loops are
    never written into the graph (see gcn_norm for their meaning and the one deviation).  cached=True keeps dinv and
    self_weight of the first call on the module.  normalize=False is the plain weighted sum of lin(x).

    forward(x, edge_index, edge_weight=None): edge_index an int64 [2, E] tensor (the tensor of knn_graph runs over its
    table; with edge_weight only when E == N*k, the weights then in position order; anything else is grouped by target
    and edge_weight permuted along), a NeighborTable (edge_weight [N, k] or [N*k]), a GraphFuture or an EdgeList
    (edge_weight in its grouped order).  A BipartiteTable or
    an (x_src, x_dst) pair with normalize=True is a ValueError.  out_channels <= 256.

    Parameters: lin.weight [out, in] (no bias, glorot), bias [out] (zeros) -- PyG's published names, **unpinned**: PyG is
    not installed here."""

    def __init__(self, in_channels: int, out_channels: int, improved: bool = False, cached: bool = False,
                 add_self_loops: bool = True, normalize: bool = True, bias: bool = True, **kwargs):
        super().__init__()
        self._refuse(kwargs, ("add", "sum"))
        self._width(out_channels)
        self.in_channels, self.out_channels = in_channels, out_channels
        self.improved, self.cached, self.add_self_loops, self.normalize = bool(improved), bool(cached), bool(add_self_loops), \
            bool(normalize)
        self.lin = torch.nn.Linear(in_channels, out_channels, bias=False)
        self.bias = torch.nn.Parameter(torch.zeros(out_channels)) if bias else None
        self._cached_norm = None
        self.reset_parameters()

    def reset_parameters(self) -> None:
        torch.nn.init.xavier_uniform_(self.lin.weight)
        if self.bias is not None:
            torch.nn.init.zeros_(self.bias)
        self._cached_norm = None

    def forward(self, x, edge_index, edge_weight: Optional[torch.Tensor] = None) -> torch.Tensor:
        pair, x_src, x_dst = self._split(x)
        if self.normalize and (pair or isinstance(edge_index, BipartiteTable)):
            raise ValueError("GCNConv: the symmetric normalisation needs one node set; a BipartiteTable or an (x_src, x_dst) "
                             "pair goes with normalize=False")
        graph, w = self._graph(edge_index, edge_weight, x_src.shape[0], x_dst.shape[0], pair)
        h = self.lin(x_src)
        if self.normalize:
            norm = self._cached_norm
            if norm is None:
                norm = gcn_norm(graph, w, x_src.shape[0], self.improved, self.add_self_loops)
                if self.cached:
                    self._cached_norm = norm
            dinv, self_weight = norm
            dinv = dinv.to(h.dtype).view(-1, 1)
            out = dinv * _aggregate("GCNConv", dinv * h, graph, w, "sum")[0]
            if self_weight is not None:
                out = out + (self_weight.to(h.dtype).view(-1, 1) * dinv * dinv) * h
        else:
            out = _aggregate("GCNConv", h, graph, w, "sum")[0]
        return out if self.bias is None else out + self.bias

    def __repr__(self) -> str:
        return f"{self.__class__.__name__}({self.in_channels}, {self.out_channels})"


class GraphConv(_PropagateConv):
    """torch_geometric.nn.GraphConv(in_channels, out_channels, aggr='add', bias=True):

        out_i = lin_rel(aggr_j w_e x_j) + lin_root(x_i),    aggr 'add' or 'mean' (the sum over the entry count)

    forward(x, edge_index, edge_weight=None): x a tensor or an (x_src, x_dst) pair (in_channels may be a pair too);
    edge_index as GCNConv's, a BipartiteTable with a pair.  The weighted sum commutes with a Linear, so the layer
    aggregates on the narrower side of lin_rel: x itself when in_channels <= out_channels, else x lin_rel.weight^T, with
    lin_rel's bias added after the aggregation either way.  The narrower side is at most 256 wide.

    Parameters: lin_rel (weight, bias), lin_root (weight) -- PyG's published names, **unpinned**: PyG is not installed
    here."""

    def __init__(self, in_channels, out_channels: int, aggr: str = "add", bias: bool = True, **kwargs):
        super().__init__()
        self.aggr = self._refuse({**kwargs, "aggr": aggr}, ("add", "sum", "mean"))
        self.in_channels, self.out_channels = in_channels, out_channels
        in_src, in_dst = self._channels(in_channels)
        self._width(min(in_src, out_channels))
        self.lin_rel = torch.nn.Linear(in_src, out_channels, bias=bias)
        self.lin_root = torch.nn.Linear(in_dst, out_channels, bias=False)

    def reset_parameters(self) -> None:
        self.lin_rel.reset_parameters()
        self.lin_root.reset_parameters()

    def forward(self, x, edge_index, edge_weight: Optional[torch.Tensor] = None) -> torch.Tensor:
        pair, x_src, x_dst = self._split(x)
        graph, w = self._graph(edge_index, edge_weight, x_src.shape[0], x_dst.shape[0], pair)
        reduce = "mean" if self.aggr == "mean" else "sum"
        if self.lin_rel.in_features <= self.out_channels:
            out = self.lin_rel(_aggregate("GraphConv", x_src, graph, w, reduce)[0])
        else:
            out = _aggregate("GraphConv", torch.nn.functional.linear(x_src, self.lin_rel.weight), graph, w, reduce)[0]
            if self.lin_rel.bias is not None:
                out = out + self.lin_rel.bias
        return out + self.lin_root(x_dst)

    def __repr__(self) -> str:
        return f"{self.__class__.__name__}({self.in_channels}, {self.out_channels}, aggr={self.aggr})"


class SAGEConv(_PropagateConv):
    """torch_geometric.nn.SAGEConv(in_channels, out_channels, aggr='mean', normalize=False, root_weight=True,
    project=False, bias=True):

        out_i = lin_l(aggr_j x_j) + lin_r(x_i),    x_j = relu(lin(x_j)) first with project=True

    aggr 'mean', 'sum' / 'add' (the weighted-sum kernel without weights) or 'max' (multi_aggregate); a node without an
    incoming edge aggregates zeros.  normalize=True: F.normalize(out, p=2, dim=-1).  forward(x, edge_index): x a tensor
    or an (x_src, x_dst) pair; edge_index as GCNConv's, a BipartiteTable with a pair.  in_channels <= 256.

    Parameters: lin_l (weight, bias), lin_r (weight; with root_weight), lin (weight, bias; with project) -- PyG's
    published names, **unpinned**: PyG is not installed here."""

    def __init__(self, in_channels, out_channels: int, aggr: str = "mean", normalize: bool = False, root_weight: bool = True,
                 project: bool = False, bias: bool = True, **kwargs):
        super().__init__()
        self.aggr = self._refuse({**kwargs, "aggr": aggr}, ("mean", "sum", "add", "max"))
        self.in_channels, self.out_channels = in_channels, out_channels
        self.normalize, self.root_weight, self.project = bool(normalize), bool(root_weight), bool(project)
        in_src, in_dst = self._channels(in_channels)
        self._width(in_src)
        if project:
            self.lin = torch.nn.Linear(in_src, in_src, bias=True)
        self.lin_l = torch.nn.Linear(in_src, out_channels, bias=bias)
        if root_weight:
            self.lin_r = torch.nn.Linear(in_dst, out_channels, bias=False)

    def reset_parameters(self) -> None:
        if self.project:
            self.lin.reset_parameters()
        self.lin_l.reset_parameters()
        if self.root_weight:
            self.lin_r.reset_parameters()

    def forward(self, x, edge_index) -> torch.Tensor:
        pair, x_src, x_dst = self._split(x)
        graph, _w = self._graph(edge_index, None, x_src.shape[0], x_dst.shape[0], pair)
        if self.project:        # as upstream: the root term keeps the rows as given
            x_src = self.lin(x_src).relu()
        if self.aggr == "max":
            agg = multi_aggregate(x_src, graph, ("max",))[0][:, 0]
        else:
            agg = _aggregate("SAGEConv", x_src, graph, None, "mean" if self.aggr == "mean" else "sum")[0]
        out = self.lin_l(agg)
        if self.root_weight:
            out = out + self.lin_r(x_dst)
        return torch.nn.functional.normalize(out, p=2.0, dim=-1) if self.normalize else out

    def __repr__(self) -> str:
        return f"{self.__class__.__name__}({self.in_channels}, {self.out_channels}, aggr={self.aggr})"


class GINConv(_PropagateConv):
    """torch_geometric.nn.GINConv(nn, eps=0.0, train_eps=False):  out_i = nn((1 + eps) x_i + sum_j x_j).

    eps is a buffer, or a parameter with train_eps=True.  forward(x, edge_index): x a tensor or an (x_src, x_dst) pair;
    edge_index as GCNConv's, a BipartiteTable with a pair.  x has at most 256 features.

    Names: nn, eps -- PyG's published names, **unpinned**: PyG is not installed here."""

    def __init__(self, nn: torch.nn.Module, eps: float = 0.0, train_eps: bool = False, **kwargs):
        super().__init__()
        self._refuse(kwargs, ("add", "sum"))
        self.nn = nn
        self.initial_eps = float(eps)
        if train_eps:
            self.eps = torch.nn.Parameter(torch.zeros(1))
        else:
            self.register_buffer("eps", torch.zeros(1))
        with torch.no_grad():
            self.eps.fill_(self.initial_eps)

    def reset_parameters(self) -> None:
        for m in self.nn.modules():
            if m is not self.nn and hasattr(m, "reset_parameters"):
                m.reset_parameters()
        with torch.no_grad():
            self.eps.fill_(self.initial_eps)

    def forward(self, x, edge_index) -> torch.Tensor:
        pair, x_src, x_dst = self._split(x)
        self._width(x_src.shape[1])
        graph, _w = self._graph(edge_index, None, x_src.shape[0], x_dst.shape[0], pair)
        out = _aggregate("GINConv", x_src, graph, None, "sum")[0]
        return self.nn(out + (1 + self.eps) * x_dst)

    def __repr__(self) -> str:
        return f"{self.__class__.__name__}(nn={self.nn})"

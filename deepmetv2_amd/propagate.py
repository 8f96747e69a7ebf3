"""Edge-weighted sum aggregation: out_i = sum_e w_e x[src(e)] with a free per-edge weight that takes a gradient of its
own -- torch_geometric's propagate(edge_index, x=x, edge_weight=edge_weight) under aggr='add' and torch_sparse.spmm.

The kernels are csrc/weighted_sum.hip: one gather of the source rows forward, a by-source pass for the gradient of x and a
by-target pass of per-position dot products for the gradient of the weights; no [E, F] tensor, no float atomics (two runs
give the same bits), and over a -1-padded table no edge list and no host sync.  gcn.py builds GCNConv, GraphConv, SAGEConv
and GINConv on it.
"""
from __future__ import annotations

from typing import Optional, Union

import torch
from torch.autograd.function import once_differentiable

from . import _native
from ._softmax_conv import by_source_index, check_graph, graph_args
from .gravnet import _upcast
from .graph import BipartiteTable, EdgeList, NeighborTable, edge_list_from_edge_index
from .pna import _sizes

MAX_FEATURES = _native.WEIGHTED_SUM_MAX_F

Graph = Union[NeighborTable, BipartiteTable, EdgeList]


class _WeightedSum(torch.autograd.Function):
    """(out[Nt, F], count[Nt]) of the weighted sums of x's rows over the rows of `graph`.  Differentiable in x and in w (one
    scalar per position, or None).  `once_differentiable`; saves x, w and the graph: nothing per edge but w itself."""

    @staticmethod
    def forward(ctx, x, w, graph):
        xf = _upcast(x, "x")
        wf = None if w is None else _upcast(w, "edge_weight")
        idx, rowptr, _tgt = graph_args(graph)
        out, count = _native._weighted_sum_fwd(xf, wf, idx, rowptr, _sizes(graph)[0])
        ctx.save_for_backward(xf, wf)
        ctx.graph, ctx.dtype = graph, x.dtype
        ctx.w_like = None if w is None else (w.dtype, w.shape)
        ctx.mark_non_differentiable(count)
        return out.to(x.dtype), count

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out, _g_count):
        xf, wf = ctx.saved_tensors
        graph = ctx.graph
        need_x = ctx.needs_input_grad[0]
        need_w = wf is not None and ctx.needs_input_grad[1]
        idx, rowptr, tgt = graph_args(graph)
        rev_ptr, rev_pos = by_source_index(graph) if need_x else (None, None)
        g_x, g_w = _native._weighted_sum_bwd(g_out.float(), xf, wf, idx, rowptr, tgt, rev_ptr, rev_pos, need_x, need_w)
        if g_x is not None:
            g_x = g_x.to(ctx.dtype)
        if g_w is not None:
            g_w = g_w.view(ctx.w_like[1]).to(ctx.w_like[0])
        return g_x, g_w, None


def _check_weight(who: str, edge_weight, graph):
    if edge_weight is None:
        return None
    if not torch.is_tensor(edge_weight):
        raise TypeError(f"{who}: edge_weight must be a tensor or None, got {type(edge_weight).__name__}")
    Nt, _Ns, width = _sizes(graph)
    if width is not None:
        if tuple(edge_weight.shape) not in ((Nt, width), (Nt * width,)):
            raise ValueError(f"{who}: edge_weight over a table must be [{Nt}, {width}] or [{Nt * width}], got "
                             f"{tuple(edge_weight.shape)}")
    elif tuple(edge_weight.shape) != (graph.num_edges,):
        raise ValueError(f"{who}: edge_weight over an edge list must be [{graph.num_edges}] in the list's grouped order, "
                         f"got {tuple(edge_weight.shape)}")
    return edge_weight


def _aggregate(who: str, x: torch.Tensor, graph, edge_weight, reduce: str):
    """(out, count) behind weighted_aggregate; the layers of gcn.py use the count as well."""
    if not torch.is_tensor(x):
        raise TypeError(f"{who}: x must be a tensor, got {type(x).__name__}")
    if reduce not in ("sum", "add", "mean"):
        raise ValueError(f"{who}: reduce={reduce!r}, supported 'sum' / 'add' and 'mean'")
    if isinstance(graph, (NeighborTable, BipartiteTable)) and graph.cnt is not None:
        graph = graph.edge_list()
    check_graph(who, graph, lambda nt, ns, width, _loops: _native.weighted_sum_check_shapes(x, None, nt, ns, width))
    edge_weight = _check_weight(who, edge_weight, graph)
    out, count = _WeightedSum.apply(x, edge_weight, graph)
    if reduce == "mean":
        out = out / count.clamp(min=1).to(out.dtype).view(-1, 1)
    return out, count


def weighted_aggregate(x: torch.Tensor, graph: Graph, edge_weight: Optional[torch.Tensor] = None,
                       reduce: str = "sum") -> torch.Tensor:
    """out [Nt, F]: out_i = sum_e w_e x[src(e)] over the entries e of row i of `graph`, w_e = 1 without edge_weight.

    graph: a -1-padded NeighborTable (knn_table), a BipartiteTable (knn_xy_table; x belongs to its candidates) or an
    EdgeList (x over its sources); a counted radius table is taken as its edge list (one host read), and edge_weight is
    then in that list's order.  edge_weight: [Nt, k] or [Nt*k] for a table, one scalar per slot (the value in an empty
    slot is never used, and its gradient is 0); [E] in the list's **grouped** order for an EdgeList.  reduce: 'sum' /
    'add', or 'mean' = the sum divided by the number of entries clamped to at least 1 -- PyG's mean of weighted messages,
    which divides by the entry count, not by the weight sum.  A row without an entry gives zeros.

    x [Ns, F], 1 <= F <= 256, table width <= 64, any in-degree in a list; anything else is a ValueError.  Terms are added
    in entry order with one rounding each (fma): the error is at most (n + 2) u sum_e |w_e x_j|, u = 2^-24.
    Differentiable (once) in x and in edge_weight; a gradient nobody needs is not computed.  bf16 input (fp16 under fp16
    autocast) is upcast exactly and the result comes back in x's dtype.  Over a table: no host sync, forward or backward."""
    return _aggregate("weighted_aggregate", x, graph, edge_weight, reduce)[0]


def spmm(index: torch.Tensor, value: torch.Tensor, m: int, n: int, matrix: torch.Tensor) -> torch.Tensor:
    """torch_sparse.spmm(index, value, m, n, matrix): the [m, n] sparse matrix with entries value[e] at (index[0, e],
    index[1, e]) times the dense matrix [n, F]; returns [m, F].  index int64 [2, nnz] in any order -- it is grouped by row
    once (one host read), value is carried into the grouped order and its gradient comes back in the caller's order.
    Duplicate coordinates add, as upstream does on an uncoalesced index.  F <= 256.  Differentiable in value and matrix."""
    if not torch.is_tensor(matrix) or matrix.dim() != 2 or matrix.shape[0] != n:
        raise ValueError(f"spmm: matrix must be [{n}, F], got "
                         f"{tuple(matrix.shape) if torch.is_tensor(matrix) else type(matrix).__name__}")
    if not torch.is_tensor(index) or index.dim() != 2 or index.shape[0] != 2:
        raise ValueError("spmm: index must be an int64 [2, nnz] tensor")
    if not torch.is_tensor(value) or value.dim() != 1 or value.numel() != index.shape[1]:
        raise ValueError(f"spmm: value must be [{index.shape[1]}], one scalar per coordinate")
    edges = edge_list_from_edge_index(index, int(m), "target_to_source", num_src=int(n))      # row 0: the output row
    if edges.perm is not None:
        value = value.index_select(0, edges.perm.long())
    return _aggregate("spmm", matrix, edges, value, "sum")[0]

"""Softmax attention over a graph (torch_geometric.nn.TransformerConv, torch_geometric.utils.softmax): a learned,
normalised weight per neighbour.

The aggregate and its backward are csrc/attention.hip: one gather of a key and a value head row per edge, the running
softmax of a row kept in registers, no [E, H*C] message tensor, no float atomics, and -- over a table -- no edge list and
no host sync.  The Linears and the skip / beta arithmetic stay torch modules with PyG's attribute names.
"""
from __future__ import annotations

from typing import Optional, Tuple, Union

import torch
from torch.autograd.function import once_differentiable

from . import _native
from ._softmax_conv import SoftmaxConv, by_source_index, check_graph, graph_args, shape_alpha
from .gravnet import _upcast
from .graph import BipartiteTable, EdgeList, NeighborTable

MAX_HEADS = _native.ATTENTION_MAX_H
MAX_HEAD_CHANNELS = _native.ATTENTION_MAX_C
MAX_HEADS_TIMES_CHANNELS = _native.ATTENTION_MAX_HC

Graph = Union[NeighborTable, BipartiteTable, EdgeList]


class _AttentionAggregate(torch.autograd.Function):
    """out[i,h,:] = sum over the entries of row i of softmax(q_i . k_j / sqrt(C)) v_j, differentiable in q, k and v.
    `once_differentiable`; saves q, k, v, out and the row's log-sum-exp, nothing per edge."""

    @staticmethod
    def forward(ctx, q, k, v, graph, want_alpha: bool):
        qf, kf, vf = _upcast(q, "q"), _upcast(k, "k"), _upcast(v, "v")
        idx, rowptr, _tgt = graph_args(graph)
        out, lse, alpha = _native.attention_fwd(qf, kf, vf, idx, rowptr, want_alpha)
        ctx.save_for_backward(qf, kf, vf, out, lse)
        ctx.graph = graph
        ctx.dtypes = (q.dtype, k.dtype, v.dtype)
        if alpha is None:
            alpha = out.new_empty(0)
        ctx.mark_non_differentiable(alpha)
        return out.to(v.dtype), alpha

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out, _g_alpha):
        qf, kf, vf, out, lse = ctx.saved_tensors
        graph = ctx.graph
        idx, rowptr, tgt = graph_args(graph)
        rev_ptr, rev_pos = by_source_index(graph)
        g_q, g_k, g_v = _native.attention_bwd(g_out.float(), qf, kf, vf, out, lse, idx, rev_ptr, rev_pos, rowptr, tgt)
        dq, dk, dv = ctx.dtypes
        return g_q.to(dq), g_k.to(dk), g_v.to(dv), None, None


def _aggregate(q, k, v, graph, want_alpha):
    """(out, alpha or None); alpha [Nt, k, H] for a table, [E, H] in the list's grouped order for an EdgeList."""
    check_graph("attention_aggregate", graph,
                lambda nt, ns, width, _loops: _native.attention_check_shapes(q, k, v, nt, ns, width))
    out, alpha = _AttentionAggregate.apply(q, k, v, graph, bool(want_alpha))
    return out, (shape_alpha(alpha, graph, q.shape[0], q.shape[1]) if want_alpha else None)


def attention_aggregate(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, graph: Graph, return_alpha: bool = False):
    """out[Nt, H, C]: for every row i of `graph` and head h, sum_j alpha_ij v[j,h,:] over the row's entries j with
    alpha_i. = softmax_j(q[i,h,:] . k[j,h,:] / sqrt(C)) -- torch_geometric.utils.softmax and the 'add' aggregation of
    TransformerConv in one kernel.  A row without an entry gives zeros.

    graph: a NeighborTable (knn_table; q, k, v over its one node set), a BipartiteTable (knn_xy_table; q belongs to its
    queries, k and v to its candidates) or an EdgeList (q over its targets, k and v over its sources).  Counted radius
    tables are refused.  q [Nt, H, C], k and v [Ns, H, C]; 1 <= C <= 64, 1 <= H <= 16, H*C <= 256, table width <= 64;
    anything else is a ValueError.  Differentiable in q, k and v.  bf16 inputs (fp16 under fp16 autocast) are upcast
    exactly and the result comes back in v's dtype.  With a table and a registered batch: no host sync.

    return_alpha=True: (out, alpha), the weights, detached -- [Nt, k, H] for a table (0 in an empty slot), [E, H] in the
    list's own (grouped) edge order for an EdgeList."""
    out, alpha = _aggregate(q, k, v, graph, return_alpha)
    return (out, alpha) if return_alpha else out


class TransformerConv(SoftmaxConv):
    """torch_geometric.nn.TransformerConv(in_channels, out_channels, heads=1, concat=True, beta=False, dropout=0.0,
    edge_dim=None, bias=True, root_weight=True), flow source_to_target:

        out_i = sum_j softmax_j(lin_query(x_i)_h . lin_key(x_j)_h / sqrt(out_channels)) lin_value(x_j)_h

    per head h, the heads concatenated (concat=True) or averaged, then out + lin_skip(x_i) (root_weight), or with beta
    b = sigmoid(lin_beta([out, x_r, out - x_r])), out = b x_r + (1 - b) out, x_r = lin_skip(x_i).  in_channels may be a
    (source, target) pair.  dropout != 0 and edge_dim are refused with a ValueError: this package has no RNG kernel for
    attention dropout and the kernels take no edge features.  heads <= 16, out_channels <= 64, heads * out_channels <= 256.

    forward(x, edge_index, return_attention_weights=None): x a tensor or an (x_src, x_dst) pair; edge_index a
    GraphFuture, a NeighborTable (knn_table), a BipartiteTable (with a pair), the int64 [2, E] tensor of knn_graph (its
    table is found again) or any other int64 [2, E] tensor (grouped by target, range-checked).  With
    return_attention_weights=True the result is (out, (edge_index, alpha[E, H])) in the caller's edge order, or
    (out, (table, alpha[Nt, k, H])) when a table was passed (a counted radius table goes through its edge list:
    alpha[E, H] over its valid slots in row order).

    PyG is not installed next to this package: the parameter names and shapes (lin_key, lin_query, lin_value, lin_skip,
    lin_beta) follow PyG's published source and are **unpinned** -- no PyG checkpoint has been loaded against them."""

    def __init__(self, in_channels: Union[int, Tuple[int, int]], out_channels: int, heads: int = 1, concat: bool = True,
                 beta: bool = False, dropout: float = 0.0, edge_dim: Optional[int] = None, bias: bool = True,
                 root_weight: bool = True):
        super().__init__()
        self._check_options(heads, out_channels, dropout, edge_dim, size_prefix="")
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.heads = heads
        self.concat = concat
        self.beta = bool(beta and root_weight)
        self.root_weight = root_weight
        self.dropout = 0.0
        self.edge_dim = None
        in_src, in_dst = (in_channels, in_channels) if isinstance(in_channels, int) else in_channels
        self.lin_key = torch.nn.Linear(in_src, heads * out_channels)
        self.lin_query = torch.nn.Linear(in_dst, heads * out_channels)
        self.lin_value = torch.nn.Linear(in_src, heads * out_channels)
        width = heads * out_channels if concat else out_channels
        if root_weight:
            self.lin_skip = torch.nn.Linear(in_dst, width, bias=bias)
        else:
            self.register_parameter("lin_skip", None)
        if self.beta:
            self.lin_beta = torch.nn.Linear(3 * width, 1, bias=False)
        else:
            self.register_parameter("lin_beta", None)
        self.reset_parameters()

    def reset_parameters(self) -> None:
        for lin in (self.lin_key, self.lin_query, self.lin_value, self.lin_skip, self.lin_beta):
            if lin is not None:
                lin.reset_parameters()

    def forward(self, x: Union[torch.Tensor, Tuple[torch.Tensor, torch.Tensor]], edge_index,
                return_attention_weights: Optional[bool] = None):
        pair, x_src, x_dst = self._split(x)
        want = bool(return_attention_weights)
        graph, how = self._resolve(edge_index, x_src.shape[0], x_dst.shape[0], pair, want)
        H, C = self.heads, self.out_channels
        query = self.lin_query(x_dst).view(-1, H, C)
        key = self.lin_key(x_src).view(-1, H, C)
        value = self.lin_value(x_src).view(-1, H, C)
        out, alpha = _aggregate(query, key, value, graph, want)
        out = out.reshape(-1, H * C) if self.concat else out.mean(dim=1)
        if self.lin_skip is not None:
            x_r = self.lin_skip(x_dst)
            if self.lin_beta is not None:
                b = self.lin_beta(torch.cat([out, x_r, out - x_r], dim=-1)).sigmoid()
                out = b * x_r + (1 - b) * out
            else:
                out = out + x_r
        return self._with_alpha(out, edge_index, graph, how, alpha) if want else out

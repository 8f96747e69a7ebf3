"""Graph attention with an additive score (torch_geometric.nn.GATConv, torch_geometric.nn.GATv2Conv): a learned,
normalised weight per neighbour from a LeakyReLU of a sum, not from a dot product.

The aggregate and its backward are csrc/gat.hip: one gather of a source head row per edge and pass (key and value are the
same row), the running softmax of a row kept in registers, no [E, H*C] tensor, no float atomics, self loops taken
implicitly, and -- over a table -- no edge list and no host sync.  The Linears, the products with att_src / att_dst, the
residual and the bias stay torch modules and operators with PyG's attribute names.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple, Union

import torch
from torch.autograd.function import once_differentiable

from . import _native
from ._softmax_conv import SoftmaxConv, by_source_index, check_graph, graph_args, shape_alpha
from .gravnet import _upcast
from .graph import BipartiteTable, EdgeList, GraphFuture, NeighborTable

MAX_HEADS = _native.GAT_MAX_H
MAX_HEAD_CHANNELS = _native.GAT_MAX_C
MAX_HEADS_TIMES_CHANNELS = _native.GAT_MAX_HC

Graph = Union[NeighborTable, BipartiteTable, EdgeList]


class _GatAggregate(torch.autograd.Function):
    """out[i,h,:] = sum over the entries of row i of softmax(score) xl_j.  mode GAT_V2: (a, b) = (xr, att), score =
    att . lrelu(xl_j + xr_i); mode GAT_V1: (a, b) = (s_src, s_dst), score = lrelu(s_src_j + s_dst_i).  Differentiable in
    xl, a and b.  `once_differentiable`; saves the inputs, out and the row's log-sum-exp, nothing per edge."""

    @staticmethod
    def forward(ctx, mode, xl, a, b, graph, slope, self_loops, want_alpha):
        names = ("xr", "att") if mode == _native.GAT_V2 else ("s_src", "s_dst")
        xf, af, bf = _upcast(xl, "xl"), _upcast(a, names[0]), _upcast(b, names[1])
        idx, rowptr, _tgt = graph_args(graph)
        out, lse, alpha = _native._gat_fwd(mode, xf, af, bf, idx, rowptr, slope, self_loops, want_alpha)
        ctx.save_for_backward(xf, af, bf, out, lse)
        ctx.graph, ctx.mode, ctx.slope, ctx.self_loops = graph, mode, slope, self_loops
        ctx.dtypes = (xl.dtype, a.dtype, b.dtype)
        ctx.b_shape = b.shape
        if alpha is None:
            alpha = out.new_zeros(0)
        ctx.mark_non_differentiable(alpha)
        return out.to(xl.dtype), alpha

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out, _g_alpha):
        xf, af, bf, out, lse = ctx.saved_tensors
        graph = ctx.graph
        idx, rowptr, tgt = graph_args(graph)
        rev_ptr, rev_pos = by_source_index(graph)
        g_xl, g_a, g_b = _native._gat_bwd(ctx.mode, g_out.float(), xf, af, bf, out, lse, idx, rev_ptr, rev_pos, rowptr, tgt,
                                         ctx.slope, ctx.self_loops)
        dx, da, db = ctx.dtypes
        return None, g_xl.to(dx), g_a.to(da), g_b.reshape(ctx.b_shape).to(db), None, None, None, None


def _aggregate(who, mode, xl, a, b, graph, slope, self_loops, want_alpha):
    """(out, alpha or None); alpha [Nt, k, H] for a table, [E, H] in the list's grouped order for an EdgeList."""
    for t in (xl, a, b):
        if not torch.is_tensor(t):
            raise TypeError(f"{who}: the inputs must be tensors, got {type(t).__name__}")
    check_graph(who, graph, lambda nt, ns, width, loops: _native.gat_check_shapes(mode, xl, a, b, nt, ns, width, slope, loops),
                self_loops)
    out, alpha = _GatAggregate.apply(mode, xl, a, b, graph, float(slope), bool(self_loops), bool(want_alpha))
    return out, (shape_alpha(alpha, graph, out.shape[0], xl.shape[1]) if want_alpha else None)


def gat_aggregate(xl: torch.Tensor, xr: torch.Tensor, att: torch.Tensor, graph: Graph, negative_slope: float = 0.2,
                  self_loops: bool = False, return_alpha: bool = False):
    """out[Nt, H, C] of GATv2Conv's attention: for every row i of `graph` and head h, sum_j alpha_ij xl[j,h,:] over the
    row's entries j with alpha_i. = softmax_j(sum_c att[h,c] leaky_relu(xl[j,h,c] + xr[i,h,c])) -- edge_update,
    torch_geometric.utils.softmax (without its 1e-16, which is below fp32 rounding beside a denominator >= 1) and the
    'add' aggregation in one kernel.  A row without an entry gives zeros.

    graph: a NeighborTable (knn_table; xl, xr over its one node set), a BipartiteTable (knn_xy_table; xr belongs to its
    queries, xl to its candidates) or an EdgeList (xr over its targets, xl over its sources).  Counted radius tables are
    refused.  xl [Ns, H, C], xr [Nt, H, C], att [H, C] or [1, H, C]; 1 <= C <= 64, 1 <= H <= 16, H*C <= 256, table width
    <= 64, negative_slope finite and >= 0; anything else is a ValueError.  self_loops=True (one node set only): written
    entries j == i are skipped and one entry i -> i is taken after the row's own -- PyG's remove_self_loops +
    add_self_loops without rewriting the graph.  Differentiable in xl, xr and att.  bf16 inputs (fp16 under fp16
    autocast) are upcast exactly and the result comes back in xl's dtype.  With a table and a registered batch: no host
    sync.

    return_alpha=True: (out, alpha), the weights of the written entries, detached -- [Nt, k, H] for a table (0 in an
    empty slot), [E, H] in the list's own (grouped) edge order for an EdgeList; 0 in a written self loop that
    self_loops=True skipped, and the implicit entry's weight is not returned."""
    out, alpha = _aggregate("gat_aggregate", _native.GAT_V2, xl, xr, att, graph, negative_slope, self_loops, return_alpha)
    return (out, alpha) if return_alpha else out


def gat_v1_aggregate(xl: torch.Tensor, s_src: torch.Tensor, s_dst: torch.Tensor, graph: Graph,
                     negative_slope: float = 0.2, self_loops: bool = False, return_alpha: bool = False):
    """out[Nt, H, C] of GATConv's attention: sum_j alpha_ij xl[j,h,:] with alpha_i. = softmax_j(leaky_relu(s_src[j,h] +
    s_dst[i,h])), s_src [Ns, H] = (xl * att_src).sum(-1) and s_dst [Nt, H] = (x_dst * att_dst).sum(-1) formed by the
    caller with torch operators, so att_src and att_dst get their gradients from autograd.  Everything else as
    gat_aggregate; differentiable in xl, s_src and s_dst."""
    out, alpha = _aggregate("gat_v1_aggregate", _native.GAT_V1, xl, s_src, s_dst, graph, negative_slope, self_loops,
                            return_alpha)
    return (out, alpha) if return_alpha else out


def _glorot(t: torch.Tensor) -> None:
    a = math.sqrt(6.0 / (t.size(-2) + t.size(-1)))
    with torch.no_grad():
        t.uniform_(-a, a)


def _linear(n_in: int, n_out: int, bias: bool) -> torch.nn.Linear:
    return torch.nn.Linear(n_in, n_out, bias=bias)


class _GatBase(SoftmaxConv):
    """What GATConv and GATv2Conv share beyond SoftmaxConv: the slope, the self loops and their refusals, the residual
    and the bias."""

    def __init__(self, in_channels, out_channels, heads, concat, negative_slope, dropout, add_self_loops, edge_dim,
                 fill_value, bias, residual):
        super().__init__()
        who = self.__class__.__name__
        self._check_options(heads, out_channels, dropout, edge_dim, size_prefix=f"{who}: ")
        slope = float(negative_slope)
        if not (math.isfinite(slope) and slope >= 0.0):
            raise ValueError(f"{who}: negative_slope={negative_slope!r} must be finite and >= 0")
        if not isinstance(in_channels, int):
            if len(in_channels) != 2:
                raise ValueError(f"{who}: in_channels must be an int or a (source, target) pair")
            if add_self_loops:
                raise ValueError(f"{who}: a (source, target) pair of node sets has no self loops; pass add_self_loops=False")
            in_channels = tuple(in_channels)
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.heads = heads
        self.concat = concat
        self.negative_slope = slope
        self.dropout = 0.0
        self.add_self_loops = bool(add_self_loops)
        self.edge_dim = None
        self.fill_value = fill_value        # only edge features would use it
        self.residual = bool(residual)
        width = heads * out_channels if concat else out_channels
        in_dst = in_channels if isinstance(in_channels, int) else in_channels[1]
        if residual:
            self.res = _linear(in_dst, width, bias=False)
        else:
            self.register_parameter("res", None)
        if bias:
            self.bias = torch.nn.Parameter(torch.zeros(width))
        else:
            self.register_parameter("bias", None)

    def _reset_shared(self) -> None:
        if self.res is not None:
            _glorot(self.res.weight)
        if self.bias is not None:
            torch.nn.init.zeros_(self.bias)

    def _split(self, x):
        pair, x_src, x_dst = super()._split(x)
        if pair and self.add_self_loops:
            raise ValueError(f"{self.__class__.__name__}: an (x_src, x_dst) pair has no self loops; construct the layer with "
                             "add_self_loops=False")
        return pair, x_src, x_dst

    def _resolve(self, edge_index, num_src: int, num_dst: int, pair: bool, want_alpha: bool):
        """SoftmaxConv._resolve's rules, after what add_self_loops=True cannot go with."""
        who = self.__class__.__name__
        if self.add_self_loops:
            if want_alpha:
                raise ValueError(f"{who}: return_attention_weights needs the self loops in the graph itself: build it with "
                                 "them, e.g. knn_table(..., loop=True), and pass add_self_loops=False")
            if isinstance(edge_index.peek() if isinstance(edge_index, GraphFuture) else edge_index, BipartiteTable):
                raise ValueError(f"{who}: a BipartiteTable has two node sets and no self loops; construct the layer with "
                                 "add_self_loops=False")
        return super()._resolve(edge_index, num_src, num_dst, pair, want_alpha)

    def _finish(self, out, x_dst, edge_index, graph, how, alpha, want):
        H, C = self.heads, self.out_channels
        out = out.reshape(-1, H * C) if self.concat else out.mean(dim=1)
        if self.res is not None:
            out = out + self.res(x_dst)
        if self.bias is not None:
            out = out + self.bias
        return self._with_alpha(out, edge_index, graph, how, alpha) if want else out


class GATv2Conv(_GatBase):
    """torch_geometric.nn.GATv2Conv(in_channels, out_channels, heads=1, concat=True, negative_slope=0.2, dropout=0.0,
    add_self_loops=True, edge_dim=None, fill_value='mean', bias=True, share_weights=False, residual=False), flow
    source_to_target:

        x_l = lin_l(x_src), x_r = lin_r(x_dst)
        out_i = sum_j softmax_j(att_h . leaky_relu(x_l[j]_h + x_r[i]_h)) x_l[j]_h

    per head h, the heads concatenated (concat=True) or averaged, plus res(x_dst) (residual) and bias.  lin_r is lin_l
    when share_weights.  in_channels may be a (source, target) pair.  add_self_loops=True (one node set) drops written
    self loops and adds one per node, inside the kernel.  Refused with a ValueError: dropout != 0 (no RNG kernel),
    edge_dim, heads > 16, out_channels > 64, heads * out_channels > 256, add_self_loops=True with a pair or a
    BipartiteTable (pass add_self_loops=False), and return_attention_weights=True with add_self_loops=True (put the loops
    into the graph, e.g. knn_table(..., loop=True), and pass add_self_loops=False).

    forward(x, edge_index, return_attention_weights=None): x a tensor or an (x_src, x_dst) pair; edge_index a
    GraphFuture, a NeighborTable (knn_table), a BipartiteTable (with a pair), the int64 [2, E] tensor of knn_graph (its
    table is found again) or any other int64 [2, E] tensor (grouped by target, range-checked).  With
    return_attention_weights=True the result is (out, (edge_index, alpha[E, H])) in the caller's edge order, or
    (out, (table, alpha[Nt, k, H])) when a table was passed.

    PyG is not installed next to this package: the parameter names and shapes (lin_l, lin_r, att, bias, res) follow PyG's
    published source and are **unpinned** -- no PyG checkpoint has been loaded against them."""

    def __init__(self, in_channels: Union[int, Tuple[int, int]], out_channels: int, heads: int = 1, concat: bool = True,
                 negative_slope: float = 0.2, dropout: float = 0.0, add_self_loops: bool = True,
                 edge_dim: Optional[int] = None, fill_value: Union[float, str] = "mean", bias: bool = True,
                 share_weights: bool = False, residual: bool = False):
        super().__init__(in_channels, out_channels, heads, concat, negative_slope, dropout, add_self_loops, edge_dim,
                         fill_value, bias, residual)
        self.share_weights = bool(share_weights)
        in_src, in_dst = (self.in_channels,) * 2 if isinstance(self.in_channels, int) else self.in_channels
        if share_weights and in_src != in_dst:
            raise ValueError(f"GATv2Conv: share_weights needs equal source and target widths, got {in_src} and {in_dst}")
        self.lin_l = _linear(in_src, heads * out_channels, bias=True)
        self.lin_r = self.lin_l if share_weights else _linear(in_dst, heads * out_channels, bias=True)
        self.att = torch.nn.Parameter(torch.zeros(1, heads, out_channels))
        self.reset_parameters()

    def reset_parameters(self) -> None:
        for lin in (self.lin_l, self.lin_r):
            lin.reset_parameters()
            _glorot(lin.weight)
        _glorot(self.att)
        self._reset_shared()

    def forward(self, x: Union[torch.Tensor, Tuple[torch.Tensor, torch.Tensor]], edge_index,
                return_attention_weights: Optional[bool] = None):
        pair, x_src, x_dst = self._split(x)
        want = bool(return_attention_weights)
        graph, how = self._resolve(edge_index, x_src.shape[0], x_dst.shape[0], pair, want)
        H, C = self.heads, self.out_channels
        xl = self.lin_l(x_src).view(-1, H, C)
        xr = xl if (self.share_weights and not pair) else self.lin_r(x_dst).view(-1, H, C)
        out, alpha = _aggregate("GATv2Conv", _native.GAT_V2, xl, xr, self.att, graph, self.negative_slope,
                                self.add_self_loops, want)
        return self._finish(out, x_dst, edge_index, graph, how, alpha, want)


class GATConv(_GatBase):
    """torch_geometric.nn.GATConv(in_channels, out_channels, heads=1, concat=True, negative_slope=0.2, dropout=0.0,
    add_self_loops=True, edge_dim=None, fill_value='mean', bias=True, residual=False), flow source_to_target:

        x_l = lin(x_src) (lin_src for a pair), s_src = (x_l * att_src).sum(-1), s_dst = (lin(x_dst) * att_dst).sum(-1)
        out_i = sum_j softmax_j(leaky_relu(s_src[j]_h + s_dst[i]_h)) x_l[j]_h

    per head h, the heads concatenated (concat=True) or averaged, plus res(x_dst) (residual) and bias.  An int
    in_channels gives one Linear `lin`, a (source, target) pair gives `lin_src` and `lin_dst`, all without bias.  The
    options, the refusals and forward(x, edge_index, return_attention_weights=None) are GATv2Conv's.

    PyG is not installed next to this package: the parameter names and shapes (lin / lin_src / lin_dst, att_src, att_dst,
    bias, res) follow PyG's published source and are **unpinned** -- no PyG checkpoint has been loaded against them."""

    def __init__(self, in_channels: Union[int, Tuple[int, int]], out_channels: int, heads: int = 1, concat: bool = True,
                 negative_slope: float = 0.2, dropout: float = 0.0, add_self_loops: bool = True,
                 edge_dim: Optional[int] = None, fill_value: Union[float, str] = "mean", bias: bool = True,
                 residual: bool = False):
        super().__init__(in_channels, out_channels, heads, concat, negative_slope, dropout, add_self_loops, edge_dim,
                         fill_value, bias, residual)
        if isinstance(self.in_channels, int):
            self.lin = _linear(self.in_channels, heads * out_channels, bias=False)
            self.lin_src = self.lin_dst = None
        else:
            self.lin = None
            self.lin_src = _linear(self.in_channels[0], heads * out_channels, bias=False)
            self.lin_dst = _linear(self.in_channels[1], heads * out_channels, bias=False)
        self.att_src = torch.nn.Parameter(torch.zeros(1, heads, out_channels))
        self.att_dst = torch.nn.Parameter(torch.zeros(1, heads, out_channels))
        self.reset_parameters()

    def reset_parameters(self) -> None:
        for lin in (self.lin, self.lin_src, self.lin_dst):
            if lin is not None:
                _glorot(lin.weight)
        _glorot(self.att_src)
        _glorot(self.att_dst)
        self._reset_shared()

    def forward(self, x: Union[torch.Tensor, Tuple[torch.Tensor, torch.Tensor]], edge_index,
                return_attention_weights: Optional[bool] = None):
        pair, x_src, x_dst = self._split(x)
        want = bool(return_attention_weights)
        graph, how = self._resolve(edge_index, x_src.shape[0], x_dst.shape[0], pair, want)
        H, C = self.heads, self.out_channels
        lin_src, lin_dst = (self.lin, self.lin) if self.lin is not None else (self.lin_src, self.lin_dst)
        xl = lin_src(x_src).view(-1, H, C)
        xd = xl if (not pair and lin_dst is lin_src) else lin_dst(x_dst).view(-1, H, C)
        s_src = (xl * self.att_src).sum(dim=-1)
        s_dst = (xd * self.att_dst).sum(dim=-1)
        out, alpha = _aggregate("GATConv", _native.GAT_V1, xl, s_src, s_dst, graph, self.negative_slope,
                                self.add_self_loops, want)
        return self._finish(out, x_dst, edge_index, graph, how, alpha, want)

"""Principal Neighbourhood Aggregation (torch_geometric.nn.PNAConv, torch_geometric.nn.aggr.DegreeScalerAggregation):
several statistics of the same neighbour rows -- sum, mean, min, max, var, std -- scaled by functions of the in-degree.

The statistics and their backward are csrc/multi_aggr.hip: every source row is gathered once per walk and all requested
statistics are formed from it in registers; the variance is centred on the row's own mean in a second walk, never a
difference of two fp32 means; the backward runs by source without float atomics; over a -1-padded table there is no edge
list and no host sync.  With PNAConv's default pre_layers=1 the per-edge message W [x_i | x_j] + b is linear and splits
into A_i + B_j, so the layer aggregates the node-level rows B_j and shifts the result by A_i: no per-edge tensor at all.
The Linears, the scalers and the towers' concatenation stay torch modules and operators with PyG's attribute names.
"""
from __future__ import annotations

import os
from typing import List, Optional, Sequence, Union

import torch
from torch.autograd.function import once_differentiable

from . import _native
from ._softmax_conv import by_source_index, check_graph, graph_args
from .gravnet import _upcast
from .graph import BipartiteTable, EdgeList, GraphFuture, NeighborTable, edge_list_from_edge_index, lookup_graph

AGGREGATORS = tuple(_native.MULTI_AGGR_KINDS)
SCALERS = ("identity", "amplification", "attenuation", "linear", "inverse_linear")
MAX_FEATURES = _native.MULTI_AGGR_MAX_F

Graph = Union[NeighborTable, BipartiteTable, EdgeList]


class _Grouping(EdgeList):
    """Per-entry rows grouped by an index, as the edge list the kernels walk: target r lists the rows perm[rowptr[r] :
    rowptr[r+1]] (perm None: the rows are grouped already).  The gather index is the grouping permutation itself, so the
    grouped copy of the rows is never made; every row is listed once, so the by-source index is the inverse permutation."""

    def __init__(self, rowptr: torch.Tensor, perm: Optional[torch.Tensor], num_rows: int, num_entries: int):
        dev = rowptr.device
        self.src = (torch.arange(num_entries, dtype=torch.int32, device=dev) if perm is None
                    else perm.to(torch.int32).contiguous())
        self.rowptr = rowptr
        self.num_nodes = num_rows
        self.num_src = num_entries
        self.num_edges = num_entries
        self.perm = None
        self._by_source = None
        self._tgt = None

    @property
    def tgt(self) -> torch.Tensor:
        if self._tgt is None:
            rows = torch.arange(self.num_nodes, dtype=torch.int32, device=self.rowptr.device)
            self._tgt = torch.repeat_interleave(rows, self.rowptr.diff().long(), output_size=self.num_edges)
        return self._tgt

    def by_source(self):
        if self._by_source is None:
            E = self.num_edges
            ar = torch.arange(E + 1, dtype=torch.int32, device=self.rowptr.device)
            # src is a permutation of the E rows: every element of the inverse is written
            inv = torch.zeros(max(E, 1), dtype=torch.int32, device=ar.device)
            if E:
                inv.index_copy_(0, self.src.long(), ar[:E])
            self._by_source = (ar, inv)
        return self._by_source


def _sizes(graph):
    """(targets, sources, table width or None) of a graph form."""
    if isinstance(graph, EdgeList):
        return graph.num_nodes, graph.num_src, None
    if isinstance(graph, BipartiteTable):
        return graph.num_queries, graph.num_candidates, graph.k
    return graph.num_nodes, graph.num_nodes, graph.k


class _MultiAggregate(torch.autograd.Function):
    """(out[Nt, G, A, F/G], count[Nt]) of the requested statistics of x's rows over the rows of `graph`.  Differentiable in
    x.  `once_differentiable`; saves x, the counts and, as the request needs them, the mean, the variance and the min /
    max positions: nothing per edge."""

    @staticmethod
    def forward(ctx, x, graph, aggrs, groups):
        xf = _upcast(x, "x")
        idx, rowptr, _tgt = graph_args(graph)
        out, count, saved = _native._multi_aggr_fwd(xf, idx, rowptr, _sizes(graph)[0], aggrs, groups)
        ctx.save_for_backward(xf, count, *saved)
        ctx.graph, ctx.aggrs, ctx.groups, ctx.dtype = graph, aggrs, groups, x.dtype
        ctx.mark_non_differentiable(count)
        return out.to(x.dtype), count

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out, _g_count):
        xf, count, mean, var, amin, amax = ctx.saved_tensors
        graph = ctx.graph
        _idx, _rowptr, tgt = graph_args(graph)
        rev_ptr, rev_pos = by_source_index(graph)
        g_x = _native._multi_aggr_bwd(g_out.float(), xf, count, (mean, var, amin, amax), rev_ptr, rev_pos, tgt,
                                      _sizes(graph)[2], ctx.aggrs, ctx.groups)
        return g_x.to(ctx.dtype), None, None, None


def _aggregate_rows(rows: torch.Tensor, rowptr: torch.Tensor, perm: Optional[torch.Tensor], num_rows: int, aggrs,
                    groups: int = 1):
    """(out[n, G, A, F/G], count[n]) of per-entry rows under a grouping (scatter._group_rows): the kernel gathers through
    the grouping permutation."""
    aggrs = tuple(aggrs)
    _native.multi_aggr_check_shapes(rows, aggrs, groups, num_rows, rows.shape[0], None)
    return _MultiAggregate.apply(rows, _Grouping(rowptr, perm, num_rows, rows.shape[0]), aggrs, groups)


def multi_aggregate(x: torch.Tensor, graph: Graph, aggrs: Sequence[str], groups: int = 1):
    """(out, count): the statistics `aggrs` (any of 'sum', 'mean', 'min', 'max', 'var', 'std', each once, in this order in
    the result) of the rows x[j] over the entries j of every row of `graph`, and the number of entries count[Nt] int32.

    out is [Nt, A, F] for groups == 1 and [Nt, G, A, F/G] otherwise: the features split into G groups (PNA's towers)
    with the A statistics side by side inside each.  var = (1/n) sum (x_j - mean)^2, centred on the row's mean (error
    at most (2n+8) u var + ((n+2) u mean|x|)^2, u = 2^-24); std = sqrt(clamp(var, min=1e-5)), exactly 0 where that is
    <= sqrt(1e-5) -- PyG's StdAggregation.  min / max keep the lowest position on ties.  A row without an entry gives
    zeros and count 0.

    Non-finite values: sum, mean and var follow IEEE (a non-finite x[j, f] makes feature f of the rows that list j
    non-finite), and std is NaN where var is: the clamp keeps a NaN, as torch.clamp does.  min / max run over the
    candidates that are numbers, +-inf included, in any order of the row: a NaN never wins and never blocks, and a
    feature whose candidates are all NaN is NaN and receives no gradient -- upstream's amin / amax propagate the NaN
    instead.  Every other row, every other feature and every gradient row of a source that shares no row with j keep
    the bits of the run without the value.

    graph: a NeighborTable (knn_table), a BipartiteTable (knn_xy_table; x belongs to its candidates) or an EdgeList (x
    over its sources); a counted radius table is taken as its edge list (one host read).  x [Ns, F], 1 <= F <= 256,
    F % groups == 0, table width <= 64, any in-degree in a list; anything else is a ValueError.  Differentiable in x
    (once).  bf16 input (fp16 under fp16 autocast) is upcast exactly and the result comes back in x's dtype.  Over a
    -1-padded table: no host sync, forward or backward."""
    if not torch.is_tensor(x):
        raise TypeError(f"multi_aggregate: x must be a tensor, got {type(x).__name__}")
    if isinstance(aggrs, str):
        aggrs = (aggrs,)
    aggrs = tuple(aggrs)
    if isinstance(graph, (NeighborTable, BipartiteTable)) and graph.cnt is not None:
        graph = graph.edge_list()
    check_graph("multi_aggregate", graph,
                lambda nt, ns, width, _loops: _native.multi_aggr_check_shapes(x, aggrs, groups, nt, ns, width))
    out, count = _MultiAggregate.apply(x, graph, aggrs, groups)
    return (out.squeeze(1) if groups == 1 else out), count


def _avg_degrees(deg: torch.Tensor):
    """(avg_deg_lin, avg_deg_log) of an in-degree histogram deg[d] = number of nodes of in-degree d, as PyG computes
    them: sum_d d deg[d] / N and sum_d log(d + 1) deg[d] / N, N = sum_d deg[d]."""
    deg = deg.detach().to(torch.float)
    total = int(deg.sum())
    if deg.dim() != 1 or total <= 0:
        raise ValueError("deg must be a 1-D histogram of in-degrees with at least one node")
    bins = torch.arange(deg.numel(), device=deg.device)
    return float((bins * deg).sum()) / total, float(((bins + 1).log() * deg).sum()) / total


class DegreeScalerAggregation(torch.nn.Module):
    """torch_geometric.nn.aggr.DegreeScalerAggregation(aggr, scaler, deg, train_norm=False): the statistics `aggr` (a name
    or a list of 'sum', 'mean', 'min', 'max', 'var', 'std') of the rows that share an index, each multiplied by every
    scaler of `scaler` ('identity', 'amplification' log(d+1) / avg_log, 'attenuation' avg_log / log(d+1), 'linear'
    d / avg_lin, 'inverse_linear' avg_lin / d, d the in-degree clamped to at least 1).  deg is the in-degree histogram of
    the training set; avg_deg_lin and avg_deg_log come from it and are buffers, or parameters with train_norm=True.

    forward(x, index=None, ptr=None, dim_size=None): x [E, F] per-entry rows, F <= 256; `ptr` (it wins) says the rows
    are grouped already, else the int64 `index` is grouped once (one host sync) and the kernel gathers through the
    grouping permutation, so no grouped copy of x is made.  The result is [n, S*A*F], scaler-major, the statistics in
    request order inside each scaler.

    PyG is not installed next to this package: the names (avg_deg_lin, avg_deg_log) follow PyG's published source and are
    **unpinned**."""

    def __init__(self, aggr: Union[str, List[str]], scaler: Union[str, List[str]], deg: torch.Tensor,
                 train_norm: bool = False):
        super().__init__()
        self.aggr = [aggr] if isinstance(aggr, str) else list(aggr)
        self.scaler = [scaler] if isinstance(scaler, str) else list(scaler)
        _native.multi_aggr_code(self.aggr)
        for s in self.scaler:
            if s not in SCALERS:
                raise ValueError(f"DegreeScalerAggregation: unknown scaler {s!r}, supported {list(SCALERS)}")
        if not self.scaler:
            raise ValueError("DegreeScalerAggregation: at least one scaler")
        self.init_avg_deg_lin, self.init_avg_deg_log = _avg_degrees(deg)
        self.train_norm = bool(train_norm)
        if train_norm:
            self.avg_deg_lin = torch.nn.Parameter(torch.zeros(1))
            self.avg_deg_log = torch.nn.Parameter(torch.zeros(1))
        else:
            self.register_buffer("avg_deg_lin", torch.zeros(1))
            self.register_buffer("avg_deg_log", torch.zeros(1))
        self.reset_parameters()

    def reset_parameters(self) -> None:
        with torch.no_grad():
            self.avg_deg_lin.fill_(self.init_avg_deg_lin)
            self.avg_deg_log.fill_(self.init_avg_deg_log)

    def factors(self, count: torch.Tensor, dtype: torch.dtype = torch.float32) -> torch.Tensor:
        """[n, S]: the scalers' factors for rows of `count` entries."""
        d = count.to(dtype).clamp(min=1)
        cols = []
        for s in self.scaler:
            if s == "identity":
                cols.append(torch.ones_like(d))
            elif s == "amplification":
                cols.append(torch.log(d + 1) / self.avg_deg_log)
            elif s == "attenuation":
                cols.append(self.avg_deg_log / torch.log(d + 1))
            elif s == "linear":
                cols.append(d / self.avg_deg_lin)
            else:
                cols.append(self.avg_deg_lin / d)
        return torch.stack(cols, dim=1)

    def forward(self, x: torch.Tensor, index: Optional[torch.Tensor] = None, ptr: Optional[torch.Tensor] = None,
                dim_size: Optional[int] = None) -> torch.Tensor:
        from .scatter import _csr_rowptr, _group_rows
        if x.dim() != 2:
            raise NotImplementedError(f"DegreeScalerAggregation: x must be [E, F], got {tuple(x.shape)}")
        E, F = x.shape
        if ptr is not None:
            n, rowptr, perm = ptr.numel() - 1, _csr_rowptr(ptr, E), None
        elif index is not None:
            n, rowptr, perm = _group_rows(index, E, F, dim_size)
        else:
            raise ValueError("DegreeScalerAggregation: the degree scalers need `index` or `ptr`")
        out, count = _aggregate_rows(x, rowptr, perm, n, self.aggr)          # [n, 1, A, F]
        fac = self.factors(count, out.dtype)                                  # [n, S]
        return (out * fac.view(n, -1, 1, 1)).reshape(n, -1)

    def __repr__(self) -> str:
        return f"{self.__class__.__name__}(aggr={self.aggr}, scaler={self.scaler}, train_norm={self.train_norm})"


_ACTS = {"relu": torch.nn.ReLU, "elu": torch.nn.ELU, "leaky_relu": torch.nn.LeakyReLU, "tanh": torch.nn.Tanh,
         "sigmoid": torch.nn.Sigmoid, "gelu": torch.nn.GELU, "silu": torch.nn.SiLU}


def _activation(act, act_kwargs) -> torch.nn.Module:
    if isinstance(act, torch.nn.Module):
        return act
    if callable(act) and not isinstance(act, str):
        return act(**(act_kwargs or {}))
    if act not in _ACTS:
        raise ValueError(f"PNAConv: unknown activation {act!r}, supported {sorted(_ACTS)} or a module")
    return _ACTS[act](**(act_kwargs or {}))


class PNAConv(torch.nn.Module):
    """torch_geometric.nn.PNAConv(in_channels, out_channels, aggregators, scalers, deg, edge_dim=None, towers=1,
    pre_layers=1, post_layers=1, divide_input=False, act='relu', act_kwargs=None, train_norm=False), flow
    source_to_target:

        m_ij   = pre_nn_t([x_i | x_j])                                  per tower t, over F_in channels
        agg_i  = [scaler(deg_i) * aggregator_j(m_ij)]                   every scaler times every aggregator
        out_i  = lin(cat_t post_nn_t([x_i | agg_i]))

    F_in = in_channels / towers with divide_input (each tower sees its slice of x), else in_channels (every tower sees
    all of x).  A node without an incoming edge aggregates zeros.  With pre_layers == 1 in fp32 the message is linear
    and the layer runs fused: A = x W_i^T + b and B = x W_j^T as one dense product each, multi_aggregate(B) over the
    graph, and A_i added to mean / min / max (count_i A_i to sum) -- no per-edge tensor, forward or backward; this needs
    towers * F_in <= 256.  Everything else (pre_layers > 1, autocast, or DMET_PNA=0 in the environment) forms the
    per-edge messages with torch indexing over the grouped edge list and aggregates them with DegreeScalerAggregation.
    edge_dim is refused with a ValueError.

    forward(x, edge_index): edge_index a GraphFuture, a NeighborTable (knn_table; a counted radius table is taken as its
    edge list), the int64 [2, E] tensor of knn_graph (its table is found again) or any other int64 [2, E] tensor
    (grouped by target, range-checked).

    PyG is not installed next to this package: the parameter names and shapes (pre_nns, post_nns, lin,
    aggr_module.avg_deg_lin / avg_deg_log) follow PyG's published source and are **unpinned** -- no PyG checkpoint has
    been loaded against them."""

    def __init__(self, in_channels: int, out_channels: int, aggregators: List[str], scalers: List[str], deg: torch.Tensor,
                 edge_dim: Optional[int] = None, towers: int = 1, pre_layers: int = 1, post_layers: int = 1,
                 divide_input: bool = False, act="relu", act_kwargs=None, train_norm: bool = False):
        super().__init__()
        if edge_dim is not None:
            raise ValueError("PNAConv: edge features (edge_dim) are not supported")
        if not isinstance(towers, int) or towers < 1:
            raise ValueError(f"PNAConv: towers={towers!r} must be a positive int")
        if divide_input and in_channels % towers:
            raise ValueError(f"PNAConv: divide_input needs in_channels={in_channels} divisible by towers={towers}")
        if out_channels % towers:
            raise ValueError(f"PNAConv: out_channels={out_channels} must be divisible by towers={towers}")
        if pre_layers < 1 or post_layers < 1:
            raise ValueError("PNAConv: pre_layers and post_layers must be at least 1")
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.aggregators = list(aggregators)
        self.scalers = list(scalers)
        self.edge_dim = None
        self.towers = towers
        self.pre_layers = pre_layers
        self.divide_input = bool(divide_input)
        self.F_in = in_channels // towers if divide_input else in_channels
        self.F_out = out_channels // towers
        self.aggr_module = DegreeScalerAggregation(self.aggregators, self.scalers, deg, train_norm)
        self.pre_nns = torch.nn.ModuleList()
        self.post_nns = torch.nn.ModuleList()
        width = (len(self.aggregators) * len(self.scalers) + 1) * self.F_in
        for _ in range(towers):
            mods = [torch.nn.Linear(2 * self.F_in, self.F_in)]
            for _ in range(pre_layers - 1):
                mods += [_activation(act, act_kwargs), torch.nn.Linear(self.F_in, self.F_in)]
            self.pre_nns.append(torch.nn.Sequential(*mods))
            mods = [torch.nn.Linear(width, self.F_out)]
            for _ in range(post_layers - 1):
                mods += [_activation(act, act_kwargs), torch.nn.Linear(self.F_out, self.F_out)]
            self.post_nns.append(torch.nn.Sequential(*mods))
        self.lin = torch.nn.Linear(out_channels, out_channels)

    def reset_parameters(self) -> None:
        for nn in list(self.pre_nns) + list(self.post_nns):
            for layer in nn:
                if hasattr(layer, "reset_parameters"):
                    layer.reset_parameters()
        self.lin.reset_parameters()
        self.aggr_module.reset_parameters()

    def route(self, x: torch.Tensor) -> str:
        """'fused' (the linear message split over multi_aggregate) or 'generic' (per-edge messages)."""
        if self.pre_layers == 1 and x.dtype == torch.float32 and not torch.is_autocast_enabled() \
                and os.environ.get("DMET_PNA", "1") != "0":
            return "fused"
        return "generic"

    def _graph(self, edge_index, num_nodes: int):
        if isinstance(edge_index, GraphFuture):
            edge_index = edge_index.peek() if isinstance(edge_index.peek(), NeighborTable) else edge_index.result()
        if isinstance(edge_index, NeighborTable):
            if edge_index.num_nodes != num_nodes:
                raise ValueError(f"PNAConv: the table has {edge_index.num_nodes} rows, x has {num_nodes}")
            return edge_index.edge_list() if edge_index.cnt is not None else edge_index
        if not torch.is_tensor(edge_index):
            raise TypeError(f"PNAConv: edge_index must be a NeighborTable, a GraphFuture or an int64 [2, E] tensor, got "
                            f"{type(edge_index).__name__}")
        hit = lookup_graph(edge_index)
        if hit is not None and hit[1] == "source_to_target" and hit[0].num_nodes == num_nodes and hit[0].cnt is None:
            return hit[0]
        return edge_list_from_edge_index(edge_index, num_nodes, "source_to_target")

    def _fused(self, xt: torch.Tensor, graph) -> torch.Tensor:
        """[N, T, S*A*F_in] from the towers' inputs xt [N, T, F_in] (divide_input) or [N, 1, F_in]."""
        T, Fi = self.towers, self.F_in
        N = xt.shape[0]
        W = torch.stack([nn[0].weight for nn in self.pre_nns])        # [T, F_in, 2 F_in]
        b = torch.stack([nn[0].bias for nn in self.pre_nns])          # [T, F_in]
        if self.divide_input:
            a_rows = torch.einsum("ntf,tgf->ntg", xt, W[:, :, :Fi]) + b
            b_rows = torch.einsum("ntf,tgf->ntg", xt, W[:, :, Fi:])
        else:       # every tower reads all of x: the towers' weights side by side, one product
            a_rows = (xt[:, 0] @ W[:, :, :Fi].reshape(T * Fi, Fi).t() + b.reshape(-1)).view(N, T, Fi)
            b_rows = (xt[:, 0] @ W[:, :, Fi:].reshape(T * Fi, Fi).t()).view(N, T, Fi)
        out, count = _MultiAggregate.apply(b_rows.reshape(N, T * Fi), graph, tuple(self.aggregators), T)    # [N, T, A, F_in]
        has = (count > 0).to(out.dtype)
        per = {"sum": count.to(out.dtype), "mean": has, "min": has, "max": has, "var": torch.zeros_like(has),
               "std": torch.zeros_like(has)}
        shift = torch.stack([per[a] for a in self.aggregators], dim=1)       # [N, A]: how often A_i enters each statistic
        agg = out + shift.view(N, 1, -1, 1) * a_rows.unsqueeze(2)
        fac = self.aggr_module.factors(count, out.dtype)                       # [N, S]
        return (agg.unsqueeze(2) * fac.view(N, 1, -1, 1, 1)).reshape(N, T, -1)

    def _generic(self, xt: torch.Tensor, graph) -> torch.Tensor:
        T, Fi = self.towers, self.F_in
        N = xt.shape[0]
        edges = graph if isinstance(graph, EdgeList) else graph.edge_list()
        if xt.shape[1] != T:
            xt = xt.expand(N, T, Fi)
        h = torch.cat([xt[edges.tgt.long()], xt[edges.src.long()]], dim=-1)          # [E, T, 2 F_in]
        msg = torch.stack([nn(h[:, t]) for t, nn in enumerate(self.pre_nns)], dim=1)     # [E, T, F_in]
        out = self.aggr_module(msg.reshape(-1, T * Fi), ptr=edges.rowptr)               # [N, S*A*(T F_in)]
        S, A = len(self.scalers), len(self.aggregators)
        return out.view(N, S, A, T, Fi).permute(0, 3, 1, 2, 4).reshape(N, T, S * A * Fi)

    def forward(self, x: torch.Tensor, edge_index) -> torch.Tensor:
        if not torch.is_tensor(x) or x.dim() != 2 or x.shape[1] != self.in_channels:
            raise ValueError(f"PNAConv: x must be [N, {self.in_channels}], got "
                             f"{tuple(x.shape) if torch.is_tensor(x) else type(x).__name__}")
        N, T = x.shape[0], self.towers
        graph = self._graph(edge_index, N)
        xt = x.view(N, T, self.F_in) if self.divide_input else x.view(N, 1, self.F_in)
        if self.route(x) == "fused":
            if isinstance(graph, NeighborTable):
                graph.join()
            agg = self._fused(xt, graph)
        else:
            agg = self._generic(xt, graph)
        xt = xt if self.divide_input else xt.expand(N, T, self.F_in)
        out = torch.cat([xt.to(agg.dtype), agg], dim=-1)
        out = torch.cat([nn(out[:, t]) for t, nn in enumerate(self.post_nns)], dim=1)
        return self.lin(out)

    def __repr__(self) -> str:
        return (f"{self.__class__.__name__}({self.in_channels}, {self.out_channels}, towers={self.towers}, "
                f"edge_dim={self.edge_dim})")

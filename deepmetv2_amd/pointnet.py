"""PointNet set abstraction (torch_geometric.nn.PointNetConv, alias PointConv): for every target i the maximum over its
neighbours j of local_nn([x_j || pos_j - pos_i]), then global_nn.

For local_nn = Sequential(Linear, ReLU | ELU, Linear[, the same activation]) and aggr 'max' the message and the maximum
are csrc/pointnet.hip: the first Linear splits per node, the second runs per entry on the fp32 matrix cores, and neither
the [E, F + D] features nor the [E, H] activations are ever written -- over a table there is no edge list and no host
sync either.  Every other local_nn or aggr takes the generic route: torch indexing over the edge list, local_nn over E
rows, the package's segment reductions.
"""
from __future__ import annotations

import os
from typing import Optional, Tuple, Union

import torch
from torch.autograd.function import once_differentiable

from . import _native
from .conv import _reset
from .graph import BipartiteTable, EdgeList, GraphFuture, NeighborTable, edge_list_from_edge_index
from .gravnet import _upcast
from .scatter import _SegmentMaxRows, _SegmentSumRows

Graph = Union[NeighborTable, BipartiteTable, EdgeList]
_ACTS = {torch.nn.ReLU: "relu", torch.nn.ELU: "elu"}


def _graph_args(graph):
    """(idx, rowptr, tgt, cnt) as the kernels take them: a table's nbr (and cnt), or a list's src, rowptr and tgt."""
    if isinstance(graph, EdgeList):
        return graph.src, graph.rowptr, graph.tgt, None
    return graph.nbr, None, None, graph.cnt


def _graph_sizes(graph) -> Tuple[int, int, Optional[int]]:
    """(targets, sources, table width or None)."""
    if isinstance(graph, NeighborTable):
        return graph.num_nodes, graph.num_nodes, graph.k
    if isinstance(graph, BipartiteTable):
        return graph.num_queries, graph.num_candidates, graph.k
    if isinstance(graph, EdgeList):
        return graph.num_nodes, graph.num_src, None
    raise TypeError("pointnet_aggregate: graph must be a NeighborTable, a BipartiteTable or an EdgeList, got "
                    f"{type(graph).__name__}")


class _PointNetAggregate(torch.autograd.Function):
    """out[i] = max over the entries of row i of act2?(W2 act(W1 [x_j || pos_j - pos_i] + b1) + b2), differentiable in x,
    both position sets and the four parameters.  `once_differentiable`; saves the node-level A, B (and S), out and the
    winners, nothing per edge."""

    @staticmethod
    def forward(ctx, x_src, pos_src, pos_dst, W1, b1, W2, b2, graph, act, act2, self_loop, one_set):
        xf = None if x_src is None else _upcast(x_src, "x")
        pf = _upcast(pos_src, "pos")
        qf = pf if one_set else _upcast(pos_dst, "pos")
        idx, rowptr, _tgt, cnt = _graph_args(graph)
        out, win, state = _native._pointnet_fwd(xf, pf, qf, idx, rowptr, cnt, W1, b1, W2, b2, act, act2, self_loop)
        ctx.save_for_backward(xf, pf, qf, W1, W2, out, win, *[t for t in state if t is not None])
        ctx.graph, ctx.act, ctx.act2, ctx.self_loop, ctx.one_set = graph, act, act2, self_loop, one_set
        ctx.has_b = (b1 is not None, b2 is not None)
        ctx.dtypes = (None if x_src is None else x_src.dtype, pos_src.dtype, pos_dst.dtype)
        ctx.mark_non_differentiable(win)
        return out, win

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out, _g_win):
        xf, pf, qf, W1, W2, out, win, a, b, *rest = ctx.saved_tensors
        s = rest[0] if rest else None
        graph = ctx.graph
        idx, rowptr, tgt, cnt = _graph_args(graph)
        rev_ptr, rev_pos = graph.by_source() if isinstance(graph, EdgeList) else graph.reverse()
        need = ctx.needs_input_grad
        want = (xf is not None and need[0], need[1], need[2], need[3], ctx.has_b[0] and need[4], need[5],
                ctx.has_b[1] and need[6])
        g_x, g_ps, g_pd, g_W1, g_b1, g_W2, g_b2 = _native._pointnet_bwd(
            g_out.float(), out, win, (a, b, s), xf, pf, qf, idx, rev_ptr, rev_pos, rowptr, tgt, cnt, W1, W2, ctx.act,
            ctx.act2, ctx.self_loop, want)
        dx, dp, dq = ctx.dtypes
        # one position tensor on both sides (one node set): autograd adds its two gradients
        return (None if g_x is None else g_x.to(dx), None if g_ps is None else g_ps.to(dp),
                None if g_pd is None else g_pd.to(dq), g_W1, g_b1, g_W2, g_b2, None, None, None, None, None)


def _as_fused_local_nn(local_nn):
    """(lin1, lin2, act name, act2) when local_nn is Sequential(Linear, ReLU | ELU(alpha 1), Linear[, the same
    activation]); None otherwise."""
    if not isinstance(local_nn, torch.nn.Sequential) or len(local_nn) not in (3, 4):
        return None
    lin1, a1, lin2 = local_nn[0], local_nn[1], local_nn[2]
    if type(lin1) is not torch.nn.Linear or type(lin2) is not torch.nn.Linear or type(a1) not in _ACTS:
        return None
    if isinstance(a1, torch.nn.ELU) and a1.alpha != 1.0:
        return None
    act2 = len(local_nn) == 4
    if act2:
        a2 = local_nn[3]
        if type(a2) is not type(a1) or (isinstance(a2, torch.nn.ELU) and a2.alpha != 1.0):
            return None
    if lin2.in_features != lin1.out_features:
        return None
    return lin1, lin2, _ACTS[type(a1)], act2


def pointnet_aggregate(x_src: Optional[torch.Tensor], pos_src: torch.Tensor, pos_dst: torch.Tensor, graph: Graph,
                       lin1: torch.nn.Linear, lin2: torch.nn.Linear, act: str = "relu", act2: bool = False,
                       self_loops: bool = False, return_winners: bool = False):
    """out[Nt, H2]: for every row i of `graph` the channel-wise maximum over its entries j of
    act2?(lin2(act(lin1([x_src[j] || pos_src[j] - pos_dst[i]])))), act in ('relu', 'elu'); a row without an entry gives
    zeros.  The fused kernels of csrc/pointnet.hip, always (there is no other route here): fp32 parameters, x_src [Ns, F]
    or None (F = 0), F <= 128, 1 <= D <= 8 position coordinates, lin1.out_features <= 128, lin2.out_features in (16, 32,
    64, 128); anything else is a ValueError.

    graph: a NeighborTable (one node set: pos_dst must be pos_src), a BipartiteTable (pos_dst its queries, x_src and
    pos_src its candidates) or an EdgeList; a counted radius table is read up to its counts and is differentiable
    through its EdgeList only (pass table.edge_list()).  self_loops=True (one node set only): entries j == i are skipped
    and one entry i -> i is taken after the row's own -- upstream's remove_self_loops + add_self_loops.  Differentiable
    in x_src, pos_src, pos_dst and the parameters; bf16 inputs (fp16 under fp16 autocast) are upcast exactly.  Over a
    -1-padded table: no edge list and no host sync, forward or backward.

    Non-finite values: the maximum runs over the messages that are numbers (+-inf included), wherever an entry stands in
    its row; a NaN message never wins and never blocks, and a channel whose messages are all NaN is NaN with win -1 --
    upstream's amax propagates the NaN instead.  ReLU (v > 0 ? v : 0) turns a NaN pre-activation into 0; ELU carries it on.
    A non-finite input of source j changes the rows that list j and nothing else, forward and backward.

    return_winners=True: (out, win), win[Nt, H2] int32 the winning table slot or grouped list position, -2 for the
    added self entry, -1 for a row without an entry."""
    Nt, Ns, width = _graph_sizes(graph)
    if act not in _native.POINTNET_ACT:
        raise ValueError(f"pointnet_aggregate: act must be 'relu' or 'elu', got {act!r}")
    if not isinstance(lin1, torch.nn.Linear) or not isinstance(lin2, torch.nn.Linear):
        raise TypeError("pointnet_aggregate: lin1 and lin2 must be torch.nn.Linear modules")
    one_set = pos_dst is pos_src
    if isinstance(graph, NeighborTable) and not one_set:
        raise ValueError("pointnet_aggregate: a NeighborTable has one node set: pass the same tensor as pos_src and pos_dst")
    if self_loops and not one_set:
        raise ValueError("pointnet_aggregate: self_loops=True needs one node set (pos_dst is pos_src); two sets have "
                         "separate index spaces")
    for p in (lin1.weight, lin1.bias, lin2.weight, lin2.bias):
        if p is not None and p.dtype != torch.float32:
            raise TypeError(f"pointnet_aggregate: the parameters must be float32, got {p.dtype}")
    _native.pointnet_check_shapes(x_src, pos_src, pos_dst, lin1.weight, lin1.bias, lin2.weight, lin2.bias, act, Nt, Ns,
                                  width, bool(self_loops))
    needs_grad = torch.is_grad_enabled() and any(
        t is not None and t.requires_grad for t in (x_src, pos_src, pos_dst, lin1.weight, lin1.bias, lin2.weight, lin2.bias))
    if not isinstance(graph, EdgeList) and graph.cnt is not None and needs_grad:
        raise ValueError("pointnet_aggregate: a counted radius table is differentiable through its edge list: pass "
                         "table.edge_list()")
    if isinstance(graph, NeighborTable):
        graph.join()
    out, win = _PointNetAggregate.apply(x_src, pos_src, pos_dst, lin1.weight, lin1.bias, lin2.weight, lin2.bias, graph, act,
                                        bool(act2), bool(self_loops), one_set)
    return (out, win) if return_winners else out


def _with_self_loops(edges: EdgeList) -> EdgeList:
    """remove_self_loops + add_self_loops on a one-set list, grouped again: a row's own entries keep their order and the
    added entry i -> i comes last.  Generic route only (boolean indexing reads the edge count)."""
    N = edges.num_nodes
    dev = edges.src.device
    keep = edges.src != edges.tgt
    ids = torch.arange(N, dtype=torch.int32, device=dev)
    tgt = torch.cat([edges.tgt[keep], ids])
    src = torch.cat([edges.src[keep], ids])
    order = torch.sort(tgt.long(), stable=True).indices
    deg = torch.bincount(tgt.long(), minlength=N)
    rowptr = torch.zeros(N + 1, dtype=torch.int32, device=dev)
    rowptr[1:] = torch.cumsum(deg, 0).to(torch.int32)
    return EdgeList(src[order].contiguous(), tgt[order].contiguous(), rowptr, N)


class PointNetConv(torch.nn.Module):
    """torch_geometric.nn.PointNetConv(local_nn=None, global_nn=None, add_self_loops=True, **kwargs):

        out_i = global_nn( max_{j in N(i) + {i}} local_nn([x_j || pos_j - pos_i]) )

    kwargs: aggr ('max' by default; 'add' / 'sum', 'mean'), flow ('source_to_target' by default).  Attribute names
    local_nn / global_nn as upstream, so state_dict keys match.

    forward(x, pos, edge_index): x a tensor, None or an (x_src, x_dst) pair (x_dst is not used by the message, as
    upstream); pos a tensor or a (pos_src, pos_dst) pair; edge_index an int64 [2, E] tensor, a NeighborTable (one node
    set), a BipartiteTable (a pos pair: candidates = sources, queries = targets) or a GraphFuture.  Two different node
    sets with add_self_loops=True raise a ValueError: upstream matches ids across two index spaces there, which means
    nothing, and its own PointNet++ example passes add_self_loops=False.

    The fused route (csrc/pointnet.hip) takes the call when local_nn is Sequential(Linear, ReLU | ELU, Linear[, the same
    activation]), parameters and inputs are fp32 on the GPU, the widths are supported (pointnet_aggregate), aggr is 'max',
    no autocast is on and ``DMET_POINTNET`` is not "0".  Over a -1-padded table it reads no edge list and never
    synchronises, forward or backward; a counted radius table runs the table form when no gradient is needed and its
    edge list (one host read) otherwise.  Everything else -- a deeper or BatchNorm-carrying local_nn, aggr add / mean,
    local_nn=None, autocast -- runs the generic route: [x_j || pos_j - pos_i] gathered with torch indexing over the edge
    list, local_nn over E rows, then the package's segment max / sum.

    PyG is not installed next to this package: names and semantics follow PyG's published source and are **unpinned**."""

    def __init__(self, local_nn=None, global_nn=None, add_self_loops: bool = True, **kwargs):
        super().__init__()
        aggr = kwargs.pop("aggr", "max")
        flow = kwargs.pop("flow", "source_to_target")
        if kwargs:
            raise TypeError(f"PointNetConv: unexpected keyword arguments {sorted(kwargs)}")
        if aggr not in ("max", "add", "sum", "mean"):
            raise ValueError(f"PointNetConv: aggr must be 'max', 'add', 'sum' or 'mean', got {aggr!r}")
        if flow not in ("source_to_target", "target_to_source"):
            raise ValueError(f"PointNetConv: flow must be 'source_to_target' or 'target_to_source', got {flow!r}")
        self.local_nn = local_nn
        self.global_nn = global_nn
        self.add_self_loops = add_self_loops
        self.aggr = aggr
        self.flow = flow
        self.reset_parameters()

    def reset_parameters(self) -> None:
        _reset(self.local_nn)
        _reset(self.global_nn)

    def _fused(self, x_src, pos_src, pos_dst):
        """(lin1, lin2, act, act2) when the fused route takes the call, else None."""
        if os.environ.get("DMET_POINTNET", "1") == "0" or self.aggr != "max" or torch.is_autocast_enabled():
            return None
        spec = _as_fused_local_nn(self.local_nn)
        if spec is None:
            return None
        lin1, lin2 = spec[0], spec[1]
        tensors = [pos_src, pos_dst, lin1.weight, lin2.weight] + [t for t in (x_src, lin1.bias, lin2.bias) if t is not None]
        if any(t.dtype != torch.float32 or not t.is_cuda for t in tensors):
            return None
        F = 0 if x_src is None else x_src.shape[1]
        if lin1.in_features != F + pos_src.shape[1]:
            return None
        if not _native.pointnet_widths_supported(F, pos_src.shape[1], lin1.out_features, lin2.out_features):
            return None
        return spec

    def forward(self, x, pos, edge_index) -> torch.Tensor:
        x_src = x[0] if isinstance(x, (tuple, list)) else x
        if isinstance(pos, (tuple, list)):
            if len(pos) != 2:
                raise ValueError("PointNetConv: pos must be a tensor or a (pos_src, pos_dst) pair")
            pos_src, pos_dst = pos
        else:
            pos_src = pos_dst = pos
        one_set = pos_dst is pos_src
        if pos_src.dim() != 2 or pos_dst.dim() != 2 or pos_src.shape[1] != pos_dst.shape[1]:
            raise ValueError(f"PointNetConv: pos must be [N, D], got {tuple(pos_src.shape)} and {tuple(pos_dst.shape)}")
        if x_src is not None and (x_src.dim() != 2 or x_src.shape[0] != pos_src.shape[0]):
            raise ValueError(f"PointNetConv: x must be [{pos_src.shape[0]}, F] beside pos, got {tuple(x_src.shape)}")
        if self.add_self_loops and not one_set:
            raise ValueError("PointNetConv: two node sets have separate index spaces, so self loops mean nothing there; "
                             "construct the layer with add_self_loops=False (as PyG's PointNet++ example does)")
        if isinstance(edge_index, GraphFuture):
            edge_index = edge_index.result()
        Ns, Nt = pos_src.shape[0], pos_dst.shape[0]
        if isinstance(edge_index, NeighborTable):
            if not one_set:
                raise ValueError("PointNetConv: a NeighborTable has one node set; a (pos_src, pos_dst) pair goes with a "
                                 "BipartiteTable or an edge_index tensor")
            if edge_index.num_nodes != Nt:
                raise ValueError(f"PointNetConv: the table has {edge_index.num_nodes} rows, pos has {Nt}")
            graph = edge_index.join()
        elif isinstance(edge_index, BipartiteTable):
            if one_set:
                raise ValueError("PointNetConv: a BipartiteTable needs a (pos_src, pos_dst) pair")
            if (edge_index.num_candidates, edge_index.num_queries) != (Ns, Nt):
                raise ValueError(f"PointNetConv: the table connects {edge_index.num_queries} queries to "
                                 f"{edge_index.num_candidates} candidates, pos_dst / pos_src have {Nt} / {Ns} rows")
            graph = edge_index
        elif torch.is_tensor(edge_index):
            graph = edge_list_from_edge_index(edge_index, Nt, self.flow, num_src=None if one_set else Ns)
        else:
            raise TypeError("PointNetConv: edge_index must be an int64 [2, E] tensor, a NeighborTable, a BipartiteTable or "
                            f"a GraphFuture, got {type(edge_index).__name__}")
        spec = self._fused(x_src, pos_src, pos_dst)
        if spec is not None:
            lin1, lin2, act, act2 = spec
            if not isinstance(graph, EdgeList) and graph.cnt is not None and torch.is_grad_enabled() and any(
                    t is not None and t.requires_grad
                    for t in (x_src, pos_src, pos_dst, lin1.weight, lin1.bias, lin2.weight, lin2.bias)):
                graph = graph.edge_list()       # a counted table's by-source index: through its list (one host read)
            out = pointnet_aggregate(x_src, pos_src, pos_dst, graph, lin1, lin2, act, act2, self.add_self_loops)
        else:
            out = self._forward_generic(x_src, pos_src, pos_dst, graph)
        if self.global_nn is not None:
            out = self.global_nn(out)
        return out

    def _forward_generic(self, x_src, pos_src, pos_dst, graph) -> torch.Tensor:
        edges = graph if isinstance(graph, EdgeList) else graph.edge_list()
        if self.add_self_loops:
            edges = _with_self_loops(edges)
        Nt = pos_dst.shape[0]
        src, tgt = edges.src.long(), edges.tgt.long()
        msg = pos_src[src] - pos_dst[tgt]
        if x_src is not None:
            msg = torch.cat([x_src[src], msg.to(x_src.dtype)], dim=1)
        if self.local_nn is not None:
            msg = self.local_nn(msg)
        if msg.dim() != 2 or msg.shape[0] != edges.num_edges:
            raise ValueError("PointNetConv: local_nn must map [E, F + D] -> [E, F_out]")
        if edges.num_edges == 0:
            return msg.new_zeros((Nt, msg.shape[1]), dtype=torch.float32)
        msg = msg.float().contiguous()      # local_nn under autocast: exact upcast, the segment reductions are fp32
        if self.aggr == "max":
            out, _arg = _SegmentMaxRows.apply(msg, edges.rowptr, Nt)
            return out
        out = _SegmentSumRows.apply(msg, edges.rowptr, Nt)
        if self.aggr == "mean":
            deg = (edges.rowptr[1:] - edges.rowptr[:-1]).clamp(min=1).to(out.dtype).view(-1, 1)
            out = out / deg
        return out

    def __repr__(self) -> str:
        return f"{self.__class__.__name__}(local_nn={self.local_nn}, global_nn={self.global_nn})"


PointConv = PointNetConv

"""What the softmax aggregations over a graph share -- attention.py (attention_aggregate, TransformerConv) and gat.py
(gat_aggregate, gat_v1_aggregate, GATConv, GATv2Conv), as their kernels share csrc/row_softmax.h: how a graph object
becomes kernel arguments, the graph forms an aggregate takes, and a layer's option checks, its x split, what it makes of
`edge_index` and how it hands the attention weights back.
"""
from __future__ import annotations

import torch

from . import _native
from .graph import BipartiteTable, EdgeList, GraphFuture, NeighborTable, edge_list_from_edge_index, lookup_graph


def graph_args(graph):
    """(idx, rowptr, tgt) as the kernels take them: a table's nbr, or a list's src, rowptr and tgt."""
    if isinstance(graph, EdgeList):
        return graph.src, graph.rowptr, graph.tgt
    return graph.nbr, None, None


def by_source_index(graph):
    """(rev_ptr, rev_pos) of the backward's by-source pass."""
    return graph.by_source() if isinstance(graph, EdgeList) else graph.reverse()


def check_graph(who: str, graph, check_shapes, self_loops: bool = False) -> None:
    """The graph forms `who` aggregates over: check_shapes(num_targets, num_sources, table width or None, self_loops)
    for a -1-padded NeighborTable (joined here if it is still being built), a -1-padded BipartiteTable (no self loops)
    or an EdgeList; anything else is refused."""
    if isinstance(graph, NeighborTable):
        if graph.cnt is not None:
            raise ValueError(f"{who} needs a -1-padded table (knn_table), not a counted radius table")
        check_shapes(graph.num_nodes, graph.num_nodes, graph.k, self_loops)
        graph.join()
    elif isinstance(graph, BipartiteTable):
        if graph.cnt is not None:
            raise ValueError(f"{who} needs a -1-padded table (knn_xy_table), not a counted radius table")
        if self_loops:
            raise ValueError(f"{who}: a BipartiteTable has two node sets and no self loops; pass self_loops=False")
        check_shapes(graph.num_queries, graph.num_candidates, graph.k, False)
    elif isinstance(graph, EdgeList):
        check_shapes(graph.num_nodes, graph.num_src, None, self_loops)
    else:
        raise TypeError(f"{who}: graph must be a NeighborTable, a BipartiteTable or an EdgeList, got "
                        f"{type(graph).__name__}")


def shape_alpha(alpha: torch.Tensor, graph, num_targets: int, heads: int) -> torch.Tensor:
    """The kernel's alpha [positions, H] as the caller gets it: [Nt, k, H] for a table, [E, H] in the list's grouped
    order for an EdgeList."""
    return alpha if isinstance(graph, EdgeList) else alpha.view(num_targets, graph.k, heads)


class SoftmaxConv(torch.nn.Module):
    """The layer plumbing of TransformerConv, GATConv and GATv2Conv; messages carry the class's own name."""

    def _check_options(self, heads, out_channels, dropout, edge_dim, size_prefix: str) -> None:
        """The constructor's refusals; size_prefix leads the heads / out_channels messages."""
        who = self.__class__.__name__
        if dropout != 0.0:
            raise ValueError(f"{who}: dropout on the attention weights is not supported (no RNG kernel); use 0.0")
        if edge_dim is not None:
            raise ValueError(f"{who}: edge features (edge_dim) are not supported")
        for name, val, top in (("heads", heads, _native.ATTENTION_MAX_H),
                               ("out_channels", out_channels, _native.ATTENTION_MAX_C)):
            if not isinstance(val, int) or isinstance(val, bool) or not 1 <= val <= top:
                raise ValueError(f"{size_prefix}{name}={val!r}, supported 1..{top}")
        if heads * out_channels > _native.ATTENTION_MAX_HC:
            raise ValueError(f"{size_prefix}heads * out_channels = {heads * out_channels}, supported up to "
                             f"{_native.ATTENTION_MAX_HC}")

    def _split(self, x):
        """(x is a pair, x_src, x_dst) of forward's x: a tensor, or an (x_src, x_dst) pair."""
        who = self.__class__.__name__
        pair = isinstance(x, (tuple, list))
        if pair:
            if len(x) != 2:
                raise ValueError(f"{who}: x must be a tensor or an (x_src, x_dst) pair")
            x_src, x_dst = x
        else:
            x_src = x_dst = x
        if not torch.is_tensor(x_src) or not torch.is_tensor(x_dst):
            raise TypeError(f"{who}: x must be a tensor or an (x_src, x_dst) pair of tensors")
        if x_src.dim() != 2 or x_dst.dim() != 2:
            raise ValueError(f"{who}: x must be [N, F], got {tuple(x_src.shape)} and {tuple(x_dst.shape)}")
        return pair, x_src, x_dst

    def _resolve(self, edge_index, num_src: int, num_dst: int, pair: bool, want_alpha: bool):
        """(graph for the aggregate, how to hand alpha back: 'table', 'flat' or 'list')."""
        who = self.__class__.__name__
        if isinstance(edge_index, GraphFuture):
            edge_index = edge_index.peek() if isinstance(edge_index.peek(), NeighborTable) else edge_index.result()
        if isinstance(edge_index, (NeighborTable, BipartiteTable)):
            if isinstance(edge_index, NeighborTable) and pair:
                raise ValueError(f"{who}: an (x_src, x_dst) pair goes with a BipartiteTable or an edge_index tensor")
            if isinstance(edge_index, BipartiteTable) and not pair:
                raise ValueError(f"{who}: a BipartiteTable needs an (x_src, x_dst) pair")
            if edge_index.cnt is not None:       # a counted radius table: its valid slots as a list (one host read)
                return edge_index.edge_list(), "list"
            return edge_index, "table"
        if not torch.is_tensor(edge_index):
            raise TypeError(f"{who}: edge_index must be a graph object or an int64 [2, E] tensor, got "
                            f"{type(edge_index).__name__}")
        hit = None if pair else lookup_graph(edge_index)
        if hit is not None and hit[1] == "source_to_target" and hit[0].num_nodes == num_dst and hit[0].cnt is None:
            table = hit[0]
            # the tensor lists the table's slots in position order when it is sized Nt*k: alpha goes back flat
            if not want_alpha or edge_index.shape[1] == table.num_nodes * table.k:
                return table, "flat"
        return edge_list_from_edge_index(edge_index, num_dst, "source_to_target", num_src=num_src if pair else None), "list"

    def _with_alpha(self, out, edge_index, graph, how: str, alpha):
        """forward's result under return_attention_weights=True: (out, (what the caller passed, alpha in its order))."""
        if how == "table":
            return out, (edge_index.peek() if isinstance(edge_index, GraphFuture) else edge_index, alpha)
        if how == "flat":
            return out, (edge_index, alpha.reshape(-1, self.heads))
        if graph.perm is not None:       # back from the grouped order to the caller's; perm is a permutation of all rows
            alpha = torch.empty_like(alpha).index_copy_(0, graph.perm.long(), alpha)
        return out, (edge_index, alpha)

    def __repr__(self) -> str:
        return f"{self.__class__.__name__}({self.in_channels}, {self.out_channels}, heads={self.heads})"

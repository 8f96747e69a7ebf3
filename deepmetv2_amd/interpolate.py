"""knn_interpolate (torch_geometric.nn.unpool.knn_interpolate): features of a coarse point set brought back to a fine
one, every fine point taking the inverse-squared-distance weighted mean of its k nearest coarse points.

The graph and its distances come from this package's two-set kNN build (rules R1 / R2 of include/dmet.h, `period=`
included), the aggregation and its backward from csrc/interpolate.hip: one gather of an x row per edge, no [2, E] edge
index, no [E, F] messages, no float atomics, no host sync.
"""
from __future__ import annotations

from typing import Optional, Union

import torch
from torch.autograd.function import once_differentiable

from . import _native
from .cluster import knn_xy_table
from .graph import BipartiteTable, NeighborTable
from .gravnet import _upcast

MAX_FEATURES = _native.INTERPOLATE_MAX_F


class _InterpolateAggregate(torch.autograd.Function):
    """sum over the rows of a table of r_t x[j_t], r_t = w_t / sum_t w_t, w_t = 1 / max(dist_t, 1e-16); differentiable in x
    only (upstream forms the weights under no_grad).  `once_differentiable`."""

    @staticmethod
    def forward(ctx, x, table, num_sources: int):
        out, wsum = _native.interpolate_fwd(_upcast(x, "x"), table.nbr, table.dist)
        ctx.save_for_backward(wsum)
        ctx.table, ctx.num_sources, ctx.dtype = table, num_sources, x.dtype
        return out.to(x.dtype)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out):
        wsum, = ctx.saved_tensors
        table = ctx.table
        rev_ptr, rev_pos = table.reverse()
        g_x = _native.interpolate_bwd(g_out.float(), table.dist, wsum, rev_ptr, rev_pos, ctx.num_sources)
        return g_x.to(ctx.dtype), None, None


def interpolate_aggregate(x: torch.Tensor, table: Union[NeighborTable, BipartiteTable]) -> torch.Tensor:
    """[N_dst, F]: for every row i of `table`, sum over its valid slots j = table.nbr[i, t] of r_t x[j] with
    r_t = w_t / sum_t w_t and w_t = 1 / clamp(table.dist[i, t], min=1e-16), the table's own fp32 squared distances.  A
    slot is valid by its id (-1 or an id outside the sources is empty, whatever its distance); a row without a valid slot
    gives zeros.

    Non-finite values: the clamp keeps a NaN, as torch.clamp does, so a NaN distance in a valid slot makes its whole row
    NaN (a table of knn_table / knn_xy_table never holds one there; a hand-built table may); a non-finite x[j, f] shows
    in feature f of the rows that list j and nowhere else.

    BipartiteTable (knn_xy_table): x belongs to the candidates.  NeighborTable (knn_table): one node set.  Differentiable
    in x; the distances carry no gradient.  1 <= F <= 256 features, k <= 64; anything else is a ValueError.  bf16 input
    (fp16 under fp16 autocast) is upcast exactly and the result comes back in x's dtype.  Reads table.nbr, table.dist and
    table.reverse(): no edge list, no host sync."""
    if isinstance(table, NeighborTable):
        if table.cnt is not None:
            raise ValueError("interpolate_aggregate needs a -1-padded table (knn_table), not a counted radius table")
        if table.dist is None:
            raise ValueError("interpolate_aggregate needs the table's distances (table.dist of knn_table); this table has none")
        num_sources = table.num_nodes
    elif isinstance(table, BipartiteTable):
        if table.cnt is not None:
            raise ValueError("interpolate_aggregate needs a -1-padded table (knn_xy_table), not a counted radius table")
        if table.dist is None:
            raise ValueError("interpolate_aggregate needs the table's distances (table.dist of knn_xy_table); this table has "
                             "none")
        num_sources = table.num_candidates
    else:
        raise TypeError(f"interpolate_aggregate: table must be a NeighborTable or a BipartiteTable, got {type(table).__name__}")
    if x.dim() == 2 and x.shape[0] != num_sources:
        raise ValueError(f"interpolate_aggregate: the table indexes {num_sources} candidates, x has {x.shape[0]} rows")
    if isinstance(table, NeighborTable):
        table.join()
    _native.interpolate_check_shapes(x, table.nbr, table.dist)
    return _InterpolateAggregate.apply(x, table, num_sources)


def knn_interpolate(x: torch.Tensor, pos_x: torch.Tensor, pos_y: torch.Tensor, batch_x: Optional[torch.Tensor] = None,
                    batch_y: Optional[torch.Tensor] = None, k: int = 3, num_workers: int = 1,
                    batch_size: Optional[int] = None, period=None) -> torch.Tensor:
    """torch_geometric.nn.unpool.knn_interpolate: x [Nx, F] at the positions pos_x, interpolated to the positions pos_y
    ([Ny, F]): y_i = sum_j w_ij x_j / sum_j w_ij over the k nearest pos_x of pos_y[i] in the same event,
    w_ij = 1 / max(|pos_x[j] - pos_y[i]|^2, 1e-16).  It is interpolate_aggregate(x, knn_xy_table(pos_x, pos_y, k, batch_x,
    batch_y, batch_size, period)): the graph follows this package's kNN rules (R1 distance chain, R2 ties to the lower
    index), a fine point whose event has fewer than k coarse points averages those there are, one whose event has none
    gets zeros.  Differentiable in x only, as upstream.  num_workers is accepted and ignored, as in PyG; period: periodic
    coordinates, see knn_table.  With both batch vectors registered (register_batch) the call never synchronises."""
    if x.dim() == 2 and pos_x.dim() == 2 and x.shape[0] != pos_x.shape[0]:
        raise ValueError(f"knn_interpolate: x has {x.shape[0]} rows, pos_x has {pos_x.shape[0]}")
    if x.dim() != 2 or not 1 <= x.shape[1] <= MAX_FEATURES:
        raise ValueError(f"knn_interpolate: x must be [Nx, F] with F in 1..{MAX_FEATURES}, got {tuple(x.shape)}")
    return interpolate_aggregate(x, knn_xy_table(pos_x.detach(), pos_y.detach(), k, batch_x, batch_y, batch_size, period))

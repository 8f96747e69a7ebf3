"""GravNet (torch_geometric.nn.GravNetConv): kNN in a learned coordinate space, neighbour features weighted by
exp(-10 d^2), aggregated with mean and max.

The graph comes from this package's kNN build (rules R1 / R2 of include/dmet.h), the aggregation and its backward from
csrc/gravnet.hip: one gather of an h row per edge, no [E, P] messages, no edge list, no host sync.  The four Linears stay
torch modules, with PyG's attribute names, so a PyG checkpoint loads.
"""
from __future__ import annotations

from typing import Optional, Tuple, Union

import torch
from torch.autograd.function import once_differentiable

from . import _native
from .cluster import MAX_K, fp16_autocast, knn_table, knn_xy_table
from .graph import BipartiteTable, NeighborTable

MAX_SPACE = _native.GRAVNET_MAX_S
MAX_PROPAGATE = _native.GRAVNET_MAX_P


def _upcast(t: torch.Tensor, name: str) -> torch.Tensor:
    # 16-bit inputs from autocast upstream: an exact upcast (bf16 always; fp16 while fp16 autocast is on, like the kNN)
    if t.dtype == torch.bfloat16 or (t.dtype == torch.float16 and fp16_autocast()):
        return t.float()
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32 (or bfloat16, or float16 under fp16 autocast), got {t.dtype}")
    return t


class _GravNetAggregate(torch.autograd.Function):
    """[mean | max] over the rows of a neighbour table of exp(-10 |s_j - s_i|^2) h_j, differentiable in h and in both
    coordinate sets (the weights carry the gradient into the learned space).  `once_differentiable`."""

    @staticmethod
    def forward(ctx, h, s_src, s_tgt, table, one_set: bool):
        hf, ssf = _upcast(h, "h"), _upcast(s_src, "s")
        stf = ssf if one_set else _upcast(s_tgt, "s_dst")
        out, arg, cnt = _native.gravnet_fwd(hf, ssf, stf, table.nbr)
        ctx.save_for_backward(hf, ssf, stf, arg, cnt)
        ctx.table, ctx.one_set = table, one_set
        ctx.dtypes = (h.dtype, s_src.dtype, None if one_set else s_tgt.dtype)
        ctx.mark_non_differentiable(arg)
        return out.to(h.dtype), arg

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out, _g_arg):
        hf, ssf, stf, arg, cnt = ctx.saved_tensors
        table = ctx.table
        rev_ptr, rev_pos = table.reverse()
        g_h, g_ss, g_st = _native.gravnet_bwd(g_out.float(), hf, ssf, stf, table.nbr, rev_ptr, rev_pos, arg, cnt)
        dh, ds, dt = ctx.dtypes
        if ctx.one_set:
            return g_h.to(dh), (g_st + g_ss).to(ds), None, None, None
        return g_h.to(dh), g_ss.to(ds), g_st.to(dt), None, None


def _aggregate(h, s, table, s_dst):
    if isinstance(table, NeighborTable):
        if s_dst is not None:
            raise ValueError("gravnet_aggregate: s_dst goes with a BipartiteTable; a NeighborTable has one node set")
        if table.cnt is not None:
            raise ValueError("gravnet_aggregate needs a -1-padded table (knn_table), not a counted radius table")
        _native.gravnet_check_shapes(h, s, s, table.nbr)
        table.join()
        return _GravNetAggregate.apply(h, s, None, table, True)
    if isinstance(table, BipartiteTable):
        if s_dst is None:
            raise ValueError("gravnet_aggregate: a BipartiteTable needs s_dst, the coordinates of its queries")
        if table.cnt is not None:
            raise ValueError("gravnet_aggregate needs a -1-padded table (knn_xy_table), not a counted radius table")
        if s.dim() == 2 and s.shape[0] != table.num_candidates:
            raise ValueError(f"gravnet_aggregate: the table indexes {table.num_candidates} candidates, s has {s.shape[0]} rows")
        _native.gravnet_check_shapes(h, s, s_dst, table.nbr)
        return _GravNetAggregate.apply(h, s, s_dst, table, False)
    raise TypeError(f"gravnet_aggregate: table must be a NeighborTable or a BipartiteTable, got {type(table).__name__}")


def gravnet_aggregate(h: torch.Tensor, s: torch.Tensor, table: Union[NeighborTable, BipartiteTable],
                      s_dst: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[N_dst, 2P]: for every row i of `table`, the mean (columns 0..P-1) and the max (P..2P-1) over its valid slots
    j = table.nbr[i, t] of exp(-10 d_ij) h[j], d_ij = |s[j] - s_i|^2 in fp32 (the kNN build's distance chain).  A row
    without a valid slot gives zeros.

    Non-finite values: the mean half follows IEEE; the max half runs over the messages that are numbers (+-inf
    included) wherever they stand in the row -- a NaN never wins and never blocks, and a channel whose messages are all
    NaN is NaN and receives no gradient (upstream's amax propagates the NaN instead).  A non-finite h[j, p] changes
    channel p of the rows that list j and nothing else, forward and backward.

    NeighborTable (knn_table): one node set, s_i = s[i].  BipartiteTable (knn_xy_table): h, s belong to the candidates x,
    s_dst to the queries y.  Differentiable in h, s and s_dst.  1 <= S <= 16 coordinates, 1 <= P <= 128 features,
    k <= 64; anything else is a ValueError.  bf16 inputs (fp16 under fp16 autocast) are upcast exactly and the aggregate
    comes back in h's dtype.  Reads table.nbr and table.reverse(): no edge list, no host sync."""
    return _aggregate(h, s, table, s_dst)[0]


class GravNetConv(torch.nn.Module):
    """torch_geometric.nn.GravNetConv(in_channels, out_channels, space_dimensions, propagate_dimensions, k).

    forward(x, batch): s = lin_s(x), h = lin_h(x); the k nearest neighbours of every node in s (self included, at
    distance 0 and weight 1, as upstream's knn(s, s, k)); out = lin_out1(x) + lin_out2([mean | max] of
    exp(-10 d^2) h_j).  forward((x_l, x_r), (batch_l, batch_r)): sources x_l, targets x_r, one output row per row of
    x_r.  The graph follows this package's kNN rules (R1 distance chain, R2 ties to the lower index); there is no
    cosine distance.  num_workers is accepted and ignored, as in PyG."""

    def __init__(self, in_channels: int, out_channels: int, space_dimensions: int, propagate_dimensions: int, k: int,
                 num_workers: Optional[int] = None, **kwargs):
        super().__init__()
        if kwargs:
            raise TypeError(f"GravNetConv: unsupported arguments {sorted(kwargs)}")
        if not 1 <= int(space_dimensions) <= MAX_SPACE:
            raise ValueError(f"space_dimensions={space_dimensions}, supported 1..{MAX_SPACE}")
        if not 1 <= int(propagate_dimensions) <= MAX_PROPAGATE:
            raise ValueError(f"propagate_dimensions={propagate_dimensions}, supported 1..{MAX_PROPAGATE}")
        if not isinstance(k, int) or isinstance(k, bool) or not 1 <= k <= MAX_K:
            raise ValueError(f"k={k!r}, supported 1..{MAX_K}")
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.k = k
        self.num_workers = num_workers
        self.lin_s = torch.nn.Linear(in_channels, space_dimensions)
        self.lin_h = torch.nn.Linear(in_channels, propagate_dimensions)
        self.lin_out1 = torch.nn.Linear(in_channels, out_channels, bias=False)
        self.lin_out2 = torch.nn.Linear(2 * propagate_dimensions, out_channels)
        self.reset_parameters()

    def reset_parameters(self) -> None:
        self.lin_s.reset_parameters()
        self.lin_h.reset_parameters()
        self.lin_out1.reset_parameters()
        self.lin_out2.reset_parameters()

    def forward(self, x: Union[torch.Tensor, Tuple[torch.Tensor, torch.Tensor]],
                batch: Union[None, torch.Tensor, Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]] = None
                ) -> torch.Tensor:
        if isinstance(x, torch.Tensor):
            if isinstance(batch, (tuple, list)):
                raise ValueError("GravNetConv: a (batch_l, batch_r) pair goes with an (x_l, x_r) pair")
            s, h = self.lin_s(x), self.lin_h(x)
            table = knn_table(s.detach(), self.k, batch, loop=True)
            return self.lin_out1(x) + self.lin_out2(gravnet_aggregate(h, s, table))
        if not isinstance(x, (tuple, list)) or len(x) != 2:
            raise ValueError("GravNetConv: x must be a tensor or an (x_l, x_r) pair")
        x_l, x_r = x
        if batch is None:
            b_l = b_r = None
        elif isinstance(batch, (tuple, list)) and len(batch) == 2:
            b_l, b_r = batch
        else:
            raise ValueError("GravNetConv: an (x_l, x_r) pair needs batch=(batch_l, batch_r) or None")
        if x_l.dim() != 2 or x_r.dim() != 2 or x_l.shape[1] != x_r.shape[1]:
            raise ValueError(f"GravNetConv: x_l and x_r must be [N, {self.in_channels}], got {tuple(x_l.shape)} and "
                             f"{tuple(x_r.shape)}")
        h_l, s_l, s_r = self.lin_h(x_l), self.lin_s(x_l), self.lin_s(x_r)
        table = knn_xy_table(s_l.detach(), s_r.detach(), self.k, b_l, b_r)
        return self.lin_out1(x_r) + self.lin_out2(gravnet_aggregate(h_l, s_l, table, s_r))

    def __repr__(self) -> str:
        return f"{self.__class__.__name__}({self.in_channels}, {self.out_channels}, k={self.k})"

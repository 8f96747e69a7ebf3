"""Segment reductions with the torch_scatter signatures, plus the fused per-event MET reduction (K4).

Reference call sites: `scatter_add(weights*px, batch)` / `scatter_add(weights*py, batch)` at
/root/reference/model/net.py:55-56 (loss) and :132-133 (metrics).  Kernels: csrc/misc.hip (event_sum_kernel),
csrc/edgeconv.hip (segment_reduce_kernel).  Sums are deterministic: a fixed-shape tree per event, no float atomics.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _native
from .graph import _batch_info, _reverse_of_column, batch_info


class _SegmentSum1D(torch.autograd.Function):
    @staticmethod
    def forward(ctx, src, index, ptr):
        ctx.save_for_backward(index)
        return _native.segment_sum_1d(src, ptr)

    @staticmethod
    def backward(ctx, g_out):
        (index,) = ctx.saved_tensors
        return g_out.index_select(0, index), None, None


class _SegmentSumRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, msg, rowptr, num_rows):
        ctx.save_for_backward(rowptr)
        ctx.E = msg.shape[0]
        return _native.segment_sum(msg, rowptr, num_rows)

    @staticmethod
    def backward(ctx, g_out):
        (rowptr,) = ctx.saved_tensors
        return _native.segment_sum_bwd(g_out, rowptr, ctx.E), None, None


class _SegmentMaxRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, msg, rowptr, num_rows):
        out, arg = _native.segment_max(msg, rowptr, num_rows)
        ctx.save_for_backward(arg, rowptr)
        ctx.E = msg.shape[0]
        ctx.mark_non_differentiable(arg)
        return out, arg

    @staticmethod
    def backward(ctx, g_out, _g_arg):
        arg, rowptr = ctx.saved_tensors
        return _native.segment_max_bwd(g_out, arg, rowptr, ctx.E), None, None


_HALF = (torch.float16, torch.bfloat16)


def _dim_size(index: torch.Tensor, dim_size: Optional[int]) -> int:
    if dim_size is not None:
        return int(dim_size)
    return int(index.max()) + 1 if index.numel() else 0


def _group_rows(index: torch.Tensor, E: int, H: int, dim_size: Optional[int]):
    """(n, rowptr[n+1] int32, perm[E] int64 or None when the rows are grouped already) for an index of [E], [E,1] or
    an [E,H] index whose columns agree.  Indices outside [0, n) raise IndexError, differing columns
    NotImplementedError; both are read in the one host sync of the grouping test, after the reverse-index sort (safe for
    any key) and before any kernel reads `src` through the grouping."""
    if index.dtype != torch.int64:
        raise TypeError(f"index must be int64, got {index.dtype}")
    if index.dim() == 1:
        idx, per_column = index, False
    elif index.dim() == 2 and index.shape[1] in (1, H):
        idx, per_column = index[:, 0], index.shape[1] > 1
    else:
        raise ValueError(f"index must be [E], [E,1] or [E,{H}] for src [E,{H}], got {tuple(index.shape)}")
    if idx.numel() != E:
        raise ValueError(f"index has {idx.numel()} rows, src {E}")
    n = _dim_size(idx, dim_size)
    if E == 0:
        return n, torch.zeros(n + 1, dtype=torch.int32, device=index.device), None
    if n <= 0:
        raise IndexError(f"scatter: {E} indices into an output of {n} rows")
    rowptr, perm = _reverse_of_column(idx.to(torch.int32), n)
    ident = torch.arange(E, dtype=torch.int32, device=idx.device)
    ragged = (index != index[:, :1]).any() if per_column else torch.zeros((), dtype=torch.bool, device=idx.device)
    grouped, lo, hi, differ = torch.stack([(perm[:E] == ident).all().to(torch.int64), idx.min(), idx.max(),
                                           ragged.to(torch.int64)]).tolist()
    if differ:
        raise NotImplementedError("scatter: an [E,H] index must hold the same row in every column")
    if lo < 0 or hi >= n:
        raise IndexError(f"scatter: index {lo if lo < 0 else hi} is out of range for an output of {n} rows")
    return n, rowptr, (None if grouped else perm[:E].to(torch.int64))


def _grouped_sum(src: torch.Tensor, index: torch.Tensor, dim_size: Optional[int]) -> torch.Tensor:
    n, rowptr, perm = _group_rows(index, src.shape[0], src.shape[1], dim_size)
    grouped = src if perm is None else src.index_select(0, perm)
    return _SegmentSumRows.apply(grouped, rowptr, n)


def scatter_add(src: torch.Tensor, index: torch.Tensor, dim: int = -1, out: Optional[torch.Tensor] = None,
                dim_size: Optional[int] = None) -> torch.Tensor:
    """torch_scatter.scatter_add for the shapes on the hot path:
    1-D `src` with a sorted `index` (the batch vector): one deterministic segmented sum per event; any other in-range
    1-D index is grouped like the 2-D form;
    2-D `src` [E,H] along dim 0 (aggr='add'): grouped by index with a stable sort, then per-row sums.
    A bf16 or fp16 `src` is summed in fp32 by the same kernels and the result returned in src.dtype, as torch_scatter
    returns it.  Indices outside [0, dim_size) raise IndexError."""
    if index.dtype != torch.int64:
        raise TypeError(f"index must be int64, got {index.dtype}")
    if src.dtype in _HALF:
        res = scatter_add(src.float(), index, dim, None, dim_size).to(src.dtype)
        if out is not None:
            out.add_(res)
            return out
        return res
    if src.dim() == 1:
        if index.shape != src.shape:
            raise ValueError("index must have the same shape as a 1-D src")
        info = _batch_info(index, src.numel(), src.device, dim_size)
        if isinstance(info, str):       # unsorted, or out of range (then the grouping raises IndexError)
            res = _grouped_sum(src.view(-1, 1), index, dim_size).view(-1)
        else:
            res = _SegmentSum1D.apply(src, index, info.ptr)
            if dim_size is not None and res.numel() < dim_size:
                res = torch.cat([res, res.new_zeros(dim_size - res.numel())])
        if out is not None:
            out.add_(res)
            return out
        return res
    if src.dim() == 2 and dim in (0, -2):
        res = _grouped_sum(src, index, dim_size)
        if out is not None:
            out.add_(res)
            return out
        return res
    raise NotImplementedError(f"scatter_add: unsupported call shape src{tuple(src.shape)} dim={dim}")


def scatter_max(src: torch.Tensor, index: torch.Tensor, dim: int = 0, out=None,
                dim_size: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """torch_scatter.scatter_max for [E,H] rows along dim 0: (out, arg); empty rows -> 0 (R3), arg = winning row
    position in `src` (lowest on ties, R4); rows with no entry report arg = E like upstream.  A bf16 or fp16 `src` is
    compared in fp32 (exact) and the maxima returned in src.dtype.  Indices outside [0, dim_size) raise IndexError."""
    if src.dim() != 2 or dim not in (0, -2) or out is not None:
        raise NotImplementedError("scatter_max: only [E,H] along dim 0 without `out` is implemented")
    if src.dtype in _HALF:
        res, arg = scatter_max(src.float(), index, dim, None, dim_size)
        return res.to(src.dtype), arg
    E = src.shape[0]
    n, rowptr, perm = _group_rows(index, E, src.shape[1], dim_size)
    grouped = src if perm is None else src.index_select(0, perm)
    res, arg = _SegmentMaxRows.apply(grouped, rowptr, n)
    arg64 = arg.to(torch.int64)
    if perm is not None:
        arg64 = torch.where(arg64 >= 0, perm[arg64.clamp(min=0)], arg64)
    arg64 = torch.where(arg64 < 0, torch.full_like(arg64, E), arg64)
    return res, arg64


# ---------------------------------------------------------------------------------------------------------------
# K4: fused per-event MET
# ---------------------------------------------------------------------------------------------------------------
class _MetReduce(torch.autograd.Function):
    @staticmethod
    def forward(ctx, w, x, ptr):
        ctx.save_for_backward(x, ptr)
        return _native.met_reduce(w, x, ptr)

    @staticmethod
    def backward(ctx, g_met):
        x, ptr = ctx.saved_tensors
        return _native.met_reduce_bwd(g_met, x, ptr), None, None


def met_reduce(weights: torch.Tensor, x: torch.Tensor, batch: Optional[torch.Tensor] = None,
               ptr: Optional[torch.Tensor] = None, num_events: Optional[int] = None) -> torch.Tensor:
    """met[b] = (sum_i w_i * x[i,0], sum_i w_i * x[i,1]) over the nodes of event b: both scatter_add calls of
    model/net.py:55-56 in one pass over w and the px/py columns.  Differentiable w.r.t. `weights`.  bf16 or fp16
    `weights` are upcast (exact); the result is fp32."""
    if weights.dtype in _HALF:
        weights = weights.float()
    if ptr is None:
        ptr = batch_info(batch, weights.numel(), weights.device, num_events).ptr
    return _MetReduce.apply(weights, x, ptr)


class _MetLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, met, truth):
        loss, g = _native.met_loss(met, truth)
        ctx.save_for_backward(g)
        return loss.view(())

    @staticmethod
    def backward(ctx, g_loss):
        (g,) = ctx.saved_tensors
        return g * g_loss, None


class _MetLossFromWeights(torch.autograd.Function):
    """loss_fn of model/net.py:49-62 as ONE autograd node: MET reduction + loss forward (two kernels), one backward kernel
    that applies the upstream gradient of the scalar loss itself (the chain of two nodes needs a [B,2] multiply)."""

    @staticmethod
    def forward(ctx, w, x, ptr, truth):
        met = _native.met_reduce(w, x, ptr)
        loss, g = _native.met_loss(met, truth)
        ctx.save_for_backward(g, x, ptr)
        return loss.view(())

    @staticmethod
    def backward(ctx, g_loss):
        g, x, ptr = ctx.saved_tensors
        return _native.met_reduce_bwd(g, x, ptr, scale=g_loss.reshape(1).float()), None, None, None


def met_loss_from_weights(weights: torch.Tensor, x: torch.Tensor, truth: torch.Tensor, batch: Optional[torch.Tensor] = None,
                          ptr: Optional[torch.Tensor] = None) -> torch.Tensor:
    """met_loss(met_reduce(weights, x), truth) with the same bits, as one autograd node (bf16 or fp16 weights upcast)."""
    if weights.dtype in _HALF:
        weights = weights.float()
    if ptr is None:
        ptr = batch_info(batch, weights.numel(), weights.device, truth.shape[0]).ptr
    return _MetLossFromWeights.apply(weights, x, ptr, truth)


def met_loss(met: torch.Tensor, truth: torch.Tensor) -> torch.Tensor:
    """0.5 * mean_b((met[b,0] + truth[b,0])^2 + (met[b,1] + truth[b,1])^2) (model/net.py:58-61) in one kernel."""
    return _MetLoss.apply(met, truth)

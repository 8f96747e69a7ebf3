"""Segment reductions with the torch_scatter signatures, plus the fused per-event MET reduction (K4).

Reference call sites: `scatter_add(weights*px, batch)` / `scatter_add(weights*py, batch)` at
/root/reference/model/net.py:55-56 (loss) and :132-133 (metrics).  Kernels: csrc/misc.hip (event_sum_kernel),
csrc/edgeconv.hip (segment_reduce_kernel).  Sums are deterministic: a fixed-shape tree per event, no float atomics.

The rest of the torch_scatter family -- scatter, scatter_sum, scatter_mean, scatter_min, scatter_softmax,
scatter_log_softmax, scatter_logsumexp, segment_csr -- and torch_geometric.utils.softmax run on csrc/segment.hip, whose
kernels put a wavefront or a workgroup along a row of any length.  scatter_std takes its centred variance from
csrc/multi_aggr.hip.

Every autograd Function here is differentiable once: the segment Functions are `once_differentiable`, the MET Functions of
the training step open their backward with _native.no_double_backward; under create_graph=True both raise.
"""
from __future__ import annotations

import sys
import types
from typing import Optional, Tuple

import torch
from torch.autograd.function import once_differentiable

from . import _native
from .graph import _batch_info, _reverse_of_column, batch_info


class _SegmentSum1D(torch.autograd.Function):
    @staticmethod
    def forward(ctx, src, index, ptr):
        ctx.save_for_backward(index)
        return _native.segment_sum_1d(src, ptr)

    @staticmethod
    @once_differentiable
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
    @once_differentiable
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
    @once_differentiable
    def backward(ctx, g_out, _g_arg):
        arg, rowptr = ctx.saved_tensors
        return _native.segment_max_bwd(g_out, arg, rowptr, ctx.E), None, None


_HALF = (torch.float16, torch.bfloat16)


def _dim_size(index: torch.Tensor, dim_size: Optional[int]) -> int:
    if dim_size is not None:
        return int(dim_size)
    return int(index.max()) + 1 if index.numel() else 0


def _group_rows(index: torch.Tensor, E: int, H: int, dim_size: Optional[int], want_len: bool = False):
    """(n, rowptr[n+1] int32, perm[E] int64 or None when the rows are grouped already) for an index of [E], [E,1] or
    an [E,H] index whose columns agree.  Indices outside [0, n) raise IndexError, differing columns
    NotImplementedError; both are read in the one host sync of the grouping test, after the reverse-index sort (safe for
    any key) and before any kernel reads `src` through the grouping.  want_len: the longest row rides along in the same
    read and is returned as a fourth value (the max_len hint of csrc/segment.hip)."""
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
        rowptr = torch.zeros(n + 1, dtype=torch.int32, device=index.device)
        return (n, rowptr, None, 0) if want_len else (n, rowptr, None)
    if n <= 0:
        raise IndexError(f"scatter: {E} indices into an output of {n} rows")
    rowptr, perm = _reverse_of_column(idx.to(torch.int32), n)
    ident = torch.arange(E, dtype=torch.int32, device=idx.device)
    ragged = (index != index[:, :1]).any() if per_column else torch.zeros((), dtype=torch.bool, device=idx.device)
    stats = [(perm[:E] == ident).all().to(torch.int64), idx.min(), idx.max(), ragged.to(torch.int64)]
    if want_len:
        stats.append(rowptr.diff().max().to(torch.int64))
    grouped, lo, hi, differ, *longest = torch.stack(stats).tolist()
    if differ:
        raise NotImplementedError("scatter: an [E,H] index must hold the same row in every column")
    if lo < 0 or hi >= n:
        raise IndexError(f"scatter: index {lo if lo < 0 else hi} is out of range for an output of {n} rows")
    perm = None if grouped else perm[:E].to(torch.int64)
    return (n, rowptr, perm, int(longest[0])) if want_len else (n, rowptr, perm)


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
# The rest of the family over csrc/segment.hip: mean, min, softmax, log_softmax, logsumexp, segment_csr
#
# Call shapes, as scatter_add: a 1-D `src` with an index of the same shape, or `src` [E,H] along dim 0 with an index of
# [E], [E,1] or [E,H] with equal columns.  Out of scope: scatter_mul, segment_coo, any other `dim`, and an
# integer `src`.  (The global pools keep their own kernels: a faster pool would change bits that tests pin.)
# ---------------------------------------------------------------------------------------------------------------
scatter_sum = scatter_add


class _SegmentMeanRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, src, rowptr, max_len):
        ctx.save_for_backward(rowptr)
        ctx.E, ctx.max_len = src.shape[0], max_len
        return _native._segment_mean(src, rowptr, max_len)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out):
        (rowptr,) = ctx.saved_tensors
        return _native._segment_mean_bwd(g_out, rowptr, ctx.E, ctx.max_len), None, None


class _SegmentMinRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, src, rowptr, max_len):
        out, arg = _native._segment_min(src, rowptr, max_len)
        ctx.save_for_backward(arg, rowptr)
        ctx.E = src.shape[0]
        ctx.mark_non_differentiable(arg)
        return out, arg

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out, _g_arg):
        arg, rowptr = ctx.saved_tensors
        return _native.segment_max_bwd(g_out, arg, rowptr, ctx.E), None, None      # the same arg convention


class _SegmentSoftmaxRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, src, rowptr, log, max_len):
        y, _lse = _native._segment_softmax_fwd(src, rowptr, log, max_len)
        ctx.save_for_backward(y, rowptr)
        ctx.log, ctx.max_len = log, max_len
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        y, rowptr = ctx.saved_tensors
        return _native._segment_softmax_bwd(y, g, rowptr, ctx.log, ctx.max_len), None, None, None


class _SegmentLogSumExpRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, src, rowptr, max_len):
        out = _native._segment_logsumexp(src, rowptr, max_len)
        ctx.save_for_backward(src, out, rowptr)
        ctx.max_len = max_len
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out):
        src, out, rowptr = ctx.saved_tensors
        return _native._segment_logsumexp_bwd(src, out, g_out, rowptr, ctx.max_len), None, None


def _rows_of_src(who: str, src: torch.Tensor, index: Optional[torch.Tensor], dim: int) -> torch.Tensor:
    """`src` as [E,H] for one of the two call shapes; everything else is refused here, before any kernel."""
    if not src.dtype.is_floating_point or src.dtype == torch.float64:
        raise TypeError(f"{who}: src must be float32, bfloat16 or float16, got {src.dtype}")
    if index is not None and index.dtype != torch.int64:
        raise TypeError(f"index must be int64, got {index.dtype}")
    if src.dim() == 1 and dim in (0, -1):
        if index is not None and index.shape != src.shape:
            raise ValueError("index must have the same shape as a 1-D src")
        return src.view(-1, 1)
    if src.dim() == 2 and dim in (0, -2):
        return src
    raise NotImplementedError(f"{who}: unsupported call shape src{tuple(src.shape)} dim={dim}")


def _scatter_rows(who: str, fn, src: torch.Tensor, index: torch.Tensor, dim: int, dim_size: Optional[int],
                  per_entry: bool = False, longest: bool = True):
    """The tensors of fn(grouped fp32 rows, rowptr, max_len) for a torch_scatter call, in src's dtype and dimensionality:
    per row, or (per_entry) per entry and back in src's own order.  Also (E, perm).  max_len is the longest row, read in
    the grouping's own host sync, or (longest=False) the mean length that segment_csr has to go by: mean sums in an order
    that depends on the form the hint selects, and a grouped index and the equal segment_csr call give the same bits."""
    rows = _rows_of_src(who, src, index, dim)
    E, H = rows.shape
    n, rowptr, perm, max_len = _group_rows(index, E, H, dim_size, want_len=True)
    if not longest:
        max_len = _mean_len(E, n)
    grouped = rows.float() if perm is None else rows.float().index_select(0, perm)
    res = fn(grouped, rowptr, max_len)
    outs = []
    for t in (res if isinstance(res, tuple) else (res,)):
        if t.is_floating_point():
            if per_entry and perm is not None:
                t = torch.zeros_like(t).index_copy_(0, perm, t)      # perm is a permutation: every row is written
            t = t.to(src.dtype)
        outs.append(t.view(-1) if src.dim() == 1 else t)
    return outs, E, perm


def _no_out(who: str, out) -> None:
    if out is not None:
        raise NotImplementedError(f"{who}: `out` is not implemented")


def scatter_mean(src: torch.Tensor, index: torch.Tensor, dim: int = -1, out: Optional[torch.Tensor] = None,
                 dim_size: Optional[int] = None) -> torch.Tensor:
    """torch_scatter.scatter_mean for the call shapes of scatter_add: fp32 sum / fp32 max(count, 1), so an empty row
    gives 0.  Differentiable; bf16 / fp16 are computed in fp32 and returned in src.dtype.  `out` and an integer `src`
    are not implemented."""
    _no_out("scatter_mean", out)
    (res,), _E, _perm = _scatter_rows("scatter_mean", _SegmentMeanRows.apply, src, index, dim, dim_size, longest=False)
    return res


def scatter_min(src: torch.Tensor, index: torch.Tensor, dim: int = -1, out=None,
                dim_size: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """torch_scatter.scatter_min: (out, arg), the mirror of scatter_max: an empty row gives 0 (R3) and arg = E, arg is
    the winning position in `src`, the lowest on ties (R4).  Differentiable in `out`.  NaN inputs are out of scope."""
    _no_out("scatter_min", out)
    (res, arg), E, perm = _scatter_rows("scatter_min", _SegmentMinRows.apply, src, index, dim, dim_size, longest=False)
    arg64 = arg.to(torch.int64)
    if perm is not None:
        arg64 = torch.where(arg64 >= 0, perm[arg64.clamp(min=0)], arg64)
    return res, torch.where(arg64 < 0, torch.full_like(arg64, E), arg64)


def scatter_std(src: torch.Tensor, index: torch.Tensor, dim: int = -1, out: Optional[torch.Tensor] = None,
                dim_size: Optional[int] = None, unbiased: bool = True) -> torch.Tensor:
    """torch_scatter.scatter_std for the call shapes of scatter_mean (rows of up to 256 features): with n the number of
    entries of a row and var = (1/n) sum (x - mean)^2,

        sqrt(n var / (max(n - 1, 1) + 1e-6))    unbiased        sqrt(n var / (n + 1e-6))    otherwise

    which is torch_scatter's published formula (sum of squared deviations over count + 1e-6; **unpinned**: torch_scatter
    is not installed next to this package).  var is csrc/multi_aggr.hip's: centred on the row's own mean in a second
    walk, never a difference of two fp32 means, and gathered through the grouping permutation, so an unsorted index
    costs no grouped copy of src.  An empty row and a row of one entry give 0.  Differentiable; the gradient at zero
    variance is infinite (the derivative of sqrt at 0), as upstream.  bf16 / fp16 are computed in fp32 and returned in
    src.dtype.  `out` is not implemented."""
    from .pna import _aggregate_rows
    _no_out("scatter_std", out)
    rows = _rows_of_src("scatter_std", src, index, dim)
    E, H = rows.shape
    n, rowptr, perm = _group_rows(index, E, H, dim_size)
    var, count = _aggregate_rows(rows.float(), rowptr, perm, n, ("var",))
    cnt = count.to(torch.float32).view(-1, 1)
    denom = ((cnt - 1).clamp(min=1) if unbiased else cnt) + 1e-6
    res = (cnt * var.view(n, H) / denom).sqrt().to(src.dtype)
    return res.view(-1) if src.dim() == 1 else res


def scatter(src: torch.Tensor, index: torch.Tensor, dim: int = -1, out: Optional[torch.Tensor] = None,
            dim_size: Optional[int] = None, reduce: str = "sum") -> torch.Tensor:
    """torch_scatter.scatter: 'sum' / 'add' and 'max' are scatter_add and scatter_max themselves (their bits), 'mean' and
    'min' the functions above; 'min' and 'max' return the values only.  'mul' (scatter_mul) is not implemented, nor is
    segment_coo, a `dim` other than the two call shapes of scatter_add, and an integer `src`."""
    if reduce in ("sum", "add"):
        return scatter_add(src, index, dim, out, dim_size)
    if reduce == "mean":
        return scatter_mean(src, index, dim, out, dim_size)
    if reduce == "min":
        return scatter_min(src, index, dim, out, dim_size)[0]
    if reduce == "max":
        return scatter_max(src, index, dim, out, dim_size)[0]
    if reduce == "mul":
        raise NotImplementedError("scatter: reduce='mul' (scatter_mul) is not implemented")
    raise ValueError(f"scatter: unknown reduce {reduce!r}")


def scatter_softmax(src: torch.Tensor, index: torch.Tensor, dim: int = -1, dim_size: Optional[int] = None) -> torch.Tensor:
    """torch_scatter.scatter_softmax: the softmax of the entries that share an index, in src's own order (an unsorted
    index is grouped, computed and un-permuted).  The row maximum is subtracted in one online pass; a -inf beside finite
    scores gives exactly 0, a row of -inf alone NaN like torch.softmax.  Differentiable."""
    (res,), _E, _perm = _scatter_rows("scatter_softmax", lambda s, rp, ml: _SegmentSoftmaxRows.apply(s, rp, False, ml), src,
                                      index, dim, dim_size, per_entry=True)
    return res


def scatter_log_softmax(src: torch.Tensor, index: torch.Tensor, dim: int = -1, eps: float = 1e-12,
                        dim_size: Optional[int] = None) -> torch.Tensor:
    """torch_scatter.scatter_log_softmax: (s - m) - logf(l).  `eps` is accepted and cannot change an fp32 result: upstream
    adds it to l = sum expf(s - m) >= 1, and 1 + 1e-12 rounds to 1."""
    (res,), _E, _perm = _scatter_rows("scatter_log_softmax", lambda s, rp, ml: _SegmentSoftmaxRows.apply(s, rp, True, ml),
                                      src, index, dim, dim_size, per_entry=True)
    return res


def scatter_logsumexp(src: torch.Tensor, index: torch.Tensor, dim: int = -1, out: Optional[torch.Tensor] = None,
                      dim_size: Optional[int] = None, eps: float = 1e-12) -> torch.Tensor:
    """torch_scatter.scatter_logsumexp: m + logf(l) per row, 0 for an empty row (what upstream's nan_to_num_ leaves).
    `eps` is accepted and cannot change an fp32 result (l >= 1, and 1 + 1e-12 rounds to 1).  `out` is not implemented."""
    _no_out("scatter_logsumexp", out)
    (res,), _E, _perm = _scatter_rows("scatter_logsumexp", _SegmentLogSumExpRows.apply, src, index, dim, dim_size)
    return res


def _csr_rowptr(indptr: torch.Tensor, E: int) -> torch.Tensor:
    """int32 rowptr of a caller's indptr without a host read: clamped to [0, E] on the device, so that a malformed indptr
    gives wrong rows and never an access outside src (a row whose end lies before its start is empty to every kernel;
    a running maximum would cost a serial scan of the whole indptr, 0.4 ms at 288 000 rows)."""
    if indptr.dim() != 1 or indptr.numel() < 1 or indptr.dtype not in (torch.int64, torch.int32):
        raise ValueError(f"indptr must be 1-D int64 with at least one entry, got {indptr.dtype} {tuple(indptr.shape)}")
    return indptr.clamp(0, E).to(torch.int32)


def _mean_len(E: int, n: int) -> int:
    """A max_len hint that needs no host read: the longest of n rows over E entries has at least ceil(E / n)."""
    return -(-E // n) if n > 0 else 0


def segment_csr(src: torch.Tensor, indptr: torch.Tensor, out: Optional[torch.Tensor] = None,
                reduce: str = "sum") -> torch.Tensor:
    """torch_scatter.segment_csr for a 1-D `indptr` over dim 0 of a 1-D or [E,H] `src`: 'sum' / 'add' and 'max' with the
    kernels (and bits) of scatter_add / scatter_max on the same grouped rows, 'mean' and 'min' as above; 'min' and 'max'
    return the values only.  No sort and no host sync: indptr is clamped on the device, not checked."""
    _no_out("segment_csr", out)
    if reduce not in ("sum", "add", "mean", "min", "max"):
        raise ValueError(f"segment_csr: unknown reduce {reduce!r}")
    rows = _rows_of_src("segment_csr", src, None, 0)
    E = rows.shape[0]
    rowptr = _csr_rowptr(indptr, E)
    n = indptr.numel() - 1
    rows = rows.float()
    if reduce in ("sum", "add"):
        res = _SegmentSumRows.apply(rows, rowptr, n)
    elif reduce == "max":
        res = _SegmentMaxRows.apply(rows, rowptr, n)[0]
    elif reduce == "mean":
        res = _SegmentMeanRows.apply(rows, rowptr, _mean_len(E, n))
    else:
        res = _SegmentMinRows.apply(rows, rowptr, _mean_len(E, n))[0]
    res = res.to(src.dtype)
    return res.view(-1) if src.dim() == 1 else res


def _event_rows(index: Optional[torch.Tensor], ptr: Optional[torch.Tensor], N: int, device, num_nodes: Optional[int]):
    """(n, rowptr int32, max_len hint) without a host sync for a `ptr` (it wins, as upstream) or a registered batch
    vector, one row over everything for neither; None for any other index (it is grouped, with the one sync of that)."""
    from .graph import _batch_registry, _registry_get
    if ptr is not None:
        n = ptr.numel() - 1
        return n, _csr_rowptr(ptr, N), _mean_len(N, n)
    if index is None:
        return 1, torch.tensor([0, N], dtype=torch.int32, device=device), N
    info = _registry_get(_batch_registry, index) if index.dim() == 1 and index.numel() == N else None
    if info is None or (num_nodes is not None and num_nodes != info.num_events):
        return None
    return info.num_events, _csr_rowptr(info.ptr, N), max(info.max_nodes or 0, _mean_len(N, info.num_events))


def softmax(src: torch.Tensor, index: Optional[torch.Tensor] = None, ptr: Optional[torch.Tensor] = None,
            num_nodes: Optional[int] = None, dim: int = 0) -> torch.Tensor:
    """torch_geometric.utils.softmax over dim 0 of a 1-D or [N,H] `src`: the softmax of the entries of each group, given by
    `ptr` (it wins when both are given, as upstream) or by `index`.  With `ptr`, or with a registered batch vector
    (register_batch, a DataLoader's batch) as `index`, there is no host sync; any other index is grouped like
    scatter_softmax's.  A long group (an event of thousands of nodes) is walked by a whole workgroup.  `ptr` is clamped to
    [0, N] and otherwise taken on trust, as upstream: it must be non-decreasing, else the entries in a gap between two
    groups are left unwritten and entries two groups share are written by both (in bounds, but undefined values)."""
    rows = _rows_of_src("softmax", src, None if ptr is not None else index, dim)
    ev = _event_rows(index, ptr, rows.shape[0], src.device, num_nodes)
    if ev is None:
        return scatter_softmax(src, index, 0 if src.dim() == 2 else -1, num_nodes)
    _n, rowptr, max_len = ev
    res = _SegmentSoftmaxRows.apply(rows.float(), rowptr, False, max_len).to(src.dtype)
    return res.view(-1) if src.dim() == 1 else res


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
        _native.no_double_backward("_MetReduce")
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
        return loss.squeeze_(0)     # the [1] tensor itself as a scalar: a view made in here could not be written in place

    @staticmethod
    def backward(ctx, g_loss):
        _native.no_double_backward("_MetLoss")
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
        return loss.squeeze_(0)     # the [1] tensor itself as a scalar: a view made in here could not be written in place

    @staticmethod
    def backward(ctx, g_loss):
        _native.no_double_backward("_MetLossFromWeights")
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


# `from deepmetv2_amd import scatter` has to give torch_scatter's `scatter`, and `deepmetv2_amd.scatter` is this module
# (met_loss_from_weights and the autograd functions are reached through it): the module itself is callable as the function.
class _ScatterModule(types.ModuleType):
    def __call__(self, src, index, dim=-1, out=None, dim_size=None, reduce="sum"):
        return scatter(src, index, dim, out, dim_size, reduce)


sys.modules[__name__].__class__ = _ScatterModule

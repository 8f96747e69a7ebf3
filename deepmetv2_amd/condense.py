"""Object-condensation inference of every event of a batch: `condensation_cluster`, `condensation_points`.

The kernel is in csrc/condense.hip (include/dmet.h, section "Condensation clustering"): the hits of an event are collected
around its highest-beta points, one workgroup per event, every event of the batch in one launch, where upstream walks a
Python loop with one device read per condensation point.  This file is argument checking, the ranking (the per-event
top-k launch of select.py over a score with the non-candidates at -inf) and the node-level torch work around the launch.
Nothing here is differentiable and nothing is an autograd Function.
"""
from __future__ import annotations

import ctypes
import math
import numbers
from typing import Optional

import torch

from . import _native
from .graph import _deferred, batch_info, register_batch

__all__ = ["condensation_cluster", "condensation_points"]


def _threshold(v, name: str, who: str, positive: bool) -> float:
    """A host number as the kernel takes it: finite (and > 0) also once rounded to fp32."""
    if isinstance(v, bool) or not isinstance(v, numbers.Real) or not math.isfinite(v):
        raise ValueError(f"{who}: {name} must be a finite number, got {v!r}")
    f = ctypes.c_float(float(v)).value
    if not math.isfinite(f) or (positive and not f > 0):
        raise ValueError(f"{who}: {name} must be {'positive and ' if positive else ''}finite in fp32, got {v!r}")
    return f


def _floating(t, name: str, who: str) -> torch.Tensor:
    if not torch.is_tensor(t) or t.dtype not in (torch.float32, torch.bfloat16, torch.float16):
        raise TypeError(f"{who}: {name} must be a float32, bfloat16 or float16 tensor, got "
                        f"{t.dtype if torch.is_tensor(t) else type(t).__name__}")
    return t.detach()


def _check(beta, x, batch, ptr, t_beta, t_d, who: str):
    """Everything the host can tell without the device: (beta [N], x [N, D], t_beta, t_d), the tensors as views of the
    caller's."""
    t_beta = _threshold(t_beta, "t_beta", who, False)
    t_d = _threshold(t_d, "t_d", who, True)
    beta, x = _floating(beta, "beta", who), _floating(x, "x", who)
    if beta.dim() == 2 and beta.shape[1] == 1:
        beta = beta.squeeze(1)
    if beta.dim() != 1:
        raise ValueError(f"{who}: beta must be [N] or [N, 1], got {list(beta.shape)}")
    if x.dim() == 1:
        x = x.unsqueeze(1)
    N = beta.numel()
    if x.dim() != 2 or x.shape[0] != N:
        raise ValueError(f"{who}: x must be [N, D] (or [N]) with N = {N} rows, got {list(x.shape)}")
    if not 1 <= x.shape[1] <= _native.CONDENSE_MAX_DIM:
        raise ValueError(f"{who}: x has D = {x.shape[1]} coordinates, 1..{_native.CONDENSE_MAX_DIM} are supported")
    if ptr is not None and (not torch.is_tensor(ptr) or ptr.dtype != torch.int64 or ptr.dim() != 1 or ptr.numel() < 1):
        raise TypeError(f"{who}: ptr must be a 1-D int64 (torch.long) tensor of B + 1 event offsets")
    if batch is not None and (not torch.is_tensor(batch) or batch.dim() != 1 or batch.numel() != N):
        raise ValueError(f"{who}: batch must be a 1-D int64 tensor of one event per node ({N}), got "
                         f"{list(batch.shape) if torch.is_tensor(batch) else type(batch).__name__}")
    return beta, x, t_beta, t_d


def _condense(beta, x, batch, ptr, t_beta, t_d, who: str):
    """(local, assoc, ncl, ptr) of the launch: the score op, the ranking launch and the walk; no host read with ptr or a
    registered batch."""
    beta, x, t_beta, t_d = _check(beta, x, batch, ptr, t_beta, t_d, who)
    dev = _native._require_device(beta, x, batch, ptr)
    beta, x = beta.to(torch.float32), x.to(torch.float32)      # bf16 / fp16 -> fp32 is exact
    N = beta.numel()
    if ptr is None:
        ptr = batch_info(batch, N, dev).ptr
    _deferred.poll()
    # the candidates lead every event's ranking: the walk ends at the first entry that is none
    score = torch.where(beta > t_beta, beta, float("-inf"))
    order, _node_map = _native._topk(score, ptr, ptr, N)
    local, assoc, ncl, flags = _native._condense(beta, x, order, ptr, t_beta, t_d)
    if flags.is_cuda and not torch.cuda.is_current_stream_capturing():      # a captured graph cannot report
        _deferred.post(flags[0:1], f"{who}: the ranking holds an entry outside its event (a defect of the ranking): the "
                                   "labels are not to be trusted")
        _deferred.post(flags[1:2], f"{who}: the walk reached its loop bound (a defect of the kernel): the labels are not to "
                                   "be trusted")
    return local, assoc, ncl, ptr


def _first_of_event(ncl: torch.Tensor) -> torch.Tensor:
    return torch.cumsum(ncl, 0) - ncl


def condensation_cluster(beta: torch.Tensor, x: torch.Tensor, batch: Optional[torch.Tensor] = None, *,
                         ptr: Optional[torch.Tensor] = None, t_beta: float = 0.1, t_d: float = 0.8,
                         return_assoc: bool = False):
    """Object-condensation inference (Kieseler 2020): labels, int64 [N] (-1 = noise); with return_assoc=True
    (labels, assoc), assoc int64 [N] the global id of every node's condensation point (a point holds itself, noise -1).

    beta [N] (or [N, 1]): the condensation weights; x [N, D], 1 <= D <= 8 (or [N]): the cluster coordinates.  float32;
    bfloat16 and float16 are upcast, which is exact; float64 is a TypeError.
    Per event (include/dmet.h, "Condensation clustering"): the candidates are the nodes with beta > t_beta (strictly, in
    fp32: a NaN is none).  They are walked by descending beta, ties to the lower index (-0.0 = +0.0, the order of `topk`).
    A candidate that is still unassigned becomes the next condensation point and takes, with itself, every still-unassigned
    node of the event within t_d of it: the squared distance in fp32 as `radius_graph` forms it, strictly below
    fp32(t_d)^2.  So a candidate is a condensation point iff no condensation point with a higher beta lies within t_d of it, and
    a node belongs to the highest-beta condensation point within t_d.  A candidate with a NaN coordinate is a point of
    itself alone.
    Labels are numbered over the batch as `dbscan` numbers them: event by event, and inside an event in the order the
    points were found (descending beta).
    batch / ptr: the events, one workgroup each (ptr: int64 [B + 1] offsets, taken on trust; neither: one event).  An
    unsorted, unregistered batch is a ValueError.  N = 0 and empty events work.
    One elementwise op, the ranking launch (`topk`'s kernel), one launch for the walk, a cumsum over the events and an add
    per node; no host read with ptr or a registered batch.  Not differentiable."""
    who = "condensation_cluster"
    local, assoc, ncl, ptr = _condense(beta, x, batch, ptr, t_beta, t_d, who)
    if ncl.numel() > 1:
        # batch-wide numbers: the clusters of the earlier events first (no host read: the counts stay on the device)
        per_node = torch.repeat_interleave(_first_of_event(ncl), ptr.diff(), output_size=local.numel())
        labels = torch.where(local >= 0, local + per_node, local)
    else:
        labels = local
    return (labels, assoc) if return_assoc else labels


def condensation_points(beta: torch.Tensor, x: torch.Tensor, batch: Optional[torch.Tensor] = None, *,
                        ptr: Optional[torch.Tensor] = None, t_beta: float = 0.1, t_d: float = 0.8):
    """(points int64 [K], points_batch int64 [K]): the condensation points of the batch, event by event and inside an event
    in the order found, and the event of each.  points[labels[i]] == assoc[i] for every node i that is not noise, with
    labels and assoc as `condensation_cluster` returns them for the same arguments: per-object properties are read as
    pred[points].
    One host read, of K.  points_batch comes back registered (register_batch), so a graph build over the points needs no
    further read."""
    who = "condensation_points"
    local, assoc, ncl, ptr = _condense(beta, x, batch, ptr, t_beta, t_d, who)
    dev, N, B = local.device, local.numel(), ncl.numel()
    first = _first_of_event(ncl)
    pptr = torch.cat([first, ncl.sum(0, keepdim=True)]) if B else torch.zeros(1, dtype=torch.int64, device=dev)
    stats = [pptr[-1]] + ([ncl.max(), ncl.min()] if B else [])
    K, *mm = (int(v) for v in torch.stack(stats).tolist())                 # the one host read
    ids = torch.arange(N, dtype=torch.int64, device=dev)
    is_point = assoc == ids
    # a point's slot: its event's first slot + its number in the event
    per_node = torch.repeat_interleave(first, ptr.diff(), output_size=N) if B else local
    slot = torch.where(is_point, local + per_node, torch.full_like(local, K))
    points = torch.full((K + 1,), -1, dtype=torch.int64, device=dev)
    points[slot] = ids                                                      # every slot below K is written by one point
    points = points[:K]
    points_batch = torch.repeat_interleave(torch.arange(B, dtype=torch.int64, device=dev), ncl, output_size=K)
    register_batch(points_batch, pptr, B, *(mm if B else (0, 0)))
    return points, points_batch

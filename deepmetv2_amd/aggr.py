"""Aggregations over the nodes of an event that are torch modules: torch_geometric.nn.aggr.AttentionalAggregation
(earlier GlobalAttention), an attention read-out -- the per-event reduction a MET regression ends in.

It is composed from the segment softmax under `softmax` (csrc/segment.hip: an event of thousands of nodes is one long row,
walked by a workgroup) and the segment sum under scatter_add, over one grouping of the index; it has no kernel of its
own."""
from __future__ import annotations

from typing import Optional

import torch

from .scatter import _SegmentSoftmaxRows, _SegmentSumRows, _event_rows, _group_rows


class AttentionalAggregation(torch.nn.Module):
    """out[b] = sum over the nodes i of event b of softmax_b(gate_nn(x))_i * nn(x)_i.

    gate_nn maps [N, F_in] to [N, 1] (one weight per node) or [N, F] (one per channel); nn (optional) maps [N, F_in] to
    [N, F].  With `ptr`, or with a registered batch vector as `index`, the forward and the backward make no host sync."""

    def __init__(self, gate_nn: torch.nn.Module, nn: Optional[torch.nn.Module] = None):
        super().__init__()
        self.gate_nn = gate_nn
        self.nn = nn

    def reset_parameters(self):
        for m in (self.gate_nn, self.nn):
            for layer in (m.modules() if m is not None else ()):
                if hasattr(layer, "reset_parameters"):
                    layer.reset_parameters()

    def forward(self, x: torch.Tensor, index: Optional[torch.Tensor] = None, ptr: Optional[torch.Tensor] = None,
                dim_size: Optional[int] = None) -> torch.Tensor:
        if x.dim() != 2:
            raise NotImplementedError(f"AttentionalAggregation: x must be [N, F], got {tuple(x.shape)}")
        gate = self.gate_nn(x)
        h = self.nn(x) if self.nn is not None else x
        if gate.dim() != 2 or gate.shape[0] != x.shape[0] or gate.shape[1] not in (1, h.shape[1]):
            raise ValueError(f"gate_nn must give [N, 1] or [N, {h.shape[1]}], got {tuple(gate.shape)}")
        ev = _event_rows(index, ptr, x.shape[0], x.device, dim_size)
        if ev is None:      # an index that is no registered batch vector: grouped once, with the one host sync of that
            n, rowptr, perm, max_len = _group_rows(index, x.shape[0], 1, dim_size, want_len=True)
            if perm is not None:
                gate, h = gate.index_select(0, perm), h.index_select(0, perm)
        else:
            n, rowptr, max_len = ev
        weighted = _SegmentSoftmaxRows.apply(gate.float(), rowptr, False, max_len).to(gate.dtype) * h
        return _SegmentSumRows.apply(weighted.float(), rowptr, n).to(weighted.dtype)

    def __repr__(self) -> str:
        return f"{self.__class__.__name__}(gate_nn={self.gate_nn}, nn={self.nn})"

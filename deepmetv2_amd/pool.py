"""Graph coarsening and readout with the torch_cluster / PyG signatures: graclus, normalized_cut, max_pool(_x),
avg_pool(_x) and the global pools.

Reference call sites: model/dynamic_reduction_network.py:89-92 (normalized_cut_2d, graclus, max_pool), :97-99
(normalized_cut_2d, graclus, max_pool_x), :101 (global_max_pool).  Kernels: csrc/pool.hip (matching, edge weights,
pair pooling) and the segment reductions of csrc/edgeconv.hip (general cluster vectors, global pools).

graclus here is torch_cluster's GPU algorithm made deterministic: the result is a function of (graph, weights, seed)
and is reproducible per seed; upstream's is random and not reproducible, so the two agree in distribution, not in bits.
"""
from __future__ import annotations

import copy
from typing import Optional, Tuple

import torch
from torch.autograd.function import once_differentiable

from . import _native
from .graph import BatchInfo, _registry_get, _registry_put, batch_info, coalesced_tag, lookup_graph, register_batch
from .scatter import _SegmentMaxRows, _SegmentSumRows, scatter_add

# graclus output tensor -> partner[N] int32 (the pair-pooling path takes it; any other cluster vector is general)
_graclus_registry = {}


# ---------------------------------------------------------------------------------------------------------------
# matching and edge weights
# ---------------------------------------------------------------------------------------------------------------
def _num_nodes(edge_index: torch.Tensor, num_nodes: Optional[int]) -> int:
    if num_nodes is not None:
        return int(num_nodes)
    return int(edge_index.max().item()) + 1 if edge_index.numel() else 0      # one host sync, as upstream


def _check_edge_index(edge_index: torch.Tensor) -> None:
    _native._require_device(edge_index)
    if edge_index.dim() != 2 or edge_index.shape[0] != 2 or edge_index.dtype != torch.int64:
        raise ValueError(f"edge_index must be an int64 [2, E] tensor, got {edge_index.dtype} {tuple(edge_index.shape)}")


def graclus(edge_index: torch.Tensor, weight: Optional[torch.Tensor] = None, num_nodes: Optional[int] = None, *,
            batch: Optional[torch.Tensor] = None, seed: Optional[int] = None, max_rounds: int = 0) -> torch.Tensor:
    """torch_cluster.graclus: greedy pairwise matching, cluster[N] int64 with cluster[u] = min(u, v) for a matched pair
    and u for a singleton (rules: include/dmet.h, dmet_graclus_f32).

    Keyword extensions: `batch` (or a batch registered with `register_batch`) gives the events, which are matched by
    one workgroup each in one launch; `seed` (default: drawn from torch's default CPU generator, so torch.manual_seed
    controls it) makes the result reproducible; `max_rounds` bounds the parallel rounds before the sequential finisher.
    Without `batch`, the events of a knn_graph / radius_graph edge index (also after to_undirected) are used; any other
    graph is matched as ONE block by one workgroup -- correct, but serial over the whole graph.
    Edges must not cross events.  No host sync when `batch` is registered (or num_nodes given with an event-tagged
    graph)."""
    _check_edge_index(edge_index)
    dev = edge_index.device
    if batch is not None:
        N = batch.numel() if num_nodes is None else int(num_nodes)
        ptr = batch_info(batch, N, dev).ptr
    else:
        N = _num_nodes(edge_index, num_nodes)
        tag = coalesced_tag(edge_index)
        ptr = tag[0] if tag is not None else None
        if ptr is None:
            g = lookup_graph(edge_index)
            ptr = g[0].ptr if g is not None else None
        if ptr is None or int(ptr.numel()) < 2:
            ptr = torch.tensor([0, N], dtype=torch.int64, device=dev)
    if seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    if weight is not None:
        _native._require_device(weight)
        weight = weight.reshape(-1)
        if weight.numel() != edge_index.shape[1]:
            raise ValueError(f"weight must hold one value per edge ({edge_index.shape[1]}), got {weight.numel()}")
    rowptr, col, w = _csr(edge_index, N, weight)
    cluster, partner, _rounds = _native.graclus(rowptr, col, w, ptr, seed, max_rounds)
    _registry_put(_graclus_registry, cluster, partner)
    return cluster


def _csr(edge_index: torch.Tensor, N: int, weight: Optional[torch.Tensor]):
    """rowptr[N+1] int64, col[E] int32, weight in ascending (row, col) order (stable: duplicates keep their order)."""
    row, col = edge_index[0], edge_index[1]
    if coalesced_tag(edge_index) is None and edge_index.shape[1] > 0:
        _key, perm = torch.sort(row * max(N, 1) + col, stable=True)
        row, col = row[perm], col[perm]
        weight = weight[perm] if weight is not None else None
    rowptr = torch.searchsorted(row.contiguous(), torch.arange(N + 1, dtype=torch.int64, device=row.device))
    w = weight.to(torch.float32).contiguous() if weight is not None else None
    return rowptr, col.to(torch.int32).contiguous(), w


def normalized_cut(edge_index: torch.Tensor, edge_attr: torch.Tensor, num_nodes: Optional[int] = None) -> torch.Tensor:
    """torch_geometric.utils.normalized_cut: edge_attr * (1/deg(row) + 1/deg(col)), deg = in-degree over col (fp32).
    Not differentiable (the weights only steer graclus)."""
    _check_edge_index(edge_index)
    N = _num_nodes(edge_index, num_nodes)
    w = _native.normalized_cut(edge_index, N, attr=edge_attr.detach())
    return w.view(edge_attr.shape)


def normalized_cut_2d(edge_index: torch.Tensor, pos: torch.Tensor) -> torch.Tensor:
    """The DRN's helper (model/dynamic_reduction_network.py, used at :89,97): normalized_cut with
    edge_attr = ||pos[row] - pos[col]||_2, fused in one kernel, pos[N, D<=64].  Not differentiable."""
    _check_edge_index(edge_index)
    if pos.dim() != 2:
        raise ValueError(f"pos must be [N, D], got {tuple(pos.shape)}")
    return _native.normalized_cut(edge_index, pos.shape[0], x=pos.detach())


# ---------------------------------------------------------------------------------------------------------------
# cluster pooling
# ---------------------------------------------------------------------------------------------------------------
class _PairPool(torch.autograd.Function):
    """Pooling of a graclus result: max (gradient to the winning member) or mean (split over the members).
    `once_differentiable`."""

    @staticmethod
    def forward(ctx, x, partner, cid, ptr, C, mode, want_batch):
        mx, arg, mean, pb = _native.pool_pairs(x, partner, cid, ptr, C, mode == "max", mode == "mean", want_batch)
        ctx.save_for_backward(partner, cid, arg)
        ctx.mode, ctx.C, ctx.F = mode, C, x.shape[1]
        out = mx if mode == "max" else mean
        if pb is None:
            pb = torch.empty(0, dtype=torch.int64, device=x.device)
        ctx.mark_non_differentiable(pb)
        return out, pb

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _g_pb):
        partner, cid, arg = ctx.saved_tensors
        gx = _native.pool_pairs_bwd(g if ctx.mode == "max" else None, arg, g if ctx.mode == "mean" else None,
                                    partner, cid, ctx.F, ctx.C)
        return gx, None, None, None, None, None, None


class _Coarsening:
    """How the nodes of one graph map to pooled rows: node_map[N] int64 (consecutive cluster ids), C, the pooled batch
    and its ptr.  Building it costs ONE host sync (the pooled size and the pooled events' largest / smallest sizes)."""

    def __init__(self, cluster: torch.Tensor, batch: Optional[torch.Tensor], N: int):
        dev = cluster.device
        self.batch_in = batch
        binfo = batch_info(batch, N, dev) if batch is not None else BatchInfo(
            torch.tensor([0, N], dtype=torch.int64, device=dev), 1, N, N, N)
        self.B = binfo.num_events
        self.partner = _registry_get(_graclus_registry, cluster)
        self.batch = None
        self.ptr = None
        self.max_nodes = self.min_nodes = None
        if self.partner is not None:
            # graclus clusters: ids from a prefix sum over the leader flags, rows already grouped by event
            self.node_map, self.ptr = _native.pool_pairs_index(self.partner, binfo.ptr)
            if self.B > 0:
                d = self.ptr.diff()
                C, mx, mn = (int(v) for v in torch.stack([self.ptr[-1], d.max(), d.min()]).tolist())
            else:
                C, mx, mn = 0, 0, 0
            self.C, self.max_nodes, self.min_nodes = C, mx, mn
            self._pair_ptr = binfo.ptr
            self._sorted = True
            return
        # any other cluster vector: PyG's consecutive_cluster (ids ranked by sorted unique value)
        if cluster.dim() != 1 or cluster.numel() != N:
            raise ValueError(f"cluster must be 1-D with {N} entries, got {tuple(cluster.shape)}")
        if N == 0:
            self.C, self.node_map = 0, cluster.new_zeros(0)
            self.order = cluster.new_zeros(0)
            self.rowptr = torch.zeros(1, dtype=torch.int32, device=dev)
            self._sorted = True
            self.ptr = torch.zeros(self.B + 1, dtype=torch.int64, device=dev)
            self.batch = cluster.new_zeros(0) if batch is not None else None
            self.max_nodes = self.min_nodes = 0
            return
        s, order = torch.sort(cluster.to(torch.int64), stable=True)
        new = torch.ones_like(s, dtype=torch.bool)
        new[1:] = s[1:] != s[:-1]
        rank = torch.cumsum(new, 0) - 1                      # consecutive id of every sorted position
        self.node_map = torch.empty_like(rank).scatter_(0, order, rank)
        self.order = order
        C_dev = rank[-1] + 1
        if batch is not None:
            pb = torch.full((N,), -1, dtype=torch.int64, device=dev).scatter_reduce_(0, self.node_map, batch, "amax")
            live = torch.arange(N, device=dev) < C_dev
            unsorted = ((pb[1:] < pb[:-1]) & live[1:]).any()
            counts = torch.zeros(max(self.B, 1), dtype=torch.int64, device=dev).index_add_(
                0, pb.clamp(min=0), live.to(torch.int64))[: self.B]
            if self.B > 0:
                stats = torch.stack([C_dev, unsorted.to(torch.int64), counts.max(), counts.min()])
            else:
                stats = torch.stack([C_dev, unsorted.to(torch.int64), C_dev * 0, C_dev * 0])
            C, uns, mx, mn = (int(v) for v in stats.tolist())
            self.batch = pb[:C]
            self._sorted = not uns
            if self._sorted:
                self.ptr = torch.cat([counts.new_zeros(1), counts.cumsum(0)])
                self.max_nodes, self.min_nodes = mx, mn
        else:
            C = int(C_dev.item())
            self._sorted = True
        self.C = C
        self.rowptr = torch.searchsorted(rank, torch.arange(C + 1, dtype=torch.int64, device=dev)).to(torch.int32)

    def pool(self, x: torch.Tensor, mode: str) -> torch.Tensor:
        if x.dim() != 2 or x.shape[0] != self.node_map.numel():
            raise ValueError(f"x must be [N, F] with N = {self.node_map.numel()}, got {tuple(x.shape)}")
        x = x if x.dtype == torch.float32 else x.float()
        if self.partner is not None:
            want_batch = self.batch is None and self.batch_in is not None
            out, pb = _PairPool.apply(x.contiguous(), self.partner, self.node_map, self._pair_ptr, self.C, mode,
                                      want_batch)
            if want_batch:
                self.batch = pb
            return out
        grouped = x.index_select(0, self.order)
        if mode == "max":
            out, _arg = _SegmentMaxRows.apply(grouped, self.rowptr, self.C)
            return out
        s = _SegmentSumRows.apply(grouped, self.rowptr, self.C)
        return s / self.rowptr.diff().to(s.dtype).unsqueeze(1)

    def pooled_batch(self) -> Optional[torch.Tensor]:
        """The pooled batch vector, registered (ptr, largest / smallest event) when it is sorted."""
        if self.batch_in is None:
            return None
        if self.batch is None:          # graclus path, nothing pooled yet
            self.batch = torch.repeat_interleave(torch.arange(self.B, device=self.ptr.device), self.ptr.diff(),
                                                 output_size=self.C)
        if self._sorted and self.ptr is not None:
            register_batch(self.batch, self.ptr, self.B, max_nodes=self.max_nodes, min_nodes=self.min_nodes)
        return self.batch


def _pool_x(cluster, x, batch, size, mode):
    if size is not None:
        raise NotImplementedError("max_pool_x / avg_pool_x: the dense size= form is not implemented")
    _native._require_device(cluster, x, batch)
    co = _Coarsening(cluster, batch, x.shape[0])
    out = co.pool(x, mode)
    return out, co.pooled_batch()


def max_pool_x(cluster: torch.Tensor, x: torch.Tensor, batch: Optional[torch.Tensor], batch_size: Optional[int] = None,
               size: Optional[int] = None) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """torch_geometric.nn.max_pool_x: (x pooled by channel-wise max over each cluster, pooled batch).  Differentiable
    through x (ties: the lower node index wins).  A graclus result pools its pairs directly; any other cluster vector
    is renumbered as PyG's consecutive_cluster does.  One host sync (the pooled size); the pooled batch comes back
    registered, so the next knn_graph on the pooled nodes needs none."""
    return _pool_x(cluster, x, batch, size, "max")


def avg_pool_x(cluster: torch.Tensor, x: torch.Tensor, batch: Optional[torch.Tensor], batch_size: Optional[int] = None,
               size: Optional[int] = None) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """torch_geometric.nn.avg_pool_x: like max_pool_x with the mean over each cluster."""
    return _pool_x(cluster, x, batch, size, "mean")


def pool_edge(node_map: torch.Tensor, edge_index: torch.Tensor, edge_attr: Optional[torch.Tensor], C: int):
    """PyG's pool_edge: map the endpoints to pooled rows, drop self loops, coalesce (edge_attr summed over duplicates).
    Plain torch bookkeeping plus the package's deterministic scatter_add."""
    ei = node_map[edge_index.reshape(-1)].view(2, -1)
    keep = ei[0] != ei[1]
    ei = ei[:, keep]
    attr = edge_attr[keep] if edge_attr is not None else None
    if ei.numel() == 0:
        return ei, attr
    key, inv = torch.unique(ei[0] * C + ei[1], sorted=True, return_inverse=True)
    ei = torch.stack([key // C, key % C], 0)
    if attr is not None:
        a2 = attr.reshape(attr.shape[0], -1).float()
        attr = scatter_add(a2, inv, dim=0, dim_size=key.numel()).view((key.numel(),) + tuple(attr.shape[1:]))
    return ei, attr


def _pool_data(cluster, data, transform, mode):
    x = getattr(data, "x", None)
    batch = getattr(data, "batch", None)
    N = x.shape[0] if x is not None else cluster.numel()
    _native._require_device(cluster, x, batch)
    co = _Coarsening(cluster, batch, N)
    out = copy.copy(data)
    if x is not None:
        out.x = co.pool(x, mode)
    pos = getattr(data, "pos", None)
    if pos is not None:
        out.pos = co.pool(pos, "mean")
    ei = getattr(data, "edge_index", None)
    if ei is not None:
        out.edge_index, out.edge_attr = pool_edge(co.node_map, ei, getattr(data, "edge_attr", None), co.C)
    out.batch = co.pooled_batch()
    if hasattr(data, "ptr") and co.ptr is not None and co._sorted:      # this package's Batch
        out.ptr = co.ptr
        if hasattr(data, "max_nodes"):
            out.max_nodes = co.max_nodes
        if hasattr(data, "min_nodes"):
            out.min_nodes = co.min_nodes
    if transform is not None:
        out = transform(out)
    return out


def max_pool(cluster: torch.Tensor, data, transform=None):
    """torch_geometric.nn.max_pool: a shallow copy of `data` with x max-pooled, pos mean-pooled, batch pooled and the
    edge index coarsened (pool_edge); a deepmetv2_amd Batch also gets its ptr / max_nodes / min_nodes updated."""
    return _pool_data(cluster, data, transform, "max")


def avg_pool(cluster: torch.Tensor, data, transform=None):
    """torch_geometric.nn.avg_pool: as max_pool with x mean-pooled."""
    return _pool_data(cluster, data, transform, "mean")


# ---------------------------------------------------------------------------------------------------------------
# global (per-event) readout
# ---------------------------------------------------------------------------------------------------------------
def _global_rowptr(x: torch.Tensor, batch: Optional[torch.Tensor], size: Optional[int]):
    _native._require_device(x, batch)
    if x.dim() != 2:
        raise ValueError(f"x must be [N, F], got {tuple(x.shape)}")
    N = x.shape[0]
    if batch is None:
        ptr, B = torch.tensor([0, N], dtype=torch.int64, device=x.device), 1
    else:
        info = batch_info(batch, N, x.device, size)
        ptr, B = info.ptr, info.num_events
    if size is not None and size > B:       # trailing empty events
        ptr = torch.cat([ptr, ptr[-1:].expand(size - B)])
        B = size
    return ptr.to(torch.int32), B, size


def _trim(out: torch.Tensor, size: Optional[int]) -> torch.Tensor:
    return out[:size] if size is not None else out


def global_max_pool(x: torch.Tensor, batch: Optional[torch.Tensor], size: Optional[int] = None) -> torch.Tensor:
    """torch_geometric.nn.global_max_pool: [B, F] channel-wise max per event (empty events give 0; batch=None: [1, F]).
    No host sync with a registered batch."""
    rowptr, B, size = _global_rowptr(x, batch, size)
    out, _arg = _SegmentMaxRows.apply(x, rowptr, B)
    return _trim(out, size)


def global_add_pool(x: torch.Tensor, batch: Optional[torch.Tensor], size: Optional[int] = None) -> torch.Tensor:
    """torch_geometric.nn.global_add_pool: [B, F] sums per event, in ascending node order."""
    rowptr, B, size = _global_rowptr(x, batch, size)
    return _trim(_SegmentSumRows.apply(x, rowptr, B), size)


def global_mean_pool(x: torch.Tensor, batch: Optional[torch.Tensor], size: Optional[int] = None) -> torch.Tensor:
    """torch_geometric.nn.global_mean_pool: [B, F] means per event (empty events give 0)."""
    rowptr, B, size = _global_rowptr(x, batch, size)
    s = _SegmentSumRows.apply(x, rowptr, B)
    return _trim(s / rowptr.diff().clamp(min=1).to(s.dtype).unsqueeze(1), size)

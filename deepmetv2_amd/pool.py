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
from .graph import (BatchInfo, _batch_registry, _deferred, _registry_get, _registry_put, batch_info, coalesced_tag, lookup_graph,
                    register_batch)
from .scatter import _SegmentMaxRows, _SegmentSumRows, scatter_add

# graclus output tensor -> partner[N] int32 (the pair-pooling path takes it; any other cluster vector is general)
_graclus_registry = {}
# voxel_grid / grid_cluster output tensor -> _VoxelRecord (same weak-reference registry, same caveat: an in-place write
# bumps the version and drops the entry; a write through .data or from a kernel does not)
_voxel_registry = {}

VOXEL_MAX_DIM = _native.VOXEL_MAX_DIM
VOXEL_MAX_CELLS = 2 ** 32 - 1           # cells of one event: the kernels keep the event-local cell id as a uint32
# Largest event whose result is registered for the one-launch coarsening.  Up to _native.SELECT_LDS_NODES nodes an event
# is ranked in LDS; above, ONE workgroup ranks it through L2 in the workspace, log2(n)^2 / 2 passes over 16 n bytes.  At
# 2^17 nodes that is 153 passes over 2 MiB, about where a global radix sort of the whole batch catches up: larger events
# (and N above this without a batch) take the generic branch.
VOXEL_MAX_EVENT = 1 << 17


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
# voxel clustering
# ---------------------------------------------------------------------------------------------------------------
class _VoxelRecord:
    """What voxel_grid / grid_cluster know about the tensor they returned: the event-local cell ids, the events, and --
    once somebody pooled it -- the coarsening (dmet_voxel_coarsen, run lazily: a caller who only wants the ids pays the
    cells launch alone)."""
    __slots__ = ("cell", "ptr", "B", "has_batch", "N", "result")

    def __init__(self, cell, ptr, B, has_batch, N):
        self.cell, self.ptr, self.B, self.has_batch, self.N = cell, ptr, B, has_batch, N
        self.result = None

    def coarsen(self):
        """(node_map, order, rowptr[C + 1], pooled batch[C], pooled ptr, C, largest, smallest pooled event); the first
        call makes the one host read (the record of three numbers)."""
        if self.result is None:
            node_map, order, rowptr, pb, ptr, record = _native._voxel_coarsen(self.cell, self.ptr)
            C, mx, mn = (int(v) for v in record.tolist())
            self.result = (node_map, order, rowptr[: C + 1], pb[:C], ptr, C, mx, mn)
        return self.result


def _voxel_spec(who: str, name: str, value, D: int):
    """size / start / end as the caller gave it -> a list of D host floats, or a [D] fp32 tensor left on its device."""
    if isinstance(value, torch.Tensor):
        if value.dim() > 1 or value.numel() not in (1, D):
            raise ValueError(f"{who}: {name} must be a number or hold {D} values (one per dimension of pos), got "
                             f"{tuple(value.shape)}")
        if value.device.type == "cpu":
            value = value.reshape(-1).tolist()
        else:
            return value.detach().to(torch.float32).reshape(-1).expand(D)
    if not hasattr(value, "__iter__"):
        return [float(value)] * D
    value = [float(v) for v in value]
    if len(value) == 1 and D > 1:
        value = value * D
    if len(value) != D:
        raise ValueError(f"{who}: {name} must be a number or hold {D} values (one per dimension of pos), got {len(value)}")
    return value


def _host_cells(size, start, end) -> int:
    """The cell count of one event from host numbers, by the kernel's rule: fp32 throughout, trunc(q) + 1 per dimension,
    1 for a NaN, infinite or negative q."""
    q = (torch.tensor(end, dtype=torch.float32) - torch.tensor(start, dtype=torch.float32)) / torch.tensor(size, dtype=torch.float32)
    cells = 1
    for v in q.tolist():
        cells *= int(v) + 1 if v >= 0.0 and v != float("inf") else 1
    return cells


def _voxel(who: str, pos: torch.Tensor, size, batch: Optional[torch.Tensor], start, end) -> torch.Tensor:
    if not isinstance(pos, torch.Tensor) or not pos.dtype.is_floating_point or pos.dtype == torch.float64:
        raise TypeError(f"{who}: pos must be a float32, bfloat16 or float16 tensor, got "
                        f"{pos.dtype if isinstance(pos, torch.Tensor) else type(pos).__name__}")
    if pos.dim() == 1:
        pos = pos.unsqueeze(1)
    if pos.dim() != 2 or not 1 <= pos.shape[1] <= VOXEL_MAX_DIM:
        raise ValueError(f"{who}: pos must be [N, D] or [N] with 1 <= D <= {VOXEL_MAX_DIM}, got {tuple(pos.shape)}")
    N, D = pos.shape
    spec = {"size": _voxel_spec(who, "size", size, D)}
    for name, value in (("start", start), ("end", end)):
        spec[name] = _voxel_spec(who, name, value, D) if value is not None else None
    if isinstance(spec["size"], list):
        s32 = torch.tensor(spec["size"], dtype=torch.float32)
        if not bool(((s32 > 0) & torch.isfinite(s32)).all()):
            raise ValueError(f"{who}: size must be positive and finite in fp32, got {spec['size']}")
    host_known = all(isinstance(v, list) for v in spec.values())
    if host_known:
        cells = _host_cells(spec["size"], spec["start"], spec["end"])
        if cells > VOXEL_MAX_CELLS:
            # B cells <= 2^63 - 1 then holds for every B <= 2^31 - 1, the largest event count the package takes
            raise ValueError(f"{who}: the grid has {cells} cells per event, more than 2^32 - 1")
    dev = _native._require_device(pos, batch, *[v for v in spec.values() if isinstance(v, torch.Tensor)])
    if N == 0:
        if batch is not None:
            batch_info(batch, N, dev)
        return torch.zeros(0, dtype=torch.int64, device=dev)
    check_batch = False
    if batch is not None:
        check_batch = _registry_get(_batch_registry, batch) is not None      # else batch_info reads and checks it here
        binfo = batch_info(batch, N, dev)
    else:
        binfo = BatchInfo(torch.arange(0, N + 1, N, dtype=torch.int64, device=dev), 1, N, N, N)      # [0, N], no copy
    posf = pos.detach().to(torch.float32).contiguous()

    def upload(rows):       # host numbers through pinned memory: a pageable copy would stall the launch thread
        return torch.tensor(rows, dtype=torch.float32).pin_memory().to(dev, non_blocking=True)

    if host_known:
        grid = upload([spec["size"], spec["start"], spec["end"]])
    else:
        rows = []
        for name, own in (("size", None), ("start", torch.amin), ("end", torch.amax)):
            v = spec[name]
            rows.append(own(posf, 0) if v is None else upload(v) if isinstance(v, list) else v)
        grid = torch.stack(rows)
    _deferred.poll()
    ids, cell, _nvox, flags = _native._voxel_cells(posf, grid, binfo.ptr, batch if check_batch else None)
    capturing = torch.cuda.is_current_stream_capturing()       # a captured graph cannot report: as _check_full_rows
    if not host_known and not capturing:
        _deferred.post(flags[0:1], f"{who}: the grid has more than 2^32 - 1 cells per event; its cell counts were cut and "
                                   "the ids clamped to them")
    if check_batch and not capturing:
        _deferred.post(flags[1:2], f"{who}: batch is not the sorted vector it was registered as; the ids follow the "
                                   "registered ptr")
    if binfo.max_nodes is not None and binfo.max_nodes <= VOXEL_MAX_EVENT:
        _registry_put(_voxel_registry, ids, _VoxelRecord(cell, binfo.ptr, binfo.num_events, batch is not None, N))
    return ids


def grid_cluster(pos: torch.Tensor, size, start=None, end=None) -> torch.Tensor:
    """torch_cluster.grid_cluster: the voxel of every point, int64 [N].  pos [N, D] or [N], 1 <= D <= 8, fp32 (bf16 /
    fp16 are upcast exactly; float64 is a TypeError); size / start / end a number, D numbers or a [D] tensor; start / end
    default to pos.min(0) / pos.max(0).  In fp32, one rounding for the subtraction and one for the division:

        nvox_d = trunc((end_d - start_d) / size_d) + 1,  c_d = trunc((pos_d - start_d) / size_d),
        id = sum_d c_d * prod_{d' < d} nvox_d'

    upstream's value bit for bit for finite pos inside [start, end].  Where upstream returns garbage: c_d is clamped to
    [0, nvox_d - 1], a NaN coordinate goes to cell 0, a non-finite or negative (end - start) / size gives nvox_d = 1.
    size <= 0 or non-finite, and more than 2^32 - 1 cells, are a ValueError when given as host numbers; a grid computed on
    the device (a device tensor, or start / end = None) that has too many cells is cut, its ids clamped, and a deferred
    check reports it (the next operator call or raise_deferred_errors()).  No host sync.  Not differentiable.
    The result is registered (events of up to 2^17 nodes): pooling it takes the one-launch coarsening."""
    return _voxel("grid_cluster", pos, size, None, start, end)


def voxel_grid(pos: torch.Tensor, size, batch: Optional[torch.Tensor] = None, start=None, end=None) -> torch.Tensor:
    """torch_geometric.nn.voxel_grid: grid_cluster with the batch id appended as one more coordinate of size 1, start 0
    and end B - 1, so id = cell + event * cells: the event is the most significant digit.  B and the events come from
    the registered batch (register_batch, a Batch, a pooled batch) without a host sync, with or without start / end; any
    other batch vector is read once (batch_info), where an unsorted one is a ValueError.  A registered batch that is not
    the sorted vector it was registered as is reported by a deferred check.  start / end = None are pos.min(0) /
    pos.max(0) over the whole batch, as upstream.  Rules, refusals and registration as grid_cluster."""
    return _voxel("voxel_grid", pos, size, batch, start, end)


def consecutive_cluster(src: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """torch_geometric.nn.pool.consecutive.consecutive_cluster: (node_map int64 [N], perm int64 [C]).  node_map[i] is
    the rank of src[i] among the sorted unique values; perm[c] is the HIGHEST node index of cluster c.  That is upstream's
    CPU result; upstream's GPU result is unspecified (a scatter with duplicate indices: whichever write lands last), this
    one is the same on every run.  A voxel_grid / grid_cluster result takes the one-launch coarsening; any other vector
    goes through torch.unique.  One host sync (C)."""
    _native._require_device(src)
    if src.dim() != 1:
        raise ValueError(f"consecutive_cluster: src must be 1-D, got {tuple(src.shape)}")
    N = src.numel()
    if N == 0:
        return torch.zeros(0, dtype=torch.int64, device=src.device), torch.zeros(0, dtype=torch.int64, device=src.device)
    vox = _registry_get(_voxel_registry, src)
    if vox is not None and vox.N == N:
        node_map, order, rowptr = vox.coarsen()[:3]
        return node_map, order.index_select(0, rowptr[1:].to(torch.int64) - 1)
    uniq, inv = torch.unique(src, sorted=True, return_inverse=True)
    perm = torch.full((uniq.numel(),), -1, dtype=torch.int64, device=src.device).scatter_reduce_(
        0, inv, torch.arange(N, dtype=torch.int64, device=src.device), "amax")
    return inv, perm


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
        vox = _registry_get(_voxel_registry, cluster)
        if vox is not None and vox.N == N and N > 0 and cluster.dim() == 1 and (
                vox.ptr is binfo.ptr if batch is not None else not vox.has_batch):
            # voxel_grid / grid_cluster ids over these very events: one ranking per event (dmet_voxel_coarsen) instead of
            # the global sort below; the same attributes, the same one host read
            self.node_map, self.order, self.rowptr, pb, ptr, self.C, mx, mn = vox.coarsen()
            self._sorted = True
            if batch is not None:
                self.batch, self.ptr, self.max_nodes, self.min_nodes = pb, ptr, mx, mn
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


def pool_edge(node_map: torch.Tensor, edge_index: torch.Tensor, edge_attr: Optional[torch.Tensor], C: int, *,
              self_loops: bool = False):
    """PyG's pool_edge: map the endpoints to pooled rows, drop self loops, coalesce (edge_attr summed over duplicates).
    Plain torch bookkeeping plus the package's deterministic scatter_add.  self_loops=True keeps the self loops, the
    edges inside a cluster among them: coalesce(node_map[edge_index]), what EdgePooling returns."""
    ei = node_map[edge_index.reshape(-1)].view(2, -1)
    attr = edge_attr
    if not self_loops:
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

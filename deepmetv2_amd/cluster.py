"""Graph builders and samplers with the torch_cluster signatures (`knn`, `knn_graph`, `radius`, `radius_graph`, `fps`,
`nearest`).

Reference call sites (relative to /root/reference): model/graph_met_network.py:63 and
model/dynamic_reduction_network.py:86,94 (knn_graph); train.py:48, evaluate.py:88, plt_weight.py:122
(radius_graph).  The kernels are in csrc/knn.hip, csrc/radius.hip and csrc/fps.hip; this file is argument checking and the int64 `edge_index` view.
"""
from __future__ import annotations

import math
import numbers
import os
import struct
from typing import Optional

import torch

from . import _native
from .graph import BipartiteTable, NeighborTable, _deferred, batch_info

MAX_K = 64  # DMET_MAX_K


def fp16_autocast() -> bool:
    """torch.autocast is on for the GPU with float16 (what torch.autocast("cuda") without a dtype gives)."""
    return torch.is_autocast_enabled() and torch.get_autocast_gpu_dtype() == torch.float16


def _check_x(x: torch.Tensor) -> torch.Tensor:
    # 16-bit features from autocast upstream: exact upcast, the graph is the one of x.float().  bf16 always; fp16 while
    # fp16 autocast is on (outside it an fp16 x stays an error, as it always was)
    if x.dtype == torch.bfloat16 or (x.dtype == torch.float16 and fp16_autocast()):
        x = x.float()
    if x.dim() == 1:
        x = x.view(-1, 1)
    if x.dim() != 2:
        raise ValueError(f"x must be [N, D], got {tuple(x.shape)}")
    if x.dtype != torch.float32:
        raise TypeError(f"x must be float32, got {x.dtype} (kNN distances are defined in fp32, rule R1)")
    return x


def knn_table(x: torch.Tensor, k: int, batch: Optional[torch.Tensor] = None, loop: bool = True,
              num_events: Optional[int] = None, dense=None, period=None) -> NeighborTable:
    """Fixed-width neighbour table for `x` (row i = the message sources of node i).  loop=False searches k+1
    and blanks j == i, exactly like upstream's `row != col` mask (a node whose k+1 nearest do not include itself,
    possible only with >= k+1 duplicates at lower index, keeps all k+1).  A bf16 `x`, or an fp16 one under fp16
    autocast, is upcast first, an exact conversion: the result is the kNN of x.float().

    period: None (torch_cluster's plain distance), or one entry per coordinate as in radius_table: None / 0 for a plain
    coordinate, or the circumference of a periodic one, e.g. [None, 2 * math.pi] for (eta, phi).  The periodic
    difference is min(|d|, L - |d|) in fp32 (include/dmet.h, dmet_knn_periodic_f32); up to 8 coordinates.  A periodic
    table with loop=True and k in (8, 16, 20, 32) carries the event-local ids, like a plain one, so the EdgeConvs take
    the same route over it."""
    x = _check_x(x)
    if not isinstance(k, int) or k < 1:
        raise ValueError(f"k must be a positive int, got {k!r}")
    kk = k if loop else k + 1
    if kk > MAX_K:
        raise ValueError(f"k={k} (searching {kk}) exceeds the supported maximum {MAX_K}")
    per = _check_period(period, x.shape[1])
    if per is not None and x.shape[1] > 8:
        raise ValueError(f"periodic coordinates are supported for up to 8 coordinates, x has {x.shape[1]}")
    info = batch_info(batch, x.shape[0], x.device, num_events)
    # the LDS gather kernel reads the table as event-local uint16 ids when the kNN kernels wrote them alongside
    # dense = (W, b, sliced_of(max_nodes)): DynamicEdgeConv asks the build to carry the node-level dense layer of its
    # fused form (table.pq = (P, Q, sliced), or None when the build could not)
    loc = None
    pq = None
    _native.knn_size_hint(info.min_nodes, info.max_nodes)    # what the loader knows about the event sizes (spent by the build below)
    if per is not None:    # D <= 8: never the dense-carrying build (32 features)
        nbr, dist, loc = _native.knn_periodic(x, info.ptr, kk, per, want_local=loop and kk in _native.LDS_GATHER_K)
    elif loop and kk in _native.LDS_GATHER_K and dense is not None and x.shape[1] == 32:
        W, b, sliced_of = dense
        nbr, dist, loc, pq = _native.knn_local_dense(x, info.ptr, kk, W, b, sliced_of(info.max_nodes))
    elif loop and kk in _native.LDS_GATHER_K:
        nbr, dist, loc = _native.knn_local(x, info.ptr, kk)
    else:
        nbr, dist = _native.knn(x, info.ptr, kk)
    # dense <=> no -1 entry anywhere.  Sizes alone cannot promise that (a NaN / inf query, or a node farther than the 1e10
    # squared-distance sentinel from every other node of its event, leaves a row short), so no table claims it.  What
    # sizes DO give is the expectation `full_rows`: self loops kept and every event >= kk nodes (batch_info, which counts
    # batch=None as one event, or register_batch(min_nodes=...)).  Only the [2,E] view of such a table is sized E = N kk
    # on the host, so the reference's call shape `conv(emb, knn_graph(emb, k, batch, loop=True))`
    # (graph_met_network.py:63) enqueues without a device->host sync; knn_graph / knn verify the expectation by a deferred
    # check (a short row appears as -1 in that view, and the next operator call raises).  The edge list the operators
    # consume (NeighborTable.edge_list) counts the valid slots: a short row is fewer edges there, never a -1 source.
    dense = False
    full_rows = bool(loop and info.min_nodes is not None and info.min_nodes >= kk and x.shape[0] > 0)
    if not loop:
        self_id = torch.arange(x.shape[0], dtype=torch.int32, device=x.device).view(-1, 1)
        nbr = torch.where(nbr == self_id, torch.full_like(nbr, -1), nbr)
    table = NeighborTable(nbr, info.ptr, dense=dense, dist=dist, max_nodes=info.max_nodes, nbr_local=loc,
                          full_rows=full_rows)
    table.pq = pq
    return table


def knn_graph(x: torch.Tensor, k: int, batch: Optional[torch.Tensor] = None, loop: bool = False,
              flow: str = "source_to_target", cosine: bool = False, num_workers: int = 1,
              batch_size: Optional[int] = None, period=None) -> torch.Tensor:
    """torch_cluster.knn_graph: edge_index[2,E] int64; [0] = neighbour j, [1] = centre i for
    flow='source_to_target'; edges grouped by ascending i, ascending (distance, j) inside a group.  period: periodic
    coordinates, see knn_table (None: torch_cluster's behaviour)."""
    if cosine:
        raise NotImplementedError("cosine=True is not on the DeepMETv2 hot path")
    if flow not in ("source_to_target", "target_to_source"):
        raise ValueError(f"flow must be 'source_to_target' or 'target_to_source', got {flow!r}")
    _deferred.poll()
    table = knn_table(x, k, batch, loop=loop, num_events=batch_size, period=period)
    _check_full_rows(table, x, "knn_graph")
    return table.edge_index(flow)


def _check_full_rows(table: NeighborTable, x: torch.Tensor, who: str) -> None:
    """The [2,E] view of a `full_rows` table is sized N k without asking the device: post the deferred check that every
    row did come out full."""
    if table.full_rows and x.is_cuda and not torch.cuda.is_current_stream_capturing():
        # rows are sorted by (d, j) with the empty slots last: the last column tells whether any row is short
        _deferred.post((table.nbr[:, -1].min() < 0).to(torch.int32),
                       f"{who}: a neighbour row came out short although every event holds at least k nodes (non-finite "
                       "coordinates, or candidates beyond the 1e10 sentinel distance): the [2,E] edge index handed out "
                       "for it carries -1 entries")


def knn(x: torch.Tensor, y: torch.Tensor, k: int, batch_x: Optional[torch.Tensor] = None,
        batch_y: Optional[torch.Tensor] = None, cosine: bool = False, num_workers: int = 1,
        batch_size: Optional[int] = None, period=None) -> torch.Tensor:
    """torch_cluster.knn: for every row of `y` (a query) the k nearest rows of `x` (the candidates) of the same event.
    Returns int64 [2,E]: row 0 = index into y, row 1 = index into x; grouped by ascending query, ascending (distance, x
    index) inside a query.  period: periodic coordinates, see knn_table.

    The self-query form (`y is x and batch_y is batch_x`, what DynamicEdgeConv uses) is knn_table(x, k, batch_x,
    loop=True) as it always was.  Any other call is the two-set build (knn_xy_table): separate index spaces, so no self
    to exclude (a point present in both sets finds its twin at distance 0), a short row for a query whose event holds
    fewer than k admissible candidates, no edge for a query event without candidates.  Its [2,E] result is sized by one
    device-to-host read of the edge count (upstream returns an exact-size tensor too); knn_xy_table has none."""
    if cosine:
        raise NotImplementedError("cosine=True is not on the DeepMETv2 hot path")
    if y is x and batch_y is batch_x:
        table = knn_table(x, k, batch_x, loop=True, num_events=batch_size, period=period)
        _check_full_rows(table, x, "knn")
        return table.edge_index("target_to_source")
    return knn_xy_table(x, y, k, batch_x, batch_y, batch_size=batch_size, period=period).edge_index()


def _xy_events(x: torch.Tensor, y: torch.Tensor, batch_x, batch_y, batch_size: Optional[int]):
    """(ptr_x, ptr_y) over the same B events for the two-set builders: both batch vectors or neither; each sorted,
    checked and cached like `batch` in knn_graph (graph.batch_info); B = the larger event count of the two, or
    batch_size."""
    if (batch_x is None) != (batch_y is None):
        raise ValueError("batch_x and batch_y must be given together (or neither: one event)")
    if x.device != y.device:
        raise RuntimeError("deepmetv2_amd: x and y must live on the same device")
    ix = batch_info(batch_x, x.shape[0], x.device, batch_size)
    iy = batch_info(batch_y, y.shape[0], y.device, batch_size)
    B = max(ix.num_events, iy.num_events)

    def upto(ptr):      # trailing events without nodes
        return ptr if ptr.numel() == B + 1 else torch.cat([ptr, ptr[-1:].expand(B + 1 - ptr.numel())])
    return upto(ix.ptr), upto(iy.ptr)


def _check_xy(x: torch.Tensor, y: torch.Tensor, period, max_dim: int, who: str):
    x, y = _check_x(x), _check_x(y)
    if x.shape[1] != y.shape[1]:
        raise ValueError(f"x has {x.shape[1]} coordinates, y has {y.shape[1]}")
    per = _check_period(period, x.shape[1])
    if x.shape[1] > max_dim:
        raise ValueError(f"{who} supports up to {max_dim} coordinates, x has {x.shape[1]}")
    if per is not None and x.shape[1] > 8:
        raise ValueError(f"periodic coordinates are supported for up to 8 coordinates, x has {x.shape[1]}")
    return x, y, per


def knn_xy_table(x: torch.Tensor, y: torch.Tensor, k: int, batch_x: Optional[torch.Tensor] = None,
                 batch_y: Optional[torch.Tensor] = None, batch_size: Optional[int] = None, period=None) -> BipartiteTable:
    """The two-set kNN as a fixed-width table, without sizing E on the host: nbr [Ny, k] int32 ids into x (-1 in empty
    slots), dist [Ny, k] fp32 (1e10 there).  With both batch vectors registered (register_batch) the call never
    synchronises.  Contract: include/dmet.h, dmet_knn_xy_f32 (the fp32 chain of knn_table, `period` included; k <= 64,
    up to 64 coordinates, 8 with a period)."""
    x, y, per = _check_xy(x, y, period, 64, "knn")
    if not isinstance(k, int) or isinstance(k, bool) or k < 1:
        raise ValueError(f"k must be a positive int, got {k!r}")
    if k > MAX_K:
        raise ValueError(f"k={k} exceeds the supported maximum {MAX_K}")
    ptr_x, ptr_y = _xy_events(x, y, batch_x, batch_y, batch_size)
    nbr, dist = _native.knn_xy(x, ptr_x, y, ptr_y, k, per)
    return BipartiteTable(nbr, ptr_x, ptr_y, x.shape[0], dist=dist)


def radius_xy_table(x: torch.Tensor, y: torch.Tensor, r: float, batch_x: Optional[torch.Tensor] = None,
                    batch_y: Optional[torch.Tensor] = None, max_num_neighbors: int = 32,
                    batch_size: Optional[int] = None, period=None, pad: bool = False) -> BipartiteTable:
    """The two-set radius search as a fixed-width table: nbr [Ny, max_num_neighbors] int32 ids into x, cnt [Ny] int32;
    row i holds the first cnt[i] rows of x (ascending id) of the query's event with squared distance < fp32(r) * fp32(r).
    Slots beyond cnt[i] are unwritten unless pad=True (-1).  No host sync once both batch vectors are registered.
    Contract: include/dmet.h, dmet_radius_xy_f32 (up to 8 coordinates)."""
    x, y, per = _check_xy(x, y, period, 8, "radius")
    if not isinstance(max_num_neighbors, int) or isinstance(max_num_neighbors, bool) or max_num_neighbors < 1:
        raise ValueError(f"max_num_neighbors must be a positive int, got {max_num_neighbors!r}")
    ptr_x, ptr_y = _xy_events(x, y, batch_x, batch_y, batch_size)
    nbr, cnt = _native.radius_xy(x, ptr_x, y, ptr_y, r, max_num_neighbors, per, pad)
    return BipartiteTable(nbr, ptr_x, ptr_y, x.shape[0], cnt=cnt)


def radius(x: torch.Tensor, y: torch.Tensor, r: float, batch_x: Optional[torch.Tensor] = None,
           batch_y: Optional[torch.Tensor] = None, max_num_neighbors: int = 32, num_workers: int = 1,
           batch_size: Optional[int] = None, period=None) -> torch.Tensor:
    """torch_cluster.radius: for every row of `y` all rows of `x` of the same event within r (squared distance
    < fp32(r) * fp32(r)), the first max_num_neighbors hits in ascending x index (radius_graph's rule).  int64 [2,E]: row 0 =
    index into y, row 1 = index into x.  period: periodic coordinates, see radius_table.  Sized by one device-to-host
    read of the edge count; radius_xy_table has none."""
    return radius_xy_table(x, y, r, batch_x, batch_y, max_num_neighbors, batch_size, period).edge_index()


def _check_period(period, D: int) -> Optional[list]:
    """radius_graph's and knn_graph's `period`: None, or D entries each None / 0 (a plain coordinate) or a positive finite number (the
    circumference of a periodic coordinate, rounded to fp32).  Returns the D fp32-representable floats, or None when no
    coordinate is periodic (the plain build then runs exactly as without the keyword)."""
    if period is None:
        return None
    if isinstance(period, (str, bytes)) or not isinstance(period, (list, tuple)):
        raise TypeError(f"period must be None or a list / tuple of {D} entries, got {type(period).__name__}")
    if len(period) != D:
        raise ValueError(f"period has {len(period)} entries, x has {D} coordinates")
    out = []
    for c, p in enumerate(period):
        if p is None:
            out.append(0.0)
            continue
        if isinstance(p, bool) or not isinstance(p, numbers.Real):
            raise TypeError(f"period[{c}] must be None, 0 or a positive number, got {p!r}")
        v = float(p)
        if v == 0.0:
            out.append(0.0)
            continue
        try:
            v32 = struct.unpack("f", struct.pack("f", v))[0] if math.isfinite(v) else v
        except OverflowError:       # beyond the fp32 range
            v32 = math.inf
        if not (v > 0.0 and math.isfinite(v32) and v32 > 0.0):
            raise ValueError(f"period[{c}]={p!r} is not 0 or a positive finite number (in fp32)")
        out.append(v32)
    return out if any(v > 0.0 for v in out) else None


def radius_table(x: torch.Tensor, r: float, batch: Optional[torch.Tensor] = None, loop: bool = False,
                 max_num_neighbors: int = 32, num_events: Optional[int] = None, int32_rows: Optional[bool] = None,
                 period=None) -> NeighborTable:
    """The radius graph as a NeighborTable.  int32_rows=False: only the event-local uint16 rows are written (what the
    fused EdgeConv reads on events of at most 65534 nodes); `.nbr` is expanded from them if somebody asks.  None: False
    when the caller registered the batch's largest event (register_batch(max_nodes=) <= 65534), else True.

    period: None (torch_cluster's plain distance), or one entry per coordinate: None / 0 for a plain coordinate, or the
    circumference of a periodic one, e.g. [None, 2 * math.pi] for (eta, phi) -- phi = +3.1 and -3.1 are then 0.08
    apart, not 6.2.  The periodic difference is min(|d|, L - |d|) in fp32 (include/dmet.h), the circular distance as
    long as every value of a periodic coordinate lies within one period (atan2 output does).  The build is windowed on
    coordinate 0: put a periodic coordinate first ([phi, eta]) and the slower all-pairs build runs."""
    x = _check_x(x)
    if x.shape[1] > 8:
        raise ValueError("radius_graph supports up to 8 coordinates")
    per = _check_period(period, x.shape[1])
    # upstream's loop=False: search max_num_neighbors + 1 and drop the node itself (done inside the kernel)
    m = max_num_neighbors if loop else max_num_neighbors + 1
    info = batch_info(batch, x.shape[0], x.device, num_events)
    # no -1 fill of the unused slots: every consumer of a table with `cnt` goes by cnt
    if int32_rows is None:
        int32_rows = not (info.max_nodes is not None and info.max_nodes <= 65534
                          and os.environ.get("DMET_RADIUS_INT32", "lazy") == "lazy")
    # a plain build is called exactly as it is without the keyword (stand-ins of _native.radius need not know `period`)
    periodic = {} if per is None else {"period": per}
    nbr, _cnt, rows16 = _native.radius(x, info.ptr, r, m, skip_self=not loop, pad=False, local=True, int32_rows=int32_rows,
                                       **periodic)
    # with self loops every node finds at least itself (the cap counts hits in index order, but a full row is not empty)
    return NeighborTable(nbr, info.ptr, dense=False, max_nodes=info.max_nodes, cnt=_cnt, nonempty=bool(loop),
                         rows16=rows16, shape=(x.shape[0], m))


def radius_graph(x: torch.Tensor, r: float, batch: Optional[torch.Tensor] = None, loop: bool = False,
                 max_num_neighbors: int = 32, flow: str = "source_to_target", num_workers: int = 1,
                 batch_size: Optional[int] = None, period=None) -> torch.Tensor:
    """torch_cluster.radius_graph (train.py:48 passes r=0.4, loop=True, max_num_neighbors=255).  period: periodic
    coordinates, see radius_table (None: torch_cluster's behaviour)."""
    if flow not in ("source_to_target", "target_to_source"):
        raise ValueError(f"flow must be 'source_to_target' or 'target_to_source', got {flow!r}")
    # the [2,E] view is cut from the int32 table: have the build write it (radius_table alone leaves it out when it can)
    return radius_table(x, r, batch, loop, max_num_neighbors, batch_size, int32_rows=True,
                        period=period).edge_index(flow)


def _fp32(v: float) -> float:
    return struct.unpack("f", struct.pack("f", v))[0]


def fps(src: torch.Tensor, batch: Optional[torch.Tensor] = None, ratio=0.5, random_start: bool = True,
        batch_size: Optional[int] = None, ptr: Optional[torch.Tensor] = None) -> torch.Tensor:
    """torch_cluster.fps: farthest point sampling.  int64 [M] global node ids, grouped by event (batch[idx] is sorted); event
    b contributes m_b = ceil(fp32(n_b) * fp32(ratio_b)) of its n_b nodes: the start node, then again and again the node
    farthest (rule R1's fp32 squared distance) from everything picked so far, ties to the lowest index (include/dmet.h,
    dmet_fps_f32; kernel: csrc/fps.hip).  Not differentiable.

    ratio: a float in (0, 1], or a tensor with one entry or one per event (its values are the caller's: a negative entry
    samples nothing).  ptr: int64 [B+1] event offsets; when given, `batch` is ignored, as upstream does.
    random_start=True draws every event's start on the device from torch's generator (floor(rand * n_b), clamped);
    False starts at the event's first node, and the result is then a function of (src, events, ratio) alone.

    The [M] result is sized by one device-to-host read of the sample count (upstream returns an exact-size tensor too),
    unless `batch` is registered with equal event sizes (register_batch(min_nodes=n, max_nodes=n)) and `ratio` is a float:
    then M = B * ceil(fp32(n) * fp32(ratio)) is formed on the host and the call never synchronises."""
    src = _check_x(src)
    float_ratio = not torch.is_tensor(ratio)
    if float_ratio:
        if isinstance(ratio, bool) or not isinstance(ratio, numbers.Real) or not 0.0 < float(ratio) <= 1.0:
            raise ValueError(f"ratio must be a float in (0, 1] or a tensor, got {ratio!r}")
        ratio = float(ratio)
    elif ratio.dim() > 1 or not ratio.is_floating_point():
        raise ValueError(f"a tensor ratio must be a floating-point scalar or vector, got {ratio.dtype} {tuple(ratio.shape)}")
    if ptr is not None and (not torch.is_tensor(ptr) or ptr.dtype != torch.int64 or ptr.dim() != 1 or ptr.numel() < 1):
        raise TypeError("ptr must be a 1-D int64 (torch.long) tensor of B + 1 event offsets")
    if not src.is_cuda:
        raise RuntimeError("deepmetv2_amd.fps: src is not on a GPU. The HIP kernel is the only implementation (no CPU "
                           "fallback); move the inputs to a ROCm device.")
    _deferred.poll()
    dev, N = src.device, src.shape[0]
    n_equal = None
    if ptr is not None:
        if ptr.device != dev:
            raise RuntimeError("deepmetv2_amd: all tensors must live on the same device")
        B = ptr.numel() - 1
    else:
        info = batch_info(batch, N, dev, batch_size)
        ptr, B = info.ptr, info.num_events
        if info.min_nodes is not None and info.min_nodes == info.max_nodes:
            n_equal = info.max_nodes
    if N == 0 or B == 0:
        return torch.empty(0, dtype=torch.int64, device=dev)
    deg = ptr[1:] - ptr[:-1]
    degf = deg.to(torch.float32)
    if float_ratio:
        m = torch.ceil(degf * ratio)
    else:
        if ratio.numel() not in (1, B):
            raise ValueError(f"a tensor ratio must hold 1 or {B} (one per event) entries, got {ratio.numel()}")
        m = torch.ceil(degf * ratio.to(device=dev, dtype=torch.float32).reshape(-1)).clamp_(min=0)
    out_ptr = torch.nn.functional.pad(torch.cumsum(m.to(torch.int64), 0), (1, 0))
    if float_ratio and n_equal is not None:
        M = B * math.ceil(_fp32(_fp32(float(n_equal)) * _fp32(ratio)))
    else:
        M = int(out_ptr[-1].item())
    start = None
    if random_start:
        r = torch.rand(B, device=dev)
        start = torch.minimum((r * degf).floor().to(torch.int64), deg - 1).clamp_(min=0)
    return _native.fps(src, ptr, out_ptr, start, M)


def nearest(x: torch.Tensor, y: torch.Tensor, batch_x: Optional[torch.Tensor] = None,
            batch_y: Optional[torch.Tensor] = None) -> torch.Tensor:
    """torch_cluster.nearest: for every row of `x` the row of `y` of the same event at the smallest squared distance (rule
    R1's fp32 chain), ties to the lower y index.  int64 [Nx].  It is the k = 1 column of knn_xy_table(y, x, 1, batch_y,
    batch_x): no host sync once both batch vectors are registered.  A row of x whose event holds no row of y (or only
    rows beyond the 1e10 sentinel distance, or non-finite ones) has no answer: its entry is -1 and a deferred check makes
    the next operator call (or raise_deferred_errors()) raise."""
    _deferred.poll()
    nbr = knn_xy_table(y, x, 1, batch_y, batch_x).nbr[:, 0]
    if nbr.numel() and nbr.is_cuda and not torch.cuda.is_current_stream_capturing():
        _deferred.post((nbr.min() < 0).to(torch.int32),
                       "nearest: a row of x found no row of y in its event (an event without y rows, non-finite "
                       "coordinates, or every candidate beyond the 1e10 sentinel distance): its entry is -1")
    return nbr.to(torch.int64)

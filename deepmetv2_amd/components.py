"""Connected components and DBSCAN of every event of a batch: `connected_components`, `largest_connected_components`,
`dbscan_graph`, `dbscan`.

The kernel is in csrc/components.hip (include/dmet.h, section "Components and DBSCAN"): a union-find over the entries of
one event, one workgroup per event, every event of the batch in one launch, integer atomics only -- the labels are a
function of the graph alone.  This file is argument checking, the graph forms and the node-level torch work around the
launch.  Nothing here is differentiable and nothing is an autograd Function.  The references the tests hold it to are
scipy.sparse.csgraph.connected_components and sklearn.cluster.DBSCAN.
"""
from __future__ import annotations

import math
import numbers
from typing import Optional

import torch

from . import _native
from .graph import EdgeList, NeighborTable, _deferred, batch_info, edge_list_from_edge_index

__all__ = ["connected_components", "largest_connected_components", "dbscan_graph", "dbscan"]


class _Operands:
    """A graph as dmet_components_i32 reads it: `kw` = the table or list operands of _native._components, N, the events'
    ptr, `perm` = the caller-order id of every grouped position (a [2, E] tensor that had to be grouped; None else)."""
    __slots__ = ("kw", "N", "ptr", "perm")


def _int_arg(v, name: str, who: str, low: int) -> int:
    if isinstance(v, bool) or not isinstance(v, numbers.Integral) or v < low:
        raise ValueError(f"{who}: {name} must be an int >= {low}, got {v!r}")
    return int(v)


def _check_graph(graph, who: str) -> tuple:
    """Everything about `graph` the host can tell without the device; returns the shape of an edge mask over it."""
    if isinstance(graph, NeighborTable):
        return (graph.num_nodes, graph.k)
    if isinstance(graph, EdgeList):
        return (graph.num_edges,)
    if not torch.is_tensor(graph):
        raise TypeError(f"{who}: the graph must be a NeighborTable, an EdgeList or an int64 [2, E] tensor, got "
                        f"{type(graph).__name__}")
    if graph.dim() != 2 or graph.shape[0] != 2:
        raise ValueError(f"{who}: edge_index must be an int64 [2, E] tensor, got {tuple(graph.shape)}")
    if graph.dtype != torch.int64:
        raise TypeError(f"{who}: edge_index must be int64 (torch.long), got {graph.dtype}")
    return (graph.shape[1],)


def _check_events(batch, ptr, who: str) -> None:
    if ptr is not None and (not torch.is_tensor(ptr) or ptr.dtype != torch.int64 or ptr.dim() != 1 or ptr.numel() < 1):
        raise TypeError(f"{who}: ptr must be a 1-D int64 (torch.long) tensor of B + 1 event offsets")
    if batch is not None and (not torch.is_tensor(batch) or batch.dim() != 1):
        raise ValueError(f"{who}: batch must be a 1-D int64 tensor of one event per node")


def _check_mask(mask, name: str, who: str) -> None:
    if mask is not None and (not torch.is_tensor(mask) or mask.dtype != torch.bool):
        raise TypeError(f"{who}: {name} must be a bool tensor, got "
                        f"{mask.dtype if torch.is_tensor(mask) else type(mask).__name__}")


def _operands(graph, num_nodes: Optional[int], batch, ptr, who: str) -> _Operands:
    """The device side of the graph forms.  A table is read in place, by its counts where it has them: no edge list, no
    host read.  A [2, E] tensor is grouped by target (edge_list_from_edge_index: a stable sort and one host read, which
    also checks the ids)."""
    op = _Operands()
    if isinstance(graph, NeighborTable):
        graph.join()
        N = graph.num_nodes
        op.kw = dict(nbr=graph.nbr, cnt=graph.cnt)
        op.perm = None
        dev = graph.nbr.device
    elif isinstance(graph, EdgeList):
        N = graph.num_nodes
        op.kw = dict(rowptr=graph.rowptr, src=graph.src, tgt=graph.tgt)
        op.perm = None
        dev = graph.rowptr.device
    else:
        dev = _native._require_device(graph, batch, ptr)
        if num_nodes is not None:
            N = int(num_nodes)
        elif batch is not None:
            N = batch.numel()
        else:
            N = int(graph.max().item()) + 1 if graph.numel() else 0      # one host sync, as upstream
        edges = edge_list_from_edge_index(graph, N, "source_to_target")
        op.kw = dict(rowptr=edges.rowptr, src=edges.src, tgt=edges.tgt)
        op.perm = edges.perm
    if num_nodes is not None and int(num_nodes) != N:
        raise ValueError(f"{who}: num_nodes={num_nodes}, the graph has {N} nodes")
    if batch is not None and batch.numel() != N:
        raise ValueError(f"{who}: batch has {batch.numel()} entries, the graph has {N} nodes")
    _native._require_device(batch, ptr, *[v for v in op.kw.values() if v is not None])
    if ptr is None:
        if batch is None and isinstance(graph, NeighborTable) and graph.ptr is not None:
            ptr = graph.ptr             # a table carries the events it was built over
        else:
            ptr = batch_info(batch, N, dev).ptr
    op.N, op.ptr = N, ptr
    return op


def _post(flags: torch.Tensor, who: str, N: int, full_message: Optional[str] = None) -> None:
    if not flags.is_cuda or torch.cuda.is_current_stream_capturing():       # a captured graph cannot report
        return
    _deferred.post(flags[0:1], f"{who}: a graph entry has an end outside [0, {N}): it joined nothing")
    _deferred.post(flags[1:2], f"{who}: a graph entry joins nodes of two events: it joined nothing")
    _deferred.post(flags[2:3], f"{who}: the union-find reached a loop bound (a defect of the kernel): the labels are not "
                               "to be trusted")
    if full_message is not None:
        _deferred.post(flags[3:4], full_message)


def connected_components(edge_index, num_nodes: Optional[int] = None, batch: Optional[torch.Tensor] = None, *,
                         ptr: Optional[torch.Tensor] = None, edge_mask: Optional[torch.Tensor] = None,
                         node_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """labels, int64 [N]: labels[i] = the smallest node id of the (weakly) connected component of node i
    (include/dmet.h, "Components and DBSCAN").  Canonical -- the same for every order of the entries and every run -- and
    a cluster vector as `consecutive_cluster`, `max_pool`, `avg_pool` and `max_pool_x` take it.
    scipy.sparse.csgraph.connected_components(connection='weak') gives the same partition.

    edge_index: a -1-padded `NeighborTable`; a counted one (`radius_table`: walked by its counts, no edge list, no host
    read); an `EdgeList`; or an int64 [2, E] tensor in any order (grouped by target with one host read, where an id
    outside [0, N) is a ValueError).  An entry joins its two ends whichever way round it is listed; duplicates and self
    entries are harmless.  N = the table's / list's node count; for a tensor num_nodes, else batch.numel(), else the
    largest id + 1 (one more host read).
    batch / ptr: the events, one workgroup each (ptr: int64 [B + 1] offsets, taken on trust; neither: a table's own events,
    else one event).  An entry with an end outside [0, N), or with its ends in two events, joins nothing and is reported
    by a deferred check (the next operator call or raise_deferred_errors()).
    node_mask: bool [N]; a node with False gets -1 and its entries join nothing.
    edge_mask: bool, one value per position -- [N, k] for a table (the value of an empty slot is never read), [E] in
    grouped order for an EdgeList, [E] in the order of edge_index for a tensor -- an entry with False joins nothing: the
    "score > threshold" case, without a filtered edge index.
    One launch.  Not differentiable."""
    who = "connected_components"
    mask_shape = _check_graph(edge_index, who)
    _check_events(batch, ptr, who)
    _check_mask(edge_mask, "edge_mask", who)
    _check_mask(node_mask, "node_mask", who)
    if num_nodes is not None:
        _int_arg(num_nodes, "num_nodes", who, 0)
    if edge_mask is not None and tuple(edge_mask.shape) != mask_shape:
        raise ValueError(f"{who}: edge_mask must be {list(mask_shape)}, one value per position, got "
                         f"{list(edge_mask.shape)}")
    if node_mask is not None and node_mask.dim() != 1:
        raise ValueError(f"{who}: node_mask must be [N], one value per node, got {list(node_mask.shape)}")
    op = _operands(edge_index, num_nodes, batch, ptr, who)
    if edge_mask is not None and op.perm is not None:
        edge_mask = edge_mask.index_select(0, op.perm.long())
    if node_mask is not None and tuple(node_mask.shape) != (op.N,):
        raise ValueError(f"{who}: node_mask must be [{op.N}], got {list(node_mask.shape)}")
    _deferred.poll()
    labels, _core, _ncl, flags = _native._components(op.ptr, op.N, edge_mask=edge_mask, node_mask=node_mask, **op.kw)
    _post(flags, who, op.N)
    return labels


def _dbscan(op: _Operands, min_samples: int, count_self: bool, return_core: bool, who: str,
            full_message: Optional[str] = None):
    _deferred.poll()
    local, core, ncl, flags = _native._components(op.ptr, op.N, min_samples=min_samples, count_self=count_self, **op.kw)
    _post(flags, who, op.N, full_message)
    if ncl.numel() > 1:
        # batch-wide numbers: the clusters of the earlier events first (no host read: the sizes stay on the device)
        first = torch.cumsum(ncl, 0) - ncl
        per_node = torch.repeat_interleave(first, op.ptr.diff(), output_size=op.N)
        labels = torch.where(local >= 0, local + per_node, local)
    else:
        labels = local
    return (labels, core) if return_core else labels


def dbscan_graph(graph, min_samples: int, batch: Optional[torch.Tensor] = None, *, ptr: Optional[torch.Tensor] = None,
                 count_self: bool = False, return_core: bool = False):
    """DBSCAN over a given neighbourhood graph: labels, int64 [N] (-1 = noise); with return_core=True (labels, core), core
    the bool [N] mask of the core samples (sklearn's `core_sample_indices_`).

    graph: as `connected_components` takes it; row i (the entries with target i) is the neighbourhood of node i.
    n_i = the entries of row i, plus 1 with count_self -- the caller's statement that rows list no self entry.  Node i is
    core when n_i >= min_samples.  Core nodes joined by an entry form clusters, the components of the core-core
    subgraph.  A node that is not core takes the cluster of the core node in its own row whose cluster has the smallest
    root (= smallest core id); with no core node in its row it is noise.  Clusters are numbered 0, 1, ... over the whole
    batch in ascending root id: event by event, and inside an event in sklearn's discovery order, so event b's
    sklearn labels are these minus the number of clusters in earlier events.
    The graph is taken as SYMMETRIC, as a radius graph is: the border rule reads a node's own row only, so an entry
    (i, j) without its mirror (j, i) does not make j a border node of i's cluster.  On a symmetric graph the labels and
    the core mask equal sklearn.cluster.DBSCAN(metric='precomputed') on the same entries.
    batch / ptr and the deferred checks: as `connected_components`.  One launch, a cumsum over the events and an add per
    node; no host read for a table or an EdgeList with a registered batch.  Not differentiable."""
    who = "dbscan_graph"
    _check_graph(graph, who)
    _check_events(batch, ptr, who)
    min_samples = _int_arg(min_samples, "min_samples", who, 1)
    op = _operands(graph, None, batch, ptr, who)
    return _dbscan(op, min_samples, bool(count_self), bool(return_core), who)


def dbscan(pos: torch.Tensor, eps: float, min_samples: int = 5, batch: Optional[torch.Tensor] = None, *,
           max_num_neighbors: int = 64, period=None, return_core: bool = False):
    """sklearn.cluster.DBSCAN(eps, min_samples) of every event of pos [N, D]: labels int64 [N] (-1 = noise), numbered over
    the batch as `dbscan_graph` numbers them; return_core=True adds the bool core mask.

    Builds radius_table(pos, eps, batch, loop=True, max_num_neighbors=max_num_neighbors + 1, period=period) -- a node
    counts itself, as in sklearn -- and runs `dbscan_graph`'s kernel over it by its counts.  period: periodic
    coordinates, e.g. [None, 2 * math.pi] for (eta, phi) (see radius_table).
    min_samples <= max_num_neighbors is required (ValueError).  A row that fills all max_num_neighbors + 1 slots has more
    than max_num_neighbors points within eps and may have been cut: the kernel counts such rows and a deferred error
    names `max_num_neighbors` (the next operator call or raise_deferred_errors()).  The labels are exact whenever no
    error is posted.  No host sync with a registered batch.
    Deviation from sklearn: the neighbourhood is radius_graph's -- the squared distance in fp32 and strictly below
    eps^2 -- where sklearn compares the float64 distance with <=."""
    who = "dbscan"
    if not torch.is_tensor(pos) or pos.dim() != 2 or not pos.is_floating_point():
        raise ValueError(f"{who}: pos must be a floating-point [N, D] tensor")
    if isinstance(eps, bool) or not isinstance(eps, numbers.Real) or not (math.isfinite(eps) and eps > 0):
        raise ValueError(f"{who}: eps must be a positive finite number, got {eps!r}")
    min_samples = _int_arg(min_samples, "min_samples", who, 1)
    max_num_neighbors = _int_arg(max_num_neighbors, "max_num_neighbors", who, 1)
    if min_samples > max_num_neighbors:
        raise ValueError(f"{who}: min_samples={min_samples} needs max_num_neighbors >= {min_samples}, got "
                         f"{max_num_neighbors} (a core test on a cut row would be wrong)")
    _check_events(batch, None, who)
    from .cluster import radius_table       # cluster.py imports graph.py only; kept local to the one user
    table = radius_table(pos, float(eps), batch, loop=True, max_num_neighbors=max_num_neighbors + 1, int32_rows=True,
                         period=period)
    op = _operands(table, None, None, table.ptr, who)
    return _dbscan(op, min_samples, False, bool(return_core), who,
                   f"{who}: a node has more than max_num_neighbors={max_num_neighbors} points within eps: its row may be "
                   "cut and the labels are not exact; raise max_num_neighbors")


def largest_connected_components(edge_index, num_nodes: Optional[int] = None, batch: Optional[torch.Tensor] = None,
                                 num_components: int = 1, *, ptr: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The bool [N] mask of the nodes in the `num_components` largest connected components of every event; size ties go to
    the component with the smaller root id (its smallest node).  torch_geometric.transforms.LargestConnectedComponents
    per event, without the trip through scipy on the host.  An event with fewer components keeps all of them.

    Node-level torch work over `connected_components`' labels: the component sizes summed at the roots and this
    package's per-event `topk` over them (descending size, ties to the lower index).  Sizes are ranked as fp32, exact up
    to 2^24 nodes (ValueError beyond).  Host reads: those of `topk` (none with a registered batch whose smallest event
    holds num_components nodes) and of `connected_components`."""
    who = "largest_connected_components"
    num_components = _int_arg(num_components, "num_components", who, 1)
    labels = connected_components(edge_index, num_nodes, batch, ptr=ptr)
    N, dev = labels.numel(), labels.device
    if N == 0:
        return torch.zeros(0, dtype=torch.bool, device=dev)
    if N > 1 << 24:
        raise ValueError(f"{who}: {N} nodes; component sizes are ranked as fp32, exact up to 2^24")
    from .select import topk
    # the size of a component at its root, 0 elsewhere (scatter_add_: bincount reads the largest label back)
    size = torch.zeros(N, dtype=torch.int64, device=dev).scatter_add_(0, labels, torch.ones_like(labels))
    if ptr is None and batch is None and isinstance(edge_index, NeighborTable):
        ptr = edge_index.ptr
    best = topk(size.to(torch.float32), num_components, batch, ptr=ptr)
    keep = torch.zeros(N, dtype=torch.bool, device=dev)
    keep[best] = size[best] > 0                                      # an event with fewer components: no root, not kept
    return keep[labels]

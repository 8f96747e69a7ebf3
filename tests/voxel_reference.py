"""Plain torch (CPU, fp32) restatements of torch_cluster.grid_cluster, torch_geometric.nn.voxel_grid and
torch_geometric.nn.pool.consecutive.consecutive_cluster, with this package's stated rule where upstream returns garbage,
and of the generic coarsening the pooling operators derive from a cluster vector.  Everything here is exact: CPU fp32
subtraction and division are IEEE, one rounding each, which is what the kernels are held to.

    nvox_d = trunc((end_d - start_d) / size_d) + 1          1 for a NaN, infinite or negative quotient
    c_d    = trunc((pos_d - start_d) / size_d)              clamped to [0, nvox_d - 1]; NaN -> 0
    id     = sum_d c_d * prod_{d' < d} nvox_d'  (+ event * prod_d nvox_d for voxel_grid)
"""
import math

import torch

MAX_CELLS = 2 ** 32 - 1


def _vec(v, D):
    t = torch.as_tensor(v, dtype=torch.float32).reshape(-1)
    return t.expand(D).clone() if t.numel() == 1 else t.clone()


def grid_spec(pos, size, start=None, end=None):
    """(size, start, end) as fp32 [D] tensors; start / end default to pos.min(0) / pos.max(0) like upstream."""
    pos = pos.detach().cpu().float()
    pos = pos.unsqueeze(1) if pos.dim() == 1 else pos
    D = pos.shape[1]
    start = pos.min(0)[0] if start is None else _vec(start, D)
    end = pos.max(0)[0] if end is None else _vec(end, D)
    return _vec(size, D), start, end


def nvox_of(size, start, end):
    """Cells per dimension as Python ints (unbounded: the caller compares the product with MAX_CELLS)."""
    q = (end - start) / size
    return [int(v) + 1 if v >= 0.0 and not math.isinf(v) else 1 for v in q.tolist()]


def cut_nvox(nvox):
    """The package's rule for a grid with more than MAX_CELLS cells: the count that passes the limit is cut."""
    out, prod = [], 1
    for nv in nvox:
        nv = min(nv, MAX_CELLS // prod)
        prod *= nv
        out.append(nv)
    return out


def grid_cluster_ref(pos, size, start=None, end=None, clamp=True):
    """int64 [N].  clamp=False is upstream's bare formula (equal to the clamped one for finite pos inside [start, end])."""
    pos = pos.detach().cpu().float()
    pos = pos.unsqueeze(1) if pos.dim() == 1 else pos
    N, D = pos.shape
    size, start, end = grid_spec(pos, size, start, end) if N else (_vec(size, D), torch.zeros(D), torch.zeros(D))
    nvox = cut_nvox(nvox_of(size, start, end))
    t = ((pos - start) / size).double()                     # the fp32 quotient, widened exactly
    out = torch.zeros(N, dtype=torch.int64)
    mul = 1
    for d in range(D):
        c = t[:, d]
        if clamp:
            c = torch.where(c > 0, c, torch.zeros_like(c))              # NaN, -inf, below start -> 0
            c = torch.minimum(c, torch.full_like(c, float(nvox[d] - 1)))
        out += c.trunc().to(torch.int64) * mul
        mul *= nvox[d]
    return out


def cells_of(pos, size, start=None, end=None):
    size, start, end = grid_spec(pos, size, start, end)
    return math.prod(cut_nvox(nvox_of(size, start, end)))


def voxel_grid_ref(pos, size, batch=None, start=None, end=None):
    """PyG: the batch id is one more coordinate with size 1, start 0, end B - 1, i.e. the most significant digit."""
    local = grid_cluster_ref(pos, size, start, end)
    if batch is None or local.numel() == 0:
        return local
    return local + batch.detach().cpu().to(torch.int64) * cells_of(pos, size, start, end)


def consecutive_cluster_ref(src):
    """(node_map, perm): rank among the sorted unique values; perm[c] = the HIGHEST node index of cluster c (upstream's
    CPU result: the last write of a scatter in index order)."""
    src = src.detach().cpu()
    uniq, inv = torch.unique(src, sorted=True, return_inverse=True)
    perm = torch.full((uniq.numel(),), -1, dtype=torch.int64)
    for i, c in enumerate(inv.tolist()):
        perm[c] = i
    return inv, perm


def coarsen_ref(cluster, batch=None, B=None):
    """What the pooling operators derive from any cluster vector: node_map, order (stable sort), rowptr, C, and with a
    batch the pooled batch, its ptr and the largest / smallest pooled event."""
    cluster = cluster.detach().cpu().to(torch.int64)
    N = cluster.numel()
    node_map, perm = consecutive_cluster_ref(cluster) if N else (cluster.clone(), cluster.clone())
    C = perm.numel()
    order = torch.sort(cluster, stable=True)[1]
    counts = torch.bincount(node_map, minlength=C)
    rowptr = torch.cat([torch.zeros(1, dtype=torch.int64), counts.cumsum(0)]).to(torch.int32)
    res = {"node_map": node_map, "order": order, "rowptr": rowptr, "C": C, "perm": perm}
    if batch is not None:
        batch = batch.detach().cpu()
        pb = batch[perm] if C else batch.new_zeros(0)
        per_event = torch.bincount(pb, minlength=B)
        res.update(batch=pb, ptr=torch.cat([torch.zeros(1, dtype=torch.int64), per_event.cumsum(0)]),
                   max_nodes=int(per_event.max()) if B else 0, min_nodes=int(per_event.min()) if B else 0)
    return res

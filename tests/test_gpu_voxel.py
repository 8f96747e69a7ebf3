"""grid_cluster / voxel_grid / consecutive_cluster and the one-launch coarsening of their result on the GPU.  Every
comparison is exact equality: the ids against tests/voxel_reference.py, the coarsening and the pooling against the
generic branch the same ids take as a clone."""
import types
import warnings

import pytest
import torch

from poisoned_alloc import run_both, to_bytes
from voxel_reference import coarsen_ref, consecutive_cluster_ref, grid_cluster_ref, voxel_grid_ref

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 2, 33, 64, 65, 130)          # the padding edges of the ranking network, an empty event first
CO_ATTRS = ("node_map", "order", "rowptr", "batch", "ptr")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _batch(dev, sizes, register=True):
    """(batch on dev, ptr on dev, B), registered with its event sizes so that no operator has to read it."""
    import deepmetv2_amd as dm
    sz = torch.tensor(sizes, dtype=torch.int64)
    ptr = torch.cat([torch.zeros(1, dtype=torch.int64), sz.cumsum(0)])
    batch = torch.repeat_interleave(torch.arange(len(sizes)), sz).to(dev)
    if register:
        dm.register_batch(batch, ptr.to(dev), len(sizes), max_nodes=max(sizes), min_nodes=min(sizes))
    return batch, ptr.to(dev), len(sizes)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool((to_bytes(a) == to_bytes(b)).all())


@pytest.fixture(autouse=True)
def _drain():
    import deepmetv2_amd as dm
    dm.raise_deferred_errors()
    yield
    dm.raise_deferred_errors()


# ---------------------------------------------------------------------------------------------------------------
# ids
# ---------------------------------------------------------------------------------------------------------------
def _boundary_positions(N, size, start, end, g):
    """start + k size and one ulp either side of it, per dimension: where a wrongly rounded division shows."""
    D = size.numel()
    nv = ((end - start) / size).trunc() + 1
    k = (torch.rand(N, D, generator=g) * nv).floor()
    p = start + k * size
    side = torch.randint(-1, 2, (N, D), generator=g)
    up, down = torch.nextafter(p, torch.full_like(p, float("inf"))), torch.nextafter(p, torch.full_like(p, float("-inf")))
    return torch.where(side > 0, up, torch.where(side < 0, down, p))


GRIDS = [                                    # D, size, start, end (None: min / max of the positions)
    (1, 0.1, -2.5, 2.5),
    (1, 1.0 / 3.0, None, None),
    (2, (0.7, 0.3), (0.37, -3.0), (9.0, 3.25)),
    (2, 0.05, None, None),
    (3, (0.1, 1.0, 0.3), None, (4.0, 9.0, 2.0)),
    (3, 0.25, 0.0, 7.0),
    (8, (0.5, 0.3, 0.7, 1.0, 0.9, 0.11, 2.0, 0.6), -1.0, 1.5),
    (8, 0.8, None, None),
]


@pytest.mark.parametrize("D,size,start,end", GRIDS)
@pytest.mark.parametrize("stray", [False, True])
def test_ids_match_reference(dev, D, size, start, end, stray):
    import deepmetv2_amd as dm
    g = _gen(17 * D + (3 if stray else 0))
    batch, _ptr, _B = _batch(dev, SIZES)
    N = batch.numel()
    sz = torch.as_tensor(size, dtype=torch.float32).reshape(-1).expand(D)
    lo = torch.as_tensor(-2.0 if start is None else start, dtype=torch.float32).reshape(-1).expand(D)
    hi = torch.as_tensor(2.0 if end is None else end, dtype=torch.float32).reshape(-1).expand(D)
    pos = _boundary_positions(N, sz, lo, hi, g)
    if stray:       # outside [start, end] and non-finite: the clamp rule
        far = 1.0 if start is None or end is None else 1e6      # min / max as bounds: the grid grows with the stray point
        pos[3] = lo - far
        pos[40] = hi + far
        pos[41, 0] = float("nan")
        pos[77, D - 1] = float("inf")
        pos[100, 0] = float("-inf")
    posd = pos.to(dev)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                 # a registered batch: no host sync, start / end given or not
    try:
        got = dm.voxel_grid(posd, size, batch, start, end)
        got1 = dm.grid_cluster(posd, size, start, end)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert got.dtype == torch.int64 and got.shape == (N,)
    assert torch.equal(got.cpu(), voxel_grid_ref(pos, size, batch, start, end))
    assert torch.equal(got1.cpu(), grid_cluster_ref(pos, size, start, end))
    if not stray and start is not None and end is not None:
        inside = ((pos >= lo) & (pos <= hi)).all(1)
        assert torch.equal(got1.cpu()[inside], grid_cluster_ref(pos, size, start, end, clamp=False)[inside])


def test_ids_argument_forms(dev):
    """size / start / end as numbers, sequences, CPU and device tensors give the same ids; [N] is [N, 1]; bf16 and fp16
    are upcast exactly; an unregistered batch is read and checked; N = 0."""
    import deepmetv2_amd as dm
    g = _gen(5)
    batch, _ptr, _B = _batch(dev, SIZES)
    N = batch.numel()
    pos = torch.rand(N, 2, generator=g) * 4 - 2
    posd = pos.to(dev)
    want = voxel_grid_ref(pos, (0.3, 0.3), batch, (-2.0, -2.0), (2.0, 2.0))
    for size, start, end in [(0.3, -2.0, 2.0), ([0.3, 0.3], (-2.0, -2.0), torch.tensor([2.0, 2.0])),
                             (torch.tensor([0.3, 0.3], device=dev), torch.tensor(-2.0, device=dev), 2.0)]:
        assert torch.equal(dm.voxel_grid(posd, size, batch, start, end).cpu(), want)
    assert torch.equal(dm.voxel_grid(posd, 0.3, batch.clone(), -2.0, 2.0).cpu(), want)
    assert torch.equal(dm.grid_cluster(posd[:, 0], 0.3).cpu(), grid_cluster_ref(pos[:, 0], 0.3))
    for dt in (torch.bfloat16, torch.float16):
        low = pos.to(dt)
        assert torch.equal(dm.voxel_grid(low.to(dev), 0.3, batch).cpu(), voxel_grid_ref(low.float(), 0.3, batch))
    empty = dm.voxel_grid(posd[:0], 0.3, batch[:0], -2.0, 2.0)
    assert empty.dtype == torch.int64 and empty.shape == (0,)
    assert dm.grid_cluster(posd[:0], 0.3).shape == (0,)
    with pytest.raises(ValueError, match="sorted"):
        dm.voxel_grid(posd, 0.3, batch.flip(0), -2.0, 2.0)
    with pytest.raises(TypeError, match="float64"):
        dm.voxel_grid(posd.double(), 0.3, batch)


def test_deferred_errors(dev):
    """A grid computed on the device with more than 2^32 - 1 cells is cut, the ids stay in range, and the deferred check
    reports it; so does a registered batch that is not the vector it was registered as."""
    import deepmetv2_amd as dm
    batch, ptr, B = _batch(dev, SIZES)
    N = batch.numel()
    pos = torch.rand(N, 2, generator=_gen(9)) * 1e6
    ids = dm.voxel_grid(pos.to(dev), 1e-4, batch)           # start / end = None: 10^10 cells per dimension
    with pytest.raises(RuntimeError, match=r"more than 2\^32 - 1 cells"):
        dm.raise_deferred_errors()
    assert torch.equal(ids.cpu(), voxel_grid_ref(pos, 1e-4, batch))
    assert int(ids.min()) >= 0 and int(ids.max()) < B * (2 ** 32 - 1)
    out, pb = dm.max_pool_x(ids, pos.to(dev), batch)        # and it pools like any other
    ref, _ = dm.max_pool_x(ids.clone(), pos.to(dev), batch)
    assert _same(out, ref)
    wrong = batch.flip(0).contiguous()
    dm.register_batch(wrong, ptr, B, max_nodes=max(SIZES), min_nodes=0)
    ids = dm.voxel_grid(pos.to(dev), 1e5, wrong, 0.0, 1e6)
    with pytest.raises(RuntimeError, match="not the sorted vector"):
        dm.raise_deferred_errors()
    assert torch.equal(ids.cpu(), voxel_grid_ref(pos, 1e5, batch, 0.0, 1e6))      # the ids follow the registered ptr


# ---------------------------------------------------------------------------------------------------------------
# coarsening
# ---------------------------------------------------------------------------------------------------------------
def _cells_1d(dev, cells, batch, ncell):
    """A registered voxel tensor whose event-local cell ids are `cells`: D = 1, cell c is [c, c + 1)."""
    import deepmetv2_amd as dm
    pos = (cells.to(torch.float32) + 0.5).to(dev)
    return dm.voxel_grid(pos, 1.0, batch, 0.0, float(ncell - 1))


def _assert_coarsening_equal(cluster, batch, N, B):
    """The registered tensor against its clone (the generic branch) and against the CPU reference."""
    from deepmetv2_amd.pool import _Coarsening, _voxel_registry
    from deepmetv2_amd.graph import _registry_get
    assert _registry_get(_voxel_registry, cluster) is not None
    fast, slow = _Coarsening(cluster, batch, N), _Coarsening(cluster.clone(), batch, N)
    ref = coarsen_ref(cluster, batch, B)
    for name in CO_ATTRS:
        a, b = getattr(fast, name), getattr(slow, name)
        assert _same(a, b), name
        assert torch.equal(a.cpu().to(torch.int64), ref[name].to(torch.int64)), name
    for name in ("C", "max_nodes", "min_nodes", "B", "_sorted"):
        assert getattr(fast, name) == getattr(slow, name), name
    assert (fast.C, fast.max_nodes, fast.min_nodes) == (ref["C"], ref["max_nodes"], ref["min_nodes"])
    return fast


PATTERNS = {
    "one_cell": lambda n, g: torch.full((n,), 5),
    "own_cell": lambda n, g: torch.arange(n),
    "descending": lambda n, g: torch.arange(n - 1, -1, -1),
    "straddle": lambda n, g: torch.arange(n) // 3,          # positions 63, 64, 65 share a cell: across the power of two
    "random": lambda n, g: torch.randint(0, max(n // 4, 1), (n,), generator=g),
}


@pytest.mark.parametrize("pattern", sorted(PATTERNS))
@pytest.mark.parametrize("sizes", [SIZES, (0, 5, 0, 0, 7, 0), (1,), (3, 0)])
def test_coarsening_matches_generic_branch(dev, pattern, sizes):
    g = _gen(len(pattern))
    batch, _ptr, B = _batch(dev, sizes)
    cells = torch.cat([PATTERNS[pattern](n, g) for n in sizes])
    cluster = _cells_1d(dev, cells, batch, 200)
    assert torch.equal(cluster.cpu(), cells + 200 * batch.cpu())
    _assert_coarsening_equal(cluster, batch, batch.numel(), B)


def test_coarsening_at_the_lds_limit(dev):
    """An event of exactly DMET_SELECT_LDS_NODES nodes ranks in LDS, one node more in the workspace: the same bits."""
    import deepmetv2_amd as dm
    from deepmetv2_amd._native import SELECT_LDS_NODES
    sizes = (SELECT_LDS_NODES, SELECT_LDS_NODES + 1)
    batch, _ptr, B = _batch(dev, sizes)
    pos = torch.rand(sum(sizes), 2, generator=_gen(3)).to(dev)
    cluster = dm.voxel_grid(pos, (0.02, 0.01), batch, 0.0, 1.0)
    fast = _assert_coarsening_equal(cluster, batch, batch.numel(), B)
    out = fast.pool(pos, "max")
    assert out.shape == (fast.C, 2)


def test_consecutive_cluster_and_no_batch(dev):
    import deepmetv2_amd as dm
    from deepmetv2_amd.pool import _Coarsening
    pos = torch.rand(300, 3, generator=_gen(4))
    cluster = dm.grid_cluster(pos.to(dev), 0.25, 0.0, 1.0)
    node_map, perm = dm.consecutive_cluster(cluster)
    ref_map, ref_perm = consecutive_cluster_ref(cluster)
    assert torch.equal(node_map.cpu(), ref_map) and torch.equal(perm.cpu(), ref_perm)
    own = torch.randint(-50, 50, (300,), generator=_gen(6))             # any vector: torch.unique, the same contract
    node_map, perm = dm.consecutive_cluster(own.to(dev))
    ref_map, ref_perm = consecutive_cluster_ref(own)
    assert torch.equal(node_map.cpu(), ref_map) and torch.equal(perm.cpu(), ref_perm)
    fast, slow = _Coarsening(cluster, None, 300), _Coarsening(cluster.clone(), None, 300)
    for name in ("node_map", "order", "rowptr"):
        assert _same(getattr(fast, name), getattr(slow, name)), name
    assert fast.C == slow.C and fast.batch is None and fast.ptr is None and fast.pooled_batch() is None


def test_unregistered_vectors_take_the_generic_branch(dev):
    """A user's own cluster vector, a clone, and voxel ids pooled over another batch give what they always gave."""
    import deepmetv2_amd as dm
    from deepmetv2_amd.pool import _Coarsening
    batch, _ptr, B = _batch(dev, SIZES)
    N = batch.numel()
    own = (torch.randint(0, 9, (N,), generator=_gen(8)) + 9 * batch.cpu()).to(dev)
    ref = coarsen_ref(own, batch, B)
    co = _Coarsening(own, batch, N)
    for name in CO_ATTRS:
        assert torch.equal(getattr(co, name).cpu().to(torch.int64), ref[name].to(torch.int64)), name
    assert (co.C, co.max_nodes, co.min_nodes) == (ref["C"], ref["max_nodes"], ref["min_nodes"])
    pos = torch.rand(N, 2, generator=_gen(2)).to(dev)
    cluster = dm.voxel_grid(pos, 0.2, batch, 0.0, 1.0)
    other, _p, _b = _batch(dev, SIZES)                      # the same values, another tensor: not the events of the ids
    co = _Coarsening(cluster, other, N)
    ref = coarsen_ref(cluster, batch, B)
    for name in CO_ATTRS:
        assert torch.equal(getattr(co, name).cpu().to(torch.int64), ref[name].to(torch.int64)), name
    cluster.add_(0)                                         # an in-place write drops the registration
    from deepmetv2_amd.graph import _registry_get
    from deepmetv2_amd.pool import _voxel_registry
    assert _registry_get(_voxel_registry, cluster) is None
    with pytest.raises(NotImplementedError):
        dm.max_pool_x(cluster, pos, batch, size=4)


# ---------------------------------------------------------------------------------------------------------------
# pooling
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [5, 64])
def test_pooling_parity(dev, F):
    import deepmetv2_amd as dm
    from deepmetv2_amd.graph import _batch_registry, _registry_get
    g = _gen(F)
    batch, _ptr, B = _batch(dev, SIZES)
    N = batch.numel()
    pos = torch.rand(N, 2, generator=g).to(dev)
    x0 = torch.randn(N, F, generator=g).to(dev)
    x0[::7] = x0[3]                                         # ties inside clusters
    for op in (dm.max_pool_x, dm.avg_pool_x):
        res = []
        for clone in (False, True):
            cluster = dm.voxel_grid(pos, (0.3, 0.2), batch)
            x = x0.clone().requires_grad_(True)
            out, pb = op(cluster.clone() if clone else cluster, x, batch)
            gout = torch.randn(out.shape, generator=_gen(1)).to(dev)
            out.backward(gout)
            res.append((out.detach(), pb, x.grad))
            info = _registry_get(_batch_registry, pb)
            assert info is not None and info.num_events == B and info.ptr[-1].item() == out.shape[0]
        for a, b in zip(*res):
            assert _same(a, b)
    for op in (dm.max_pool, dm.avg_pool):
        res = []
        for clone in (False, True):
            cluster = dm.voxel_grid(pos, (0.3, 0.2), batch)
            x = x0.clone().requires_grad_(True)
            data = types.SimpleNamespace(x=x, pos=pos, batch=batch)
            out = op(cluster.clone() if clone else cluster, data)
            out.x.backward(torch.ones_like(out.x))
            res.append((out.x.detach(), out.pos, out.batch, x.grad))
        for a, b in zip(*res):
            assert _same(a, b)


def test_pooled_batch_feeds_knn_graph_without_a_sync(dev):
    import deepmetv2_amd as dm
    batch, _ptr, _B = _batch(dev, SIZES[1:])                # no empty event: every pooled event holds a node
    pos = torch.rand(batch.numel(), 2, generator=_gen(12)).to(dev)
    cluster = dm.voxel_grid(pos, 0.25, batch, 0.0, 1.0)
    ppos, pb = dm.avg_pool_x(cluster, pos, batch)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ei = dm.knn_graph(ppos, 1, pb, loop=True)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert ei.shape == (2, ppos.shape[0])


def _count_syncs(fn):
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            fn()
        finally:
            torch.cuda.set_sync_debug_mode(0)
    return sum("called a synchronizing" in str(r.message) for r in rec)


def test_sync_counts(dev):
    import deepmetv2_amd as dm
    batch, _ptr, _B = _batch(dev, SIZES)
    pos = torch.rand(batch.numel(), 2, generator=_gen(13)).to(dev)
    x = torch.randn(batch.numel(), 5, generator=_gen(14)).to(dev)
    held = {}
    assert _count_syncs(lambda: held.update(a=dm.voxel_grid(pos, 0.25, batch, 0.0, 1.0))) == 0
    assert _count_syncs(lambda: held.update(b=dm.voxel_grid(pos, 0.25, batch))) == 0
    assert _count_syncs(lambda: dm.max_pool_x(held["a"], x, batch)) == 1        # the record (C, largest, smallest)
    assert _count_syncs(lambda: dm.avg_pool_x(held["b"], x, batch)) == 1


# ---------------------------------------------------------------------------------------------------------------
# determinism
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", [SIZES, (16385, 40)])
def test_same_bits_whatever_the_buffers_held(dev, sizes):
    import deepmetv2_amd as dm
    from deepmetv2_amd.pool import _Coarsening
    batch, _ptr, _B = _batch(dev, sizes)
    N = batch.numel()
    pos = torch.rand(N, 2, generator=_gen(21)).to(dev)

    def call():
        cluster = dm.voxel_grid(pos, (0.05, 0.1), batch)
        co = _Coarsening(cluster, batch, N)
        return [cluster] + [getattr(co, name) for name in CO_ATTRS] + [torch.tensor([co.C, co.max_nodes, co.min_nodes])]

    runs = run_both(call)
    plain = [t.cpu() for t in call()]
    for other in list(runs.values()) + [[t.cpu() for t in call()]]:
        assert len(other) == len(plain)
        for a, b in zip(plain, other):
            assert _same(a, b)

"""Farthest point sampling and nearest on the GPU (csrc/fps.hip; deepmetv2_amd.fps / nearest) against the exact numpy
restatements tests/fps_reference.py and tests/knn_xy_reference.py.  Every comparison is equality of the whole index
vector: the contract (include/dmet.h, dmet_fps_f32) fixes the fp32 distance chain and the tie rule, so there is no
tolerance.  The shapes are the smallest that reach each path of the kernel: events around one wavefront and around the
workgroup (T = FPS_THREADS: a thread then owns one, two or three points), every compiled coordinate count and the generic
one, an event one node above the on-chip cap (distances in the workspace, coordinates through L2), exact ties."""
import numpy as np
import pytest
import torch

import fps_reference as ref
import knn_xy_reference as kref

pytestmark = pytest.mark.gpu


def _T():
    from deepmetv2_amd import _native
    return _native.FPS_THREADS


def _events(sizes, dev):
    sizes = np.asarray(sizes, dtype=np.int64)
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.from_numpy(sizes)).to(dev)
    return ptr, batch


def _check(dev, x, sizes, ratio, **kw):
    """fps(random_start=False) of the ragged batch against the reference; returns the ids."""
    import deepmetv2_amd as dm
    ptr, batch = _events(sizes, dev)
    r_np = ratio.numpy() if torch.is_tensor(ratio) else ratio
    want = ref.fps(x, ptr, ref.sample_counts(ptr, r_np))
    r_dev = ratio.to(dev) if torch.is_tensor(ratio) else ratio
    got = dm.fps(torch.from_numpy(x).to(dev), batch, r_dev, random_start=False, **kw)
    assert got.dtype == torch.int64 and got.device.type == "cuda"
    assert np.array_equal(got.cpu().numpy(), want)
    return want


SINGLE = {"1": lambda T: 1, "2": lambda T: 2, "63": lambda T: 63, "64": lambda T: 64, "65": lambda T: 65,
          "T-1": lambda T: T - 1, "T": lambda T: T, "T+1": lambda T: T + 1, "2T+1": lambda T: 2 * T + 1}


@pytest.mark.parametrize("D", [1, 2, 3, 8])
@pytest.mark.parametrize("ratio", [1.0, 0.3])
@pytest.mark.parametrize("size", list(SINGLE))
def test_single_event(dev, size, ratio, D):
    n = SINGLE[size](_T())
    x = np.random.default_rng(1000 * n + D).standard_normal((n, D)).astype(np.float32)
    want = _check(dev, x, [n], ratio)
    assert len(want) == int(np.ceil(np.float32(n) * np.float32(ratio)))
    if ratio == 1.0:
        assert sorted(want.tolist()) == list(range(n))        # distinct points: a permutation of the event


@pytest.mark.parametrize("D", [4, 5, 13])
def test_other_coordinate_counts(dev, D):
    """D = 4 is the last compiled width, 5 the first that takes the generic loop (its one-by-one tail only; D = 8 above is
    one block of eight coordinates without a tail), 13 a block of eight and a tail."""
    n = _T() + 1
    x = np.random.default_rng(40 + D).standard_normal((n, D)).astype(np.float32)
    _check(dev, x, [n], 0.3)


def test_many_exact_ties_and_duplicates(dev):
    x = np.random.default_rng(3).integers(0, 4, size=(300, 2)).astype(np.float32)
    want = _check(dev, x, [300], 1.0)
    assert len(want) == 300 and len(np.unique(x, axis=0)) <= 16
    assert (want[16:] == 0).all()                              # every distinct point taken: index 0 repeats


def test_all_points_equal(dev):
    x = np.full((130, 3), 0.75, dtype=np.float32)
    want = _check(dev, x, [130], 0.5)
    assert want.tolist() == [0] * 65


def test_ragged_batch_with_empty_events(dev):
    import deepmetv2_amd as dm
    sizes = [5, 0, _T() + 3, 1, 70, 0]
    x = np.random.default_rng(5).standard_normal((sum(sizes), 2)).astype(np.float32)
    _check(dev, x, sizes, 0.4, batch_size=6)
    per_event = torch.tensor([1.0, 0.5, 0.1, 1.0, 0.3, 0.7])
    want = _check(dev, x, sizes, per_event, batch_size=6)
    _check(dev, x, sizes, torch.tensor([0.25]), batch_size=6)
    # ptr= instead of the batch vector (which is then ignored)
    ptr, batch = _events(sizes, dev)
    got = dm.fps(torch.from_numpy(x).to(dev), None, per_event.to(dev), random_start=False, ptr=torch.from_numpy(ptr).to(dev))
    assert np.array_equal(got.cpu().numpy(), want)
    assert bool((batch[got][1:] >= batch[got][:-1]).all())     # grouped by event


def test_start_is_clamped_and_more_samples_than_nodes(dev):
    """The native entry with starts outside their events and m > n (the wrapper never asks for either)."""
    from deepmetv2_amd import _native
    sizes = [9, 70, 3]
    ptr, _batch = _events(sizes, dev)
    x = np.random.default_rng(6).standard_normal((sum(sizes), 3)).astype(np.float32)
    m = np.array([14, 20, 3])
    start = np.array([-3, 10 ** 6, 1])
    out_ptr = np.concatenate([[0], np.cumsum(m)]).astype(np.int64)
    got = _native.fps(torch.from_numpy(x).to(dev), torch.from_numpy(ptr).to(dev), torch.from_numpy(out_ptr).to(dev),
                      torch.from_numpy(start).to(dev), int(out_ptr[-1]))
    want = ref.fps(x, ptr, m, start)
    assert np.array_equal(got.cpu().numpy(), want)
    assert want[0] == 0 and want[14] == 9 + 69 and (want[9:14] == 0).all()


def test_above_the_on_chip_cap(dev):
    from deepmetv2_amd import _native
    D = 3
    big = _native.FPS_LDS_NODES(D) + 1
    sizes = [big, 100]
    x = np.random.default_rng(7).standard_normal((sum(sizes), D)).astype(np.float32)
    want = _check(dev, x, sizes, torch.tensor([40.0 / big, 0.5]))
    assert 40 <= len(want) - 50 <= 41
    # the event at the cap itself stays on chip
    _check(dev, x[:big - 1], [big - 1], 40.0 / big)


def test_wide_rows(dev):
    from deepmetv2_amd import _native
    x = np.random.default_rng(8).standard_normal((40, 64)).astype(np.float32)
    _check(dev, x, [40], 1.0)
    n = _native.FPS_LDS_NODES(64) + 1                           # the smallest event whose rows no longer fit in LDS
    x = np.random.default_rng(9).standard_normal((n, 64)).astype(np.float32)
    _check(dev, x, [n], 0.05)
    _check(dev, x[:n - 1], [n - 1], 0.05)


def test_random_start(dev):
    import deepmetv2_amd as dm
    sizes = [33, 1, 200, 64]
    ptr, batch = _events(sizes, dev)
    x = np.random.default_rng(11).standard_normal((sum(sizes), 2)).astype(np.float32)
    xd = torch.from_numpy(x).to(dev)
    m = ref.sample_counts(ptr, 0.5)
    out_ptr = np.concatenate([[0], np.cumsum(m)])
    torch.manual_seed(1234)
    a = dm.fps(xd, batch, 0.5, random_start=True).cpu().numpy()
    torch.manual_seed(1234)
    b = dm.fps(xd, batch, 0.5, random_start=True).cpu().numpy()
    assert np.array_equal(a, b)
    start = a[out_ptr[:-1]] - ptr[:-1]
    assert ((start >= 0) & (start < np.asarray(sizes))).all()
    assert np.array_equal(a, ref.fps(x, ptr, m, start))


def test_no_host_sync_with_equal_registered_events(dev):
    """150 * fp32(0.3) rounds to 45.0 in fp32 (the exact product is above 45): the host's M and the device's out_ptr must
    agree on it."""
    import deepmetv2_amd as dm
    B, n = 4, 150
    ptr, batch = _events([n] * B, dev)
    x = np.random.default_rng(12).standard_normal((B * n, 2)).astype(np.float32)
    xd = torch.from_numpy(x).to(dev)
    dm.register_batch(batch, torch.from_numpy(ptr).to(dev), B, max_nodes=n, min_nodes=n)
    dm.fps(xd, batch, 0.3)                                      # module load, allocator and generator warm-up
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        fixed = dm.fps(xd, batch, 0.3, random_start=False)
        drawn = dm.fps(xd, batch, 0.3, random_start=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert fixed.shape == drawn.shape == (B * 45,)
    assert np.array_equal(fixed.cpu().numpy(), ref.fps(x, ptr, [45] * B))
    assert np.array_equal(drawn.cpu().numpy() // n, np.repeat(np.arange(B), 45))


def test_non_finite_coordinates_stay_inside_the_event(dev):
    import deepmetv2_amd as dm
    sizes = [200, 200]
    _ptr, batch = _events(sizes, dev)
    x = np.random.default_rng(13).standard_normal((400, 2)).astype(np.float32)
    x[17] = np.nan
    x[200 + 31] = np.inf
    got = dm.fps(torch.from_numpy(x).to(dev), batch, 0.5, random_start=False).cpu().numpy()
    assert got.shape == (200,)
    assert ((got[:100] >= 0) & (got[:100] < 200)).all() and ((got[100:] >= 200) & (got[100:] < 400)).all()


# ---- nearest --------------------------------------------------------------------------------------------------------
def test_nearest_matches_the_reference(dev):
    import deepmetv2_amd as dm
    sx, sy = [30, 4, 50, 7], [10, 5, 20, 3]
    ptr_x, bx = _events(sx, dev)
    ptr_y, by = _events(sy, dev)
    rng = np.random.default_rng(14)
    x = rng.standard_normal((sum(sx), 3)).astype(np.float32)
    y = rng.standard_normal((sum(sy), 3)).astype(np.float32)
    y[3] = x[5]                                     # one point present in both sets (event 0)
    y[ptr_y[2] + 11] = y[ptr_y[2] + 4]              # two rows of y tie for every x of event 2: the lower index wins
    x[ptr_x[2] + 8] = y[ptr_y[2] + 4]
    got = dm.nearest(torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev), bx, by)
    want = kref.knn_table(y, ptr_y, x, ptr_x, 1)[0][:, 0].astype(np.int64)
    assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), want)
    assert want[5] == 3 and want[ptr_x[2] + 8] == ptr_y[2] + 4 and not (want == ptr_y[2] + 11).any()
    dm.raise_deferred_errors()                      # every row found its row of y


def test_nearest_without_candidates_raises_at_the_next_call(dev):
    import deepmetv2_amd as dm
    _px, bx = _events([5, 4], dev)
    _py, by = _events([3, 0], dev)
    x = torch.randn(9, 2, device=dev)
    y = torch.randn(3, 2, device=dev)
    dm.raise_deferred_errors()
    out = dm.nearest(x, y, bx, by)
    assert out.shape == (9,)
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="nearest: a row of x found no row of y"):
        dm.knn_graph(x, 2, bx)
    dm.raise_deferred_errors()                      # reported once


# ---- sampling, assignment and pooling end to end ------------------------------------------------------------------
def test_sample_assign_pool_chain(dev):
    import deepmetv2_amd as dm
    sizes = [40, 300, 123]
    ptr, batch = _events(sizes, dev)
    rng = np.random.default_rng(15)
    pos = rng.standard_normal((sum(sizes), 2)).astype(np.float32)
    feat = rng.standard_normal((sum(sizes), 5)).astype(np.float32)
    posd = torch.from_numpy(pos).to(dev)
    idx = dm.fps(posd, batch, 0.25, random_start=False)
    cluster = dm.nearest(posd, posd[idx], batch, batch[idx])
    pooled, pooled_batch = dm.max_pool_x(cluster, torch.from_numpy(feat).to(dev), batch)
    m = ref.sample_counts(ptr, 0.25)
    idx_ref = ref.fps(pos, ptr, m)
    out_ptr = np.concatenate([[0], np.cumsum(m)]).astype(np.int64)
    cl_ref = kref.knn_table(pos[idx_ref], out_ptr, pos, ptr, 1)[0][:, 0].astype(np.int64)
    M = len(idx_ref)
    assert np.array_equal(idx.cpu().numpy(), idx_ref)
    assert np.array_equal(cluster.cpu().numpy(), cl_ref)
    assert np.array_equal(cl_ref[idx_ref], np.arange(M))       # every centre is a member of its own cluster
    want = np.stack([feat[cl_ref == c].max(0) for c in range(M)])
    assert np.array_equal(pooled.cpu().numpy(), want)
    assert np.array_equal(pooled_batch.cpu().numpy(), np.repeat(np.arange(3), m))

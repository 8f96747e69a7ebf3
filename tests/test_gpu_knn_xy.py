"""knn(x, y) / radius(x, y) on the GPU: the two-set builders (dmet_knn_xy_f32 / dmet_radius_xy_f32).

Ids AND distance bits against the exact numpy restatement (tests/knn_xy_reference.py), no exclusions: ragged events with
unrelated counts on the two sides, every kernel form (packed D <= 8, wide, both ends of k), exact ties, NaN / inf / beyond
the sentinel, periodic phi, and against the merged self-query builds (matrix-core kNN, radius_table) on a copy."""
import math

import numpy as np
import pytest
import torch

import knn_xy_reference as xy
from radius_periodic_reference import F32, pair_d2

pytestmark = pytest.mark.gpu

TWO_PI = 2 * math.pi
PI32 = float(np.float32(np.pi))
# (candidates, queries) per event: unrelated counts, 0 candidates, 0 queries, fewer than k candidates, one on each side,
# more than one 128-query tile against few candidates and the reverse
SX = [300, 0, 70, 5, 1, 40, 700, 129]
SY = [150, 30, 0, 64, 1, 900, 3, 257]


def _ptr(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def _batch(sizes, dev):
    return torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes)).to(dev)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy() if torch.is_tensor(t) else np.asarray(t, F32).view(np.int32)


def _fma32(a, acc):
    """fp32 fmaf(a, a, acc) with torch, exact: radius_periodic_reference._fma32 restated (the product is exact in float64,
    TwoSum makes the sum exact, round to odd before the cast to fp32)."""
    p, q = a.double() * a.double(), acc.double()
    s = p + q
    bb = s - p
    err = (p - (s - bb)) + (q - bb)
    fix = torch.isfinite(s) & (err != 0) & ((s.view(torch.int64) & 1) == 0)
    toward = torch.where(err > 0, torch.full_like(s, float("inf")), torch.full_like(s, float("-inf")))
    return torch.where(fix, torch.nextafter(s, toward), s).float()


def _sets(D, seed, sx=SX, sy=SY):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(sum(sx), D, generator=g), torch.randn(sum(sy), D, generator=g)


def _check_knn(dev, x, y, sx, sy, k, period=None, batched=True):
    import deepmetv2_amd as dm
    bx, by = (_batch(sx, dev), _batch(sy, dev)) if batched else (None, None)
    ref_nbr, ref_dist = xy.knn_table(x.numpy(), _ptr(sx), y.numpy(), _ptr(sy), k, period)
    t = dm.knn_xy_table(x.to(dev), y.to(dev), k, bx, by, period=period, batch_size=len(sx) if batched else None)
    assert t.nbr.dtype == torch.int32 and t.nbr.shape == (y.shape[0], k)
    assert np.array_equal(t.nbr.cpu().numpy(), ref_nbr)
    assert np.array_equal(_bits(t.dist), _bits(ref_dist))
    ei = dm.knn(x.to(dev), y.to(dev), k, bx, by, period=period, batch_size=len(sx) if batched else None)
    assert ei.dtype == torch.int64 and np.array_equal(ei.cpu().numpy(), xy.edges_of(ref_nbr))
    assert ei.numel() == 0 or int(ei.min()) >= 0
    t2 = dm.knn_xy_table(x.to(dev), y.to(dev), k, bx, by, period=period, batch_size=len(sx) if batched else None)
    assert torch.equal(t.nbr, t2.nbr) and np.array_equal(_bits(t.dist), _bits(t2.dist))       # same bits twice
    return ref_nbr, ref_dist


# the packed form (D <= 8) and the wide forms (16 / 32: two queries per lane, 64: one), both ends of k, padded and exact D
@pytest.mark.parametrize("D,k", [(1, 1), (1, 64), (2, 16), (2, 20), (3, 8), (3, 64), (8, 1), (8, 16), (8, 64),
                                 (12, 16), (32, 1), (32, 16), (32, 64), (64, 1), (64, 8), (64, 20), (64, 64)])
def test_knn_ragged_events(dev, D, k):
    x, y = _sets(D, 100 * D + k)
    ref_nbr, _ = _check_knn(dev, x, y, SX, SY, k)
    short = (ref_nbr < 0).any(1)
    assert bool(short[sum(SY[:1]):sum(SY[:2])].all())            # the event without candidates: empty rows
    if k > 5:
        assert bool(short[sum(SY[:3]):sum(SY[:4])].all())        # 5 candidates: short rows


@pytest.mark.parametrize("D,k", [(2, 16), (32, 8), (64, 16)])
def test_knn_one_event_without_batch_vectors(dev, D, k):
    x, y = _sets(D, 7, [333], [517])
    _check_knn(dev, x, y, [333], [517], k, batched=False)


@pytest.mark.parametrize("D", [2, 32])
def test_knn_tail_only_and_many_small_events(dev, D):
    """few tiles (every tile is split over the candidate range) and many small events (no split)"""
    sx, sy = [3000, 1500], [200, 130]
    x, y = _sets(D, 17, sx, sy)
    _check_knn(dev, x, y, sx, sy, 16)
    g = torch.Generator().manual_seed(5)
    sx = torch.randint(0, 40, (300,), generator=g).tolist()
    sy = torch.randint(0, 40, (300,), generator=g).tolist()
    x, y = _sets(D, 18, sx, sy)
    _check_knn(dev, x, y, sx, sy, 16)


def test_knn_exact_ties_on_a_lattice(dev):
    """integers in [-3, 3]^2 and duplicated rows: many candidates share the distance at rank k (R2 decides)"""
    g = torch.Generator().manual_seed(3)
    sx, sy = [300, 300], [300, 40]
    x = torch.randint(-3, 4, (sum(sx), 2), generator=g).float()
    y = torch.randint(-3, 4, (sum(sy), 2), generator=g).float()
    x[310:330] = x[300]
    k = 16
    d2 = pair_d2(y[:300, None, :].numpy(), x[None, :300, :].numpy(), None)
    srt = np.sort(d2, 1)
    tied = int((srt[:, k - 1] == srt[:, k]).sum())
    assert tied > 150, tied                                      # most queries have a tie across rank k
    _check_knn(dev, x, y, sx, sy, k)
    _check_knn(dev, x, y, sx, sy, 1)


@pytest.mark.parametrize("D", [2, 32])
def test_knn_nonfinite_and_beyond_the_sentinel(dev, D):
    sx, sy = [200, 90], [130, 70]
    x, y = _sets(D, 23, sx, sy)
    x[3, 0] = float("nan"); x[4, D - 1] = float("inf"); x[5, 0] = float("-inf"); x[6, 0] = 2.0e5    # 4e10 > 1e10
    x[205, D - 1] = float("nan")
    y[2, 0] = float("nan"); y[7, D - 1] = float("inf"); y[140, 0] = float("-inf"); y[9, 0] = -3.0e5
    ref_nbr, _ = _check_knn(dev, x, y, sx, sy, 16)
    assert bool((ref_nbr[[2, 7, 9, 140]] < 0).all())            # such a query selects nothing
    assert not np.isin(ref_nbr, [3, 4, 5, 6, 205]).any()          # such a candidate is never selected


@pytest.mark.parametrize("layout", ["etaphi", "phieta", "8d"])
def test_knn_periodic(dev, layout):
    g = torch.Generator().manual_seed(31)

    def phi(n):
        p = torch.atan2(torch.randn(n, generator=g), torch.randn(n, generator=g))
        p[: n // 4] = torch.where(torch.rand(n // 4, generator=g) < 0.5, -1.0, 1.0) * (PI32 - 0.05 * torch.rand(n // 4, generator=g))
        return p
    Nx, Ny = sum(SX), sum(SY)
    eta_x, eta_y = (torch.rand(Nx, generator=g) - 0.5) * 0.6, (torch.rand(Ny, generator=g) - 0.5) * 0.6
    px, py = phi(Nx), phi(Ny)
    px[0], px[1], py[0], py[1] = PI32, -PI32, -PI32, PI32         # seam twins: distance 0 in phi
    if layout == "etaphi":
        x, y, per = torch.stack([eta_x, px], 1), torch.stack([eta_y, py], 1), [None, TWO_PI]
    elif layout == "phieta":
        x, y, per = torch.stack([px, eta_x], 1), torch.stack([py, eta_y], 1), [TWO_PI, None]
    else:
        x, y = torch.randn(Nx, 8, generator=g), torch.randn(Ny, 8, generator=g)
        x[:, 0], y[:, 0], x[:, 7], y[:, 7] = px, py, px.flip(0), py.flip(0)
        per = [TWO_PI, None, None, 0, None, None, None, TWO_PI]
    ref_nbr, ref_dist = _check_knn(dev, x, y, SX, SY, 8, period=per)
    plain = xy.knn_table(x.numpy(), _ptr(SX), y.numpy(), _ptr(SY), 8, None)[0]
    assert (plain != ref_nbr).any(1).sum() > 20                  # the wrap matters for these points
    _check_knn(dev, x, y, SX, SY, 20, period=per)


def _check_radius(dev, x, y, sx, sy, r, m, period=None):
    import deepmetv2_amd as dm
    bx, by = _batch(sx, dev), _batch(sy, dev)
    ref_nbr, ref_cnt = xy.radius_table(x.numpy(), _ptr(sx), y.numpy(), _ptr(sy), r, m, period)
    t = dm.radius_xy_table(x.to(dev), y.to(dev), r, bx, by, m, batch_size=len(sx), period=period, pad=True)
    assert np.array_equal(t.cnt.cpu().numpy(), ref_cnt) and np.array_equal(t.nbr.cpu().numpy(), ref_nbr)
    t0 = dm.radius_xy_table(x.to(dev), y.to(dev), r, bx, by, m, batch_size=len(sx), period=period)      # counted form
    slot = np.arange(m)[None, :] < ref_cnt[:, None]
    assert np.array_equal(t0.cnt.cpu().numpy(), ref_cnt) and np.array_equal(t0.nbr.cpu().numpy()[slot], ref_nbr[slot])
    ei = dm.radius(x.to(dev), y.to(dev), r, bx, by, m, batch_size=len(sx), period=period)
    assert np.array_equal(ei.cpu().numpy(), xy.edges_of(ref_nbr)) and (ei.numel() == 0 or int(ei.min()) >= 0)
    return ref_nbr, ref_cnt


@pytest.mark.parametrize("D,r,m", [(1, 0.05, 8), (2, 0.4, 4), (2, 0.7, 64), (3, 0.7, 16), (4, 0.9, 32), (8, 2.2, 8)])
def test_radius_ragged_events(dev, D, r, m):
    x, y = _sets(D, 40 + D)
    _nbr, cnt = _check_radius(dev, x, y, SX, SY, r, m)
    assert int((cnt == m).sum()) > 0 and int(((cnt > 0) & (cnt < m)).sum()) > 0      # some rows hit the cap, some do not


def test_radius_ties_at_the_cap_nonfinite_and_periodic(dev):
    g = torch.Generator().manual_seed(9)
    sx, sy = [300, 300], [300, 40]
    x = torch.randint(-3, 4, (600, 2), generator=g).float()
    y = torch.randint(-3, 4, (340, 2), generator=g).float()
    _nbr, cnt = _check_radius(dev, x, y, sx, sy, 1.5, 16)       # d2 in {0, 1, 2} < 2.25: ~55 hits per query, cap 16
    assert int((cnt == 16).sum()) > 250
    _check_radius(dev, x, y, sx, sy, 1.0, 16)                   # strict: d2 = 1 is no hit
    x2, y2 = _sets(2, 77)
    x2[3, 0] = float("nan"); x2[4, 1] = float("inf"); y2[2, 0] = float("nan"); y2[7, 1] = float("-inf")
    _check_radius(dev, x2, y2, SX, SY, 0.5, 8)
    x2, y2 = _sets(2, 78)
    x2[:, 1] = (x2[:, 1] * 2).clamp(-PI32, PI32); y2[:, 1] = (y2[:, 1] * 2).clamp(-PI32, PI32)      # many at +-pi exactly
    a, _ = _check_radius(dev, x2, y2, SX, SY, 0.4, 32, period=[None, TWO_PI])
    b, _ = xy.radius_table(x2.numpy(), _ptr(SX), y2.numpy(), _ptr(SY), 0.4, 32, None)
    assert (a != b).any(1).sum() > 10
    _check_radius(dev, x2.flip(1).contiguous(), y2.flip(1).contiguous(), SX, SY, 0.4, 32, period=[TWO_PI, None])


def test_copy_on_both_sides_equals_the_self_query_builds(dev):
    """knn(x, x.clone()) against the merged matrix-core build, radius against radius_table: ids and distance bits"""
    import deepmetv2_amd as dm
    g = torch.Generator().manual_seed(51)
    sizes = [4500, 900, 2300, 1200, 3100]
    x = torch.randn(sum(sizes), 32, generator=g).to(dev)
    b = _batch(sizes, dev)
    for k in (16, 8):
        old = dm.knn_table(x, k, b, loop=True)
        new = dm.knn_xy_table(x, x.clone(), k, b, b.clone())
        assert torch.equal(old.nbr, new.nbr) and np.array_equal(_bits(old.dist), _bits(new.dist))
    ei_old = dm.knn(x, x, 16, b, b)
    ei_new = dm.knn(x, x.clone(), 16, b, b.clone())
    assert torch.equal(ei_old, ei_new)
    x2 = torch.stack([(torch.rand(sum(sizes), generator=g) - 0.5) * 6, (torch.rand(sum(sizes), generator=g) - 0.5) * TWO_PI], 1).to(dev)
    for per, xx in ((None, x2), ([None, TWO_PI], x2), ([TWO_PI, None], x2.flip(1).contiguous())):
        old = dm.radius_table(xx, 0.4, b, loop=True, max_num_neighbors=32, int32_rows=True, period=per)
        new = dm.radius_xy_table(xx, xx.clone(), 0.4, b, b.clone(), 32, period=per)
        assert torch.equal(old.cnt, new.cnt) and int((new.cnt == 32).sum()) > 0
        slot = torch.arange(32, device=dev).view(1, -1) < new.cnt.view(-1, 1)
        assert torch.equal(old.nbr[slot], new.nbr[slot])


# the subset of events compared against the numpy reference at full size (the reference costs 2 s per event at D = 2 and
# 17 s at D = 32 on a CPU); every event is checked for what needs no reference
FULL_REF_EVENTS = {2: [0, 9, 18, 27, 36, 45, 54, 63], 32: [0, 31, 63]}


@pytest.mark.parametrize("D", [2, 32])
def test_full_size(dev, D):
    import deepmetv2_amd as dm
    B, ny, k = 64, 4500, 16
    g = torch.Generator().manual_seed(60 + D)
    sx = torch.randint(1800, 2700, (B,), generator=g).tolist()      # about half as many candidates, different per event
    sy = [ny] * B
    x, y = _sets(D, 61 + D, sx, sy)
    xd, yd, bx, by = x.to(dev), y.to(dev), _batch(sx, dev), _batch(sy, dev)
    t = dm.knn_xy_table(xd, yd, k, bx, by)
    nbr, dist = t.nbr, t.dist
    px, py = _ptr(sx), _ptr(sy)
    for ev in FULL_REF_EVENTS[D]:
        rn, rd = xy.knn_table(x[px[ev]:px[ev + 1]].numpy(), [0, sx[ev]], y[py[ev]:py[ev + 1]].numpy(), [0, ny], k)
        assert np.array_equal(nbr[py[ev]:py[ev + 1]].cpu().numpy(), rn + px[ev]), ev
        assert np.array_equal(_bits(dist[py[ev]:py[ev + 1]]), _bits(rd)), ev
    # every event: full rows, ids inside the query's own x event, distances ascending (ties: ids ascending), and every
    # distance the fp32 chain of the returned pair, recomputed with torch on the GPU
    lo = torch.from_numpy(px[:-1]).to(dev)[by].view(-1, 1)
    hi = torch.from_numpy(px[1:]).to(dev)[by].view(-1, 1)
    assert bool(((nbr >= lo) & (nbr < hi)).all())
    assert bool((dist[:, 1:] >= dist[:, :-1]).all())
    assert bool(((dist[:, 1:] > dist[:, :-1]) | (nbr[:, 1:] > nbr[:, :-1])).all())
    acc = torch.zeros_like(dist)
    xj = xd[nbr.long()]                                             # [Ny, k, D]
    for c in range(D):
        acc = _fma32(xj[:, :, c] - yd[:, c].view(-1, 1), acc)
    assert np.array_equal(_bits(acc), _bits(dist))
    ei = dm.knn(xd, yd, k, bx, by)
    assert ei.shape == (2, B * ny * k) and int(ei.min()) >= 0


def test_tables_do_not_synchronise_on_registered_batches(dev):
    import deepmetv2_amd as dm
    sx, sy = [500, 0, 120, 64], [64, 10, 300, 0]
    x, y = _sets(2, 71, sx, sy)
    xd, yd, bx, by = x.to(dev), y.to(dev), _batch(sx, dev), _batch(sy, dev)
    dm.register_batch(bx, torch.from_numpy(_ptr(sx)).to(dev), 4, max_nodes=500, min_nodes=0)
    dm.register_batch(by, torch.from_numpy(_ptr(sy)).to(dev), 4, max_nodes=300, min_nodes=0)
    dm.knn_xy_table(xd, yd, 8, bx, by)                             # warm-up (library load, allocator)
    dm.radius_xy_table(xd, yd, 0.4, bx, by, 16)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        t = dm.knn_xy_table(xd, yd, 8, bx, by)
        tp = dm.knn_xy_table(xd, yd, 8, bx, by, period=[None, TWO_PI])
        r = dm.radius_xy_table(xd, yd, 0.4, bx, by, 16, period=[None, TWO_PI])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    ref = xy.knn_table(x.numpy(), _ptr(sx), y.numpy(), _ptr(sy), 8)[0]
    assert np.array_equal(t.nbr.cpu().numpy(), ref) and tp.nbr.shape == ref.shape and r.cnt.shape == (374,)

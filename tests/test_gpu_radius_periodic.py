"""radius_graph(..., period=) on the GPU: periodic coordinates (phi wraps at +-pi, train.py:47-48).

1. the kernels against the exact numpy restatement (tests/radius_periodic_reference.py), bit for bit;
2. the windowed form against the all-pairs form;
3. a plain period (None / all zero) against today's radius_graph and the oracle;
4. the geometry against a float64 circular distance, and invariance under a rotation of phi;
5. the EdgeConv routes on a periodic graph;
6. the static-table training step: captured replay, no host sync."""
import functools
import math

import numpy as np
import pytest
import torch

import radius_periodic_reference as rp

pytestmark = pytest.mark.gpu

PI32 = float(np.float32(np.pi))           # what atan2 returns at the seam
TWO_PI = 2 * math.pi                       # rounded to fp32 by the package: 2 * PI32
SIZES = [0, 1, 3, 64, 65, 129, 1500]       # ragged; wavefronts straddle events


def _ptr(sizes):
    return torch.cat([torch.zeros(1, dtype=torch.int64), torch.tensor(sizes, dtype=torch.int64).cumsum(0)])


def _phi(n, g):
    """atan2 output: phi in [-PI32, PI32]."""
    return torch.atan2(torch.randn(n, generator=g), torch.randn(n, generator=g))


def _seam_specials(x, lo, col_eta, col_phi):
    """Nodes at exactly +-PI32, pairs at a = L/2 and a = L, a dense cluster across the seam, from node lo on."""
    x[lo + 0, col_phi] = PI32
    x[lo + 1, col_phi] = -PI32                                     # a = L: distance 0 across the seam
    x[lo + 2, col_phi] = 0.0
    x[lo + 3, col_phi] = PI32                                      # a = L/2 from node lo+2
    x[lo + 4, col_phi] = -1.0
    x[lo + 5, col_phi] = float(np.float32(-1.0 + PI32))            # a close to L/2
    for k in range(6):
        x[lo + k, col_eta] = 0.05 * k
    # dense cluster across the seam: > 255 nodes within r of each other, half of them on each side
    n = 300
    g = torch.Generator().manual_seed(lo)
    side = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    x[lo + 10:lo + 10 + n, col_phi] = side * (PI32 - 0.08 * torch.rand(n, generator=g))
    x[lo + 10:lo + 10 + n, col_eta] = 1.0 + 0.08 * torch.rand(n, generator=g)


def _layout(name):
    """(x [N, D] fp32, sizes, period, r)"""
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    sizes = list(SIZES)
    N = sum(sizes)
    eta = (torch.rand(N, generator=g) - 0.5) * 10
    big = sum(sizes[:-1])                                          # the 1500-node event starts here
    if name == "etaphi":
        x = torch.stack([eta, _phi(N, g)], 1)
        _seam_specials(x, big, 0, 1)
        x[big + 400, 0] = float("nan"); x[big + 401, 1] = float("nan")
        x[big + 402, 0] = float("inf"); x[big + 403, 1] = float("inf"); x[big + 404, 1] = float("-inf")
        return x, sizes, [None, TWO_PI], 0.4
    if name == "phieta":
        x = torch.stack([_phi(N, g), eta], 1)
        _seam_specials(x, big, 1, 0)
        x[big + 400, 1] = float("nan"); x[big + 401, 0] = float("nan")
        x[big + 402, 1] = float("inf"); x[big + 403, 0] = float("inf"); x[big + 404, 0] = float("-inf")
        return x, sizes, [TWO_PI, None], 0.4
    if name == "3d_two_periodic":
        x = torch.stack([eta, _phi(N, g), (torch.rand(N, generator=g) - 0.5) * 2.0], 1)
        _seam_specials(x, big, 0, 1)
        x[big + 10:big + 310, 2] = torch.where(torch.arange(300) % 2 == 0, 0.97, -0.97)   # wraps in both
        return x, sizes, [None, TWO_PI, 2.0], 0.4
    if name == "1d_periodic":
        x = _phi(N, g).view(-1, 1)
        x[big:big + 6, 0] = torch.tensor([PI32, -PI32, 0.0, PI32, -1.0, 2.0])
        return x, sizes, [TWO_PI], 0.01
    if name == "8d_one_periodic":
        x = torch.cat([eta.view(-1, 1), 0.1 * torch.randn(N, 4, generator=g), _phi(N, g).view(-1, 1),
                       0.1 * torch.randn(N, 2, generator=g)], 1)
        _seam_specials(x, big, 0, 5)
        x[big + 400, 7] = float("nan"); x[big + 401, 5] = float("inf")
        return x, sizes, [None, 0, 0, None, 0, TWO_PI, None, 0], 0.6
    if name == "lattice_ties":
        # L = 8 and a 0.25 lattice: wrapped distances hit r = 0.5 exactly (strict <: no edge)
        x = torch.stack([torch.round(eta) / 4, torch.round((torch.rand(N, generator=g) - 0.5) * 32) / 4], 1)
        x[big:big + 4] = torch.tensor([[0.0, 3.75], [0.0, -3.75], [0.0, 4.0], [0.0, -4.0]])
        return x, sizes, [None, 8.0], 0.5
    if name == "wide_r":
        # r >= L/2 on a short periodic coordinate
        x = torch.stack([eta * 0.1, (torch.rand(N, generator=g) - 0.5) * 1.0], 1)
        x[big:big + 3, 1] = torch.tensor([0.5, -0.5, 0.0])
        return x, sizes, [None, 1.0], 0.6
    raise KeyError(name)


LAYOUTS = ["etaphi", "phieta", "3d_two_periodic", "1d_periodic", "8d_one_periodic", "lattice_ties", "wide_r"]


@functools.lru_cache(maxsize=None)
def _ref_hits(name):
    x, sizes, period, r = _layout(name)
    per = [None if p is None else float(np.float32(p)) for p in period]
    return rp.radius_hits(x.numpy(), _ptr(sizes).numpy(), r, per)


def _expected_rows16(nbr, cnt, ptr, stride16):
    """Event-local uint16 rows as int16: ids in the first cnt slots, 0xFFFF up to the next multiple of 8."""
    N = nbr.shape[0]
    counts = (ptr[1:] - ptr[:-1]).long()
    lo = torch.repeat_interleave(ptr[:-1], counts).view(-1, 1)
    loc = torch.full((N, stride16), 0xFFFF, dtype=torch.long)
    loc[:, :nbr.shape[1]] = torch.where(nbr >= 0, nbr.long() - lo, torch.full_like(lo, 0xFFFF))
    loc = torch.where(loc >= 0x8000, loc - 0x10000, loc).to(torch.int16)
    written = torch.arange(stride16).view(1, -1) < ((cnt.long() + 7) // 8 * 8).view(-1, 1)
    return loc, written


# ---- 1. bits against the restatement ------------------------------------------------------------------------------
@pytest.mark.parametrize("loop,mx", [(True, 255), (False, 255), (True, 32), (False, 32), (True, 4), (False, 4)])
@pytest.mark.parametrize("name", LAYOUTS)
def test_bits_against_restatement(dev, monkeypatch, name, loop, mx):
    import deepmetv2_amd as dm
    from deepmetv2_amd import _native
    x, sizes, period, r = _layout(name)
    ptr = _ptr(sizes)
    m = mx if loop else mx + 1
    want_nbr, want_cnt = rp.cap(_ref_hits(name), m, skip_self=not loop)
    want_nbr, want_cnt = torch.from_numpy(want_nbr), torch.from_numpy(want_cnt)
    per = [0.0 if p is None else float(np.float32(p)) for p in period]
    if name in ("etaphi", "phieta") and mx < 255:                  # the cap bites, on wrapped hits too
        assert max(len(h) for h in _ref_hits(name)) > m and int(want_cnt.max()) in (m - 1, m)
    xd, pd = x.to(dev), ptr.to(dev)
    for form in ("windowed", "sweep"):
        monkeypatch.setattr(_native, "RADIUS_FORM", form)
        nbr, cnt, rows16 = _native.radius_periodic(xd, pd, r, m, per, skip_self=not loop, pad=True, local=True)
        assert torch.equal(cnt.cpu(), want_cnt), (name, form)
        assert torch.equal(nbr.cpu(), want_nbr), (name, form)
        windowed = form == "windowed" and per[0] == 0.0
        assert (rows16 is not None) == windowed
        if rows16 is not None:
            loc, written = _expected_rows16(want_nbr, want_cnt, ptr, rows16.shape[1])
            assert torch.equal(rows16.cpu()[written], loc[written]), (name, form)
        # the public entry: table and [2,E] view
        table = dm.radius_table(xd, r, _batch(sizes, dev), loop=loop, max_num_neighbors=mx, period=period)
        assert torch.equal(table.cnt.cpu(), want_cnt)
        ei = dm.radius_graph(xd, r, _batch(sizes, dev), loop=loop, max_num_neighbors=mx, period=period)
        assert torch.equal(ei.cpu(), _edge_index(want_nbr, want_cnt))


def _batch(sizes, dev):
    return torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes)).to(dev)


def _edge_index(nbr, cnt):
    """[2,E] source_to_target: row 0 = neighbour j, row 1 = centre i, rows in order, slots in order."""
    N, m = nbr.shape
    keep = torch.arange(m).view(1, -1) < cnt.view(-1, 1)
    src = nbr[keep].long()
    tgt = torch.arange(N).view(-1, 1).expand(N, m)[keep]
    return torch.stack([src, tgt])


def test_int32_rows_off_keeps_the_uint16_rows(dev):
    """The default of a registered batch: only the uint16 rows are written; expanded on demand they are the table."""
    import deepmetv2_amd as dm
    x, sizes, period, r = _layout("etaphi")
    want_nbr, want_cnt = rp.cap(_ref_hits("etaphi"), 255)
    table = dm.radius_table(x.to(dev), r, _batch(sizes, dev), loop=True, max_num_neighbors=255, period=period,
                            int32_rows=False)
    assert table.rows16 is not None
    assert torch.equal(table.cnt.cpu(), torch.from_numpy(want_cnt))
    assert torch.equal(table.edge_index().cpu(), _edge_index(torch.from_numpy(want_nbr), torch.from_numpy(want_cnt)))


# ---- 2. window against all pairs ----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["etaphi", "tiny_events", "dense_seam", "three_d", "nonfinite"])
def test_windowed_equals_all_pairs(dev, monkeypatch, case):
    from deepmetv2_amd import _native
    g = torch.Generator().manual_seed(31)
    r, mx = 0.4, 255
    if case == "tiny_events":
        sizes = [int(v) for v in torch.randint(0, 40, (300,), generator=g)]
    else:
        sizes = [700, 0, 3, 1500, 64, 65, 129]
    N = sum(sizes)
    x = torch.stack([(torch.rand(N, generator=g) - 0.5) * 6, _phi(N, g)], 1)
    period = [0.0, 2 * PI32]
    if case == "dense_seam":
        x[100:600, 0] = x[100, 0] + 0.05 * torch.randn(500, generator=g)
        x[100:600, 1] = torch.where(torch.rand(500, generator=g) < 0.5, -PI32, PI32) * (1 - 0.01 * torch.rand(500, generator=g))
        mx = 32
    elif case == "three_d":
        x = torch.cat([x, (torch.rand(N, 1, generator=g) - 0.5) * 2], 1).contiguous()
        period = [0.0, 2 * PI32, 2.0]
    elif case == "nonfinite":
        x[5, 0] = float("nan"); x[17, 1] = float("nan"); x[40, 0] = float("inf"); x[41, 1] = float("-inf")
    ptr = _ptr(sizes).to(dev)
    xd = x.to(dev)
    for skip_self in (False, True):
        for pad in (True, False):
            monkeypatch.setattr(_native, "RADIUS_FORM", "sweep")
            n0, c0 = _native.radius_periodic(xd, ptr, r, mx, period, skip_self=skip_self, pad=pad)
            monkeypatch.setattr(_native, "RADIUS_FORM", "windowed")
            n1, c1 = _native.radius_periodic(xd, ptr, r, mx, period, skip_self=skip_self, pad=pad)
            assert torch.equal(c0, c1), case
            if pad:
                assert torch.equal(n0, n1), case
            else:
                keep = torch.arange(mx, device=dev).view(1, -1) < c0.view(-1, 1)
                assert torch.equal(n0[keep], n1[keep]), case


# ---- 3. zero period -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("period", [None, [0, 0], [None, None], [0.0, None]])
def test_plain_period_is_todays_graph(dev, period):
    import deepmetv2_amd as dm
    from oracle import ref_ops
    g = torch.Generator().manual_seed(3)
    sizes = [300, 5, 1000]
    N = sum(sizes)
    etaphi = torch.stack([(torch.rand(N, generator=g) - 0.5) * 6, (torch.rand(N, generator=g) - 0.5) * 6.28], 1)
    batch = torch.repeat_interleave(torch.arange(3), torch.tensor(sizes))
    for loop, mx in [(True, 255), (False, 12), (True, 4)]:
        ref = ref_ops.radius_graph(etaphi, 0.4, batch, loop=loop, max_num_neighbors=mx)
        plain = dm.radius_graph(etaphi.to(dev), 0.4, batch.to(dev), loop=loop, max_num_neighbors=mx)
        got = dm.radius_graph(etaphi.to(dev), 0.4, batch.to(dev), loop=loop, max_num_neighbors=mx, period=period)
        assert torch.equal(got, plain)
        assert torch.equal(got.cpu(), ref)
        t0 = dm.radius_table(etaphi.to(dev), 0.4, batch.to(dev), loop=loop, max_num_neighbors=mx)
        t1 = dm.radius_table(etaphi.to(dev), 0.4, batch.to(dev), loop=loop, max_num_neighbors=mx, period=period)
        assert torch.equal(t0.cnt, t1.cnt) and torch.equal(t0.edge_index(), t1.edge_index())


def test_all_zero_period_abi_is_the_plain_entry(dev):
    """dmet_radius_(windowed_)periodic_f32 with an all-zero period: the tables of the plain entries."""
    import ctypes
    from deepmetv2_amd import _lib, _native
    g = torch.Generator().manual_seed(4)
    sizes = [700, 3, 129]
    x = torch.stack([(torch.rand(sum(sizes), generator=g) - 0.5) * 6, _phi(sum(sizes), g)], 1).to(dev)
    ptr = _ptr(sizes).to(dev)
    N, D, B, mx = x.shape[0], 2, len(sizes), 64
    L = _lib.load()
    per = (ctypes.c_float * 2)(0.0, 0.0)
    st = _native._stream(dev)
    for skip in (0, 1):
        out = [torch.empty((N, mx), dtype=torch.int32, device=dev) for _ in range(4)]
        cnt = [torch.empty((N,), dtype=torch.int32, device=dev) for _ in range(4)]
        ws = torch.empty((L.dmet_radius_workspace_bytes(N),), dtype=torch.uint8, device=dev)
        _lib.check(L.dmet_radius_f32(x.data_ptr(), ptr.data_ptr(), B, N, D, 0.4, mx, skip, out[0].data_ptr(),
                                     cnt[0].data_ptr(), st))
        _lib.check(L.dmet_radius_periodic_f32(x.data_ptr(), ptr.data_ptr(), B, N, D, 0.4, mx, skip, 1,
                                              ctypes.cast(per, ctypes.c_void_p), out[1].data_ptr(), cnt[1].data_ptr(), st))
        _lib.check(L.dmet_radius_windowed_f32(x.data_ptr(), ptr.data_ptr(), B, N, D, 0.4, mx, skip, 1, out[2].data_ptr(),
                                              cnt[2].data_ptr(), ws.data_ptr(), ws.numel(), st))
        _lib.check(L.dmet_radius_windowed_periodic_f32(x.data_ptr(), ptr.data_ptr(), B, N, D, 0.4, mx, skip, 1,
                                                       ctypes.cast(per, ctypes.c_void_p), out[3].data_ptr(),
                                                       cnt[3].data_ptr(), None, 0, ws.data_ptr(), ws.numel(), st))
        for k in range(1, 4):
            assert torch.equal(out[k], out[0]) and torch.equal(cnt[k], cnt[0]), (skip, k)


# ---- 4. geometry --------------------------------------------------------------------------------------------------
def _circular_edges(etaphi, sizes, r):
    """(set of (j, i) with float64 circular distance < r, set of near-tie pairs within 1e-6 relative of r^2)."""
    x = etaphi.double().numpy()
    ptr = _ptr(sizes).numpy()
    L = 2 * PI32
    edges, ties = set(), set()
    for b in range(len(sizes)):
        lo, hi = int(ptr[b]), int(ptr[b + 1])
        e = x[lo:hi]
        de = e[None, :, 0] - e[:, None, 0]
        dp = np.abs(e[None, :, 1] - e[:, None, 1])
        dp = np.minimum(dp, L - dp)
        d2 = de * de + dp * dp
        ii, jj = np.nonzero(d2 < r * r)
        edges.update(zip((jj + lo).tolist(), (ii + lo).tolist()))
        ii, jj = np.nonzero(np.abs(d2 - r * r) <= 1e-6 * r * r)
        ties.update(zip((jj + lo).tolist(), (ii + lo).tolist()))
    return edges, ties


def _edge_set(ei):
    return set(zip(ei[0].tolist(), ei[1].tolist()))


def test_geometry_against_circular_distance_and_rotation(dev):
    import deepmetv2_amd as dm
    g = torch.Generator().manual_seed(8)
    sizes = [1500, 700, 1200]
    N = sum(sizes)
    # phi on a 2^-22 grid: the rotation by PI32 = L/2 (one fp32 add or subtract, results below 4 in magnitude) is exact
    phi = torch.round(_phi(N, g).double() * 2 ** 22) / 2 ** 22
    etaphi = torch.stack([(torch.rand(N, generator=g) - 0.5) * 10, phi.float()], 1)
    batch = _batch(sizes, dev)
    rot = etaphi.clone()
    rot[:, 1] = torch.where(phi > 0, phi - PI32, phi + PI32).float()
    assert torch.equal(rot[:, 1].double(), torch.where(phi > 0, phi - PI32, phi + PI32))
    assert bool((rot[:, 1].abs() <= PI32).all())
    want, ties = _circular_edges(etaphi, sizes, 0.4)
    want_r, ties_r = _circular_edges(rot, sizes, 0.4)
    skip = ties | ties_r
    got = _edge_set(dm.radius_graph(etaphi.to(dev), 0.4, batch, loop=True, max_num_neighbors=255,
                                    period=[None, TWO_PI]).cpu())
    got_r = _edge_set(dm.radius_graph(rot.to(dev), 0.4, batch, loop=True, max_num_neighbors=255,
                                      period=[None, TWO_PI]).cpu())
    assert (got ^ want) <= skip
    assert (got_r ^ want_r) <= skip
    assert (got ^ got_r) <= skip                                     # rotating phi by pi changes no edge
    plain = _edge_set(dm.radius_graph(etaphi.to(dev), 0.4, batch, loop=True, max_num_neighbors=255).cpu())
    plain_r = _edge_set(dm.radius_graph(rot.to(dev), 0.4, batch, loop=True, max_num_neighbors=255).cpu())
    assert len(want - plain) > 100 and len((plain ^ plain_r) - skip) > 100   # the seamed graph cannot pass this
    assert plain <= got                                                        # the wrap only shortens distances


# ---- 5. consumers on a periodic graph -----------------------------------------------------------------------------
def _periodic_inputs(dev, sizes=(600, 300, 45), seed=9):
    g = torch.Generator().manual_seed(seed)
    N = sum(sizes)
    etaphi = torch.stack([(torch.rand(N, generator=g) - 0.5) * 3, _phi(N, g)], 1)
    etaphi[:40, 1] = torch.where(torch.arange(40) % 2 == 0, PI32, -PI32) * (1 - 0.01 * torch.rand(40, generator=g))
    return etaphi.to(dev), _batch(list(sizes), dev), g


@pytest.mark.parametrize("loop", [True, False])
@pytest.mark.parametrize("as_table", [True, False])
def test_edgeconv_linear_max(dev, loop, as_table):
    import deepmetv2_amd as dm
    from oracle import ref_ops
    etaphi, batch, g = _periodic_inputs(dev)
    N = etaphi.shape[0]
    emb = torch.randn(N, 32, generator=g)
    gup = torch.randn(N, 32, generator=g)
    lin = torch.nn.Sequential(torch.nn.Linear(64, 32))
    conv = dm.EdgeConv(nn=lin)
    table = dm.radius_table(etaphi, 0.4, batch, loop=loop, max_num_neighbors=255, period=[None, TWO_PI])
    ei = table.edge_index("source_to_target")
    plain = dm.radius_graph(etaphi, 0.4, batch, loop=loop, max_num_neighbors=255)
    assert ei.shape[1] > plain.shape[1]                      # the wrap adds edges
    graph = table if as_table else dm.radius_graph(etaphi, 0.4, batch, loop=loop, max_num_neighbors=255,
                                                   period=[None, TWO_PI])
    if not as_table:
        assert torch.equal(graph, ei)
    xr = emb.clone().requires_grad_(True)
    ref = ref_ops.edge_conv(xr, ei.cpu(), lin)
    ref.backward(gup)
    gw_ref, gb_ref, gx_ref = lin[0].weight.grad.clone(), lin[0].bias.grad.clone(), xr.grad.clone()
    lin.zero_grad()
    conv = conv.to(dev)
    xd = emb.to(dev).requires_grad_(True)
    out = conv(xd, graph)
    out.backward(gup.to(dev))
    tol = lambda t: dict(rtol=1e-4, atol=1e-5 * max(1.0, float(t.abs().max())))
    torch.testing.assert_close(out.detach().cpu(), ref.detach(), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(xd.grad.cpu(), gx_ref, **tol(gx_ref))
    torch.testing.assert_close(lin[0].weight.grad.cpu(), gw_ref, **tol(gw_ref))
    torch.testing.assert_close(lin[0].bias.grad.cpu(), gb_ref, **tol(gb_ref))


@pytest.mark.parametrize("aggr", ["add", "mean"])
@pytest.mark.parametrize("as_table", [True, False])
def test_edgeconv_linear_sum_route(dev, monkeypatch, aggr, as_table):
    import deepmetv2_amd as dm
    import test_gpu_edgeconv_linear_sum as lsum
    etaphi, batch, g = _periodic_inputs(dev, seed=10)
    x = torch.randn(etaphi.shape[0], 32, generator=g).to(dev)
    if as_table:
        table = dm.radius_table(etaphi, 0.4, batch, loop=True, max_num_neighbors=255, period=[None, TWO_PI])
        el = table.edge_list()
        graph, ei = table, torch.stack([el.src.long(), el.tgt.long()])
    else:
        graph = ei = dm.radius_graph(etaphi, 0.4, batch, loop=True, max_num_neighbors=255, period=[None, TWO_PI])
    lsum._parity(dev, lsum._lin(32, 64, seed=11), x, graph, ei, aggr, monkeypatch=monkeypatch, form="table")


@pytest.mark.parametrize("aggr", ["max", "add"])
def test_edge_mlp_f32_route(dev, monkeypatch, aggr):
    import deepmetv2_amd as dm
    import test_gpu_edge_mlp_f32 as m32
    etaphi, batch, g = _periodic_inputs(dev, sizes=(120, 60), seed=12)
    x = torch.randn(etaphi.shape[0], 16, generator=g).to(dev)
    ei = dm.radius_graph(etaphi, 0.4, batch, loop=True, max_num_neighbors=255, period=[None, TWO_PI])
    m32._check_route(dev, m32._mlp(16, 24, 16, bn="train", seed=13), x, ei, aggr, monkeypatch=monkeypatch)


# ---- 6. the static-table step -------------------------------------------------------------------------------------
@pytest.mark.parametrize("side_stream", [False, True])
def test_graphed_static_table_step_matches_eager(dev, side_stream):
    """The periodic table built inside the captured step (graph_fn; with build_async on a side stream): replay walks
    the eager step's parameter trajectory bit for bit."""
    import deepmetv2_amd as dm
    from deepmetv2_amd import synth
    from deepmetv2_amd.model import Net
    from deepmetv2_amd.parallel import FlatModule, GradSync, GraphedTrainStep, train_step
    sizes = [700, 90, 1300]
    x, y, batch, ptr = synth.make_events(sizes, seed=5, device=dev)
    dm.register_batch(batch, ptr, len(sizes), max_nodes=max(sizes))

    def radius(xx):
        etaphi = torch.stack([xx[:, 3], torch.atan2(xx[:, 1], xx[:, 0])], 1)
        return dm.radius_table(etaphi, r=0.4, batch=batch, loop=True, max_num_neighbors=255, period=[None, TWO_PI])

    finals = []
    for graphed in (False, True):
        torch.manual_seed(1)
        model = Net(8, 3, graph="static", k=16).to(dev).train()
        flat = FlatModule(model); sync = GradSync(flat)
        opt = torch.optim.AdamW([flat.flat_param], lr=1e-3, capturable=True)
        if graphed:
            p0 = flat.flat_param.detach().clone()
            bufs0 = [b.detach().clone() for b in model.buffers()]
            fn = (lambda xx: dm.build_async(lambda: radius(xx))) if side_stream else radius
            step = GraphedTrainStep(model, flat, sync, opt, x, y, batch, ptr, warmup=1, graph_fn=fn)
            with torch.no_grad():
                flat.flat_param.copy_(p0)
                for b, b0 in zip(model.buffers(), bufs0):
                    b.copy_(b0)
                for st in opt.state.values():
                    for name, v in st.items():
                        if torch.is_tensor(v):
                            v.zero_()
        for it in range(4):
            loss = step() if graphed else train_step(model, flat, sync, opt, x, y, batch, ptr, edge_index=radius(x))
        torch.cuda.synchronize()
        finals.append((flat.flat_param.detach().clone(), float(loss)))
    assert finals[0][1] == finals[1][1]
    assert torch.equal(finals[0][0], finals[1][0])


def test_periodic_table_on_registered_batch_needs_no_sync(dev):
    import deepmetv2_amd as dm
    from deepmetv2_amd import synth
    sizes = [500, 3, 900]
    x, _y, batch, ptr = synth.make_events(sizes, seed=6, device=dev)
    dm.register_batch(batch, ptr, len(sizes), max_nodes=max(sizes), min_nodes=min(sizes))
    etaphi = torch.stack([x[:, 3], torch.atan2(x[:, 1], x[:, 0])], 1)
    conv = dm.EdgeConv(nn=torch.nn.Sequential(torch.nn.Linear(64, 32))).to(dev)
    emb = torch.randn(x.shape[0], 32, device=dev)
    want = dm.radius_table(etaphi, r=0.4, batch=batch, loop=True, max_num_neighbors=255, period=[None, TWO_PI])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for period in ([None, TWO_PI], (0, 2 * math.pi)):
            table = dm.radius_table(etaphi, r=0.4, batch=batch, loop=True, max_num_neighbors=255, period=period)
            out = conv(emb, table)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.equal(table.cnt, want.cnt)
    assert torch.equal(out, conv(emb, want))

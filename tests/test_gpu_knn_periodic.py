"""knn_table / knn_graph / knn(..., period=) on the GPU: periodic coordinates (phi wraps at +-pi, train.py:47).

1. the kernel against the exact numpy restatement (tests/knn_periodic_reference.py), bit for bit: nbr, dist, nbr_local;
2. a plain period (None / all zero) against today's table and the oracle;
3. the geometry against a float64 circular-distance kNN, and invariance under a rotation of phi;
4. the EdgeConv routes over a periodic table, and the native route it takes;
5. captured replay of build + EdgeConv, and no host sync on a registered batch."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import knn_periodic_reference as kp

pytestmark = pytest.mark.gpu

PI32 = float(np.float32(np.pi))           # what atan2 returns at the seam
TWO_PI = 2 * math.pi                       # rounded to fp32 by the package: 2 * PI32
TWO_PI_F32 = float(np.float32(TWO_PI))
SIZES = [0, 1, 3, 64, 65, 129, 1500]       # ragged; wavefronts straddle events


def _ptr(sizes):
    return torch.cat([torch.zeros(1, dtype=torch.int64), torch.tensor(sizes, dtype=torch.int64).cumsum(0)])


def _batch(sizes, dev):
    return torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes)).to(dev)


def _phi(n, g):
    """atan2 output: phi in [-PI32, PI32]."""
    return torch.atan2(torch.randn(n, generator=g), torch.randn(n, generator=g))


def _seam_specials(x, lo, col_eta, col_phi):
    """+-PI32 twins, a = L/2 and next to it, a dense cluster straddling the seam, exact ties, from node lo on."""
    x[lo + 0, col_phi] = PI32
    x[lo + 1, col_phi] = -PI32                                     # a = L: distance 0 across the seam
    x[lo + 2, col_phi] = 0.0
    x[lo + 3, col_phi] = PI32                                      # a = L/2 from node lo+2
    x[lo + 4, col_phi] = -1.0
    x[lo + 5, col_phi] = float(np.float32(-1.0 + PI32))            # a next to L/2
    x[lo + 6, col_phi] = float(np.nextafter(np.float32(PI32 - 1.0), np.float32(0)))
    for k in range(7):
        x[lo + k, col_eta] = 0.05 * k
    n = 300                                                        # dense cluster across the seam
    g = torch.Generator().manual_seed(lo)
    side = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    x[lo + 10:lo + 10 + n, col_phi] = side * (PI32 - 0.08 * torch.rand(n, generator=g))
    x[lo + 10:lo + 10 + n, col_eta] = 1.0 + 0.08 * torch.rand(n, generator=g)
    x[lo + 320:lo + 330] = x[lo + 20]                              # exact ties: R2 decides
    x[lo + 330:lo + 340, col_phi] = -x[lo + 330:lo + 340, col_phi].abs().clamp(min=3.0)


def _nonfinite(x, lo, col_a, col_b):
    x[lo + 400, col_a] = float("nan"); x[lo + 401, col_b] = float("nan")
    x[lo + 402, col_a] = float("inf"); x[lo + 403, col_b] = float("inf"); x[lo + 404, col_b] = float("-inf")


@functools.lru_cache(maxsize=None)
def _layout(name):
    """(x [N, D] fp32, period)"""
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    N = sum(SIZES)
    eta = (torch.rand(N, generator=g) - 0.5) * 10
    big = sum(SIZES[:-1])                                          # the 1500-node event starts here
    if name == "etaphi":                                           # periodic coordinate last
        x = torch.stack([eta, _phi(N, g)], 1)
        _seam_specials(x, big, 0, 1)
        _nonfinite(x, big, 0, 1)
        return x, [None, TWO_PI]
    if name == "phieta":                                           # periodic coordinate first
        x = torch.stack([_phi(N, g), eta], 1)
        _seam_specials(x, big, 1, 0)
        _nonfinite(x, big, 1, 0)
        return x, [TWO_PI, None]
    if name == "1d":
        x = _phi(N, g).view(-1, 1)
        x[big:big + 7, 0] = torch.tensor([PI32, -PI32, 0.0, PI32, -1.0, 2.0, -PI32])
        return x, [TWO_PI]
    if name == "3d_both":                                          # first and last periodic
        x = torch.stack([_phi(N, g), eta, (torch.rand(N, generator=g) - 0.5) * 2.0], 1)
        _seam_specials(x, big, 1, 0)
        x[big + 10:big + 310, 2] = torch.where(torch.arange(300) % 2 == 0, 0.97, -0.97)   # wraps in both
        return x, [TWO_PI, None, 2.0]
    if name == "8d":                                               # D = 8, EXACT_D, periodic first and last
        x = torch.cat([_phi(N, g).view(-1, 1), 0.1 * torch.randn(N, 5, generator=g), eta.view(-1, 1),
                       _phi(N, g).view(-1, 1)], 1)
        _seam_specials(x, big, 6, 7)
        _seam_specials(x, big, 6, 0)
        x[big + 400, 3] = float("nan"); x[big + 401, 7] = float("inf")
        return x, [TWO_PI, 0, None, 0, 0, None, None, TWO_PI]
    if name == "lattice_ties":                                     # L = 8 on a 0.25 lattice: many exact ties
        x = torch.stack([torch.round(eta) / 4, torch.round((torch.rand(N, generator=g) - 0.5) * 32) / 4], 1)
        x[big:big + 4] = torch.tensor([[0.0, 3.75], [0.0, -3.75], [0.0, 4.0], [0.0, -4.0]])
        return x, [None, 8.0]
    raise KeyError(name)


LAYOUTS = ["etaphi", "phieta", "1d", "3d_both", "8d", "lattice_ties"]


@functools.lru_cache(maxsize=None)
def _ref(name, k):
    x, period = _layout(name)
    per = [0.0 if p is None else float(np.float32(p)) for p in period]
    return kp.knn_table(x.numpy(), _ptr(SIZES).numpy(), k, per)


# ---- 1. bits ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 8, 16, 20, 32, 64])
@pytest.mark.parametrize("name", LAYOUTS)
def test_native_bits_against_restatement(dev, name, k):
    from deepmetv2_amd import _native
    x, period = _layout(name)
    per = [0.0 if p is None else float(np.float32(p)) for p in period]
    nbr, dist, loc = _native.knn_periodic(x.to(dev), _ptr(SIZES).to(dev), k, per, want_local=True)
    want_nbr, want_dist, want_loc = _ref(name, k)
    assert np.array_equal(nbr.cpu().numpy(), want_nbr)
    assert np.array_equal(dist.cpu().numpy().view(np.int32), want_dist.view(np.int32))
    assert np.array_equal(loc.cpu().numpy().view(np.uint16), want_loc)
    nbr2, dist2, loc2 = _native.knn_periodic(x.to(dev), _ptr(SIZES).to(dev), k, per, want_local=False)
    assert loc2 is None and torch.equal(nbr2, nbr) and torch.equal(dist2, dist)


@pytest.mark.parametrize("loop", [True, False])
@pytest.mark.parametrize("k", [8, 16, 31])
@pytest.mark.parametrize("name", ["etaphi", "phieta", "3d_both"])
def test_table_and_graph_bits(dev, name, k, loop):
    import deepmetv2_amd as dm
    x, period = _layout(name)
    kk = k if loop else k + 1
    want_nbr, want_dist, want_loc = _ref(name, kk)
    if not loop:
        want_nbr = np.where(want_nbr == np.arange(x.shape[0])[:, None], -1, want_nbr)
    batch = _batch(SIZES, dev)
    table = dm.knn_table(x.to(dev), k, batch, loop=loop, period=period)
    assert np.array_equal(table.nbr.cpu().numpy(), want_nbr)
    assert np.array_equal(table.dist.cpu().numpy().view(np.int32), want_dist.view(np.int32))
    if loop and kk in (8, 16, 20, 32):
        assert np.array_equal(table.nbr_local.cpu().numpy().view(np.uint16), want_loc)
    else:
        assert table.nbr_local is None
    tgt = np.repeat(np.arange(x.shape[0]), kk)
    src = want_nbr.reshape(-1)
    keep = src >= 0
    want_ei = np.stack([src[keep], tgt[keep]]).astype(np.int64)
    ei = dm.knn_graph(x.to(dev), k, batch, loop=loop, period=period)
    assert np.array_equal(ei.cpu().numpy(), want_ei)
    ei_t = dm.knn_graph(x.to(dev), k, batch, loop=loop, flow="target_to_source", period=period)
    assert np.array_equal(ei_t.cpu().numpy(), want_ei[::-1])


def test_knn_self_query_form(dev):
    import deepmetv2_amd as dm
    x, period = _layout("etaphi")
    xd, batch = x.to(dev), _batch(SIZES, dev)
    want_nbr, _, _ = _ref("etaphi", 16)
    tgt = np.repeat(np.arange(x.shape[0]), 16)
    src = want_nbr.reshape(-1)
    keep = src >= 0
    got = dm.knn(xd, xd, 16, batch, batch, period=period)
    assert np.array_equal(got.cpu().numpy(), np.stack([tgt[keep], src[keep]]))


# ---- 2. plain periods --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("period", [None, [0, 0], [None, None], [0.0, None]])
@pytest.mark.parametrize("loop", [True, False])
def test_plain_period_is_todays_table(dev, period, loop):
    import deepmetv2_amd as dm
    from oracle import ref_ops
    x, _ = _layout("etaphi")
    xd, batch = x.to(dev), _batch(SIZES, dev)
    t0 = dm.knn_table(xd, 16, batch, loop=loop)
    t1 = dm.knn_table(xd, 16, batch, loop=loop, period=period)
    assert torch.equal(t0.nbr, t1.nbr) and torch.equal(t0.dist, t1.dist)
    assert (t0.nbr_local is None) == (t1.nbr_local is None)
    if t0.nbr_local is not None:
        assert torch.equal(t0.nbr_local, t1.nbr_local)
    kk = 16 if loop else 17
    nbr_ref, dist_ref = ref_ops.knn_table(x, _ptr(SIZES), kk)
    if not loop:
        nbr_ref = torch.where(nbr_ref == torch.arange(x.shape[0], dtype=torch.int32).view(-1, 1), -1, nbr_ref)
    assert torch.equal(t1.nbr.cpu(), nbr_ref)
    assert torch.equal(t1.dist.cpu(), dist_ref)
    assert torch.equal(dm.knn_graph(xd, 16, batch, loop=loop), dm.knn_graph(xd, 16, batch, loop=loop, period=period))


@pytest.mark.parametrize("D", [1, 2, 3, 8])
def test_all_zero_period_abi_is_the_plain_entry(dev, D):
    from deepmetv2_amd import _lib, _native
    g = torch.Generator().manual_seed(D)
    x = torch.randn(sum(SIZES), D, generator=g).to(dev)
    ptr = _ptr(SIZES).to(dev)
    nbr0, dist0, loc0 = _native.knn_local(x, ptr, 16)
    L = _lib.load()
    per = (ctypes.c_float * D)(*([0.0] * D))
    N, B = x.shape[0], len(SIZES)
    nbr = torch.empty_like(nbr0); dist = torch.empty_like(dist0); loc = torch.empty_like(loc0)
    ws = torch.empty(L.dmet_knn_workspace_bytes(N, B, D, 16), dtype=torch.uint8, device=dev)
    _lib.check(L.dmet_knn_periodic_f32(x.data_ptr(), ptr.data_ptr(), B, N, D, 16, ctypes.cast(per, ctypes.c_void_p),
                                       nbr.data_ptr(), dist.data_ptr(), loc.data_ptr(), ws.data_ptr(), ws.numel(),
                                       torch.cuda.current_stream(dev).cuda_stream), "dmet_knn_periodic_f32")
    torch.cuda.synchronize()
    assert torch.equal(nbr, nbr0) and torch.equal(dist, dist0) and torch.equal(loc, loc0)


# ---- 3. geometry -------------------------------------------------------------------------------------------------
def test_geometry_against_circular_distance_and_rotation(dev):
    import deepmetv2_amd as dm
    g = torch.Generator().manual_seed(21)
    sizes = [700, 250, 1200]
    N = sum(sizes)
    etaphi = torch.stack([(torch.rand(N, generator=g) - 0.5) * 5, _phi(N, g)], 1)
    batch = _batch(sizes, dev)
    k = 16
    nbr = dm.knn_table(etaphi.to(dev), k, batch, loop=True, period=[None, TWO_PI]).nbr.cpu().numpy()
    rot = etaphi.clone()
    rot[:, 1] = torch.remainder(rot[:, 1] + 2 * PI32, 2 * PI32) - PI32      # phi + pi, back into one period
    nbr_rot = dm.knn_table(rot.to(dev), k, batch, loop=True, period=[None, TWO_PI]).nbr.cpu().numpy()
    ptr = _ptr(sizes).numpy()
    checked = 0
    for b in range(len(sizes)):
        lo, hi = ptr[b], ptr[b + 1]
        d64 = kp.circular_d2_f64(etaphi[lo:hi].numpy(), [None, TWO_PI_F32])
        for i in range(hi - lo):
            srt = np.sort(d64[i])
            if srt[k] - srt[k - 1] < 1e-3 * max(srt[k], 1e-6):   # the k-th and (k+1)-th too close to call in fp32
                continue
            want = set((np.argsort(d64[i], kind="stable")[:k] + lo).tolist())
            assert set(nbr[lo + i].tolist()) == want
            assert set(nbr_rot[lo + i].tolist()) == want
            checked += 1
    assert checked > 0.9 * N
    seam = (etaphi[:, 1].abs() > PI32 - 0.4).numpy()
    plain = dm.knn_table(etaphi.to(dev), k, batch, loop=True).nbr.cpu().numpy()
    assert (plain[seam] != nbr[seam]).any(axis=1).mean() > 0.3        # the wrap changes rows near the seam


# ---- 4. EdgeConv over a periodic table ---------------------------------------------------------------------------
def _periodic_inputs(dev, sizes=(600, 300, 45), seed=9):
    g = torch.Generator().manual_seed(seed)
    N = sum(sizes)
    etaphi = torch.stack([(torch.rand(N, generator=g) - 0.5) * 3, _phi(N, g)], 1)
    etaphi[:40, 1] = torch.where(torch.arange(40) % 2 == 0, PI32, -PI32) * (1 - 0.01 * torch.rand(40, generator=g))
    return etaphi.to(dev), _batch(list(sizes), dev), g


@pytest.mark.parametrize("k", [16, 5])
@pytest.mark.parametrize("loop", [True, False])
def test_edgeconv_linear_max(dev, k, loop):
    import deepmetv2_amd as dm
    from oracle import ref_ops
    etaphi, batch, g = _periodic_inputs(dev)
    N = etaphi.shape[0]
    emb = torch.randn(N, 32, generator=g)
    gup = torch.randn(N, 32, generator=g)
    lin = torch.nn.Sequential(torch.nn.Linear(64, 32))
    conv = dm.EdgeConv(nn=lin).to(dev)
    table = dm.knn_table(etaphi, k, batch, loop=loop, period=[None, TWO_PI])
    ei = table.edge_index("source_to_target")
    assert not torch.equal(ei, dm.knn_graph(etaphi, k, batch, loop=loop))        # the wrap changes the graph
    lin_ref = torch.nn.Sequential(torch.nn.Linear(64, 32))
    lin_ref.load_state_dict(lin.state_dict())
    xr = emb.clone().requires_grad_(True)
    ref = ref_ops.edge_conv(xr, ei.cpu(), lin_ref)
    ref.backward(gup)
    for graph in (table, ei):                                      # the fused route and the generic edge_index route
        conv.zero_grad()
        xd = emb.to(dev).requires_grad_(True)
        out = conv(xd, graph)
        out.backward(gup.to(dev))
        tol = lambda t: dict(rtol=1e-4, atol=1e-5 * max(1.0, float(t.abs().max())))     # noqa: E731
        torch.testing.assert_close(out.detach().cpu(), ref.detach(), rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(xd.grad.cpu(), xr.grad, **tol(xr.grad))
        torch.testing.assert_close(lin[0].weight.grad.cpu(), lin_ref[0].weight.grad, **tol(lin_ref[0].weight.grad))
        torch.testing.assert_close(lin[0].bias.grad.cpu(), lin_ref[0].bias.grad, **tol(lin_ref[0].bias.grad))


@pytest.mark.parametrize("aggr", ["add", "mean"])
@pytest.mark.parametrize("as_table", [True, False])
def test_edgeconv_linear_sum_route(dev, monkeypatch, aggr, as_table):
    import deepmetv2_amd as dm
    import test_gpu_edgeconv_linear_sum as lsum
    etaphi, batch, g = _periodic_inputs(dev, seed=10)
    x = torch.randn(etaphi.shape[0], 32, generator=g).to(dev)
    if as_table:
        table = dm.knn_table(etaphi, 16, batch, loop=True, period=[None, TWO_PI])
        el = table.edge_list()
        graph, ei = table, torch.stack([el.src.long(), el.tgt.long()])
    else:
        graph = ei = dm.knn_graph(etaphi, 16, batch, loop=True, period=[None, TWO_PI])
    lsum._parity(dev, lsum._lin(32, 64, seed=11), x, graph, ei, aggr, monkeypatch=monkeypatch, form="table")


@pytest.mark.parametrize("aggr", ["max", "add"])
def test_edge_mlp_f32_route(dev, monkeypatch, aggr):
    import deepmetv2_amd as dm
    import test_gpu_edge_mlp_f32 as m32
    etaphi, batch, g = _periodic_inputs(dev, sizes=(120, 60), seed=12)
    x = torch.randn(etaphi.shape[0], 16, generator=g).to(dev)
    ei = dm.knn_graph(etaphi, 16, batch, loop=True, period=[None, TWO_PI])
    m32._check_route(dev, m32._mlp(16, 24, 16, bn="train", seed=13), x, ei, aggr, monkeypatch=monkeypatch)


class _EntrySpy:
    """Stands in for the loaded library and records which C entries are looked up."""

    def __init__(self, lib):
        self._lib, self.names = lib, []

    def __getattr__(self, name):
        if name.startswith("dmet_"):
            self.names.append(name)
        return getattr(self._lib, name)


@pytest.mark.parametrize("k", [16, 8, 32, 12])
def test_periodic_table_takes_the_plain_tables_route(dev, monkeypatch, k):
    """A periodic table feeds Linear(64, 32) max EdgeConv through the same C entries as a plain kNN table of the same
    k: the LDS-resident gather on the event-local ids for k in (8, 16, 20, 32)."""
    import deepmetv2_amd as dm
    from deepmetv2_amd import _lib
    etaphi, batch, g = _periodic_inputs(dev, seed=14)
    emb = torch.randn(etaphi.shape[0], 32, generator=g).to(dev).requires_grad_(True)
    conv = dm.EdgeConv(nn=torch.nn.Sequential(torch.nn.Linear(64, 32))).to(dev)
    tables = {"plain": dm.knn_table(etaphi, k, batch, loop=True),
              "periodic": dm.knn_table(etaphi, k, batch, loop=True, period=[None, TWO_PI])}
    real = _lib.load()
    routes = {}
    for name, table in tables.items():
        spy = _EntrySpy(real)
        monkeypatch.setattr(_lib, "load", lambda: spy)
        out = conv(emb, table)
        out.sum().backward()
        torch.cuda.synchronize()
        monkeypatch.setattr(_lib, "load", lambda: real)
        routes[name] = spy.names
    assert routes["periodic"] == routes["plain"]
    lds = [n for n in routes["periodic"] if "lds" in n]
    assert bool(lds) == (k in (8, 16, 20, 32)), routes["periodic"]


# ---- 5. captured replay, host syncs -------------------------------------------------------------------------------
def test_captured_build_and_edgeconv_replays_new_inputs(dev):
    import deepmetv2_amd as dm
    sizes = [700, 90, 1300]
    N = sum(sizes)
    batch = _batch(sizes, dev)
    ptr = _ptr(sizes).to(dev)
    dm.register_batch(batch, ptr, len(sizes), max_nodes=max(sizes), min_nodes=min(sizes))
    conv = dm.EdgeConv(nn=torch.nn.Sequential(torch.nn.Linear(64, 32))).to(dev)
    g = torch.Generator().manual_seed(15)

    def inputs():
        return (torch.stack([(torch.rand(N, generator=g) - 0.5) * 5, _phi(N, g)], 1).to(dev),
                torch.randn(N, 32, generator=g).to(dev))

    def fwd(etaphi, emb):
        table = dm.knn_table(etaphi, 16, batch, loop=True, period=[None, TWO_PI])
        return conv(emb, table), table.nbr

    s_etaphi, s_emb = inputs()
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side), torch.no_grad():
        for _ in range(2):
            fwd(s_etaphi, s_emb)
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):
        s_out, s_nbr = fwd(s_etaphi, s_emb)
    for _ in range(3):
        etaphi, emb = inputs()
        s_etaphi.copy_(etaphi); s_emb.copy_(emb)
        graph.replay()
        with torch.no_grad():
            want_out, want_nbr = fwd(etaphi, emb)
        torch.cuda.synchronize()
        assert torch.equal(s_nbr, want_nbr)
        assert torch.equal(s_out, want_out)


def test_periodic_table_on_registered_batch_needs_no_sync(dev):
    import deepmetv2_amd as dm
    from deepmetv2_amd import synth
    sizes = [500, 30, 900]
    x, _y, batch, ptr = synth.make_events(sizes, seed=6, device=dev)
    dm.register_batch(batch, ptr, len(sizes), max_nodes=max(sizes), min_nodes=min(sizes))
    etaphi = torch.stack([x[:, 3], torch.atan2(x[:, 1], x[:, 0])], 1)
    conv = dm.EdgeConv(nn=torch.nn.Sequential(torch.nn.Linear(64, 32))).to(dev)
    emb = torch.randn(x.shape[0], 32, device=dev)
    want = dm.knn_table(etaphi, 16, batch, loop=True, period=[None, TWO_PI])
    want_out = conv(emb, want)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for period in ([None, TWO_PI], (0, 2 * math.pi)):
            table = dm.knn_table(etaphi, 16, batch, loop=True, period=period)
            out = conv(emb, table)
            ei = dm.knn_graph(etaphi, 16, batch, loop=True, period=period)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.equal(table.nbr, want.nbr)
    assert torch.equal(out, want_out)
    assert ei.shape[1] == x.shape[0] * 16
